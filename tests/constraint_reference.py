"""CPU reference of grammar-constrained decoding, in float64.

The plank grammar: at step t = 6 k + c the written token of a free row must lie in ``window(t, prev, ...)``, prev being the row's own
token at t - 3.  A vocab candidate k writes token k, a pointer candidate j < t writes the row's token at j and is judged by it, a
pointer j >= t is never allowed.  The constraint only removes candidates from the selection: the p of the others, and with them every
score, stay what the unconstrained references compute.

``ConstrainedStepper`` is ``beam_reference._Stepper`` plus the rows' token history (written in ``feed``, permuted in ``reorder``) and a
``dist()`` that zeroes the p of disallowed candidates.  The beam, sampling and prefix references drop p = 0 candidates already, so
installing the subclass (``constrained(...)``, a context manager that restores the modules' ``_Stepper``) makes ``BR.beam_search``,
``SR.sample_decode`` and ``PR.beam_search`` / ``PR.sample_decode`` constrained as they stand.  Greedy has its own loop here: its arg-max
runs over the allowed candidates (one with p = 0 still beats a disallowed one, so zeroing is not enough) and its near-tie flag is taken
among allowed candidates only.  The subclass knows nothing of forced positions (which are not filtered): use it with prefixes whose
forced candidates the grammar allows, or with none.
"""
from __future__ import annotations

import contextlib

import torch

import beam_reference as BR
import prefix_reference as PR
import sample_reference as SR

DOF = 6


def default_max_planks(steps):
    """The last plank boundary that still leaves room for END."""
    return (steps - 1) // DOF


def resolve(steps, min_planks=1, max_planks=None):
    """(min_planks, max_planks) as the step uses them: a caller's max_planks clamped to the default."""
    top = default_max_planks(steps)
    return min_planks, top if max_planks is None else min(max_planks, top)


def window(t, prev, n_val, min_planks, max_planks):
    """(lo, hi, end_ok): tokens lo .. hi are allowed (lo > hi: none), plus END when end_ok.  ``prev`` = the row's token at t - 3 (read
    for t % 6 >= 3 only)."""
    c, k = t % DOF, t // DOF
    if c == 0:
        if k >= max_planks:
            return 1, 0, True
        return 0, n_val - 2, k >= min_planks
    if c < 3:
        return 0, n_val - 2, False
    return min(int(prev), n_val - 2) + 1, n_val - 1, False


def allowed_mask(t, history, V, end, n_val, min_planks, max_planks, width):
    """bool [rows, width] over the candidate indices of last_row_dist (vocab k at k, pointer j at V + j)."""
    rows = history.shape[0]
    mask = torch.zeros(rows, width, dtype=torch.bool)
    for r in range(rows):
        lo, hi, end_ok = window(t, history[r, t - 3] if t % DOF >= 3 else 0, n_val, min_planks, max_planks)
        tok_ok = torch.zeros(V, dtype=torch.bool)
        if lo <= hi:
            tok_ok[lo:hi + 1] = True
        tok_ok[end] = end_ok
        mask[r, :V] = tok_ok
        n_ptr = min(width - V, t)                                    # pointers j < t only
        if n_ptr > 0:
            mask[r, V:V + n_ptr] = tok_ok[history[r, :n_ptr]]
    return mask


def make_stepper(min_planks=1, max_planks=None):
    class ConstrainedStepper(BR._Stepper):
        def __init__(self, p, cfg, batch, K, steps):
            super().__init__(p, cfg, batch, K, steps)
            self.steps = steps
            self.history = torch.zeros(self.rows, steps, dtype=torch.long)
            self.n_val = min(cfg.end, cfg.pad)
            self.min_planks, self.max_planks = resolve(steps, min_planks, max_planks)

        def allowed(self, t, width):
            return allowed_mask(t, self.history, self.cfg.vocab, self.cfg.end, self.n_val, self.min_planks, self.max_planks, width)

        def raw_dist(self, t):
            return super().dist(t)

        def dist(self, t):
            d = super().dist(t)
            return torch.where(self.allowed(t, d.shape[1]), d, torch.zeros_like(d))

        def reorder(self, idx):
            super().reorder(idx)
            self.history = self.history[idx]

        def feed(self, tok, t):
            super().feed(tok, t)
            self.history[:, t] = tok

    return ConstrainedStepper


@contextlib.contextmanager
def constrained(min_planks=1, max_planks=None):
    """Inside: BR / SR / PR build constrained steppers.  The modules' own ``_Stepper`` is restored on the way out."""
    mods = (BR, SR, PR)
    saved = [m._Stepper for m in mods]
    cls = make_stepper(min_planks, max_planks)
    try:
        for m in mods:
            m._Stepper = cls
        yield cls
    finally:
        for m, s in zip(mods, saved):
            m._Stepper = s


def greedy(sd, cfg, batch, constraint=None, max_steps=None, dtype=torch.float64, tie_tol=1e-5):
    """Greedy decode of every step (no early stop).  ``constraint``: None (free: prefix_reference.greedy's selection) or a dict of
    ``min_planks`` / ``max_planks``.  Returns ``tokens`` / ``attach`` [B, steps], ``first_end`` [B] and ``near_tie`` bool [B, steps]:
    the two largest p among the candidates the arg-max ran over are within ``tie_tol`` relative."""
    if constraint is None:
        r = PR.greedy(sd, cfg, batch, None, max_steps=max_steps, dtype=dtype, tie_tol=tie_tol)
        return {k: r[k] for k in ("tokens", "attach", "first_end", "near_tie")}
    p = BR._params(sd, dtype)
    steps = int(max_steps or cfg.max_output_length)
    B = batch["input_value"].shape[0]
    st = make_stepper(**constraint)(p, cfg, batch, 1, steps)
    V, END = cfg.vocab, cfg.end
    tokens = torch.zeros(B, steps, dtype=torch.long)
    attach = torch.full((B, steps), -1, dtype=torch.long)
    fe = torch.full((B,), -1, dtype=torch.long)
    near = torch.zeros(B, steps, dtype=torch.bool)
    for t in range(steps):
        dist = st.raw_dist(t)
        ok = st.allowed(t, dist.shape[1])
        for r in range(B):
            cand = ok[r].nonzero()[:, 0]                              # index order: the first maximum is the smallest index
            pv = dist[r, cand]
            idx = int(cand[int(torch.sort(-pv, stable=True).indices[0])])
            if len(cand) > 1:
                top = torch.topk(pv, 2).values
                near[r, t] = float(top[0] - top[1]) <= tie_tol * float(top[0])
            tok, att = (int(tokens[r, idx - V]), idx - V) if idx >= V else (idx, -1)
            tokens[r, t], attach[r, t] = tok, att
            if tok == END and fe[r] < 0:
                fe[r] = t
        st.feed(tokens[:, t], t)
    return {"tokens": tokens, "attach": attach, "first_end": fe, "near_tie": near}
