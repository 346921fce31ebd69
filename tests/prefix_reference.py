"""CPU reference of forced-prefix decoding and sequence scoring, in float64.

Built from ``beam_reference._Stepper`` and the oracle's public functions; the selection rules of the free steps are those of
tests/beam_reference.py (beam) and tests/sample_reference.py (``select`` / ``sample_u``), restated here only as far as the loops
need them.  A prefix is given per hypothesis ROW as ``(plen [R], ptok [R, P], patt [R, P])``: at step t a row with t < plen[r] takes
the candidate ptok (patt = -1) or the pointer patt (index V + patt) without arg-max, ranking or draw:
  * lp = log p of that candidate under ``last_row_dist``; a candidate that does not exist at its step (a pointer with patt >= t or
    while t + 1 < 6, an index outside the table) has lp = -inf;
  * token / attach written: ptok / -1, or for a pointer the row's own token at patt / patt;
  * greedy: nothing is frozen - forced positions after END are still forced and their lp recorded, but the prefix score stops after
    the row's first END (END's own lp included), as ``beam_reference.teacher_forced_logprob`` sums;
  * beam: a finished row is frozen as without a prefix; a forced live row has the single candidate (lp, token, attach), so beam 0
    carries the hypothesis through the prefix and the first free step fans out; the lp also joins the beam score;
  * sampling: a row frozen by END ignores the rest of its prefix; u is not consumed by a forced step (it is a function of
    (seed, b, n, t) anyway); the lp joins the sample's score.
Every function returns per-row ``prefix_lp`` [R, steps] (0 where nothing was forced) and ``prefix_score`` [R], and the near-tie /
near-boundary flags of its FREE steps.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import sample_reference as SR
from beam_reference import _Stepper, _params


def no_prefix(R):
    return torch.zeros(R, dtype=torch.long), torch.zeros(R, 0, dtype=torch.long), torch.zeros(R, 0, dtype=torch.long)


def forced(dist, tokens, r, t, V, ptok, patt):
    """(lp, token, attach) of the forced candidate of row r at step t; dist: last_row_dist [R, V (+ t + 1)]."""
    tok, att = int(ptok[r, t]), int(patt[r, t])
    if att < 0:
        if not 0 <= tok < V:
            return float("-inf"), tok, -1
        pv = float(dist[r, tok])
        return (math.log(pv) if pv > 0 else float("-inf")), tok, -1
    if att >= t or t + 1 < 6:
        return float("-inf"), tok, -1
    pv = float(dist[r, V + att])
    return (math.log(pv) if pv > 0 else float("-inf")), int(tokens[r, att]), att


def greedy(sd, cfg, batch, prefix=None, max_steps=None, dtype=torch.float64, tie_tol=1e-5):
    """Greedy decode of every step (no early stop) with forced positions.  Returns ``tokens`` / ``attach`` [B, steps],
    ``prefix_lp`` [B, steps], ``prefix_score`` [B], ``first_end`` [B] and ``near_tie`` bool [B, steps] (free steps whose two largest
    p are within ``tie_tol`` relative)."""
    p = _params(sd, dtype)
    steps = int(max_steps or cfg.max_output_length)
    B = batch["input_value"].shape[0]
    plen, ptok, patt = prefix if prefix is not None else no_prefix(B)
    st = _Stepper(p, cfg, batch, 1, steps)
    V, END = cfg.vocab, cfg.end
    tokens = torch.zeros(B, steps, dtype=torch.long)
    attach = torch.full((B, steps), -1, dtype=torch.long)
    lp = torch.zeros(B, steps, dtype=torch.float64)
    score = torch.zeros(B, dtype=torch.float64)
    fe = torch.full((B,), -1, dtype=torch.long)
    near = torch.zeros(B, steps, dtype=torch.bool)
    for t in range(steps):
        dist = st.dist(t)
        for r in range(B):
            if t < int(plen[r]):
                l, tok, att = forced(dist, tokens, r, t, V, ptok, patt)
                lp[r, t] = l
                if fe[r] < 0:
                    score[r] += l
            else:
                top = torch.topk(dist[r], 2)
                idx = int(torch.sort(-dist[r], stable=True).indices[0])          # first maximum
                a, b = float(top.values[0]), float(top.values[1])
                near[r, t] = (a - b) <= tie_tol * a
                tok, att = (int(tokens[r, idx - V]), idx - V) if idx >= V else (idx, -1)
            tokens[r, t], attach[r, t] = tok, att
            if tok == END and fe[r] < 0:
                fe[r] = t
        st.feed(tokens[:, t], t)
    return {"tokens": tokens, "attach": attach, "prefix_lp": lp, "prefix_score": score, "first_end": fe, "near_tie": near}


def score(sd, cfg, batch, tokens, attach=None, lengths=None, dtype=torch.float64):
    """The scorer: greedy with every position forced for max(lengths) steps.  Returns (scores [B], logprobs [B, n])."""
    B, P = tokens.shape
    attach = torch.full_like(tokens, -1) if attach is None else attach
    if lengths is None:
        lengths = torch.tensor([default_length(tokens[r], cfg) for r in range(B)])
    n = int(lengths.max())
    r = greedy(sd, cfg, batch, (lengths, tokens, attach), max_steps=n, dtype=dtype)
    return r["prefix_score"], r["prefix_lp"]


def default_length(row, cfg):
    """Up to and including the first END, else up to the first PAD, else all."""
    for i, v in enumerate(row.tolist()):
        if v == cfg.end:
            return i + 1
        if v == cfg.pad:
            return i
    return len(row)


def beam_search(sd, cfg, batch, K, prefix=None, max_steps=None, early_stop=True, length_penalty=0.0, dtype=torch.float64,
                tie_tol=1e-5):
    """beam_reference.beam_search with forced positions; ``prefix`` per ROW (every row of a drawing the same).  The same result dict
    plus ``prefix_lp`` [B, K, n] / ``prefix_score`` [B, K] (those of the drawing's row b*K, which carries the hypothesis)."""
    p = _params(sd, dtype)
    steps = int(max_steps or cfg.max_output_length)
    B = batch["input_value"].shape[0]
    R = B * K
    plen, ptok, patt = prefix if prefix is not None else no_prefix(R)
    st = _Stepper(p, cfg, batch, K, steps)
    V, PAD, END = cfg.vocab, cfg.pad, cfg.end
    tokens = torch.zeros(R, steps, dtype=torch.long)
    attach = torch.full((R, steps), -1, dtype=torch.long)
    score = torch.full((R,), float("-inf"), dtype=dtype)
    score[::K] = 0.0
    fin = torch.zeros(R, dtype=torch.bool)
    fe = torch.full((R,), -1, dtype=torch.long)
    plp = torch.zeros(R, steps, dtype=torch.float64)
    psc = torch.zeros(R, dtype=torch.float64)
    ties = []
    done = 0
    for t in range(steps):
        dist = st.dist(t)
        if dist.shape[1] > V:
            dist = dist[:, :V + t]                                   # the self pointer j = t is no candidate
        tie = torch.zeros(B, dtype=torch.bool)
        cands = []
        for r in range(R):
            if bool(fin[r]):
                cands.append([(0.0, PAD, -1)])
                continue
            if t < int(plen[r]):
                l, tok, att = forced(dist, tokens, r, t, V, ptok, patt)
                plp[r, t] = l
                psc[r] += l
                cands.append([(l, tok, att)] + [(float("-inf"), PAD, -1)] * (K - 1))
                continue
            pr = dist[r]
            order = torch.sort(-pr, stable=True).indices
            top = order[:K + 1]
            lst = []
            for idx in top[:K].tolist():
                pv = float(pr[idx])
                if pv <= 0.0:
                    break
                lst.append((math.log(pv), int(tokens[r, idx - V]), idx - V) if idx >= V else (math.log(pv), idx, -1))
            cands.append(lst)
            if len(top) > K and math.isfinite(float(score[r])):
                a, b = float(pr[top[K - 1]]), float(pr[top[K]])
                if a > 0 and (a - b) <= tie_tol * a:
                    tie[r // K] = True
        parent = torch.empty(R, dtype=torch.long)
        new = []
        for b in range(B):
            pool = []
            for k in range(K):
                r = b * K + k
                for rank, (l, tok, att) in enumerate(cands[r]):
                    pool.append((float(score[r]) + l, k, rank, tok, att))
            pool.sort(key=lambda c: (-c[0], c[1], c[2]))
            while len(pool) < K:                                     # (fewer than K candidates in the drawing: no beam)
                pool.append((float("-inf"), 0, K, PAD, -1))
            if len(pool) > K and math.isfinite(pool[K - 1][0]) and pool[K - 1][0] - pool[K][0] <= tie_tol:
                tie[b] = True
            for k in range(K):
                s, kp, _, tok, att = pool[k]
                parent[b * K + k] = b * K + kp
                new.append((s, tok, att))
        ties.append(tie)
        tokens, attach = tokens[parent], attach[parent]
        fin, fe = fin[parent], fe[parent]
        st.reorder(parent)
        for r, (s, tok, att) in enumerate(new):
            score[r] = s
            tokens[r, t] = tok
            attach[r, t] = att
            if not bool(fin[r]) and tok == END:
                fin[r] = True
                fe[r] = t
        st.feed(tokens[:, t], t)
        done = t + 1
        if early_stop and bool(fin.all()):
            break
    n = int(fe.max()) + 1 if bool(fin.all()) else steps
    sc = score.view(B, K)
    lengths = torch.where(fe >= 0, fe + 1, torch.full_like(fe, steps)).view(B, K)
    key = sc / lengths.to(dtype) ** length_penalty if length_penalty != 0.0 else sc
    order = torch.sort(-key, dim=1, stable=True).indices
    bt = tokens.view(B, K, steps)[:, :, :n].gather(1, order[:, :, None].expand(B, K, n))
    ba = attach.view(B, K, steps)[:, :, :n].gather(1, order[:, :, None].expand(B, K, n))
    return {"tokens": bt[:, 0], "attach": ba[:, 0], "beam_tokens": bt, "beam_attach": ba, "scores": sc.gather(1, order),
            "finished": fin.view(B, K).gather(1, order), "lengths": lengths.gather(1, order),
            "near_tie": torch.stack(ties, dim=1), "steps": done,
            "prefix_lp": plp.view(B, K, steps)[:, :1, :n].expand(B, K, n), "prefix_score": psc.view(B, K)[:, :1].expand(B, K)}


def sample_decode(sd, cfg, batch, N, prefix=None, seed=0, temperature=1.0, top_k=0, top_p=1.0, max_steps=None, early_stop=True,
                  dtype=torch.float64, tol=1e-4):
    """sample_reference.sample_decode with forced positions; ``prefix`` per ROW.  The same per-row result dict plus ``prefix_lp``
    [R, steps] / ``prefix_score`` [R]."""
    temperature = float(np.float32(temperature))
    top_p = float(np.float32(top_p))
    p = _params(sd, dtype)
    steps = int(max_steps or cfg.max_output_length)
    B = batch["input_value"].shape[0]
    R = B * N
    plen, ptok, patt = prefix if prefix is not None else no_prefix(R)
    st = _Stepper(p, cfg, batch, N, steps)
    V, PAD, END = cfg.vocab, cfg.pad, cfg.end
    tokens = torch.zeros(R, steps, dtype=torch.long)
    attach = torch.full((R, steps), -1, dtype=torch.long)
    score = np.zeros(R, dtype=np.float64)
    fe = np.full(R, -1, dtype=np.int64)
    near = np.zeros((R, steps), dtype=bool)
    plp = torch.zeros(R, steps, dtype=torch.float64)
    psc = torch.zeros(R, dtype=torch.float64)
    rb, rn = np.arange(R) // N, np.arange(R) % N
    done = 0
    for t in range(steps):
        dist = st.dist(t)
        if dist.shape[1] > V:
            dist = dist[:, :V + t]
        u = SR.sample_u(seed, rb, rn, t)
        dn = dist.numpy()
        for r in range(R):
            if fe[r] >= 0:
                tokens[r, t], attach[r, t] = PAD, -1
                continue
            if t < int(plen[r]):
                l, tok, att = forced(dist, tokens, r, t, V, ptok, patt)
                tokens[r, t], attach[r, t] = tok, att
                plp[r, t] = l
                psc[r] += l
                score[r] += l
            else:
                idx, nr = SR.select(dn[r], float(u[r]), temperature, top_k, top_p, tol)
                near[r, t] = nr
                if idx >= V:
                    tokens[r, t], attach[r, t] = tokens[r, idx - V], idx - V
                else:
                    tokens[r, t] = idx
                score[r] += math.log(dn[r, idx])
            if int(tokens[r, t]) == END:
                fe[r] = t
        st.feed(tokens[:, t], t)
        done = t + 1
        if early_stop and bool((fe >= 0).all()):
            break
    return {"tokens": tokens, "attach": attach, "scores": torch.from_numpy(score), "first_end": torch.from_numpy(fe),
            "near": torch.from_numpy(near), "steps": done, "prefix_lp": plp, "prefix_score": psc}
