"""Host side of the KV-cached greedy decode (reference models.py:267-323, eval_step).

One decode step is a fixed kernel sequence that reads its step index from device memory
(csrc/decode.hip), so the step is captured ONCE in a hipGraph and replayed; the reference's
early-stop test (models.py:306, a device->host sync per token) becomes a check of a device flag
every ``check_every`` replays.

A lane is one runtime handle with its own encoder workspace and decode arena, stepping its share of the batch on its own stream.
One lane is the default: the single-stream step (1.210 ms at B 256) is ahead of two half-batch lanes in one captured graph (1.239 ms;
their kernels overlap for only 6.6 % of the busy time), so ``lanes=2`` stays as a measured alternative.  DESIGN.md has the rest.
"""
from __future__ import annotations

import collections
import functools
import ctypes as C
import math
import os

import torch

from . import _lib as L


class _Arena:
    """One growable uint8 device tensor that the library uses as a 256-byte-aligned workspace."""

    def __init__(self, slack=256):
        self.buf = None
        self.slack = slack                             # bytes allocated beyond the library's size (at least the 256 of the alignment)
        self.grown = 0                                 # allocations so far

    def ensure(self, nbytes, device):
        """Room for ``nbytes`` behind a 256-byte-aligned base.  Returns (base pointer, bytes usable from it)."""
        if self.buf is None or self.buf.numel() < nbytes + 256:
            self.buf = torch.empty(nbytes + self.slack, dtype=torch.uint8, device=device)
            self.grown += 1
        base = (self.buf.data_ptr() + 255) // 256 * 256
        return base, self.buf.numel() - (base - self.buf.data_ptr())

    def view(self, ptr, nbytes, dtype, shape):
        """The typed view of ``nbytes`` at a device pointer the library handed back."""
        off = ptr - self.buf.data_ptr()
        return self.buf[off: off + nbytes].view(dtype).view(shape)

    def data_ptr(self):
        return None if self.buf is None else self.buf.data_ptr()


def _buffers(name, handle, n):
    """The n device pointers of a ``*_buffers`` entry."""
    ptrs = [C.c_void_p() for _ in range(n)]
    L.check(getattr(L.lib(), name)(handle, *[C.byref(p) for p in ptrs]), name)
    return [p.value for p in ptrs]


class _Lane:
    def __init__(self, model, own_handle):
        self.model = model
        self.own = own_handle
        self.handle = model.new_bound_handle() if own_handle else None
        self.enc_ws = _Arena(slack=512)
        self.ws = _Arena()
        self.keep = None
        self.key = None                                # what a captured step depends on: (B, S, Tmax, flat, shadow, ws pointer, ws allocation, group)
        self.stream = None

    def h(self):
        return self.handle if self.own else self.model._handle

    def close(self):
        if self.own and self.handle is not None:
            L.lib().pa_model_destroy(self.handle)
            self.handle = None

    def begin(self, batch, Tmax, group=1):
        """Encoder on the batch as given + cross-K/V projection + state reset for this lane's rows: ``group`` decode rows per drawing
        of the batch over one memory per drawing (pa_decode_group_begin).  Returns the rows, B * group."""
        m, lib = self.model, L.lib()
        b, keep = m._make_batch(batch, with_output=False)
        b.T = 1
        dev = m.flat_params.device
        base, room = self.enc_ws.ensure(L.ws_bytes("pa_model_train_ws_bytes", self.h(), b.B, b.S, 1), dev)
        stats = torch.empty(L.lib().pa_model_stats_floats(), dtype=torch.float32, device=dev)   # include/plank_hip.h: f32[8]
        L.check(lib.pa_model_train_fwd(self.h(), C.byref(b), C.c_void_p(base), C.c_int64(room), C.c_uint32(0), 0,
                                       L.ptr(stats), L.stream()), "pa_model_train_fwd(encoder)")
        group = int(group)
        base, room = self.ws.ensure(L.ws_bytes("pa_decode_group_ws_bytes", self.h(), b.B, group, b.S, Tmax), dev)
        L.check(lib.pa_decode_group_begin(self.h(), group, C.c_void_p(base), C.c_int64(room), Tmax, L.stream()), "pa_decode_group_begin")
        self.keep = (b, keep, stats)
        shadow = m._shadow.data_ptr() if m._shadow is not None else 0
        self.key = (b.B, b.S, Tmax, m._flat.data_ptr(), shadow, self.ws.data_ptr(), self.ws.grown, group)
        return b.B * group

    def step(self):
        L.check(L.lib().pa_decode_step(self.h(), L.stream()), "pa_decode_step")

    def buffers(self, B, Tmax):
        tokens, attach, first_end, _ = _buffers("pa_decode_buffers", self.h(), 4)
        return (self.ws.view(tokens, B * Tmax * 8, torch.int64, (B, Tmax)), self.ws.view(attach, B * Tmax * 8, torch.int64, (B, Tmax)),
                self.ws.view(first_end, B * 4, torch.int32, (B,)))


def _split_batch(batch, lo, hi):
    out = {}
    for k, v in batch.items():
        if k.startswith("_"):
            continue                                   # packing / groupings are per sub-batch: recomputed by the lane
        out[k] = v[lo:hi] if (torch.is_tensor(v) or isinstance(v, list)) else v
    return out


def prefix_table(prefix, B, Tmax, vocab_size, end_token, pad_token, strict=True):
    """Checked forced prefix (include/plank_hip.h pa_decode_prefix_begin) of a batch of B drawings.

    ``prefix``: a dict with ``tokens`` int [B, P], optional ``attach`` int [B, P] (-1 = the vocab entry ``tokens``, j >= 0 = the
    pointer candidate j; default all -1) and optional ``lengths`` int [B] (default: up to and including the row's first END, else up
    to its first PAD, else P).  Returns CPU tensors (lengths int64 [B], tokens int64 [B, Tmax], attach int64 [B, Tmax]), zero /
    -1 beyond each row's length.  ValueError for P > Tmax, a length outside [0, P], a token outside [0, vocab_size) inside a row's
    length and - ``strict``, what the decoders ask for - a pointer with attach[t] >= t, a pointer at t < 5, an attach below -1, or
    tokens[t] != tokens[attach[t]].  ``strict=False`` (PlankModel.score) leaves those to the kernel, which scores a candidate that
    does not exist as -inf."""
    if not isinstance(prefix, dict) or "tokens" not in prefix:
        raise ValueError("prefix must be a dict with 'tokens' [B, P] (and optional 'attach', 'lengths')")
    tok = torch.as_tensor(prefix["tokens"]).detach().cpu().long()
    if tok.dim() != 2 or tok.shape[0] != B:
        raise ValueError(f"prefix tokens must be [B = {B}, P], got {tuple(tok.shape)}")
    P = tok.shape[1]
    if P > Tmax:
        raise ValueError(f"prefix of {P} positions is longer than the decode (Tmax {Tmax})")
    att = prefix.get("attach")
    att = torch.full_like(tok, -1) if att is None else torch.as_tensor(att).detach().cpu().long()
    if att.shape != tok.shape:
        raise ValueError(f"prefix attach must have the shape of tokens {tuple(tok.shape)}, got {tuple(att.shape)}")
    pos = torch.arange(P)[None, :].expand(B, P)
    lengths = prefix.get("lengths")
    if lengths is None:
        def first(mask, add):
            return torch.where(mask.any(1), mask.long().argmax(1) + add, torch.full((B,), P))
        lengths = torch.minimum(first(tok == end_token, 1), first(tok == pad_token, 0)) if P > 0 else torch.zeros(B, dtype=torch.long)
    else:
        lengths = torch.as_tensor(lengths).detach().cpu().long().reshape(-1)
        if lengths.shape[0] != B or bool(((lengths < 0) | (lengths > P)).any()):
            raise ValueError(f"prefix lengths must be [B = {B}] values in [0, P = {P}]")
    inside = pos < lengths[:, None]
    if bool((inside & ((tok < 0) | (tok >= vocab_size))).any()):
        raise ValueError(f"prefix token outside [0, {vocab_size}) inside a row's length")
    if strict:
        ptr = inside & (att != -1)
        if bool((inside & (att < -1)).any()):
            raise ValueError("prefix attach below -1")
        if bool((ptr & (att >= pos)).any()):
            raise ValueError("prefix pointer with attach[t] >= t")
        if bool((ptr & (pos < 5)).any()):
            raise ValueError("prefix pointer at t < 5 (the first plank has no pointer candidates)")
        src = tok.gather(1, att.clamp(0, max(P - 1, 0))) if P > 0 else tok
        if bool((ptr & (src != tok)).any()):
            raise ValueError("prefix tokens[t] != tokens[attach[t]] at a pointer")
    ptok = torch.zeros(B, Tmax, dtype=torch.long)
    patt = torch.full((B, Tmax), -1, dtype=torch.long)
    ptok[:, :P] = torch.where(inside, tok, torch.zeros_like(tok))
    patt[:, :P] = torch.where(inside, att, torch.full_like(att, -1))
    return lengths, ptok, patt


PlankGrammar = collections.namedtuple("PlankGrammar", "min_planks max_planks")
_NO_MAX = 2 ** 31 - 1                                  # max_planks None: the library clamps to the decode's last plank boundary


def plank_grammar(min_planks=1, max_planks=None):
    """Checked parameters of the plank grammar (include/plank_hip.h pa_decode_constraint_set): END is allowed
    from plank boundary ``min_planks`` on and forced at boundary ``max_planks`` (None: the last boundary that leaves room for END,
    (Tmax - 1) // 6, to which a larger value is clamped).  ValueError for what the library would refuse: a value that is no integer,
    min_planks < 0, max_planks < max(min_planks, 1)."""
    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if not is_int(min_planks) or not 0 <= min_planks < _NO_MAX:
        raise ValueError(f"MIN_PLANKS must be an integer >= 0, got {min_planks!r}")
    if max_planks is not None and (not is_int(max_planks) or not max(min_planks, 1) <= max_planks <= _NO_MAX):
        raise ValueError(f"MAX_PLANKS must be an integer >= max(MIN_PLANKS, 1) = {max(min_planks, 1)} (or None), got {max_planks!r}")
    return PlankGrammar(min_planks, max_planks)


def check_planks(tokens, end, n_val, min_planks=1):
    """Is every row a valid plank program up to its first END?  ``tokens`` int [B, n]; returns bool [B] (CPU).
    Valid: the row has an END, at a plank boundary (position 6 k) with k >= ``min_planks``; every position before it holds a
    coordinate value in [0, ``n_val``) - so no PAD - and each plank x0 y0 z0 x1 y1 z1 has max > min on every axis."""
    tok = torch.as_tensor(tokens).detach().cpu().long()
    B, n = tok.shape
    is_end = tok == end
    has_end = is_end.any(1)
    e = torch.where(has_end, is_end.long().argmax(1), torch.zeros(B, dtype=torch.long))
    ok = has_end & (e % 6 == 0) & (e // 6 >= min_planks)
    pos = torch.arange(n)[None, :]
    inside = pos < e[:, None]
    bad = inside & ((tok < 0) | (tok >= n_val))
    if n > 3:
        lo = torch.zeros_like(tok)
        lo[:, 3:] = tok[:, :-3]
        bad |= inside & (pos % 6 >= 3) & (tok <= lo)
    return ok & ~bad.any(1)


class GreedyDecoder:
    _repeat = None                                     # rows per drawing (BeamDecoder: K, SampleDecoder: N; None: the batch as given)
    share_encoder = False                              # the _repeat rows of a drawing as a decode group over ONE encoder pass and memory

    def __init__(self, model, use_graph=None, check_every=16, strict_graph=False, lanes=None):
        """``strict_graph``: a failed hipGraph capture raises instead of falling back to eager launches (benchmarks must
        not silently measure the slow path; PLANK_DECODE_GRAPH=1 has the same effect).  ``lanes``: 1 or 2 (default 1,
        PLANK_DECODE_LANES overrides); batches of fewer than 32 samples always run as one lane."""
        self.model = model
        self.check_every = check_every
        self.strict_graph = strict_graph
        if use_graph is None:
            use_graph = os.environ.get("PLANK_DECODE_GRAPH", "1") != "0"
        self.use_graph = use_graph
        # one lane by default since round 3: with the K/V append folded into the attention kernel the single-stream step
        # (1.210 ms at B 256) is ahead of the two half-batch lanes (1.239 ms)
        self.max_lanes = int(lanes if lanes is not None else os.environ.get("PLANK_DECODE_LANES", "1"))
        self._lanes = []
        self._graph = None
        self._side = None
        self._active = 0
        self.last_steps = 0
        self._key = {"lanes": None, "mode": None, "prefix": None, "constraint": None}   # what the captured step depends on (_rekey)
        self._mws = _Arena()                               # the mode's workspace (beam / sampling)
        self._pws = _Arena()                               # prefix workspace (pa_decode_prefix_begin)
        self._pkeep = None
        self.last_prefix_scores = None
        self.last_prefix_logprobs = None

    def __del__(self):
        try:
            for ln in self._lanes:
                ln.close()
        except Exception:
            pass

    def _lane(self, i):
        while len(self._lanes) <= i:
            self._lanes.append(_Lane(self.model, own_handle=len(self._lanes) > 0))
        return self._lanes[i]

    def _rekey(self, **parts):
        """The one place a captured step is dropped: when a part of what it captured - ``lanes``, ``mode``, ``prefix``,
        ``constraint`` - changed."""
        key = {**self._key, **parts}
        if key != self._key:
            self._graph = None
        self._key = key

    def _mode_begin(self, lane, rows, Tmax):
        """The mode's own begin on the begun lane (greedy: nothing).  Returns the mode's part of the graph key."""
        return None

    def begin(self, batch, max_len=None):
        """Encoder (on the batch with every drawing repeated ``_repeat`` times, or - ``share_encoder`` - on the batch as given, its
        ``_repeat`` rows per drawing a decode group over the drawing's one memory) + cross-K/V projection + state reset + the mode's
        begin.  Returns (rows, Tmax)."""
        m = self.model
        group = 1
        if self._repeat is not None and self.share_encoder:
            group = self._repeat
        elif self._repeat is not None:
            batch = _repeat_batch(batch, self._repeat)
            if m.unpad:
                batch = m.prepare_batch(batch, groups=False)
        Tmax = int(max_len or m.max_output_length)
        B = batch["input_value"].shape[0] * group
        n = 2 if (self.max_lanes >= 2 and B >= 32) else 1
        if n == 2 and group > 1:
            raise ValueError("a decode group (share_encoder) needs the one-lane decode (lanes=1)")
        self._bounds = [(0, B)] if n == 1 else [(0, B // 2), (B // 2, B)]
        self._active = n
        if n == 2 and self._side is None:
            self._side = torch.cuda.Stream()
        main = torch.cuda.current_stream()
        for i, (lo, hi) in enumerate(self._bounds):
            ln = self._lane(i)
            sub = batch if n == 1 else m.prepare_batch(_split_batch(batch, lo, hi), groups=False) if m.unpad else _split_batch(batch, lo, hi)
            if i == 0:
                ln.begin(sub, Tmax, group)
            else:
                self._side.wait_stream(main)
                with torch.cuda.stream(self._side):
                    ln.begin(sub, Tmax)
                main.wait_stream(self._side)
        self._rekey(lanes=tuple(ln.key for ln in self._lanes[:n]), mode=self._mode_begin(self._lanes[0], B, Tmax))
        return B, Tmax

    def _step_eager(self):
        main = torch.cuda.current_stream()
        if self._active == 2:
            self._side.wait_stream(main)               # fork
            with torch.cuda.stream(self._side):
                self._lanes[1].step()
            self._lanes[0].step()
            main.wait_stream(self._side)               # join
        else:
            self._lanes[0].step()

    def _capture(self):
        g = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream()
        cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cap):
            with torch.cuda.graph(g, stream=cap):
                self._step_eager()
        torch.cuda.current_stream().wait_stream(cap)
        return g

    def steps(self, n):
        """Enqueue n decode steps (graph replay when enabled)."""
        if self.use_graph and self._graph is None:
            try:
                self._graph = self._capture()
            except Exception as exc:                                  # pragma: no cover
                if self.strict_graph or os.environ.get("PLANK_DECODE_GRAPH") == "1":
                    raise
                print(f"[plankassembly_amd] hipGraph capture of the decode step failed ({exc}); running eagerly")
                self.use_graph = False
        for _ in range(n):
            if self.use_graph:
                self._graph.replay()
            else:
                self._step_eager()

    def _check_prefix(self, prefix, batch, max_len, strict=True):
        """The checked table of ``prefix`` (prefix_table) for this batch, before anything is launched; None without a prefix."""
        if prefix is None:
            return None
        if self.max_lanes >= 2:
            raise ValueError("a forced prefix needs the one-lane decode (lanes=1)")
        m = self.model
        return prefix_table(prefix, batch["input_value"].shape[0], int(max_len or m.max_output_length), m.vocab_size, m.token.END,
                            m.token.PAD, strict=strict)

    def _prefix_begin(self, table, repeat, rows, Tmax):
        """pa_decode_prefix_begin on the begun decode (every drawing's prefix repeated ``repeat`` times, _repeat_batch's layout), or -
        table None - nothing.  A captured step is dropped when the prefix appears, goes away or its workspace moves; a new table on
        the same workspace replays the same graph.  Returns (prefix_score [rows], prefix_lp [rows, Tmax]) device views, or None."""
        if table is None:
            self._rekey(prefix=None)
            return None
        ln = self._lanes[0]
        dev = self.model.flat_params.device
        lengths, ptok, patt = table
        plen = lengths.repeat_interleave(repeat).to(torch.int32).to(dev)
        ptok = ptok.repeat_interleave(repeat, dim=0).contiguous().to(dev)
        patt = patt.repeat_interleave(repeat, dim=0).contiguous().to(dev)
        assert plen.shape[0] == rows and ptok.shape == (rows, Tmax)
        base, room = self._pws.ensure(L.ws_bytes("pa_decode_prefix_ws_bytes", ln.h(), rows, Tmax), dev)
        L.check(L.lib().pa_decode_prefix_begin(ln.h(), L.ptr(plen), L.ptr(ptok), L.ptr(patt), C.c_void_p(base), C.c_int64(room),
                                               L.stream()), "pa_decode_prefix_begin")
        self._pkeep = (plen, ptok, patt)
        self._rekey(prefix=self._pws.data_ptr())
        score, lp = _buffers("pa_decode_prefix_buffers", ln.h(), 2)
        return self._pws.view(score, rows * 4, torch.float32, (rows,)), self._pws.view(lp, rows * Tmax * 4, torch.float32, (rows, Tmax))

    def _check_constraint(self, constraint):
        """The checked grammar of ``constraint`` (a plank_grammar() result; True: the default grammar), before anything is launched;
        None for None / False."""
        if constraint is None or constraint is False:
            return None
        if constraint is True:
            constraint = plank_grammar()
        if not isinstance(constraint, PlankGrammar):
            raise ValueError(f"constraint must come from decode.plank_grammar(), got {constraint!r}")
        constraint = plank_grammar(*constraint)
        if self.max_lanes >= 2:
            raise ValueError("a constraint needs the one-lane decode (lanes=1)")
        if getattr(self.model, "num_output_dof", 6) != 6:
            raise ValueError("the plank grammar is defined for six output DOF")
        return constraint

    def _constraint_begin(self, grammar):
        """pa_decode_constraint_set on the begun decode (``grammar`` None: nothing - pa_decode_begin cleared it).  The parameters are
        kernel arguments of the step: a captured step is dropped when they change, and replayed when they are the same."""
        if grammar is None:
            self._rekey(constraint=None)
            return
        tk = self.model.token
        p = L.ConstraintParams(min(tk.END, tk.PAD), grammar.min_planks, _NO_MAX if grammar.max_planks is None else grammar.max_planks, 0)
        L.check(L.lib().pa_decode_constraint_set(self._lanes[0].h(), C.byref(p)), "pa_decode_constraint_set")
        self._rekey(constraint=(p.n_val, p.min_planks, p.max_planks))

    def _loop(self, Tmax, early_stop, all_done, min_steps=0, max_steps=None):
        """The stepping loop of every mode: ``max_steps`` steps exactly, or up to Tmax with - ``early_stop`` - one look at the device
        (``all_done()``: has every row finished) after every ``check_every`` replays once ``min_steps`` have run; that look is the
        loop's only host sync.  Sets ``last_steps`` and returns the number of steps run."""
        if max_steps is not None:
            done = max(0, min(int(max_steps), Tmax))
            self.steps(done)
        else:
            done = 0
            while done < Tmax:
                k = min(self.check_every, Tmax - done) if early_stop else Tmax - done
                self.steps(k)
                done += k
                if early_stop and done >= min_steps and all_done():
                    break
        self.last_steps = done
        return done

    def run(self, batch, max_len=None, early_stop=True, prefix=None, max_steps=None, strict_prefix=True, constraint=None):
        """Full greedy decode.  Returns (samples int64 [B, n], attach int64 [B, n]) with the
        reference's early-stop length n.

        ``prefix`` (prefix_table): every row's first ``lengths`` positions are forced instead of taken by
        arg-max, and scored: ``last_prefix_scores`` f32 [B] (sum of log p over the forced positions up to and including the row's
        first END) and ``last_prefix_logprobs`` f32 [B, n] (per position, 0 where nothing was forced) are left on the decoder as CPU
        tensors (None after a run without a prefix).  The loop never stops before max(lengths) steps and n is at least that.
        ``max_steps``: run exactly this many steps (n = max_steps; the scorer).  ``strict_prefix=False``: prefix_table's
        non-strict checks (the scorer).

        ``constraint`` (plank_grammar()): the arg-max of every free step runs over the candidates the plank
        grammar allows, so every row is a valid program up to its first END.  Forced positions are not filtered."""
        table = self._check_prefix(prefix, batch, max_len, strict_prefix)
        grammar = self._check_constraint(constraint)
        B, Tmax = self.begin(batch, max_len)
        pbuf = self._prefix_begin(table, 1, B, Tmax)
        self._constraint_begin(grammar)
        bufs = [self._lanes[i].buffers(hi - lo, Tmax) for i, (lo, hi) in enumerate(self._bounds)]
        min_steps = int(table[0].max()) if table is not None and B > 0 else 0
        ends = None                                                   # every row's first END, once the host has seen them all

        def all_done():
            nonlocal ends
            fe = torch.cat([b[2] for b in bufs]).cpu()
            ends = fe if bool((fe >= 0).all()) else None
            return ends is not None

        n = self._loop(Tmax, early_stop, all_done, min_steps, max_steps)
        if max_steps is None:
            n = Tmax if ends is None else max(int(ends.max()) + 1, min_steps)
        self.last_prefix_scores = self.last_prefix_logprobs = None
        if pbuf is not None:
            self.last_prefix_scores, self.last_prefix_logprobs = pbuf[0].cpu(), pbuf[1][:, :n].cpu()
        tokens = torch.cat([b[0][:, :n] for b in bufs]) if len(bufs) > 1 else bufs[0][0][:, :n].clone()
        attach = torch.cat([b[1][:, :n] for b in bufs]) if len(bufs) > 1 else bufs[0][1][:, :n].clone()
        return tokens, attach


def _share_flag(v):
    if not isinstance(v, bool):
        raise ValueError(f"SHARE_ENCODER must be a bool, got {v!r}")
    return v


def _repeat_batch(batch, K):
    """Every drawing repeated K times, drawing-major (row b*K + k is beam k of drawing b)."""
    out = {}
    for k, v in batch.items():
        if k.startswith("_"):
            continue                                   # packing / groupings belong to the repeated batch: recomputed
        if torch.is_tensor(v):
            out[k] = v.repeat_interleave(K, dim=0)
        elif isinstance(v, list):
            out[k] = [x for x in v for _ in range(K)]
        else:
            out[k] = v
    return out


class BeamDecoder(GreedyDecoder):
    """Beam search over the KV-cached decode step (include/plank_hip.h pa_decode_beam_*).

    The decode runs B*K hypothesis rows - the encoder on the batch with every drawing repeated K times - and each captured step
    ends with the beam selection (per-row top-K of the greedy step's own distribution, merge per drawing, history reorder)
    instead of the greedy arg-max.  Always one lane.  ``length_penalty`` (alpha) only changes the final ranking of a drawing's
    beams, by score / len^alpha (len = first END + 1, or Tmax); 0 ranks by the raw cumulative log-probability.  K = 1 gives the
    greedy tokens up to each row's first END (PAD / attach -1 after it).  ``share_encoder``: the encoder runs on the batch as given and
    the K beams of a drawing decode over its one memory - the same search."""

    def __init__(self, model, beam_size, length_penalty=0.0, use_graph=None, check_every=16, strict_graph=False, share_encoder=False):
        super().__init__(model, use_graph=use_graph, check_every=check_every, strict_graph=strict_graph, lanes=1)
        self.share_encoder = _share_flag(share_encoder)
        self.beam_size = int(beam_size)
        self.length_penalty = float(length_penalty)
        self._repeat = self.beam_size
        model._ensure_handle()
        # the library validates K (1 <= K <= PA_BEAM_MAX): PlankHipError here rather than at the first run
        L.ws_bytes("pa_decode_beam_ws_bytes", model._handle, self.beam_size, 1, 1, self.beam_size)

    def _mode_begin(self, lane, rows, Tmax):
        K = self.beam_size
        base, room = self._mws.ensure(L.ws_bytes("pa_decode_beam_ws_bytes", lane.h(), rows, lane.keep[0].S, Tmax, K),
                                      self.model.flat_params.device)
        L.check(L.lib().pa_decode_beam_begin(lane.h(), K, C.c_void_p(base), C.c_int64(room), L.stream()), "pa_decode_beam_begin")
        return self._mws.data_ptr(), K

    def _beam_buffers(self, rows):
        return [self._mws.view(p, rows * 4, dt, (rows,))
                for p, dt in zip(_buffers("pa_decode_beam_buffers", self._lanes[0].h(), 3), (torch.float32, torch.int32, torch.int32))]

    def run(self, batch, max_len=None, early_stop=True, prefix=None, constraint=None):
        """Full beam search.  Returns a dict: ``tokens`` / ``attach`` int64 [B, n] (the best beam), ``beam_tokens`` /
        ``beam_attach`` int64 [B, K, n], ``scores`` f32 [B, K] (cumulative log-probability), ``finished`` bool [B, K] and
        ``lengths`` int64 [B, K], beams in final-ranking order.  n = max over rows of first END + 1 once every beam has
        finished, else Tmax - the same with and without ``early_stop``.

        ``prefix`` (prefix_table, per drawing): the first ``lengths`` positions of every drawing are forced;
        beam 0 carries the hypothesis through them and the first free step fans out.  The dict always has ``prefix_scores`` f32
        [B, K] and ``prefix_logprobs`` f32 [B, K, n] - the log-probabilities of the forced positions, which every beam of a drawing
        shares; zeros without a prefix.  ``scores`` stay the log-likelihood of the whole sequence.

        ``constraint`` (plank_grammar()): the per-row top-K of every free step is taken among the candidates
        the plank grammar allows; ``scores`` are not renormalised."""
        K = self.beam_size
        table = self._check_prefix(prefix, batch, max_len)
        grammar = self._check_constraint(constraint)
        rows, Tmax = self.begin(batch, max_len)
        pbuf = self._prefix_begin(table, K, rows, Tmax)
        self._constraint_begin(grammar)
        B = rows // K
        tokens, attach, first_end = self._lanes[0].buffers(rows, Tmax)
        scores, _, finished = self._beam_buffers(rows)
        self._loop(Tmax, early_stop, lambda: bool((finished != 0).all().cpu()))
        if pbuf is not None:                                          # the drawing's forced positions were scored on its row b*K
            pbuf = (pbuf[0].view(B, K)[:, :1].expand(B, K).reshape(rows),
                    pbuf[1].view(B, K, Tmax)[:, :1].expand(B, K, Tmax).reshape(rows, Tmax))
        return _ranked("beam", tokens, attach, first_end, scores, finished != 0, B, K, Tmax, self.length_penalty, pbuf)


def _ranked(prefix, tokens, attach, first_end, scores, finished, B, K, Tmax, length_penalty, pbuf=None):
    """The final ranking shared by beam search and sampling: the K rows b*K + k of every drawing b ordered by score / len^alpha
    descending, stable (len = first END + 1, or Tmax; alpha = 0 ranks by the raw score).  n = max over rows of first END + 1 once
    every row has finished, else Tmax.  Returns the decoders' result dict, ``<prefix>_tokens`` / ``<prefix>_attach`` [B, K, n];
    ``pbuf``: the rows' (prefix_score [rows], prefix_lp [rows, Tmax]) of a forced prefix, ranked alike (None: zeros)."""
    fe = first_end.view(B, K).long().cpu()
    fin = finished.view(B, K).cpu()
    n = int(fe.max()) + 1 if bool(fin.all()) else Tmax
    sc = scores.view(B, K).cpu()
    lengths = torch.where(fe >= 0, fe + 1, torch.full_like(fe, Tmax))
    key = sc / lengths.to(torch.float32) ** length_penalty if length_penalty != 0.0 else sc
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    dev = tokens.device
    od = order.to(dev)
    bt = tokens.view(B, K, Tmax)[:, :, :n].gather(1, od[:, :, None].expand(B, K, n)).contiguous()
    ba = attach.view(B, K, Tmax)[:, :, :n].gather(1, od[:, :, None].expand(B, K, n)).contiguous()
    if pbuf is None:
        ps, pl = torch.zeros(B, K), torch.zeros(B, K, n)
    else:
        ps = pbuf[0].view(B, K).cpu().gather(1, order)
        pl = pbuf[1].view(B, K, Tmax)[:, :, :n].cpu().gather(1, order[:, :, None].expand(B, K, n))
    return {"tokens": bt[:, 0].clone(), "attach": ba[:, 0].clone(), f"{prefix}_tokens": bt, f"{prefix}_attach": ba,
            "scores": sc.gather(1, order), "finished": fin.gather(1, order), "lengths": lengths.gather(1, order),
            "prefix_scores": ps, "prefix_logprobs": pl}


def sample_params(num_samples, temperature=1.0, top_k=0, top_p=1.0, seed=0):
    """Checked sampling parameters (include/plank_hip.h pa_sample_params): ValueError for a value the library would refuse."""
    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if not is_int(num_samples) or not 1 <= num_samples <= 64:
        raise ValueError(f"NUM_SAMPLES must be an integer in [1, 64], got {num_samples!r}")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or temperature <= 0:
        raise ValueError(f"TEMPERATURE must be a finite number > 0, got {temperature!r}")
    if not is_int(top_k) or top_k < 0:
        raise ValueError(f"TOP_K must be an integer >= 0 (0 = off), got {top_k!r}")
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not 0 < top_p <= 1:
        raise ValueError(f"TOP_P must be a number in (0, 1] (1 = off), got {top_p!r}")
    if not is_int(seed) or not 0 <= seed < 2 ** 32:
        raise ValueError(f"SAMPLE_SEED must be an integer in [0, 2^32), got {seed!r}")
    return L.SampleParams(seed, num_samples, float(temperature), top_k, float(top_p))


class SampleDecoder(GreedyDecoder):
    """Seeded top-k / top-p sampling over the KV-cached decode step (include/plank_hip.h pa_decode_sample_*).

    The decode runs B*N sample rows - the encoder on the batch with every drawing repeated N times, row b*N + n is sample n of
    drawing b - and each captured step ends with one random draw per row (dec_sample_draw_kernel) instead of the greedy arg-max.
    The draw of sample n of drawing b at step t depends on (seed, b, n, t) only, so drawings are keyed by their position in the
    batch.  Always one lane.  Every sample carries its score, the sum of log p of its tokens under the model (untempered,
    unfiltered); ``length_penalty`` (alpha) ranks a drawing's samples by score / len^alpha.  top_k = 1 gives the greedy tokens up
    to each row's first END (PAD / attach -1 after it).  ``share_encoder``: the encoder runs on the batch as given and the N samples
    of a drawing decode over its one memory - the same draws (seed, b, n, t)."""

    def __init__(self, model, num_samples, temperature=1.0, top_k=0, top_p=1.0, seed=0, length_penalty=0.0, use_graph=None,
                 check_every=16, strict_graph=False, share_encoder=False):
        super().__init__(model, use_graph=use_graph, check_every=check_every, strict_graph=strict_graph, lanes=1)
        self.share_encoder = _share_flag(share_encoder)
        self.params = sample_params(num_samples, temperature, top_k, top_p, seed)
        self.num_samples = int(num_samples)
        self.length_penalty = float(length_penalty)
        self._repeat = self.num_samples
        model._ensure_handle()

    def _mode_begin(self, lane, rows, Tmax):
        base, room = self._mws.ensure(L.ws_bytes("pa_decode_sample_ws_bytes", lane.h(), rows), self.model.flat_params.device)
        L.check(L.lib().pa_decode_sample_begin(lane.h(), C.byref(self.params), C.c_void_p(base), C.c_int64(room), L.stream()),
                "pa_decode_sample_begin")
        return self._mws.data_ptr(), self.num_samples

    def _scores(self, rows):
        return self._mws.view(_buffers("pa_decode_sample_buffers", self._lanes[0].h(), 1)[0], rows * 4, torch.float32, (rows,))

    def run(self, batch, max_len=None, early_stop=True, seed=None, prefix=None, constraint=None):
        """N samples per drawing.  ``seed``: this call's seed instead of the decoder's (pa_decode_sample_set: the captured step is
        reused).  Returns a dict: ``tokens`` / ``attach`` int64 [B, n] (the best sample), ``sample_tokens`` / ``sample_attach``
        int64 [B, N, n], ``scores`` f32 [B, N] (log-likelihood of each sample), ``finished`` bool [B, N] and ``lengths`` int64
        [B, N], samples in final-ranking order.  n = max over rows of first END + 1 once every sample has finished, else Tmax -
        the same with and without ``early_stop``.

        ``prefix`` (prefix_table, per drawing): the first ``lengths`` positions of every sample of a drawing
        are forced (no draw; the random numbers of the free steps are those of a run without a prefix).  The dict always has
        ``prefix_scores`` f32 [B, N] and ``prefix_logprobs`` f32 [B, N, n], zeros without a prefix; ``scores`` stay the
        log-likelihood of the whole sample.

        ``constraint`` (plank_grammar()): the candidate set of every free step is what the plank grammar
        allows; temperature, top-k, top-p and the draw act on that set, u is unchanged and ``scores`` are not renormalised."""
        N = self.num_samples
        table = self._check_prefix(prefix, batch, max_len)
        grammar = self._check_constraint(constraint)
        rows, Tmax = self.begin(batch, max_len)
        pbuf = self._prefix_begin(table, N, rows, Tmax)
        self._constraint_begin(grammar)
        if seed is not None:
            p = self.params
            q = sample_params(N, p.temperature, p.top_k, p.top_p, seed)
            L.check(L.lib().pa_decode_sample_set(self._lanes[0].h(), C.byref(q), L.stream()), "pa_decode_sample_set")
        B = rows // N
        tokens, attach, first_end = self._lanes[0].buffers(rows, Tmax)
        scores = self._scores(rows)
        self._loop(Tmax, early_stop, lambda: bool((first_end >= 0).all().cpu()))
        return _ranked("sample", tokens, attach, first_end, scores, first_end >= 0, B, N, Tmax, self.length_penalty, pbuf)

    def run_device(self, batch, max_len=None, early_stop=True, seed=None, constraint=None):
        """``run`` up to and including the stepping loop, for callers that go on working on the device (PlankModel.sequence_batch;
        DESIGN.md section 24): the same begin, seed, constraint and steps, then the decoder's own buffers as they are - unranked,
        not cut to the longest row, nothing copied to the host beyond the loop's early-stop look.  Returns ``tokens`` / ``attach``
        int64 [rows, Tmax], ``first_end`` int32 [rows] (-1: the row never ended) and ``scores`` f32 [rows], rows = B * N with row
        b * N + n sample n of drawing b.  They are views into the decoder's workspaces: valid until this decoder's next ``begin``
        (its next ``run`` / ``run_device``), which overwrites them in place or moves them."""
        grammar = self._check_constraint(constraint)
        rows, Tmax = self.begin(batch, max_len)
        self._prefix_begin(None, self.num_samples, rows, Tmax)
        self._constraint_begin(grammar)
        if seed is not None:
            p = self.params
            q = sample_params(self.num_samples, p.temperature, p.top_k, p.top_p, seed)
            L.check(L.lib().pa_decode_sample_set(self._lanes[0].h(), C.byref(q), L.stream()), "pa_decode_sample_set")
        tokens, attach, first_end = self._lanes[0].buffers(rows, Tmax)
        scores = self._scores(rows)
        self._loop(Tmax, early_stop, lambda: bool((first_end >= 0).all().cpu()))
        return tokens, attach, first_end, scores


@functools.lru_cache(maxsize=8)
def _consensus_pairs(B, N, device):
    """The B * N (N - 1) / 2 row pairs n < m of a [B * N, n] sample matrix (int32 [P, 2] on ``device``) and the (n, m) index rows."""
    iu = torch.triu_indices(N, N, 1)
    base = torch.arange(B)[:, None] * N
    pairs = torch.stack([(base + iu[0]).reshape(-1), (base + iu[1]).reshape(-1)], 1).to(torch.int32)
    return pairs.to(device), iu[0].to(device), iu[1].to(device)


def consensus_select(sample_tokens, end_token, threshold=0.5):
    """Minimum-Bayes-risk choice among the N samples of every drawing under the project's own metric.

    ``sample_tokens`` int64 [B, N, n] on the device.  One ``ops.plank_match`` launch compares the samples of a drawing pairwise as
    sets of planks (both sides without their zero-extent planks, edges at IoU > ``threshold``, ties no edges); F1(n, m) = 2 tp /
    (n_a + n_b) in float64, 0 where tp == 0.  The utility of sample n is the INTEGER sum over m != n of rint(F1 * 2^40): integer
    sums do not depend on their order, so duplicated samples - common at low temperature - get exactly equal utilities and the
    lowest index (the most likely sample) wins among equals.  Everything stays on the device; nothing is read back.
    Returns ``consensus_index`` int64 [B] and ``consensus_f1`` float64 [B, N] = utility / 2^40 / max(N - 1, 1)."""
    from . import ops
    B, N, n = sample_tokens.shape
    dev = sample_tokens.device
    if N == 1 or B == 0:
        return {"consensus_index": torch.zeros(B, dtype=torch.int64, device=dev),
                "consensus_f1": torch.zeros(B, N, dtype=torch.float64, device=dev)}
    flat = sample_tokens.reshape(B * N, n)
    pairs, iu0, iu1 = _consensus_pairs(B, N, dev)
    c = ops.plank_match(flat, flat, pairs, end_token=end_token, filter_a=True, filter_b=True, threshold=threshold,
                        check_pairs=False).view(B, -1, 4).to(torch.int64)
    f1 = (2 * c[..., 0]).double() / (c[..., 1] + c[..., 2]).clamp(min=1).double()
    q = torch.round(f1 * 2.0 ** 40).to(torch.int64)
    pairwise = torch.zeros(B, N, N, dtype=torch.int64, device=dev)
    pairwise[:, iu0, iu1] = q
    pairwise[:, iu1, iu0] = q
    utility = pairwise.sum(2)
    best = utility.max(1, keepdim=True).values
    index = torch.where(utility == best, torch.arange(N, device=dev)[None, :], N).min(1).values
    # (a device tensor as the divisor: torch divides by a host scalar as a multiplication by its reciprocal, one rounding too many)
    others = torch.full((), float(max(N - 1, 1)), dtype=torch.float64, device=dev)
    return {"consensus_index": index, "consensus_f1": utility.double() / 2.0 ** 40 / others}


def redraw_planks(tokens, end_token, num_bits, dof=6):
    """Decoded rows -> the planks they state: ``tokens`` integer [B, n] (any device) -> (coords float64 [B, n // dof, dof],
    n_planks int64 [B]).  A row is cut at its first ``end_token`` (its whole length without one) into L // dof planks; every
    token is dequantised as ``datasets.dequantize_values`` does (q * 2 / (2^bits - 1) - 1, each operation rounded on its own),
    whatever it is - a token that is no coordinate lands outside [-1, 1] and puts the row out of the renderer's domain.  torch
    ops only, nothing is read back."""
    B, n = tokens.shape
    dev = tokens.device
    is_end = tokens == end_token
    length = torch.full((B,), n, dtype=torch.int64, device=dev)
    if n > 0:                                          # (argmax over an empty dimension raises)
        length = torch.where(is_end.any(1), is_end.long().argmax(1), length)
    P = n // dof
    # (a device tensor as the divisor: torch divides by a host scalar as a multiplication by its reciprocal, one rounding too many)
    rq = torch.full((), float(2 ** int(num_bits) - 1), dtype=torch.float64, device=dev)
    coords = (tokens[:, :P * dof].to(torch.float64) * 2.0) / rq + (-1.0)
    return coords.reshape(B, P, dof).contiguous(), torch.div(length, dof, rounding_mode="floor")


def _redraw(tokens, end_token, pad_token, num_bits, dof, max_input_length, with_type=True):
    """``redraw`` on plain values.  A row wider than the render kernel's plank cap is not refused for its width: the planks
    tensor is cut at the cap, and a row that STATES more planks than the cap renders the first ones and gets
    PA_RENDER_TRUNCATED - the flag is set here with torch ops, so nothing is read back."""
    from . import ops
    coords, n_planks = redraw_planks(tokens, end_token, num_bits, dof)
    cap = ops.RENDER_MAX_PLANKS
    out = ops.render_drawings(coords[:, :cap].contiguous(), n_planks.clamp(max=cap), max_input_length=max_input_length,
                              num_bits=num_bits, end_token=end_token, pad_token=pad_token, with_type=with_type)
    if coords.shape[1] > cap:
        over = (n_planks > cap).to(torch.int32) * 2                # include/plank_hip.h PA_RENDER_TRUNCATED
        out["_render_flags"] = out["_render_flags"] | over
    return out


def redraw(tokens, token, data_cfg):
    """The model's input for the programs it decoded: ``tokens`` int64 [B, n] on the device
    (``output_value`` of a decode: values, END, PAD) are cut into planks and dequantised (``redraw_planks``), rendered on the
    device (``ops.render_drawings``; plank 0 is the bounding box and is not drawn) and returned as an input batch the model
    accepts, with ``_render_flags`` / ``_lines`` / ``_views`` / ``_types`` / ``_n_lines``.  Rows of any width are taken; a row
    that states more than PA_RENDER_MAX_PLANKS (32) planks renders its first 32 and is flagged PA_RENDER_TRUNCATED.  Nothing
    is read back."""
    return _redraw(tokens, int(token.END), int(token.PAD), int(data_cfg.NUM_BITS), int(data_cfg.get("NUM_OUTPUT_DOF", 6)),
                   int(data_cfg.MAX_INPUT_LENGTH))


REPROJECTION_TYPES = ("ignore", "match", "visible")


def check_reprojection(tol=1, types="ignore"):
    """The two options of the reprojection score, validated -> (tol int in 0 .. 255, types)."""
    if isinstance(tol, bool) or not isinstance(tol, int) or not 0 <= tol <= 255:
        raise ValueError(f"REPROJECTION_TOL must be an integer in [0, 255], got {tol!r}")
    if types not in REPROJECTION_TYPES:
        raise ValueError(f"REPROJECTION_TYPES must be one of {REPROJECTION_TYPES}, got {types!r}")
    return tol, types


def _reprojection(batch, tokens, end_token, pad_token, num_bits, dof, max_input_length, with_type, tol, types, pairs):
    """``reprojection_scores`` on plain values."""
    from . import ops
    from .metric import overlap_scores
    tol, types = check_reprojection(tol, types)
    given = (batch["input_value"], batch["input_view"], batch.get("input_type"))
    if types == "match" and (given[2] is None or not with_type):
        raise ValueError("types='match' needs input_type in the batch and a rendering with types")
    dev = tokens.device
    given = tuple(None if t is None else t.to(device=dev, dtype=torch.int64) for t in given)
    drawn = _redraw(tokens, end_token, pad_token, num_bits, dof, max_input_length, with_type=with_type)
    counts = ops.line_overlap(given, drawn, pairs, end_token=end_token, num_bits=num_bits, tol=tol, types=types, check_pairs=False)
    rec, prec, f1 = overlap_scores(counts)
    return {"reprojection_precision": prec, "reprojection_recall": rec, "reprojection_f1": f1, "reprojection_counts": counts,
            "reprojection_flags": drawn["_render_flags"]}


def reprojection_scores(batch, tokens, token, data_cfg_or_bits, *, tol=1, types="ignore", pairs=None):
    """How well the three views of decoded programs match the drawings that were given - a score that
    needs no ground truth and nothing of the other samples.

    ``batch``: the input batch (``input_value`` / ``input_view`` / optional ``input_type`` int64 [B, S] on the device; LINE
    drawings only - the tokens of a sideface input are faces, not lines).  ``tokens`` int64 [R, n] on the device: one program
    per row (values, END, PAD).  They are rendered on the device (``_redraw``: plank 0, the bounding box, is not drawn) and
    compared with the given rows by one ``ops.line_overlap``: pair i is (row i of the batch, row i of ``tokens``), or
    ``pairs`` int [P, 2] of (batch row, tokens row) - which must exist, they are not checked.  ``data_cfg_or_bits``: the DATA
    config (NUM_BITS, MAX_INPUT_LENGTH, NUM_OUTPUT_DOF) or the number of bits alone (the rendering is then as wide as the batch).
    ``tol``: a rendered line counts within this many quantisation levels (default 1: the dataset quantises the mirrored
    coordinate itself, one level off the mirrored token, on every view's second axis).  ``types``: ``ignore`` | ``match`` |
    ``visible`` (``ops.line_overlap``).

    Returns ``reprojection_recall`` = cov(given | rendered) / len(given), ``reprojection_precision`` = cov(rendered | given) /
    len(rendered) and ``reprojection_f1`` = 2 p r / (p + r), float64 [P], each 0 where its denominator is 0;
    ``reprojection_counts`` int32 [P, 8]; ``reprojection_flags`` int32 [R], the ``_render_flags`` of every row of ``tokens``: a
    row outside the renderer's domain renders nothing and scores 0, truncated and overflow rows are scored as rendered.
    Nothing is read back."""
    if hasattr(data_cfg_or_bits, "NUM_BITS"):
        cfg = data_cfg_or_bits
        bits, dof, width = int(cfg.NUM_BITS), int(cfg.get("NUM_OUTPUT_DOF", 6)), int(cfg.MAX_INPUT_LENGTH)
    else:
        bits, dof, width = int(data_cfg_or_bits), 6, int(batch["input_value"].shape[1]) + 1
    return _reprojection(batch, tokens, int(token.END), int(token.PAD), bits, dof, width, True, tol, types, pairs)


@functools.lru_cache(maxsize=8)
def _reprojection_pairs(B, N, device):
    """(drawing b, sample row b * N + n) for every sample: int32 [B * N, 2] on ``device``."""
    rows = torch.arange(B * N, dtype=torch.int32)
    return torch.stack([torch.div(rows, N, rounding_mode="floor"), rows], 1).to(device)


def _pick_reprojection(r, B, N):
    """The flat result ``r`` of B * N pairs (b, b * N + n) as [B, N, ...] tensors, with ``reprojection_index``."""
    out = {k: v.reshape(B, N, *v.shape[1:]) for k, v in r.items()}
    f1 = out["reprojection_f1"]
    best = f1.max(1, keepdim=True).values
    out["reprojection_index"] = torch.where(f1 == best, torch.arange(N, device=f1.device)[None, :], N).min(1).values
    return out


def reprojection_select(batch, sample_tokens, token, data_cfg_or_bits, *, tol=1, types="ignore"):
    """The sample of every drawing whose rendering matches the given drawing best: ``sample_tokens``
    int64 [B, N, n] on the device with N >= 1, sample n of drawing b scored against row b of ``batch`` by
    ``reprojection_scores`` (pairs (b, b * N + n); line drawings only).  Returns ``reprojection_index`` int64 [B] - the largest
    F1, the lowest index (the most likely sample) among equal bits - and the keys of ``reprojection_scores`` reshaped to
    [B, N, ...].  Nothing is read back."""
    B, N, n = sample_tokens.shape
    r = reprojection_scores(batch, sample_tokens.reshape(B * N, n), token, data_cfg_or_bits, tol=tol, types=types,
                            pairs=_reprojection_pairs(B, N, sample_tokens.device))
    return _pick_reprojection(r, B, N)


def volume_scores(reference_tokens, tokens, end_token, pairs=None):
    """Decoded programs as solids: how much of the space the reference occupies a program occupies too,
    and how much of a program's plank volume lies inside another of its own planks.

    ``tokens`` int64 [R, n] on the device: one program per row; ``reference_tokens`` int64 [Rr, m] on the device (side a, the
    ground truth) or None.  One ``ops.plank_volume`` launch: pair i is (row i, row i), or ``pairs`` int [P, 2] of (reference
    row, tokens row) - which must exist, they are not checked.  Returns ``volume_iou`` = inter / union, ``volume_recall`` =
    inter / union(reference), ``volume_precision`` = inter / union(tokens), ``self_overlap`` = (sum - union) / sum of ``tokens``,
    float64 [P], each 0 where its denominator is 0, and ``volume_counts`` int64 [P, 8].  With ``reference_tokens=None`` - no
    ground truth is needed for it - only ``self_overlap`` and ``volume_counts`` (``pairs``: int [P] rows of ``tokens``, which are
    then side a of the counts).  Nothing is read back."""
    from . import ops
    from .metric import volume_scores as scores_of
    if reference_tokens is None:
        counts = ops.plank_volume(tokens, None, pairs, end_token=end_token, check_pairs=False)
        return {"self_overlap": scores_of(counts)["self_overlap_a"], "volume_counts": counts}
    counts = ops.plank_volume(reference_tokens, tokens, pairs, end_token=end_token, check_pairs=False)
    s = scores_of(counts)
    return {"volume_iou": s["volume_iou"], "volume_precision": s["volume_precision"], "volume_recall": s["volume_recall"],
            "self_overlap": s["self_overlap_b"], "volume_counts": counts}


def _pick_volume(counts, N, iu0, iu1):
    """``volume_select`` from the int64 [B, N (N - 1) / 2, 8] counts of the pairs (iu0[k], iu1[k]) - on any device."""
    from .metric import volume_scores as scores_of
    B = counts.shape[0]
    dev = counts.device
    q = torch.round(scores_of(counts)["volume_iou"] * 2.0 ** 40).to(torch.int64)
    pairwise = torch.zeros(B, N, N, dtype=torch.int64, device=dev)
    pairwise[:, iu0, iu1] = q
    pairwise[:, iu1, iu0] = q
    utility = pairwise.sum(2)
    best = utility.max(1, keepdim=True).values
    index = torch.where(utility == best, torch.arange(N, device=dev)[None, :], N).min(1).values
    own = torch.zeros(B, N, 8, dtype=torch.int64, device=dev)              # (union, sum) of every sample, as side a of a pair
    own[:, iu0, :2] = counts[..., 0:2]                                     # every pair of a sample states the same two integers
    own[:, iu1, :2] = counts[..., 2:4]
    # (a device tensor as the divisor: torch divides by a host scalar as a multiplication by its reciprocal, one rounding too many)
    others = torch.full((), float(max(N - 1, 1)), dtype=torch.float64, device=dev)
    return {"volume_index": index, "volume_iou": utility.double() / 2.0 ** 40 / others,
            "self_overlap": scores_of(own)["self_overlap_a"]}


def volume_select(sample_tokens, end_token):
    """Minimum-Bayes-risk choice among the N samples of every drawing with the shape IoU as the utility:
    as ``consensus_select``, with ``volume_iou(n, m)`` in place of the pairwise F1 - graded, so it still ranks where no two
    samples share a plank at IoU > 0.5.

    ``sample_tokens`` int64 [B, N, n] on the device.  One ``ops.plank_volume`` launch over the pairs n < m of every drawing.  The
    utility of sample n is the INTEGER sum over m != n of rint(iou * 2^40); the largest wins, the lowest index among equals;
    two samples that both occupy nothing have IoU 0 with each other.  Returns ``volume_index`` int64 [B], ``volume_iou``
    float64 [B, N] = utility / 2^40 / max(N - 1, 1) and ``self_overlap`` float64 [B, N], every sample's (sum - union) / sum from
    the same counts.  Nothing is read back."""
    from . import ops
    from .metric import volume_scores as scores_of
    B, N, n = sample_tokens.shape
    dev = sample_tokens.device
    flat = sample_tokens.reshape(B * N, n)
    if N == 1 or B == 0:
        own = ops.plank_volume(flat, None, end_token=end_token)
        return {"volume_index": torch.zeros(B, dtype=torch.int64, device=dev),
                "volume_iou": torch.zeros(B, N, dtype=torch.float64, device=dev),
                "self_overlap": scores_of(own)["self_overlap_a"].reshape(B, N)}
    pairs, iu0, iu1 = _consensus_pairs(B, N, dev)
    counts = ops.plank_volume(flat, flat, pairs, end_token=end_token, check_pairs=False)
    return _pick_volume(counts.view(B, -1, 8), N, iu0, iu1)
