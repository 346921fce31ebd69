"""CPU reference of the sampling decode, in float64.

The cached decoder loop of tests/beam_reference.py (``_Stepper``, no reorder: samples are independent) on B*N rows, row b*N + n
being sample n of drawing b, and per live row and step the selection of section 13:
  * candidates: the vocab entries and the pointers j < t of ``last_row_dist`` (the self pointer j = t never), p = 0 never;
  * rank order: p descending, ties to the smaller index; w = exp((log p - log p_max) / tau), p / p_max at tau = 1;
  * top_k > 0 keeps the first top_k in rank order; top_p < 1 then keeps the shortest rank-order prefix whose cumulative w reaches
    top_p times the sum of the kept w;
  * u = (h >> 8) 2^-24, h = mix32(t ^ mix32(n ^ mix32(b ^ mix32(seed + 0x9e3779b9)))) (``sample_u``, tests/dropout_masks.py mix32);
    the chosen candidate is the first kept one in index order whose inclusive prefix sum of w exceeds u W (W = the total), else
    the last kept one;
  * a pointer j takes the row's own token at j; the score gains log p (untempered, unfiltered); a row that has emitted END is
    frozen (PAD, attach -1, score + 0, PAD as the next input).
Temperature and top_p are used as the float32 values the library receives.  Besides the samples it returns a near-boundary flag per
row and step: the decision was within a relative ``tol`` of changing (u W against the chosen candidate's two prefix-sum edges,
relative to W; the k-th against the (k+1)-th p; the top-p running sum against top_p W at the nucleus edge, and the p of the last
candidate in the nucleus against the next one).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from beam_reference import _Stepper, _params
from dropout_masks import mix32


def sample_hash(seed, b, n, t):
    """The 32-bit hash h of sample n of drawing b at step t (uint64 numpy holding uint32; broadcasting over b, n, t)."""
    u32 = lambda v: np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    return mix32(u32(t) ^ mix32(u32(n) ^ mix32(u32(b) ^ mix32(u32(int(seed) + 0x9E3779B9)))))


def sample_u(seed, b, n, t):
    """u = (h >> 8) 2^-24 in [0, 1) (float64, exact)."""
    return (sample_hash(seed, b, n, t) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def select(p, u, temperature=1.0, top_k=0, top_p=1.0, tol=1e-4):
    """One draw from the candidate probabilities p (float64 numpy [nc], index order).  Returns (index, near-boundary flag)."""
    order = np.argsort(-p, kind="stable")                          # rank order: p descending, ties to the smaller index
    order = order[p[order] > 0]
    pmax = p[order[0]]
    w = np.zeros_like(p)
    if temperature == 1.0:
        w[order] = p[order] / pmax
    else:
        w[order] = np.exp((np.log(p[order]) - math.log(pmax)) / temperature)
    near = False
    kept = order
    if 0 < top_k < len(order):
        a, b = p[order[top_k - 1]], p[order[top_k]]
        near |= bool(a > b and a - b <= tol * a)                   # (exact ties resolve by index alike)
        kept = order[:top_k]
    if top_p < 1.0:
        cs = np.cumsum(w[kept])
        tw = top_p * cs[-1]
        m = min(int(np.searchsorted(cs, tw, side="left")), len(kept) - 1)
        near |= bool(abs(cs[m] - tw) <= tol * cs[-1] or (m > 0 and abs(cs[m - 1] - tw) <= tol * cs[-1]))
        if m + 1 < len(kept):
            a, b = p[kept[m]], p[kept[m + 1]]
            near |= bool(a > b and a - b <= tol * a)
        kept = kept[:m + 1]
    wk = np.zeros_like(p)
    wk[kept] = w[kept]
    c = np.cumsum(wk)
    W = c[-1]
    uw = u * W
    hit = np.nonzero((wk > 0) & (c > uw))[0]
    idx = int(hit[0]) if len(hit) else int(np.nonzero(wk > 0)[0][-1])
    near |= bool(abs(uw - (c[idx] - wk[idx])) <= tol * W or abs(c[idx] - uw) <= tol * W)
    return idx, near


def sample_decode(sd, cfg, batch, N, seed=0, temperature=1.0, top_k=0, top_p=1.0, max_steps=None, early_stop=True,
                  dtype=torch.float64, tol=1e-4):
    """Returns a dict of per-ROW results (row b*N + n): ``tokens`` / ``attach`` int64 [R, steps], ``scores`` [R],
    ``first_end`` [R] (-1 = never), ``near`` bool [R, steps] and ``steps`` (the steps run)."""
    temperature = float(np.float32(temperature))
    top_p = float(np.float32(top_p))
    p = _params(sd, dtype)
    steps = int(max_steps or cfg.max_output_length)
    B = batch["input_value"].shape[0]
    R = B * N
    st = _Stepper(p, cfg, batch, N, steps)
    V, PAD, END = cfg.vocab, cfg.pad, cfg.end
    tokens = torch.zeros(R, steps, dtype=torch.long)
    attach = torch.full((R, steps), -1, dtype=torch.long)
    score = np.zeros(R, dtype=np.float64)
    fe = np.full(R, -1, dtype=np.int64)
    near = np.zeros((R, steps), dtype=bool)
    rb, rn = np.arange(R) // N, np.arange(R) % N
    done = 0
    for t in range(steps):
        dist = st.dist(t)
        if dist.shape[1] > V:
            dist = dist[:, :V + t]                                   # the self pointer j = t is no candidate
        dist = dist.numpy()
        u = sample_u(seed, rb, rn, t)
        for r in range(R):
            if fe[r] >= 0:
                tokens[r, t], attach[r, t] = PAD, -1
                continue
            idx, nr = select(dist[r], float(u[r]), temperature, top_k, top_p, tol)
            near[r, t] = nr
            if idx >= V:
                tokens[r, t], attach[r, t] = tokens[r, idx - V], idx - V
            else:
                tokens[r, t] = idx
            score[r] += math.log(dist[r, idx])
            if int(tokens[r, t]) == END:
                fe[r] = t
        st.feed(tokens[:, t], t)
        done = t + 1
        if early_stop and bool((fe >= 0).all()):
            break
    return {"tokens": tokens, "attach": attach, "scores": torch.from_numpy(score), "first_end": torch.from_numpy(fe),
            "near": torch.from_numpy(near), "steps": done}
