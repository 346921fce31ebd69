"""Teacher-forced sequences and CPU references for the log-probability parity tests of the decode step
(tests/test_decode_logprob_cpu.py, tests/test_decode_logprob_gpu.py).

With every position forced (PlankModel.score) the step cannot leave the reference's sequence, so its per-token log p can be compared
with a float64 evaluation at any length.  The forced candidates are RANDOM, not the arg-max: vocabulary entries, pointers to near
and far positions and the 1e-6 fill are all probed, at every cache length."""
from __future__ import annotations

import os

import numpy as np
import torch

import bf16_decode_sim as SIM
import large_cases as LC
import prefix_reference as PR
import shape_cases as SC
from oracle import plank_oracle as O

N_VOCAB_FORCED = 512          # forced vocabulary tokens are drawn from [0, 512): never END (512) / PAD (513)
STEP_RANGES = ((0, 6), (6, 128), (128, 512), (512, 1024))
SMALL = dict(d_model=64, n_head=4, d_ff=128, n_enc=2, n_dec=2, max_input_length=65, max_output_length=36)

# The GPU cases (tests/test_decode_logprob_gpu.py): large_cases case, device batch, steps, rows scored on the CPU.
TWO_ROWS = os.environ.get("PLANK_LOGPROB_TWO_ROWS") == "1"         # the child runs of case A score two rows
CASES = {
    "A": dict(case="headline", B=16, n=128, rows=[0, 15] if TWO_ROWS else [0, 5, 10, 15]),
    "B": dict(case="headline", B=40, n=128, rows=[0, 13, 26, 39]),
    "C": dict(case="headline", B=256, n=128, rows=[0, 1, 31, 63, 64, 100, 127, 128, 129, 160, 191, 192, 200, 223, 254, 255]),
    "D": dict(case="t1024", B=4, n=1024, rows=[0, 3]),
    "E": dict(case="sideface", B=520, n=128, rows=[0, 173, 346, 519]),
    "F": dict(case="small", B=4, n=36, rows=[0, 1, 2, 3]),
}
CASES.update(SC.logprob_cases())                                   # the shape lattice (tests/test_shape_lattice_gpu.py): all 3 rows, 30 steps
_ALLOWED = (O.pointer_mask(O.OracleCfg(), 1024) != 0).numpy()      # the oracle's eval pointer mask [t][j] (pinned by the golden tests)


def pointer_allowed(t, j):
    return bool(_ALLOWED[t, j])


def case_dict(cid):
    name = CASES[cid]["case"]
    if name == "small":
        from conftest import load_fixture
        sd, batch, _ = load_fixture("fixture_small.npz")
        return dict(sd=sd, cfg=O.OracleCfg(**SMALL), batch=batch, d=64, ff=128)
    c = LC.CASES[name] if name in LC.CASES else SC.CASES[name]      # (names large_cases does not know: the shape lattice)
    return dict(c, decode_seed=10) if name == "sideface" else c      # (sideface has no decode batch of its own)


def _env_int(name, default):
    v = os.environ.get(name)
    return default if v is None else int(v)


def sim_mode(cid):
    """The simulation mode of the bf16 step form csrc/decode.hip decode_modes() selects for this case in this process: `f32res` at
    d_model 512 and at most 512 rows unless PLANK_DECODE_F32_RESID=0 or the LayerNorm fold is forced off.  (decode_modes() also asks
    for at most 512 output tiles, ceil(B / 64) * ceil(3 d / 64): 24 * 8 = 192 at d 512, B 512 - it cannot bind where the rest holds.)"""
    c, B = case_dict(cid), CASES[cid]["B"]
    d, ff = c["d"], c["ff"]
    fold_force = _env_int("PLANK_DECODE_FOLD_LN", -1)
    fold = (fold_force != 0 if fold_force >= 0 else (d == 512 and B <= 512)) and d % 64 == 0 and ff % 32 == 0 and ff >= d
    f32res = fold and _env_int("PLANK_DECODE_F32_RESID", 1) != 0 and d == 512 and B <= 512 and ff % 512 == 0
    return "step_f32res" if f32res else "step_all_bf16"


def fill_positions(r, n):
    """The two positions of row r that carry a pointer the eval mask disallows (both >= 12, distinct for n >= 24)."""
    assert n >= 24
    return 12 + r % 7, n - 1 - r % 5


def random_forced(rows, n, seed):
    """tokens, attach int64 [len(rows), n].  Row r depends on (seed, r) only.  Per step: where the eval pointer mask allows an earlier
    position, with probability 1/2 a pointer uniformly among the allowed j < t (token = the row's own token at j), otherwise a
    vocabulary token uniform in [0, 512); at fill_positions(r, n) a pointer uniformly among the DISALLOWED j < t (the 1e-6 fill)."""
    tokens = torch.zeros(len(rows), n, dtype=torch.long)
    attach = torch.full((len(rows), n), -1, dtype=torch.long)
    for i, r in enumerate(rows):
        rng = np.random.default_rng([int(seed), int(r)])
        fills = fill_positions(int(r), n)
        for t in range(n):
            ok = [j for j in range(t) if pointer_allowed(t, j)]
            coin, pick, voc = rng.random(), rng.random(), int(rng.integers(0, N_VOCAB_FORCED))     # the same draws at every step
            if t in fills:
                bad = [j for j in range(t) if not pointer_allowed(t, j)]
                j = bad[int(pick * len(bad))]
            elif ok and coin < 0.5:
                j = ok[int(pick * len(ok))]
            else:
                tokens[i, t] = voc
                continue
            tokens[i, t], attach[i, t] = tokens[i, j], j
    return tokens, attach


def sd_cfg(case):
    """(state_dict, OracleCfg) of a large_cases case dict, or of dict(sd=..., cfg=...) (the small fixture)."""
    if "sd" in case:
        return case["sd"], case["cfg"]
    return LC.case_state_dict(case), LC.case_oracle_cfg(case)


def sub_batch(batch, rows):
    return {k: v[list(rows)] for k, v in batch.items()}


def reference(case, batch, rows, tokens, attach, f32_rows=None):
    """float64 lp [len(rows), n] of the forced candidates (prefix_reference.score on the sub-batch of `rows`; all finite, asserted),
    and the same in float32 - the yardstick of the f32 bounds - on the first `f32_rows` of them (default: all, so that the largest
    cumulative deviation of the device and of the yardstick are taken over the same row set):
    {"lp": ..., "lp32": [f32_rows, n], "rows32": positions in `rows`}."""
    sd, cfg = sd_cfg(case)
    n = tokens.shape[1]
    with torch.no_grad():
        _, lp = PR.score(sd, cfg, sub_batch(batch, rows), tokens, attach, torch.full((len(rows),), n))
        assert lp.dtype == torch.float64 and bool(torch.isfinite(lp).all()), "a forced position is no candidate"
        k = list(range(len(rows) if f32_rows is None else min(f32_rows, len(rows))))
        _, lp32 = PR.score(sd, cfg, sub_batch(batch, [rows[i] for i in k]), tokens[k], attach[k], torch.full((len(k),), n),
                           dtype=torch.float32)
    return {"lp": lp, "lp32": lp32, "rows32": k}


def simulated(case, batch, rows, tokens, attach, mode):
    """float64 lp [len(rows), n] of the forced candidates under the bf16 rounding simulation (bf16_decode_sim.run, mode `mode`)."""
    sd, cfg = sd_cfg(case)
    with torch.no_grad():
        _, _, lp = SIM.run(sd, cfg, sub_batch(batch, rows), mode, tokens.shape[1], forced=(tokens, attach))
    return lp


def range_stats(diff):
    """diff float64 [R, n] -> {"all" | (lo, hi): (max |.|, mean |.|, signed mean, count)} over all steps and over each of
    STEP_RANGES (empty ranges left out)."""
    n = diff.shape[1]
    out = {}
    for key, lo, hi in [("all", 0, n)] + [((lo, hi), lo, hi) for lo, hi in STEP_RANGES]:
        d = diff[:, lo:min(hi, n)]
        if d.numel():
            out[key] = (float(d.abs().max()), float(d.abs().mean()), float(d.mean()), d.numel())
    return out


F32_TOKEN_BOUND = 1e-4        # the project's parity bound (README): never raised
F32_CPU_FLOAT32_MAX = 2.5e-5  # what the CPU's own float32 evaluation may deviate from float64 per token: the bound keeps a margin of 4
F32_CUM_FACTOR = 15.0         # cumulative per row: this many times the CPU float32 evaluation's cumulative deviation


def f32_per_token_failures(lp, lp64):
    """Positions [k, 2] (row, step) where an f32 evaluation misses the per-token bound: non-finite on either side, or further than
    F32_TOKEN_BOUND from float64.  Empty = the bound holds on every token."""
    lp, lp64 = lp.double(), lp64.double()
    bad = ~torch.isfinite(lp) | ~torch.isfinite(lp64) | ~((lp - lp64).abs() <= F32_TOKEN_BOUND)
    return bad.nonzero()
