"""The shape lattice: one small model per (d_model, heads, d_ff) that pa_model_create accepts (head dimension 16, 32 or 64, d_model and
d_ff multiples of 8) and that the three shapes of the rest of the suite - (512, 8, 512 | 1024), (128, 8, 256), (64, 4, 128) - do not
reach, for tests/test_shape_lattice_gpu.py (train step and decode step against float64) and tests/test_shape_lattice_cpu.py (the plan
bits and the properties below, without a GPU).  Cases are large_cases case dicts: case_state_dict, case_batch and case_oracle_cfg take them.

Common to all: 1 encoder and 2 decoder layers, GAINS, S 40 (max_in 41) with ragged lengths [29, 17, 33] in the train batch and
[21, 25, 9] in the decode batch, T 30, B 3, weight seed 100 + i in table order.  What each case is for - the form bits are pa_decode_plan's (fold, f32res, mq,
mq_contract, mq_self, mq_self_bf) at B 3, S 40, Tmax 30, bf16 / f32, derived by hand from csrc/decode.hip plan_decode and asserted by
every decode test before it runs a step:

  d512_h16_ff512     head dim 32 in the folded step at d_model 512: more than 8 heads, so per-layer K / V caches       110000 / 100000
  d512_h32_ff1024    head dim 16, the same                                                                             110000 / 100000
  d512_h8_ff544      the absorbed step with d_ff 544 (K = 544 in the folded skinny GEMM; no f32 residual stream)       101000 / 101110
  d512_h8_ff256      d_ff < d_model: the generic step at d_model 512 with at most 512 rows                             000000 / 000000
  d512_h8_ff520      d_ff no multiple of 32: the same                                                                  000000 / 000000
  d256_h8_ff512      d_model 256, head dim 32; under PLANK_DECODE_FOLD_LN=1 the forced fold off d_model 512 (bf16)     000000 / 000000, 100000
  d256_h4_ff256      head dim 64 off d_model 512                                                                       000000 / 000000
  d1024_h16_ff1024   d_model 1024                                                                                      000000 / 000000
  d48_h3_ff72        head dim 16, an odd head count, nothing a multiple of 16 (3 d = 144, K = 72)                      000000 / 000000
  d96_h3_ff200       head dim 32, an odd head count                                                                    000000 / 000000

Properties of these seeds, evaluated on the CPU by tests/test_shape_lattice_cpu.py (to be re-checked when a seed changes):
  - the smallest relative top-2 margin of the float64 oracle's 30-step greedy decode lies between 2.5e-3 and 3.0e-2 per case (the
    token-exact t1024 fixture of large_cases has 2.1e-4), so the f32 step can be held to the oracle's tokens bit for bit;
  - the CPU's float32 evaluation of the forced log-probabilities (decode_logprob_cases.random_forced(range(3), 30, 2027)) is 6.9e-6
    from float64 per token at the most (asserted below 1e-5: the last digit is the host BLAS's); the f32 rule's cap on that yardstick is 2.5e-5;
  - bf16_decode_sim runs at these widths: mean |simulation - float64| per token between 9e-3 and 3e-2."""
import os

from large_cases import GAINS

COMMON = dict(ne=1, nd=2, gains=GAINS, max_in=41, max_out=30, B=3, bseed=5, lines=(1, 10), planks=(2, 4), with_type=True, decode_b=3, decode_seed=6)
SHAPES = [   # name, d_model, heads, d_ff, form bits bf16, form bits f32
    ("d512_h16_ff512", 512, 16, 512, "110000", "100000"),
    ("d512_h32_ff1024", 512, 32, 1024, "110000", "100000"),
    ("d512_h8_ff544", 512, 8, 544, "101000", "101110"),
    ("d512_h8_ff256", 512, 8, 256, "000000", "000000"),
    ("d512_h8_ff520", 512, 8, 520, "000000", "000000"),
    ("d256_h8_ff512", 256, 8, 512, "000000", "000000"),
    ("d256_h4_ff256", 256, 4, 256, "000000", "000000"),
    ("d1024_h16_ff1024", 1024, 16, 1024, "000000", "000000"),
    ("d48_h3_ff72", 48, 3, 72, "000000", "000000"),
    ("d96_h3_ff200", 96, 3, 200, "000000", "000000"),
]
CASES = {name: dict(COMMON, d=d, h=h, ff=ff, wseed=100 + i) for i, (name, d, h, ff, _, _) in enumerate(SHAPES)}
NAMES = list(CASES)
BITS = {(name, dt): [int(ch) for ch in bits] for name, _, _, _, bf, f32 in SHAPES for dt, bits in (("bf16", bf), ("f32", f32))}
S_IN, TMAX, ROWS = 40, 30, 3
FORCED_SEED = 2027
# the one run under a switch: the forced fold off d_model 512 (plan_decode folds the bf16 step wherever d_model % 64 == 0 when told to)
FOLD_CASE, FOLD_ENV, FOLD_BITS = "d256_h8_ff512", {"PLANK_DECODE_FOLD_LN": "1"}, [1, 0, 0, 0, 0, 0]
LOGPROB_ID = "lattice:"         # decode_logprob_cases.CASES ids of the lattice: LOGPROB_ID + name


def expected_bits(name, dtype):
    """The form bits pa_decode_plan must report for a case in THIS process (the switches are read once per process)."""
    on = {k: v for k, v in os.environ.items() if k.startswith("PLANK_DECODE_")}
    if not on:
        return BITS[(name, dtype)]
    assert on == FOLD_ENV and name == FOLD_CASE and dtype == "bf16", (on, name, dtype)
    return FOLD_BITS


def logprob_cases():
    """The lattice's entries of decode_logprob_cases.CASES: every row of the decode batch is scored, 30 steps."""
    return {LOGPROB_ID + name: dict(case=name, B=ROWS, n=TMAX, rows=list(range(ROWS))) for name in NAMES}
