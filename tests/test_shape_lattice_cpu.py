"""The shape lattice (tests/shape_cases.py) without a GPU: the form bits its table states are the ones pa_decode_plan reports - so each case
reaches the step form it is named for - and the three properties of its seeds that tests/test_shape_lattice_gpu.py relies on hold on the
CPU: greedy margins wide enough for a token-exact f32 decode, the float32 yardstick of the f32 log-prob rule under its cap, and the bf16
rounding simulation running at every width."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_logprob_cases as DL                                   # noqa: E402
import large_cases as LC                                            # noqa: E402
import shape_cases as SC                                            # noqa: E402
from test_decode_plan_cpu import PA_BF16, PA_F32, model_cfg         # noqa: E402


def plan_bits(name, dtype):
    from plankassembly_amd import _lib as L
    c = SC.CASES[name]
    case = (PA_BF16 if dtype == "bf16" else PA_F32, c["d"], c["h"], c["ff"], c["nd"], SC.ROWS, SC.S_IN, SC.TMAX)
    info = L.DecodePlanInfo()
    L.check(L.lib().pa_decode_plan(C.byref(model_cfg(case)), *case[5:], C.byref(info)), "pa_decode_plan")
    return [info.fold, info.f32res, info.mq, info.mq_contract, info.mq_self, info.mq_self_bf]


def test_the_table_holds_ten_accepted_shapes_with_ragged_batches():
    assert len(SC.NAMES) == 10 and [c["wseed"] for c in SC.CASES.values()] == list(range(100, 110))
    for name, c in SC.CASES.items():
        assert name == f"d{c['d']}_h{c['h']}_ff{c['ff']}" and c["d"] % c["h"] == 0 and c["d"] // c["h"] in (16, 32, 64)
        assert c["d"] % 8 == 0 and c["ff"] % 8 == 0                 # what pa_model_create accepts
        b, db = LC.case_batch(c), LC.case_batch(c, decode=True)
        assert b["input_value"].shape == db["input_value"].shape == (SC.ROWS, SC.S_IN) and b["output_value"].shape == (SC.ROWS, SC.TMAX)
        assert (~b["input_mask"]).sum(1).tolist() == [29, 17, 33] and (~db["input_mask"]).sum(1).tolist() == [21, 25, 9]      # ragged
    assert {c["d"] // c["h"] for c in SC.CASES.values()} == {16, 32, 64}
    assert set(DL.CASES) >= {SC.LOGPROB_ID + n for n in SC.NAMES}


@pytest.mark.parametrize("name", SC.NAMES)
def test_plan_bits_of_the_table_are_the_librarys(name):
    assert not any(k.startswith("PLANK_DECODE_") for k in os.environ)
    for dtype in ("bf16", "f32"):
        assert plan_bits(name, dtype) == SC.expected_bits(name, dtype) == SC.BITS[(name, dtype)], (name, dtype, plan_bits(name, dtype))


def test_each_case_reaches_the_form_it_is_named_for():
    bits = {k: "".join(map(str, v)) for k, v in SC.BITS.items()}
    for name in ("d512_h16_ff512", "d512_h32_ff1024"):              # folded, K / V caches (no absorbed cross-attention: more than 8 heads)
        assert bits[(name, "bf16")] == "110000" and bits[(name, "f32")] == "100000"
    assert bits[("d512_h8_ff544", "bf16")] == "101000" and bits[("d512_h8_ff544", "f32")] == "101110"      # absorbed, K = 544
    for name in SC.NAMES[3:]:                                       # the generic step
        assert bits[(name, "bf16")] == bits[(name, "f32")] == "000000"


def test_forced_fold_off_d512_is_planned_in_a_child_process():
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PLANK_DECODE_", "PLANK_HIP_LIB"))}
    env.update(SC.FOLD_ENV)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.splitlines()[-1])
    assert got == dict(bits=SC.FOLD_BITS, expected=SC.FOLD_BITS, mode="step_all_bf16"), got


@pytest.mark.parametrize("name", SC.NAMES)
def test_seed_properties(name):
    from oracle import plank_oracle as O
    c = SC.CASES[name]
    sd, cfg, db = LC.case_state_dict(c), LC.case_oracle_cfg(c), LC.case_batch(c, decode=True)
    rows = list(range(SC.ROWS))
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            _, _, marg = O.greedy_decode_cached({k: v.double() for k, v in sd.items()}, cfg, db, early_stop=False, return_margins=True)
    finally:
        torch.set_default_dtype(torch.float32)
    tokens, attach = DL.random_forced(rows, SC.TMAX, SC.FORCED_SEED)
    ref = DL.reference(c, db, rows, tokens, attach)
    own = float((ref["lp32"] - ref["lp"]).abs().max())
    sim = DL.simulated(c, db, rows, tokens, attach, DL.sim_mode(SC.LOGPROB_ID + name))
    mean = float((sim - ref["lp"]).abs().mean())
    print(f"{name}: smallest relative top-2 margin {float(marg.min()):.3e}; float32 yardstick max {own:.3e}; "
          f"simulation {DL.sim_mode(SC.LOGPROB_ID + name)} mean |sim - float64| {mean:.3e} max {float((sim - ref['lp']).abs().max()):.3e}")
    assert marg.shape == (SC.ROWS, SC.TMAX) and float(marg.min()) >= 2.5e-3     # (ten times the t1024 fixture's)
    assert own <= 1e-5 < DL.F32_CPU_FLOAT32_MAX                      # (at most 6.9e-6 here; the last digit is the host BLAS's)
    assert bool(torch.isfinite(sim).all()) and 3e-3 <= mean <= 1e-1                # (9e-3 .. 3e-2 here: a yardstick neither vanishing nor useless)


if __name__ == "__main__":
    print(json.dumps(dict(bits=plan_bits(SC.FOLD_CASE, "bf16"), expected=SC.expected_bits(SC.FOLD_CASE, "bf16"),
                          mode=DL.sim_mode(SC.LOGPROB_ID + SC.FOLD_CASE))))
