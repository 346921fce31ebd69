"""Float64 parity of the assembled model at every kind of shape pa_model_create accepts (tests/shape_cases.py: head dimensions 16, 32
and 64 on and off d_model 512, d_ff below d_model and no multiple of 32, d_model 256 and 1024, odd head counts, nothing a multiple of 16).
The kernel suites hold every kernel to float64 in isolation; this file holds the WIRING - row strides, head splits and the decode step's
choice of form (csrc/decode.hip plan_decode) - at the shapes the rest of the suite never builds.

  train   f32 and x3: the f32 gate of tests/test_headline_gpu.py unchanged (loss / memory / hiddens within 1e-4, every gradient element within
          1e-5 + 1e-4 x scale of the float64 oracle on the device's ReLU branches, at most 256 ties); bf16: the per-tensor rule of
          test_bf16_train_step_per_tensor unchanged.
  decode  every test first asserts that pa_decode_plan reports the case's form bits (shape_cases.BITS).  f32: GreedyDecoder without early stop,
          eager and under graph replay, tokens and attach bit-equal to the float64 oracle's cached greedy decode.  Teacher-forced log p
          (PlankModel.score on random candidates, all 3 rows, 30 steps): f32 under check_f32, bf16 under check_bf16 of
          tests/test_decode_logprob_gpu.py against the rounding simulation of the step form sim_mode gives.
  child   d256_h8_ff512 in bf16 under PLANK_DECODE_FOLD_LN=1 - the forced fold off d_model 512 - in one child process (the switches are
          read once per process), its log p under the same rule.
Measured on MI355X: profiles/shape_lattice_parity.txt."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

import decode_logprob_cases as DL
import large_cases as LC
import shape_cases as SC
import test_decode_logprob_gpu as LP
from test_headline_gpu import _split_stats, bf16_per_tensor_gate, f32_gate, hip_model, oracle_f64, run_hip_train

pytestmark = pytest.mark.gpu

_CACHE = {}          # name: state dict and train batch; (name, "f64"): the float64 oracle's train step; (name, "greedy"): its decode


def weights(name):
    if name not in _CACHE:
        c = SC.CASES[name]
        _CACHE[name] = (c, LC.case_state_dict(c), LC.case_batch(c))
    return _CACHE[name]


def oracle_step(name):
    """The float64 oracle's train step on its own ReLU branches (the bf16 rule's reference), once per case."""
    if (name, "f64") not in _CACHE:
        c, sd, batch = weights(name)
        _CACHE[(name, "f64")] = oracle_f64(c, sd, batch)
    return _CACHE[(name, "f64")]


def assert_plan_bits(m, name, dtype):
    from plankassembly_amd import _lib as L
    info = L.DecodePlanInfo()
    m._ensure_handle()
    L.check(L.lib().pa_decode_plan(C.byref(m._cfg_struct()), SC.ROWS, SC.S_IN, SC.TMAX, C.byref(info)), "pa_decode_plan")
    bits = [info.fold, info.f32res, info.mq, info.mq_contract, info.mq_self, info.mq_self_bf]
    assert bits == SC.expected_bits(name, dtype), (name, dtype, bits, SC.expected_bits(name, dtype))
    return "".join(map(str, bits))


@pytest.mark.parametrize("mode", ["f32", "x3"])
@pytest.mark.parametrize("name", SC.NAMES)
def test_train_step_passes_the_f32_gate(name, mode):
    c, sd, batch = weights(name)
    assert batch["input_value"].shape == (SC.ROWS, SC.S_IN) and batch["output_value"].shape[1] == SC.TMAX
    m = hip_model(c, mode, sd)
    _split_stats(reset=True)
    out, mem, hid, grads = run_hip_train(m, batch)
    taken, declined = _split_stats()
    keep = {}
    fb = f32_gate(f"{name}-{mode}", c, sd, batch, m, out, mem, hid, grads, keep=(keep, 0))
    r64 = keep[0][4]
    worst = max((float((grads[k].double() - r64[k].double()).abs().max()) / (1e-5 + 1e-4 * float(r64[k].abs().max())), k) for k in grads)
    print(f"LATTICE train {name} {mode}: worst gradient error {worst[0]:.3f} x the bound ({worst[1]}); ReLU ties {fb.flips}; "
          f"GEMMs run as bf16x3 {taken}, run exact {declined}")


@pytest.mark.parametrize("name", SC.NAMES)
def test_bf16_train_step_per_tensor(name):
    c, sd, batch = weights(name)
    ref, rgrads = oracle_step(name)
    m = hip_model(c, "bf16", sd)
    out, mem, hid, grads = run_hip_train(m, batch)
    st = bf16_per_tensor_gate(name, batch, ref, rgrads, out, mem, hid, grads)
    big = [r for r in st["rows"] if r[3] > 1e-3]
    print(f"LATTICE train {name} bf16: loss {out['loss'].item():.5f} vs {float(ref['loss']):.5f}; rel-L2 memory {st['r_mem']:.2e} hiddens {st['r_hid']:.2e}; "
          f"tensors above 1e-3 of the norm: worst cosine {min(r[1] for r in big):.5f} rel-L2 {max(r[2] for r in big):.4f}; "
          f"all: worst cosine {min(r[1] for r in st['rows']):.5f} rel-L2 {max(r[2] for r in st['rows']):.4f}")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", SC.NAMES)
def test_f32_greedy_decode_matches_the_oracle(name, graph):
    from oracle import plank_oracle as O
    import plankassembly_amd.decode as D
    c, sd, _ = weights(name)
    db = LC.case_batch(c, decode=True)
    if (name, "greedy") not in _CACHE:
        with torch.no_grad():
            _CACHE[(name, "greedy")] = O.greedy_decode_cached(sd, LC.case_oracle_cfg(c), db, early_stop=False, return_margins=True)
    s_ref, a_ref, marg = _CACHE[(name, "greedy")]
    m = hip_model(c, "f32", sd).eval()
    bits = assert_plan_bits(m, name, "f32")
    m._refresh_shadow()
    dec = D.GreedyDecoder(m, use_graph=graph, strict_graph=graph)
    with torch.no_grad():
        s, a = dec.run(m.prepare_batch(db), early_stop=False)
    s, a = s.cpu(), a.cpu()
    assert (dec._graph is not None) == graph
    assert s.shape == (SC.ROWS, SC.TMAX) == s_ref.shape
    print(f"LATTICE greedy {name} f32 {'graph' if graph else 'eager'}: plan bits {bits}; {int((a_ref >= 0).sum())} pointers, "
          f"{len(set(s_ref.flatten().tolist()))} distinct tokens; smallest relative top-2 margin of the oracle {float(marg.min()):.2e}")
    neq = ((s != s_ref) | (a != a_ref)).nonzero()
    if len(neq):
        r, t = int(neq[0][0]), int(neq[0][1])
        pytest.fail(f"{name}: row {r} step {t}: HIP {int(s[r, t])}/{int(a[r, t])} oracle {int(s_ref[r, t])}/{int(a_ref[r, t])}, oracle margin {float(marg[r, t]):.3e}")


LOGPROB_RUNS = [(name, dtype) for name in SC.NAMES for dtype in ("f32", "bf16")]


@pytest.mark.parametrize("name,dtype", LOGPROB_RUNS, ids=[f"{n}-{d}" for n, d in LOGPROB_RUNS])
def test_forced_logprobs_against_float64(name, dtype):
    cid = SC.LOGPROB_ID + name
    assert LP.SEED == SC.FORCED_SEED and DL.CASES[cid]["rows"] == list(range(SC.ROWS))
    bits = assert_plan_bits(LP.model(cid, dtype), name, dtype)
    print(f"LATTICE logprob {name} {dtype}: plan bits {bits}" + (f"; simulation mode {DL.sim_mode(cid)}" if dtype == "bf16" else ""))
    got = LP.device_score(cid, dtype)
    (LP.check_f32 if dtype == "f32" else LP.check_bf16)(cid, got)


def test_forced_fold_off_d512_in_a_child_process():
    """PLANK_DECODE_FOLD_LN=1: d256_h8_ff512 in bf16 takes the folded step (plan bits 100000), which no default configuration off d_model
    512 reaches.  One child pytest process under its own time limit; it takes the plan bits it must see and its simulation mode from
    its own switches (shape_cases.expected_bits, decode_logprob_cases.sim_mode)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PLANK_DECODE_", "PLANK_HIP_LIB", "PLANK_LOGPROB_"))}
    env.update(SC.FOLD_ENV)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", "-q", "-x", "-s", "tests/test_shape_lattice_gpu.py", "-k",
                        f"test_forced_logprobs_against_float64 and {SC.FOLD_CASE}-bf16"], cwd=root, env=env, capture_output=True, text=True)
    print("\n".join(ln.lstrip(".") for ln in r.stdout.splitlines() if ln.lstrip(".").startswith(("    [", "LATTICE"))))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert re.search(r"(?<![0-9])1 passed", r.stdout) and "skipped" not in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]
    assert f"LATTICE logprob {SC.FOLD_CASE} bf16: plan bits {''.join(map(str, SC.FOLD_BITS))}" in r.stdout, r.stdout[-2000:]
