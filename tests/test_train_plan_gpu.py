"""pa_train_plan (the dry run of the training step's host side, tests/test_train_plan_cpu.py) pinned to the real path, and the real
path pinned to the one before the plan function existed: one forward + backward under the GEMM recorder must make the launches of
tests/golden/train_launches.json - recorded by record() of this file on the commit before - in the same order with the same shapes,
splits, kernels, groups and slab offsets; the weight gradients among them must be, member for member, what pa_train_plan reports;
and the exact-f32 step (ordered reductions: run-to-run bit-identical, confirmed on that commit in two processes) must give the same
loss bits and the same gradient bytes.  So must the bf16x3 step under PA_DETERMINISTIC=1 (its bias, LayerNorm and embedding-table
sums are then ordered too): the commit before the bf16x3 cut plan (tests/test_x3_plan_cpu.py) gave the same bits in two processes,
and those are the x3_* values of the golden file.

The smallest shape with a deferred split-K member in bf16: d_model 128, 2 heads, d_ff 256, 1 encoder and 2 decoder layers, B 4,
S 160 unpadded (640 encoder rows: 10 K tiles of 64, the first count whose cap 10 / 4 is above 1), T 24, dropout 0.1, training mode."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import types

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "train_launches.json")
sys.path.insert(0, REPO)
D, H, FF, N_ENC, N_DEC, B, S, T = 128, 2, 256, 1, 2, 4, 160, 24
DTYPES = ("bf16", "f32", "x3")


def step(dtype):
    """One training step of the test model under the recorder: launches [(M, N, K, batch, splitk, splitk_defer, kind, group, slab
    offset in floats relative to the lowest deferred slab of the recording, or -1), ...], the weight gradients among them, loss bits
    and the digest of the flat gradient, and the model."""
    import torch
    from plankassembly_amd import _lib as L
    from plankassembly_amd.data import SynthSpec, synth_batch
    from plankassembly_amd.models import PlankModel
    torch.manual_seed(0)
    m = PlankModel(D, H, FF, 0.1, "relu", True, N_ENC, N_DEC, 3, 2, 4, 6, S + 1, T, 514, types.SimpleNamespace(END=512, PAD=513),
                   compute_dtype=dtype).cuda().train()
    batch = synth_batch(B, SynthSpec(S + 1, T, (39, 39), (2, 3), True), seed=11)
    batch.pop("name")
    batch["input_value"][batch["input_mask"]] = 7                 # unpadded: every encoder row is a token
    batch["input_mask"][:] = False
    # (prepared as the trainer does: the embedding gradients are then segment sums in token order, not atomic scatter-adds)
    batch = m.prepare_batch({k: v.cuda() for k, v in batch.items()})
    lib = L.lib()
    torch.cuda.synchronize()
    lib.pa_gemm_record(1)
    try:
        out = m(batch)
        out["loss"].backward()
        torch.cuda.synchronize()
    finally:
        n = lib.pa_gemm_record(0)
    kinds, groups, rec = (C.c_int32 * n)(), (C.c_int32 * n)(), (L.GemmArgs * n)()
    assert lib.pa_gemm_recorded_kinds(C.cast(kinds, C.c_void_p), n) == n and lib.pa_gemm_recorded_groups(C.cast(groups, C.c_void_p), n) == n
    assert lib.pa_gemm_recorded(C.cast(rec, C.c_void_p), n) == n
    slabs = [g.ws for g in rec if g.splitk_defer and g.ws]
    base = min(slabs) if slabs else 0
    launches = [[g.M, g.N, g.K, g.batch, g.splitk, g.splitk_defer, kinds[i], groups[i], (g.ws - base) // 4 if g.splitk_defer else -1]
                for i, g in enumerate(rec)]
    # a weight gradient: both operands contracted over their rows, f32 out, unbatched (the pointer head's are batched over B)
    dw = [e for e, g in zip(launches, rec) if not g.a_kcontig and not g.b_kcontig and g.batch == 1 and g.out_dtype == L.PA_F32]
    loss_bits = int(out["loss"].detach().float().view(torch.int32).item())
    digest = hashlib.sha256(m._gflat.detach().cpu().numpy().tobytes()).hexdigest()
    return dict(launches=launches, dw=dw, loss_bits=loss_bits, grad_sha256=digest), m


_STEPS = {}


def stepped(dtype):
    if dtype not in _STEPS:
        _STEPS[dtype] = step(dtype)
    return _STEPS[dtype]


def x3_bits_in_a_child():
    """Loss bits and gradient digest of the x3 step under PA_DETERMINISTIC=1, which is read once per process: this file as a script."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--x3-bits"], env=dict(os.environ, PA_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def record():
    """The golden file's content: run on the commit before (this file copied into its tests/).  The x3 bits come from two child
    processes, which must agree."""
    out = {dt: step(dt)[0] for dt in DTYPES}
    x3 = x3_bits_in_a_child()
    assert x3 == x3_bits_in_a_child(), "the x3 step does not repeat under PA_DETERMINISTIC=1"
    print(json.dumps({"launches": {dt: out[dt]["launches"] for dt in DTYPES}, "f32_loss_bits": out["f32"]["loss_bits"],
                      "f32_grad_sha256": out["f32"]["grad_sha256"], "x3_loss_bits": x3["loss_bits"],
                      "x3_grad_sha256": x3["grad_sha256"]}, separators=(",", ":")))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_step_makes_the_recorded_launches(dtype):
    want = json.load(open(GOLDEN))["launches"][dtype]
    got = stepped(dtype)[0]["launches"]
    assert len(got) == len(want), (len(got), len(want))
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} launches differ, first: {wrong[:4]}"
    if dtype == "bf16":
        assert any(e[5] and e[7] >= 0 for e in got), "no deferred split-K member of a grouped launch at this shape"


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_weight_gradients_are_the_planned_members(dtype):
    from plankassembly_amd import _lib as L
    res, m = stepped(dtype)
    info = L.TrainPlanInfo()
    m._split(True, retain=True)                                   # (x3: the plan is made under the model's own mode)
    try:
        L.check(L.lib().pa_train_plan(C.byref(m._cfg_struct()), B, S, T, B * S, C.byref(info)), "pa_train_plan")
    finally:
        m._split(False)
    assert info.ws_bytes == L.ws_bytes("pa_model_train_ws_bytes", m._handle, B, S, T)
    assert info.n_segments == int(L.lib().pa_model_train_num_segments(m._handle)) == N_ENC + N_DEC + 4
    assert list(info.n_members) == [2, 7, 4]
    plan = []
    for kind in [0] + [1] * N_DEC + [2] * N_ENC:                   # the segments that queue weight gradients, in execution order
        plan += [(p.rows, p.cols, p.k, p.splitk, p.slab) for p in info.member[kind][:info.n_members[kind]]]
    got = res["dw"]
    assert len(got) == len(plan) == 2 + 7 * N_DEC + 4 * N_ENC
    for e, (rows, cols, k, splitk, slab) in zip(got, plan):
        # (x3: a grouped launch records its members as the bf16 GEMMs over 3 K rows they run as)
        assert e[0] == rows and e[1] == cols and e[2] in ((k, 3 * k) if dtype == "x3" else (k,)), (e, rows, cols, k)
        assert e[4] == splitk and e[5] == (splitk > 1) and e[8] == slab, (e, splitk, slab)
    assert any(p[3] > 1 for p in plan)


def test_exact_f32_step_is_bit_identical_to_the_recorded_one():
    gold = json.load(open(GOLDEN))
    res = stepped("f32")[0]
    assert res["loss_bits"] == gold["f32_loss_bits"] and res["grad_sha256"] == gold["f32_grad_sha256"]


def test_x3_step_with_ordered_reductions_is_bit_identical_to_the_recorded_one():
    gold = json.load(open(GOLDEN))
    got = x3_bits_in_a_child()
    assert got["loss_bits"] == gold["x3_loss_bits"] and got["grad_sha256"] == gold["x3_grad_sha256"], (got, gold["x3_loss_bits"])


if __name__ == "__main__":
    if "--x3-bits" in sys.argv:
        res = step("x3")[0]
        print(json.dumps({"loss_bits": res["loss_bits"], "grad_sha256": res["grad_sha256"]}))
    else:
        record()
