"""The kernels csrc/decode.hip itself defines - dec_attn_kernel<T, DH>, the distribution code of the four step tails (row_dist_prepare /
row_dist_visit through dec_row_dist_kernel), dec_split_heads_kernel and dec_embed_kernel - held PER ELEMENT to a float64 reference through
pa_dec_attn, pa_dec_row_dist, pa_dec_split_heads and pa_dec_embed.  tests/dec_step_parity.py holds the case table, the restated dispatch,
the references and the derivation of the bounds; tests/test_dec_step_parity_cpu.py tests that checker on seeded defects.

Every case goes through the C ABI with pointers into guarded buffers (rowops_parity.Guarded through the Run of
tests/test_rowops_float64_gpu.py: outputs pattern-filled, inputs between sentinels and compared bit for bit afterwards) - twice, for the
same bits - and through plankassembly_amd.ops, which must give the C ABI's bits.  Before each launch the host asserts that the last
element the restated dispatch lets the kernel touch (clamped rows included) lies inside the operand's window.  None of these kernels reads
a switch, so there are no child processes.

With DEC_STEP_PARITY_REPORT=<file> every case appends `kernel case r(got) r_cpu32` (the figures of profiles/dec_step_float64_parity.txt).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dec_step_parity as dp                                        # noqa: E402
from test_rowops_float64_gpu import Run, call, _FAULTED             # noqa: E402,F401  (the guarded-buffer runner and its first-fault memory)

pytestmark = pytest.mark.gpu

ATTN, DIST, EMBED, SPLIT = dp.attn_cases(), dp.dist_cases(), dp.embed_cases(), dp.split_cases()
I32, I64, F32, BF16 = torch.int32, torch.int64, torch.float32, torch.bfloat16
ids = lambda cs: [c["name"] for c in cs]


def _L():
    from plankassembly_amd import _lib as L
    return L


def _report(kernel, c, r, r_cpu):
    fig = f"{r:.4g} {r_cpu:.4g}" if r is not None else "exact exact"
    print(f"{kernel} {c['name']} r(got) r_cpu32 = {fig}")
    path = os.environ.get("DEC_STEP_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(f"{kernel} {c['name']} {fig}\n")


def _inside(c, r, alias=None):
    """Every operand's last touched element (dec_step_parity.extents) lies inside its window."""
    for key, hi in dp.extents(c).items():
        g = r.g[(alias or {}).get(key, key)]
        assert 0 < hi <= g.rows * g.ld, f"{c['name']}: the launch would touch element {hi - 1} of {key}, whose window has {g.rows * g.ld}"


def _win(r, key):
    return r.g[key].view(r.dev[key])


def _f32(x):
    return x.to(torch.float32).numpy()


def _bits(x):
    return x.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[x.element_size()])


def _same(name, what, a, b):
    assert torch.equal(_bits(a), _bits(b)), f"{name}: {what} ({int((_bits(a) != _bits(b)).sum())} element(s) differ)"


# ------------------------------------------------------------------------------------------------ attention
def _attn_args(c, t, r, out, q, newkv, t_dev):
    kpm = r.p("kpm") if "kpm" in r.g else None
    cu = r.p("cu") if "cu" in r.g else None
    return (out, q, c["ldq"], r.p("kc"), r.p("vc"), c["Lmax"], kpm, c.get("fixed_lk", 0), t_dev, t.B, c["H"], t.d, dp.PADT[c["dt"]], cu, newkv, c["G"])


def _attn_ops(c, t, r, qkey, newkey, t_dev):
    from plankassembly_amd import ops
    shape = (t.nb, c["H"], c["Lmax"], c["dh"])
    return ops.dec_attn(_win(r, qkey), _win(r, "kc").view(shape), _win(r, "vc").view(shape), H=c["H"], d=t.d,
                        kpm=_win(r, "kpm") if "kpm" in r.g else None, fixed_lk=c.get("fixed_lk", 0), t_dev=t_dev,
                        cu=_win(r, "cu").view(-1) if "cu" in r.g else None, newkv=_win(r, newkey) if newkey else None, group=c["G"])


def _attn_setup(c, t):
    dt = dp.DT[c["dt"]]
    r = Run(c)
    rows = t.nb * c["H"] * c["Lmax"]
    r.out("kc", (rows, c["dh"]), dt, init=t.kc0)
    r.out("vc", (rows, c["dh"]), dt, init=t.vc0)
    r.inp("kpm", t.kpm)
    r.inp("cu", t.cu)
    return r, dt


def _caches(r, t, c):
    shape = (t.nb, c["H"], c["Lmax"], c["dh"])
    return _f32(r.now("kc")).reshape(shape), _f32(r.now("vc")).reshape(shape)


@pytest.mark.parametrize("c", [c for c in ATTN if not c["steps"]], ids=ids([c for c in ATTN if not c["steps"]]))
def test_attn_case(c):
    ok, plan = dp.on_edge(c)
    assert ok, f"{c['name']}: meant for {c['edge']}, dispatched as {plan}"
    L = _L(); lib = L.lib(); st = L.stream()
    t = dp.AttnTensors(c)
    ref, cpu = dp.attn_reference(c, t), dp.attn_cpu32(c, t)
    r, dt = _attn_setup(c, t)
    self_ = c["form"] == "self"
    if self_:
        r.inp("newkv", t.newkv.to(dt))
        r.inp("t_dev", torch.tensor([c["lens"][0] - 1], dtype=I32))
        q = newkv = r.p("newkv")
        t_dev = r.p("t_dev")
    else:
        q, newkv, t_dev = r.inp("q", t.q.reshape(t.B, t.d).to(dt)), None, None
    out = r.out("out", (t.B, t.d), dt)
    qkey = "newkv" if self_ else "q"
    assert all(r.aligned16(k) for k in (qkey, "kc", "vc", "out"))
    _inside(c, r, {"q": qkey})
    call("pa_dec_attn", lib.pa_dec_attn(*_attn_args(c, t, r, out, q, newkv, t_dev), st))
    first, kc1, vc1 = r.now("out"), r.now("kc"), r.now("vc")
    call("pa_dec_attn", lib.pa_dec_attn(*_attn_args(c, t, r, out, q, newkv, t_dev), st))
    _same(c["name"], "two launches differ in out", first, r.now("out"))
    _same(c["name"], "two launches differ in the K cache", kc1, r.now("kc"))
    _same(c["name"], "two launches differ in the V cache", vc1, r.now("vc"))
    viaops = _attn_ops(c, t, r, qkey, "newkv" if self_ else None, _win(r, "t_dev").view(-1) if self_ else None)
    r.sync()
    _same(c["name"], "plankassembly_amd.ops and the C ABI differ", viaops.cpu(), first.reshape(t.B, t.d))
    kc, vc = _caches(r, t, c)
    w = r.finish()                                                  # the guards of out / kc / vc; q or newkv, kpm, cu, t_dev bit for bit as before
    rr, r_cpu = dp.attn_judge(c, t, w["out"].to(torch.float64).numpy(), kc, vc, ref, cpu)
    _report("attn", c, rr, r_cpu)


@pytest.mark.parametrize("c", [c for c in ATTN if c["steps"]], ids=ids([c for c in ATTN if c["steps"]]))
def test_attn_chain(c):
    """t = 0 .. 9 on pattern-filled caches, t_dev advanced on the device: every step meets the reference built from the newkv rows alone."""
    L = _L(); lib = L.lib(); st = L.stream()
    t = dp.AttnTensors(c)
    r, dt = _attn_setup(c, t)
    cells = torch.zeros(64, dtype=I32, device="cuda")
    t_dev = cells[32:33]
    caches = (t.kc0.numpy().copy(), t.vc0.numpy().copy())
    worst = (0.0, 0.0)
    for step in range(c["steps"]):
        ref = dp.attn_reference(c, t, step)
        cpu = dp.attn_cpu32(c, t, step=step, caches=caches)
        key = f"newkv{step}"
        nk = r.inp(key, t.new_steps[step].to(dt))
        out = r.out(f"out{step}", (t.B, t.d), dt)
        assert int(t_dev.item()) == step and (step + 1) <= c["Lmax"]
        _inside(dict(c, lens=[step + 1] * t.B), r, {"q": key, "newkv": key, "out": f"out{step}"})
        args = (out, nk, c["ldq"], r.p("kc"), r.p("vc"), c["Lmax"], None, 0, C.c_void_p(t_dev.data_ptr()), t.B, c["H"], t.d, dp.PADT[c["dt"]], None, nk, 1)
        call("pa_dec_attn", lib.pa_dec_attn(*args, st))
        first = r.now(f"out{step}")
        call("pa_dec_attn", lib.pa_dec_attn(*args, st))
        _same(c["name"], f"step {step}: two launches differ", first, r.now(f"out{step}"))
        viaops = _attn_ops(c, t, r, key, key, t_dev)
        r.sync()
        _same(c["name"], f"step {step}: plankassembly_amd.ops and the C ABI differ", viaops.cpu(), first.reshape(t.B, t.d))
        kc, vc = _caches(r, t, c)
        rr = dp.attn_judge(c, t, first.to(torch.float64).numpy().reshape(t.B, t.d), kc, vc, ref, cpu, step)
        worst = (max(worst[0], rr[0]), max(worst[1], rr[1]))
        t_dev.add_(1)                                               # on the device, as dec_advance_kernel does in the step
    r.finish()
    assert cells.cpu().tolist() == [0] * 32 + [c["steps"]] + [0] * 31
    _report("attn", c, *worst)


def test_attn_refusals_return_before_any_launch():
    L = _L(); lib = L.lib(); st = L.stream()
    for c, status in dp.attn_rejections():
        dt = dp.DT[c["dt"]]
        r = Run(c)
        q = r.inp("q", torch.zeros(4, 256, dtype=dt))               # (room for every shape the calls claim)
        kc, vc = r.out("kc", (64, 128), dt), r.out("vc", (64, 128), dt)
        td = r.inp("t_dev", torch.tensor([3], dtype=I32))
        kpm, cu = r.inp("kpm", torch.zeros(2, 16, dtype=torch.uint8)), r.inp("cu", torch.tensor([0, 4, 8], dtype=I32))
        out = r.out("out", (4, 256), dt)
        ptr = {"out": out, "q": q, "kc": kc, "vc": vc, "t_dev": td, "newkv": q if c["form"] == "self" else None}
        if c.get("null"):
            ptr[c["null"]] = None
        if c.get("misalign"):
            ptr[c["misalign"]] = C.c_void_p(ptr[c["misalign"]].value + 8)
        B = c.get("rows", c["Bd"] * max(c["G"], 1))
        rc = lib.pa_dec_attn(ptr["out"], ptr["q"], c["ldq"], ptr["kc"], ptr["vc"], c["Lmax"], kpm if c.get("with_kpm") else None, c.get("fixed_lk", 0),
                             ptr["t_dev"], B, c["H"], c["H"] * c["dh"], dp.PADT[c["dt"]], cu if c.get("with_cu") else None, ptr["newkv"], c["G"], st)
        call(c["name"], rc, status)
        w = r.finish()
        for key in ("out", "kc", "vc"):
            assert bool((w[key] == torch.full((1,), dp.PATTERN, dtype=dt)).all()), f"{c['name']}: {key} of a refused launch was written"


# ------------------------------------------------------------------------------------------------ the distribution
@pytest.mark.parametrize("c", DIST, ids=ids(DIST))
def test_dist_case(c):
    ok, plan = dp.on_edge(c)
    assert ok, f"{c['name']}: meant for {c['edge']}, dispatched as {plan}"
    from plankassembly_amd import ops
    L = _L(); lib = L.lib(); st = L.stream()
    t = dp.DistTensors(c)
    ref, cpu = dp.dist_reference(c, t), dp.dist_cpu32(c, t)
    dt = dp.DT[c["dt"]]
    rows, d, V, Tmax = c["rows"], c["d"], c["V"], c["Tmax"]
    r = Run(c)
    vlog, pfeat, h = r.inp("vlog", t.vlog), r.inp("pfeat", t.pfeat.to(dt)), r.inp("h", t.h.to(dt))
    sw_w, sw_b, td = r.inp("sw_w", t.sw_w), r.inp("sw_b", t.sw_b), r.inp("t_dev", torch.tensor([c["t"]], dtype=I32))
    cache = r.out("cache", (Tmax * rows, d), dt, init=t.cache0)
    p, stats = r.out("p", (rows, V + Tmax), F32), r.out("stats", (rows, 5), F32)
    assert all(r.aligned16(k) for k in ("pfeat", "h", "cache", "sw_w"))
    _inside(c, r)
    args = (p, stats, vlog, c["ldv"], pfeat, h, cache, sw_w, sw_b, td, rows, Tmax, d, V, dp.PADT[c["dt"]], st)
    call("pa_dec_row_dist", lib.pa_dec_row_dist(*args))
    p1, s1, c1 = r.now("p"), r.now("stats"), r.now("cache")
    call("pa_dec_row_dist", lib.pa_dec_row_dist(*args))
    _same(c["name"], "two launches differ in p", p1, r.now("p"))
    _same(c["name"], "two launches differ in the statistics", s1, r.now("stats"))
    _same(c["name"], "two launches differ in the cache", c1, r.now("cache"))
    po, so = ops.dec_row_dist(_win(r, "vlog"), V, _win(r, "pfeat"), _win(r, "h"), _win(r, "cache").view(Tmax, rows, d), _win(r, "sw_w").view(-1),
                              _win(r, "sw_b").view(-1), _win(r, "t_dev").view(-1), fill=dp.PATTERN)
    r.sync()
    _same(c["name"], "plankassembly_amd.ops and the C ABI differ in p", po.cpu(), p1)
    _same(c["name"], "plankassembly_amd.ops and the C ABI differ in the statistics", so.cpu(), s1)
    w = r.finish()
    got = w["p"].numpy().copy()
    got[got == np.float32(dp.PATTERN)] = np.nan                     # (no p is -123.5: what still holds the pattern was not written)
    rr, r_cpu = dp.dist_judge(c, t, got, w["stats"].numpy(), _f32(w["cache"]).reshape(Tmax, rows, d), ref, cpu)
    _report("dist", c, rr, r_cpu)


# ------------------------------------------------------------------------------------------------ the copies
@pytest.mark.parametrize("c", EMBED, ids=ids(EMBED))
def test_embed_case(c):
    ok, plan = dp.on_edge(c)
    assert ok, f"{c['name']}: meant for {c['edge']}, dispatched as {plan}"
    from plankassembly_amd import ops
    L = _L(); lib = L.lib(); st = L.stream()
    t = dp.EmbedTensors(c)
    dt = dp.DT[c["dt"]]
    r = Run(c)
    value, coord, pos = r.inp("value", t.value), r.inp("coord", t.coord), r.inp("pos", t.pos)
    tokens, td = r.inp("tokens", t.tokens), r.inp("t_dev", torch.tensor([c["t"]], dtype=I32))
    x = r.out("x", (c["B"], c["d"]), dt)
    x_lp = r.out("x_lp", (c["B"], c["d"]), BF16) if c["lp"] else None
    _inside(c, r)
    assert int(t.tokens.max()) < c["nval"] and int(t.tokens.min()) >= 0
    args = (x, x_lp, value, coord, pos, tokens, c["Tmax"], td, c["B"], c["d"], c["dof"], dp.PADT[c["dt"]], st)
    call("pa_dec_embed", lib.pa_dec_embed(*args))
    first = r.now("x")
    call("pa_dec_embed", lib.pa_dec_embed(*args))
    _same(c["name"], "two launches differ", first, r.now("x"))
    res = ops.dec_embed(_win(r, "value"), _win(r, "coord"), _win(r, "pos"), _win(r, "tokens"), _win(r, "t_dev").view(-1), c["dof"], dtype=dt,
                        low_precision_copy=bool(c["lp"]))
    r.sync()
    w = r.finish()
    want_x, want_lp = dp.embed_want(c, t)
    dp.same_bits(c["name"], "x against (value + coord) + pos in float32", _f32(w["x"]), want_x)
    _same(c["name"], "plankassembly_amd.ops and the C ABI differ", (res[0] if c["lp"] else res).cpu(), w["x"])
    if c["lp"]:
        dp.same_bits(c["name"], "the bf16 copy against one RNE of the float32 row", _f32(w["x_lp"]), want_lp)
        _same(c["name"], "plankassembly_amd.ops and the C ABI differ in the bf16 copy", res[1].cpu(), w["x_lp"])
    if c["t"] == 0:
        assert not np.signbit(_f32(w["x"])).any() and not (_f32(w["x"]) != 0).any()
    _report("embed", c, None, None)


@pytest.mark.parametrize("c", SPLIT, ids=ids(SPLIT))
def test_split_heads_case(c):
    ok, plan = dp.on_edge(c)
    assert ok, f"{c['name']}: meant for {c['edge']}, dispatched as {plan}"
    from plankassembly_amd import ops
    L = _L(); lib = L.lib(); st = L.stream()
    t = dp.SplitTensors(c)
    dt = dp.DT[c["dt"]]
    B, H, S, d = c["B"], c["H"], c["S"], c["d"]
    r = Run(c)
    kv, cu, rowmap = r.inp("kv", t.kv.to(dt)), r.inp("cu", t.cu), r.inp("rowmap", t.rowmap)
    kc, vc = r.out("kc", (B * H * S, d // H), dt), r.out("vc", (B * H * S, d // H), dt)
    _inside(c, r)
    if t.rowmap is not None:                                        # every destination the index arithmetic reaches lies inside the window
        s_ = np.arange(t.rows) - t.cu.numpy()[t.rowmap.numpy() // S]
        assert (s_ >= 0).all() and (s_ < S).all() and (t.rowmap.numpy() // S < B).all()
    args = (kc, vc, kv, C.c_int64(t.rows), S, d, H, dp.PADT[c["dt"]], cu, rowmap, st)
    call("pa_dec_split_heads", lib.pa_dec_split_heads(*args))
    k1 = r.now("kc")
    call("pa_dec_split_heads", lib.pa_dec_split_heads(*args))
    _same(c["name"], "two launches differ", k1, r.now("kc"))
    ko, vo = ops.dec_split_heads(_win(r, "kv"), B, S, H, cu=_win(r, "cu").view(-1) if t.cu is not None else None,
                                 rowmap=_win(r, "rowmap").view(-1) if t.rowmap is not None else None)
    r.sync()
    w = r.finish()
    wk, wv = dp.split_want(c, t)
    shape = (B, H, S, d // H)
    dp.same_bits(c["name"], "K against index arithmetic", _f32(w["kc"]).reshape(shape), wk)
    dp.same_bits(c["name"], "V against index arithmetic", _f32(w["vc"]).reshape(shape), wv)
    mapped = torch.from_numpy(wk != np.float32(dp.PATTERN))
    _same(c["name"], "plankassembly_amd.ops and the C ABI differ in K", ko.cpu()[mapped], w["kc"].reshape(shape)[mapped])
    _same(c["name"], "plankassembly_amd.ops and the C ABI differ in V", vo.cpu()[mapped], w["vc"].reshape(shape)[mapped])
    _report("split", c, None, None)
