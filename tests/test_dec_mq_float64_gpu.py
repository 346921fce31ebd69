"""The absorbed decode attention of csrc/decode_mq.h - dec_cross_mq_kernel (bf16), dec_cross_mq32_kernel and dec_cross_mq32w8_kernel (f32) -
held PER ELEMENT to a float64 reference through every pa_dec_*_mq* entry of include/plank_hip.h: dense, key-padding mask, packed rows, the
self form with its device-read key count, range blocks (forced, by rule, with a scratch that is too small, misaligned or missing), decode
groups with one and two rows per block.  tests/dec_mq_parity.py holds the case table, the restated dispatch, the reference and the
derivation of the bounds; tests/test_dec_mq_parity_cpu.py tests that checker on seeded defects.

Every case goes through the C ABI with pointers into guarded buffers (rowops_parity.Guarded through the Run of
tests/test_rowops_float64_gpu.py) - twice, for the same bits - and through plankassembly_amd.ops, which must give the C ABI's bits.  The
range-block scratch is filled before every launch (tickets zero, partials NaN) and checked after it (tickets zero again, nothing behind it
written, and nothing in it at all where the launch falls back to one block).

The switches are read once per process, so each bundle of dec_mq_parity.BUNDLES runs this file as a script in a fresh child process, one
after the other, on the cases whose restated dispatch it changes; the parent stops at the first child that fails.

With DEC_MQ_PARITY_REPORT=<file> every case appends `kernel case bundle r(got) r_emu` (the figures of profiles/dec_mq_float64_parity.txt).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dec_mq_parity as dp                                          # noqa: E402
from test_rowops_float64_gpu import Run, call, _FAULTED             # noqa: E402  (the guarded-buffer runner and its first-fault memory)

pytestmark = pytest.mark.gpu

BUNDLE = os.environ.get("DEC_MQ_PARITY_BUNDLE", "")                 # set in a bundle's child process only
ENV = {k: os.environ[k] for k in dp.SWITCHES if k in os.environ}    # the switches of this process, as the library reads them
ALL = dp.cases()
CASES = [c for c in ALL if dp.dispatch(c, ENV) != dp.dispatch(c)] if BUNDLE else ALL
_CHILD_FAILED = []
WS_GUARD = 256
I32 = torch.int32


def _L():
    from plankassembly_amd import _lib as L
    return L


class Scratch:
    """The range-block scratch of a case: `need` bytes (256-byte aligned; 16 bytes further on for the misaligned case) and a guard."""

    def __init__(self, p):
        self.p, self.need = p, p["ws_need"]
        self.off = 16 if p["ws"] == "misaligned" else 0
        self.buf = torch.empty(self.off + self.need + WS_GUARD, dtype=torch.uint8, device="cuda") if p["ws"] else None
        if self.buf is not None:
            assert self.buf.data_ptr() % 256 == 0
        self.tick = dp.tick_bytes(p["units"])

    def view(self):
        """What the library is given: the tensor of `ws_bytes` bytes (None without scratch)."""
        return None if self.buf is None else self.buf[self.off:self.off + self.p["ws_bytes"]]

    def fill(self):
        if self.buf is not None:
            self.buf.fill_(0xFF)                                    # partials (and the guard): NaN
            self.buf[self.off:self.off + self.tick] = 0             # tickets

    def check(self, name):
        if self.buf is None:
            return
        h = self.buf.cpu()
        tick, rest = h[self.off:self.off + self.tick], h[self.off + self.tick:]
        assert int(tick.to(torch.int64).sum()) == 0, f"{name}: a ticket word is not zero after the launch"
        assert bool((h[:self.off] == 0xFF).all()) and bool((rest[self.need - self.tick:] == 0xFF).all()), f"{name}: bytes around the scratch were written"
        if self.p["nparts"] == 1:
            assert bool((rest == 0xFF).all()), f"{name}: a launch that fell back to one block wrote into the scratch"


def _launch(lib, L, c, p, r, ctx, sc, entry=None):
    """One launch of the case through the C ABI, into the guarded window `ctx`."""
    f32 = c["dt"] == "f32"
    entry = entry or c["entry"]
    B, G, H, S = c["B"], c["G"], c["H"], c["S"]
    qt, mem = r.p("qt"), r.p("mem")
    kpm = r.p("kpm") if "kpm" in r.g else None
    cu = r.p("cu") if "cu" in r.g else None
    ws = sc.view()
    wp, wb = (C.c_void_p(ws.data_ptr()) if ws is not None else None), C.c_int64(ws.numel() if ws is not None else 0)
    st = L.stream()
    sc.fill()
    if entry == "plain":
        name = "pa_dec_cross_mq32" if f32 else "pa_dec_cross_mq"
        rc = getattr(lib, name)(ctx, qt, mem, kpm, cu, B, S, H, dp.D, st)
    elif entry == "ws":
        name = "pa_dec_cross_mq32_ws" if f32 else "pa_dec_cross_mq_ws"
        rc = getattr(lib, name)(ctx, qt, mem, kpm, cu, B, S, H, dp.D, wp, wb, st)
    elif entry == "group":
        name = "pa_dec_cross_mq32_group" if f32 else "pa_dec_cross_mq_group"
        rc = getattr(lib, name)(ctx, qt, mem, kpm, cu, B, G, S, H, dp.D, c["rpb"], c["nparts"], wp, wb, st)
    elif entry == "self_ws":
        name = "pa_dec_self_mq_ws"
        rc = lib.pa_dec_self_mq_ws(ctx, qt, mem, r.p("t_dev"), B, S, H, dp.D, dp.PADT[c["dt"]], c["nparts"], wp, wb, st)
    else:
        name = "pa_dec_self_mq32"
        rc = lib.pa_dec_self_mq32(ctx, qt, mem, r.p("t_dev"), B, S, H, dp.D, st)
    call(name, rc)
    r.sync()
    sc.check(f"{c['name']}: {name}")


def _ops_launch(c, r, sc):
    """The same launch through plankassembly_amd.ops, on views of the guarded buffers; ctx is ops' own allocation."""
    from plankassembly_amd import ops
    B, G, H, S = c["B"], c["G"], c["H"], c["S"]
    win = lambda key: r.g[key].view(r.dev[key])
    qt = win("qt").view(B * G, H, dp.D)
    mem = win("mem")[:win("mem").shape[0] - dp.NTAIL]
    kpm = win("kpm").view(B, S) if "kpm" in r.g else None
    cu = win("cu").view(-1) if "cu" in r.g else None
    if c["form"] != "packed":
        mem = mem.view(B, S, dp.D)
    ws = sc.view()
    sc.fill()
    if c["entry"] == "self_ws":
        out = ops.dec_self_mq(qt, mem, win("t_dev").view(-1), nparts=c["nparts"], ws=ws)
    elif c["entry"] == "group":
        out = ops.dec_cross_mq_group(qt, mem, G, kpm=kpm, cu=cu, S=S, rows_per_block=c["rpb"], nparts=c["nparts"], ws=ws)
    else:
        if c["entry"] == "ws":
            assert (ws is None) == (int(_L().lib().pa_dec_cross_mq_ws_bytes(B, S)) == 0) and (c["ws"] != "ok" or ops.dec_cross_mq_ws(B, S, "cuda").numel() == ws.numel())
        out = ops.dec_cross_mq(qt, mem, kpm=kpm, cu=cu, S=S, ws=ws)
    r.sync()
    sc.check(f"{c['name']}: ops")
    return out.reshape(-1, dp.D).cpu()


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def run_case(c):
    """One case on the device: (r(got), r(emulation))."""
    L = _L(); lib = L.lib()
    p = dp.dispatch(c, ENV)
    assert p["status"] == 0
    t = dp.Tensors(c)
    ref, emu = dp.reference(c, t), dp.emulate(c, t)
    dt, H = dp.DT[c["dt"]], c["H"]
    r = Run(c)
    r.inp("qt", t.qt.reshape(t.R * H, dp.D).to(dt))
    r.inp("mem", t.mem.to(dt))
    r.inp("kpm", t.kpm)
    r.inp("cu", t.cu)
    if c["form"] == "self":
        r.inp("t_dev", torch.tensor([c["t"]], dtype=I32))
    ctx = r.out("ctx", (t.R * H, dp.D), dt)
    assert all(r.aligned16(k) for k in ("qt", "mem", "ctx"))
    sc = Scratch(p)
    _launch(lib, L, c, p, r, ctx, sc)
    first = r.now("ctx")
    _launch(lib, L, c, p, r, ctx, sc)
    again = r.now("ctx")
    assert torch.equal(_bits(first), _bits(again)), f"{c['name']}: two launches differ ({int((_bits(first) != _bits(again)).sum())} element(s))"
    assert torch.equal(_bits(_ops_launch(c, r, sc)), _bits(first)), f"{c['name']}: plankassembly_amd.ops and the C ABI differ"
    # entries that must give each other's bits
    twin = None
    if c["entry"] == "self_ws" and c["dt"] == "f32" and c["nparts"] == 0:
        twin = "self32"                                             # pa_dec_self_mq32
    elif c["entry"] == "group" and (c["G"], c["rpb"], c["nparts"]) == (1, 1, 0):
        twin = "ws"                                                 # pa_dec_cross_mq_ws / pa_dec_cross_mq32_ws
    if twin:
        ctx2 = r.out("ctx2", (t.R * H, dp.D), dt)
        _launch(lib, L, c, p, r, ctx2, sc, entry=twin)
        assert torch.equal(_bits(r.now("ctx2")), _bits(first)), f"{c['name']}: the {twin} entry gives other bits"
    w = r.finish()                                                  # guards of ctx, and qt / mem / kpm / cu / t_dev bit for bit as before
    got = w["ctx"].to(torch.float64).numpy().reshape(t.R, H, dp.D)
    return p, dp.judge(c, t, got, ref, emu, env=ENV)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case(c):
    if BUNDLE:
        assert dp.dispatch(c, ENV) != dp.dispatch(c)
    else:
        ok, plan = dp.on_branch(c, ENV)
        assert ok, f"{c['name']}: meant for {c['branch']}, dispatched as {plan}"
    p, (r, r_emu) = run_case(c)
    print(f"{p['kern']} {c['name']} {BUNDLE or 'default'} r(got) r_emu = {r:.4g} {r_emu:.4g}")
    path = os.environ.get("DEC_MQ_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(f"{p['kern']} {c['name']} {BUNDLE or 'default'} {r:.4g} {r_emu:.4g}\n")


def test_shapes_and_pointers_outside_the_contract_are_rejected():
    """Every rejection of dec_mq_parity.rejections() from the real library - the status comes back before any launch, ctx keeps its pattern."""
    if BUNDLE:
        return
    L = _L(); lib = L.lib(); st = L.stream()
    for c, status in dp.rejections():
        dt = dp.DT[c["dt"]]
        r = Run(c)
        qt = r.inp("qt", torch.zeros(16, dp.D, dtype=dt))           # (the operands of the accepted base shape B 2, S 32, H 8, whatever the call claims)
        mem = r.inp("mem", torch.zeros(64, dp.D, dtype=dt))
        td = r.inp("t_dev", torch.tensor([3], dtype=I32))
        ctx = r.out("ctx", (16, dp.D), dt)
        ptr = {"qt": qt, "mem": mem, "ctx": ctx, "t_dev": td}
        if c.get("null"):
            ptr[c["null"]] = None
        if c.get("misalign"):
            ptr[c["misalign"]] = C.c_void_p(ptr[c["misalign"]].value + 8)
        f32 = c["dt"] == "f32"
        B, G, H, S, d = c["B"], c["G"], c["H"], c["S"], c.get("d", dp.D)
        e = c["entry"]
        if e == "plain":
            rc = (lib.pa_dec_cross_mq32 if f32 else lib.pa_dec_cross_mq)(ptr["ctx"], ptr["qt"], ptr["mem"], None, None, B, S, H, d, st)
        elif e == "ws":
            rc = (lib.pa_dec_cross_mq32_ws if f32 else lib.pa_dec_cross_mq_ws)(ptr["ctx"], ptr["qt"], ptr["mem"], None, None, B, S, H, d, None, C.c_int64(0), st)
        elif e == "group":
            rc = (lib.pa_dec_cross_mq32_group if f32 else lib.pa_dec_cross_mq_group)(ptr["ctx"], ptr["qt"], ptr["mem"], None, None, B, G, S, H, d, c["rpb"], c["nparts"],
                                                                                     None, C.c_int64(0), st)
        elif e == "self_ws":
            rc = lib.pa_dec_self_mq_ws(ptr["ctx"], ptr["qt"], ptr["mem"], ptr["t_dev"], B, S, H, d, dp.PADT[c["dt"]], c["nparts"], None, C.c_int64(0), st)
        else:
            rc = lib.pa_dec_self_mq32(ptr["ctx"], ptr["qt"], ptr["mem"], ptr["t_dev"], B, S, H, d, st)
        call(c["name"], rc, status)
        w = r.finish()
        assert bool((w["ctx"] == torch.full((1,), dp.PATTERN, dtype=dt)).all()), f"{c['name']}: ctx of a rejected launch was written"


# ------------------------------------------------------------------------------------------------ the switch bundles, one child each
@pytest.mark.parametrize("bundle", list(dp.BUNDLES))
def test_switch_bundle_in_a_child_process(bundle):
    assert not _FAULTED, f"an earlier launch faulted the device ({_FAULTED[0]}): no child is started"
    assert not _CHILD_FAILED, f"the child of bundle {_CHILD_FAILED[0]} failed: no further child is started"
    env = {k: v for k, v in os.environ.items() if k not in dp.SWITCHES}
    env.update(dp.BUNDLES[bundle], DEC_MQ_PARITY_BUNDLE=bundle, PYTHONPATH=REPO + os.pathsep + env.get("PYTHONPATH", ""))
    n_cases = sum(dp.dispatch(c, dp.BUNDLES[bundle]) != dp.dispatch(c) for c in ALL)
    assert n_cases
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--bundle", bundle], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _CHILD_FAILED.append(bundle)
        raise
    if r.returncode != 0:
        _CHILD_FAILED.append(bundle)
    assert r.returncode == 0, f"bundle {bundle}: exit {r.returncode}\n" + r.stdout[-4000:] + r.stderr[-2000:]
    assert f"{n_cases} passed" in r.stdout, r.stdout[-2000:]


if __name__ == "__main__":
    assert sys.argv[1] == "--bundle" and BUNDLE == sys.argv[2]
    assert ENV == dp.BUNDLES[BUNDLE], (ENV, dp.BUNDLES[BUNDLE])
    assert CASES, f"bundle {BUNDLE}: the restated dispatch of no case differs from the default"
    sys.exit(pytest.main(["-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "test_case"]))
