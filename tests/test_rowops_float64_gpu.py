"""Every entry point of csrc/rowops.hip (LayerNorm forward / backward and their finishers, switch head, GELU, mixture NLL, Adam, casts,
embedding gathers and scatter-adds, batch-preparation sorts) held PER ELEMENT to a float64 reference at every branch of its host dispatch,
with guarded outputs and poisoned input padding (tests/rowops_parity.py: the checker, the case table, the restated dispatch and the
derivation of the bounds; tests/test_rowops_parity_cpu.py tests the checker itself on seeded defects).

Calls go through plankassembly_amd._lib with pointers into the guarded buffers.  rowops.hip has no plan or record call: every case first
asserts that the restated dispatch (rowops_parity.dispatch, a pure function of the arguments and the switches) puts it on the branch it is
meant for, and that the operands have the alignment that dispatch assumes.  The first HIP error of a process is remembered and nothing more
is launched after it.

PA_LNB_512, PA_DETERMINISTIC and PA_EMBED_ORDERED_GROUPS are read once per process, so each of the four bundles runs this file as a script
in a fresh child process, one after the other: the child asserts - before anything touches the device - that its switch changes the restated
dispatch of some case, then runs the cases whose dispatch it changes.

With ROWOPS_PARITY_REPORT=<file> every case appends `bundle kernel dtype case r(got) r_cpu` (the figures of profiles/rowops_float64_parity.txt).
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

import rowops_parity as rp                                          # noqa: E402

pytestmark = pytest.mark.gpu

BUNDLE = os.environ.get("ROWOPS_PARITY_BUNDLE", "")                 # set in a bundle's child process only
ENV = {k: os.environ[k] for k in rp.SWITCHES if k in os.environ}    # the switches of this process, as the library reads them
ALL = rp.all_cases()
CASES = [c for c in ALL if rp.dispatch(c, ENV) != rp.dispatch(c)] if BUNDLE else ALL
_FAULTED = []                                                      # first HIP error of this process, if any
_CHILD_DIED = []                                                   # a child that ended on a signal or at its time limit
F32, BF16, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64


def _L():
    from plankassembly_amd import _lib as L
    return L


def call(what, rc, want=0):
    if rc > 0:
        _FAULTED.append(f"{what}: hipError {rc}")
    assert rc == want, f"{what} returned {rc} ({_L()._ERR.get(rc, 'a raw HIP error code')}), want {want}"


def _report(c, rows):
    path = os.environ.get("ROWOPS_PARITY_REPORT")
    for kernel, dt, r, r_cpu in rows:
        fig = "- -" if r is None else f"{r:.4g} {r_cpu:.4g}"       # (-: no f32 output among those of the case, so no r)
        print(f"{c['name']} [{kernel} {dt}] r(got) r_cpu = {fig}")
        if path:
            with open(path, "a") as f:
                f.write(f"{BUNDLE or 'default'} {kernel} {dt} {c['name']} {fig}\n")


class Run:
    """The operands of one case on the device, each a window of a guarded buffer."""

    def __init__(self, c):
        assert not _FAULTED, f"an earlier launch faulted the device ({_FAULTED[0]}): nothing more is started on it"
        self.c, self.g, self.dev, self.win = c, {}, {}, None

    def _add(self, key, g):
        assert key not in self.g, key
        self.g[key], self.dev[key] = g, g.buf.to("cuda")
        return self.p(key)

    def inp(self, key, values, **kw):
        return None if values is None else self._add(key, rp.Guarded(values.contiguous(), **kw))

    def out(self, key, shape, dtype, init=None, **kw):
        g = rp.Guarded(shape=shape, dtype=dtype, out=True, **kw)
        if init is not None:
            g.view().copy_(init.reshape(g.rows, g.cols))
        return self._add(key, g)

    def p(self, key):
        return C.c_void_p(self.dev[key].data_ptr() + self.g[key].byte_offset())

    def aligned16(self, key):
        return (self.p(key).value & 15) == 0

    def sync(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                                   # a HIP error after a launch: the later cases of this process fail unstarted
            _FAULTED.append(str(e).splitlines()[0])
            raise

    def now(self, key):
        """The window of `key` as the device holds it now (a copy on the CPU)."""
        self.sync()
        return self.g[key].view(self.dev[key].cpu()).clone()

    def finish(self):
        """After the launches: every guard and every input checked; {key: window on the CPU}."""
        self.sync()
        self.win = {}
        for key, g in self.g.items():
            after = self.dev[key].cpu()
            g.check(after, f"{self.c['name']}: {key}")
            self.win[key] = g.view(after)
        return self.win


def _np(x):
    return x.to(torch.float64).numpy()


def _untouched(w, what):
    fill = torch.full((1,), rp.PATTERN if w.dtype.is_floating_point else -123, dtype=w.dtype)
    assert bool((w == fill).all()), f"{what}: written"


# ------------------------------------------------------------------------------------------------ the runners: one case on the device -> `got`
def run_ln(c, t):
    L = _L(); lib = L.lib(); st = L.stream()
    r = Run(c)
    rows, d, tdt, pdt = c["rows"], c["d"], rp.DT[c["dt"]], rp.PADT[c["dt"]]
    plan = rp.dispatch(c, ENV)
    assert lib.pa_layernorm_bwd_can_img(d, pdt) == plan["can_img"], (c["name"], plan)
    nparts = lib.pa_layernorm_bwd_nparts(rows)
    assert nparts == plan["nparts"] and lib.pa_layernorm_ws_floats(rows, d) == nparts * 3 * d
    z, gamma, beta = r.inp("z", t["z"]), r.inp("gamma", t["gamma"]), r.inp("beta", t["beta"])
    dy = r.inp("dy", t["dy"], lead=c["mis"])
    y, mean, rstd = r.out("y", (rows, d), tdt), r.out("mean", (rows,), F32), r.out("rstd", (rows,), F32)
    img = r.out("img", (rows, 3 * d), BF16) if c["img"] is not None else None
    call("pa_layernorm_fwd_img", lib.pa_layernorm_fwd_img(y, z, gamma, beta, mean, rstd, rows, d, c["eps"], pdt, img, c["img"] or 0, st))
    all16 = all(r.aligned16(k) for k in ("z", "gamma", "dy"))
    assert all16 == (c["mis"] == 0), "the operands do not have the alignment the restated dispatch assumes"
    stats = [(r.now("mean").reshape(-1), r.now("rstd").reshape(-1)), rp.f64_stats(c, t)]
    launches = [(0, c["drop_p"]), (1, c["drop_p"])] + ([(0, 0.0)] if c["drop_p"] else [])        # the last: dz must not depend on the dropout
    for i, (which, p) in enumerate(launches):
        mi, ri = r.inp(f"mean{i}", stats[which][0]), r.inp(f"rstd{i}", stats[which][1])
        dz = r.out(f"dz{i}", (rows, d), tdt)
        dd = r.out(f"dd{i}", (rows, d), tdt) if p else None
        part = r.out(f"partial{i}", (nparts, 3 * d), F32)
        dg, db = r.out(f"dg{i}", (d,), F32, init=t["dgamma0"]), r.out(f"db{i}", (d,), F32, init=t["dbeta0"])
        ds = r.out(f"ds{i}", (d,), F32, init=t["dzsum0"]) if c["dzsum"] else None
        bimg = r.out(f"bimg{i}", (rows, 3 * d), BF16) if (c["img"] is not None and plan["can_img"]) else None
        assert r.aligned16(f"dz{i}") and r.aligned16(f"partial{i}") and (dd is None or r.aligned16(f"dd{i}"))
        call("pa_layernorm_bwd_partial_img", lib.pa_layernorm_bwd_partial_img(dz, dd, dy, z, gamma, mi, ri, c["dzsum"], part, rows, d, pdt, p, t["seed"], bimg,
                                                                               c["img"] or 0, st))
        desc = rp.LnFinishDesc(part.value, dg.value, db.value, ds.value if ds else None, nparts, 0)
        call("pa_layernorm_finish_many", lib.pa_layernorm_finish_many(C.byref(desc), 1, d, st))
    w = r.finish()
    got = dict(mean=_np(w["mean"]).reshape(-1), rstd=_np(w["rstd"]).reshape(-1), y=_np(w["y"]), bwd=[])
    for i in (0, 1):
        got["bwd"].append(dict(mean32=stats[i][0], rstd32=stats[i][1], dz=_np(w[f"dz{i}"]), ddrop=_np(w[f"dd{i}"]) if c["drop_p"] else None,
                               dgamma=_np(w[f"dg{i}"]).reshape(-1), dbeta=_np(w[f"db{i}"]).reshape(-1), dzsum=_np(w[f"ds{i}"]).reshape(-1) if c["dzsum"] else None))
        if not c["dzsum"]:
            _untouched(w[f"partial{i}"][:, 2 * d:], f"{c['name']}: the dzsum third of the partials without want_dzsum")
    if c["drop_p"]:
        it = torch.int32 if c["dt"] == "f32" else torch.int16
        assert torch.equal(w["dz2"].contiguous().view(it), w["dz0"].contiguous().view(it)), f"{c['name']}: dz differs between the dropout and the no-dropout launch"
    if c["img"] is not None:
        assert torch.equal(w["img"].view(torch.int16).reshape(rows, 3, d), rp.split_planes(w["y"], c["img"])), f"{c['name']}: forward bf16x3 planes"
        if plan["can_img"]:
            src = w["dd0"] if c["drop_p"] else w["dz0"]
            assert torch.equal(w["bimg0"].view(torch.int16).reshape(rows, 3, d), rp.split_planes(src, c["img"])), f"{c['name']}: backward bf16x3 planes"
    return got


def run_finish(c, t):
    L = _L(); lib = L.lib()
    r, d = Run(c), c["d"]
    descs = (rp.LnFinishDesc * len(c["nparts"]))()
    for i, n in enumerate(c["nparts"]):
        part = r.inp(f"partial{i}", t["partial"][i])
        outs = [r.out(f"o{i}{q}", (d,), F32, init=t["init"][i][q]) for q in range(3)]
        descs[i] = rp.LnFinishDesc(part.value, outs[0].value, outs[1].value, None if i == c["null_dzsum"] else outs[2].value, n, 0)
    call("pa_layernorm_finish_many", lib.pa_layernorm_finish_many(C.cast(descs, C.c_void_p), len(c["nparts"]), d, L.stream()))
    w = r.finish()
    i = c["null_dzsum"]
    assert torch.equal(w[f"o{i}2"].reshape(-1), t["init"][i][2]), f"{c['name']}: the output behind a null dzsum was written"
    return [[_np(w[f"o{i}{q}"]).reshape(-1) for q in range(3)] for i in range(len(c["nparts"]))]


def run_switch(c, t):
    L = _L(); lib = L.lib(); st = L.stream()
    r = Run(c)
    rows, d, tdt, pdt = c["rows"], c["d"], rp.DT[c["dt"]], rp.PADT[c["dt"]]
    nparts = -(-rows // 8)
    h, w_, b, ds = r.inp("h", t["h"]), r.inp("w", t["w"]), r.inp("b", t["b"]), r.inp("ds", t["ds"])
    s = r.out("s", (rows,), F32)
    call("pa_switch_fwd", lib.pa_switch_fwd(s, h, pdt, w_, b, rows, d, st))
    if d > 2048:
        dh = r.out("dh", (rows, d), tdt)
        call("pa_switch_bwd", lib.pa_switch_bwd(dh, 0, w_, b, ds, h, pdt, w_, w_, rows, d, st), rp.PA_EINVAL)
        w = r.finish()
        return dict(s=_np(w["s"]).reshape(-1))
    dh = r.out("dh", (rows, d), tdt, init=t["dh0"] if c["acc"] else None)
    dw, db = r.out("dw", (d,), F32, init=t["dw0"]), r.out("db", (1,), F32, init=t["db0"])
    part = r.out("partial", (nparts, 2 * d), F32)
    call("pa_switch_bwd", lib.pa_switch_bwd(dh, c["acc"], dw, db, ds, h, pdt, w_, part, rows, d, st))
    w = r.finish()
    return dict(s=_np(w["s"]).reshape(-1), dh=_np(w["dh"]), dw=_np(w["dw"]).reshape(-1), db=_np(w["db"]).reshape(-1)[0])


def run_gelu(c, t):
    L = _L(); lib = L.lib(); st = L.stream()
    r = Run(c)
    rows, cols, ld, tdt, pdt = c["rows"], c["cols"], c["ld"], rp.DT[c["dt"]], rp.PADT[c["dt"]]
    x, dh = r.inp("x", t["x"], ld=ld), r.inp("dh", t["dh"], ld=ld)
    y, dp = r.out("y", (rows, cols), tdt, ld=ld), r.out("dpre", (rows, cols), tdt, ld=ld)
    call("pa_gelu_fwd", lib.pa_gelu_fwd(y, x, rows, cols, ld, pdt, c["drop_p"], t["seed"], st))
    call("pa_gelu_bwd", lib.pa_gelu_bwd(dp, dh, x, rows, cols, ld, pdt, c["drop_p"], t["seed"], st))
    w = r.finish()
    return dict(y=_np(w["y"]), dpre=_np(w["dpre"]))


def run_nll(c, t):
    L = _L(); lib = L.lib(); st = L.stream()
    r = Run(c)
    B, T, V, ldv, pad = c["B"], c["T"], c["V"], c["ldv"], t["pad"]
    n = B * T
    vocab, ptr, sw, lab, up = r.inp("vocab", t["vocab"], ld=ldv), r.inp("ptr", t["ptr"]), r.inp("sw", t["sw"]), r.inp("label", t["label"]), r.inp("up", t["up"])
    for form, fn in (("fwd", lib.pa_mixture_nll_fwd), ("fin", lib.pa_mixture_nll_fwd_fin)):
        stats, lse = r.out(f"stats_{form}", (8,), F32, init=torch.zeros(8)), r.out(f"lse_{form}", (n, 2), F32)
        call(f"pa_mixture_nll_{form}", fn(stats, lse, vocab, ldv, ptr, sw, lab, B, T, V, pad, st))
    for k, (odt, gscale, use_up) in enumerate(rp.NLL_BWD_FORMS):
        dv, dp, dsw = r.out(f"dv{k}", (n, ldv), rp.DT[odt]), r.out(f"dp{k}", (n, T), rp.DT[odt]), r.out(f"dsw{k}", (n,), F32)
        args = (dv, dp, rp.PADT[odt], dsw, r.p("stats_fin"), r.p("lse_fin"), vocab, ldv, ptr, sw, lab, B, T, V, pad, gscale)
        if use_up:
            call("pa_mixture_nll_bwd_up", lib.pa_mixture_nll_bwd_up(*args, up, st))
        else:
            call("pa_mixture_nll_bwd", lib.pa_mixture_nll_bwd(*args, st))
    w = r.finish()
    assert bool((w["stats_fwd"].reshape(-1)[3:] == 0).all()), f"{c['name']}: pa_mixture_nll_fwd wrote behind its three sums"
    sf = w["stats_fin"].reshape(-1)
    got = dict(fwd=dict(stats=_np(w["stats_fwd"]).reshape(-1)[:3], lse=_np(w["lse_fwd"])), fin=dict(stats=_np(sf)[:6], lse=_np(w["lse_fin"])), bwd=[])
    for k, (odt, gscale, use_up) in enumerate(rp.NLL_BWD_FORMS):
        dv = w[f"dv{k}"]
        assert bool((dv[:, V:] == 0).all()), f"{c['name']}: the gradient columns V .. ldv - 1 are not all zero"
        got["bwd"].append(dict(lse32=w["lse_fin"].clone(), count32=np.float32(float(sf[1])), up32=np.float32(t["up"][0]) if use_up else np.float32(float(sf[3])),
                               dv=_np(dv[:, :V]), dp=_np(w[f"dp{k}"]), dsw=_np(w[f"dsw{k}"]).reshape(-1)))
    return got


def run_adam(c, t):
    L = _L(); lib = L.lib(); st = L.stream()
    r, n, hp = Run(c), c["n"], rp.ADAM_HP
    p, m, v = (r.out(k, (n,), F32, init=t[k]) for k in ("p", "m", "v"))
    pb = r.out("pb", (n,), BF16)
    got = []
    for k in range(hp["steps"]):
        g = r.inp(f"g{k}", t["g"][k])
        call("pa_adam_step", lib.pa_adam_step(p, g, m, v, pb, n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], k + 1, hp["gscale"], st))
        got.append(dict(p=r.now("p").reshape(-1), m=r.now("m").reshape(-1), v=r.now("v").reshape(-1), pb=r.now("pb").reshape(-1).view(torch.int16)))
    r.finish()
    return got


def run_cast(c, t):
    L = _L(); lib = L.lib()
    r = Run(c)
    src, dst = r.inp("src", t["src"]), r.out("dst", (c["n"],), rp.DT[c["dst"]])
    call("pa_cast", lib.pa_cast(dst, rp.PADT[c["dst"]], src, rp.PADT[c["src"]], c["n"], L.stream()))
    return r.finish()["dst"].reshape(-1).clone()


def _ptrs(ps):
    arr = (C.c_void_p * len(ps))()
    for i, p in enumerate(ps):
        arr[i] = p.value if p is not None else None
    return arr


def run_embed_in(c, t, want_bwd=0):
    L = _L(); lib = L.lib(); st = L.stream()
    r = Run(c)
    n, d, nt = c["n_tok"], c["d"], len(c["rows"])
    tabs = [r.inp(f"table{k}", t["tables"][k]) for k in range(nt)]
    idx = [None if k == c["absent"] else r.inp(f"idx{k}", t["idx"][k]) for k in range(nt)]
    rowmap, dout = r.inp("rowmap", t["rowmap"]), r.inp("dout", t["dout"])
    out = r.out("out", (n, d), rp.DT[c["dt"]])
    dtabs = [r.out(f"dtable{k}", (c["rows"][k], d), F32, init=t["dtab0"][k]) for k in range(nt)]
    call("pa_embed_input_fwd", lib.pa_embed_input_fwd(out, rp.PADT[c["dt"]], _ptrs(tabs), _ptrs(idx), rowmap, nt, n, d, st))
    rows = (C.c_int32 * nt)(*c["rows"])
    call("pa_embed_input_bwd", lib.pa_embed_input_bwd(dout, rp.PADT[c["dt"]], _ptrs(dtabs), _ptrs(idx), rowmap, rows, nt, n, d, st), want_bwd)
    w = r.finish()
    if c["absent"] is not None:
        assert torch.equal(w[f"dtable{c['absent']}"], t["dtab0"][c["absent"]]), f"{c['name']}: the gradient of the absent table was written"
    return dict(out=_np(w["out"]), grads=[_np(w[f"dtable{k}"]) for k in range(nt)])


def run_embed_out(c, t):
    L = _L(); lib = L.lib(); st = L.stream()
    r = Run(c)
    B, T, d, dof, pdt = c["B"], c["T"], c["d"], c["dof"], rp.PADT[c["dt"]]
    tok = r.inp("tok", t["tok"], ld=c["tok_ld"])
    value, coord, pos, dout = r.inp("value", t["value"]), r.inp("coord", t["coord"]), r.inp("pos", t["pos"]), r.inp("dout", t["dout"])
    out = r.out("out", (B * T, d), rp.DT[c["dt"]])
    gr = [r.out(f"g{k}", tuple(t[s].shape), F32, init=t[s]) for k, s in enumerate(("dv0", "dc0", "dp0"))]
    call("pa_embed_output_fwd", lib.pa_embed_output_fwd(out, pdt, value, coord, pos, tok, c["tok_ld"], B, T, d, dof, st))
    call("pa_embed_output_bwd", lib.pa_embed_output_bwd(dout, pdt, gr[0], gr[1], gr[2], tok, c["tok_ld"], B, T, d, dof, st))
    w = r.finish()
    return dict(out=_np(w["out"]), grads=[_np(w[f"g{k}"]) for k in range(3)])


def run_seg(c, t):
    L = _L(); lib = L.lib(); st = L.stream()
    r = Run(c)
    nt, d = len(c["rows"]), c["d"]
    dout = r.inp("dout", t["dout"])
    order, seg = [r.inp(f"order{k}", t["order"][k]) for k in range(nt)], [r.inp(f"seg{k}", t["seg"][k]) for k in range(nt)]
    rows = (C.c_int32 * nt)(*c["rows"])
    for rep in (0, 1):                                              # twice from the same start: the ordered kernels repeat their bits
        dt_ = [r.out(f"dtable{rep}_{k}", (c["rows"][k], d), F32, init=t["dtab0"][k]) for k in range(nt)]
        call("pa_embed_segment_bwd", lib.pa_embed_segment_bwd(dout, rp.PADT[c["dt"]], _ptrs(dt_), _ptrs(order), _ptrs(seg), rows, nt, t["n_rows"], d, st))
    w = r.finish()
    if rp.dispatch(c, ENV)["kernel"] != "atomic":
        for k in range(nt):
            assert torch.equal(w[f"dtable0_{k}"].view(torch.int32), w[f"dtable1_{k}"].view(torch.int32)), f"{c['name']}: table {k}: two ordered calls differ"
    return [_np(w[f"dtable0_{k}"]) for k in range(nt)]


def run_pack(c, t):
    L = _L(); lib = L.lib()
    r = Run(c)
    B, S = c["B"], c["S"]
    mask = r.inp("mask", t["mask"])
    cu, rowmap = r.out("cu", (2 * B + 1,), I32), r.out("rowmap", (B * S,), I32)
    call("pa_pack_rows", lib.pa_pack_rows(mask, B, S, cu, rowmap, L.stream()))
    w = r.finish()
    cu_, rm = w["cu"].reshape(-1), w["rowmap"].reshape(-1)
    nv = int(cu_[B])
    assert 0 <= nv <= B * S
    _untouched(rm[nv:], f"{c['name']}: rowmap behind the valid rows")
    return dict(cu=cu_[:B + 1].clone(), rowmap=rm[:nv].clone(), order=cu_[B + 1:].clone())


def run_group(c, t, want=0):
    L = _L(); lib = L.lib()
    r = Run(c)
    descs = (L.GroupDesc * len(c["descs"]))()
    for i, (q, tt) in enumerate(zip(c["descs"], t["tabs"])):
        idx = r.inp(f"idx{i}", tt["idx"])
        rowmap = r.inp(f"rowmap{i}", tt["rowmap"])
        order, seg = r.out(f"order{i}", (q["n"],), I32), r.out(f"seg{i}", (q["R"] + 1,), I32)
        g = descs[i]
        g.idx, g.rowmap, g.order, g.seg = (idx.value if idx else None), (rowmap.value if rowmap else None), order.value, seg.value
        g.n, g.rows, g.kind = q["n"], q["R"], q["kind"]
        g.T, g.dof, g.tok_ld = (q["T"] or 0), q["dof"], (q["T"] + 2 if q["T"] else 0)
    call("pa_group_rows", lib.pa_group_rows(C.cast(descs, C.c_void_p), len(c["descs"]), L.stream()), want)
    w = r.finish()
    got = []
    for i, q in enumerate(c["descs"]):
        seg, order = w[f"seg{i}"].reshape(-1), w[f"order{i}"].reshape(-1)
        if want:
            _untouched(seg, "seg of a rejected launch"); _untouched(order, "order of a rejected launch")
            continue
        used = int(seg[q["R"]])
        assert 0 <= used <= q["n"]
        _untouched(order[used:], f"{c['name']}: table {i}: order behind the grouped entries")
        got.append(dict(seg=seg.clone(), order=order[:used].clone()))
    return got


RUNNERS = {"ln": run_ln, "ln_finish": run_finish, "switch": run_switch, "gelu": run_gelu, "nll": run_nll, "adam": run_adam, "cast": run_cast,
           "embed_in": run_embed_in, "embed_out": run_embed_out, "embed_seg": run_seg, "pack_rows": run_pack, "group_rows": run_group}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case(c):
    if BUNDLE:                                                      # a bundle's child: the expectation is the restated dispatch under its switches
        assert rp.dispatch(c, ENV) != rp.dispatch(c)
    else:
        ok, plan = rp.on_branch(c, ENV)
        assert ok, f"{c['name']}: meant for {c['branch']}, dispatched as {plan}"
    inputs, _, verify, _ = rp.GROUPS[c["kernel"]]
    t = inputs(c)
    got = RUNNERS[c["kernel"]](c, t)
    _report(c, verify(c, t, got))


def test_widths_and_types_outside_the_contract_are_rejected():
    """LayerNorm d = 2052 and d = 6 (PA_EINVAL), the switch backward at d = 2052 (PA_EINVAL; its forward has no cap and runs), pa_embed_input_bwd at
    d = 1028 (PA_ESHAPE), pa_group_rows at R = 2049 (PA_ESHAPE), pa_cast bf16 -> bf16 (PA_EINVAL): nothing is written."""
    L = _L(); lib = L.lib(); st = L.stream()
    for d in (2052, 6):
        c = dict(kernel="ln", name=f"ln_reject_d{d}", dt="f32", rows=5, d=d, eps=1e-5, kind="unit", dzsum=1, drop_p=0.0, mis=0, img=None)
        t = rp.ln_inputs(c)
        r = Run(c)
        z, gamma, beta, dy = (r.inp(k, t[k]) for k in ("z", "gamma", "beta", "dy"))
        y, mean, rstd, part = r.out("y", (5, d), F32), r.out("mean", (5,), F32), r.out("rstd", (5,), F32), r.out("partial", (1, 3 * d), F32)
        call("pa_layernorm_fwd", lib.pa_layernorm_fwd(y, z, gamma, beta, mean, rstd, 5, d, 1e-5, rp.PA_F32, st), rp.PA_EINVAL)
        call("pa_layernorm_bwd_partial", lib.pa_layernorm_bwd_partial(y, None, dy, z, gamma, mean, rstd, 1, part, 5, d, rp.PA_F32, 0.0, 0, st), rp.PA_EINVAL)
        r.finish()
        _untouched(r.win["y"], "y of a rejected launch"); _untouched(r.win["partial"], "partial of a rejected launch")
    for dt in ("f32", "bf16"):                                      # the switch forward has no width cap
        c = dict(kernel="switch", name=f"switch_{dt}_r9_d2052", dt=dt, rows=9, d=2052, acc=0)
        t = rp.switch_inputs(c)
        got = run_switch(c, t)
        ref, cpu = rp.switch_ref(c, t), rp.switch_cpu32(c, t)
        _report(c, [("switch_fwd", dt) + rp.check(c["name"], "s", "switch_fwd", got["s"], *ref["s"], cpu=cpu["s"])])
    c = dict(kernel="embed_in", name="embed_in_reject_d1028", dt="f32", n_tok=5, d=1028, rowmap=0, absent=None, rows=rp.EMB_TABLE_ROWS)
    t = rp.embed_in_inputs(c)
    got = run_embed_in(c, t, want_bwd=rp.PA_ESHAPE)
    for k in range(5):
        assert np.array_equal(got["grads"][k], rp.f64(t["dtab0"][k]))
    c = dict(kernel="group_rows", name="group_reject_R2049", descs=[rp._gdesc(0, 2049, 63)])
    run_group(c, rp.group_inputs(c), want=rp.PA_ESHAPE)
    c = dict(kernel="cast", name="cast_reject_bf16_bf16", src="bf16", dst="bf16", n=257)
    r = Run(c)
    src, dst = r.inp("src", rp.cast_inputs(c)["src"]), r.out("dst", (257,), BF16)
    call("pa_cast", lib.pa_cast(dst, rp.PA_BF16, src, rp.PA_BF16, 257, st), rp.PA_EINVAL)
    _untouched(r.finish()["dst"], "dst of a rejected cast")


# ------------------------------------------------------------------------------------------------ the switch bundles, one child each
def _bundle_child(bundle):
    """In the child, before anything touches the device: the switch is set as the bundle says and changes the restated dispatch of a case."""
    assert ENV == rp.BUNDLES[bundle], (ENV, rp.BUNDLES[bundle])
    assert CASES, f"bundle {bundle}: the restated dispatch of no case differs from the default"
    if bundle == "lnb512_0":
        assert any(c["kernel"] == "ln" and c["dt"] == "f32" and rp.dispatch(c, ENV)["bwd"] == "generic" and rp.dispatch(c)["bwd"] == "bwd512" for c in CASES)
        assert all(rp.dispatch(c, ENV)["can_img"] == 0 for c in CASES)
    else:
        assert all(c["kernel"] == "embed_seg" for c in CASES)
        want = {"deterministic_0": {"f32": "atomic"}, "deterministic_1": {"bf16": "ordered4"}, "ordered_groups_1": {"f32": "one_group_ordered"}}[bundle]
        for dt, kern in want.items():
            assert any(c["dt"] == dt and rp.dispatch(c, ENV)["kernel"] == kern for c in CASES), (bundle, dt, kern)


@pytest.mark.parametrize("bundle", list(rp.BUNDLES))
def test_switch_bundle_in_a_child_process(bundle):
    assert not _FAULTED, f"an earlier launch faulted the device ({_FAULTED[0]}): no child is started"
    assert not _CHILD_DIED, f"the child of bundle {_CHILD_DIED[0]} ended on a signal or at its time limit: no further child is started"
    env = {k: v for k, v in os.environ.items() if k not in rp.SWITCHES}
    env.update(rp.BUNDLES[bundle], ROWOPS_PARITY_BUNDLE=bundle, PYTHONPATH=REPO + os.pathsep + env.get("PYTHONPATH", ""))
    n_cases = sum(rp.dispatch(c, rp.BUNDLES[bundle]) != rp.dispatch(c) for c in ALL)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--bundle", bundle], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append(bundle)
        raise
    if r.returncode < 0:                                            # (ended on a signal: it fails here, once; nothing is retried)
        _CHILD_DIED.append(bundle)
    assert r.returncode == 0, f"bundle {bundle}: exit {r.returncode}\n" + r.stdout[-4000:] + r.stderr[-2000:]
    assert f"{n_cases} passed" in r.stdout, r.stdout[-2000:]


if __name__ == "__main__":
    assert sys.argv[1] == "--bundle" and BUNDLE == sys.argv[2]
    _bundle_child(sys.argv[2])
    sys.exit(pytest.main(["-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "test_case"]))
