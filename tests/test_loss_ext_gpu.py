"""The extended mixture NLL kernels (include/plank_hip.h pa_mixture_nll_fwd_ext / pa_mixture_nll_bwd_ext) at kernel level through
plankassembly_amd.ops, on the mixture-NLL case table of tests/rowops_parity.py: bit-identity with the un-extended entries when everything is
off, and parity per element against the float64 restatement of tests/loss_ext_reference.py (tiers 1 / 2) with smoothing and weights on.
Every output is a window of a guarded buffer, every input is poisoned around its window and compared bit for bit after the launches
(the Run class of tests/test_rowops_float64_gpu.py).

With LOSS_EXT_PARITY_REPORT=<file> every (case, eps, weight) appends `kernel case eps weight r(got) r_cpu`."""
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

import loss_ext_reference as R                                      # noqa: E402
import rowops_parity as rp                                          # noqa: E402
from test_rowops_float64_gpu import Run, _np, _untouched, call     # noqa: E402

pytestmark = pytest.mark.gpu

CASES = rp.nll_cases()
IDS = [c["name"] for c in CASES]
F32, I32, I64 = torch.float32, torch.int32, torch.int64


def _ops():
    from plankassembly_amd import _lib as L, ops
    return L, ops


def _win(r, key):
    """The window of `key` as a tensor on the device (what ops takes), row stride as the guarded buffer has it."""
    g = r.g[key]
    return torch.as_strided(r.dev[key], (g.rows, g.cols), (g.ld, 1), g.off)


def _inputs(r, c, t, w):
    B, T = c["B"], c["T"]
    r.inp("vocab", t["vocab"], ld=c["ldv"]); r.inp("ptr", t["ptr"]); r.inp("sw", t["sw"]); r.inp("label", t["label"]); r.inp("up", t["up"])
    if w is not None:
        r.inp("weight", w.reshape(-1))
    return dict(vocab=_win(r, "vocab"), ptr=_win(r, "ptr"), sw=_win(r, "sw").view(-1), label=_win(r, "label").view(B, T), up=_win(r, "up").view(-1),
                weight=None if w is None else _win(r, "weight").view(w.shape))


def _ext_fwd(r, c, t, d, eps, tag="", token=True):
    _, ops = _ops()
    n = c["B"] * c["T"]
    r.out(f"stats{tag}", (8,), F32); r.out(f"lse{tag}", (n, 2), F32); r.out(f"ext{tag}", (4,), F32)
    out = dict(stats8=_win(r, f"stats{tag}").view(-1), row_lse=_win(r, f"lse{tag}"), ext_stats=_win(r, f"ext{tag}").view(-1))
    if token:
        r.out(f"token{tag}", (n,), F32)
        out["token_nll"] = _win(r, f"token{tag}").view(c["B"], c["T"])
    ops.mixture_nll_ext_fwd(d["vocab"], d["ptr"], d["sw"], d["label"], c["V"], t["pad"], smoothing=eps, weight=d["weight"], out=out)
    return out


def _ext_bwd(r, c, t, d, eps, fwd, k, form, tag=""):
    _, ops = _ops()
    odt, gscale, use_up = form
    n, T, ldv = c["B"] * c["T"], c["T"], c["ldv"]
    r.out(f"dv{tag}{k}", (n, ldv), rp.DT[odt]); r.out(f"dp{tag}{k}", (n, T), rp.DT[odt]); r.out(f"dsw{tag}{k}", (n,), F32)
    out = dict(dvocab=_win(r, f"dv{tag}{k}"), dptr=_win(r, f"dp{tag}{k}"), dsw=_win(r, f"dsw{tag}{k}").view(-1))
    ops.mixture_nll_ext_bwd(fwd["stats8"], fwd["row_lse"], fwd["ext_stats"], d["vocab"], d["ptr"], d["sw"], d["label"], c["V"], t["pad"], smoothing=eps,
                            weight=d["weight"], gscale=gscale, upstream=d["up"] if use_up else None, out=out)


def _bits(x):
    return x.contiguous().view({2: torch.int16, 4: I32}[x.element_size()])


# ------------------------------------------------------------------------------------------------ 6: everything off = the present entries, bit for bit
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_off_is_bit_identical_to_the_unextended_entries(c):
    L, _ = _ops()
    lib, st = L.lib(), L.stream()
    t = rp.nll_inputs(c)
    B, T, V, ldv, pad = c["B"], c["T"], c["V"], c["ldv"], t["pad"]
    n = B * T
    r = Run(c)
    d = _inputs(r, c, t, None)
    stats, lse = r.out("stats_old", (8,), F32), r.out("lse_old", (n, 2), F32)
    call("pa_mixture_nll_fwd_fin", lib.pa_mixture_nll_fwd_fin(stats, lse, r.p("vocab"), ldv, r.p("ptr"), r.p("sw"), r.p("label"), B, T, V, pad, st))
    fwd = _ext_fwd(r, c, t, d, 0.0)
    for k, form in enumerate(rp.NLL_BWD_FORMS):
        odt, gscale, use_up = form
        dv, dp, dsw = r.out(f"dv_old{k}", (n, ldv), rp.DT[odt]), r.out(f"dp_old{k}", (n, T), rp.DT[odt]), r.out(f"dsw_old{k}", (n,), F32)
        call("pa_mixture_nll_bwd_up", lib.pa_mixture_nll_bwd_up(dv, dp, rp.PADT[odt], dsw, stats, lse, r.p("vocab"), ldv, r.p("ptr"), r.p("sw"), r.p("label"),
                                                                B, T, V, pad, gscale, r.p("up") if use_up else None, st))
        _ext_bwd(r, c, t, d, 0.0, fwd, k, form)
    w = r.finish()
    ck = rp.Checked(c)
    ck.exact("stats8", _bits(w["stats"]), _bits(w["stats_old"]))
    ck.exact("row_lse", _bits(w["lse"]), _bits(w["lse_old"]))
    for k, form in enumerate(rp.NLL_BWD_FORMS):
        for q in ("dv", "dp", "dsw"):
            ck.exact(f"{q} {form}", _bits(w[f"{q}{k}"]), _bits(w[f"{q}_old{k}"]))
    # the additional outputs: the plain mean is the loss, token_nll sums to the NLL sum
    ext, sf = w["ext"].reshape(-1), w["stats_old"].reshape(-1)
    assert float(ext[3]) == 0.0
    if int(sf[1]):
        assert _bits(ext[2:3]).item() == _bits(sf[4:5]).item(), (float(ext[2]), float(sf[4]))
        assert _bits(ext[:2]).view(I64).item() == _bits(sf[6:8]).view(I64).item()
        tok = w["token"].double().sum().item()
        assert abs(tok - float(sf[0])) <= 4 * rp.U24 * abs(tok) + n * 2.0 ** -31


# ------------------------------------------------------------------------------------------------ 7: parity per element
def _report(c, eps, kind, rows):
    path = os.environ.get("LOSS_EXT_PARITY_REPORT")
    for kernel, r_, rc in rows:
        line = f"{kernel} {c['name']} eps {eps} weight {kind} r(got) r_cpu = {r_:.4g} {rc:.4g}"
        print(line)
        if path:
            with open(path, "a") as f:
                f.write(line + "\n")


@pytest.mark.parametrize("kind", R.WEIGHT_KINDS, ids=["w_none", "w_B", "w_BT"])
@pytest.mark.parametrize("eps", [0.1, 0.5])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_parity_per_element(c, eps, kind):
    L, _ = _ops()
    lib, st = L.lib(), L.stream()
    t = rp.nll_inputs(c)
    wt = R.ext_weight(c, kind)
    B, T, V, ldv, pad = c["B"], c["T"], c["V"], c["ldv"], t["pad"]
    n = B * T
    r = Run(c)
    d = _inputs(r, c, t, wt)
    stats, lse = r.out("stats_old", (8,), F32), r.out("lse_old", (n, 2), F32)
    call("pa_mixture_nll_fwd_fin", lib.pa_mixture_nll_fwd_fin(stats, lse, r.p("vocab"), ldv, r.p("ptr"), r.p("sw"), r.p("label"), B, T, V, pad, st))
    fwd = _ext_fwd(r, c, t, d, eps)
    fwd2 = _ext_fwd(r, c, t, d, eps, tag="_again")
    for k, form in enumerate(rp.NLL_BWD_FORMS):
        _ext_bwd(r, c, t, d, eps, fwd, k, form)
    _ext_bwd(r, c, t, d, eps, fwd2, 0, rp.NLL_BWD_FORMS[0], tag="_again")
    w = r.finish()                                                   # (guards of every output, every input bit for bit)
    ck = rp.Checked(c)
    sf, so, ext = w["stats"].reshape(-1), w["stats_old"].reshape(-1), w["ext"].reshape(-1)
    # ---- exact: count, hits, accuracy and row_lse are the un-extended kernel's; the upstream slot is armed; two runs repeat their bits
    ck.exact("count, hits, upstream", _bits(sf[1:4]), _bits(so[1:4]))
    ck.exact("accuracy", _bits(sf[5:6]), _bits(so[5:6]))
    ck.exact("row_lse", _bits(w["lse"]), _bits(w["lse_old"]))
    for key in ("stats", "lse", "ext", "token", "dv0", "dp0", "dsw0"):
        ck.exact(f"{key}: second run", _bits(w[key.replace("0", "_again0") if key[-1] == "0" else key + "_again"]), _bits(w[key]))
    assert float(ext[3]) == 0.0
    # ---- PAD rows and zero-weight rows: +0.0 bit for bit in every gradient, PAD rows in token_nll too
    lab = t["label"]
    padrow = lab == pad
    wrow = torch.from_numpy(R._row_weight(c, wt))
    dead = padrow | (wrow == 0)
    assert not bool(_bits(w["token"].reshape(-1))[padrow].any()), "token_nll at a PAD row"
    for k, (odt, _, _) in enumerate(rp.NLL_BWD_FORMS):
        for q in ("dv", "dp", "dsw"):
            g = _bits(w[f"{q}{k}"]).reshape(n, -1)
            assert not bool(g[dead].any()), f"{c['name']}: {q}{k}: a PAD or zero-weight row is not +0.0 throughout"
        assert not bool(_bits(w[f"dv{k}"])[:, V:].any()), f"{c['name']}: the gradient columns V .. ldv - 1 are not all zero"
    if kind == "B" and B == 3:
        assert bool((~padrow[T:2 * T]).any()) and float(wt[1]) == 0.0           # the zero-weight drawing has real rows
    # ---- parity
    word = _bits(ext[:2]).view(I64).item()
    got = dict(fwd=dict(obj=float(sf[0]), loss=float(sf[4]), nll=word * 2.0 ** -30, mean=float(ext[2]), count=float(sf[1]), hits=float(sf[2]),
                        token=_np(w["token"]).reshape(-1), lse=_np(w["lse"])), bwd=[])
    for k, (odt, gscale, use_up) in enumerate(rp.NLL_BWD_FORMS):
        got["bwd"].append(dict(lse32=w["lse"].clone(), count32=np.float32(float(sf[1])), up32=np.float32(t["up"][0]) if use_up else np.float32(float(sf[3])),
                               dv=_np(w[f"dv{k}"][:, :V]), dp=_np(w[f"dp{k}"]), dsw=_np(w[f"dsw{k}"]).reshape(-1)))
    _report(c, eps, kind, R.verify(c, t, eps, wt, got))


@pytest.mark.parametrize("name", ["nll_B2_T36_V514_ld520_x1", "nll_B3_T256_V1024_ld1024_x30", "nll_B2_T257_V514_ld514_x1"])
def test_per_token_weights_equal_to_a_broadcast_vector_give_the_same_bits(name):
    c = next(c for c in CASES if c["name"] == name)
    t = rp.nll_inputs(c)
    wb = R.ext_weight(c, "B")
    outs = []
    for wt in (wb, wb[:, None].expand(c["B"], c["T"]).contiguous()):
        r = Run(c)
        d = _inputs(r, c, t, wt)
        fwd = _ext_fwd(r, c, t, d, 0.1)
        _ext_bwd(r, c, t, d, 0.1, fwd, 0, rp.NLL_BWD_FORMS[0])
        outs.append(r.finish())
    ck = rp.Checked(c)
    for key in ("stats", "lse", "ext", "token", "dv0", "dp0", "dsw0"):
        ck.exact(key, _bits(outs[1][key]), _bits(outs[0][key]))


def test_bad_arguments_are_rejected_and_nothing_is_written():
    L, ops = _ops()
    c = next(c for c in CASES if c["name"] == "nll_B2_T36_V514_ld520_x1")
    t = rp.nll_inputs(c)
    B, T, V, ldv, pad = c["B"], c["T"], c["V"], c["ldv"], t["pad"]
    n = B * T
    lib, st = L.lib(), L.stream()
    r = Run(c)
    d = _inputs(r, c, t, R.ext_weight(c, "B"))
    r.out("stats", (8,), F32); r.out("lse", (n, 2), F32); r.out("ext", (4,), F32, lead=2); r.out("token", (n,), F32)
    r.out("dv", (n, ldv), F32); r.out("dp", (n, T), F32); r.out("dsw", (n,), F32)
    assert r.p("ext").value % 8 == 0
    good = dict(smoothing=0.1, weight_per_token=0, weight=r.p("weight").value, token_nll=r.p("token").value, ext_stats=r.p("ext").value)
    bad = [dict(smoothing=1.0), dict(smoothing=-0.01), dict(smoothing=float("nan")), dict(smoothing=float("inf")), dict(ext_stats=None),
           dict(ext_stats=r.p("ext").value + 4), dict(weight_per_token=2), dict(weight_per_token=-1)]
    for over in bad:
        e = L.LossExt(**dict(good, **over))
        call(f"pa_mixture_nll_fwd_ext {over}", lib.pa_mixture_nll_fwd_ext(r.p("stats"), r.p("lse"), r.p("vocab"), ldv, r.p("ptr"), r.p("sw"), r.p("label"),
                                                                          B, T, V, pad, C.byref(e), st), rp.PA_EINVAL)
        call(f"pa_mixture_nll_bwd_ext {over}", lib.pa_mixture_nll_bwd_ext(r.p("dv"), r.p("dp"), rp.PA_F32, r.p("dsw"), r.p("stats"), r.p("lse"), r.p("vocab"), ldv,
                                                                          r.p("ptr"), r.p("sw"), r.p("label"), B, T, V, pad, 1.0, None, C.byref(e), st), rp.PA_EINVAL)
    call("pa_mixture_nll_fwd_ext NULL block", lib.pa_mixture_nll_fwd_ext(r.p("stats"), r.p("lse"), r.p("vocab"), ldv, r.p("ptr"), r.p("sw"), r.p("label"),
                                                                         B, T, V, pad, None, st), rp.PA_EINVAL)
    with pytest.raises(L.PlankHipError, match="PA_EINVAL"):          # the ops wrapper hands the library's answer on
        ops.mixture_nll_ext_fwd(d["vocab"], d["ptr"], d["sw"], d["label"], V, pad, smoothing=1.0,
                                out=dict(stats8=_win(r, "stats").view(-1), row_lse=_win(r, "lse"), ext_stats=_win(r, "ext").view(-1)))
    with pytest.raises(ValueError, match="loss_weight"):
        ops.mixture_nll_ext_fwd(d["vocab"], d["ptr"], d["sw"], d["label"], V, pad, weight=torch.ones(B + 1, device="cuda"))
    w = r.finish()
    for key in ("stats", "lse", "ext", "token", "dv", "dp", "dsw"):
        _untouched(w[key], f"{key} of a rejected launch")
