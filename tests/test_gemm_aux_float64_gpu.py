"""The GEMM companion kernels at the end of csrc/gemm.hip - pa_colsum, pa_colsum_many, pa_splitk_reduce_many, pa_transpose_many,
pa_segment_tail, pa_ln_fold_weights(_f32), pa_gemm_norm_a, pa_gemm_ln - held PER ELEMENT to a float64 reference at every branch of their
host code, with guarded outputs, poisoned input padding and seeded accumulators (tests/gemm_aux_parity.py: the checker, the case table, the
restated dispatch and the derivation of the bounds; tests/test_gemm_aux_parity_cpu.py tests the checker itself on seeded defects).

Calls go through plankassembly_amd._lib with pointers into the guarded buffers.  Every case first asserts that the restated dispatch puts it
on the branch it is meant for (pa_gemm_norm_a: that pa_gemm_plan(args, ext) names its family).  The first HIP error of a process is
remembered and nothing more is launched after it.

The f32 atomic forms are reached in-process as the bf16x3 train step reaches them: pa_gemm_split_config(1, ..) around the call, inside a
split context of the test's own.  PA_DETERMINISTIC is read once per process, so PA_DETERMINISTIC=1 (bf16 ordered) and PA_DETERMINISTIC=0
(f32 atomic outside the bf16x3 mode) each run this file as a script in a fresh child process: the child asserts - before anything touches
the device - that its switch changes the restated dispatch of some case, then runs the cases whose dispatch it changes.

With GEMM_AUX_PARITY_REPORT=<file> every case appends `branch kernel dtype case r(got) r_cpu` (the figures of
profiles/gemm_aux_float64_parity.txt).
"""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gemm_aux_parity as gap                                       # noqa: E402

pytestmark = pytest.mark.gpu

BUNDLE = os.environ.get("GEMM_AUX_PARITY_BUNDLE", "")               # set in a bundle's child process only
ENV = {k: os.environ[k] for k in gap.SWITCHES if k in os.environ}   # the switches of this process, as the library reads them
ALL = gap.all_cases()
CASES = gap.switch_cases(ENV) if BUNDLE else ALL
_FAULTED = []                                                      # first HIP error of this process, if any
_CHILD_DIED = []                                                   # a child that ended on a signal or at its time limit
X3_WS_BYTES = 1 << 20


def _L():
    from plankassembly_amd import _lib as L
    return L


def call(what, rc, want=0):
    if rc > 0:
        _FAULTED.append(f"{what}: hipError {rc}")
    assert rc == want, f"{what} returned {rc} ({_L()._ERR.get(rc, 'a raw HIP error code')}), want {want}"


def _report(c, rows):
    path = os.environ.get("GEMM_AUX_PARITY_REPORT")
    branch = BUNDLE or ("x3" if c.get("x3") else "default")
    for kernel, dt, r, r_cpu in rows:
        fig = "- -" if r is None else f"{r:.4g} {r_cpu:.4g}"       # (-: no f32 output of that kernel in the case, so no r)
        print(f"{c['name']} [{branch} {kernel} {dt}] r(got) r_cpu = {fig}")
        if path:
            with open(path, "a") as f:
                f.write(f"{branch} {kernel} {dt} {c['name']} {fig}\n")


def _vp(x):
    return None if x is None else C.c_void_p(x)


# ------------------------------------------------------------------------------------------------ the launches of one case
def launch_colsum(c, t, G, P, lib, st):
    lead, ldx = gap.colsum_layout(c)
    assert ((P("X") & 15) == 0) == (lead == 0) and ldx == G["X"].ld, "the operand does not have the alignment the restated dispatch assumes"
    part = torch.empty(int(lib.pa_colsum_ws_floats(c["M"], c["N"])), dtype=torch.float32, device="cuda")
    call("pa_colsum", lib.pa_colsum(P("X"), gap.PADT[c["dt"]], c["M"], c["N"], ldx, P("out"), c["acc"], part.data_ptr(), st))


def _colsum_descs(descs, G, P, pre=""):
    arr = (gap.ColsumDesc * max(len(descs), 1))()
    for i, (M, N) in enumerate(descs):
        assert (P(f"{pre}X{i}") & 15) == 0
        arr[i] = gap.ColsumDesc(P(f"{pre}X{i}"), P(f"{pre}out{i}"), M, N, G[f"{pre}X{i}"].ld, 0)
    return arr


def _reduce_descs(descs, G, P, pre=""):
    arr = (gap.ReduceDesc * max(len(descs), 1))()
    for i, (rows, cols, ld, sk) in enumerate(descs):
        assert (P(f"{pre}ws{i}") & 15) == 0 and (P(f"{pre}red{i}") & 15) == 0 and G[f"{pre}red{i}"].ld == ld
        arr[i] = gap.ReduceDesc(P(f"{pre}ws{i}"), P(f"{pre}red{i}"), rows, cols, ld, sk)
    return arr


def launch_colsum_many(c, t, G, P, lib, st):
    arr = _colsum_descs(c["descs"], G, P)
    call("pa_colsum_many", lib.pa_colsum_many(C.cast(arr, C.c_void_p), len(c["descs"]), gap.PADT[c["dt"]], st))


def launch_reduce(c, t, G, P, lib, st):
    arr = _reduce_descs(c["descs"], G, P)
    call("pa_splitk_reduce_many", lib.pa_splitk_reduce_many(C.cast(arr, C.c_void_p), len(c["descs"]), st))


def launch_transpose(c, t, G, P, lib, st):
    plan = gap.dispatch(c, ENV)
    arr, begin = (gap.TrDesc * len(c["descs"]))(), 0
    for i, (rows, cols, xs, xd, lead) in enumerate(c["descs"]):
        es = G[f"dst{i}"].buf.element_size()
        assert (P(f"src{i}") & 7) == 0 and ((P(f"dst{i}") & 7) == 0) == ((lead * es) % 8 == 0), "alignment the restated dispatch assumes"
        arr[i] = gap.TrDesc(P(f"src{i}"), P(f"dst{i}"), rows, cols, G[f"src{i}"].ld, G[f"dst{i}"].ld, begin, 0)
        begin += plan["tiles"][i]
    assert begin == plan["total_tiles"]
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to("cuda")      # the descriptors live in device memory
    call("pa_transpose_many", lib.pa_transpose_many(dev.data_ptr(), len(c["descs"]), begin, gap.PADT[c["dt"]], st))
    torch.cuda.synchronize()                                        # (dev stays alive until the kernel has read it)


def launch_tail(c, t, G, P, lib, st):
    ln = (gap.LnFinishDesc * max(len(c["ln"]), 1))()
    for i, (n, dz) in enumerate(c["ln"]):
        ln[i] = gap.LnFinishDesc(P(f"partial{i}"), P(f"ln{i}_0"), P(f"ln{i}_1"), P(f"ln{i}_2") if dz else None, n, 0)
    cs, rd = _colsum_descs(c["cs"], G, P), _reduce_descs(c["rd"], G, P)
    call("pa_segment_tail", lib.pa_segment_tail(C.cast(ln, C.c_void_p) if c["ln"] else None, len(c["ln"]), c["d"], C.cast(cs, C.c_void_p) if c["cs"] else None,
                                                len(c["cs"]), gap.PADT[c["dt"]], C.cast(rd, C.c_void_p) if c["rd"] else None, len(c["rd"]), st))
    if c["rd"]:
        alone = _reduce_descs(c["rd"], G, P, pre="alone_")
        call("pa_splitk_reduce_many", lib.pa_splitk_reduce_many(C.cast(alone, C.c_void_p), len(c["rd"]), st))


def launch_fold(c, t, G, P, lib, st):
    fn = lib.pa_ln_fold_weights if c["dt"] == "bf16" else lib.pa_ln_fold_weights_f32
    call(fn.__name__, fn(_vp(P("Wf")), _vp(P("u")), _vp(P("v")), _vp(P("W")), _vp(P("bias")) if c["bias"] else None, _vp(P("gamma")), _vp(P("beta")),
                         C.c_int32(c["N"]), C.c_int32(c["K"]), st))


def launch_norm_a(c, t, G, P, lib, st):
    L = _L()
    rc, kind, info = gap.norm_a_plan(L, c, G, P)
    assert rc == 0 and kind == gap.FAMILY[c["form"]], f"{c['name']}: pa_gemm_plan: status {rc}, family {kind}; the case is meant for {gap.FAMILY[c['form']]}"
    assert gap.norm_a_dry_run(L, c)[:2] == (rc, kind), "the dry run on made-up addresses of the same alignment plans another kernel"
    g, x = gap.norm_a_args(L, c, G, P)
    call("pa_gemm_norm_a", lib.pa_gemm_norm_a(C.byref(g), C.byref(x), st))


def launch_gemm_ln(c, t, G, P, lib, st):
    L = _L()
    opt = lambda key, on=True: P(key) if (on and key in G) else None

    def args(Z, Y, mean, rstd):
        a = L.GemmLnArgs()
        a.A, a.W, a.bias, a.R, a.Z, a.Y, a.gamma, a.beta, a.mean, a.rstd = P("A"), P("W"), opt("bias"), opt("R"), Z, Y, P("gamma"), P("beta"), mean, rstd
        a.M, a.N, a.K, a.lda, a.ldw, a.ldr, a.ldz, a.ldy = c["M"], 512, c["K"], G["A"].ld, G["W"].ld, 516, 516, 516
        a.eps, a.drop_p, a.drop_seed = c["eps"], c["drop"], gap.GL_SEED
        return a
    call("pa_gemm_ln", lib.pa_gemm_ln(C.byref(args(P("Z"), P("Y"), P("mean"), P("rstd"))), st))
    call("pa_gemm_ln", lib.pa_gemm_ln(C.byref(args(opt("Z2"), P("Y2"), opt("mean2"), opt("rstd2"))), st))      # Z / mean / rstd NULL as the case says
    if c["drop"]:                                                   # the two-launch path
        g = L.GemmArgs()
        g.A, g.B, g.C, g.bias, g.R = P("A"), P("W"), P("Z0"), opt("bias"), opt("R")
        g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.ldr = c["M"], 512, c["K"], G["A"].ld, G["W"].ld, 512, 516
        g.batch, g.a_kcontig, g.b_kcontig, g.in_dtype, g.out_dtype = 1, 1, 1, gap.PA_BF16, gap.PA_BF16
        g.alpha, g.aux_scale, g.splitk, g.drop_p, g.drop_seed = 1.0, 1.0, 1, c["drop"], gap.GL_SEED
        call("pa_gemm", lib.pa_gemm(C.byref(g), st))
        call("pa_layernorm_fwd", lib.pa_layernorm_fwd(P("Y0"), P("Z0"), P("gamma"), P("beta"), P("mean0"), P("rstd0"), c["M"], 512, c["eps"], gap.PA_BF16, st))


LAUNCH = {"colsum": launch_colsum, "colsum_many": launch_colsum_many, "reduce": launch_reduce, "transpose": launch_transpose, "tail": launch_tail,
          "fold": launch_fold, "norm_a": launch_norm_a, "gemm_ln": launch_gemm_ln}


def run_on_device(c, t, G):
    """The buffers of a case after its launches on the device."""
    assert not _FAULTED, f"an earlier launch faulted the device ({_FAULTED[0]}): nothing more is started on it"
    L = _L(); lib = L.lib()
    dev = {k: g.buf.to("cuda") for k, g in G.items()}
    P = lambda key: dev[key].data_ptr() + G[key].byte_offset()
    mode = contextlib.nullcontext()
    if c.get("x3"):
        ws = torch.empty(X3_WS_BYTES, dtype=torch.uint8, device="cuda")
        mode = gap.x3_mode(lib, ws.data_ptr(), X3_WS_BYTES)
    try:
        with mode:
            LAUNCH[c["kernel"]](c, t, G, P, lib, L.stream())
        torch.cuda.synchronize()
    except RuntimeError as e:                                       # a HIP error after a launch: the later cases of this process fail unstarted
        _FAULTED.append(str(e).splitlines()[0])
        raise
    assert lib.pa_gemm_split_active() == 0
    return {k: d.cpu() for k, d in dev.items()}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case(c):
    if BUNDLE:                                                      # a bundle's child: the expectation is the restated dispatch under its switches
        assert gap.dispatch(c, ENV) != gap.dispatch(c)
    else:
        ok, plan = gap.on_branch(c, ENV)
        assert ok, f"{c['name']}: meant for {c['branch']}, dispatched as {plan}"
    _, inputs, build, _, verify = gap.GROUPS[c["kernel"]]
    t = inputs(c)
    G = build(c, t)
    _report(c, verify(c, t, G, run_on_device(c, t, G), ENV))


def test_calls_outside_the_contract_are_rejected_before_any_launch():
    for name, fn, want in gap.rejections(_L()):
        rc = fn()
        assert rc == want, f"{name}: status {rc}, want {want}"


# ------------------------------------------------------------------------------------------------ PA_DETERMINISTIC, one child each
def _bundle_child(bundle):
    """In the child, before anything touches the device: the switch is set as the bundle says and changes the restated dispatch of a case."""
    assert ENV == gap.BUNDLES[bundle], (ENV, gap.BUNDLES[bundle])
    assert CASES, f"bundle {bundle}: the restated dispatch of no case differs from the default"
    dt, ordered = {"deterministic_1": ("bf16", True), "deterministic_0": ("f32", False)}[bundle]
    for kernel in ("colsum", "colsum_many", "tail"):
        assert any(c["kernel"] == kernel and c["dt"] == dt and gap.dispatch(c, ENV)["ordered"] == ordered and gap.dispatch(c)["ordered"] != ordered for c in CASES), (bundle, kernel)
    assert all(c["kernel"] in ("colsum", "colsum_many", "tail") and c["dt"] == dt for c in CASES)


@pytest.mark.parametrize("bundle", list(gap.BUNDLES))
def test_switch_bundle_in_a_child_process(bundle):
    assert not _FAULTED, f"an earlier launch faulted the device ({_FAULTED[0]}): no child is started"
    assert not _CHILD_DIED, f"the child of bundle {_CHILD_DIED[0]} ended on a signal or at its time limit: no further child is started"
    env = {k: v for k, v in os.environ.items() if k not in gap.SWITCHES}
    env.update(gap.BUNDLES[bundle], GEMM_AUX_PARITY_BUNDLE=bundle, PYTHONPATH=REPO + os.pathsep + env.get("PYTHONPATH", ""))
    n_cases = len(gap.switch_cases(gap.BUNDLES[bundle]))
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
