"""Every GEMM kernel family of csrc/gemm.hip / gemm8.h (pair, ring, small, wide, tall, big, skinny; f32 and bf16; four operand
layouts; aligned, unaligned and direct-to-LDS variants) held PER ELEMENT to a float64 reference, with guarded outputs and poisoned
operand padding (tests/gemm_parity.py: the checker, the case table and the derivation of the bounds; tests/test_gemm_parity_cpu.py
tests the checker itself on seeded defects).

Every case first asserts the family it is meant for - through pa_gemm_plan before the launch and through pa_gemm_record /
pa_gemm_recorded_kinds after it.  A case that reaches another family is an error, not a skip.

The PA_GEMM_* switches are read once per process, so every switch bundle runs this file as a script in a child process: the child
asserts - before anything touches the device - that its bundle changes the plan of some case against the default plan handed over by
the parent, then runs the same case table with the family expectations taken from its own pa_gemm_plan.

With GEMM_PARITY_REPORT=<file> every case appends `bundle family in out case r(got) r_cpu` to that file (the figures of
profiles/gemm_float64_parity.txt).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gemm_parity as gp                                            # noqa: E402

CASES = gp.cases()
GROUP = gp.group_cases()
DEFER = gp.defer_cases()
REJECT = gp.rejection_cases()
PLANNED = CASES + DEFER + REJECT                                    # what the dry runs plan, in this order
BUNDLE = os.environ.get("GEMM_PARITY_BUNDLE", "")                   # set in a bundle's child process only
_FAULTED = []                                                      # first HIP error of this process, if any
SWITCH_PREFIXES = ("PA_GEMM_", "PA_RESERVE_CUS", "PA_DW_XCD", "PLANK_HIP_LIB")

# bundle -> (environment, {case name: (family, tile_h or None, tile_w or None)} asserted in the child before the device is touched)
BUNDLES = {
    # everything on the pair kernel, direct-to-LDS at single-round shapes (an out_lp, which only the skinny kernel writes, is rejected)
    "v3_0_skinny_0": ({"PA_GEMM_V3": "0", "PA_GEMM_SKINNY": "0"}, "all PAIR"),
    # PA_GEMM_TALL=1 takes every plain Linear of at most 256 tall units, (8320, 512, 64) included: the ring with several units per
    # block is reached by the same shape with B stored [K][N], which the tall kernel does not take
    "v3_2_small_0_wide_1_tall_1": ({"PA_GEMM_V3": "2", "PA_GEMM_SMALL": "0", "PA_GEMM_WIDE": "1", "PA_GEMM_TALL": "1"},
                                   {"pair_bf16_8320x512x64_nt": ("RING", 128, 128), "switch_8300x512x64": ("WIDE", 192, 128),
                                    "small_130x200x64": ("RING", 128, 128), "wide_4100x1030x64": ("WIDE", 128, 256)}),
    "big_2": ({"PA_GEMM_BIG": "2"}, {"switch_4100x264x64": ("BIG", 256, 128), "switch_5400x1530x64": ("BIG", 256, 192)}),
    # PA_GEMM_NST and PA_GEMM_EPRE do not show in pa_gemm_plan_info: they pick the pair kernel's instantiation inside launch_t
    # (csrc/gemm.hip: `deep` / `flat` read sw.nst, the epilogue-prefetch branch reads sw.epre).  The plan change these bundles assert is
    # that of the switch they come with (V3=0 / NOGLDS=1 send the ring shapes to the pair kernel, where NST / EPRE act).
    "v3_0_nst_3": ({"PA_GEMM_V3": "0", "PA_GEMM_NST": "3"}, {"ring_130x200x128_nt": ("PAIR", 128, 128), "small_130x200x64": ("PAIR", 128, 128)}),
    "v3_0_nst_1": ({"PA_GEMM_V3": "0", "PA_GEMM_NST": "1"}, {"ring_130x200x128_nt": ("PAIR", 128, 128), "small_130x200x64": ("PAIR", 128, 128)}),
    "bk_32": ({"PA_GEMM_BK": "32"}, {"ring_130x200x128_nt": ("PAIR", 128, 128), "wide_4100x1030x64": ("PAIR", 128, 128)}),
    "noglds_1_epre_0": ({"PA_GEMM_NOGLDS": "1", "PA_GEMM_EPRE": "0"}, {"ring_130x200x128_nt": ("PAIR", 128, 128), "skinny_bf16_37x200x512": ("PAIR", 128, 128)}),
}


def _L():
    from plankassembly_amd import _lib as L
    return L


def _report(c, family, r, r_cpu):
    path = os.environ.get("GEMM_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(f"{BUNDLE or 'default'} {family} {c['in_dt']} {c['out_dt']} {c['name']} {r:.4g} {r_cpu:.4g}\n")


# ------------------------------------------------------------------------------------------------ one launch, fully checked
class Launch:
    """Operands of a case on the device (windows of guarded buffers) and its argument block."""

    def __init__(self, c):
        L = _L()
        assert not _FAULTED, f"an earlier launch faulted the device ({_FAULTED[0]}): nothing more is started on it"
        self.c, self.t = c, gp.make_tensors(c)
        self.dev = {k: p.buf.to("cuda") for k, p in self.t.items() if isinstance(p, gp.Plane)}
        self.g = gp.gemm_args(L, c, self.t, ptr=lambda key, plane: self.dev[key].data_ptr() + plane.off * plane.buf.element_size())
        self.rc, self.kind, self.info = gp.plan(L, self.g)

    def assert_plan(self, want_family):
        L, c = _L(), self.c
        assert self.rc == 0, f"{c['name']}: pa_gemm_plan rejects the case: {self.rc}"
        if want_family is not None:
            assert self.kind == want_family, f"{c['name']}: planned for {self.kind}, the case is meant for {want_family}"
        eff = L.lib().pa_gemm_effective_splitk(c["K"], self.g.in_dtype, c["splitk"])
        assert gp.eff_splitk(c) == eff == self.info.splitk, (c["name"], gp.eff_splitk(c), eff, self.info.splitk)

    def finish(self, recorded_kinds, want_kinds):
        """After the launch(es): the recorded family, the guards, both tiers, the exact decisions, out_lp."""
        c, t = self.c, self.t
        assert [gp.KINDS[k] for k in recorded_kinds] == want_kinds, f"{c['name']}: launched on {[gp.KINDS[k] for k in recorded_kinds]}, planned {want_kinds}"
        family = want_kinds[0]
        for key, what in (("C", "C"), ("lp", "out_lp"), ("ws", "split-K slabs")):
            if key in t:
                gp.check_sentinels(t[key], self.dev[key], what, c["name"])
        for key in ("A", "B", "bias", "R", "aux"):                 # operands are read-only
            if key in t:
                assert torch.equal(self.dev[key].cpu().view(torch.uint8), t[key].buf.view(torch.uint8)), f"{c['name']}: operand {key} was written"
        got = t["C"].view(self.dev["C"].cpu())
        parts = gp.reference_parts(c, t)
        sk = gp.eff_splitk(c)
        r_cpu = gp.ratio(gp.cpu_float32(c, t), parts["ref"], parts["S"], c["K"], sk)
        tile = (self.info.tile_h or 128, self.info.tile_w or 128)
        r = gp.ratio(got.double().numpy(), parts["ref"], parts["S"], c["K"], sk)
        print(f"{c['name']} [{family}] r(got) = {r:.4g}  r_cpu = {r_cpu:.4g}")
        _report(c, family, r, r_cpu)
        gp.check(got.double().numpy(), parts["ref"], parts["S"], c["K"], sk, c["out_dt"], name=c["name"], family=family, tile=tile, parts=parts, r_cpu=r_cpu)
        if "lp" in t:                                               # the copy is the exact round-to-nearest bf16 image of the f32 output
            lp = t["lp"].view(self.dev["lp"].cpu())
            assert torch.equal(lp.view(torch.int16), got.to(torch.bfloat16).view(torch.int16)), f"{c['name']}: out_lp is not the bf16 image of C"


def _recorded(fn):
    """pa_gemm_record around fn(): the kernel family of every launch it made (as test_kernels_gpu.py _gemm_kinds)."""
    lib = _L().lib()
    torch.cuda.synchronize()
    lib.pa_gemm_record(1)
    try:
        fn()
        torch.cuda.synchronize()
    except RuntimeError as e:                                       # a HIP error after a launch: the later cases of this process fail unstarted
        _FAULTED.append(str(e).splitlines()[0])
        raise
    finally:
        n = lib.pa_gemm_record(0)
    kinds = (C.c_int32 * max(n, 1))()
    nk = lib.pa_gemm_recorded_kinds(C.cast(kinds, C.c_void_p), n)
    return [kinds[i] for i in range(nk)]


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case(c):
    L = _L()
    run = Launch(c)
    if BUNDLE and run.rc != 0:
        # a bundle that switches a case's only kernel off (out_lp without the skinny kernel): rejected as planned, nothing stored
        assert c["lp"] and run.rc == -1 and L.lib().pa_gemm(C.byref(run.g), L.stream()) == -1, (c["name"], run.rc)
        torch.cuda.synchronize()
        assert torch.equal(run.dev["C"].cpu(), run.t["C"].buf) and torch.equal(run.dev["lp"].cpu(), run.t["lp"].buf)
        return
    run.assert_plan(None if BUNDLE else c["family"])                # (a bundle's child: the expectation is its own plan)
    kinds = _recorded(lambda: L.check(L.lib().pa_gemm(C.byref(run.g), L.stream()), "pa_gemm"))
    run.finish(kinds, [run.kind])


@pytest.mark.gpu
def test_skinny_rejections_on_the_device():
    """The skinny kernel takes no gate and no dropout: such a launch runs on another family, and with an out_lp - which only the skinny
    kernel writes - it is rejected, by the plan and by pa_gemm alike, before anything is stored."""
    L = _L()
    for c in REJECT:
        if not c["lp"]:
            continue
        run = Launch(c)
        assert run.rc == -1, (c['name'], run.rc)
        assert L.lib().pa_gemm(C.byref(run.g), L.stream()) == -1
        torch.cuda.synchronize()
        assert torch.equal(run.dev["C"].cpu(), run.t["C"].buf) and torch.equal(run.dev["lp"].cpu(), run.t["lp"].buf)


def _reduce(items):
    from plankassembly_amd import ops
    L = _L()
    descs = (ops.ReduceDesc * len(items))()
    for d, (run, sk) in zip(descs, items):
        d.ws, d.out = run.g.ws, run.g.C
        d.rows, d.cols, d.ld_out, d.splitk = run.c["M"], run.c["N"], run.t["C"].ld, sk
    L.check(L.lib().pa_splitk_reduce_many(C.cast(descs, C.c_void_p), len(items), L.stream()), "pa_splitk_reduce_many")


@pytest.mark.gpu
def test_grouped_weight_gradients():
    """pa_gemm_group: three dW products of different shapes in one ring launch, one of them split with the deferred reduction."""
    L = _L()
    runs = [Launch(c) for c in GROUP]
    args = (L.GemmArgs * len(runs))()
    for i, run in enumerate(runs):
        assert L.lib().pa_gemm_effective_splitk(run.c["K"], run.g.in_dtype, run.c["splitk"]) == gp.eff_splitk(run.c)
        args[i] = run.g
    assert any(gp.eff_splitk(r.c) > 1 for r in runs)

    def go():
        L.check(L.lib().pa_gemm_group(C.cast(args, C.c_void_p), len(runs), L.stream()), "pa_gemm_group")
        _reduce([(r, gp.eff_splitk(r.c)) for r in runs if gp.eff_splitk(r.c) > 1])
    kinds = _recorded(go)
    assert [gp.KINDS[k] for k in kinds] == ["RING"] * len(runs)
    for run in runs:
        run.info.tile_h = run.info.tile_w = 128
        run.finish([1], ["RING"])


@pytest.mark.gpu
def test_deferred_splitk_reduction():
    """pa_gemm(splitk_defer = 1) writes only its slabs (C stays untouched); pa_splitk_reduce_many sums them."""
    L = _L()
    runs = [Launch(c) for c in DEFER]
    kinds = []
    for run in runs:
        run.assert_plan(None if BUNDLE else run.c["family"])
        kinds.append(_recorded(lambda: L.check(L.lib().pa_gemm(C.byref(run.g), L.stream()), "pa_gemm")))
        assert torch.equal(run.dev["C"].cpu(), run.t["C"].buf), f"{run.c['name']}: the deferred launch wrote C"
    _reduce([(r, gp.eff_splitk(r.c)) for r in runs])
    torch.cuda.synchronize()
    for run, k in zip(runs, kinds):
        run.finish(k, [run.kind])


# ------------------------------------------------------------------------------------------------ plans without a device, bundles
def plans_of_this_process():
    return gp.plan_rows(_L(), PLANNED)


_DEFAULT_PLANS = []


def default_plans():
    """The plan of every case under default switches, from a child process with the PA_GEMM_* environment cleared."""
    if not _DEFAULT_PLANS:
        env = {k: v for k, v in os.environ.items() if not k.startswith(SWITCH_PREFIXES) and k != "GEMM_PARITY_BUNDLE"}
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plan"], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        _DEFAULT_PLANS.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("[")][-1]))
    return _DEFAULT_PLANS[0]


def _bundle_child(bundle, default_rows):
    """In the child, before anything touches the device: the bundle changes the plan (kind, grid, block or units) of at least one case,
    and sends the cases it exists for to the kernel it exists for."""
    rows = plans_of_this_process()
    assert len(rows) == len(default_rows)
    changed = [c["name"] for c, r, d in zip(PLANNED, rows, default_rows) if r[:5] != d[:5]]
    assert changed, f"bundle {bundle}: the plan of no case differs from the default plan"
    want = BUNDLES[bundle][1]
    by_name = {c["name"]: r for c, r in zip(PLANNED, rows)}
    if want == "all PAIR":
        off = [(c["name"], r[:2]) for c, r in zip(PLANNED, rows) if r[:2] != ([-1, None] if c["lp"] else [0, "PAIR"])]
        assert not off, off
        return
    for name, (fam, th, tw) in want.items():
        r = by_name[name]
        assert r[0] == 0 and (r[1], r[6], r[7]) == (fam, th, tw), f"bundle {bundle}: {name} planned as {r}"
    if bundle.startswith("v3_2"):
        r = by_name["pair_bf16_8320x512x64_nt"]
        assert r[4] > r[2], f"bundle {bundle}: {r} is not several units per block"


@pytest.mark.gpu
@pytest.mark.parametrize("bundle", list(BUNDLES))
def test_switch_bundle_in_a_child_process(bundle, tmp_path):
    default_file = tmp_path / "default_plans.json"
    default_file.write_text(json.dumps(default_plans()))
    env = {k: v for k, v in os.environ.items() if not k.startswith(SWITCH_PREFIXES)}
    env.update(BUNDLES[bundle][0], GEMM_PARITY_BUNDLE=bundle, PYTHONPATH=REPO + os.pathsep + env.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--bundle", bundle, str(default_file)], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=900)
    # (a child that dies of a signal has a negative return code: it fails here, once; nothing is retried)
    assert r.returncode == 0, f"bundle {bundle}: exit {r.returncode}\n" + r.stdout[-4000:] + r.stderr[-2000:]
    assert f"{len(CASES) + 1} passed" in r.stdout, r.stdout[-2000:]


if __name__ == "__main__":
    if sys.argv[1] == "--plan":
        print(json.dumps(plans_of_this_process()))
        sys.exit(0)
    if sys.argv[1] == "--bundle-plan":                              # the child's plan assertions alone (no device needed)
        _bundle_child(sys.argv[2], json.load(open(sys.argv[3])))
        print("bundle plan ok")
        sys.exit(0)
    assert sys.argv[1] == "--bundle" and BUNDLE == sys.argv[2]
    _bundle_child(sys.argv[2], json.load(open(sys.argv[3])))
    sys.exit(pytest.main(["-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "test_case or test_deferred_splitk_reduction"]))
