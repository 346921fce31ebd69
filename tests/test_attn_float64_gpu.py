"""Every attention kernel of csrc/attention.hip, attention5.h and attention_x3.h held PER ELEMENT to a float64 reference, forward and
backward, with guarded outputs and poisoned operand padding (tests/attn_parity.py: the checker, the case table, the input regimes and
the derivation of the bounds; tests/test_attn_parity_cpu.py tests the checker itself on seeded defects).

The C ABI is called directly (pa_attn_args), so the test owns every buffer.  Every case first asserts the kernels it is meant for through
pa_attn_plan; a case that reaches other kernels is an error, not a skip.  The backward kernels receive the forward kernel's own stored
o and lse, as the model gives them.

The PA_ATTN_* / PA_X3_* switches are read once per process, so every switch bundle runs this file as a script in a child process, one
after another, each under its own timeout.  After a child that ended on a signal or at its timeout nothing more is started on the
device: the remaining bundle tests fail unstarted.  The last test collects the kernel names pa_attn_plan reported for every launched
case of every bundle and holds the set to `names` of tests/golden/attn_plan.json: every kernel is compared with float64 at least once.

With ATTN_PARITY_REPORT=<file> every case appends `bundle case output r(got) r(emulation)` to that file (the figures of
profiles/attn_float64_parity.txt).
"""
import ctypes as C
import json
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

import attn_parity as ap                                            # noqa: E402
import gemm_parity as gp                                            # noqa: E402

BUNDLE = os.environ.get("ATTN_PARITY_BUNDLE", "default")            # set in a bundle's child process only
ALL = ap.cases()
CASES = [c for c in ALL if c["bundle"] == BUNDLE]
CHILD_BUNDLES = [b for b in ap.BUNDLES if b != "default"]
SWITCH_PREFIXES = ("PA_ATTN_", "PA_X3_")
CHILD_TIMEOUT = 300
_FAULTED = []                                                      # first HIP error of this process, if any
_CHILD_FAULT = []                                                  # first bundle whose child ended on a signal or at its timeout
_LAUNCHED = {}                                                     # bundle -> kernel names planned for the cases that were launched


def _L():
    from plankassembly_amd import _lib as L
    return L


def _report(c, rs):
    path = os.environ.get("ATTN_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            for what, (r, r_emu) in rs.items():
                f.write(f"{BUNDLE} {c['name'].split(':', 1)[1]} {what} {r:.4g} {r_emu:.4g}\n")


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                       # a HIP error after a launch: the later cases of this process fail unstarted
        _FAULTED.append(f"{what}: {str(e).splitlines()[0]}")
        raise


def run_case(c):
    L = _L()
    assert not _FAULTED, f"an earlier launch faulted the device ({_FAULTED[0]}): nothing more is started on it"
    t = ap.Tensors(c)
    dev = {k: p.buf.to("cuda") for k, p in t.planes.items()}
    aux_t = {}
    if t.kpm is not None:
        aux_t["kpm"] = torch.from_numpy(t.kpm).to("cuda")
    if t.cu is not None:
        aux_t["cu"] = t.cu.to("cuda")
    if t.order is not None:
        aux_t["order"] = t.order.to("cuda")
    ws_bytes = 0
    if c["ws"]:
        ws_bytes = int(L.lib().pa_attn_ws_bytes(t.Rq, c["B"], c["H"], c["Lq"]))
        assert ws_bytes > 0, f"{c['name']}: the range-block scratch has no size under this process's switches"
        aux_t["ws"] = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    aux = {k: v.data_ptr() for k, v in aux_t.items()}
    a = ap.attn_args(L, c, t, ptr=lambda key, plane, col=0: dev[key].data_ptr() + (plane.off + col) * plane.buf.element_size(), aux=aux,
                     ws_bytes=ws_bytes)
    want_f, want_b = ap.kernel_names(c)
    L.check(L.lib().pa_attn_split_config(c["x3"]), "pa_attn_split_config")
    try:
        rc_f, names_f, info_f = ap.plan(L, a, 0)
        rc_b, names_b, info_b = ap.plan(L, a, 1)
        assert (rc_f, rc_b) == (0, 0), f"{c['name']}: pa_attn_plan rejects the case: {rc_f}, {rc_b}"
        assert names_f == want_f and names_b == want_b, f"{c['name']}: planned for {names_f} / {names_b}, the case is meant for {want_f} / {want_b}"
        if BUNDLE == "no_v5_x3_parts" and c["x3"] and c["Lk"] >= 128:  # PA_X3_PARTS=2: the streamed side cut in two, partial sums added with atomics
            assert info_b.parts_q == 2 and (info_b.parts_kv == 2 or c["Lk"] > c["Lq"]), (c["name"], info_b.parts_q, info_b.parts_kv)
        if c["ws"]:
            assert info_f.balanced == 2 and info_b.balanced == 2 and info_f.sp_slots > 0, (c["name"], info_f.balanced, info_b.balanced, info_f.sp_slots)
        for rep in range(2 if c["ws"] else 1):                      # range blocks: twice on one scratch buffer
            L.check(L.lib().pa_attn_fwd(C.byref(a), L.stream()), "pa_attn_fwd")
            _sync(c["name"] + " forward")
            L.check(L.lib().pa_attn_bwd(C.byref(a), L.stream()), "pa_attn_bwd")
            _sync(c["name"] + " backward")
    finally:
        L.check(L.lib().pa_attn_split_config(0), "pa_attn_split_config")
    _LAUNCHED.setdefault(BUNDLE, set()).update(names_f + names_b)
    if os.environ.get("ATTN_PARITY_NAMES"):                         # a bundle's child: for the parent's coverage test
        with open(os.environ["ATTN_PARITY_NAMES"], "a") as f:
            f.write("".join(n + "\n" for n in names_f + names_b))
    if c["ws"]:
        nt = int(L.lib().pa_attn_ws_ticket_bytes(ws_bytes))
        assert nt > 0 and int(aux_t["ws"][:nt].view(torch.int32).abs().sum()) == 0, f"{c['name']}: ticket words are not zero after the launches"
    # ---- windows and operands
    for key in ("o", "dq", "dk", "dv", "lse", "delta"):
        gp.check_sentinels(t.planes[key], dev[key], key, c["name"])
    for key in ("xq", "xkv", "do"):
        if key in dev:
            assert torch.equal(dev[key].cpu().view(torch.uint8), t.planes[key].buf.view(torch.uint8)), f"{c['name']}: operand {key} was written"
    H, dh = c["H"], c["dh"]
    got = {}
    for key in ("o", "dq", "dk", "dv"):
        got[key] = t.planes[key].view(dev[key].cpu())[0].to(torch.float64).numpy().reshape(-1, H, dh)
    lse = t.planes["lse"].view(dev["lse"].cpu()).reshape(c["B"], H, c["Lq"]).clone()
    valid = torch.from_numpy(t.lse_valid())
    pattern_bits = torch.full((1,), ap.PATTERN, dtype=torch.float32).view(torch.int32)[0]
    assert bool((lse.view(torch.int32)[~valid] == pattern_bits).all()), f"{c['name']}: lse rows past a packed element's length were written"
    lse[~valid] = 0.0
    got["lse"] = lse.to(torch.float64).numpy()
    ref = ap.reference(c, t)
    emu = ap.stored(c, ap.emulate(c, t))
    for what in ap.OUTPUTS:                                         # every figure before any assertion
        eps = ap.eps_of(c, what)
        print(f"{c['name']} {what}: r(got) = {ap.ratio(got[what], ref[what], ref['S_' + what], eps):.4g}  "
              f"r(emulation) = {ap.ratio(emu[what], ref[what], ref['S_' + what], eps):.4g}")
    rs = {what: (ap.ratio(got[what], ref[what], ref["S_" + what], ap.eps_of(c, what)),
                 ap.ratio(emu[what], ref[what], ref["S_" + what], ap.eps_of(c, what))) for what in ap.OUTPUTS}
    _report(c, rs)
    ap.check_all(c, got, ref, emu)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["name"].split(":", 1)[1] for c in CASES])
def test_case(c):
    run_case(c)


def _names_file(tmp_dir, bundle):
    return os.path.join(str(tmp_dir), f"launched_{bundle}.txt")


@pytest.fixture(scope="module")
def names_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("attn_parity_names")


@pytest.mark.gpu
@pytest.mark.parametrize("bundle", CHILD_BUNDLES)
def test_switch_bundle_in_a_child_process(bundle, names_dir):
    assert not _CHILD_FAULT, f"not run: an earlier child faulted ({_CHILD_FAULT[0]})"
    assert not _FAULTED, f"not run: an earlier launch of this process faulted the device ({_FAULTED[0]})"
    n = sum(c["bundle"] == bundle for c in ALL)
    env = {k: v for k, v in os.environ.items() if not k.startswith(SWITCH_PREFIXES)}
    env.update(ap.BUNDLES[bundle], ATTN_PARITY_BUNDLE=bundle, ATTN_PARITY_NAMES=_names_file(names_dir, bundle),
               PYTHONPATH=REPO + os.pathsep + env.get("PYTHONPATH", ""))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--bundle", bundle], cwd=REPO, env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _CHILD_FAULT.append(f"bundle {bundle}: no end after {CHILD_TIMEOUT} s")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _CHILD_FAULT.append(f"bundle {bundle}: exit {r.returncode}")
    assert r.returncode == 0, f"bundle {bundle}: exit {r.returncode}\n" + r.stdout[-4000:] + r.stderr[-2000:]
    assert f"{n} passed" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
def test_every_kernel_is_compared_with_float64(names_dir):
    """The kernels planned for the launched cases of this process and of every bundle's child are all the kernels there are."""
    golden = set(json.load(open(os.path.join(REPO, "tests", "golden", "attn_plan.json")))["names"])
    seen = set(_LAUNCHED.get("default", ()))
    missing_bundles = []
    for bundle in CHILD_BUNDLES:
        path = _names_file(names_dir, bundle)
        if os.path.exists(path):
            seen |= set(open(path).read().splitlines())
        else:
            missing_bundles.append(bundle)
    assert not missing_bundles, f"no record of the launched kernels of {missing_bundles}: this test runs after the cases and the bundles of this file"
    assert seen == golden, f"never compared with float64: {sorted(golden - seen)}; unknown to tests/golden/attn_plan.json: {sorted(seen - golden)}"


def planned_everywhere():
    """Without a device: {bundle: kernel names of its cases' expectations} - what the coverage test will see when every case launches."""
    out = {}
    for c in ALL:
        f, b = ap.kernel_names(c)
        out.setdefault(c["bundle"], set()).update(f + b)
    return out


if __name__ == "__main__":
    assert sys.argv[1] == "--bundle" and BUNDLE == sys.argv[2]
    sys.exit(int(pytest.main(["-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "test_case"])))
