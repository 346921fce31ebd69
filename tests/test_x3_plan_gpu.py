"""The bf16x3 cut plan on the GPU: the real driver of tests/x3_plan_scenarios.py runs every scenario once (milliseconds each) and
  - records what tests/golden/x3_plan.json holds (the golden file was recorded from the commit before the plan functions existed),
  - agrees call by call with the dry run: pa_gemm_split_plan(commit = 0) over the very addresses right before each real call, and
    the dry driver's whole replay (commit = 1) over made-up addresses,
  - every GEMM output matches the float64 product of its operands to the split's precision - a wrong parts pattern or a stale
    image is an error of bf16 size (2^-9), far outside the bound."""
import json

import pytest

import x3_plan_scenarios as X

pytestmark = pytest.mark.gpu

SCENARIOS = X.scenarios()


@pytest.fixture(scope="module")
def runs():
    lib = X.load_lib(dry=True)
    out = {}
    for name, sc in SCENARIOS.items():
        errors = []
        out[name] = (X.real_run(lib, sc, errors, dry_check=True), errors)
    return lib, out


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_real_run_gives_the_recorded_plan(runs, name):
    with open(X.GOLDEN) as f:
        want = json.load(f)[name]
    got = runs[1][name][0]
    assert len(got) == len(want)
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} calls differ, first: {wrong[:2]}"


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_dry_run_equals_the_real_run(runs, name):
    lib, out = runs
    assert X.dry_run(lib, SCENARIOS[name]) == out[name][0]


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_every_product_matches_float64(runs, name):
    from test_kernels_gpu import X3_SPLIT_TOL                    # the bound of test_gemm_x3_layouts_match_float64_to_split_precision
    errors = runs[1][name][1]
    n_gemms = sum(len(c[1]) if c[0] == "group" else 1 for c in SCENARIOS[name]["calls"] if c[0] in ("gemm", "group"))
    print(name, [(k, i, int(taken), f"{err:.3g}") for k, i, taken, err in errors])
    assert errors and len(errors) <= n_gemms
    bad = [(k, i, taken, err) for k, i, taken, err in errors if not err < X3_SPLIT_TOL]
    assert not bad, bad
    if name not in ("declines", "group_declines", "declined_deferred"):
        assert any(taken for _, _, taken, _ in errors)
