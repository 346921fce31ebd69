"""The row-kernel parity checker (tests/rowops_parity.py) tested on the CPU: at the case table's own shapes every float32 restatement passes
it, every seeded defect is caught by some case of its kernel group, the conditions on the inputs hold on the reference alone, and the
restated host dispatch puts every case on the branch it is meant for (and every switch bundle changes the dispatch of some case).
No GPU and no library needed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_parity as rp                                          # noqa: E402

CASES = rp.all_cases()
BY_GROUP = {g: [c for c in CASES if c["kernel"] == g] for g in rp.GROUPS}
_INPUTS = {}


def inputs(c):
    if c["name"] not in _INPUTS:
        _INPUTS[c["name"]] = rp.GROUPS[c["kernel"]][0](c)
    return _INPUTS[c["name"]]


def test_every_group_has_cases_and_every_case_is_on_its_branch():
    for g, cs in BY_GROUP.items():
        assert cs, g
    for c in CASES:
        ok, got = rp.on_branch(c)
        assert ok, f"{c['name']}: meant for {c['branch']}, the restated dispatch gives {got}"


def test_case_table_covers_what_the_kernels_branch_on():
    ln = BY_GROUP["ln"]
    for d in rp.LN_D:
        rows = {c["rows"] for c in ln if c["d"] == d}
        assert rows & {1, 5} and rows & {37, 270}, (d, rows)
        assert {c["dt"] for c in ln if c["d"] == d} == {"f32", "bf16"}
    assert {c["eps"] for c in ln} == {1e-5, 1.0} and {c["kind"] for c in ln} == {"unit", "offset"}
    assert {(c["dzsum"], c["drop_p"]) for c in ln} == {(0, 0.0), (0, 0.2), (1, 0.0), (1, 0.2)}
    assert {rp.dispatch(c)["nv"] for c in ln} == {1, 2, 4, 8}
    assert any(rp.dispatch(c)["lds_over_64k"] for c in ln)                                  # d > 1364: more than 64 KB of dynamic LDS
    assert {(c["dt"], rp.dispatch(c)["bwd"]) for c in ln if c["d"] == 512} >= {("f32", "bwd512"), ("bf16", "bwd512"), ("bf16", "generic")}
    assert any(rp.dispatch(c)["stride_loop"] for c in BY_GROUP["gelu"]) and any(rp.dispatch(c)["stride_loop"] for c in BY_GROUP["adam"])
    assert {rp.dispatch(c)["path"] for c in BY_GROUP["nll"]} == {"fast", "strided"}
    assert any(rp.dispatch(c)["lds"] > 65536 for c in BY_GROUP["embed_in"])
    assert {rp.dispatch(c)["kernel"] for c in BY_GROUP["embed_seg"]} == {"ordered4", "one_group_ordered", "atomic"}
    assert {ch for c in BY_GROUP["embed_seg"] for ch in rp.dispatch(c)["ch"]} == {0, 1}
    pk = [rp.dispatch(c) for c in BY_GROUP["pack_rows"]]
    assert {p["path"] for p in pk} == {"fused", "four_kernel"} and {p["order"] for p in pk} == {"rank", "iota"}
    assert max(p["scan_rounds"] for p in pk if p["path"] == "fused") > 1 and max(p["passes"] for p in pk) == 2
    gr = [rp.dispatch(c) for c in BY_GROUP["group_rows"]]
    assert any(p["set_attribute"] for p in gr) and any(p["scan_rounds"] == 2 for p in gr) and any(p["refetch"] for p in gr)


@pytest.mark.parametrize("bundle", list(rp.BUNDLES))
def test_every_switch_bundle_changes_the_dispatch_of_some_case(bundle):
    changed = [c["name"] for c in CASES if rp.dispatch(c, rp.BUNDLES[bundle]) != rp.dispatch(c)]
    assert changed, bundle
    if bundle == "lnb512_0":
        assert all(rp.dispatch(c, rp.BUNDLES[bundle])["bwd"] == "generic" for c in BY_GROUP["ln"])
        assert any(c["dt"] == "f32" and c["d"] == 512 for c in CASES if c["name"] in changed)
    else:
        assert all(n.startswith("embed_seg") for n in changed)


@pytest.mark.parametrize("group", list(rp.GROUPS))
def test_float32_restatement_passes(group):
    _, simulate, verify, _ = rp.GROUPS[group]
    for c in BY_GROUP[group]:
        verify(c, inputs(c), simulate(c, inputs(c)))


@pytest.mark.parametrize("group,defect", [(g, d) for g, v in rp.GROUPS.items() for d in v[3]])
def test_seeded_defect_is_caught(group, defect):
    _, simulate, verify, _ = rp.GROUPS[group]
    caught = []
    for c in BY_GROUP[group]:
        try:
            verify(c, inputs(c), simulate(c, inputs(c), defect))
        except AssertionError:
            caught.append(c["name"])
    print(f"{group} / {defect}: caught by {len(caught)} of {len(BY_GROUP[group])} cases")
    assert caught, f"no case of {group} catches the defect {defect}: a case is missing"


def test_one_pass_variance_is_caught_by_the_offset_rows():
    _, simulate, verify, _ = rp.GROUPS["ln"]
    offs = [c for c in BY_GROUP["ln"] if c["kind"] == "offset" and c["dt"] == "f32" and c["eps"] == 1e-5]
    assert offs
    for c in offs:
        with pytest.raises(AssertionError):
            verify(c, inputs(c), simulate(c, inputs(c), "one_pass_variance"))


def test_checker_accepts_a_correct_bf16_store_and_rejects_a_truncated_one():
    c = next(c for c in BY_GROUP["gelu"] if c["dt"] == "bf16" and c["rows"] == 33 and c["drop_p"] == 0.0)
    t = inputs(c)
    ref = rp.gelu_ref(c, t)
    y32 = torch.from_numpy(ref["y"][0]).float()
    rp.check(c["name"], "y", "gelu_fwd", rp.store(y32, "bf16"), *ref["y"], out_dt="bf16")
    trunc = ((y32.view(torch.int32) >> 16) << 16).view(torch.float32)
    with pytest.raises(AssertionError):
        rp.check(c["name"], "y", "gelu_fwd", trunc.double().numpy(), *ref["y"], out_dt="bf16")


def test_guards_catch_a_write_outside_the_window_and_a_written_input():
    g = rp.Guarded(shape=(3, 8), dtype=torch.float32, out=True, ld=12)
    after = g.buf.clone()
    g.view(after).fill_(1.0)
    g.check(after, "window only")
    for flat in (g.off - 1, g.off + 8, g.off + 3 * 12):             # in front, between cols and ld, behind
        bad = after.clone()
        bad[flat] = 0.0
        with pytest.raises(AssertionError):
            g.check(bad, "outside")
    i = rp.Guarded(torch.arange(6, dtype=torch.int64).reshape(2, 3))
    i.check(i.buf.clone(), "untouched")
    bad = i.buf.clone()
    bad[i.off] = 7
    with pytest.raises(AssertionError):
        i.check(bad, "written")


# ------------------------------------------------------------------------------------------------ conditions on the inputs (reference alone)
@pytest.mark.parametrize("c", BY_GROUP["nll"], ids=[c["name"] for c in BY_GROUP["nll"]])
def test_mixture_inputs_meet_their_conditions(c):
    t = inputs(c)
    R = rp.nll_rows(c, t)
    lab = t["label"].numpy()
    assert ((lab >= 0) & (lab < c["V"] + c["T"]) | (lab == t["pad"])).all()
    assert int((R["valid"] & ~R["sure"]).sum()) == 0, "a committed case has a row whose two best entries are closer than their bounds"
    # switch logits: from the fixed set, and float32 and float64 agree on which side of 1e-6 every probability lies
    s = t["sw"]
    assert set(s.tolist()) <= set(rp.SWITCH_LOGITS) and min(abs(abs(v) - np.log(1e6 - 1)) for v in rp.SWITCH_LOGITS) >= 1.0
    p32 = 1.0 / (1.0 + torch.exp(-s))
    p64 = 1.0 / (1.0 + np.exp(-s.double().numpy()))
    assert np.array_equal((p32 >= rp.C6).numpy(), p64 >= rp.C6) and np.array_equal((1 - p32 >= rp.C6).numpy(), 1 - p64 >= rp.C6)
    if not c["allpad"]:
        i = R["i"]
        assert (R["is_p"] & (lab - c["V"] >= i)).any() and (R["is_p"] & (lab - c["V"] < i)).any() or c["T"] < 6
        assert R["is_v"].any() and (~R["valid"]).any() and R["valid"][0]
        if c["B"] > 1:
            assert not R["valid"][(c["B"] - 1) * c["T"]:].any()
    else:
        assert not R["valid"].any() and np.isnan(rp.nll_fwd_ref(c, t)["loss"][0])


NLL_TEST_ORDERS = 2000


@pytest.mark.parametrize("c", BY_GROUP["nll"], ids=[c["name"] for c in BY_GROUP["nll"]])
def test_nll_sum_passes_in_every_arrival_order_and_every_defect_still_fails(c):
    """pa_mixture_nll_fwd adds its block partials with float atomics: the order of addition is the arrival order.  The kernel's sum restated on
    the CPU (float32 rows, four per block, (r0 + r1) + (r2 + r3), the non-zero partials added in float32) passes verify_nll in the natural order
    and in 2000 seeded orders - seeded apart from the 64 orders behind the yardstick (rowops_parity.nll_sum_yardstick) - and the checker
    still rejects every listed defect.  verify_nll reads the sum's VALUE alone, so it runs once per distinct value the orders produce."""
    t = inputs(c)
    sim = rp.simulate_nll(c, t)
    rows = rp.nll_fwd_cpu32(c, t)["row_nll"]
    sums = rp.nll_order_sums(rows, rp.seed_of(c["name"], 1), NLL_TEST_ORDERS)
    assert sums.dtype == np.float32 and sums.shape == (1 + NLL_TEST_ORDERS,)
    values, counts = np.unique(sums, return_counts=True)
    ref = rp.nll_fwd_ref(c, t)["nll"]
    e = ref[1] + 0.5 * rp.TINY
    print(f"{c['name']}: {len(rp.nll_block_partials(rows))} non-zero block partials; {len(values)} distinct float32 sums over {len(sums)} orders: "
          + ", ".join(f"r {abs(float(v) - ref[0]) / e:.4g} ({100.0 * n / len(sums):.1f} %)" for v, n in zip(values, counts))
          + f"; yardstick r {abs(rp.nll_sum_yardstick(c, rp.nll_fwd_cpu32(c, t), ref[0]) - ref[0]) / e:.4g}, torch's float32 sum r {abs(sim['fwd']['stats'][0] - ref[0]) / e:.4g}")
    for v in values:
        got = dict(sim, fwd=dict(sim["fwd"], stats=np.array([float(v), sim["fwd"]["stats"][1], sim["fwd"]["stats"][2]])))
        rp.verify_nll(c, t, got)
    # The defects: each uses the kernel's own restated sum of its float32 rows; what a case catches is what it caught under the one-order rule.
    for defect in rp.GROUPS["nll"][3]:
        bad = rp.simulate_nll(c, t, defect)
        dsum = rp.nll_order_sums(rp.nll_fwd_cpu32(c, t, defect)["row_nll"], 0, 0)[0]
        bad["fwd"] = dict(bad["fwd"], stats=np.array([float(dsum), bad["fwd"]["stats"][1], bad["fwd"]["stats"][2]]))
        if defect in NLL_DEFECT_NOT_SEEN.get(c["name"], NLL_DEFECT_NOT_SEEN["x1" if c["scale"] == 1 else "x30"]):
            rp.verify_nll(c, t, bad)                                # (the defect changes nothing this case can see: it must not fail for another reason)
        else:
            with pytest.raises(AssertionError):
                rp.verify_nll(c, t, bad)


# Defects a case cannot see (all others must fail it): without the maximum, exp overflows only at scale 30 with more than 3 entries; the all-pad
# case has no valid row, so only the masked pointer entries of row_lse differ; at V 1030, T 7, scale 30 no switch probability of a valid row
# lies beyond the clamp.
NLL_DEFECT_NOT_SEEN = {"x1": {"lse_without_max"}, "x30": set(), "nll_B1_T5_V3_ld3_x30": {"lse_without_max"},
                       "nll_B1_T7_V1030_ld1032_x30": {"switch_clamp_ignored"},
                       "nll_B2_T36_V514_ld520_allpad": {"lse_without_max", "argmax_larger_index_on_tie", "switch_clamp_ignored", "gscale_left_out"}}


def test_segment_lengths_are_placed_by_construction():
    for c in BY_GROUP["embed_seg"]:
        t = inputs(c)
        lens = set()
        for sg in t["seg"]:
            lens |= set((sg[1:] - sg[:-1]).tolist())
        want = set(rp.SEG_LENGTHS)
        assert want <= lens, (c["name"], sorted(want - lens))


def test_specials_cover_ties_subnormals_infinities_and_nan():
    sp = rp.f32_specials()
    b = sp.to(torch.bfloat16)
    assert torch.isnan(sp).sum() >= 3 and torch.isinf(sp).sum() == 2 and torch.isnan(b).sum() == torch.isnan(sp).sum()
    assert torch.isinf(b).sum() > 2                                 # the largest finite float32 rounds to infinity
    bits = sp.view(torch.int32)
    ties = (bits & 0xFFFF) == 0x8000
    up = ((b.view(torch.int16).int() & 0xFFFF) != ((bits >> 16) & 0xFFFF)) & ties
    assert bool(up.any()) and bool((ties & ~up & ~torch.isnan(sp)).any())       # ties that round up and ties that round down
    assert bool(((bits & 0x7F800000) == 0).sum() >= 5)              # zeros and subnormals
