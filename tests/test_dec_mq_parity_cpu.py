"""The float64 checker of the absorbed decode attention (tests/dec_mq_parity.py) tested on the CPU, with float32 torch standing in for the
kernels of csrc/decode_mq.h:

  - both float32 emulations - the plain one that is tier 2's yardstick and the tiled one with the kernels' structure - pass both tiers and
    the exact zeros at every case, under the default switches and under every bundle that changes a case's range blocks (which also proves
    that the inputs keep correct float32 arithmetic inside the bounds);
  - every seeded defect of dec_mq_parity.DEFECTS is refused on a committed case, in bf16 and in f32 where it can occur there; the table of
    defect, case and tier is printed, with what the tensor-wide metric of tests/test_decode_mq_gpu.py says to the same output;
  - dispatch() puts every case on the branch it is named for, names all 8 + 2 + 2 instantiations and every path label over the cases and
    bundles, agrees with the library's own pa_dec_cross_mq_ws_bytes, and every rejection has the status the table gives it;
  - every kernel meets every key count and every regime, and the spot keys reach every edge of a 272-key drawing;
  - the GPU file calls every pa_dec_*_mq* entry of include/plank_hip.h.
"""
import functools
import os
import re

import numpy as np
import pytest

import dec_mq_parity as dp

ALL = dp.cases()
BY_NAME = {c["name"]: c for c in ALL}
HERE = os.path.dirname(os.path.abspath(__file__))
GPU_FILE = os.path.join(HERE, "test_dec_mq_float64_gpu.py")
HEADER = os.path.join(os.path.dirname(HERE), "include", "plank_hip.h")
ENVS = dict(default={}, **dp.BUNDLES)


@functools.lru_cache(maxsize=None)
def prepared(name):
    c = BY_NAME[name]
    t = dp.Tensors(c)
    return c, t, dp.reference(c, t), dp.emulate(c, t)


@pytest.mark.parametrize("c", ALL, ids=[c["name"] for c in ALL])
def test_the_float32_emulations_pass_both_tiers(c):
    c, t, ref, emu = prepared(c["name"])
    r, r_emu = dp.judge(c, t, emu, ref, emu)
    assert r == r_emu and r <= 2.0
    for bundle, env in ENVS.items():
        if bundle != "default" and dp.dispatch(c, env)["nparts"] == dp.dispatch(c)["nparts"] and dp.dispatch(c, env)["kern"] == dp.dispatch(c)["kern"]:
            continue
        r, _ = dp.judge(c, t, dp.emulate_tiled(c, t, env=env), ref, emu, env=env)
        assert r <= 2.0, (bundle, r)


# ------------------------------------------------------------------------------------------------ seeded defects
def _tier(msg):
    return "tier 1" if "tier 1" in msg else "tier 2" if "tier 2" in msg else "exact" if "exact" in msg else msg[:40]


def _first_refusal(defect, dt, env=None):
    for c in ALL:
        if c["dt"] != dt or not dp.applies(defect, c, env):
            continue
        c, t, ref, emu = prepared(c["name"])
        got = dp.emulate_tiled(c, t, defect, env)
        try:
            dp.judge(c, t, got, ref, emu, env=env)
        except AssertionError as e:
            return c["name"], _tier(str(e)), dp.old_metric_passes(c, got, ref)
    return None


# Defects that no table can show through a bf16 output, recorded as such:
#   p_rounded_twice          one more rounding of 2^-9: inside tier 1 (2 eps covers two of them) and a factor sqrt(2) in tier 2.
#   denominator_from_bf16_p  the output becomes sum bf(p) m / sum bf(p): the correct output times sum p / sum bf(p) = 1 + delta, |delta| <= 2^-9 -
#                            one uniform relative 2^-9, under the half ulp of the bf16 store that every output carries anyway.  Tier 1 allows
#                            2 x 2^-9 S with S >= |ref|; in tier 2 r(got) <= (2^-9 |ref| + half ulp) / (2^-9 S) <= 1.5 / (1 + 2 A) while the store alone
#                            gives the emulation r >= 0.25 / (1 + 2 A): a ratio of at most 6, against a factor that starts at 16.
BELOW_BF16 = {"p_rounded_twice", "denominator_from_bf16_p"}


def test_every_seeded_defect_is_refused_on_a_committed_case():
    rows, missed = [], []
    for defect in dp.DEFECTS:
        for dt, env in (("bf16", None), ("f32", None), ("f32", dp.BUNDLES["w8_0"])):
            kern = "mq" if dt == "bf16" else ("mq32" if env else "mq32w8")
            if not any(c["dt"] == dt and dp.applies(defect, c, env) for c in ALL):
                assert dt == "f32" and defect in ("p_rounded_twice", "denominator_from_bf16_p") or (env and (defect.startswith("range_") or defect.startswith("partial_"))), (defect, dt)
                continue
            hit = _first_refusal(defect, dt, env)
            if hit is None:
                rows.append((defect, kern, "-", "none: below what bf16 can show" if defect in BELOW_BF16 else "NOT REFUSED", ""))
                if defect not in BELOW_BF16:
                    missed.append((defect, kern))
                continue
            rows.append((defect, kern, hit[0], hit[1], "passes" if hit[2] else "fails"))
    print("\n%-34s %-7s %-44s %-32s %s" % ("defect", "kernel", "first case that refuses it", "tier", "old tensor-wide metric"))
    for row in rows:
        print("%-34s %-7s %-44s %-32s %s" % row)
    assert not missed, f"no committed case refuses {missed}: the case table is too weak"
    assert {r[0] for r in rows} == set(dp.DEFECTS)
    # p rounded twice passes tier 1 in bf16 (2 eps covers the second rounding); whether tier 2 sees it is in the table above
    c, t, ref, emu = prepared("dense_S272_H8_bf16")
    dp.check(c, t, dp.emulate_tiled(c, t, "p_rounded_twice"), ref)


def test_a_single_wrong_key_under_the_spot_is_hundreds_of_bounds():
    """What the spot regime is for: the chosen key of ONE head slot read from the neighbouring row - every other key right."""
    for name in ("dense_S272_H8_bf16", "dense_S272_H8_f32"):
        c, t, ref, emu = prepared(name)
        r = t.regime.index("spot")
        k = t.chosen[(r, 3)]
        row0 = t.el[r // c["G"]][0]
        keep = t.mem[row0 + k].clone()
        t.mem[row0 + k, 33:] = t.mem[row0 + (k + 1 if k + 1 < t.el[r // c["G"]][1] else k - 1), 33:]
        try:
            got = dp.emulate(c, t)
        finally:
            t.mem[row0 + k] = keep
        with pytest.raises(AssertionError, match="tier 1") as e:
            dp.check(c, t, got, ref)
        assert f"spot key {k}" in str(e.value) and float(re.search(r"= ([0-9.e+]+) x the bound", str(e.value)).group(1)) > 100, str(e.value)


# ------------------------------------------------------------------------------------------------ dispatch
@pytest.mark.parametrize("c", ALL, ids=[c["name"] for c in ALL])
def test_dispatch_puts_the_case_on_its_branch(c):
    ok, p = dp.on_branch(c)
    assert ok, f"{c['name']}: meant for {c['branch']}, dispatched as {p}"
    assert p["grid"] == p["units"] * p["nparts"] and p["lds"] <= 160 * 1024 and p["slots"] <= dp.SLOTS
    assert c["S"] <= 272 and c["B"] <= 6 and max(l for _, l in dp.key_counts(c)) <= 272


def test_dispatch_names_every_instantiation_and_every_path():
    kernels, paths = set(), set()
    for env in ENVS.values():
        for c in ALL:
            p = dp.dispatch(c, env)
            kernels.add(p["kernel"])
            paths |= p["path"]
    assert kernels == set(dp.INSTANTIATIONS) and len(dp.INSTANTIATIONS) == 12
    assert paths == dp.PATH_LABELS, dp.PATH_LABELS - paths
    # each bundle changes the dispatch of some case, of the right type only
    for bundle, env in dp.BUNDLES.items():
        changed = [c for c in ALL if dp.dispatch(c, env) != dp.dispatch(c)]
        assert changed, bundle
        if bundle in ("swap_0", "nt_0", "swap_0_nt_0"):
            assert {c["name"] for c in changed} == {c["name"] for c in ALL if c["dt"] == "bf16"}
        if bundle == "w8_0":
            assert {c["name"] for c in changed} == {c["name"] for c in ALL if c["dt"] == "f32"}
    mint = dp.dispatch(BY_NAME["ranges_rule_B2_S272_bf16"], dp.BUNDLES["mint_1"])
    assert mint["nparts"] == 17 and mint["grid"] == 34               # one tile per range block at S = 272
    assert dp.dispatch(BY_NAME["ranges_rule_B2_S272_f32"], dp.BUNDLES["parts_3"])["nparts"] == 3
    assert dp.dispatch(BY_NAME["ranges_forced3_S272_f32"], dp.BUNDLES["w8_0"])["nparts"] == 1      # the four-wave kernel never splits


def test_the_parts_rule_agrees_with_the_library():
    from plankassembly_amd import _lib as L
    env = {k: os.environ[k] for k in dp.SWITCHES if k in os.environ}
    sw = dp._switches(env)
    for B, S in ((2, 272), (1, 272), (5, 272), (2, 40), (16, 1024), (300, 1024), (3, 129), (64, 2048), (1, 16384)):
        parts = dp.mq_parts(B, S, sw["parts"], sw["mint"])
        want = dp.tick_bytes(B) + B * parts * 40 * 1024 if parts > 1 else 0
        assert int(L.lib().pa_dec_cross_mq_ws_bytes(B, S)) == want == dp.split_bytes(B, parts), (B, S, parts)
    assert int(L.lib().pa_dec_cross_mq_ws_bytes(0, 272)) == 0 and int(L.lib().pa_dec_cross_mq_ws_bytes(2, 0)) == 0


def test_rejections_carry_the_status_of_the_restated_dispatch():
    rs = dp.rejections()
    assert {st for _, st in rs} == {dp.PA_EINVAL, dp.PA_EALIGN, dp.PA_ESHAPE}
    names = " ".join(c["name"] for c, _ in rs)
    for word in ("d256", "H9", "H0", "S0", "S16385_bf16", "S16001_f32", "rpb2_G3", "rpb3", "G0", "qt_off", "mem_off", "null_qt", "null_mem", "null_ctx", "null_t_dev"):
        assert word in names, word


# ------------------------------------------------------------------------------------------------ coverage of the table
def test_every_kernel_meets_every_key_count_regime_and_edge():
    for dt in ("bf16", "f32"):
        counts, regimes, spots, H, t_self = set(), set(), set(), set(), set()
        for c in ALL:
            if c["dt"] != dt:
                continue
            t = prepared(c["name"])[1]
            counts |= {l for _, l in t.el}
            regimes |= set(t.regime)
            H.add(c["H"])
            if c["form"] == "self":
                t_self.add(c["t"])
            for (r, h), k in t.chosen.items():
                if t.regime[r] == "spot" and t.el[r // c["G"]][1] == 272 and dp.dispatch(c)["nparts"] == 1:
                    spots.add(k)
        assert set(dp.KEY_COUNTS) | {0} <= counts, set(dp.KEY_COUNTS) - counts
        assert regimes == set(dp.REGIMES) and H == {8, 5, 4, 1} and t_self == {0, 15, 16, 111, 112, 271}
        assert set(dp.edges(272)) <= spots, set(dp.edges(272)) - spots
    assert {0, 15, 16, 271, 96, 111, 112, 127, 128, 143, 48, 63, 64, 79} <= set(dp.edges(272))
    for n in (2, 3, 5):
        for p in range(n):
            lo, hi = dp.split_range(17, p, n)
            if lo < hi:
                assert {lo * 16, hi * 16 - 1} <= set(dp.edges(272, n))


def test_the_gpu_file_calls_every_entry_of_the_header():
    with open(HEADER) as f:
        entries = set(re.findall(r"\b(pa_dec_(?:cross|self)_mq\w*)\s*\(", f.read()))
    assert {"pa_dec_cross_mq", "pa_dec_cross_mq32", "pa_dec_cross_mq_ws", "pa_dec_cross_mq32_ws", "pa_dec_cross_mq_ws_bytes", "pa_dec_cross_mq_group",
            "pa_dec_cross_mq32_group", "pa_dec_self_mq32", "pa_dec_self_mq_ws"} == entries, entries
    with open(GPU_FILE) as f:
        src = f.read()
    for e in entries:
        assert re.search(r"\b%s\b" % e, src), f"{e} is not called by {os.path.basename(GPU_FILE)}"
