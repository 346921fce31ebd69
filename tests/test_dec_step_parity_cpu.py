"""The float64 checker of the decode step's own kernels (tests/dec_step_parity.py) tested on the CPU, with the float32 restatements
standing in for dec_attn_kernel, the distribution code, dec_split_heads_kernel and dec_embed_kernel of csrc/decode.hip:

  - the restatements pass both tiers and every exact check at every case of the table (so the inputs keep correct float32 arithmetic
    inside the bounds), the ten steps of the chained cases included;
  - every seeded defect of ATTN_DEFECTS, DIST_DEFECTS and COPY_DEFECTS is refused on a committed case in bf16 and in f32; the table of
    defect, type, case and tier is printed.  One cannot occur in f32 and is recorded as such:
        output_rounded_twice   the f32 kernel stores num / den as it is: there is no second rounding to make.  In bf16 it is refused
                               (two roundings of 2^-9 in front of the store's own against a slack of half an ulp);
  - for every attention case, dropping, doubling or shifting the spot key of every (row, head) in the restatement moves some output by
    at least 100 tier-1 bounds (doubling and shifting need a second allowed key: one key alone has weight 1 whatever it counts);
  - dispatch() puts every case on the edge it is named for; over the table every (type, dh) meets every key count of the issue, every
    form, d 48 and 96 with three heads, and the distribution meets every NCH branch, the generic loop, every t and i % 6 class;
  - every refusal has the status the table gives it, and the GPU file calls every new entry of include/plank_hip.h.
"""
import functools
import os
import re

import numpy as np
import pytest

import dec_step_parity as dp

ATTN = dp.attn_cases()
DIST = dp.dist_cases()
EMBED = dp.embed_cases()
SPLIT = dp.split_cases()
ALL = ATTN + DIST + EMBED + SPLIT
BY_NAME = {c["name"]: c for c in ALL}
HERE = os.path.dirname(os.path.abspath(__file__))
GPU_FILE = os.path.join(HERE, "test_dec_step_float64_gpu.py")
HEADER = os.path.join(os.path.dirname(HERE), "include", "plank_hip.h")
ids = lambda cs: [c["name"] for c in cs]


@functools.lru_cache(maxsize=None)
def prepared(name):
    c = BY_NAME[name]
    if c["kernel"] == "attn":
        t = dp.AttnTensors(c)
        return c, t, (None if c["steps"] else dp.attn_reference(c, t)), (None if c["steps"] else dp.attn_cpu32(c, t))
    t = dp.DistTensors(c)
    return c, t, dp.dist_reference(c, t), dp.dist_cpu32(c, t)


# ------------------------------------------------------------------------------------------------ the restatements pass
@pytest.mark.parametrize("c", ATTN, ids=ids(ATTN))
def test_the_attention_restatement_passes_both_tiers(c):
    c, t, ref, cpu = prepared(c["name"])
    if c["steps"]:
        caches = (t.kc0.numpy().copy(), t.vc0.numpy().copy())
        for step in range(c["steps"]):
            ref = dp.attn_reference(c, t, step)
            cpu = dp.attn_cpu32(c, t, step=step, caches=caches)
            r, r_cpu = dp.attn_judge(c, t, cpu["out"], cpu["kc"], cpu["vc"], ref, cpu, step)
            assert r == r_cpu
        return
    r, r_cpu = dp.attn_judge(c, t, cpu["out"], cpu["kc"], cpu["vc"], ref, cpu)
    assert r == r_cpu
    if c["dt"] == "f32":
        assert r <= 1.0, r                                          # (float32 arithmetic in the kernel's order sits inside the FIRST-order bound)


@pytest.mark.parametrize("c", DIST, ids=ids(DIST))
def test_the_distribution_restatement_passes_both_tiers(c):
    c, t, ref, cpu = prepared(c["name"])
    r, r_cpu = dp.dist_judge(c, t, cpu["p"], cpu["stats"], cpu["cache"], ref, cpu)
    assert r == r_cpu and r <= 1.0, r


# ------------------------------------------------------------------------------------------------ seeded defects
def _tier(msg):
    return "tier 1" if "tier 1" in msg else "tier 2" if "tier 2" in msg else "exact" if "exact" in msg else msg[:40]


def _refusal_attn(defect, dt):
    for c in ATTN:
        if c["dt"] != dt or not dp.attn_applies(defect, c):
            continue
        c, t, ref, cpu = prepared(c["name"])
        bad = dp.attn_cpu32(c, t, defect)
        try:
            dp.attn_judge(c, t, bad["out"], bad["kc"], bad["vc"], ref, None)        # tier 1 and the exact checks alone
        except AssertionError as e:
            return c["name"], _tier(str(e))
    return None


def _refusal_dist(defect, dt):
    for c in DIST:
        if c["dt"] != dt:
            continue
        c, t, ref, cpu = prepared(c["name"])
        bad = dp.dist_cpu32(c, t, defect)
        try:
            dp.dist_judge(c, t, bad["p"], bad["stats"], bad["cache"], ref, None)
        except AssertionError as e:
            return c["name"], _tier(str(e))
    return None


def _refusal_copy(defect, dt):
    for c in (EMBED if defect.startswith("t_mod") else SPLIT):
        if c["dt"] != dt:
            continue
        if c["kernel"] == "embed":
            t = dp.EmbedTensors(c)
            got, want = dp.embed_want(c, t, defect), dp.embed_want(c, t)
        else:
            t = dp.SplitTensors(c)
            got, want = dp.split_want(c, t, defect), dp.split_want(c, t)
        try:
            for g, w in zip(got, want):
                if w is not None:
                    dp.same_bits(c["name"], "copy", g, w)
        except AssertionError as e:
            return c["name"], _tier(str(e))
    return None


NOT_IN_F32 = {"output_rounded_twice"}                               # (module docstring)


def test_every_seeded_defect_is_refused_at_tier_1_in_both_types():
    rows, missed = [], []
    table = [(d, _refusal_attn) for d in dp.ATTN_DEFECTS] + [(d, _refusal_dist) for d in dp.DIST_DEFECTS] + [(d, _refusal_copy) for d in dp.COPY_DEFECTS]
    for defect, find in table:
        for dt in ("bf16", "f32"):
            if dt == "f32" and defect in NOT_IN_F32:
                assert not any(dp.attn_applies(defect, c) for c in ATTN if c["dt"] == "f32")
                rows.append((defect, dt, "-", "cannot occur: no second rounding in an f32 store"))
                continue
            hit = find(defect, dt)
            rows.append((defect, dt) + (hit or ("-", "NOT REFUSED")))
            if hit is None or hit[1] not in ("tier 1", "exact"):
                missed.append((defect, dt, hit))
    print("\n%-52s %-5s %-44s %s" % ("defect", "type", "first case that refuses it", "by"))
    for row in rows:
        print("%-52s %-5s %-44s %s" % row)
    assert not missed, f"not refused at tier 1 / exactly: {missed}: the case table is too weak"
    assert len(dp.ATTN_DEFECTS) >= 14 and len(dp.DIST_DEFECTS) >= 9 and len(dp.COPY_DEFECTS) >= 2


STATIC = [c for c in ATTN if not c["steps"]]


@pytest.mark.parametrize("c", STATIC, ids=ids(STATIC))
def test_the_spot_key_dropped_doubled_or_shifted_is_a_hundred_bounds(c):
    c, t, ref, cpu = prepared(c["name"])
    assert t.spot, c["name"]
    bound = np.repeat(np.ones_like(ref["has"], dtype=bool), c["dh"], axis=1) * (2.0 * ref["E"] + dp.TINY)
    if c["dt"] == "bf16":
        bound = bound + dp.half_ulp_bf16(np.abs(ref["ref"]))
    several = any(t.allowed[r if c["form"] == "self" else r // c["G"]].sum() > 1 for (r, h) in t.spot)
    for how in ("drop", "double", "shift"):
        if how != "drop" and not several:
            continue
        moved = np.abs(dp.attn_cpu32(c, t, edit=how)["out"] - cpu["out"])
        with np.errstate(invalid="ignore"):
            worst = float(np.nanmax(np.where(np.isfinite(moved), moved / bound, np.inf)))
        assert worst >= dp.SPOT_MIN_BOUNDS, (c["name"], how, worst)


# ------------------------------------------------------------------------------------------------ dispatch and coverage
@pytest.mark.parametrize("c", ALL, ids=ids(ALL))
def test_dispatch_puts_the_case_on_its_edge(c):
    ok, p = dp.on_edge(c)
    assert ok, f"{c['name']}: meant for {c['edge']}, dispatched as {p}"
    for key, hi in dp.extents(c).items():
        assert hi > 0, (c["name"], key)


def test_the_attention_table_covers_what_the_issue_lists():
    for dt in ("f32", "bf16"):
        for dh in (16, 32, 64):
            g = dp.geometry(dt, dh)
            mine = [c for c in ATTN if c["dt"] == dt and c["dh"] == dh and not c["steps"]]
            self_lk = {c["lens"][0] for c in mine if c["form"] == "self"}
            assert self_lk == set(dp.lk_list(g)), (dt, dh, self_lk)
            assert {dp.lk_label(L, g) for L in self_lk} == set(dp.LK_LABELS)
            assert {c["form"] for c in mine} == {"self", "kpm", "packed", "dense"}
            assert {c["G"] for c in mine} == {1, 2, 3} and {c["Bd"] for c in mine} <= {2, 3} and {c["H"] for c in mine} == {2, 3}
            lens = {L for c in mine if c["form"] == "packed" for L in c["lens"]}
            assert {0, 1} <= lens
            assert {(c["form"]) for c in mine if c["G"] > 1} == {"dense", "packed", "kpm"}
            for c in mine:
                if c["form"] == "kpm":
                    m = dp.attn_mask(c)
                    S = c["lens"][0]
                    assert m[0, 0] and m[1, S - 1] and m[-1, :S].all() and 0 < m[0, 1:S - 1].sum() < S - 2 and c["Lmax"] > S
    assert max(L for c in ATTN for L in c["lens"]) == 2051
    assert {(c["H"] * c["dh"], c["H"]) for c in ATTN} >= {(48, 3), (96, 3)}
    table = {("f32", 16): (64, 512), ("f32", 32): (32, 256), ("f32", 64): (16, 128), ("bf16", 16): (128, 1024), ("bf16", 32): (64, 512), ("bf16", 64): (32, 256)}
    for (dt, dh), (P, I) in table.items():
        g = dp.geometry(dt, dh)
        assert (g["pass_keys"], g["iter_keys"]) == (P, I)
    assert sum(1 for c in ATTN if c["steps"] == 10) == 2


def test_the_distribution_table_covers_what_the_issue_lists():
    for dt in ("f32", "bf16"):
        mine = [c for c in DIST if c["dt"] == dt]
        assert {c["d"] for c in mine} == {256, 512, 768, 1024, 48, 96}
        assert {dp.dispatch(c)["nch"] for c in mine} == {0, 1, 2, 3, 4}
        ts = {c["t"] for c in mine}
        assert {0, 4, 5, 6, 7, 8, 9, 10, 11, 31, 32, 33, 63, 64, 65, 255, 256, 257} <= ts and all(c["t"] == c["Tmax"] - 1 for c in mine if c["t"] in (299, 2047))
        assert {c["t"] % 6 for c in mine if c["t"] >= 6} == set(range(6))
        for d in (256, 1024, 48, 96, 768, 512):                     # the second iteration of the pointer loop and its tail, and the wrapped softmax, at every width
            sub = [dp.dispatch(c) for c in mine if c["d"] == d]
            assert any(p["ptr_iters"] >= 2 for p in sub) and any(p["softmax_wrap"] for p in sub), d
            assert d in (48, 96) or any(p["ptr_tail"] and p["ptr_iters"] >= 2 for p in sub), d
        assert all(c["V"] % 256 and c["ldv"] > c["V"] for c in mine) and any(c["V"] < 256 for c in mine)
        assert {c["scale"] for c in mine} == {1.0, 30.0} and {c["gate"] for c in mine} == {"mid", "sat_hi", "sat_lo"}
        for c in mine[:6]:
            t = dp.DistTensors(c)
            assert np.isnan(t.vlog[:, c["V"]:].numpy()).all() and np.isnan(t.cache0[c["t"] + 1:].numpy()).all()
    sat = [prepared(c["name"])[2]["stats"][:, 4] for c in DIST if c["gate"] != "mid" and c["t"] >= 5]
    assert min(s.min() for s in sat) < 1e-10 and max(s.max() for s in sat) > 1 - 1e-10


def test_refusals_carry_the_status_of_the_restated_dispatch():
    rs = dp.attn_rejections()
    assert {st for _, st in rs} == {dp.PA_EINVAL, dp.PA_EALIGN, dp.PA_ESHAPE}
    names = " ".join(c["name"] for c, _ in rs)
    for word in ("null_out", "null_q", "null_kc", "null_vc", "null_t_dev", "dh8", "dh24", "dh128", "out_off", "q_off", "kc_off", "vc_off", "newkv_off",
                 "ldq_no_vector", "G0", "rows3_G2", "newkv_with_cu", "newkv_with_kpm", "newkv_with_G2"):
        assert word in names, word
    assert all(dp.dispatch(c)["status"] == st for c, st in rs)


def test_the_gpu_file_calls_every_new_entry_of_the_header():
    with open(HEADER) as f:
        head = f.read()
    entries = {"pa_dec_attn", "pa_dec_split_heads", "pa_dec_embed", "pa_dec_row_dist"}
    for e in entries:
        assert re.search(r"\bint %s\(" % e, head), e
    from plankassembly_amd import _lib, ops
    with open(_lib.__file__) as f:
        bound = f.read()
    with open(GPU_FILE) as f:
        src = f.read()
    for e in entries:
        assert f'"{e}"' in bound and re.search(r"\b%s\b" % e, src), e
    for w in ("dec_attn", "dec_split_heads", "dec_embed", "dec_row_dist"):
        assert callable(getattr(ops, w)) and re.search(r"ops\.%s\b" % w, src), w
