"""The float64 GEMM parity checker (tests/gemm_parity.py) tested on the CPU, with float32 arithmetic standing in for the kernels:

  - a CORRECT product - float32, accumulated K block by K block as a tiled kernel does - passes both tiers for every case of the GPU
    list (which also proves that the inputs keep the reference arithmetic inside the bounds);
  - eight seeded defects, each applied to ONE edge tile, all fail;
  - the same defects under the metric of the older GEMM tests (max |got - ref| / max |ref| < 2.5e-2 over the tensor) are printed:
    a record of what that metric misses, not an assertion;
  - the dispatch dry run (pa_gemm_plan, no device) sends every case to the family it is meant for under default switches, and every
    switch bundle of tests/test_gemm_float64_gpu.py changes the plan and reaches the kernels it exists for.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_parity as gp
import test_gemm_float64_gpu as G

ALL = gp.cases() + gp.group_cases() + gp.defer_cases()
BY_NAME = {c["name"]: c for c in ALL}


def tile_of(c):
    return {"SMALL": (64, 64), "WIDE": (128, 256), "SKINNY": (32, 32)}.get(c["family"], (128, 128))


def judged(c, t, got, parts=None):
    """gp.check on a CPU `got` (float32 values, stored as the case's output type), r_cpu from torch.matmul."""
    parts = parts or gp.reference_parts(c, t)
    sk = gp.eff_splitk(c)
    r_cpu = gp.ratio(gp.cpu_float32(c, t), parts["ref"], parts["S"], c["K"], sk)
    return gp.check(gp.store(c, got), parts["ref"], parts["S"], c["K"], sk, c["out_dt"], name=c["name"], family=c["family"], tile=tile_of(c),
                    parts=parts, r_cpu=r_cpu), r_cpu


@pytest.mark.parametrize("c", ALL, ids=[c["name"] for c in ALL])
def test_a_correct_float32_product_passes_both_tiers(c):
    t = gp.make_tensors(c)
    got = gp.cpu_float32(c, t, matmul=gp.blocked_matmul32)
    r, r_cpu = judged(c, t, got)
    assert 0 < r_cpu < 2.0, r_cpu                                   # the reference arithmetic sits inside tier 1, and not at zero
    assert c["out_dt"] == "bf16" or r < 2.0, r                      # (a bf16 store adds its own rounding to r)


# ------------------------------------------------------------------------------------------------ seeded defects
def edge(c):
    """The last row tile x last column tile of the last batch member (128 x 128 tiling)."""
    M, N = c["M"], c["N"]
    return (c["batch"] - 1, slice((M - 1) // 128 * 128, M), slice((N - 1) // 128 * 128, N))


def graft(good, bad, where):
    out = good.copy()
    out[where] = bad[where]
    return out


def _acc(c, t, k_range=None):
    a, b = t["A"].view().float(), t["B"].view().float()
    a = a if c["akc"] else a.transpose(1, 2)
    b = b.transpose(1, 2) if c["bkc"] else b
    if k_range:
        a, b = a[:, :, k_range[0]:k_range[1]], b[:, k_range[0]:k_range[1], :]
    return torch.matmul(a.contiguous(), b.contiguous())


def d_last_k_dropped(c, t, good):
    return graft(good, gp.cpu_float32(c, t, k_range=(0, c["K"] - 1)), edge(c))


def d_slab_omitted(c, t, good):
    sk = gp.eff_splitk(c)
    n_tiles = (c["K"] + 63) // 64
    per = (n_tiles + sk - 1) // sk * 64                             # K elements per slice; the last slice is left out
    return graft(good, gp.cpu_float32(c, t, k_range=(0, per * (sk - 1))), edge(c))


def d_row_through_bf16(c, t, good):
    out = good.copy()
    b, rows, cols = edge(c)
    out[b, c["M"] - 1, cols] = torch.from_numpy(good[b, c["M"] - 1, cols].copy()).to(torch.bfloat16).float().numpy()
    return out


def d_bias_of_member_0(c, t, good):
    bias0 = t["bias"].view()[0:1].expand(c["batch"], 1, c["N"])
    return graft(good, gp.epilogue32(c, t, _acc(c, t), bias=bias0), edge(c))


def d_padding_leaked(c, t, good):
    out = good.copy()
    b, m, n = c["batch"] - 1, c["M"] - 1, c["N"] - 1
    bn0 = float(t["B"].view()[b, n, 0] if c["bkc"] else t["B"].view()[b, 0, n])
    out[b, m, n] = np.float32(out[b, m, n] + np.float32(gp.POISON) * np.float32(bn0))      # one more k: A's padding times B[0][n]
    return out


def d_dropped_left_nonzero(c, t, good):
    b, rows, cols = edge(c)
    dropped = np.argwhere(~gp.keep_mask(c)[b, rows, cols])
    m, n = rows.start + int(dropped[0][0]), cols.start + int(dropped[0][1])
    out = good.copy()                                               # (good there is 0 + R: the survivor's value goes on top of it)
    out[b, m, n] += np.float32(_acc(c, t)[b, m, n].item() * gp.dm.linear_scale(gp.EPILOGUES[c["epi"]]["drop_p"]))
    return out


def d_residual_before_dropout(c, t, good):
    return graft(good, gp.epilogue32(c, t, _acc(c, t), res_first=True), edge(c))


DEFECTS = [
    ("last k element dropped in the last row tile", d_last_k_dropped,
     ["pair_bf16_130x200x72_nn", "pair_bf16_257x514x96_nt", "pair_f32_257x514x96_nn", "ring_130x200x72_tt", "small_129x65x448", "skinny_f32_250x514x512"]),
    ("one split-K slab omitted", d_slab_omitted, ["ring_130x200x512_sk4", "ring_130x200x576_sk4", "defer_130x200x1000_tt_sk5"]),
    ("one row rounded through bf16 before an f32 store", d_row_through_bf16,
     ["pair_bf16_130x200x72_nn", "wide_4100x1030x64", "skinny_bf16_512x96x1024", "pair_f32_130x200x40_nn"]),
    ("bias of batch member 0 used for member 2", d_bias_of_member_0,
     ["ring_b3_130x200x128_nt_member_bias", "ring_b3_70x96x256_sk4_member_bias", "small_b3_130x200x64_member_bias"]),
    ("2^60 padding leaked into one element", d_padding_leaked, ["pair_bf16_130x200x72_nn", "epi_pair_f32_none_bf16out", "ring_130x200x72_tt"]),
    ("a dropped element left non-zero", d_dropped_left_nonzero, ["epi_pair_bf16_drop_res_f32out", "epi_ring_bf16_drop_res_bf16out"]),
    ("+R applied before the dropout", d_residual_before_dropout, ["epi_pair_bf16_drop_res_f32out", "epi_small_bf16_drop_res_bf16out", "ring_b3_130x200x128_nt_drop_res"]),
]
PAST_N = "one element stored one column past N"
PAST_N_CASES = ["pair_bf16_130x200x72_nn", "epi_small_bf16_none_bf16out", "ring_b3_130x200x128_nt_member_bias"]
_OUTCOMES = {}


def old_metric_passes(got, ref):
    """rel_err of tests/test_kernels_gpu.py under its bf16 tolerance."""
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12)) < 2.5e-2


def outcome(what, defect, name):
    """(the checker's failure message or None, whether the tensor-wide metric lets the defect through), computed once."""
    if (what, name) not in _OUTCOMES:
        c = BY_NAME[name]
        t = gp.make_tensors(c)
        parts = gp.reference_parts(c, t)
        good = gp.cpu_float32(c, t, matmul=gp.blocked_matmul32)
        judged(c, t, good, parts)                                   # the product the defect is grafted onto passes
        bad = defect(c, t, good)
        n_changed = int((gp.store(c, bad) != gp.store(c, good)).sum())
        assert 0 < n_changed <= 128 * 128, (what, name, n_changed)
        try:
            judged(c, t, bad, parts)
            msg = None
        except AssertionError as e:
            msg = str(e)
        _OUTCOMES[(what, name)] = (msg, old_metric_passes(gp.store(c, bad), parts["ref"]))
    return _OUTCOMES[(what, name)]


def past_n_outcome(name):
    """The store one column past N: the C window is right, only the guard behind it is hit."""
    if (PAST_N, name) not in _OUTCOMES:
        c = BY_NAME[name]
        t = gp.make_tensors(c)
        plane = t["C"]
        after = plane.buf.clone()
        plane.view(after).copy_(torch.from_numpy(gp.cpu_float32(c, t)).to(plane.dtype))
        gp.check_sentinels(plane, after, "C", name)                 # a store inside the window leaves the guards alone
        after[plane.off + (c["batch"] - 1) * plane.sb + (c["M"] - 1) * plane.ld + c["N"]] = 1.0
        try:
            gp.check_sentinels(plane, after, "C", name)
            msg = None
        except AssertionError as e:
            msg = str(e)
        _OUTCOMES[(PAST_N, name)] = (msg, old_metric_passes(plane.view(after).double().numpy(), gp.reference_parts(c, t)["ref"]))
    return _OUTCOMES[(PAST_N, name)]


@pytest.mark.parametrize("what,defect,names", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_seeded_defect_in_one_edge_tile_is_caught(what, defect, names):
    for name in names:
        c = BY_NAME[name]
        msg, _ = outcome(what, defect, name)
        assert msg is not None, f"{what}: not caught at {name}"
        assert name in msg and f"[{c['family']}]" in msg and "(b, m, n) = (" in msg and "tile (" in msg and "bound" in msg, msg


def test_store_one_column_past_n_is_caught_by_the_sentinels():
    for name in PAST_N_CASES:
        c = BY_NAME[name]
        msg, _ = past_n_outcome(name)
        assert msg is not None and f"(b, m, n) = ({c['batch'] - 1}, {c['M'] - 1}, {c['N']})" in msg, msg
    # a guard row above the first member, the element before the window and the slack behind the last member are watched too
    plane = gp.make_tensors(BY_NAME[PAST_N_CASES[2]])["C"]
    for flat in (plane.off - 1, plane.off - plane.ld, plane.buf.numel() - 1, plane.off + plane.sb - 1):
        after = plane.buf.clone()
        after[flat] = 0.0
        with pytest.raises(AssertionError):
            gp.check_sentinels(plane, after, "C", "guards")


def test_what_the_tensor_wide_metric_misses(capsys):
    """A record, not an assertion: which seeded defects max |got - ref| / max |ref| < 2.5e-2 over the tensor (the metric and bf16
    tolerance of the older GEMM tests) lets through.  Every one of them fails the checker (the two tests above)."""
    rows = [(what, name, outcome(what, defect, name)) for what, defect, names in DEFECTS for name in names]
    rows += [(PAST_N, name, past_n_outcome(name)) for name in PAST_N_CASES]
    with capsys.disabled():
        print("\n  seeded defect, one edge tile                          case                                        rel_err < 2.5e-2    this checker")
        for what, name, (msg, passes) in rows:
            print(f"  {what:52s} {name:42s}  {'MISSES it' if passes else 'catches it':18s}  {'catches it' if msg else 'MISSES it'}")
        print(f"  the tensor-wide metric misses {sum(p for _, _, (_, p) in rows)} of {len(rows)}")


def test_a_nan_and_a_wrong_exact_zero_are_failures():
    c = BY_NAME["epi_pair_bf16_gate_f32out"]
    t = gp.make_tensors(c)
    parts = gp.reference_parts(c, t)
    good = gp.cpu_float32(c, t)
    bad = good.copy()
    bad[0, 3, 5] = np.nan
    with pytest.raises(AssertionError, match="tier 1"):
        judged(c, t, bad, parts)
    b, m, n = (int(i[0]) for i in np.nonzero(parts["zero"]))
    bad = good.copy()
    bad[b, m, n] = 1e-30                                            # far inside tier 1, but a gated-off element is exactly zero
    with pytest.raises(AssertionError, match="exact decision"):
        judged(c, t, bad, parts)


# ------------------------------------------------------------------------------------------------ the dispatch, without a device
def test_every_case_reaches_its_family_in_the_dry_run():
    rows = G.default_plans()
    assert len(rows) == len(G.PLANNED)
    wrong = [(c["name"], c["family"], r[:2]) for c, r in zip(G.PLANNED, rows) if c["family"] is not None and (r[0] != 0 or r[1] != c["family"])]
    assert not wrong, wrong
    for c, r in zip(G.PLANNED, rows):
        if c in G.REJECT:                                           # no gate / dropout on the skinny kernel; out_lp nowhere else
            assert (r[0] == -1) if c["lp"] else (r[0] == 0 and r[1] != "SKINNY"), (c["name"], r)
    fams = {(r[1], c["in_dt"]) for c, r in zip(G.PLANNED, rows)}
    assert {("PAIR", "bf16"), ("PAIR", "f32"), ("RING", "bf16"), ("SMALL", "bf16"), ("WIDE", "bf16"), ("SKINNY", "bf16"), ("SKINNY", "f32")} <= fams
    c576 = rows[[c["name"] for c in G.PLANNED].index("ring_130x200x576_sk4")]
    assert c576[5] == 3 == gp.eff_splitk(BY_NAME["ring_130x200x576_sk4"])      # 9 K tiles over 4 slices: 3 non-empty


@pytest.mark.parametrize("bundle", list(G.BUNDLES))
def test_every_bundle_changes_the_plan_and_reaches_its_kernels(bundle, tmp_path):
    default_file = tmp_path / "default_plans.json"
    default_file.write_text(json.dumps(G.default_plans()))
    env = {k: v for k, v in os.environ.items() if not k.startswith(G.SWITCH_PREFIXES)}
    env.update(G.BUNDLES[bundle][0], GEMM_PARITY_BUNDLE=bundle)
    r = subprocess.run([sys.executable, os.path.abspath(G.__file__), "--bundle-plan", bundle, str(default_file)], cwd=G.REPO, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bundle plan ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
