"""Float64 parity checker for pa_attn_fwd / pa_attn_bwd (TEST INFRASTRUCTURE; plain numpy / torch, no GPU).

One case table for tests/test_attn_parity_cpu.py (the checker tested on seeded defects) and tests/test_attn_float64_gpu.py (every kernel
of csrc/attention.hip, attention5.h and attention_x3.h held to it).  The layout follows tests/gemm_parity.py.

Reference: float64, from the stored operand values, of the documented function of include/plank_hip.h - scaled scores; kpm, causal
j <= i or the packed ranges of cu_q / cu_k; softmax over the allowed keys; dropout decisions of tests/dropout_masks.py attn_keep, the
survivors scaled by 1 / (1 - p); P V; lse - and the float64 gradient of that function (dQ, dK, dV) for the given dO.

Per-element error scale (first order, independent of the summation order):
    A_ij = scale sum_c |q_ic| |k_jc|      Abar_i = sum_j P_ij A_ij      w_ij = P_ij (1 + A_ij + Abar_i)      D_ij = keep_ij / (1 - p)
    Bm_ij = sum_c |dO_ic| |v_jc|          G_i = sum_j P_ij D_ij Bm_ij   T_ij = w_ij (D_ij Bm_ij + G_i)
    S_O = (w D) |v|     S_lse = 1 + Abar     S_dV = (w D)^T |dO|     S_dQ = scale T |k|     S_dK = scale T^T |q|

tier 1 (derived)   |got - ref| <= 2 eps S per element (+ half a bf16 ulp at max(|ref|, |got|) for a bf16 output, + 2^-23 |lse| for lse).
                   eps = n 2^-9 + (max(Lq, Lk) + dh + 8) 2^-24 with n the bf16 roundings between the inputs and that output, counted in the
                   kernels (bf16x3: 2^-15 per product in place of 2^-9); n = 0 for the first-generation f32 kernels:

                   family (forward)                       O  lse   where
                   B32  attn_fwd_bf16_kernel              1   0    P packed for the P V MFMA (attention.hip mma_tr3, pack_bf16)
                   V4   attn4_fwd_kernel                  2   1    q scale log2(e) re-rounded (scale_row4, l. 1663); P (pack_p4, l. 1788)
                   V5   attn5_fwd_kernel                  2   1    q scale log2(e) re-rounded (attention5.h l. 90); P (l. 287)
                   X3   attnx_fwd_kernel                  2   1    products Q K^T and P V, 2^-15 each

                   family (backward)                     dQ  dK  dV   + the lse count of the forward that produced lse
                   B32  attn_bwd_dq/dkv_bf16_kernel       2   2   1   O as stored, for delta (l. 1185); dS (mma_tr3 l. 1272 / 1409); P (l. 1408)
                   V4   attn4_bwd_dq/dkv/merged_kernel    3   3   2   the above + q resp. k scale log2(e) re-rounded (l. 1868 / 2050)
                   X3   attnx_bwd_dq/dkv_kernel           3   3   2   products Q K^T, dO V^T and dS K resp. dS^T Q / P^T dO
tier 2 (measured)  r(x) = max |x - ref| / (eps S) per case and output;  r(got) <= TIER2 r(emulation): plain torch on the CPU in torch's own
                   order, float32 throughout for the f32 kernels, float32 with the intermediates listed above rounded to bf16 (three-term
                   products for bf16x3) for the others.  profiles/attn_float64_parity.txt holds the measurements.
exact              dK / dV rows of masked keys, rows without an allowed key (O = 0, lse = 0, dQ = 0): S = 0 there, the bound is 0.
sentinels          o / dq / dk / dv / lse / delta are interior windows of buffers prefilled with gemm_parity.PATTERN; q / k / v are views of a
                   [rows, 3 H dh + 8] projection whose padding (and every other byte no launch may address) holds 2^60; K / V rows of
                   masked keys hold 2^20.
"""
import ctypes as C

import numpy as np
import torch

import dropout_masks as dm
import gemm_parity as gp

PA_F32, PA_BF16 = 0, 1
DT = gp.DT
POISON, PATTERN, GUARD_ROWS = gp.POISON, gp.PATTERN, gp.GUARD_ROWS
MASKED_KV = 2.0 ** 20
U24, U9, U15 = 2.0 ** -24, 2.0 ** -9, 2.0 ** -15
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
DROP_SEED = 4711
OUTPUTS = ("o", "lse", "dq", "dk", "dv")
REGIMES = ("gauss", "peaked", "ramp_up", "ramp_down", "steps", "late_spike", "offset")
FAMILIES = ("F32", "B32", "V4", "V5", "X3")

# bf16 roundings (bf16x3: three-term products) on the path to each output; the module docstring lists where each one is
N_FWD = {"F32": dict(o=0, lse=0), "B32": dict(o=1, lse=0), "V4": dict(o=2, lse=1), "V5": dict(o=2, lse=1), "X3": dict(o=2, lse=1)}
N_BWD = {"F32": dict(dq=0, dk=0, dv=0), "B32": dict(dq=2, dk=2, dv=1), "V4": dict(dq=3, dk=3, dv=2), "X3": dict(dq=3, dk=3, dv=2)}
# The tier-2 factor in force per family: 16 unless a correct family was MEASURED above it on the hardware (then twice its worst
# measured value, never above 256); profiles/attn_float64_parity.txt.
TIER2 = {"F32": 16.0, "B32": 16.0, "V4": 16.0, "V5": 16.0, "X3": 16.0}

# switch bundles (read once per process: each runs in a child of tests/test_attn_float64_gpu.py)
BUNDLES = {
    "default": {},
    "occupancies_unmerged_keysplit": {"PA_ATTN_V5_OCC": "2", "PA_ATTN_OCC": "43", "PA_X3_DKV_OCC": "2", "PA_ATTN_BWD_MERGE": "0", "PA_ATTN_KSPLIT": "2"},
    "no_v5_x3_parts": {"PA_ATTN_V5": "0", "PA_X3_PARTS": "2", "PA_X3_PARTS_MIN": "128"},
    "no_v4_no_v5": {"PA_ATTN_V4": "0", "PA_ATTN_V5": "0"},
    "v4_2": {"PA_ATTN_V4": "2"},
    "v5_2": {"PA_ATTN_V5": "2"},
    # with PA_ATTN_V4=0: at these sizes dh 64 reaches the 32-row-wave backward only without the 16-row-wave kernels
    "occ_43": {"PA_ATTN_OCC": "43", "PA_ATTN_V4": "0"},
    # PA_ATTN_KSPLIT=0: with at most 256 blocks the dQ launch would take the in-block key split instead of range blocks
    "range_blocks": {"PA_ATTN_SPLIT": "1", "PA_ATTN_SPLIT_KMAX": "2", "PA_ATTN_SPLIT_PMAX": "4", "PA_ATTN_KSPLIT": "0"},
    "ksplit_2_min_2": {"PA_ATTN_KSPLIT": "2", "PA_ATTN_KSPLIT_MIN": "2"},
}


# ------------------------------------------------------------------------------------------------ the case table
def _b(x):
    return "true" if x else "false"


def kernel_names(c):
    """(forward, backward) kernel names a case expects from pa_attn_plan, from the kinds it names."""
    dh, D, Cz = c["dh"], _b(c["drop"] > 0), _b(c["causal"])
    fwd = {"f32": f"attn_fwd_kernel<float, {dh}>", "b32": f"attn_fwd_bf16_kernel<{dh}, {D}>", "v4": f"attn4_fwd_kernel<{D}, 1>",
           "v4ks": f"attn4_fwd_kernel<{D}, 2>", "v5o3": f"attn5_fwd_kernel<{D}, 3, 3>", "v5o2": f"attn5_fwd_kernel<{D}, 4, 2>",
           "x3": f"attnx_fwd_kernel<64, {D}>"}[c["fwd"]]
    delta = f"attn_delta_kernel<float, {dh}>"
    bwd = {"f32": [delta, f"attn_bwd_dkv_kernel<float, {dh}>", f"attn_bwd_dq_kernel<float, {dh}>"],
           "b32": [f"attn_bwd_dq_bf16_kernel<{dh}, {D}, 3>", f"attn_bwd_dkv_bf16_kernel<{dh}, {D}, 2, {Cz}>"],
           "b32_43": [f"attn_bwd_dq_bf16_kernel<{dh}, {D}, 4>", f"attn_bwd_dkv_bf16_kernel<{dh}, {D}, 3, {Cz}>"],
           "merged": [f"attn4_bwd_merged_kernel<{D}, {Cz}>"],
           "unmerged": [f"attn4_bwd_dq_kernel<{D}, 1>", f"attn4_bwd_dkv_kernel<{D}, {Cz}>"],
           "unmerged_ks": [f"attn4_bwd_dq_kernel<{D}, 2>", f"attn4_bwd_dkv_kernel<{D}, {Cz}>"],
           "x3o1": [delta, f"attnx_bwd_dkv_kernel<64, {D}, 1>", f"attnx_bwd_dq_kernel<64, {D}>"],
           "x3o2": [delta, f"attnx_bwd_dkv_kernel<64, {D}, 2>", f"attnx_bwd_dq_kernel<64, {D}>"]}[c["bwd"]]
    return [fwd], bwd


_FAM_OF = {"f32": "F32", "b32": "B32", "b32_43": "B32", "v4": "V4", "v4ks": "V4", "v5o3": "V5", "v5o2": "V5", "x3": "X3", "merged": "V4",
           "unmerged": "V4", "unmerged_ks": "V4", "x3o1": "X3", "x3o2": "X3"}


def cases():
    """The case table.  Every case runs under ONE switch bundle and names the kernels it expects there; the regimes rotate through the
    cases of a family so that every family meets every regime (tests/test_attn_parity_cpu.py asserts it)."""
    cs = []
    turn = {}

    def add(tag, dt, dh, Lq, Lk, fwd, bwd, *, B=2, H=2, causal=0, mask=None, layout="dense", lens=None, order=0, drop=0.0, bundle="default",
            regime=None, ws=0):
        fam = _FAM_OF[fwd]
        if lens is not None:
            B = len(lens)
            Lk = max(lens)
            if layout == "packed_self":
                Lq = Lk
        wide = bool({fam, _FAM_OF[bwd]} & {"V4", "V5"})             # q (k) scale log2(e) re-rounded: eps (1 + A + Abar) is large where |q| |k| is
        while regime is None:
            i = turn.get(fam, 0)
            turn[fam] = i + 1
            regime = REGIMES[i % len(REGIMES)]
            # Inputs under which a seeded defect of tests/test_attn_parity_cpu.py would sit inside the bound of a CORRECT kernel are not used:
            # a missing 1 / (1 - p) moves an output by at most p / (1 - p) = 0.25 of a tile's share, below 2 eps (1 + A + Abar) of these
            # families at A ~ 30 (peaked) or 12 (the spike); one of five key tiles missing from lse is log(5 / 4) = 0.22 against 2 eps 61.
            if wide and ((drop and regime in ("peaked", "late_spike")) or (regime == "offset" and Lk > 256)):
                regime = None
        x3 = int(fam == "X3")
        name = f"{bundle}:{tag}_{dt}_dh{dh}_{Lq}x{Lk}{'_causal' if causal else ''}{'_' + mask if mask else ''}" \
               f"{'_' + layout if layout != 'dense' else ''}{'_order' if order else ''}{'_drop' if drop else ''}_{regime}"
        cs.append(dict(name=name, dt=dt, dh=dh, Lq=Lq, Lk=Lk, B=B, H=H, causal=causal, mask=mask, layout=layout, lens=lens, order=order, drop=drop,
                       bundle=bundle, regime=regime, fwd=fwd, bwd=bwd, fam=fam, bfam=_FAM_OF[bwd], x3=x3, ws=ws))

    # ---- first-generation f32: dh 16 / 32 / 64, rectangular and causal
    for i, (dh, (Lq, Lk, causal)) in enumerate((dh, s) for dh in (16, 32, 64) for s in ((70, 100, 0), (130, 130, 1), (129, 300, 0))):
        if dh == 64 and Lq == 129:
            continue                                                # (keeps the float64 work of the CPU test down)
        add("f32", "f32", dh, Lq, Lk, "f32", "f32", causal=causal, drop=0.2 if i % 3 == 1 else 0.0, mask="hole" if i % 3 == 0 else None)
    # ---- bf16, 32-row waves: dh 16 / 32 by default; every DROP x CAUSAL instantiation
    for dh in (16, 32):
        for drop, causal, (Lq, Lk) in ((0.0, 0, (70, 100)), (0.2, 1, (130, 130)), (0.2, 0, (129, 300)), (0.0, 1, (130, 130))):
            add("b32", "bf16", dh, Lq, Lk, "b32", "b32", causal=causal, drop=drop, mask="hole" if (Lq, causal) == (70, 0) else None)
    for dh in (16, 32, 64):                                          # four / three blocks per CU
        for drop, causal, (Lq, Lk) in ((0.0, 0, (70, 100)), (0.2, 1, (130, 130)), (0.2, 0, (129, 200)), (0.0, 1, (70, 70))):
            add("b32_occ", "bf16", dh, Lq, Lk, "v5o3" if (dh == 64 and Lq > 128 and not causal) else "b32", "b32_43", causal=causal, drop=drop, bundle="occ_43")
    for drop, causal, (Lq, Lk) in ((0.0, 0, (70, 100)), (0.2, 1, (130, 130)), (0.2, 0, (129, 300)), (0.0, 1, (130, 130))):   # dh 64 without v4 / v5
        add("b32", "bf16", 64, Lq, Lk, "b32", "b32", causal=causal, drop=drop, bundle="no_v4_no_v5")
    # ---- v4 forward unsplit / in-block key split (five key tiles: an odd count; four), merged backward (gq % 8 == 0)
    for drop in (0.0, 0.2):
        add("v4", "bf16", 64, 70, 100, "v4", "merged", B=1, H=8, drop=drop, mask="hole" if drop else None)
        add("v4", "bf16", 64, 128, 130, "v4", "merged", B=1, H=8, causal=1, drop=drop)
        add("v4_split", "bf16", 64, 128, 300, "v4ks", "merged", B=1, H=8, drop=drop)
    add("v4_split", "bf16", 64, 128, 256, "v4ks", "merged", B=1, H=8)
    add("v4_split", "bf16", 64, 128, 0, "v4ks", "unmerged_ks", layout="packed_keys", lens=[40, 577], drop=0.2)     # element 0 runs unsplit
    # ---- unmerged backward: dQ with and without the key split, dK / dV causal and not; v5 forward (Lq > 128, not causal)
    for drop in (0.0, 0.2):
        add("v5", "bf16", 64, 129, 300, "v5o3", "unmerged_ks", drop=drop)
        add("v5", "bf16", 64, 260, 200, "v5o3", "unmerged", drop=drop, mask="hole" if drop else None)
        add("v4", "bf16", 64, 260, 260, "v4", "unmerged", causal=1, drop=drop)
        add("v5", "bf16", 64, 300, 129, "v5o2", "unmerged", drop=drop, bundle="occupancies_unmerged_keysplit")
        add("v5", "bf16", 64, 129, 300, "v5o2", "unmerged_ks", drop=drop, bundle="occupancies_unmerged_keysplit")
    add("v4_split", "bf16", 64, 128, 300, "v4ks", "unmerged_ks", B=1, H=8, bundle="occupancies_unmerged_keysplit")  # BWD_MERGE=0
    add("b32_occ", "bf16", 16, 129, 200, "b32", "b32_43", bundle="occupancies_unmerged_keysplit")
    for Lq, Lk in ((70, 100), (128, 300)):                           # V5=2: every non-causal launch, a single query tile included
        add("v5", "bf16", 64, Lq, Lk, "v5o3", "merged", B=1, H=8, bundle="v5_2", drop=0.2 if Lq == 70 else 0.0)
    add("v5", "bf16", 64, 300, 300, "v5o3", "unmerged_ks", bundle="v5_2")
    add("v4", "bf16", 64, 260, 300, "v4ks", "unmerged_ks", bundle="no_v5_x3_parts")       # V5=0: the v4 forward at two query tiles
    add("v4", "bf16", 64, 260, 200, "v4", "unmerged", bundle="no_v5_x3_parts", drop=0.2)
    add("v5", "bf16", 64, 129, 300, "v5o3", "unmerged_ks", bundle="v4_2")
    add("v4", "bf16", 64, 70, 100, "v4", "merged", B=1, H=8, bundle="v4_2", causal=1)
    add("v4_split", "bf16", 64, 128, 130, "v4", "merged", B=1, H=8, bundle="ksplit_2_min_2")        # three key tiles: under four, never split
    add("v5", "bf16", 64, 260, 256, "v5o3", "unmerged_ks", bundle="ksplit_2_min_2", drop=0.2)
    add("v4_split", "bf16", 64, 128, 0, "v4ks", "unmerged_ks", layout="packed_keys", lens=[40, 130, 300], bundle="ksplit_2_min_2")   # 130 keys: three tiles, split
    # ---- bf16x3 (f32 launches with dh 64 while pa_attn_split_config(1))
    for drop in (0.0, 0.2):
        add("x3", "f32", 64, 70, 100, "x3", "x3o1", drop=drop, mask="hole" if drop else None)
        add("x3", "f32", 64, 130, 130, "x3", "x3o1", causal=1, drop=drop)
        add("x3", "f32", 64, 129, 200, "x3", "x3o2", drop=drop, bundle="occupancies_unmerged_keysplit")
        add("x3", "f32", 64, 200, 200, "x3", "x3o1", drop=drop, bundle="no_v5_x3_parts")          # parts_q = parts_kv = 2
    add("x3", "f32", 64, 129, 0, "x3", "x3o1", layout="packed_self", lens=[129, 40, 200], bundle="no_v5_x3_parts")
    # ---- packed self-attention with `order` (H = 8: length-balanced block order)
    add("packed", "bf16", 64, 0, 0, "v5o3", "unmerged_ks", H=8, layout="packed_self", lens=[300, 1, 129, 64], order=1, drop=0.2)
    add("packed", "bf16", 64, 0, 0, "v5o3", "unmerged_ks", H=8, layout="packed_self", lens=[300, 1, 129, 64], order=1)
    add("packed", "f32", 32, 0, 0, "f32", "f32", H=2, layout="packed_self", lens=[130, 1, 70])
    add("packed", "bf16", 32, 0, 0, "b32", "b32", H=8, layout="packed_self", lens=[130, 1, 70], order=1, drop=0.2)
    # ---- range blocks: the merge with unequal partial maxima, at three elements instead of a thousand rows
    for regime, drop in (("steps", 0.0), ("ramp_up", 0.2), ("late_spike", 0.0), ("gauss", 0.2)):
        add("ranges", "bf16", 64, 0, 0, "v5o3", "unmerged", H=8, layout="packed_self", lens=[300, 64, 577], order=1, drop=drop, bundle="range_blocks",
            regime=regime, ws=1)
    # ---- rows without an allowed key, in every family
    for dt, dh, fwd, bwd, H8 in (("f32", 16, "f32", "f32", 0), ("bf16", 32, "b32", "b32", 0), ("bf16", 64, "v4", "merged", 1), ("f32", 64, "x3", "x3o1", 0)):
        kw = dict(B=1, H=8) if H8 else {}
        add("keyless", dt, dh, 70, 70, fwd, bwd, causal=1, mask="key0", regime="gauss", **kw)
        add("keyless", dt, dh, 70, 0, fwd, "unmerged" if H8 else bwd, layout="packed_keys", lens=[70, 0, 130], regime="ramp_down", drop=0.2)
        add("keyless", dt, dh, 70, 100, fwd, "unmerged" if H8 else bwd, mask="all_b1", regime="gauss", B=2)
    add("keyless", "bf16", 64, 129, 200, "v5o3", "unmerged", mask="all_b1", regime="gauss")
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


# ------------------------------------------------------------------------------------------------ geometry, inputs
def elements(c):
    """Per batch element: (first q row, q rows, first k row, k rows) in the row numbering of the q resp. k / v matrices."""
    B, Lq, Lk = c["B"], c["Lq"], c["Lk"]
    if c["layout"] == "dense":
        return [(b * Lq, Lq, b * Lk, Lk) for b in range(B)]
    cu = np.concatenate(([0], np.cumsum(c["lens"]))).astype(int)
    if c["layout"] == "packed_self":
        return [(int(cu[b]), int(c["lens"][b]), int(cu[b]), int(c["lens"][b])) for b in range(B)]
    return [(b * Lq, Lq, int(cu[b]), int(c["lens"][b])) for b in range(B)]


def key_mask(c):
    """kpm uint8 [B, Lk] (1 = masked) or None."""
    if not c["mask"]:
        return None
    B, Lk = c["B"], c["Lk"]
    m = np.zeros((B, Lk), dtype=np.uint8)
    if c["mask"] == "hole":                                         # holes inside tiles, a masked tail of different length per element
        for b in range(B):
            m[b, [3, 17, min(66, Lk - 2)]] = 1
            m[b, Lk - 5 - 9 * b:] = 1
    elif c["mask"] == "key0":
        m[:, 0] = 1
        m[-1, 5] = 1
    elif c["mask"] == "all_b1":
        m[B - 1, :] = 1
        m[0, 7] = 1
    return m


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _regime_qk(regime, g, Lq, Lk, H, dh, scale):
    """q [Lq, H, dh], k [Lk, H, dh] of one batch element (float32 holding bf16 values)."""
    rn = lambda *s: torch.randn(*s, generator=g)
    i, j = torch.arange(Lq, dtype=torch.float32), torch.arange(Lk, dtype=torch.float32)
    if regime == "gauss":
        return rn(Lq, H, dh), rn(Lk, H, dh)
    if regime == "peaked":                                          # scores of standard deviation ~ 6 natural units
        s = 6.0 ** 0.5
        return rn(Lq, H, dh) * s, rn(Lk, H, dh) * s
    q, k = rn(Lq, H, dh) * 0.5, rn(Lk, H, dh) * 0.5
    q[..., 0:2] = 0
    k[..., 0:2] = 0
    if regime in ("ramp_up", "ramp_down"):                          # 3 log2 units per 64-key tile along e_0
        per_key = 3.0 * LN2 / 64.0 * (1 if regime == "ramp_up" else -1)
        q[..., 0] = 4.0
        k[..., 0] = (per_key * j / (4.0 * scale))[:, None]
    elif regime == "steps":                                         # jumps of 7 natural (10 log2) units at tile boundaries and inside tiles
        level = sum((j >= t).float() for t in (64, 144, 208, 320, 400, 528))
        q[..., 0] = 4.0
        k[..., 0] = (7.0 * level / (4.0 * scale))[:, None]
    elif regime == "late_spike":                                    # odd rows: a key of the last (ragged) tile; even rows: the first key
        a = 8.0
        c = 12.0 / (a * scale)
        q[1::2, :, 0] = a
        q[0::2, :, 1] = a
        if Lk:
            k[max(Lk - 4, 0), :, 0] = c
            k[0, :, 1] = c                                           # (key 0: an element that reads one row too many meets the next one's spike)
    elif regime == "offset":                                        # all scores of a row near +60 or -60 natural units
        a = 8.0
        q[..., 0] = (a * (1 - 2 * ((torch.arange(Lq) // 2) % 2)).float())[:, None]
        k[..., 0] = 60.0 / (a * scale)
    return q, k


class Tensors:
    """The operands of a case on the CPU.  Planes (gemm_parity.Plane): xq / xkv the packed projections (one buffer when q, k and v have the
    same rows), do, and the outputs o, dq, dk, dv, lse, delta."""

    def __init__(self, c, values=True):
        B, H, dh, Lq, Lk = c["B"], c["H"], c["dh"], c["Lq"], c["Lk"]
        self.c, self.dm = c, H * dh
        dmod, dt = self.dm, DT[c["dt"]]
        self.scale = float(np.float32(dh ** -0.5))
        self.el = elements(c)
        self.Rq = max(e[0] + e[1] for e in self.el)
        self.Rk = max(e[2] + e[3] for e in self.el)
        self.shared = c["layout"] == "packed_self" or (c["layout"] == "dense" and Lq == Lk)
        self.kpm = key_mask(c)
        P = gp.Plane
        self.planes = {}
        self.planes["xq"] = P(1, self.Rq, 3 * dmod, dt, POISON, 2, alloc=values)
        if not self.shared:
            self.planes["xkv"] = P(1, self.Rk, 3 * dmod, dt, POISON, 2, alloc=values)
        self.planes["do"] = P(1, self.Rq, dmod, dt, POISON, 2, alloc=values)
        for key, rows in (("o", self.Rq), ("dq", self.Rq), ("dk", self.Rk), ("dv", self.Rk)):
            self.planes[key] = P(1, rows, dmod, dt, PATTERN, GUARD_ROWS, alloc=values)
        for key in ("lse", "delta"):
            self.planes[key] = P(1, 1, B * H * Lq, torch.float32, PATTERN, 0, lead=64, extra=64, alloc=values)
        self.cu = None
        if c["lens"] is not None:
            self.cu = torch.tensor(np.concatenate(([0], np.cumsum(c["lens"]))), dtype=torch.int32)
        self.order = torch.argsort(torch.tensor(c["lens"]), descending=True, stable=True).to(torch.int32) if c["order"] else None
        if not values:
            return
        g = torch.Generator().manual_seed(1000 * (sum(map(ord, c["name"])) % 997) + 7)
        q, k = torch.zeros(self.Rq, H, dh), torch.zeros(self.Rk, H, dh)
        for (q0, nq, k0, nk) in self.el:
            qe, ke = _regime_qk(c["regime"], g, nq, nk, H, dh, self.scale)
            q[q0:q0 + nq] = qe
            k[k0:k0 + nk] = ke
        v = torch.randn(self.Rk, H, dh, generator=g)
        do = torch.randn(self.Rq, H, dh, generator=g)
        q, k, v, do = _bf(q), _bf(k), _bf(v), _bf(do)
        if self.kpm is not None:                                    # rows of masked keys: large, finite
            for b, (_, _, k0, nk) in enumerate(self.el):
                rows = torch.from_numpy(np.nonzero(self.kpm[b, :nk])[0]) + k0
                k[rows] = MASKED_KV
                v[rows] = MASKED_KV
        self.q, self.k, self.v, self.do = q, k, v, do
        xq = self.planes["xq"].view()[0]
        xk = xq if self.shared else self.planes["xkv"].view()[0]
        xq[:, :dmod] = q.reshape(self.Rq, dmod).to(dt)
        xk[:, dmod:2 * dmod] = k.reshape(self.Rk, dmod).to(dt)
        xk[:, 2 * dmod:] = v.reshape(self.Rk, dmod).to(dt)
        self.planes["do"].set(do.reshape(1, self.Rq, dmod).to(dt))

    def allowed(self, b):
        """bool [Lq_b, Lk_b] of batch element b."""
        _, nq, _, nk = self.el[b]
        a = np.ones((nq, nk), dtype=bool)
        if self.c["causal"]:
            a &= np.arange(nk)[None, :] <= np.arange(nq)[:, None]
        if self.kpm is not None:
            a &= (self.kpm[b, :nk] == 0)[None, :]
        return a

    def keep(self, b):
        """Dropout decisions bool [H, Lq_b, Lk_b] of batch element b (row = (b H + h) Lq + i, key = j inside the element), or None."""
        c = self.c
        if not c["drop"]:
            return None
        _, nq, _, nk = self.el[b]
        rows = (b * c["H"] + np.arange(c["H"])[:, None]) * c["Lq"] + np.arange(nq)[None, :]
        return dm.attn_keep(DROP_SEED, rows, nk, c["drop"])

    def lse_valid(self):
        """bool [B, H, Lq]: rows of lse a launch writes (rows past a packed element's length stay untouched)."""
        c = self.c
        ok = np.zeros((c["B"], c["H"], c["Lq"]), dtype=bool)
        for b, (_, nq, _, _) in enumerate(self.el):
            ok[b, :, :nq] = True
        return ok


# ------------------------------------------------------------------------------------------------ float64 reference
def _core64(q, k, v, do, allowed, D, scale, scales=True):
    """One batch element in float64.  q, do [H, Lq, dh]; k, v [H, Lk, dh]; allowed bool, D = keep / (1 - p) [H, Lq, Lk] (None: no dropout)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = scale * np.einsum("hic,hjc->hij", q, k)
        sm = np.where(allowed, s, -np.inf)
        m = sm.max(axis=-1, initial=-np.inf)
        has = np.isfinite(m)
        ms = np.where(has, m, 0.0)
        e = np.where(allowed, np.exp(np.where(allowed, s, 0.0) - ms[..., None]), 0.0)
        l = e.sum(-1)
        P = e / np.where(has, l, 1.0)[..., None]
        lse = np.where(has, ms + np.log(np.where(has, l, 1.0)), 0.0)
    D = np.ones_like(P) if D is None else D
    PD = P * D
    out = dict(P=P, D=D)
    out["o"] = np.einsum("hij,hjc->hic", PD, v)
    out["lse"] = lse
    vz = np.where(np.abs(v) >= MASKED_KV, 0.0, v)                   # (masked rows: P is 0 there; keeps inf * 0 out of the sums)
    kz = np.where(np.abs(k) >= MASKED_KV, 0.0, k)
    dP = D * np.einsum("hic,hjc->hij", do, vz)
    delta = (P * dP).sum(-1)
    dS = P * (dP - delta[..., None])
    out["dq"] = scale * np.einsum("hij,hjc->hic", dS, kz)
    out["dk"] = scale * np.einsum("hij,hic->hjc", dS, q)
    out["dv"] = np.einsum("hij,hic->hjc", PD, do)
    if scales:
        A = scale * np.einsum("hic,hjc->hij", np.abs(q), np.abs(kz))
        Abar = (P * A).sum(-1)
        w = P * (1.0 + A + Abar[..., None])
        Bm = np.einsum("hic,hjc->hij", np.abs(do), np.abs(vz))
        G = (PD * Bm).sum(-1)
        T = w * (D * Bm + G[..., None])
        out["S_o"] = np.einsum("hij,hjc->hic", w * D, np.abs(vz))
        out["S_lse"] = 1.0 + Abar
        out["S_dv"] = np.einsum("hij,hic->hjc", w * D, np.abs(do))
        out["S_dq"] = scale * np.einsum("hij,hjc->hic", T, np.abs(kz))
        out["S_dk"] = scale * np.einsum("hij,hic->hjc", T, np.abs(q))
    return out


def _hfirst(x, r0, n):
    return x[r0:r0 + n].to(torch.float64).numpy().transpose(1, 0, 2)        # [rows, H, dh] -> [H, n, dh]


def reference(c, t, element_hook=None, scales=True, only=None):
    """Float64 reference of a case: o, dq [Rq, H, dh]; dk, dv [Rk, H, dh]; lse [B, H, Lq] (0 where no launch writes) and the scales S_*.
    element_hook(b, q, k, v, do, allowed, D) -> the same tuple, changed: how the seeded defects of the checker's test get in (a defect
    may lengthen k / v: the gradients of the extra rows land on the rows that follow in the buffer).  only: the batch elements wanted."""
    H, dh = c["H"], c["dh"]
    ref = {k_: np.zeros((t.Rq if k_ in ("o", "dq") else t.Rk, H, dh)) for k_ in ("o", "dq", "dk", "dv")}
    ref["lse"] = np.zeros((c["B"], H, c["Lq"]))
    if scales:
        for k_ in ("o", "dq", "dk", "dv"):
            ref["S_" + k_] = np.zeros_like(ref[k_])
        ref["S_lse"] = np.ones_like(ref["lse"])
    dscale = dm.attn_scale(c["drop"]) if c["drop"] else 1.0
    for b, (q0, nq, k0, nk) in enumerate(t.el):
        if nq == 0 or (only is not None and b not in only):
            continue
        q, do = _hfirst(t.q, q0, nq), _hfirst(t.do, q0, nq)
        k, v = _hfirst(t.k, k0, nk), _hfirst(t.v, k0, nk)
        allowed = np.broadcast_to(t.allowed(b), (H, nq, nk)).copy()
        keep = t.keep(b)
        D = None if keep is None else keep * dscale
        if element_hook is not None:
            q, k, v, do, allowed, D = element_hook(b, q, k, v, do, allowed, D)
        r = _core64(q, k, v, do, allowed, D, t.scale, scales)
        nk_ = nk
        nx = min(r["dk"].shape[1], t.Rk - k0)
        for k_ in ("o", "dq"):
            ref[k_][q0:q0 + nq] = r[k_].transpose(1, 0, 2)
        for k_ in ("dk", "dv"):
            ref[k_][k0:k0 + nx] += r[k_][:, :nx].transpose(1, 0, 2)
        ref["lse"][b, :, :nq] = r["lse"]
        if scales:
            for k_ in ("o", "dq"):
                ref["S_" + k_][q0:q0 + nq] = r["S_" + k_].transpose(1, 0, 2)
            for k_ in ("dk", "dv"):
                ref["S_" + k_][k0:k0 + nk] = r["S_" + k_][:, :nk_].transpose(1, 0, 2)
            ref["S_lse"][b, :, :nq] = r["S_lse"]
    return ref


# ------------------------------------------------------------------------------------------------ float32 emulation
def _split3(x):
    hi = _bf(x)
    return hi, _bf(x - hi)


def _mm(a, b, x3):
    """a @ b in float32; bf16x3: hi hi + hi lo + lo hi of the operands' bf16 parts."""
    if not x3:
        return torch.matmul(a, b)
    ah, al = _split3(a)
    bh, bl = _split3(b)
    return torch.matmul(ah, bh) + torch.matmul(ah, bl) + torch.matmul(al, bh)


def emulate(c, t):
    """The kernels' arithmetic in plain torch float32 on the CPU, in torch's own order, with the roundings of the family: o, lse, and the
    backward from the emulated stored o and lse.  Returns float64 arrays shaped as reference()."""
    H, dh, fam, bfam = c["H"], c["dh"], c["fam"], c["bfam"]
    out_bf = c["dt"] == "bf16"
    st = (lambda x: _bf(x)) if out_bf else (lambda x: x)
    rnd_f = lambda on: (_bf if on else (lambda x: x))
    r_q = rnd_f(fam in ("V4", "V5"))
    r_p = rnd_f(fam in ("B32", "V4", "V5"))
    r_qb = rnd_f(bfam == "V4")
    r_pb = rnd_f(bfam in ("B32", "V4"))
    x3f, x3b = fam == "X3", bfam == "X3"
    out = {k_: np.zeros((t.Rq if k_ in ("o", "dq") else t.Rk, H, dh)) for k_ in ("o", "dq", "dk", "dv")}
    out["lse"] = np.zeros((c["B"], H, c["Lq"]))
    scale = torch.tensor(t.scale, dtype=torch.float32)
    dscale = float(np.float32(dm.attn_scale(c["drop"]))) if c["drop"] else 1.0
    sl = scale * np.float32(LOG2E)
    for b, (q0, nq, k0, nk) in enumerate(t.el):
        if nq == 0:
            continue
        q, do = (x[q0:q0 + nq].transpose(0, 1).contiguous() for x in (t.q, t.do))
        k, v = (x[k0:k0 + nk].transpose(0, 1).contiguous() for x in (t.k, t.v))
        allowed = torch.from_numpy(t.allowed(b))[None].expand(H, nq, nk)
        keep = t.keep(b)
        D = torch.ones(H, nq, nk) if keep is None else torch.from_numpy(keep).float() * dscale
        masked_rows = (k.abs() >= MASKED_KV).any(-1, keepdim=True)
        kz, vz = torch.where(masked_rows, torch.zeros_like(k), k), torch.where(masked_rows, torch.zeros_like(v), v)
        neg = torch.full((), float("-inf"))

        def scores2(qq, kk, rq, rk, x3):                            # log2 units
            if rq is not None:
                return _mm(rq(qq * sl), kk.transpose(1, 2), x3)
            if rk is not None:
                return _mm(qq, rk(kk * sl).transpose(1, 2), x3)
            return _mm(qq, kk.transpose(1, 2), x3) * sl
        s2 = torch.where(allowed, scores2(q, kz, r_q if fam in ("V4", "V5") else None, None, x3f), neg)
        m = s2.max(-1).values if nk else torch.full((H, nq), float("-inf"))
        has = torch.isfinite(m)
        ms = torch.where(has, m, torch.zeros_like(m))
        e = torch.where(allowed, torch.exp2(torch.where(allowed, s2, torch.zeros_like(s2)) - ms[..., None]), torch.zeros_like(s2))
        l = e.sum(-1)
        linv = torch.where(has, 1.0 / torch.where(has, l, torch.ones_like(l)), torch.zeros_like(l))
        o = st(_mm(r_p(e) * (D > 0), vz, x3f) * (dscale * linv)[..., None])
        lse = torch.where(has, (ms + torch.log2(torch.where(has, l, torch.ones_like(l)))) * np.float32(LN2), torch.zeros_like(l))
        # backward, from the stored o and lse
        delta = (o * do).sum(-1)
        lse2 = lse * np.float32(LOG2E)

        def probs(rq, rk):
            s = scores2(q, kz, rq, rk, x3b)
            return torch.where(allowed & has[..., None], torch.exp2(s - lse2[..., None]), torch.zeros_like(s))
        p_q = probs(r_qb if bfam == "V4" else None, None)
        p_k = probs(None, r_qb if bfam == "V4" else None)
        dP = _mm(do, vz.transpose(1, 2), x3b) * D
        dS_q = r_pb(p_q * (dP - delta[..., None]))
        dS_k = r_pb(p_k * (dP - delta[..., None]))
        dq = st(_mm(dS_q, kz, x3b) * scale)
        dk = st(_mm(dS_k.transpose(1, 2), q, x3b) * scale)
        dv = st(_mm((r_pb(p_k) * D).transpose(1, 2), do, x3b))
        for k_, x in (("o", o), ("dq", dq)):
            out[k_][q0:q0 + nq] = x.double().numpy().transpose(1, 0, 2)
        for k_, x in (("dk", dk), ("dv", dv)):
            out[k_][k0:k0 + nk] = x.double().numpy().transpose(1, 0, 2)
        out["lse"][b, :, :nq] = lse.double().numpy()
    return out


# ------------------------------------------------------------------------------------------------ the checks
def eps_of(c, what):
    """eps of one output of a case (module docstring)."""
    f32 = (max(c["Lq"], c["Lk"]) + c["dh"] + 8) * U24
    if what in ("o", "lse"):
        n, u = N_FWD[c["fam"]][what], (U15 if c["fam"] == "X3" else U9)
    else:
        n_own, u = N_BWD[c["bfam"]][what], (U15 if c["bfam"] == "X3" else U9)
        n_lse = N_FWD[c["fam"]]["lse"]
        return n_own * u + n_lse * (U15 if c["fam"] == "X3" else U9) + f32
    return n * u + f32


def ratio(x, ref, S, eps):
    """r(x) = max |x - ref| / (eps S) over the elements with S > 0 (a non-finite x: inf)."""
    x = np.asarray(x, dtype=np.float64)
    if not np.isfinite(x).all():
        return float("inf")
    ok = S > 0
    return float((np.abs(x - ref)[ok] / (eps * S[ok])).max()) if ok.any() else 0.0


def _where(c, what, idx):
    idx = tuple(int(i) for i in idx)
    if what == "lse":
        b, h, i = idx
        return f"(b, h, row) = ({b}, {h}, {i}), query tile {i // 128}, 16-row wave {i % 128 // 16}, 32-row wave {i % 128 // 32}"
    r, h, col = idx
    side = "q" if what in ("o", "dq") else "k"
    for b, (q0, nq, k0, nk) in enumerate(elements(c)):
        r0, n = (q0, nq) if side == "q" else (k0, nk)
        if r0 <= r < r0 + n:
            i = r - r0
            return f"(row, h, c) = ({r}, {h}, {col}): element {b} {side}-row {i} of {n}, 128-row tile {i // 128}, 64-row tile {i // 64}, row {i % 64} in it"
    return f"(row, h, c) = {idx}"


def check_output(c, what, got, ref, S, *, r_emu=None, out_bf16=None):
    """Assert one output per element (tier 1, which holds the exact zeros where S = 0, then tier 2).  Returns r(got)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == S.shape, (c["name"], what, got.shape, ref.shape)
    eps = eps_of(c, what)
    fam = c["fam"] if what in ("o", "lse") else c["bfam"]
    tag = f"{c['name']} {what} [{fam}]"
    bound = 2.0 * eps * S
    if what == "lse":
        bound = bound + 2.0 ** -23 * np.abs(ref)
    elif (c["dt"] == "bf16") if out_bf16 is None else out_bf16:
        bound = bound + gp.half_ulp_bf16(np.maximum(np.abs(ref), np.abs(np.where(np.isfinite(got), got, 0.0))))
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - ref) <= bound)                         # (a NaN is never inside)
    if bad.any():
        err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
        with np.errstate(over="ignore"):
            rel = np.where(bad, err / np.maximum(bound, 1e-300), 0.0)
        idx = np.unravel_index(int(np.argmax(rel)), rel.shape)
        zero = " (an exact zero: masked key or row without keys)" if S[idx] == 0 else ""
        raise AssertionError(f"{tag}: tier 1: {int(bad.sum())} of {bad.size} elements outside the bound; worst at {_where(c, what, idx)}: got {got[idx]!r}, "
                             f"ref {ref[idx]!r}, |got - ref| = {rel[idx]:.3g} x the bound ({bound[idx]:.3g}){zero}")
    r = ratio(got, ref, S, eps)
    if r_emu is not None:
        f = TIER2[fam]
        if not r <= f * r_emu:
            ok = S > 0
            rr = np.where(ok, np.abs(got - ref) / np.where(ok, eps * S, 1.0), 0.0)
            idx = np.unravel_index(int(np.argmax(rr)), rr.shape)
            raise AssertionError(f"{tag}: tier 2: r(got) = {r:.4g} > {f:g} x r(emulation) = {f:g} x {r_emu:.4g}; worst at {_where(c, what, idx)}: "
                                 f"got {got[idx]!r}, ref {ref[idx]!r}")
    return r


def check_all(c, got, ref, emu=None):
    """Every output of a case; `got`, `emu`: dicts shaped as reference().  Returns {output: (r(got), r(emulation))}."""
    rs = {}
    for what in OUTPUTS:
        S = ref["S_" + what]
        r_emu = ratio(emu[what], ref[what], S, eps_of(c, what)) if emu is not None else None
        rs[what] = (check_output(c, what, got[what], ref[what], S, r_emu=r_emu), r_emu)
    return rs


def store(c, x):
    """What a kernel stores of a value: itself as float32, or its round-to-nearest bf16 image (as float64)."""
    v = torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32)
    return (v.to(torch.bfloat16) if c["dt"] == "bf16" else v).to(torch.float64).numpy()


def stored(c, outs):
    return {k_: (store(c, v) if k_ != "lse" else np.asarray(v, dtype=np.float32).astype(np.float64)) for k_, v in outs.items() if k_ in OUTPUTS}


def old_metric_passes(c, got, ref):
    """The metric of tests/test_kernels_gpu.py: max |got - ref| / max |ref| over the tensor, below 2.5e-2 (bf16) / 1e-4 (f32), for o, dq,
    dk and dv (lse is not held to it there)."""
    tol = 2.5e-2 if c["dt"] == "bf16" else 1e-4
    for what in ("o", "dq", "dk", "dv"):
        g, r = np.asarray(got[what], dtype=np.float64), ref[what]
        if not np.isfinite(g).all() or np.abs(g - r).max() / max(np.abs(r).max(), 1e-30) >= tol:
            return False
    return True


# ------------------------------------------------------------------------------------------------ the argument block
def fake_ptr(key, plane, col=0):
    return gp.FAKE_BASE.get(key, 0x90000000 + 0x10000000 * (sum(map(ord, key)) % 6)) + (plane.off + col) * plane.buf.element_size()


FAKE_AUX = {"kpm": 0x20000000, "cu": 0x30000000, "order": 0x40000000, "ws": 0x50000000}


def attn_args(L, c, t, ptr=fake_ptr, aux=FAKE_AUX, ws_bytes=0):
    """The pa_attn_args block of a case, built directly so that every operand is a window of a guarded buffer.  ptr(key, plane, col) ->
    address of column `col` of the window's first row; aux: addresses of kpm / cu / order / ws."""
    a = L.AttnArgs()
    dmod, pl = t.dm, t.planes
    kv = "xq" if t.shared else "xkv"
    a.q, a.k, a.v = ptr("xq", pl["xq"], 0), ptr(kv, pl[kv], dmod), ptr(kv, pl[kv], 2 * dmod)
    a.o, a.lse = ptr("o", pl["o"]), ptr("lse", pl["lse"])
    a.B, a.H, a.Lq, a.Lk, a.dh = c["B"], c["H"], c["Lq"], c["Lk"], c["dh"]
    a.ldq, a.ldk, a.ldv, a.ldo = pl["xq"].ld, pl[kv].ld, pl[kv].ld, pl["o"].ld
    a.causal, a.scale, a.drop_p, a.drop_seed = int(c["causal"]), t.scale, c["drop"], DROP_SEED
    a.dtype = PA_BF16 if c["dt"] == "bf16" else PA_F32
    a.dout, a.dq, a.dk, a.dv, a.delta = ptr("do", pl["do"]), ptr("dq", pl["dq"]), ptr("dk", pl["dk"]), ptr("dv", pl["dv"]), ptr("delta", pl["delta"])
    a.lddo, a.lddq, a.lddk, a.lddv = pl["do"].ld, pl["dq"].ld, pl["dk"].ld, pl["dv"].ld
    if t.kpm is not None:
        a.kpm = aux["kpm"]
    if c["layout"] != "dense":
        a.cu_k = aux["cu"]
        if c["layout"] == "packed_self":
            a.cu_q = aux["cu"]
    if c["order"]:
        a.order = aux["order"]
    if c["ws"]:
        a.ws, a.ws_bytes = aux["ws"], ws_bytes
    return a


def plan(L, a, bwd):
    """pa_attn_plan on an argument block: (status, [kernel names], info)."""
    info = L.AttnPlanInfo()
    rc = L.lib().pa_attn_plan(C.byref(a), int(bwd), C.byref(info))
    return rc, [ln.kernel.decode() for ln in info.launch[:info.n_launches]] if rc == 0 else [], info


def planned_names(L, c, ws_bytes=1 << 26):
    """The kernels pa_attn_plan reports for a case under this process's switches, forward and backward (no GPU needed)."""
    t = Tensors(c, values=False)
    L.lib().pa_attn_split_config(c["x3"])
    try:
        a = attn_args(L, c, t, ws_bytes=ws_bytes)
        return [plan(L, a, bwd)[1] for bwd in (0, 1)]
    finally:
        L.lib().pa_attn_split_config(0)
