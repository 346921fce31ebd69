"""Float64 parity checker for the absorbed decode attention of csrc/decode_mq.h (TEST INFRASTRUCTURE; plain numpy / torch, no GPU).

One case table for tests/test_dec_mq_parity_cpu.py (the checker tested on seeded defects) and tests/test_dec_mq_float64_gpu.py (every
pa_dec_*_mq* entry of include/plank_hip.h held to it, under the default switches and under every switch bundle).  The layout follows
tests/attn_parity.py and tests/rowops_parity.py, whose helpers it uses (gemm_parity.PATTERN / U24 / half_ulp_bf16, rowops_parity.seed_of;
the GPU file takes its guarded buffers - 2^60 around inputs, PATTERN around outputs - from rowops_parity.Guarded).

`dispatch(c, env)` restates the host side - the entry points of csrc/decode.hip (l. 1625-1720), launch_cross_mq / launch_cross_mq32 / mq_units /
mq_parts / mq_split_bytes of csrc/decode_mq.h (l. 751-843) - as a pure function of a case and the process's switches: status, kernel and
template arguments, units, head slots, gdiv, the range blocks in force (1 where the scratch is missing, too small or misaligned, and
always 1 in the four-wave f32 kernel, which has no range blocks), LDS bytes.  A case carries the `branch` it exists for.

Reference: float64 from the stored values (bf16 widened exactly).  For the head slot (row r, head h) of a unit, over the keys s of drawing
r / G that are allowed (s < Lk, kpm = 0):  x_s = sum_j qt_j m_sj (log2 domain: the query carries scale * log2 e),  P = softmax base 2 of x,
ctx_j = sum_s P_s m_sj.  A slot without an allowed key is +0.0 exactly.

tier 1 (derived)   the error scale of tests/attn_parity.py with q = qt, k = v = mem, scale ln 2:
                       A_s = ln2 sum_j |qt_j| |m_sj|     Abar = sum_s P_s A_s     w_s = P_s (1 + A_s + Abar)     S_j = sum_s w_s |m_sj|
                   |got - ref| <= 2 eps S_j per element,   eps = n 2^-9 + (Lk + 512 + 8) 2^-24 (+ (nparts + 2) 2^-24 with range blocks: one
                   rescale per partial in the merge, decode_mq.h l. 228-235 / 606-613), + half a bf16 ulp at max(|ref|, |got|) for a bf16 output,
                   + 2^-126 wherever S > 0 (as tests/rowops_parity.py: below the smallest normal float32 the rounding unit is absolute and a
                   result may be flushed to zero - the address dims of a ramp_up row hold weights of 2^-160).
                   The first-order terms: x_s is an f32 sum of 512 exact products (MFMA, l. 143 / 344 / 514): |dx_s| <= 512 u A_s / ln2, so
                   dP_s / P_s <= ln2 (|dx_s| + sum P |dx|) = 512 u (A_s + Abar); exp2 (v_exp_f32, 1 ulp, l. 168-171) and the subtraction of the
                   reference point add a few u (1 + A_s); the sums over Lk keys (l, O) add Lk u; the division one u.
                   n counts the bf16 roundings between the stored inputs and the output:
                       dec_cross_mq_kernel      n = 1   P is packed to bf16 for the P^T M MFMA (l. 178: pack_bf16, one v_cvt_pk_bf16_f32,
                                                        round to nearest even - csrc/pa_device.h l. 41-48) while the denominator l is summed
                                                        from the f32 p (l. 172): the rounding does not cancel in P / l and counts once.
                                                        The output store (l. 242) is the half ulp above.
                       dec_cross_mq32_kernel    n = 0   f32 throughout (v_mfma_f32_16x16x4_f32)
                       dec_cross_mq32w8_kernel  n = 0
tier 2 (measured)  r(x) = max |x - ref| / (eps S) per case;  r(got) <= FACTOR[kernel] r(emulation): emulate() is plain float32 torch on the
                   CPU in torch's own order (one softmax over all keys, no tiles, no range blocks), P rounded to bf16 before the second
                   product for the bf16 kernel, the bf16 output rounded once.  profiles/dec_mq_float64_parity.txt holds the measurements.
exact              slots without an allowed key (zero keys, fully masked) are +0.0 bit for bit; every launch gives the same bits twice (range
                   blocks merge in range order); every ticket word is zero after every launch; pa_dec_self_mq_ws with f32, nparts 0 gives the
                   bits of pa_dec_self_mq32; a group launch with G = 1, rpb = 1, nparts 0 gives the bits of the _ws entry.
guards             ctx is an interior window of a buffer prefilled with gemm_parity.PATTERN (head slots >= H and the second row of a pair of
                   the LAST unit land behind the window); qt and mem are preceded and followed by 2^60; memory rows that no launch may fetch
                   hold NaN (behind cu[B], behind row t of the self form, NTAIL rows behind the last drawing); rows of masked keys hold 2^20
                   (they are fetched and multiplied by p = 0); the partials area of ws is NaN before each launch, the tickets zero; inputs
                   are compared bit for bit after the launches.

Inputs (one memory per drawing, shared by its G rows; seeded with seed_of(name)).  A memory row is: dims 0 .. 31 the ADDRESS dims (zero
but for one 3.0 per chosen key), dim 32 the RAMP dim 0.15 (s - 136), dims 33 .. 511 N(0, 1): a per-key signature of order 1 in every
output element, against bounds of order 2^-8.  The query of a row decides the regime:
    gauss        0.15 N(0, 1) on dims 33 ..: the data of tests/test_decode_mq_gpu.py (scores of ~3.4 log2 units)
    flat         0.01 N(0, 1): every key weighs ~1 / Lk
    ramp_up      0.075 N(0, 1) and +4 on the ramp dim: 0.6 log2 units per key, the largest score LAST - every tile moves the reference
                 point (the alpha rescale), the first tiles underflow at 272 keys
    ramp_down    -4 on the ramp dim: the first key is the largest
    spot         0.01 N(0, 1) and 4 on the address dim g H + h of its head slot: the slot's chosen key stands 12 log2 units above the rest
                 and carries ~1 - Lk 2^-12 of the weight - a chosen key that is dropped, read from another ring stage or from the
                 neighbouring drawing moves every output element by ~|m|, hundreds of bounds.  The chosen keys walk edges(): 0, 15, 16,
                 Lk - 1, the first and last key of tiles 6, 7, 8 (prologue and wrap of the 8-stage ring), 3, 4 (the 4-stage ring) and of
                 every range block's first and last tile.
    spot_masked  as spot, but the edge key itself is MASKED (its row holds 2^20) and the nearest allowed key is the chosen one.
"""
import numpy as np
import torch

from gemm_parity import PATTERN, U24, half_ulp_bf16             # noqa: F401  (PATTERN: the guard pattern the GPU file looks for)
from rowops_parity import seed_of

PA_F32, PA_BF16 = 0, 1
PA_EINVAL, PA_EALIGN, PA_ESHAPE = -1, -2, -3
PA_SAMPLE_MAX = 64
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
PADT = {"f32": PA_F32, "bf16": PA_BF16}
D, KT, MAXH, SLOTS = 512, 16, 8, 16                                 # decode_mq.h MQ_D, MQ_KT, MQ_MAXH, MQ_SLOTS
MAXS = {"bf16": 16384, "f32": 16000}                                # MQ_MAXS, MAXS32
SP_BYTES = 40 * 1024                                                # MQ_SP_BYTES
RING = {"mq": 8, "mq32": 4, "mq32w8": 4}                            # MQ_NS, MQF_NS
NTAIL = 3                                                           # NaN rows behind the last drawing's memory
MASKED_ROW = 2.0 ** 20
U9 = 2.0 ** -9
TINY = 2.0 ** -126                                                  # below the smallest normal float32 a result may be flushed to zero
LN2 = 0.6931471805599453
KERNELS = ("mq", "mq32", "mq32w8")
N_BF16 = {"mq": 1, "mq32": 0, "mq32w8": 0}
# The tier-2 factor in force per kernel: 16 unless a kernel that passes tier 1 was MEASURED above it on the MI355X (then twice its worst
# measured value, never above 256); profiles/dec_mq_float64_parity.txt.
FACTOR = {"mq": 16.0, "mq32": 16.0, "mq32w8": 16.0}
REGIMES = ("gauss", "flat", "ramp_up", "ramp_down", "spot", "spot_masked")
KEY_COUNTS = (1, 15, 16, 17, 96, 111, 112, 113, 127, 128, 129, 144, 257, 272)

SWITCHES = ("PLANK_DECODE_MQ_SWAP", "PLANK_DECODE_MQ_NT", "PLANK_DECODE_MQ32_W8", "PLANK_DECODE_MQ_MINT", "PLANK_DECODE_MQ_PARTS")
# switch bundles (read once per process: each runs in a child of tests/test_dec_mq_float64_gpu.py, on the cases whose dispatch it changes)
BUNDLES = {
    "swap_0": {"PLANK_DECODE_MQ_SWAP": "0"},
    "nt_0": {"PLANK_DECODE_MQ_NT": "0"},
    "swap_0_nt_0": {"PLANK_DECODE_MQ_SWAP": "0", "PLANK_DECODE_MQ_NT": "0"},
    "w8_0": {"PLANK_DECODE_MQ32_W8": "0"},
    "mint_1": {"PLANK_DECODE_MQ_MINT": "1"},
    "parts_3": {"PLANK_DECODE_MQ_PARTS": "3"},
}


# ------------------------------------------------------------------------------------------------ the restated host dispatch
def mq_parts(B, S, force, mint):                                    # decode_mq.h l. 753
    if force > 0:
        return min(force, 64)
    ntiles = (S + KT - 1) // KT
    p = min(256 // max(B, 1), ntiles // max(mint, 1))
    return max(1, min(p, 64))


def tick_bytes(n):                                                  # mq_tick_bytes
    return (n * 4 + 255) // 256 * 256


def split_bytes(n, nparts):                                         # mq_split_bytes (tick_n 0)
    return tick_bytes(n) + n * nparts * SP_BYTES if nparts > 1 else 0


def split_range(n, part, nparts):                                   # split_merge.h split_range
    per = (n + nparts - 1) // nparts
    lo = min(n, part * per)
    return lo, min(n, lo + per)


def _switches(env):
    env = env or {}
    g = lambda k, d: int(env.get(k, d))
    return dict(parts=g("PLANK_DECODE_MQ_PARTS", 0), mint=g("PLANK_DECODE_MQ_MINT", 8), nt=g("PLANK_DECODE_MQ_NT", 1),
                swap=g("PLANK_DECODE_MQ_SWAP", 1), w8=g("PLANK_DECODE_MQ32_W8", 1))


def _b(x):
    return "true" if x else "false"


def dispatch(c, env=None):
    """What the library does with a case under the switches `env`: dict(status, ...) - see the module docstring.  `requested` is the
    number of range blocks the entry asks launch_cross_mq* for, `nparts` what the launch runs with; `ws_need` the bytes that hold them."""
    sw = _switches(env)
    f32, entry = c["dt"] == "f32", c["entry"]
    B, G, H, S, rpb, d = c["B"], c["G"], c["H"], c["S"], c["rpb"], c.get("d", D)
    null, mis = c.get("null"), c.get("misalign")
    forced = c["nparts"]
    # ---- the entry (decode.hip)
    if entry == "group":
        if null or B <= 0 or G < 1 or G > PA_SAMPLE_MAX or forced < 0 or H < 1:
            return dict(status=PA_EINVAL)
        if mis:
            return dict(status=PA_EALIGN)
        if rpb not in (1, 2) or (rpb == 2 and (G % 2 or 2 * H > SLOTS)):
            return dict(status=PA_EINVAL)
        requested = min(forced, 64) if forced > 0 else mq_parts(B * G // rpb, S, sw["parts"], sw["mint"])
    else:
        if null or (entry == "self_ws" and forced < 0):
            return dict(status=PA_EINVAL)
        if mis and not (mis == "ctx" and not f32 and entry in ("plain", "ws")):      # (the bf16 cross entries do not look at ctx)
            return dict(status=PA_EALIGN)
        requested = {"plain": 1, "self32": 1, "ws": mq_parts(B, S, sw["parts"], sw["mint"]), "self_ws": min(forced, 64) if forced > 0 else 1}[entry]
    # ---- the launch (decode_mq.h)
    if d != D or H < 1 or H > MAXH or B * G <= 0 or S <= 0 or S > MAXS[c["dt"]]:
        return dict(status=PA_ESHAPE)
    units, slots, gdiv = B * G // rpb, H * rpb, G // rpb
    mask = c["form"] == "kpm"
    mbytes = (S + 31) // 16 * 16 if mask else 0
    need = split_bytes(units, requested)
    ws = c["ws"] if (entry in ("ws", "group", "self_ws") and need) else None
    ws_bytes = {None: 0, "ok": need, "small": need - 256, "misaligned": need}[ws]
    nparts, why = requested, "ranges" if requested > 1 else "one_block"
    if requested > 1:
        if f32 and not sw["w8"]:
            nparts, why = 1, "never_splits"
        elif ws is None:
            nparts, why = 1, "fallback_no_ws"
        elif need > ws_bytes:
            nparts, why = 1, "fallback_small"
        elif ws == "misaligned":
            nparts, why = 1, "fallback_misaligned"
    if not f32:
        kern, name, block = "mq", f"dec_cross_mq_kernel<{2 if sw['nt'] else 0}, {_b(sw['swap'])}, {_b(mask)}>", 256
        lds = 8 * KT * D * 2 + mbytes
    elif sw["w8"]:
        kern, name, block, lds = "mq32w8", f"dec_cross_mq32w8_kernel<{_b(mask)}>", 512, 4 * KT * D * 4 + 2 * 8 * 1024 + mbytes
    else:
        kern, name, block, lds = "mq32", f"dec_cross_mq32_kernel<{_b(mask)}>", 256, 4 * KT * D * 4 + 2 * 4 * 1024 + mbytes
    path = {"mask" if mask else "no_mask", why, "pair" if rpb == 2 else ("group" if G > 1 else "single"),
            "full_slots" if slots == SLOTS else "partial_slots", "t_dev" if c["form"] == "self" else ("cu" if c["form"] == "packed" else "dense")}
    return dict(status=0, kern=kern, kernel=name, units=units, slots=slots, gdiv=gdiv, requested=requested, nparts=nparts, lds=lds,
                grid=units * nparts, block=block, ws=ws, ws_need=need, ws_bytes=ws_bytes, path=frozenset(path))


PATH_LABELS = {"mask", "no_mask", "ranges", "one_block", "never_splits", "fallback_no_ws", "fallback_small", "fallback_misaligned", "pair", "group",
               "single", "full_slots", "partial_slots", "t_dev", "cu", "dense"}
INSTANTIATIONS = [f"dec_cross_mq_kernel<{a}, {s}, {m}>" for a in (0, 2) for s in ("false", "true") for m in ("false", "true")] + \
                 [f"dec_cross_mq32_kernel<{m}>" for m in ("false", "true")] + [f"dec_cross_mq32w8_kernel<{m}>" for m in ("false", "true")]


def on_branch(c, env=None):
    """Does dispatch() put the case where it is meant to go?  c["branch"]: a set of path labels plus optional exact fields."""
    p = dispatch(c, env)
    want = c["branch"]
    ok = p["status"] == 0 and want["path"] <= p["path"] and all(p[k] == v for k, v in want.items() if k != "path")
    return ok, p


# ------------------------------------------------------------------------------------------------ the case table
def _case(name, dt, form, *, B=2, S=0, H=8, G=1, rpb=1, lens=None, t=None, mask=None, entry="plain", nparts=0, ws=None, regimes=None, path=(), **want):
    if lens is not None:
        B, S = len(lens), max(lens)
    c = dict(name=f"{name}_{dt}", dt=dt, form=form, B=B, S=S, H=H, G=G, rpb=rpb, lens=lens, t=t, mask=mask, entry=entry, nparts=nparts, ws=ws,
             regimes=list(regimes or REGIMES[:5]))
    c["branch"] = dict(path=set(path), **want)
    return c


def cases():
    """The case table: the smallest shapes that reach every branch (at most 272 keys, 6 drawings).  Every case names its branch; the
    regimes of a case are dealt to its rows in turn (row r: regimes[r % len])."""
    cs = []
    five = REGIMES[:5]
    rot = lambda k: [five[(i + k) % 5] for i in range(5)]
    for dt in ("bf16", "f32"):
        k = 0 if dt == "bf16" else 2
        # ---- every key count, packed (ragged lengths; 0 and 1 next to a long one)
        cs.append(_case("packed_1_15_16_17_96_111", dt, "packed", lens=[1, 15, 16, 17, 96, 111], regimes=rot(k), path={"cu", "no_mask", "one_block", "single"}))
        cs.append(_case("packed_112_113_127_128_129_144", dt, "packed", lens=[112, 113, 127, 128, 129, 144], regimes=rot(k + 1), path={"cu", "one_block"}))
        cs.append(_case("packed_257_0_1_272_0", dt, "packed", lens=[257, 0, 1, 272, 0], regimes=["spot", "gauss", "spot", "ramp_up", "flat"], path={"cu", "one_block"}))
        cs.append(_case("packed_272_spot_144_spot", dt, "packed", lens=[272, 144, 129, 113, 112, 257], regimes=["spot"], H=5, path={"cu", "partial_slots"}))
        # ---- dense, every regime, H from {8, 5, 4, 1}
        for S, H in ((272, 8), (144, 5), (113, 4), (17, 1), (128, 8), (96, 4)):
            cs.append(_case(f"dense_S{S}_H{H}", dt, "dense", B=5, S=S, H=H, regimes=rot(k + S), path={"dense", "no_mask", "one_block"}))
        # ---- dense with kpm: holes, a hole in front of a valid key, a masked last key, a masked edge key under the spot, a drawing without keys
        for S, H in ((272, 8), (129, 5), (16, 8)):
            cs.append(_case(f"kpm_S{S}_H{H}", dt, "kpm", B=4, S=S, H=H, mask="holes", regimes=["spot_masked", "gauss", "flat", "spot"],
                            path={"mask", "dense", "one_block"}))
        cs.append(_case("kpm_S113_tail", dt, "kpm", B=3, S=113, mask="tail", regimes=["ramp_up", "spot_masked", "ramp_down"], path={"mask"}))
        # ---- the self form: key count t + 1 read on the device
        for t, Tmax in ((0, 16), (15, 32), (16, 32), (111, 128), (112, 128), (271, 272)):
            cs.append(_case(f"self_t{t}_Tmax{Tmax}", dt, "self", B=3, S=Tmax, t=t, H=(8, 5, 8, 4, 8, 8)[t % 6], entry="self_ws",
                            regimes=["spot", "ramp_up", "gauss"] if t % 2 else ["ramp_down", "spot", "flat"], path={"t_dev", "one_block"}))
        # ---- range blocks
        for n in (2, 3, 5):
            cs.append(_case(f"ranges_forced{n}_S272", dt, "dense", B=3, S=272, entry="group", nparts=n, ws="ok", regimes=["spot", "ramp_up", "gauss"],
                            path={"ranges"}, nparts_=n))
        cs.append(_case("ranges_forced3_S272_kpm", dt, "kpm", B=3, S=272, mask="holes", entry="group", nparts=3, ws="ok", regimes=["spot_masked", "spot", "ramp_down"],
                        path={"ranges", "mask"}))
        cs.append(_case("ranges_forced4_S40_empty_block", dt, "dense", B=2, S=40, entry="group", nparts=4, ws="ok", regimes=["spot", "ramp_up"], path={"ranges"}))
        cs.append(_case("ranges_forced4_self_t0", dt, "self", B=2, S=64, t=0, entry="self_ws", nparts=4, ws="ok", regimes=["gauss", "spot"], path={"ranges", "t_dev"}))
        cs.append(_case("ranges_forced3_self_t271", dt, "self", B=2, S=272, t=271, entry="self_ws", nparts=3, ws="ok", regimes=["spot", "ramp_up"], path={"ranges", "t_dev"}))
        cs.append(_case("ranges_rule_B2_S272", dt, "dense", B=2, S=272, entry="ws", ws="ok", regimes=["ramp_up", "spot"], path={"ranges"}, nparts_=2))
        cs.append(_case("ranges_rule_packed", dt, "packed", lens=[272, 17, 0], entry="ws", ws="ok", regimes=["spot", "gauss", "flat"], path={"ranges", "cu"}, nparts_=2))
        cs.append(_case("ranges_scratch_too_small", dt, "dense", B=2, S=272, entry="ws", ws="small", regimes=["spot", "gauss"], path={"fallback_small"}, nparts_=1))
        cs.append(_case("ranges_scratch_misaligned", dt, "dense", B=2, S=272, entry="group", nparts=3, ws="misaligned", regimes=["gauss", "spot"],
                        path={"fallback_misaligned"}, nparts_=1))
        cs.append(_case("ranges_no_scratch", dt, "dense", B=2, S=272, entry="group", nparts=2, ws=None, regimes=["spot", "flat"], path={"fallback_no_ws"}, nparts_=1))
        # ---- decode groups: G rows per drawing, one or two of them per block; the two rows of a pair get different regimes
        i = 0
        for H in (8, 5):
            for G, rpb in ((1, 1), (2, 1), (2, 2), (3, 1), (4, 1), (4, 2)):
                form = ("dense", "kpm", "packed")[i % 3]
                n = (0, 2, 3)[(i + (dt == "f32")) % 3]
                kw = dict(lens=[113, 272]) if form == "packed" else dict(B=2, S=(144, 272)[i % 2])
                regs = ["spot", "ramp_up", "gauss", "spot", "flat", "ramp_down", "spot"] if form != "kpm" else ["spot", "spot_masked", "gauss", "ramp_up", "spot"]
                cs.append(_case(f"group_G{G}_rpb{rpb}_H{H}_{form}_n{n}", dt, form, H=H, G=G, rpb=rpb, mask="holes" if form == "kpm" else None, entry="group",
                                nparts=n, ws="ok", regimes=regs, path={"pair" if rpb == 2 else ("group" if G > 1 else "single"), "full_slots" if H * rpb == 16 else "partial_slots"},
                                gdiv=G // rpb, slots=H * rpb, **kw))
                i += 1
    for c in cs:                                                    # (nparts_: the range blocks in force under the default switches)
        if "nparts_" in c["branch"]:
            c["branch"]["nparts"] = c["branch"].pop("nparts_")
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


def rejections():
    """(case, status): launches the host refuses before anything reaches the device; `dispatch` must name the same status."""
    base = dict(dt="bf16", form="dense", B=2, S=32, H=8, G=1, rpb=1, lens=None, t=None, mask=None, entry="plain", nparts=0, ws=None, regimes=["gauss"], branch={})
    rs = []

    def add(name, status, **kw):
        for dt in ("bf16", "f32"):
            c = dict(base, name=f"reject_{name}_{dt}", dt=dt, **kw)
            if c["form"] == "self":
                c["t"] = 3
            rs.append((c, status))
    for entry in ("plain", "ws", "group", "self_ws"):
        form = "self" if entry == "self_ws" else "dense"
        add(f"{entry}_d256", PA_ESHAPE, entry=entry, form=form, d=256)
        add(f"{entry}_H9", PA_ESHAPE, entry=entry, form=form, H=9)
        add(f"{entry}_H0", PA_EINVAL if entry == "group" else PA_ESHAPE, entry=entry, form=form, H=0)
        add(f"{entry}_S0", PA_ESHAPE, entry=entry, form=form, S=0)
        add(f"{entry}_null_qt", PA_EINVAL, entry=entry, form=form, null="qt")
        add(f"{entry}_null_mem", PA_EINVAL, entry=entry, form=form, null="mem")
        add(f"{entry}_null_ctx", PA_EINVAL, entry=entry, form=form, null="ctx")
        add(f"{entry}_qt_off_8_bytes", PA_EALIGN, entry=entry, form=form, misalign="qt")
        add(f"{entry}_mem_off_8_bytes", PA_EALIGN, entry=entry, form=form, misalign="mem")
    add("self32_null_t_dev", PA_EINVAL, entry="self32", form="self", null="t_dev")
    add("self_ws_null_t_dev", PA_EINVAL, entry="self_ws", form="self", null="t_dev")
    add("group_rpb2_G3", PA_EINVAL, entry="group", G=3, rpb=2)
    add("group_rpb3", PA_EINVAL, entry="group", G=3, rpb=3)
    add("group_G0", PA_EINVAL, entry="group", G=0)
    for c, st in [(dict(base, name="reject_S16385_bf16", S=16385), PA_ESHAPE), (dict(base, name="reject_S16001_f32", dt="f32", S=16001), PA_ESHAPE)]:
        rs.append((c, st))
    rs = [(c, st) for c, st in rs if not (c["dt"] == "bf16" and c["entry"] == "self32")]
    assert all(dispatch(c)["status"] == st for c, st in rs), [c["name"] for c, st in rs if dispatch(c)["status"] != st]
    return rs


# ------------------------------------------------------------------------------------------------ geometry, inputs
def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def key_counts(c):
    """Per drawing: (first memory row, keys Lk) as the kernels see them."""
    B, S = c["B"], c["S"]
    if c["form"] == "packed":
        cu = np.concatenate(([0], np.cumsum(c["lens"]))).astype(int)
        return [(int(cu[b]), int(c["lens"][b])) for b in range(B)]
    if c["form"] == "self":
        return [(b * S, c["t"] + 1) for b in range(B)]
    return [(b * S, S) for b in range(B)]


def base_mask(c):
    """kpm uint8 [B, S] of the case's mask kind (the masked edge keys of spot_masked rows are added by Tensors)."""
    B, S = c["B"], c["S"]
    m = np.zeros((B, S), dtype=np.uint8)
    if c["mask"] == "holes":
        for b in range(B):
            m[b, [x for x in (3, 17 + b, 66, 130) if x < S - 1]] = 1
        m[0, S - 1] = 1                                             # a masked last key
        m[1 % B, 0] = 1                                             # a hole in front of a valid key
        if B > 2:
            m[B - 1, :] = 1                                         # a drawing without an allowed key
    elif c["mask"] == "tail":
        for b in range(B):
            m[b, S - 5 - 9 * b:] = 1
    return m


def edges(Lk, nparts=1):
    """The edge keys of a drawing of Lk keys walked by nparts range blocks (module docstring)."""
    e = [0, 15, 16, Lk - 1]
    for t in (6, 7, 8, 3, 4):
        e += [t * KT, t * KT + KT - 1]
    nt = (Lk + KT - 1) // KT
    if nparts > 1:
        for p in range(nparts):
            lo, hi = split_range(nt, p, nparts)
            if lo < hi:
                e += [lo * KT, lo * KT + KT - 1, (hi - 1) * KT, hi * KT - 1]
    out = []
    for k in e:
        k = min(k, Lk - 1)
        if 0 <= k and k not in out:
            out.append(k)
    return out


def _nearest_allowed(allowed, k, taken=()):
    n = len(allowed)
    for dist in range(n):
        for q in (k + dist, k - dist):
            if 0 <= q < n and allowed[q] and q not in taken:
                return q
    return None


class Tensors:
    """The operands of a case on the CPU: qt [R, H, 512] and mem [rows + NTAIL, 512] (float32 holding values of the case's type), kpm, cu,
    allowed[b] (bool per key), chosen[(r, h)] (the spot key of a head slot, whether its row uses it or not)."""

    def __init__(self, c):
        B, G, H, S = c["B"], c["G"], c["H"], c["S"]
        self.c, self.R = c, B * G
        self.el = key_counts(c)
        self.rows = {"packed": sum(c["lens"] or [0]), "self": B * S}.get(c["form"], B * S)
        g = torch.Generator().manual_seed(seed_of(c["name"]))
        rn = lambda *s: torch.randn(*s, generator=g)
        nparts = dispatch(c)["nparts"]
        regime = lambda r: c["regimes"][r % len(c["regimes"])]
        self.regime = [regime(r) for r in range(self.R)]
        kpm = base_mask(c) if c["form"] == "kpm" else None
        mem = torch.full((self.rows + NTAIL, D), float("nan"))
        qt = torch.zeros(self.R, H, D)
        self.chosen, self.allowed = {}, []
        off = seed_of(c["name"]) % 7
        for b, (row0, Lk) in enumerate(self.el):
            m = rn(Lk, D)
            m[:, :32] = 0.0
            m[:, 32] = 0.15 * (torch.arange(Lk, dtype=torch.float32) - 136.0)
            ok = np.ones(Lk, dtype=bool) if kpm is None else (kpm[b, :Lk] == 0)
            ed = edges(Lk, nparts) if Lk else []
            if kpm is not None and ok.any():                        # spot_masked rows: the edge key is masked
                for gi in range(G):
                    if regime(b * G + gi) == "spot_masked":
                        for h in range(H):
                            k = ed[(off + (b * G + gi) * H + h) % len(ed)]
                            if ok.sum() > 1:
                                ok[k] = False
            for gi in range(G):
                for h in range(H):
                    if not ok.any():
                        continue
                    k = _nearest_allowed(ok, ed[(off + (b * G + gi) * H + h) % len(ed)])
                    self.chosen[(b * G + gi, h)] = k
                    m[k, gi * H + h] = 3.0
            m[~torch.from_numpy(ok)] = MASKED_ROW
            if kpm is not None:
                kpm[b, :Lk] = (~ok).astype(np.uint8)
            mem[row0:row0 + Lk] = m
            self.allowed.append(ok)
        for r in range(self.R):
            reg, gi = self.regime[r], r % G
            q = rn(H, D)
            q[:, :33] = 0.0
            if reg == "gauss":
                q *= 0.15
            elif reg in ("ramp_up", "ramp_down"):
                q *= 0.075
                q[:, 32] = 4.0 if reg == "ramp_up" else -4.0
            else:
                q *= 0.01
                if reg in ("spot", "spot_masked"):
                    for h in range(H):
                        q[h, gi * H + h] = 4.0
            qt[r] = q
        if c["dt"] == "bf16":
            qt, mem = _bf(qt), _bf(mem)
        self.qt, self.mem = qt, mem
        self.kpm = torch.from_numpy(kpm) if kpm is not None else None
        self.cu = torch.tensor(np.concatenate(([0], np.cumsum(c["lens"]))), dtype=torch.int32) if c["form"] == "packed" else None

    def keys_of(self, r):
        """(memory rows [Lk, 512] float32, allowed bool [Lk]) of query row r."""
        b = r // self.c["G"]
        row0, Lk = self.el[b]
        return self.mem[row0:row0 + Lk], self.allowed[b]


# ------------------------------------------------------------------------------------------------ float64 reference, float32 emulations
def reference(c, t):
    """ref, S [R, H, 512] (float64), eps [R] and has [R, H] (a slot with an allowed key)."""
    R, H = t.R, c["H"]
    ref, S = np.zeros((R, H, D)), np.zeros((R, H, D))
    eps, has = np.zeros(R), np.zeros((R, H), dtype=bool)
    p = dispatch(c)
    n = N_BF16[p["kern"]]
    for r in range(R):
        m32, ok = t.keys_of(r)
        Lk = len(ok)
        eps[r] = n * U9 + (Lk + D + 8) * U24
        if not ok.any():
            continue
        has[r] = True
        m = m32[torch.from_numpy(ok)].to(torch.float64).numpy()
        q = t.qt[r].to(torch.float64).numpy()
        x = q @ m.T
        x = x - x.max(axis=1, keepdims=True)
        e = np.exp2(x)
        P = e / e.sum(axis=1, keepdims=True)
        ref[r] = P @ m
        A = LN2 * (np.abs(q) @ np.abs(m).T)
        Abar = (P * A).sum(axis=1, keepdims=True)
        S[r] = (P * (1.0 + A + Abar)) @ np.abs(m)
    return dict(ref=ref, S=S, eps=eps, has=has)


def eps_rows(c, ref, nparts):
    """eps per row under `nparts` range blocks in force."""
    return ref["eps"] + ((nparts + 2) * U24 if nparts > 1 else 0.0)


def store(c, x):
    """What a kernel stores of float32 values: themselves, or their round-to-nearest-even bf16 image (as float64)."""
    x = x.to(torch.float32)
    return (_bf(x) if c["dt"] == "bf16" else x).to(torch.float64).numpy()


def emulate(c, t):
    """Plain float32 torch in torch's own order: one softmax over all allowed keys; P rounded to bf16 before the second product for the
    bf16 kernel.  The yardstick of tier 2.  Returns the stored values [R, H, 512] as float64."""
    out = torch.zeros(t.R, c["H"], D)
    bf = c["dt"] == "bf16"
    for r in range(t.R):
        m, ok = t.keys_of(r)
        if not ok.any():
            continue
        m = m[torch.from_numpy(ok)]
        x = t.qt[r] @ m.T
        p = torch.exp2(x - x.max(dim=1, keepdim=True).values)
        l = p.sum(dim=1, keepdim=True)
        out[r] = ((_bf(p) if bf else p) @ m) / l
    return store(c, out)


DEFECTS = ("last_key_dropped", "first_key_of_a_tile_dropped", "tile_from_the_stage_a_ring_back", "tile_processed_twice", "mask_ignored",
           "mask_shifted_by_one_key", "key_bound_le", "range_boundary_tile_dropped", "range_boundary_tile_duplicated", "partial_left_out_of_the_merge",
           "partial_merged_without_rescale", "alpha_rescale_missing", "denominator_from_bf16_p", "unnormalised", "head_slots_swapped", "pair_rows_swapped",
           "drawing_u_for_u_div_gdiv", "cu_off_by_one_row", "self_counts_t_keys", "wave_dims_swapped", "p_rounded_twice")


def emulate_tiled(c, t, defect=None, env=None):
    """The kernels' STRUCTURE in float32 torch - 16-key tiles, the running reference point with its alpha rescale, range blocks merged in
    range order - so that the seeded defects of tests/test_dec_mq_parity_cpu.py have a place to go.  defect None: a second correct
    emulation (it must pass both tiers like emulate())."""
    p_ = dispatch(c, env)
    kern, nparts, bf = p_["kern"], p_["nparts"], c["dt"] == "bf16"
    ring, G, H, B = RING[kern], c["G"], c["H"], c["B"]
    out = torch.zeros(t.R, H, D)
    NEG = float("-inf")
    for r in range(t.R):
        b = r // G
        if defect == "drawing_u_for_u_div_gdiv":
            b = min((r // c["rpb"]), B - 1)
        row0, Lk = t.el[b]
        ok = t.allowed[b].copy()
        if defect == "cu_off_by_one_row":
            row0 += 1
        if defect == "self_counts_t_keys" and c["form"] == "self":
            Lk -= 1
            ok = ok[:Lk]
        if Lk <= 0:
            continue
        if defect == "mask_ignored":
            ok[:] = True
        if defect == "mask_shifted_by_one_key":
            ok = np.concatenate(([True], ok[:-1]))
        if defect == "last_key_dropped":
            ok[Lk - 1] = False
        nt = (Lk + KT - 1) // KT
        fetch = lambda tile: t.mem[row0 + torch.clamp(torch.arange(tile * KT, tile * KT + KT), max=Lk - 1)]      # rows past the end re-read the last row
        valid = np.zeros(nt * KT, dtype=bool)
        valid[:Lk] = ok
        if defect == "key_bound_le" and Lk < nt * KT:
            valid[Lk] = ok[Lk - 1]
        if defect == "first_key_of_a_tile_dropped":
            valid[(nt // 2) * KT] = False
        q = t.qt[r]
        parts = []
        for part in range(nparts):
            t0, t1 = split_range(nt, part, nparts) if nparts > 1 else (0, nt)
            if defect == "range_boundary_tile_dropped" and part > 0 and t0 < t1:
                t0 += 1
            if defect == "range_boundary_tile_duplicated" and part + 1 < nparts and t1 < nt:
                t1 += 1
            m_run, l_run, acc = torch.full((H, 1), NEG), torch.zeros(H, 1), torch.zeros(H, D)
            tiles = list(range(t0, t1))
            if defect == "tile_processed_twice" and tiles:
                tiles.insert(len(tiles) // 2, tiles[len(tiles) // 2])
            for tile in tiles:
                src = tile - ring if (defect == "tile_from_the_stage_a_ring_back" and tile - ring >= t0) else tile
                mt = fetch(src)
                v = torch.from_numpy(valid[tile * KT:(tile + 1) * KT])
                s = torch.where(v[None, :], q @ mt.T, torch.full((), NEG))
                m_new = torch.maximum(m_run, s.max(dim=1, keepdim=True).values)
                m_safe = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
                alpha = torch.exp2(m_run - m_safe)
                p = torch.exp2(s - m_safe)
                pb = _bf(p) if bf else p
                if defect == "p_rounded_twice":
                    pb = _bf(_bf(p) * 1.00390625)                    # (a second multiply-and-round in bf16: 1 + 2^-8, one more rounding)
                l_run = l_run * alpha + (_bf(p) if defect == "denominator_from_bf16_p" else p).sum(dim=1, keepdim=True)
                m_run = m_new
                if defect != "alpha_rescale_missing":
                    acc = acc * alpha
                acc = acc + pb @ mt                                  # (rows of masked keys are finite: p = 0 there)
            parts.append((m_run, l_run, acc))
        if nparts > 1:
            if defect == "partial_left_out_of_the_merge":
                parts = parts[:1] + parts[2:]
            m_all = torch.stack([p[0] for p in parts]).max(dim=0).values
            ms = torch.where(torch.isinf(m_all), torch.zeros_like(m_all), m_all)
            l_run, acc = torch.zeros(H, 1), torch.zeros(H, D)
            for (mp, lp, ap) in parts:
                a1 = torch.exp2(mp - ms)
                if defect == "partial_merged_without_rescale":
                    a1 = torch.where(torch.isinf(mp), a1, torch.ones_like(a1))
                l_run = l_run + lp * a1
                acc = acc + ap * a1
        else:
            m_run, l_run, acc = parts[0]
        inv = torch.where(l_run > 0, 1.0 / torch.where(l_run > 0, l_run, torch.ones_like(l_run)), torch.zeros_like(l_run))
        out[r] = acc if defect == "unnormalised" else acc * inv
    if defect == "head_slots_swapped" and H > 1:
        out[:, [0, 1]] = out[:, [1, 0]]
    if defect == "pair_rows_swapped" and c["rpb"] == 2:
        out = out.reshape(t.R // 2, 2, H, D).flip(1).reshape(t.R, H, D)
    if defect == "wave_dims_swapped":
        w = 64 if kern == "mq32w8" else 128
        out = torch.cat([out[..., w:2 * w], out[..., :w], out[..., 2 * w:]], dim=-1)
    return store(c, out)


def applies(defect, c, env=None):
    """Can the defect change anything at this case?"""
    p = dispatch(c, env)
    if defect in ("mask_ignored", "mask_shifted_by_one_key"):
        return c["form"] == "kpm"
    if defect.startswith("range_") or defect.startswith("partial_"):
        return p["nparts"] > 1
    if defect == "pair_rows_swapped":
        return c["rpb"] == 2
    if defect == "drawing_u_for_u_div_gdiv":
        return p["gdiv"] > 1
    if defect == "cu_off_by_one_row":
        return c["form"] == "packed"
    if defect == "self_counts_t_keys":
        return c["form"] == "self"
    if defect == "head_slots_swapped":
        return c["H"] > 1
    if defect in ("p_rounded_twice", "denominator_from_bf16_p"):
        return c["dt"] == "bf16"
    if defect == "tile_from_the_stage_a_ring_back":
        return max(l for _, l in key_counts(c)) > KT * RING[p["kern"]]
    return True


# ------------------------------------------------------------------------------------------------ the checks
def ratio(x, ref, S, eps):
    """r(x) = max |x - ref| / (eps S) over the elements with S > 0 (a non-finite x: inf).  eps per row."""
    x = np.asarray(x, dtype=np.float64)
    if not np.isfinite(x).all():
        return float("inf")
    ok = S > 0
    e = np.broadcast_to(eps[:, None, None], S.shape)
    return float((np.abs(x - ref)[ok] / (e[ok] * S[ok] + 0.5 * TINY)).max()) if ok.any() else 0.0


def _where(c, t, idx):
    r, h, j = (int(i) for i in idx)
    G, rpb = c["G"], c["rpb"]
    b = r // G
    return (f"(row, head, dim) = ({r}, {h}, {j}): drawing {b} ({t.el[b][1]} keys), unit {r // rpb}, head slot {(r % rpb) * c['H'] + h}, regime {t.regime[r]}, "
            f"spot key {t.chosen.get((r, h))}, dims of wave {j // 128} (bf16 / 4-wave f32) / {j // 64} (8-wave f32)")


def check(c, t, got, ref, *, r_emu=None, env=None):
    """Assert ctx per element: tier 1 (which holds the exact zeros: S = 0 there), +0.0 bit for bit on slots without keys, then tier 2.
    got: [R, H, 512] float64 (the stored values).  Returns r(got)."""
    p = dispatch(c, env)
    got = np.asarray(got, dtype=np.float64)
    R, S = ref["ref"], ref["S"]
    assert got.shape == R.shape, (c["name"], got.shape, R.shape)
    eps = eps_rows(c, ref, p["nparts"])
    tag = f"{c['name']} [{p['kernel']}, {p['nparts']} range block(s)]"
    bound = 2.0 * eps[:, None, None] * S + TINY * (S > 0)
    if c["dt"] == "bf16":
        bound = bound + half_ulp_bf16(np.maximum(np.abs(R), np.abs(np.where(np.isfinite(got), got, 0.0))))
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - R) <= bound)                           # (a NaN is never inside)
    if bad.any():
        err = np.where(np.isfinite(got), np.abs(got - R), np.inf)
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            rel = np.where(bad, err / np.maximum(bound, 1e-300), 0.0)
        idx = np.unravel_index(int(np.argmax(rel)), rel.shape)
        zero = " (an exact zero: a slot without an allowed key)" if S[idx] == 0 else ""
        raise AssertionError(f"{tag}: tier 1: {int(bad.sum())} of {bad.size} elements outside the bound; worst at {_where(c, t, idx)}: got {got[idx]!r}, "
                             f"ref {R[idx]!r}, |got - ref| = {rel[idx]:.3g} x the bound ({bound[idx]:.3g}){zero}")
    keyless = ~ref["has"]
    if keyless.any():
        z = got[keyless]
        assert not (np.signbit(z).any() or (z != 0).any()), f"{tag}: exact: a slot without an allowed key is not +0.0"
    r = ratio(got, R, S, eps)
    if r_emu is not None:
        f = FACTOR[p["kern"]]
        if not r <= f * r_emu:
            ok = S > 0
            rr = np.where(ok, np.abs(got - R) / np.where(ok, eps[:, None, None] * S + 0.5 * TINY, 1.0), 0.0)
            idx = np.unravel_index(int(np.argmax(rr)), rr.shape)
            raise AssertionError(f"{tag}: tier 2: r(got) = {r:.4g} > {f:g} x r(emulation) = {f:g} x {r_emu:.4g}; worst at {_where(c, t, idx)}: "
                                 f"got {got[idx]!r}, ref {R[idx]!r}")
    return r


def judge(c, t, got, ref, emu, env=None):
    """check() with the tier-2 yardstick of the emulation `emu`: (r(got), r(emulation))."""
    r_emu = ratio(emu, ref["ref"], ref["S"], eps_rows(c, ref, dispatch(c, env)["nparts"]))
    return check(c, t, got, ref, r_emu=r_emu, env=env), r_emu


def old_metric_passes(c, got, ref):
    """The metric of tests/test_decode_mq_gpu.py: max |got - ref| over a row's [H, 512] context below 2e-2 (bf16) / 2e-5 (f32) of max |ref|."""
    tol = 2e-2 if c["dt"] == "bf16" else 2e-5
    g = np.asarray(got, dtype=np.float64)
    if not np.isfinite(g).all():
        return False
    return all(np.abs(g[r] - ref["ref"][r]).max() <= tol * max(np.abs(ref["ref"][r]).max(), 1e-3) for r in range(g.shape[0]))
