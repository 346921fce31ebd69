"""Float64 parity checker for pa_gemm (TEST INFRASTRUCTURE; plain numpy / torch, no GPU).

One case table for tests/test_gemm_parity_cpu.py (the checker tested on seeded defects) and tests/test_gemm_float64_gpu.py (every
kernel family and switch bundle of csrc/gemm.hip / gemm8.h held to it).  The checks are per ELEMENT, against a float64 reference
computed from the stored operand values:

  tier 1 (derived)   |got - ref| <= 2 (K + splitk + 4) 2^-24 S,   S = |alpha| (|A| @ |B|) + |bias| + |R|   per element
                     (+ half a bf16 ulp at max(|ref|, |got|) for a bf16 output: 2^-9 ... 2^-8 of it).  (K + n) 2^-24 S is the worst-case bound of an f32 sum of K exact
                     products and n epilogue roundings in any order; the factor 2 covers MFMA accumulation that does not round to nearest.
  tier 2 (measured)  f32 outputs: r(x) = max |x - ref| / ((K + splitk + 4) 2^-24 S);  r(got) <= TIER2_FACTOR[family] * r(float32 torch.matmul
                     on the CPU with the same epilogue in float32).  A different summation order changes the constant, not the growth with K;
                     an intermediate kept in bf16 is 2^15 / sqrt(K) times larger.
  exact decisions    a gated-off or dropped element is exactly 0 (+ R).
  sentinels          C (and out_lp, and the split-K slabs) are interior windows of larger buffers prefilled with a bit pattern that must
                     survive; the padding of A / B / R / aux / bias holds 2^60 (finite: kernels may multiply masked lanes by zero).
"""
import ctypes as C

import numpy as np
import torch

import dropout_masks as dm

PA_F32, PA_BF16 = 0, 1
KINDS = ["PAIR", "RING", "WIDE", "SMALL", "SKINNY", "BIG"]          # PA_GEMM_KIND_* by value (include/plank_hip.h)
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
POISON = 2.0 ** 60                                                  # operand padding
PATTERN = -123.5                                                    # output guard pattern: the same 8 significant bits in f32 and bf16
GUARD_ROWS = 8
U24 = 2.0 ** -24

# The tier-2 factor in force per kernel family (profiles/gemm_float64_parity.txt holds the measurements behind it).  16 unless a
# correct family was MEASURED above it on the hardware: then twice its worst measured value, never above 256.
TIER2_FACTOR = {"PAIR": 16.0, "RING": 16.0, "WIDE": 16.0, "SMALL": 16.0, "SKINNY": 16.0, "BIG": 16.0}

EPILOGUES = {
    "none": {},
    "bias_relu": dict(bias=True, relu=True),
    "alpha_bias_res": dict(alpha=0.5, bias=True, res=True),
    "gate": dict(gate=True, aux_scale=1.25),
    "drop_res": dict(drop_p=0.3, drop_seed=20251, res=True),
    "inplace": dict(res=True, inplace=True),
    "gate_res": dict(gate=True, aux_scale=0.5, bias=True, res=True),
}


def case(name, family, in_dt, M, N, K, akc=1, bkc=1, out_dt="f32", epi="none", splitk=1, batch=1, mis=0, lp=0, member_bias=0,
         group=None, defer=0):
    return dict(name=name, family=family, in_dt=in_dt, out_dt=out_dt, M=M, N=N, K=K, akc=akc, bkc=bkc, epi=epi, splitk=splitk, batch=batch,
                mis=mis, lp=lp, member_bias=member_bias, group=group, defer=defer)


LAYOUTS4 = [(1, 1), (1, 0), (0, 1), (0, 0)]


def _lay(akc, bkc):
    return f"{'n' if akc else 't'}{'n' if bkc else 't'}"


def cases():
    """The case table (default switches, 256 CUs: `family` is what plan_gemm selects; the tests assert it through pa_gemm_plan)."""
    cs = []
    # ---- pair, bf16
    for M, N, K in [(130, 200, 72), (257, 514, 96)]:                # K tail, no direct-to-LDS
        for akc, bkc in LAYOUTS4[:3]:
            cs.append(case(f"pair_bf16_{M}x{N}x{K}_{_lay(akc, bkc)}", "PAIR", "bf16", M, N, K, akc, bkc))
    cs.append(case("pair_bf16_130x200x70_unaligned", "PAIR", "bf16", 130, 200, 70))
    cs.append(case("pair_bf16_130x200x72_A_off_2_bytes", "PAIR", "bf16", 130, 200, 72, mis=1))
    for M, N, K in [(8320, 512, 64), (8300, 520, 64)]:              # > 256 units, ragged last tiles, the transposing loads of CAN_TR
        for akc, bkc in LAYOUTS4:
            cs.append(case(f"pair_bf16_{M}x{N}x{K}_{_lay(akc, bkc)}", "PAIR", "bf16", M, N, K, akc, bkc))
    for epi in ["alpha_bias_res", "gate", "gate_res", "inplace"]:   # bf16 R / gate rows, bf16 output: the epilogue-prefetch variant
        cs.append(case(f"pair_bf16_8300x520x64_epre_{epi}", "PAIR", "bf16", 8300, 520, 64, out_dt="bf16", epi=epi))
    cs.append(case("pair_bf16_8300x520x64_nt_epre_gate", "PAIR", "bf16", 8300, 520, 64, 1, 0, out_dt="bf16", epi="gate"))
    # ---- pair, f32: 16-deep K tile with a tail of 8
    for M, N, K in [(130, 200, 40), (257, 514, 96)]:
        for akc, bkc in LAYOUTS4:
            cs.append(case(f"pair_f32_{M}x{N}x{K}_{_lay(akc, bkc)}", "PAIR", "f32", M, N, K, akc, bkc))
    cs.append(case("pair_f32_130x200x37_unaligned", "PAIR", "f32", 130, 200, 37))
    # ---- ring, bf16
    cs.append(case("ring_130x200x128_nt", "RING", "bf16", 130, 200, 128, 1, 0))
    cs.append(case("ring_130x200x72_tt", "RING", "bf16", 130, 200, 72, 0, 0))           # K tail on the ring
    cs.append(case("ring_130x200x512_sk4", "RING", "bf16", 130, 200, 512, splitk=4))
    cs.append(case("ring_130x200x576_sk4", "RING", "bf16", 130, 200, 576, splitk=4))    # 9 K tiles over 4 slices: 3 non-empty
    cs.append(case("ring_130x200x512_sk4_alpha_bias_res", "RING", "bf16", 130, 200, 512, splitk=4, epi="alpha_bias_res"))
    cs.append(case("ring_130x200x512_sk4_drop_res_bf16out", "RING", "bf16", 130, 200, 512, splitk=4, epi="drop_res", out_dt="bf16"))
    cs.append(case("ring_b3_130x200x128_nt_member_bias", "RING", "bf16", 130, 200, 128, 1, 0, batch=3, epi="bias_relu", member_bias=1))
    cs.append(case("ring_b3_70x96x256_sk4_member_bias", "RING", "bf16", 70, 96, 256, splitk=4, batch=3, epi="alpha_bias_res", member_bias=1))
    cs.append(case("ring_b3_130x200x128_nt_drop_res", "RING", "bf16", 130, 200, 128, 1, 0, batch=3, epi="drop_res"))
    # ---- small, bf16
    cs.append(case("small_130x200x64", "SMALL", "bf16", 130, 200, 64))                  # last row tile of 2 rows, last column tile of 8
    cs.append(case("small_64x64x64", "SMALL", "bf16", 64, 64, 64))
    cs.append(case("small_129x65x448", "SMALL", "bf16", 129, 65, 448))                  # 7 K tiles: more than the ring depth
    cs.append(case("small_b3_130x200x64_member_bias", "SMALL", "bf16", 130, 200, 64, batch=3, epi="bias_relu", member_bias=1))
    # ---- wide, bf16
    cs.append(case("wide_4100x1030x64", "WIDE", "bf16", 4100, 1030, 64))
    # ---- skinny
    for M, N, K in [(37, 200, 512), (250, 514, 512), (512, 96, 1024)]:
        cs.append(case(f"skinny_bf16_{M}x{N}x{K}", "SKINNY", "bf16", M, N, K))
    for M, N, K in [(37, 200, 256), (250, 514, 512)]:
        cs.append(case(f"skinny_f32_{M}x{N}x{K}", "SKINNY", "f32", M, N, K))
    for dt, K in [("bf16", 512), ("f32", 256)]:                     # out_lp: the exact bf16 image of the f32 output
        cs.append(case(f"skinny_{dt}_37x200x{K}_lp", "SKINNY", dt, 37, 200, K, lp=1))
        cs.append(case(f"skinny_{dt}_250x514x512_lp_alpha_bias_res", "SKINNY", dt, 250, 514, 512, lp=1, epi="alpha_bias_res"))
    # ---- every family, every epilogue it accepts, f32 and bf16 output
    six = ["none", "bias_relu", "alpha_bias_res", "gate", "drop_res", "inplace"]
    four = ["none", "bias_relu", "alpha_bias_res", "inplace"]       # the skinny kernel takes no gate and no dropout
    for fam, dt, (M, N, K), (akc, bkc), epis in [
            ("PAIR", "bf16", (130, 200, 72), (1, 1), six), ("PAIR", "f32", (130, 200, 40), (1, 1), six),
            ("RING", "bf16", (130, 200, 128), (1, 0), six), ("SMALL", "bf16", (130, 200, 64), (1, 1), six),
            ("WIDE", "bf16", (4100, 1030, 64), (1, 1), six),
            ("SKINNY", "bf16", (37, 200, 512), (1, 1), four), ("SKINNY", "f32", (37, 200, 256), (1, 1), four)]:
        for epi in epis:
            for out_dt in ("f32", "bf16"):
                if epi == "none" and out_dt == "f32":
                    continue                                        # (in the lists above)
                cs.append(case(f"epi_{fam.lower()}_{dt}_{epi}_{out_dt}out", fam, dt, M, N, K, akc, bkc, out_dt=out_dt, epi=epi))
    # ---- shapes that the switch bundles send elsewhere (default: where plan_gemm puts them)
    cs.append(case("switch_8300x512x64", "PAIR", "bf16", 8300, 512, 64))                # tall under TALL=1
    cs.append(case("switch_4100x264x64", "SMALL", "bf16", 4100, 264, 64))               # BIG=2: 128-wide tiles
    # BIG=2 picks the tile width of the fewest rounds, ties to the narrower: 192 needs 22 ... 32 row tiles at N ~ 1536 (at 4100 rows
    # 128-wide tiles are one round as well and win)
    cs.append(case("switch_5400x1530x64", "PAIR", "bf16", 5400, 1530, 64))              # BIG=2: 192-wide tiles
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


def group_cases():
    """pa_gemm_group (dW = dY^T X): three products of different shapes in one ring launch, one of them split (deferred reduction)."""
    return [case("group_dw_136x72_rows300_sk2", "RING", "bf16", 136, 72, 300, 0, 0, splitk=2, group=0, defer=1),
            case("group_dw_200x130_rows520", "RING", "bf16", 200, 130, 520, 0, 0, group=0),
            case("group_dw_264x96_rows200", "RING", "bf16", 264, 96, 200, 0, 0, group=0)]


def defer_cases():
    """pa_gemm(splitk_defer = 1) + pa_splitk_reduce_many: K = 1000 with 5 requested slices leaves 4 non-empty ones."""
    return [case("defer_130x200x1000_tt_sk5", "RING", "bf16", 130, 200, 1000, 0, 0, splitk=5, defer=1),
            case("defer_64x36x300_tt_sk3", "RING", "bf16", 64, 36, 300, 0, 0, splitk=3, defer=1)]


def rejection_cases():
    """The skinny kernel takes no gate and no dropout: at its shapes such a launch goes to another family (`family` None: any but
    SKINNY), and with an out_lp, which only the skinny kernel writes, it is rejected (PA_EINVAL)."""
    return [case(f"skinny_shape_{dt}_{epi}{'_lp' if lp else ''}", None, dt, 37, 200, K, epi=epi, lp=lp)
            for dt, K in (("bf16", 512), ("f32", 256)) for epi in ("gate", "drop_res") for lp in (0, 1)]


def eff_splitk(c, bk=None):
    """Non-empty contraction slices (csrc/gemm.hip eff_splitk over whole K tiles); the GPU test holds it to pa_gemm_effective_splitk."""
    bk = bk or (64 if c["in_dt"] == "bf16" else 16)
    nt = -(-c["K"] // bk)
    sk = max(1, min(c["splitk"], nt))
    per = -(-nt // sk)
    return -(-nt // per)


# ------------------------------------------------------------------------------------------------ tensors
class Plane:
    """[batch][rows][cols] window of a flat buffer: row stride wider than the row, guard rows above and below every member, optionally
    `lead` elements off the buffer's (16-byte aligned) start.  Everything outside the windows holds `fill`."""

    def __init__(self, batch, rows, cols, dtype, fill, guard, lead=0, extra=8, alloc=True):
        self.batch, self.rows, self.cols, self.dtype, self.fill, self.lead = batch, rows, cols, dtype, fill, lead
        self.ld = (cols + 7) // 8 * 8 + extra
        self.sb = (rows + 2 * guard) * self.ld + (16 if batch > 1 else 0)       # batch stride > rows * ld
        self.off = lead + guard * self.ld
        self.buf = torch.full((lead + batch * self.sb + 16,), fill, dtype=dtype) if alloc else torch.empty(0, dtype=dtype)

    def view(self, buf=None):
        return torch.as_strided(self.buf if buf is None else buf, (self.batch, self.rows, self.cols), (self.sb, self.ld, 1), self.off)

    def set(self, values):
        if self.buf.numel():
            self.view().copy_(values() if callable(values) else values)
        return self

    def outside(self, buf):
        """Bits of every element of `buf` (a copy of the buffer after a launch) outside the windows, and their flat indices."""
        ints = buf.cpu().contiguous().view(torch.int16 if self.dtype == torch.bfloat16 else torch.int32)
        mask = torch.ones(ints.numel(), dtype=torch.bool)
        torch.as_strided(mask, (self.batch, self.rows, self.cols), (self.sb, self.ld, 1), self.off).fill_(False)
        return ints, mask

    def locate(self, flat):
        """(b, row, col) of a flat buffer index, relative to the window (rows / columns outside it are negative or >= the extent)."""
        e = flat - self.off
        b = max(0, min(self.batch - 1, e // self.sb)) if self.batch > 1 else 0
        e -= b * self.sb
        return b, e // self.ld, e % self.ld


def check_sentinels(plane, buf_after, what, name=""):
    """Every element of the buffer outside the windows is bit-identical to the pattern it was prefilled with."""
    ints, mask = plane.outside(buf_after)
    want = torch.full((1,), plane.fill, dtype=plane.dtype).view(ints.dtype)[0]
    bad = mask & (ints != want)
    if bool(bad.any()):
        flat = int(torch.nonzero(bad)[0])
        b, r, c = plane.locate(flat)
        raise AssertionError(f"{name}: {what}: {int(bad.sum())} element(s) outside the {plane.rows} x {plane.cols} window overwritten, first at "
                             f"(b, m, n) = ({b}, {r}, {c}) [row stride {plane.ld}], bits {int(ints[flat]) & 0xFFFFFFFF:#x}")


def _randn(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def make_tensors(c, seed=0, values=True):
    """The operands of a case on the CPU, as Planes.  A / B / bias / R / aux are padded with 2^60, C / out_lp / the slab workspace with
    the guard pattern.  In place (R == C): the C window starts out holding R."""
    ep = EPILOGUES[c["epi"]]
    idt, odt = DT[c["in_dt"]], DT[c["out_dt"]]
    nb, M, N, K = c["batch"], c["M"], c["N"], c["K"]
    s = 1000 * (sum(map(ord, c["name"])) % 997) + seed
    t = {}
    ar, ac = (M, K) if c["akc"] else (K, M)
    br, bc = (N, K) if c["bkc"] else (K, N)
    t["A"] = Plane(nb, ar, ac, idt, POISON, 2, lead=1 if c["mis"] else 0, alloc=values).set(lambda: _randn((nb, ar, ac), idt, s + 1))
    t["B"] = Plane(nb, br, bc, idt, POISON, 2, alloc=values).set(lambda: _randn((nb, br, bc), idt, s + 2))
    t["C"] = Plane(nb, M, N, odt, PATTERN, GUARD_ROWS, alloc=values)
    if ep.get("bias"):
        n_bias = nb if c["member_bias"] else 1
        t["bias"] = Plane(n_bias, 1, N, torch.float32, POISON, 0, alloc=values).set(lambda: _randn((n_bias, 1, N), torch.float32, s + 3))
    if ep.get("res"):
        r = _randn((nb, M, N), odt, s + 4) if values else None
        if ep.get("inplace"):
            t["C"].set(r)
            t["R_values"] = r
        else:
            t["R"] = Plane(nb, M, N, odt, POISON, 2, alloc=values).set(r)
    if ep.get("gate"):
        t["aux"] = Plane(nb, M, N, idt, POISON, 2, alloc=values).set(lambda: _randn((nb, M, N), idt, s + 5))
    if c["lp"]:
        t["lp"] = Plane(1, M, N, torch.bfloat16, PATTERN, GUARD_ROWS, alloc=values)
    sk = eff_splitk(c)
    if sk > 1:
        t["ws"] = Plane(1, 1, sk * nb * M * N, torch.float32, PATTERN, 0, extra=64, lead=64, alloc=values)
    return t


def _f64(x):
    return x.to(torch.float64).numpy()


def operands64(c, t):
    """A [b, M, K], B [b, K, N] widened exactly to float64."""
    a, b = _f64(t["A"].view()), _f64(t["B"].view())
    return (a if c["akc"] else a.transpose(0, 2, 1)), (b.transpose(0, 2, 1) if c["bkc"] else b)


def keep_mask(c):
    ep = EPILOGUES[c["epi"]]
    nb, M, N = c["batch"], c["M"], c["N"]
    if not ep.get("drop_p"):
        return None
    return dm.linear_keep(ep["drop_seed"], np.arange(nb * M), N, ep["drop_p"]).reshape(nb, M, N)      # row = b * M + m


def reference_parts(c, t):
    """Float64 reference in the epilogue order of include/plank_hip.h: *alpha, +bias, relu, gate, dropout, +R.
    ref = act(pre) * mult + add;  `zero`: elements an exact decision (gate / dropout) switches off."""
    ep = EPILOGUES[c["epi"]]
    a, b = operands64(c, t)
    alpha = float(np.float32(ep.get("alpha", 1.0)))
    acc = np.matmul(a, b)
    S = abs(alpha) * np.matmul(np.abs(a), np.abs(b))
    pre = alpha * acc
    if "bias" in t:
        bias = _f64(t["bias"].view())                               # [1 | b, 1, N]
        pre = pre + bias
        S = S + np.abs(bias)
    mult = np.ones_like(pre)
    zero = np.zeros(pre.shape, dtype=bool)
    if "aux" in t:
        on = _f64(t["aux"].view()) > 0
        mult = np.where(on, mult * float(np.float32(ep["aux_scale"])), 0.0)
        zero |= ~on
    keep = keep_mask(c)
    if keep is not None:
        mult = np.where(keep, mult * dm.linear_scale(ep["drop_p"]), 0.0)
        zero |= ~keep
    add = np.zeros_like(pre)
    if ep.get("res"):
        add = _f64(t["R_values"] if ep.get("inplace") else t["R"].view())
        S = S + np.abs(add)
    act = np.maximum(pre, 0.0) if ep.get("relu") else pre
    return dict(ref=act * mult + add, S=S, pre=pre, mult=mult, add=add, zero=zero, relu=bool(ep.get("relu")))


def reference(c, t):
    p = reference_parts(c, t)
    return p["ref"], p["S"]


def blocked_matmul32(a, b, block=32):
    """float32 product accumulated K-block by K-block (the order of a tiled kernel), for the checker's own test."""
    acc = torch.zeros(a.shape[0], a.shape[1], b.shape[2], dtype=torch.float32)
    for k in range(0, a.shape[2], block):
        acc += torch.matmul(a[:, :, k:k + block], b[:, k:k + block, :])
    return acc


def cpu_float32(c, t, matmul=torch.matmul, k_range=None):
    """The reference ARITHMETIC: float32 product on the CPU and the same epilogue in float32 (numpy float32 [b, M, N])."""
    ep = EPILOGUES[c["epi"]]
    a, b = t["A"].view().float(), t["B"].view().float()
    a = a if c["akc"] else a.transpose(1, 2)
    b = b.transpose(1, 2) if c["bkc"] else b
    if k_range is not None:
        a, b = a[:, :, k_range[0]:k_range[1]], b[:, k_range[0]:k_range[1], :]
    v = matmul(a.contiguous(), b.contiguous())
    return epilogue32(c, t, v)


def epilogue32(c, t, v, bias=None, res_first=False):
    """float32 epilogue on a float32 accumulator v [b, M, N] (torch); `bias`, `res_first`: the seeded defects of the checker's test."""
    ep = EPILOGUES[c["epi"]]
    v = v * np.float32(ep.get("alpha", 1.0))
    if "bias" in t:
        v = v + (t["bias"].view() if bias is None else bias)
    if ep.get("relu"):
        v = torch.relu(v)
    if "aux" in t:
        v = torch.where(t["aux"].view().float() > 0, v * np.float32(ep["aux_scale"]), torch.zeros_like(v))
    r = None
    if ep.get("res"):
        r = (t["R_values"] if ep.get("inplace") else t["R"].view()).float()
    if res_first and r is not None:
        v, r = v + r, None
    keep = keep_mask(c)
    if keep is not None:
        v = torch.where(torch.from_numpy(keep), v * np.float32(dm.linear_scale(ep["drop_p"])), torch.zeros_like(v))
    if r is not None:
        v = v + r
    return v.numpy()


def store(c, v32):
    """What a kernel stores of a float32 value: itself, or its round-to-nearest bf16 image (as float64)."""
    v = torch.from_numpy(np.ascontiguousarray(v32))
    return (v.to(torch.bfloat16) if c["out_dt"] == "bf16" else v).to(torch.float64).numpy()


# ------------------------------------------------------------------------------------------------ the checks
def unit_bound(S, K, splitk):
    return (K + splitk + 4) * U24 * S


def ratio(x, ref, S, K, splitk):
    """r(x) = max_ij |x - ref| / ((K + splitk + 4) 2^-24 S)."""
    u = unit_bound(S, K, splitk)
    err = np.abs(np.asarray(x, dtype=np.float64) - ref)
    ok = u > 0
    return float((err[ok] / u[ok]).max()) if ok.any() else 0.0


def half_ulp_bf16(x):
    """Half a unit in the last place of bf16 (8 significant bits) at |x|: what a round-to-nearest bf16 store may add.  Between
    2^-9 |x| (top of a binade) and 2^-8 |x| (bottom of it): a flat 2^-9 |x| fails a correctly rounded store in the lower part of every
    binade - 16.0623 stores as 16.0, 0.0623 = 2^-8.01 x 16 away (tests/test_gemm_parity_cpu.py)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)                                              # x = m 2^e, 0.5 <= m < 1: ulp = 2^(e - 8)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.ldexp(1.0, e - 9), 0.0)


def _where(idx, tile):
    b, m, n = (int(i) for i in idx)
    return f"(b, m, n) = ({b}, {m}, {n}), tile ({m // tile[0]}, {n // tile[1]}) of {tile[0]} x {tile[1]}, row {m % tile[0]} col {n % tile[1]} in it"


def check(got, ref, S, K, splitk, out_dtype, *, name="", family="", tile=(128, 128), parts=None, r_cpu=None, factor=None):
    """Assert per element.  `got`, `ref`, `S`: [b, M, N]; out_dtype "f32" | "bf16".  `parts` (reference_parts): the ReLU interval and the
    exact decisions.  `r_cpu`: r of the float32 CPU product - tier 2, f32 outputs only.  Returns r(got)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == S.shape, (name, got.shape, ref.shape)
    tag = f"{name} [{family}]"
    u = unit_bound(S, K, splitk)
    bound = 2.0 * u
    slack = half_ulp_bf16(np.maximum(np.abs(ref), np.abs(got))) if out_dtype == "bf16" else 0.0
    lo, hi = ref - bound, ref + bound
    if parts is not None and parts["relu"]:
        # an element whose pre-activation is within its bound of zero may land on either side
        lo = np.maximum(parts["pre"] - bound, 0.0) * parts["mult"] + parts["add"]
        hi = np.maximum(parts["pre"] + bound, 0.0) * parts["mult"] + parts["add"]
    with np.errstate(invalid="ignore"):
        bad = ~((got >= lo - slack) & (got <= hi + slack))           # (a NaN is never inside)
    err = np.abs(got - ref)
    if bad.any():
        rel = np.where(bad, err / np.maximum(bound + slack, 1e-300), 0.0)
        rel = np.where(np.isfinite(rel), rel, np.inf)
        idx = np.unravel_index(int(np.argmax(rel)), rel.shape)
        raise AssertionError(f"{tag}: tier 1: {int(bad.sum())} of {bad.size} elements outside the bound; worst at {_where(idx, tile)}: got {got[idx]!r}, "
                             f"ref {ref[idx]!r}, |got - ref| = {rel[idx]:.3g} x the bound ({float((bound + slack)[idx] if np.ndim(slack) else bound[idx]):.3g})")
    if parts is not None and parts["zero"].any():
        z = parts["zero"]
        wrong = z & (got != parts["add"])
        if wrong.any():
            idx = tuple(int(i[0]) for i in np.nonzero(wrong))
            raise AssertionError(f"{tag}: exact decision: {int(wrong.sum())} gated-off / dropped element(s) are not exactly 0 (+ R); first at "
                                 f"{_where(idx, tile)}: got {got[idx]!r}, want {parts['add'][idx]!r} (ratio to the bound {err[idx] / max(bound[idx], 1e-300):.3g})")
    ok = u > 0
    r = float((err[ok] / u[ok]).max()) if ok.any() else 0.0
    if out_dtype == "f32" and r_cpu is not None:
        f = TIER2_FACTOR.get(family, 16.0) if factor is None else factor
        if not r <= f * r_cpu:
            rr = np.where(ok, err / np.where(ok, u, 1.0), 0.0)
            idx = np.unravel_index(int(np.argmax(rr)), rr.shape)
            raise AssertionError(f"{tag}: tier 2: r(got) = {r:.4g} > {f:g} x r_cpu = {f:g} x {r_cpu:.4g}; worst at {_where(idx, tile)}: got {got[idx]!r}, "
                                 f"ref {ref[idx]!r}, |got - ref| = {rr[idx] / 2:.3g} x the tier-1 bound")
    return r


# ------------------------------------------------------------------------------------------------ the argument block
FAKE_BASE = {k: 0x10000000 * (i + 1) for i, k in enumerate(["A", "B", "C", "bias", "R", "aux", "ws", "lp"])}


def fake_ptr(key, plane):
    """Made-up operand address with the real one's alignment (pa_gemm_plan dereferences nothing)."""
    return FAKE_BASE[key] + plane.off * plane.buf.element_size()


def gemm_args(L, c, t, ptr=fake_ptr, splitk=None):
    """The pa_gemm_args block of a case, built directly (as plankassembly_amd.ops.gemm builds it) so that every operand can be a window
    of a guarded buffer.  ptr(key, plane) -> address."""
    ep = EPILOGUES[c["epi"]]
    nb = c["batch"]
    g = L.GemmArgs()
    A, B, Cp = t["A"], t["B"], t["C"]
    g.A, g.B, g.C = ptr("A", A), ptr("B", B), ptr("C", Cp)
    g.M, g.N, g.K = c["M"], c["N"], c["K"]
    g.lda, g.ldb, g.ldc = A.ld, B.ld, Cp.ld
    g.sA, g.sB, g.sC = (A.sb, B.sb, Cp.sb) if nb > 1 else (0, 0, 0)
    g.batch, g.a_kcontig, g.b_kcontig = nb, c["akc"], c["bkc"]
    g.in_dtype = PA_BF16 if c["in_dt"] == "bf16" else PA_F32
    g.out_dtype = PA_BF16 if c["out_dt"] == "bf16" else PA_F32
    g.alpha, g.relu, g.aux_scale = ep.get("alpha", 1.0), int(bool(ep.get("relu"))), ep.get("aux_scale", 1.0)
    g.drop_p, g.drop_seed = ep.get("drop_p", 0.0), ep.get("drop_seed", 0)
    g.ldr = Cp.ld
    if "bias" in t:
        g.bias = ptr("bias", t["bias"])
        g.sBias = t["bias"].sb if (c["member_bias"] and nb > 1) else 0
    if ep.get("res"):
        R = Cp if ep.get("inplace") else t["R"]
        g.R, g.ldr, g.sR = ptr("C" if ep.get("inplace") else "R", R), R.ld, (R.sb if nb > 1 else 0)
    if "aux" in t:
        g.aux, g.ldaux, g.sAux = ptr("aux", t["aux"]), t["aux"].ld, (t["aux"].sb if nb > 1 else 0)
    if "lp" in t:
        g.C_lp, g.ldc_lp = ptr("lp", t["lp"]), t["lp"].ld
    g.splitk = eff_splitk(c) if splitk is None else splitk          # slabs actually written, as ops.gemm asks for them
    if "ws" in t:
        g.ws = ptr("ws", t["ws"])
        g.splitk_defer = c["defer"]
    return g


def plan(L, g):
    """pa_gemm_plan on an argument block: (status, kind name or None, info)."""
    info = L.GemmPlanInfo()
    rc = L.lib().pa_gemm_plan(C.byref(g), None, C.byref(info))
    return rc, (KINDS[info.kind] if rc == 0 else None), info


def plan_rows(L, cs):
    """[[status, kind, grid, block, units, splitk, tile_h, tile_w], ...] of the cases under this process's switches (no GPU needed)."""
    rows = []
    for c in cs:
        rc, kind, info = plan(L, gemm_args(L, c, make_tensors_layout(c)))
        rows.append([rc, kind, info.grid, info.block, info.units, info.splitk, info.tile_h, info.tile_w])
    return rows


def make_tensors_layout(c):
    """Strides / offsets of make_tensors(c) without allocating or filling the operands (the dry run needs no values)."""
    return make_tensors(c, values=False)
