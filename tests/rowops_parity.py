"""Float64 parity checker for the row kernels of csrc/rowops.hip (TEST INFRASTRUCTURE; plain numpy / torch, no GPU).

One case table for tests/test_rowops_parity_cpu.py (the checker tested on seeded defects) and tests/test_rowops_float64_gpu.py (every
entry point of csrc/rowops.hip held to it at every branch of its host dispatch).  `dispatch(c, env)` restates that host dispatch as a
pure function of a case's arguments and the process's switches (rowops.hip has no plan call): NV from d, bwd512 or generic, fused or
four-kernel pack, scan rounds, ordered or atomic segment kernel, ch per table, LDS bytes.  It is the expectation, reviewed against the
host code; a case carries the `branch` it exists for and the tests assert that dispatch() puts it there.

All checks are per ELEMENT against a float64 reference computed from the STORED operand values (bf16 widened exactly; mean / rstd,
row_lse and the loss statistics that a backward reads are inputs: their stored f32 values go into its reference).

  tier 1 (derived)   |got - ref| <= 2 e, with e the first-order propagation of u = 2^-24 per operation and the worst case
                     n u sum|terms| for every f32 sum of n terms, in any order (atomic sums get the same bound as ordered ones); the factor 2
                     covers fused multiply-adds and the library's expf / logf / erff.  A bf16 output adds half a bf16 ulp at max(|ref|, |got|); every
                     bound has 2^-126 added: below the smallest normal float32 the rounding unit is absolute, and a result may be flushed to zero.
      LayerNorm forward, row of d values x:   e_mu = (d + 1) u mean|x|;   t = x - mu: e_t = e_mu + u |t|;
          var = mean t^2: e_var = 2 mean(e_t |t|) + e_mu^2 + (d + 4) u var;   rstd = (var + eps)^-1/2: e_rs = rstd (e_var / (2 (var + eps)) + 3 u);
          y = t rstd gamma + beta: e_y = |gamma| (rstd e_t + |t| e_rs) + 3 u (|t rstd gamma| + |beta|).
      LayerNorm backward (mean, rstd as stored):  xh = (z - mu) rstd: e_xh = 2 u |xh|;  g = dy gamma;  s1 = mean g: e_s1 = (d + 2) u mean|g|;
          s2 = mean g xh: e_s2 = (d + 4) u mean|g xh|;  dz = rstd (g - s1 - xh s2): e_dz = rstd (e_s1 + |xh| e_s2 + e_xh |s2|) + 4 u rstd (|g| + |s1| + |xh s2|);
          ddrop = dz scale: e_dd = scale e_dz + u |ddrop|;  column sums over `rows` rows, added to what the output held:
          dgamma: (rows + 3) u (sum|dy xh| + |init|);  dbeta: (rows + 1) u (sum|dy| + |init|);  dzsum: sum e_dd + (rows + 1) u (sum|ddrop| + |init|).
      finishers: out = init + sum of nparts partials: (nparts + 1) u (|init| + sum|partial|).
      switch head: s = h . w + b: (d + 2) u (sum|h w| + |b|);  dh = ds w (+ dh): 2 u (|ds w| + |dh|);  dw, db: (rows + 2) u (sum|ds h| + |init|).
      GELU: y = x Phi(x) scale: 4 u |x| scale + 3 u |y| (the rounding of 1 + erf is absolute: u, not u Phi);
          dpre = dh (Phi(x) + x phi(x)) scale: u |dh| scale (4 + |x| phi(x) (x^2 + 6)) + 2 u |dpre| (the argument -x^2 / 2 of expf carries x^2 u).
      mixture NLL: lse over n terms of range R: e_lse = u (n + 2 R + 8) + 2 u |lse| (the online form rescales its sum by expf of the maximum's steps, which
          add up to at most R);  prob = 1 / (1 + exp(-s)): e_p = u prob (2 + (1 - prob)(|s| + 1));  log(max(1 - prob, 1e-6)): u |l| when clamped, else
          (e_p + u (1 - prob)) / (1 - prob) + u |l| (the cancellation in 1 - prob is the formula's own);  log p = x - lse + l: e_lse + e_l + 2 u (|x| + |lse| + |l|);
          nll = -sum log p: sum e + (count + 2) u sum|log p| (+ 2^-31 per block for the fixed-point word of the stats8 form);  loss = nll / count: e / count + u |loss|.
          gradients (row_lse, count as stored), g = gscale upstream / count, E = exp(x - lse): u |g| (E (|x - lse| + 4) + 2 |E - hot|);
          dsw: |g| (e_p + u) + 3 u |dsw|.
      Adam, per step (errors carried from step to step):  e_m' = b1 e_m + 4 u (|b1 m| + |(1 - b1) g|);  e_v' = b2 e_v + 4 u v';
          upd = step m' / (sqrt(v') c + eps): e_upd = |upd| (6 u + e_v' / (2 v')) + step e_m' / (sqrt(v') c + eps);  e_p' = e_p + e_upd + u |p'|.
      embeddings: a sum of n rows (added to what the output held): (n + 1) u (|init| + sum|rows|).
  tier 2 (measured)  f32 outputs: r(x) = max |x - ref| / e;  r(got) <= FACTOR[kernel] * r(cpu32) with cpu32 the same operation restated in float32 on
                     the CPU (never the kernel's own output), against the same float64 reference: the GEMM checker's rule.
      order-free sums: a checked scalar that the kernel adds up with float atomics has no order of addition, so ONE float32 restatement is one draw
                     from the values a correct kernel may return, and luck can put it arbitrarily close to the float64 value (r(cpu32) -> 0).  Its
                     yardstick is the worst r of the restatement over the natural order and NLL_ORDERS = 64 permutations, seeded from seed_of(name), of the
                     non-zero block partials, built as the kernel builds them (mixture NLL: four rows per block, (r0 + r1) + (r2 + r3)).  Tier 1 and
                     FACTOR stay as they are.  This holds for pa_mixture_nll_fwd's "nll sum" alone: it is the one checked f32 scalar of csrc/rowops.hip
                     that meets in a float atomicAdd (stats[0]).  count and hits are whole numbers below 2^24, exact in any order; the `fin` form's sum and
                     loss meet in a 64-bit fixed-point word; the switch head's db and the LayerNorm column sums go through per-block partials and an ordered
                     finisher.  The other float atomics of the file (embedding gradients) write tensors that are checked per element over the whole tensor.
  exact              dropped elements are 0; ddrop = dz * scale to one rounding (f32: from the kernel's own dz); dz is the same bits with and without
                     dropout; p_bf16 / pa_cast / the bf16x3 planes are round-to-nearest-even of the f32 value bit for bit; count and hits are whole numbers;
                     pa_pack_rows / pa_group_rows equal torch.sort(stable=True) / bincount / nonzero; the ordered segment kernel repeats its bits.
  hits               within one part (vocabulary or pointers) the arg-max compares STORED logits, exactly, first index on a tie; only the comparison of
                     the two parts' best entries goes through arithmetic.  A row whose two best log-probabilities (one per part) are closer than their
                     tier-1 bounds may count either way; at most 2 % of a case's rows (none at the committed seeds).
  guards             every output is an interior window of a buffer prefilled with the GEMM checker's pattern, every input is preceded and followed
                     by 2^60 (between `cols` and `ld` too); inputs are compared bit for bit after the launch; accumulating outputs start from seeded values.
"""
import ctypes as C
import math

import numpy as np
import torch

import dropout_masks as dm
from gemm_parity import PATTERN, POISON, U24, half_ulp_bf16

PA_F32, PA_BF16 = 0, 1
PA_EINVAL, PA_ESHAPE = -1, -3
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
PADT = {"f32": PA_F32, "bf16": PA_BF16}
GUARD = 64                                                          # elements in front of and behind every window (keeps 16-byte alignment)
TINY = 2.0 ** -126                                                  # below the smallest normal float32 a result may be flushed (expf of -100)
C6 = float(np.float32(1e-6))                                        # the 1e-6f of the pointer fill and of the switch clamps, as the kernels hold it

# The tier-2 factor in force per kernel (profiles/rowops_float64_parity.txt holds the measurements behind it).  16 unless a kernel that
# passes tier 1 was MEASURED above it on the hardware: then twice its worst measured value, never above 256.
KERNELS = ["ln_fwd", "ln_bwd", "ln_finish", "switch_fwd", "switch_bwd", "gelu_fwd", "gelu_bwd", "nll_fwd", "nll_bwd", "adam", "cast",
           "embed_in_fwd", "embed_in_bwd", "embed_out_fwd", "embed_out_bwd", "embed_seg_bwd", "pack_rows", "group_rows"]
FACTOR = {k: 16.0 for k in KERNELS}
# switch_bwd: db of switch_bf16_r270_d4_acc1, one element summed over 270 rows through 34 block partials, measured r(got) = 0.0008788 (tier 1 allows 2)
# against r_cpu = 5.403e-05, torch's float32 sum being within half an ulp of the exact one there: 16.27 x.  Twice that.
FACTOR["switch_bwd"] = 32.53


ENTRY_POINTS = {  # kernel group of a case (c["kernel"]) -> the entry points of include/plank_hip.h its runner calls
    "ln": ["pa_layernorm_fwd_img", "pa_layernorm_bwd_partial_img", "pa_layernorm_finish_many", "pa_layernorm_bwd_can_img", "pa_layernorm_ws_floats"],
    "ln_finish": ["pa_layernorm_finish_many"], "switch": ["pa_switch_fwd", "pa_switch_bwd"], "gelu": ["pa_gelu_fwd", "pa_gelu_bwd"],
    "nll": ["pa_mixture_nll_fwd", "pa_mixture_nll_fwd_fin", "pa_mixture_nll_bwd", "pa_mixture_nll_bwd_up"], "adam": ["pa_adam_step"], "cast": ["pa_cast"],
    "embed_in": ["pa_embed_input_fwd", "pa_embed_input_bwd"], "embed_out": ["pa_embed_output_fwd", "pa_embed_output_bwd"],
    "embed_seg": ["pa_embed_segment_bwd"], "pack_rows": ["pa_pack_rows"], "group_rows": ["pa_group_rows"]}


class LnFinishDesc(C.Structure):                                    # include/plank_hip.h pa_ln_finish_desc
    _fields_ = [("partial", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("dzsum", C.c_void_p), ("nparts", C.c_int32), ("pad_", C.c_int32)]


def seed_of(name, k=0):
    return 1000 * (sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 99991) + k


def randn(shape, seed, dtype=torch.float32, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype)


def f64(x):
    return x.to(torch.float64).numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)


def rne_bf16_bits(x32):
    """int16 bits of the round-to-nearest-even bf16 image of a float32 tensor."""
    return x32.to(torch.bfloat16).view(torch.int16)


# ------------------------------------------------------------------------------------------------ guarded buffers
_FILL_IN = {torch.float32: POISON, torch.bfloat16: POISON, torch.int64: 1 << 60, torch.int32: 0x7F7F7F7F, torch.uint8: 0}
_FILL_OUT = {torch.float32: PATTERN, torch.bfloat16: PATTERN, torch.int32: -123}
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class Guarded:
    """[rows][cols] window (row stride ld >= cols) of a flat buffer, GUARD (+ lead) elements in; everything outside the window - the
    columns cols .. ld - 1 included - holds 2^60 (an input) or the guard pattern (an output)."""

    def __init__(self, values=None, shape=None, dtype=None, out=False, ld=None, lead=0):
        if values is not None:
            values = values.reshape(values.shape[0], -1) if values.dim() > 1 else values.reshape(1, -1)
            shape, dtype = tuple(values.shape), values.dtype
        elif len(shape) == 1:
            shape = (1, shape[0])
        self.rows, self.cols = shape
        self.ld, self.dtype, self.out = ld or self.cols, dtype, out
        self.fill = (_FILL_OUT if out else _FILL_IN)[dtype]
        self.off = GUARD + lead
        self.buf = torch.full((self.off + self.rows * self.ld + GUARD,), self.fill, dtype=dtype)
        if values is not None:
            self.view().copy_(values)

    def view(self, buf=None):
        return torch.as_strided(self.buf if buf is None else buf, (self.rows, self.cols), (self.ld, 1), self.off)

    def byte_offset(self):
        return self.off * self.buf.element_size()

    def check(self, after, name):
        """An input: every bit as before.  An output: every element outside the window still holds the pattern."""
        it = _INT[self.buf.element_size()]
        a, b = after.contiguous().view(it), self.buf.view(it)
        if not self.out:
            assert torch.equal(a, b), f"{name}: the input was written ({int((a != b).sum())} element(s))"
            return
        mask = torch.ones(a.numel(), dtype=torch.bool)
        torch.as_strided(mask, (self.rows, self.cols), (self.ld, 1), self.off).fill_(False)
        bad = mask & (a != b)
        if bool(bad.any()):
            flat = int(torch.nonzero(bad)[0]) - self.off
            raise AssertionError(f"{name}: {int(bad.sum())} element(s) outside the {self.rows} x {self.cols} window overwritten, first at row "
                                 f"{flat // self.ld} col {flat % self.ld} (row stride {self.ld})")


# ------------------------------------------------------------------------------------------------ the checks
def ratio(x, ref, e):
    err = np.abs(np.asarray(x, dtype=np.float64) - ref)
    ok = e > 0
    with np.errstate(invalid="ignore"):
        r = err[ok] / e[ok]
    if r.size and not np.all(np.isfinite(r)):
        return float("inf")
    return float(r.max()) if r.size else (0.0 if np.all(err[~ok] == 0) else float("inf"))


def check(name, what, kernel, got, ref, e, out_dt="f32", cpu=None, zero=None):
    """Assert one output per element: tier 1, the exact zeros of `zero`, tier 2 against the float32 restatement `cpu` (f32 outputs).
    Returns (r(got), r(cpu))."""
    got, ref, e = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(e, dtype=np.float64)
    assert got.shape == ref.shape == e.shape, (name, what, got.shape, ref.shape, e.shape)
    tag = f"{name}: {what} [{kernel}]"
    e = e + 0.5 * TINY                                              # (r(got) is then in units of the bound that is applied)
    slack = half_ulp_bf16(np.maximum(np.abs(ref), np.abs(got))) if out_dt == "bf16" else 0.0
    bound = 2.0 * e + slack
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - ref) <= bound)
        bad &= ~(np.isnan(ref) & np.isnan(got))                     # (0 / 0 of an all-pad batch: NaN on both sides)
    if bad.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(bad, np.abs(got - ref) / np.maximum(bound, 1e-300), 0.0)
        rel = np.where(np.isfinite(rel), rel, np.inf)
        idx = np.unravel_index(int(np.argmax(rel)), rel.shape)
        raise AssertionError(f"{tag}: tier 1: {int(bad.sum())} of {bad.size} elements outside the bound; worst at {tuple(int(i) for i in idx)}: got {got[idx]!r}, "
                             f"ref {ref[idx]!r}, |got - ref| = {rel[idx]:.3g} x the bound ({bound[idx]:.3g})")
    if zero is not None and zero.any():
        wrong = zero & (got != 0.0)
        if wrong.any():
            idx = tuple(int(i[0]) for i in np.nonzero(wrong))
            raise AssertionError(f"{tag}: exact decision: {int(wrong.sum())} dropped / masked element(s) are not exactly 0; first at {idx}: {got[idx]!r}")
    fin = np.isfinite(ref)
    r = ratio(got[fin], ref[fin], e[fin])
    r_cpu = None
    if cpu is not None:
        cpu = np.asarray(cpu, dtype=np.float64)
        r_cpu = ratio(cpu[fin], ref[fin], e[fin])
        if out_dt == "f32" and not r <= FACTOR[kernel] * r_cpu:
            raise AssertionError(f"{tag}: tier 2: r(got) = {r:.4g} > {FACTOR[kernel]:g} x r_cpu = {FACTOR[kernel]:g} x {r_cpu:.4g}")
    return r, r_cpu


class Checked:
    """Collects the checks of one case: check() per output, then the worst r(got) / r(cpu) of the case for the report."""

    def __init__(self, c, kernel=None):
        self.c, self.kernel, self.r, self.r_cpu = c, kernel or c["kernel"], None, None           # (None: no f32 output, so no r)

    def __call__(self, what, got, ref, e, out_dt="f32", cpu=None, zero=None, kernel=None):
        r, rc = check(self.c["name"], what, kernel or self.kernel, got, ref, e, out_dt, cpu, zero)
        if out_dt == "f32":
            self.r, self.r_cpu = max(self.r or 0.0, r), max(self.r_cpu or 0.0, rc or 0.0)

    def exact(self, what, got, want):
        got, want = torch.as_tensor(got), torch.as_tensor(want)
        assert got.shape == want.shape, (self.c["name"], what, got.shape, want.shape)
        if not torch.equal(got, want):
            bad = torch.nonzero((got != want).reshape(-1))
            i = int(bad[0])
            raise AssertionError(f"{self.c['name']}: {what}: {bad.numel()} of {got.numel()} element(s) differ, first at flat index {i}: got "
                                 f"{got.reshape(-1)[i].item()!r}, want {want.reshape(-1)[i].item()!r}")


# ================================================================================================ LayerNorm
LN_D = [4, 8, 252, 256, 260, 512, 516, 1024, 1028, 2048]


def _nv(d):
    return 1 if d <= 256 else 2 if d <= 512 else 4 if d <= 1024 else 8


def ln_cases():
    """Every d meets rows = 1 or 5 and one of 37 or 270; both dtypes, both kinds of rows, both eps; backward with want_dzsum 0 / 1 and
    drop_p 0 / 0.2.  d = 512: the aligned call (bwd512), the bf16 call with dy 8 bytes off (generic), the _img forms."""
    cs = []
    for i, d in enumerate(LN_D):
        for j, rows in enumerate([(1, 5)[i % 2], (37, 270)[(i // 2) % 2], 9] if d in (4, 260, 512, 2048) else [(1, 5)[i % 2], (37, 270)[(i // 2) % 2]]):
            for dt in ("f32", "bf16"):
                k = i + j + (dt == "bf16")
                cs.append(dict(kernel="ln", name=f"ln_{dt}_r{rows}_d{d}", dt=dt, rows=rows, d=d, eps=(1e-5, 1.0)[k % 2], kind=("unit", "offset")[(k // 2) % 2],
                               dzsum=(k + 1) % 2, drop_p=(0.0, 0.2)[(i + j) % 2], mis=0, img=None,
                               branch=dict(nv=_nv(d), bwd="bwd512" if d == 512 else "generic")))
    for d, rows, kind in [(8, 5, "offset"), (2048, 37, "offset"), (4, 270, "unit"), (260, 1, "offset"), (516, 5, "offset"), (1028, 9, "unit")]:
        cs.append(dict(kernel="ln", name=f"ln_f32_r{rows}_d{d}_{kind}_eps1e-5", dt="f32", rows=rows, d=d, eps=1e-5, kind=kind, dzsum=1, drop_p=0.2, mis=0, img=None,
                       branch=dict(nv=_nv(d), bwd="generic")))
    cs.append(dict(kernel="ln", name="ln_bf16_r37_d512_dy_off_8_bytes", dt="bf16", rows=37, d=512, eps=1e-5, kind="unit", dzsum=1, drop_p=0.2, mis=4, img=None,
                   branch=dict(nv=2, bwd="generic")))
    cs.append(dict(kernel="ln", name="ln_f32_r270_d512_switch", dt="f32", rows=270, d=512, eps=1e-5, kind="unit", dzsum=1, drop_p=0.2, mis=0, img=None,
                   branch=dict(nv=2, bwd="bwd512")))                # the PA_LNB_512=0 child sends it to the f32 generic kernel
    for pat in (0, 1):
        cs.append(dict(kernel="ln", name=f"ln_f32_r9_d512_img{pat}", dt="f32", rows=9, d=512, eps=1e-5, kind="unit", dzsum=1, drop_p=(0.0, 0.2)[pat], mis=0,
                       img=pat, branch=dict(nv=2, bwd="bwd512")))
        cs.append(dict(kernel="ln", name=f"ln_f32_r5_d{(260, 1028)[pat]}_img{pat}", dt="f32", rows=5, d=(260, 1028)[pat], eps=1e-5, kind="unit", dzsum=0,
                       drop_p=0.0, mis=0, img=pat, branch=dict(nv=_nv((260, 1028)[pat]), bwd="generic")))
    return cs


def ln_inputs(c):
    s, rows, d, dt = seed_of(c["name"]), c["rows"], c["d"], DT[c["dt"]]
    z = randn((rows, d), s + 1) if c["kind"] == "unit" else randn((rows, d), s + 1, scale=0.01, shift=1000.0)
    if c["kind"] == "offset" and rows >= 5:
        z[rows // 2] = 1000.0                                       # a constant row: rstd = 1 / sqrt(eps)
    return dict(z=z.to(dt), dy=randn((rows, d), s + 2, dt), gamma=randn((d,), s + 3, scale=0.5, shift=1.0), beta=randn((d,), s + 4),
                dgamma0=randn((d,), s + 5), dbeta0=randn((d,), s + 6), dzsum0=randn((d,), s + 7), seed=20251 + s % 1000)


def ln_fwd_ref(c, t):
    z, gamma, beta, d = f64(t["z"]), f64(t["gamma"]), f64(t["beta"]), c["d"]
    eps = float(np.float32(c["eps"]))
    mu = z.mean(1)
    e_mu = (d + 1) * U24 * np.abs(z).mean(1)
    tc = z - mu[:, None]
    e_t = e_mu[:, None] + U24 * np.abs(tc)
    var = (tc * tc).mean(1)
    e_var = 2 * (e_t * np.abs(tc)).mean(1) + e_mu ** 2 + (d + 4) * U24 * var
    rs = 1.0 / np.sqrt(var + eps)
    e_rs = rs * (0.5 * e_var / (var + eps) + 3 * U24)
    y = tc * rs[:, None] * gamma + beta
    e_y = np.abs(gamma) * (rs[:, None] * e_t + np.abs(tc) * e_rs[:, None]) + 3 * U24 * (np.abs(tc * rs[:, None] * gamma) + np.abs(beta))
    return dict(mean=(mu, e_mu), rstd=(rs, e_rs), y=(y, e_y))


def ln_fwd_cpu32(c, t, defect=None):
    z, gamma, beta, d = t["z"].float(), t["gamma"], t["beta"], c["d"]
    eps = np.float32(c["eps"])
    mu = (z[:, :d - 4] if defect == "mean_skips_last_vector" else z).sum(1) / d
    if defect == "one_pass_variance":
        var = (z * z).sum(1) / d - mu * mu
    else:
        tc = z - mu[:, None]
        var = (tc * tc).sum(1) / (d - 1 if defect == "divide_by_d_minus_1" else d)
    rs = 1.0 / torch.sqrt(var + eps)
    y = (z - mu[:, None]) * rs[:, None] * gamma + beta
    return dict(mean=mu.numpy(), rstd=rs.numpy(), y=y.numpy())


def ln_keep(c, t):
    if not c["drop_p"]:
        return None, 1.0
    return dm.linear_keep(t["seed"], np.arange(c["rows"]), c["d"], c["drop_p"]), dm.linear_scale(c["drop_p"])


def ln_bwd_ref(c, t, mean32, rstd32):
    """mean32 / rstd32: the STORED f32 statistics the kernel is handed (torch float32 [rows])."""
    z, dy, gamma, d, rows = f64(t["z"]), f64(t["dy"]), f64(t["gamma"]), c["d"], c["rows"]
    mu, rs = f64(mean32)[:, None], f64(rstd32)[:, None]
    xh = (z - mu) * rs
    g = dy * gamma
    s1, s2 = g.mean(1)[:, None], (g * xh).mean(1)[:, None]
    e_s1, e_s2 = (d + 2) * U24 * np.abs(g).mean(1)[:, None], (d + 4) * U24 * np.abs(g * xh).mean(1)[:, None]
    dz = rs * (g - s1 - xh * s2)
    e_dz = np.abs(rs) * (e_s1 + np.abs(xh) * e_s2 + 2 * U24 * np.abs(xh * s2)) + 4 * U24 * np.abs(rs) * (np.abs(g) + np.abs(s1) + np.abs(xh * s2))
    keep, scale = ln_keep(c, t)
    dd, e_dd = dz, e_dz
    if keep is not None:
        dd = np.where(keep, dz * scale, 0.0)
        e_dd = np.where(keep, scale * e_dz + U24 * np.abs(dd), 0.0)
    dg0, db0, ds0 = f64(t["dgamma0"]), f64(t["dbeta0"]), f64(t["dzsum0"])
    out = dict(dz=(dz, e_dz), ddrop=(dd, e_dd), keep=keep, scale=scale,
               dgamma=(dg0 + (dy * xh).sum(0), (rows + 3) * U24 * (np.abs(dy * xh).sum(0) + np.abs(dg0))),
               dbeta=(db0 + dy.sum(0), (rows + 1) * U24 * (np.abs(dy).sum(0) + np.abs(db0))),
               dzsum=(ds0 + dd.sum(0), e_dd.sum(0) + (rows + 1) * U24 * (np.abs(dd).sum(0) + np.abs(ds0))))
    return out


def ln_bwd_cpu32(c, t, mean32, rstd32, defect=None):
    z, dy, gamma, d, rows = t["z"].float(), t["dy"].float(), t["gamma"], c["d"], c["rows"]
    xh = (z - mean32[:, None]) * rstd32[:, None]
    g = dy * gamma
    s1, s2 = g.sum(1, keepdim=True) / d, (g * xh).sum(1, keepdim=True) / d
    dz = rstd32[:, None] * (g - s1 - (0 if defect == "dz_without_xhat_s2" else xh * s2))
    keep, scale = ln_keep(c, t)
    dd = dz
    if keep is not None:
        kt = torch.from_numpy(keep)
        h = dm.linear_keep(t["seed"], np.arange(d), rows, c["drop_p"]).T if defect == "dropout_hash_row_col_swapped" else None
        kt = torch.from_numpy(np.ascontiguousarray(h)) if h is not None else kt
        dd = torch.where(kt, dz * (1.0 if defect == "dropout_without_scale" else np.float32(scale)), torch.zeros_like(dz))
    last = (rows - 1) // 8 * 8                                      # first row of the last block of 8
    dgp = (dy * xh)[:last].sum(0) if defect == "dgamma_misses_last_block" else (dy * xh).sum(0)
    over = defect == "finisher_overwrites"
    return dict(dz=dz.numpy(), ddrop=dd.numpy(), dgamma=(dgp + (0 if over else t["dgamma0"])).numpy(), dbeta=(dy.sum(0) + (0 if over else t["dbeta0"])).numpy(),
                dzsum=((dz if defect == "dzsum_sums_dz" else dd).sum(0) + (0 if over else t["dzsum0"])).numpy())


def split_planes(o32, pat):
    """The three bf16 planes pa_device.h split_store4 writes for f32 values o32 [rows][d]: hi, then (pat 0) hi, lo or (pat 1) lo, hi; int16 bits
    [rows][3][d].  hi = RNE bf16 of the value, lo = RNE bf16 of the f32 remainder."""
    hi = o32.to(torch.bfloat16)
    lo = (o32 - hi.float()).to(torch.bfloat16)
    planes = [hi, lo, hi] if pat else [hi, hi, lo]
    return torch.stack(planes, 1).view(torch.int16)


FINISH_CASE = dict(kernel="ln_finish", name="ln_finish_many_d260_parts_1_34_40", d=260, nparts=[1, 34, 40], null_dzsum=1,
                   branch=dict(full_unroll=[False, True, True], nq=3))


def finish_inputs(c):
    s, d = seed_of(c["name"]), c["d"]
    return dict(partial=[randn((n, 3 * d), s + i) for i, n in enumerate(c["nparts"])],
                init=[[randn((d,), s + 10 * i + q + 100) for q in range(3)] for i in range(len(c["nparts"]))])


def finish_ref(c, t):
    out = []
    for i, n in enumerate(c["nparts"]):
        p = f64(t["partial"][i]).reshape(n, 3, c["d"])
        row = []
        for q in range(3):
            i0 = f64(t["init"][i][q])
            if q == 2 and i == c["null_dzsum"]:
                row.append(None)
                continue
            row.append((i0 + p[:, q].sum(0), (n + 1) * U24 * (np.abs(i0) + np.abs(p[:, q]).sum(0))))
        out.append(row)
    return out


def finish_cpu32(c, t, defect=None):
    return [[(t["partial"][i].reshape(n, 3, c["d"])[:, q].sum(0) + (0 if defect == "finisher_overwrites" else t["init"][i][q])).numpy() for q in range(3)]
            for i, n in enumerate(c["nparts"])]


# ================================================================================================ switch head
def switch_cases():
    cs = []
    for i, (rows, d) in enumerate([(1, 4), (9, 260), (270, 512), (9, 2048), (270, 4), (1, 2048), (9, 512), (270, 260)]):
        for dt in ("f32", "bf16"):
            cs.append(dict(kernel="switch", name=f"switch_{dt}_r{rows}_d{d}_acc{(i + (dt == 'bf16')) % 2}", dt=dt, rows=rows, d=d, acc=(i + (dt == "bf16")) % 2,
                           branch=dict(nparts=-(-rows // 8))))
    return cs


def switch_inputs(c):
    s, rows, d, dt = seed_of(c["name"]), c["rows"], c["d"], DT[c["dt"]]
    return dict(h=randn((rows, d), s + 1, dt), w=randn((d,), s + 2), b=randn((1,), s + 3), ds=randn((rows,), s + 4), dh0=randn((rows, d), s + 5, dt),
                dw0=randn((d,), s + 6), db0=randn((1,), s + 7))


def switch_ref(c, t):
    h, w, b, ds, rows, d = f64(t["h"]), f64(t["w"]), f64(t["b"]), f64(t["ds"]), c["rows"], c["d"]
    dh0 = f64(t["dh0"]) if c["acc"] else np.zeros_like(h)
    dw0, db0 = f64(t["dw0"]), f64(t["db0"])
    return dict(s=(h @ w + b, (d + 2) * U24 * (np.abs(h) @ np.abs(w) + np.abs(b))),
                dh=(ds[:, None] * w + dh0, 2 * U24 * (np.abs(ds[:, None] * w) + np.abs(dh0))),
                dw=(dw0 + ds @ h, (rows + 2) * U24 * (np.abs(ds) @ np.abs(h) + np.abs(dw0))),
                db=(db0 + ds.sum(), (rows + 2) * U24 * (np.abs(ds).sum() + np.abs(db0))))


def switch_cpu32(c, t, defect=None):
    h, w, b, ds = t["h"].float(), t["w"], t["b"], t["ds"]
    dh0 = t["dh0"].float() if c["acc"] and defect != "accumulate_ignored" else 0
    over = defect == "finisher_overwrites"
    return dict(s=(h @ w + b).numpy(), dh=(ds[:, None] * w + dh0).numpy(), dw=((0 if over else t["dw0"]) + ds @ h).numpy(),
                db=((0 if over else t["db0"]) + ds.sum()).numpy())


# ================================================================================================ GELU
def gelu_cases():
    cs = []
    for rows, cols, ld, grid, loop in [(7, 12, 20, 1, False), (33, 128, 128, 5, False), (5, 2048, 2052, 10, False), (2050, 2048, 2048, 4096, True)]:
        for dt in ("f32", "bf16"):
            for p in (0.0, 0.3):
                cs.append(dict(kernel="gelu", name=f"gelu_{dt}_{rows}x{cols}_ld{ld}_p{p}", dt=dt, rows=rows, cols=cols, ld=ld, drop_p=p,
                               branch=dict(grid=grid, stride_loop=loop)))
    return cs


def gelu_inputs(c):
    s, rows, cols, dt = seed_of(c["name"]), c["rows"], c["cols"], DT[c["dt"]]
    g = torch.Generator().manual_seed(s)
    x = torch.rand(rows, cols, generator=g) * 20 - 10
    x.view(-1)[::7] = 0.0
    x.view(-1)[3::11] = -0.0
    x.view(-1)[5::13] *= 0.05                                       # and the region around zero, where phi is large
    return dict(x=x.to(dt), dh=randn((rows, cols), s + 1, dt), seed=777 + s % 1000)


def gelu_keep(c, t):
    if not c["drop_p"]:
        return None, 1.0
    return dm.linear_keep(t["seed"], np.arange(c["rows"]), c["cols"], c["drop_p"]), dm.linear_scale(c["drop_p"])


def gelu_ref(c, t):
    x, dh = f64(t["x"]), f64(t["dh"])
    Phi = 0.5 * (1 + torch.erf(torch.from_numpy(x) / math.sqrt(2.0)).numpy())
    phi = np.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    keep, scale = gelu_keep(c, t)
    k = scale if keep is None else np.where(keep, scale, 0.0)
    y, dp = x * Phi * k, dh * (Phi + x * phi) * k
    e_y = 4 * U24 * np.abs(x) * k + 3 * U24 * np.abs(y)
    e_dp = U24 * np.abs(dh) * k * (4 + np.abs(x) * phi * (x * x + 6)) + 2 * U24 * np.abs(dp)
    return dict(y=(y, e_y), dpre=(dp, e_dp), zero=None if keep is None else ~keep)


def gelu_cpu32(c, t, defect=None):
    x, dh = t["x"].float(), t["dh"].float()
    if defect == "tanh_approximation":
        Phi = 0.5 * (1 + torch.tanh(np.float32(math.sqrt(2 / math.pi)) * (x + np.float32(0.044715) * x ** 3)))
    else:
        Phi = 0.5 * (1 + torch.erf(x * np.float32(math.sqrt(0.5))))
    phi = torch.exp(-0.5 * x * x) * np.float32(1 / math.sqrt(2 * math.pi))
    keep, scale = gelu_keep(c, t)
    k = np.float32(1.0)
    if keep is not None:
        if defect == "dropout_hash_row_col_swapped":
            keep = np.ascontiguousarray(dm.linear_keep(t["seed"], np.arange(c["cols"]), c["rows"], c["drop_p"]).T)
        k = torch.from_numpy(keep).float() * np.float32(1.0 if defect == "dropout_without_scale" else scale)
    return dict(y=(x * Phi * k).numpy(), dpre=(dh * (Phi + (0 if defect == "gradient_without_x_phi" else x * phi)) * k).numpy())


# ================================================================================================ mixture NLL
SWITCH_LOGITS = [0.0, 5.0, -5.0, 12.0, -12.0, 16.0, -16.0, 30.0, -30.0]     # all at least 1 from the clamp threshold ln(10^6 - 1) = 13.8155
NLL_SHAPES = [(1, 5, 3, 3, "fast"), (2, 36, 514, 514, "fast"), (2, 36, 514, 520, "fast"), (3, 256, 1024, 1024, "fast"), (2, 257, 514, 514, "strided"),
              (1, 7, 1030, 1032, "strided")]


def nll_cases():
    cs = []
    for B, T, V, ldv, path in NLL_SHAPES:
        for scale in (1, 30):
            cs.append(dict(kernel="nll", name=f"nll_B{B}_T{T}_V{V}_ld{ldv}_x{scale}", B=B, T=T, V=V, ldv=ldv, scale=scale, allpad=0, branch=dict(path=path)))
    cs.append(dict(kernel="nll", name="nll_B2_T36_V514_ld520_allpad", B=2, T=36, V=514, ldv=520, scale=1, allpad=1, branch=dict(path="fast")))
    return cs


def nll_inputs(c):
    s, B, T, V = seed_of(c["name"]), c["B"], c["T"], c["V"]
    n = B * T
    pad = V + T                                                     # the pad label: outside 0 .. V + T - 1
    g = torch.Generator().manual_seed(s)
    vocab, ptr = randn((n, V), s + 1, scale=c["scale"]), randn((n, T), s + 2, scale=c["scale"])
    # (at scale 30 each part's best entry has nearly all of its part's mass: a switch logit of 0 would make the two parts' best entries tie)
    lo = 1 if c["scale"] > 1 else 0
    sw = torch.tensor(SWITCH_LOGITS)[torch.randint(lo, len(SWITCH_LOGITS), (n,), generator=g)]
    i = torch.arange(n) % T
    kind = torch.randint(0, 10, (n,), generator=g)                  # 0..4 vocabulary, 5..7 pointer j < i, 8 pointer j >= i, 9 pad
    lab = torch.randint(0, V, (n,), generator=g)
    below = V + (torch.rand(n, generator=g) * i).long().clamp(max=T - 1)
    above = V + i + (torch.rand(n, generator=g) * (T - i)).long().clamp(max=T - 1 - i)
    lab = torch.where((kind >= 5) & (kind <= 7) & (i > 0), below, lab)
    lab = torch.where(kind == 8, above, lab)
    lab = torch.where(kind == 9, torch.full_like(lab, pad), lab)
    lab[0] = V                                                      # row i = 0 with a pointer label (j = 0 >= i)
    if T >= 5:
        lab[2], lab[3] = V + 1, V + 3                               # a pointer label with j < i and one with j >= i in every case
    if T > 1:
        r = 1                                                       # an exact tie of the best vocabulary logits (first, last, and one 64 further on
        vocab[r, 0] = vocab[r].max() + 2.0                          # in the first one's lane): the first index wins
        vocab[r, V - 1] = vocab[r, 0]
        if V > 64:
            vocab[r, 64] = vocab[r, 0]
        lab[r], sw[r] = 0, -5.0
    if B == 1:
        lab[n - 1] = pad
    if B > 1:
        lab[(B - 1) * T:] = pad                                     # one batch element all pad
    if c["allpad"]:
        lab[:] = pad
    return dict(vocab=vocab, ptr=ptr, sw=sw, label=lab, pad=pad, up=torch.tensor([0.75]))


def nll_rows(c, t):
    """Per-row float64 quantities of the loss formula (tests/test_kernels_gpu.py test_mixture_nll_vs_oracle spells it out)."""
    B, T, V = c["B"], c["T"], c["V"]
    x, p, s, lab = f64(t["vocab"]), f64(t["ptr"]).copy(), f64(t["sw"]), t["label"].numpy()
    n = B * T
    i = np.arange(n) % T
    masked = np.arange(T)[None, :] >= i[:, None]
    p[masked] = C6

    def lse(a):
        m = a.max(1)
        l = m + np.log(np.exp(a - m[:, None]).sum(1))
        return l, U24 * (a.shape[1] + 2 * (m - a.min(1)) + 8) + 2 * U24 * np.abs(l)
    lse_v, e_lv = lse(x)
    lse_p, e_lp = lse(p)
    prob = 1.0 / (1.0 + np.exp(-s))
    e_prob = U24 * prob * (2 + (1 - prob) * (np.abs(s) + 1))
    q = 1 - prob
    lv, lp = np.log(np.maximum(q, C6)), np.log(np.maximum(prob, C6))
    e_swv = np.where(q < C6, 0.0, (e_prob + U24 * q) / np.maximum(q, C6)) + U24 * np.abs(lv)
    e_swp = np.where(prob < C6, 0.0, e_prob / np.maximum(prob, C6)) + U24 * np.abs(lp)
    valid = lab != t["pad"]
    is_v = valid & (lab < V)
    is_p = valid & (lab >= V)
    r = np.arange(n)
    xl = np.where(is_v, x[r, np.clip(lab, 0, V - 1)], p[r, np.clip(lab - V, 0, T - 1)])
    logp = np.where(is_v, xl - lse_v + lv, xl - lse_p + lp)
    e_logp = np.where(is_v, e_lv + e_swv + 2 * U24 * (np.abs(xl) + np.abs(lse_v) + np.abs(lv)), e_lp + e_swp + 2 * U24 * (np.abs(xl) + np.abs(lse_p) + np.abs(lp)))
    av, ap = x.argmax(1), p.argmax(1)                               # first index on a tie (the comparison of stored values is exact)
    best_v, best_p = x[r, av] - lse_v + lv, p[r, ap] - lse_p + lp
    e_bv = e_lv + e_swv + 2 * U24 * (np.abs(x[r, av]) + np.abs(lse_v) + np.abs(lv))
    e_bp = e_lp + e_swp + 2 * U24 * (np.abs(p[r, ap]) + np.abs(lse_p) + np.abs(lp))
    pred = np.where(best_p > best_v, V + ap, av)
    sure = np.abs(best_p - best_v) > 2 * (e_bv + e_bp)
    return dict(x=x, p=p, masked=masked, i=i, s=s, lab=lab, valid=valid, is_v=is_v, is_p=is_p, lse_v=lse_v, lse_p=lse_p, e_lse_v=e_lv, e_lse_p=e_lp, prob=prob,
                e_prob=e_prob, logp=np.where(valid, logp, 0.0), e_logp=np.where(valid, e_logp, 0.0), pred=pred, sure=sure, hit=valid & (pred == lab))


def nll_fwd_ref(c, t, fixed=False):
    R = nll_rows(c, t)
    cnt = int(R["valid"].sum())
    nll = -R["logp"].sum()
    blocks = -(-(c["B"] * c["T"]) // 4)
    e_nll = R["e_logp"].sum() + (cnt + 2) * U24 * np.abs(R["logp"]).sum() + (blocks * 2.0 ** -31 if fixed else 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float64(nll) / np.float64(cnt)
        e_loss = (e_nll / cnt + U24 * abs(loss)) if cnt else 0.0
    hits_sure = int((R["hit"] & R["sure"]).sum())
    unsure = int((R["valid"] & ~R["sure"]).sum())
    return dict(R=R, nll=(nll, e_nll), count=cnt, hits=(hits_sure, hits_sure + unsure), unsure=unsure, loss=(loss, e_loss),
                lse=(np.stack([R["lse_v"], R["lse_p"]], 1), np.stack([R["e_lse_v"], R["e_lse_p"]], 1)))


def nll_fwd_cpu32(c, t, defect=None):
    B, T, V = c["B"], c["T"], c["V"]
    x, p, s, lab = t["vocab"], t["ptr"].clone(), t["sw"], t["label"]
    n = B * T
    i = torch.arange(n) % T
    j = torch.arange(T)[None, :]
    p[(j > i[:, None]) if defect == "pointer_mask_j_gt_i" else (j >= i[:, None])] = C6

    def lse(a):
        if defect == "lse_without_max":
            return torch.log(torch.exp(a).sum(1))
        m = a.max(1).values
        return m + torch.log(torch.exp(a - m[:, None]).sum(1))
    lse_v, lse_p = lse(x), lse(p)
    prob = 1.0 / (1.0 + torch.exp(-s))
    lv, lp = torch.log(torch.clamp(1 - prob, min=C6)), torch.log(torch.clamp(prob, min=C6))
    valid = lab != t["pad"]
    is_v = valid & (lab < V)
    r = torch.arange(n)
    logp = torch.where(is_v, x[r, lab.clamp(0, V - 1)] - lse_v + lv, p[r, (lab - V).clamp(0, T - 1)] - lse_p + lp)
    logp = torch.where(valid, logp, torch.zeros_like(logp))
    if defect == "argmax_larger_index_on_tie":
        av, ap = V - 1 - x.flip(1).argmax(1), T - 1 - p.flip(1).argmax(1)
    else:
        av, ap = x.argmax(1), p.argmax(1)
    pred = torch.where(p[r, ap] - lse_p + lp > x[r, av] - lse_v + lv, V + ap, av)
    cnt = int(valid.sum())
    nll = -logp.sum()
    return dict(nll=float(nll), count=cnt, hits=int((valid & (pred == lab)).sum()), loss=float(nll / cnt) if cnt else float("nan"),
                lse=torch.stack([lse_v, lse_p], 1).numpy(), row_nll=(-logp).numpy())


NLL_ORDERS = 64                                                     # seeded arrival orders behind the tier-2 yardstick of the `fwd` form's sum


def nll_block_partials(row_nll):
    """The non-zero float32 block partials of pa_mixture_nll_fwd's sum as mixture_nll_fwd_kernel forms them: NLL_ROWS = 4 rows per block, one per
    wave (a pad row and a row behind the last one add 0), (r0 + r1) + (r2 + r3); a block whose partial is 0 sends no atomic."""
    r = np.asarray(row_nll, dtype=np.float32)
    r = np.concatenate([r, np.zeros(-len(r) % 4, dtype=np.float32)]).reshape(-1, 4)
    part = (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])
    return part[part != 0]


def nll_order_sums(row_nll, seed, orders):
    """float32 [1 + orders]: the block partials added one by one in float32 from 0, as float atomics into the zeroed stats[0] do - in the natural
    order first, then in `orders` permutations seeded by `seed`.  Every entry is a value a correct kernel may return."""
    part = nll_block_partials(row_nll)
    rng = np.random.default_rng(seed)
    perm = np.stack([np.arange(len(part))] + [rng.permutation(len(part)) for _ in range(orders)])
    if not len(part):
        return np.zeros(1 + orders, dtype=np.float32)
    return np.add.accumulate(part[perm], axis=1, dtype=np.float32)[:, -1]            # (accumulate adds in sequence, not pairwise)


def nll_sum_yardstick(c, cpu, ref_nll):
    """The tier-2 yardstick of the `fwd` form's "nll sum": of the natural order and NLL_ORDERS seeded permutations of the restated block
    partials, the float32 sum furthest from the float64 value (see the module docstring, tier 2, order-free sums)."""
    sums = nll_order_sums(cpu["row_nll"], seed_of(c["name"]), NLL_ORDERS).astype(np.float64)
    return sums[int(np.argmax(np.abs(sums - ref_nll)))]


def nll_bwd_ref(c, t, row_lse32, count32, up32, gscale):
    """Gradients from the STORED row_lse [n][2], count and upstream value (float32 as the kernel reads them)."""
    R = nll_rows(c, t)
    V, T = c["V"], c["T"]
    n = c["B"] * T
    lse_v, lse_p = f64(row_lse32)[:, 0], f64(row_lse32)[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = float(np.float64(np.float32(gscale)) * np.float64(up32) / np.float64(count32))
    r = np.arange(n)
    hot_v = np.zeros((n, V)); hot_v[r[R["is_v"]], R["lab"][R["is_v"]]] = 1.0
    hot_p = np.zeros((n, T)); hot_p[r[R["is_p"]], R["lab"][R["is_p"]] - V] = 1.0
    hot_p[R["masked"]] = 0.0
    if not R["valid"].any():
        z = np.zeros
        return dict(dv=(z((n, V)), z((n, V))), dp=(z((n, T)), z((n, T))), dsw=(z(n), z(n)), zero_v=np.ones((n, V), bool), zero_p=np.ones((n, T), bool))
    with np.errstate(over="ignore"):
        Ev = np.exp(R["x"] - lse_v[:, None])
        Ep = np.where(R["masked"], 0.0, np.exp(np.where(R["masked"], 0.0, f64(t["ptr"])) - lse_p[:, None]))
    dv = np.where(R["is_v"][:, None], g * (Ev - hot_v), 0.0)
    dp = np.where(R["is_p"][:, None] & ~R["masked"], g * (Ep - hot_p), 0.0)
    e_dv = np.where(R["is_v"][:, None], U24 * abs(g) * (Ev * (np.abs(R["x"] - lse_v[:, None]) + 4) + 2 * np.abs(Ev - hot_v)), 0.0)
    e_dp = np.where(R["is_p"][:, None] & ~R["masked"], U24 * abs(g) * (Ep * (np.abs(np.where(R["masked"], 0.0, f64(t["ptr"])) - lse_p[:, None]) + 4) + 2 * np.abs(Ep - hot_p)), 0.0)
    prob, q = R["prob"], 1 - R["prob"]
    dsw = np.where(R["is_v"], np.where(q >= C6, g * prob, 0.0), np.where(R["is_p"], np.where(prob >= C6, -g * q, 0.0), 0.0))
    e_dsw = np.where(R["valid"], abs(g) * (R["e_prob"] + U24) + 3 * U24 * np.abs(dsw), 0.0)
    return dict(dv=(dv, e_dv), dp=(dp, e_dp), dsw=(dsw, e_dsw), zero_v=~R["is_v"][:, None] & np.ones((1, V), bool), zero_p=~(R["is_p"][:, None] & ~R["masked"]))


def nll_bwd_cpu32(c, t, row_lse32, count32, up32, gscale, defect=None):
    V, T = c["V"], c["T"]
    n = c["B"] * T
    x, p, s, lab = t["vocab"], t["ptr"], t["sw"], t["label"]
    i = torch.arange(n) % T
    masked = torch.arange(T)[None, :] >= i[:, None]
    valid = lab != t["pad"]
    is_v, is_p = valid & (lab < V), valid & (lab >= V)
    g = np.float32(1.0 if defect == "gscale_left_out" else gscale) * np.float32(up32) / np.float32(count32) if float(count32) else np.float32(0)
    r = torch.arange(n)
    hot_v = torch.zeros(n, V); hot_v[r[is_v], lab[is_v]] = 1.0
    hot_p = torch.zeros(n, T); hot_p[r[is_p], lab[is_p] - V] = 1.0
    hot_p[masked] = 0.0
    dv = torch.where(is_v[:, None], g * (torch.exp(x - row_lse32[:, :1]) - hot_v), torch.zeros(1))
    dp = torch.where(is_p[:, None] & ~masked, g * (torch.exp(p - row_lse32[:, 1:]) - hot_p), torch.zeros(1))
    prob = 1.0 / (1.0 + torch.exp(-s))
    on_v = torch.ones_like(valid) if defect == "switch_clamp_ignored" else (1 - prob >= C6)
    on_p = torch.ones_like(valid) if defect == "switch_clamp_ignored" else (prob >= C6)
    dsw = torch.where(is_v, torch.where(on_v, g * prob, torch.zeros(1)), torch.where(is_p, torch.where(on_p, -g * (1 - prob), torch.zeros(1)), torch.zeros(1)))
    return dict(dv=dv.numpy(), dp=dp.numpy(), dsw=dsw.numpy())


# ================================================================================================ Adam / cast
ADAM_N = [(1, 1, 1, False), (3, 1, 3, False), (4, 1, 0, False), (5, 1, 1, False), (1027, 1, 3, False), (2048 * 256 * 4 + 7, 2048, 3, True)]   # n, grid, tail, loop
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, gscale=0.5, steps=3)


def adam_cases():
    return [dict(kernel="adam", name=f"adam_n{n}", n=n, branch=dict(grid=grid, tail=tail, stride_loop=loop)) for n, grid, tail, loop in ADAM_N]


def adam_inputs(c):
    s, n = seed_of(c["name"]), c["n"]
    g = [randn((n,), s + 10 + k) * (10.0 ** ((k % 3) - 1)) for k in range(ADAM_HP["steps"])]
    for gk in g:
        gk[::5] = 0.0                                               # exact zeros: v stays 0 where every step's gradient is 0
    return dict(p=randn((n,), s + 1), m=randn((n,), s + 2, scale=0.1), v=randn((n,), s + 3).abs() * 0.01, g=g)


def adam_host_scalars(step):
    """pa_adam_step's host arithmetic: (step_size, inv_sqrt_bc2) as the float32 values the kernel receives."""
    b1, b2 = float(np.float32(ADAM_HP["b1"])), float(np.float32(ADAM_HP["b2"]))
    lr = float(np.float32(ADAM_HP["lr"]))
    return float(np.float32(lr / (1.0 - b1 ** step))), float(np.float32(1.0 / math.sqrt(1.0 - b2 ** step)))


def adam_ref(c, t, bias_step_offset=0):
    b1, b2, eps, gs = (float(np.float32(ADAM_HP[k])) for k in ("b1", "b2", "eps", "gscale"))
    p, m, v = f64(t["p"]), f64(t["m"]), f64(t["v"])
    e_p, e_m, e_v = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
    out = []
    for k in range(ADAM_HP["steps"]):
        ss, c2 = adam_host_scalars(k + 1 + bias_step_offset)
        gj = f64(t["g"][k]) * gs
        e_m = b1 * e_m + 4 * U24 * (np.abs(b1 * m) + np.abs((1 - b1) * gj))
        m = b1 * m + (1 - b1) * gj
        v = b2 * v + (1 - b2) * gj * gj
        e_v = b2 * e_v + 4 * U24 * v
        den = np.sqrt(v) * c2 + eps
        upd = ss * m / den
        with np.errstate(divide="ignore", invalid="ignore"):
            rel_v = np.where(v > 0, 0.5 * e_v / np.where(v > 0, v, 1.0), 0.0)
        p = p - upd
        e_p = e_p + np.abs(upd) * (6 * U24 + rel_v) + ss * e_m / den + U24 * np.abs(p)
        out.append(dict(p=(p, e_p), m=(m, e_m), v=(v, e_v)))
    return out


def adam_cpu32(c, t, defect=None):
    b1, b2, eps, gs = (np.float32(ADAM_HP[k]) for k in ("b1", "b2", "eps", "gscale"))
    p, m, v = t["p"].clone(), t["m"].clone(), t["v"].clone()
    out = []
    for k in range(ADAM_HP["steps"]):
        step = k + 1 - (1 if defect == "bias_correction_of_step_minus_1" and k > 0 else 0)
        ss, c2 = (np.float32(a) for a in adam_host_scalars(step))
        gj = t["g"][k] * (np.float32(1) if defect == "gscale_left_out" else gs)
        m = b1 * m + (np.float32(1) - b1) * gj
        v = b2 * v + (np.float32(1) - b2) * gj * gj
        p = p - ss * m / (torch.sqrt(v) * c2 + eps)
        pb = p.view(torch.int32).__rshift__(16).to(torch.int16) if defect == "bf16_by_truncation" else rne_bf16_bits(p)
        out.append(dict(p=p.clone(), m=m.clone(), v=v.clone(), pb=pb))
    return out


def f32_specials():
    """float32 bit patterns: ties to even both ways, just off a tie, subnormals, +-inf, the largest finite values, NaNs."""
    bits = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F817FFF, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x00000001, 0x00008000,
            0x00018000, 0x007FFFFF, 0x80008001, 0x00800000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F8000, 0x7F7F7FFF,
            0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F80FFFF, 0x3F800000, 0x477FE000]
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


CAST_N = [(1, 1, False), (255, 1, False), (257, 2, False), (2048 * 256 + 3, 2048, True)]     # n, grid, grid-stride loop


def cast_cases():
    return [dict(kernel="cast", name=f"cast_{a}_to_{b}_n{n}", src=a, dst=b, n=n, branch=dict(grid=grid, stride_loop=loop))
            for a, b in (("f32", "bf16"), ("bf16", "f32"), ("f32", "f32")) for n, grid, loop in CAST_N]


def cast_inputs(c):
    n = c["n"]
    x = randn((n,), seed_of(c["name"])) * 3
    sp = f32_specials()
    x[:min(n, sp.numel())] = sp[:n]
    if n > 300:
        x[-sp.numel():] = sp
    return dict(src=x if c["src"] == "f32" else x.to(torch.bfloat16))


def cast_want(c, t, defect=None):
    if c["dst"] == "bf16" and defect == "bf16_by_truncation":
        return (t["src"].view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)
    return t["src"].to(DT[c["dst"]])


def same_bits_or_nan(got, want):
    """Bit for bit, except that a NaN only has to stay a NaN."""
    it = _INT[got.element_size()]
    nan = torch.isnan(want.float())
    return bool(torch.equal(torch.isnan(got.float()), nan)) and bool(torch.equal(got.view(it)[~nan], want.view(it)[~nan]))


# ================================================================================================ embeddings
EMB_TABLE_ROWS = (514, 20, 8, 9, 3)                                 # the 8 / 9 boundary (LDS path against global atomics) falls between two tables


def embed_in_cases():
    cs = []
    lanes = {4: 256, 64: 16, 192: 5, 512: 2, 1024: 1}              # tokens a block works on at once: 256 / (d / 4)
    nsmall = {None: 2, 1: 2, 3: 2}                                  # tables of at most 8 rows among those present: the 8- and the 3-row one
    for i, (n_tok, d) in enumerate([(1, 4), (63, 64), (65, 192), (200, 512), (63, 1024), (200, 4), (65, 64), (1, 192)]):
        for dt in ("f32", "bf16"):
            k = i + (dt == "bf16")
            absent = (None, 1, 3, None)[k % 4]
            cs.append(dict(kernel="embed_in", name=f"embed_in_{dt}_n{n_tok}_d{d}_map{k % 2}_absent{absent}", dt=dt, n_tok=n_tok, d=d, rowmap=k % 2, absent=absent,
                           rows=EMB_TABLE_ROWS, branch=dict(lanes=lanes[d], nsmall=nsmall[absent], lds=nsmall[absent] * 32 * d)))
    # the accepted width with three small tables: 96 KB of dynamic LDS
    cs.append(dict(kernel="embed_in", name="embed_in_f32_n200_d1024_three_small", dt="f32", n_tok=200, d=1024, rowmap=1, absent=None, rows=(514, 8, 8, 9, 3),
                   branch=dict(lanes=1, nsmall=3, lds=3 * 8 * 1024 * 4)))
    return cs


def embed_in_inputs(c):
    s, n, d, dt = seed_of(c["name"]), c["n_tok"], c["d"], DT[c["dt"]]
    g = torch.Generator().manual_seed(s)
    n_pos = n + n // 3 + 2 if c["rowmap"] else n                    # positions of the [B * S] id tensors; the rowmap is a strict subset, in order
    rowmap = torch.sort(torch.randperm(n_pos, generator=g)[:n]).values.to(torch.int32) if c["rowmap"] else None
    idx = [torch.randint(0, r, (n_pos,), generator=g) for r in c["rows"]]
    tables = [randn((r, d), s + 10 + k) for k, r in enumerate(c["rows"])]
    dout = randn((n, d), s + 2, dt)
    dout[2::5] = 0.0                                                # rows exactly zero (padded positions)
    if n > 1:
        dout[1, 0] = -0.0
    return dict(idx=idx, tables=tables, rowmap=rowmap, dout=dout, dtab0=[randn((r, d), s + 20 + k) for k, r in enumerate(c["rows"])])


def _positions(c, t):
    return t["rowmap"].long() if t["rowmap"] is not None else torch.arange(c["n_tok"])


def embed_in_ref(c, t):
    pos, d = _positions(c, t), c["d"]
    fwd, s_abs = np.zeros((c["n_tok"], d)), np.zeros((c["n_tok"], d))
    grads = []
    g = f64(t["dout"])
    for k, r in enumerate(c["rows"]):
        if k == c["absent"]:
            grads.append(None)
            continue
        ids = t["idx"][k][pos].numpy()
        tab = f64(t["tables"][k])
        fwd += tab[ids]
        s_abs += np.abs(tab[ids])
        g0 = f64(t["dtab0"][k])
        acc, aabs = g0.copy(), np.abs(g0)
        np.add.at(acc, ids, g)
        np.add.at(aabs, ids, np.abs(g))
        cnt = np.bincount(ids, minlength=r)[:, None]
        grads.append((acc, (cnt + 1) * U24 * aabs))
    return dict(out=(fwd, 5 * U24 * s_abs), grads=grads)


def embed_in_cpu32(c, t, defect=None):
    pos = _positions(c, t)
    if defect == "rowmap_ignored":
        pos = torch.arange(c["n_tok"])
    fwd = torch.zeros(c["n_tok"], c["d"])
    grads = []
    g = t["dout"].float()
    for k, r in enumerate(c["rows"]):
        if k == c["absent"]:
            grads.append(None)
            continue
        ids = t["idx"][k][pos]
        fwd = fwd + t["tables"][k][ids]
        acc = t["dtab0"][k].clone()
        acc.index_add_(0, ids, g)
        grads.append(acc.numpy())
    return dict(out=fwd.numpy(), grads=grads)


def embed_out_cases():
    return [dict(kernel="embed_out", name=f"embed_out_{dt}_B{B}_T{T}_d{d}_dof{dof}", dt=dt, B=B, T=T, d=d, dof=dof, tok_ld=T + 3, V=V, branch=dict(zero_row_only=T == 1))
            for dt in ("f32", "bf16") for B, T, d, dof, V in [(3, 19, 64, 6, 514), (2, 19, 260, 4, 20), (4, 1, 64, 6, 514), (1, 19, 4, 6, 3)]]


def embed_out_inputs(c):
    s, B, T, d, dof = seed_of(c["name"]), c["B"], c["T"], c["d"], c["dof"]
    g = torch.Generator().manual_seed(s)
    npos = max(1, -(-(T - 1) // dof))
    return dict(tok=torch.randint(0, c["V"], (B, T), generator=g), value=randn((c["V"], d), s + 1), coord=randn((dof, d), s + 2), pos=randn((npos, d), s + 3),
                dout=randn((B * T, d), s + 4, DT[c["dt"]]), dv0=randn((c["V"], d), s + 5), dc0=randn((dof, d), s + 6), dp0=randn((npos, d), s + 7))


def embed_out_ref(c, t):
    B, T, d, dof = c["B"], c["T"], c["d"], c["dof"]
    out, s_abs = np.zeros((B, T, d)), np.zeros((B, T, d))
    g = f64(t["dout"]).reshape(B, T, d)
    tabs = [f64(t["value"]), f64(t["coord"]), f64(t["pos"])]
    acc = [f64(t["dv0"]).copy(), f64(t["dc0"]).copy(), f64(t["dp0"]).copy()]
    aabs = [np.abs(a) for a in acc]
    cnt = [np.zeros((a.shape[0], 1)) for a in acc]
    if T > 1:
        t1 = np.arange(T - 1)
        ids = [t["tok"][:, :T - 1].numpy(), np.broadcast_to(t1 % dof, (B, T - 1)), np.broadcast_to(t1 // dof, (B, T - 1))]
        for k in range(3):
            out[:, 1:] += tabs[k][ids[k]]
            s_abs[:, 1:] += np.abs(tabs[k][ids[k]])
            np.add.at(acc[k], ids[k].reshape(-1), g[:, 1:].reshape(-1, d))
            np.add.at(aabs[k], ids[k].reshape(-1), np.abs(g[:, 1:]).reshape(-1, d))
            np.add.at(cnt[k], ids[k].reshape(-1), 1.0)
    zero = np.zeros((B, T, d), bool)
    zero[:, 0] = True
    return dict(out=(out.reshape(B * T, d), 3 * U24 * s_abs.reshape(B * T, d)), zero=zero.reshape(B * T, d), grads=[(acc[k], (cnt[k] + 1) * U24 * aabs[k]) for k in range(3)])


def embed_out_cpu32(c, t, defect=None):
    B, T, d, dof = c["B"], c["T"], c["d"], c["dof"]
    out = torch.zeros(B, T, d)
    g = t["dout"].float().reshape(B, T, d)
    acc = [t["dv0"].clone(), t["dc0"].clone(), t["dp0"].clone()]
    if T > 1:
        t1 = torch.arange(T - 1)
        shift = 1 if defect == "token_not_shifted" else 0          # decoder row t embeds token t - 1
        ids = [t["tok"][:, shift:T - 1 + shift], (t1 % dof).expand(B, T - 1), (t1 // dof).expand(B, T - 1)]
        for k, tab in enumerate((t["value"], t["coord"], t["pos"])):
            out[:, 1:] += tab[ids[k]]
            acc[k].index_add_(0, ids[k].reshape(-1), g[:, 1:].reshape(-1, d))
    return dict(out=out.reshape(B * T, d).numpy(), grads=[a.numpy() for a in acc])


SEG_LENGTHS = [0, 1, 7, 8, 9, 31, 32, 33, 64, 65, 600]


def seg_cases():
    """pa_embed_segment_bwd: tables of 3, 64, 65 and 514 rows whose segment lengths are placed by construction; `ordered` under default switches
    is f32 (the children cross the pairs)."""
    cs = []
    for dt in ("f32", "bf16"):
        for d in (4, 512, 516, 2048, 2052):
            if d > 2048 and dt == "bf16":
                continue
            cs.append(dict(kernel="embed_seg", name=f"embed_seg_{dt}_d{d}", dt=dt, d=d, rows=(3, 64, 65, 514) if d < 2048 else (3, 64, 65),
                           branch=dict(kernel=("ordered4" if d <= 2048 else "one_group_ordered") if dt == "f32" else "atomic", passes=-(-d // 512))))
    return cs


def seg_inputs(c):
    s, d = seed_of(c["name"]), c["d"]
    g = torch.Generator().manual_seed(s)
    lens_all = []
    for r in c["rows"]:
        lens = [SEG_LENGTHS[(q + r) % len(SEG_LENGTHS)] for q in range(r)]
        if r == 3:
            lens = [600, 0, 33]
        else:                                                       # one segment of 600 per table
            first = lens.index(600)
            lens = [l if l < 600 or q == first else 2 for q, l in enumerate(lens)]
        lens_all.append(lens)
    n_rows = max(sum(l) for l in lens_all)
    order, seg = [], []
    for lens in lens_all:                                           # every table groups (a subset of) the same n_rows gradient rows
        perm = torch.randperm(n_rows, generator=g)[:sum(lens)]
        sg = np.concatenate([[0], np.cumsum(lens)])
        order.append(torch.cat([torch.sort(perm[sg[q]:sg[q + 1]]).values for q in range(len(lens))]).to(torch.int32) if sum(lens) else torch.zeros(0, dtype=torch.int32))
        seg.append(torch.from_numpy(sg).to(torch.int32))
    return dict(dout=randn((n_rows, d), s + 1, DT[c["dt"]]), order=order, seg=seg, dtab0=[randn((r, d), s + 5 + k) for k, r in enumerate(c["rows"])], n_rows=n_rows)


def seg_ref(c, t):
    g = f64(t["dout"])
    out = []
    for k, r in enumerate(c["rows"]):
        g0 = f64(t["dtab0"][k])
        acc, aabs = g0.copy(), np.abs(g0)
        sg, od = t["seg"][k].numpy(), t["order"][k].numpy()
        for q in range(r):
            rows = od[sg[q]:sg[q + 1]]
            acc[q] += g[rows].sum(0)
            aabs[q] += np.abs(g[rows]).sum(0)
        out.append((acc, ((sg[1:] - sg[:-1])[:, None] + 1) * U24 * aabs))
    return out


def seg_cpu32(c, t, defect=None):
    g = t["dout"].float()
    out = []
    for k, r in enumerate(c["rows"]):
        acc = t["dtab0"][k].clone()
        sg, od = t["seg"][k].numpy(), t["order"][k].long()
        for q in range(r):
            hi = sg[q] + (sg[q + 1] - sg[q]) // 8 * 8 if defect == "tail_after_last_group_of_8_dropped" else sg[q + 1]
            acc[q] += g[od[sg[q]:hi]].sum(0)
        out.append(acc.numpy())
    return out


# ================================================================================================ batch preparation (exact)
def pack_cases():
    table = [  # B, S, path, batch rows per wave, scan rounds (of 64 counts), passes over S (of 1280 columns), order
        (1, 1, "fused", 1, 1, 1, "rank"), (5, 77, "fused", 1, 1, 1, "rank"), (17, 1280, "fused", 2, 1, 1, "rank"), (65, 1281, "fused", 5, 2, 2, "rank"),
        (1024, 77, "fused", 64, 16, 1, "rank"), (1025, 1, "four_kernel", 65, 17, 1, "rank"), (1025, 77, "four_kernel", 65, 17, 1, "rank"),
        (8193, 1, "four_kernel", 513, 129, 1, "iota"), (17, 1, "fused", 2, 1, 1, "rank"), (65, 77, "fused", 5, 2, 1, "rank")]
    return [dict(kernel="pack_rows", name=f"pack_B{B}_S{S}", B=B, S=S, branch=dict(path=path, rows_per_wave=rpw, scan_rounds=rounds, passes=passes, order=order))
            for B, S, path, rpw, rounds, passes, order in table]


def pack_inputs(c):
    B, S = c["B"], c["S"]
    g = torch.Generator().manual_seed(seed_of(c["name"]))
    valid_len = torch.randint(0, S + 1, (B,), generator=g)
    valid_len[::3] = valid_len[0]                                   # ties in the row counts
    mask = torch.arange(S)[None, :] >= valid_len[:, None]           # True = PAD
    mask ^= (torch.rand(B, S, generator=g) < 0.05)                  # holes: the valid positions are not a prefix
    if B > 2:
        mask[1], mask[B - 1] = True, False                          # a fully masked and a fully valid row
    return dict(mask=mask.to(torch.uint8))


def pack_want(c, t, defect=None):
    B, S = c["B"], c["S"]
    valid = t["mask"] == 0
    cnt = valid.sum(1)
    cu = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(cnt, 0)]).to(torch.int32)
    rowmap = torch.nonzero(valid.reshape(-1))[:, 0].to(torch.int32)
    if B > 8192:
        order = torch.arange(B)                                     # documented: above 8192 batch elements the order is the batch order
    elif defect == "sort_not_stable":
        order = torch.sort(cnt * B + torch.arange(B), descending=True).indices      # ties in REVERSE batch order
    else:
        order = torch.sort(cnt, descending=True, stable=True).indices
    return dict(cu=cu, rowmap=rowmap, order=order.to(torch.int32))


def _gdesc(kind, R, n, rowmap=0, bad=0, B=None, T=None, dof=6):
    return dict(kind=kind, R=R, n=n, rowmap=rowmap, bad=bad, B=B, T=T, dof=dof)


def group_cases():
    """One case = one pa_group_rows launch (one block per table; the largest table sizes the dynamic LDS of all)."""
    launches = {
        "small": [_gdesc(0, 1, 1), _gdesc(0, 2, 63, rowmap=1), _gdesc(0, 6, 1000, bad=1), _gdesc(0, 514, 1000, rowmap=1, bad=1), _gdesc(0, 514, 63), _gdesc(0, 2, 1)],
        "scan2": [_gdesc(0, 1024, 24577, rowmap=1, bad=1), _gdesc(0, 1025, 1000, bad=1), _gdesc(0, 6, 24577)],
        "lds139k": [_gdesc(0, 2048, 24577, bad=1), _gdesc(0, 2048, 63, rowmap=1)],
        "decoder": [_gdesc(1, 514, 63, B=7, T=10, bad=1), _gdesc(2, 6, 63, B=7, T=10), _gdesc(3, 2, 63, B=7, T=10), _gdesc(1, 1024, 1000, B=8, T=126),
                    _gdesc(2, 6, 1000, B=8, T=126, dof=4), _gdesc(3, 1025, 1000, B=8, T=126, dof=4), _gdesc(3, 2, 1000, B=8, T=126)],
    }
    branch = {  # 4 (17 R + 17) bytes of LDS for the largest table of the launch
        "small": dict(lds=35020, set_attribute=False, scan_rounds=1, refetch=False), "scan2": dict(lds=69768, set_attribute=True, scan_rounds=2, refetch=True),
        "lds139k": dict(lds=139332, set_attribute=True, scan_rounds=2, refetch=True), "decoder": dict(lds=69768, set_attribute=True, scan_rounds=2, refetch=False)}
    return [dict(kernel="group_rows", name=f"group_{name}", descs=descs, branch=branch[name]) for name, descs in launches.items()]


def group_inputs(c):
    g = torch.Generator().manual_seed(seed_of(c["name"]))
    out = []
    for q in c["descs"]:
        R, n = q["R"], q["n"]
        if q["kind"] == 0:
            n_pos = n + n // 4 + 1 if q["rowmap"] else n
            idx = torch.randint(0, R, (n_pos,), generator=g)
            idx[::3] = idx[0]                                       # a heavily used row: long runs of ties
            rowmap = torch.sort(torch.randperm(n_pos, generator=g)[:n]).values.to(torch.int32) if q["rowmap"] else None
            if q["bad"] and n > 8:
                where = (rowmap.long() if rowmap is not None else torch.arange(n))[torch.tensor([1, n // 2, n - 2, n // 3])]
                idx[where] = torch.tensor([R, R + 5, -1, -7])       # left out of seg[R] and of order
            out.append(dict(idx=idx, rowmap=rowmap))
        else:
            B, T = q["B"], q["T"]
            idx = torch.randint(0, R, (B, T + 2), generator=g)      # tok_ld = T + 2
            if q["bad"]:
                idx[0, 1], idx[B - 1, T - 2], idx[1, 0] = R, -1, R + 9
            out.append(dict(idx=idx if q["kind"] == 1 else None, rowmap=None))
    return dict(tabs=out)


def group_want(c, t, defect=None):
    out = []
    for q, tt in zip(c["descs"], t["tabs"]):
        R, n = q["R"], q["n"]
        i = torch.arange(n)
        if q["kind"] == 0:
            ids, rows = tt["idx"][tt["rowmap"].long() if tt["rowmap"] is not None else i], i
        else:
            T = q["T"]
            b, t1 = i // (T - 1), i % (T - 1)
            rows = b * T + t1 + 1
            ids = tt["idx"][b, t1] if q["kind"] == 1 else (t1 % q["dof"] if q["kind"] == 2 else t1 // q["dof"])
        ok = (ids >= 0) & (ids < R)
        seg = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(ids[ok], minlength=R), 0)]).to(torch.int32)
        if defect == "sort_not_stable":
            perm = torch.sort(ids[ok] * n + (n - 1 - i[ok])).indices                 # ties in REVERSE entry order
        else:
            perm = torch.sort(ids[ok], stable=True).indices
        out.append(dict(seg=seg, order=rows[ok][perm].to(torch.int32)))
    return out


# ================================================================================================ the case table and the host dispatch
def all_cases():
    cs = (ln_cases() + [FINISH_CASE] + switch_cases() + gelu_cases() + nll_cases() + adam_cases() + cast_cases() + embed_in_cases() + embed_out_cases()
          + seg_cases() + pack_cases() + group_cases())
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


SWITCHES = ("PA_LNB_512", "PA_DETERMINISTIC", "PA_EMBED_ORDERED_GROUPS")
BUNDLES = {"lnb512_0": {"PA_LNB_512": "0"}, "deterministic_0": {"PA_DETERMINISTIC": "0"}, "deterministic_1": {"PA_DETERMINISTIC": "1"},
           "ordered_groups_1": {"PA_EMBED_ORDERED_GROUPS": "1"}}


def _env_int(env, key):
    try:
        return int(env[key]) if key in env else None
    except ValueError:
        return 0                                                    # atoi of text that is no number


def dispatch(c, env=None):
    """The host dispatch of csrc/rowops.hip for a case, restated: a pure function of the case's arguments and of the process's switches (`env`)."""
    env = env or {}
    k = c["kernel"]
    if k == "ln":
        d, es = c["d"], 4 if c["dt"] == "f32" else 2
        v512 = _env_int(env, "PA_LNB_512") != 0
        aligned = (c["mis"] * es) % 16 == 0                         # every operand is a 16-byte aligned window unless `mis` elements push dy off
        bwd = "bwd512" if d == 512 and v512 and aligned else "generic"
        return dict(nv=_nv(d), bwd=bwd, grid_fwd=-(-c["rows"] // 4), nparts=-(-c["rows"] // 8), lds=0 if bwd == "bwd512" else 48 * d,
                    lds_over_64k=bwd == "generic" and 48 * d > 65536, can_img=int(d == 512 and c["dt"] == "f32" and v512))
    if k == "ln_finish":
        return dict(full_unroll=[n > 32 for n in c["nparts"]], nq=3 if any(i != c["null_dzsum"] for i in range(len(c["nparts"]))) else 2)
    if k == "switch":
        return dict(nparts=-(-c["rows"] // 8))
    if k == "gelu":
        blocks = -(-(c["rows"] * (c["cols"] // 4)) // 256)
        return dict(grid=min(blocks, 4096), stride_loop=blocks > 4096)
    if k == "nll":
        return dict(path="fast" if c["V"] <= 1024 and c["T"] <= 256 else "strided")
    if k == "adam":
        n4 = c["n"] >> 2
        return dict(grid=min(max(1, -(-n4 // 256)), 2048), tail=c["n"] & 3, stride_loop=n4 > 2048 * 256)
    if k == "cast":
        return dict(grid=min(-(-c["n"] // 256), 2048), stride_loop=c["n"] > 2048 * 256)
    if k == "embed_in":
        present = [r for q, r in enumerate(c["rows"]) if q != c["absent"]]
        ns = sum(r <= 8 for r in present)
        return dict(lanes=max(1, 256 // (c["d"] // 4)), nsmall=ns, lds=ns * 8 * c["d"] * 4)
    if k == "embed_out":
        return dict(zero_row_only=c["T"] == 1)
    if k == "embed_seg":
        det = _env_int(env, "PA_DETERMINISTIC")
        ordered = (c["dt"] == "f32") if det is None else det != 0
        ord4 = _env_int(env, "PA_EMBED_ORDERED_GROUPS") != 1
        kern = ("ordered4" if ord4 and c["d"] <= 2048 else "one_group_ordered") if ordered else "atomic"
        return dict(kernel=kern, passes=-(-c["d"] // 512), ch=[1 if ordered or r > 64 else 0 for r in c["rows"]])
    if k == "pack_rows":
        B, S = c["B"], c["S"]
        return dict(path="fused" if B <= 1024 else "four_kernel", rows_per_wave=-(-B // 16), scan_rounds=-(-B // 64), passes=-(-S // 1280),
                    order="rank" if B <= 8192 else "iota")
    if k == "group_rows":
        rmax = max(g["R"] for g in c["descs"])
        lds = (17 * rmax + 17) * 4
        return dict(lds=lds, set_attribute=lds > 65536, scan_rounds=max(-(-g["R"] // 1024) for g in c["descs"]),
                    refetch=any(-(-(-(-g["n"] // 16)) // 64) * 64 > 24 * 64 for g in c["descs"]))
    raise KeyError(k)


def on_branch(c, env=None):
    """The case reaches the branch it is meant for (every key of c['branch'] as dispatch() gives it)."""
    got = dispatch(c, env)
    return all(got[k] == v for k, v in c["branch"].items()), got


# ================================================================================================ verify(): one case's outputs against the reference
# `got` is what an implementation produced for a case, in a fixed layout per kernel group: the GPU test fills it from the device, the CPU test
# from simulate() - the float32 restatement, with or without a seeded defect.  verify() returns [(kernel, dtype, r(got), r(cpu32)), ...].
def store(x32, dt):
    """What a kernel stores of float32 values: themselves, or their round-to-nearest bf16 image (float64 numpy)."""
    x = torch.as_tensor(np.ascontiguousarray(x32)) if not isinstance(x32, torch.Tensor) else x32
    return (x.to(torch.bfloat16) if dt == "bf16" else x).to(torch.float64).numpy()


def f64_stats(c, t):
    """mean / rstd of the float64 reference, rounded to float32: the second pair of statistics the backward is run on."""
    ref = ln_fwd_ref(c, t)
    return torch.from_numpy(ref["mean"][0]).float(), torch.from_numpy(ref["rstd"][0]).float()


def simulate_ln(c, t, defect=None):
    f = ln_fwd_cpu32(c, t, defect)
    got = dict(mean=f["mean"], rstd=f["rstd"], y=store(f["y"], c["dt"]), bwd=[])
    for mean32, rstd32 in ((torch.from_numpy(f["mean"]), torch.from_numpy(f["rstd"])), f64_stats(c, t)):
        b = ln_bwd_cpu32(c, t, mean32, rstd32, defect)
        got["bwd"].append(dict(mean32=mean32, rstd32=rstd32, dz=store(b["dz"], c["dt"]), ddrop=store(b["ddrop"], c["dt"]) if c["drop_p"] else None,
                               dgamma=b["dgamma"], dbeta=b["dbeta"], dzsum=b["dzsum"] if c["dzsum"] else None))
    return got


def verify_ln(c, t, got):
    dt = c["dt"]
    ck, ckb = Checked(c, "ln_fwd"), Checked(c, "ln_bwd")
    ref, cpu = ln_fwd_ref(c, t), ln_fwd_cpu32(c, t)
    ck("mean", got["mean"], *ref["mean"], cpu=cpu["mean"])
    ck("rstd", got["rstd"], *ref["rstd"], cpu=cpu["rstd"])
    ck("y", got["y"], *ref["y"], out_dt=dt, cpu=cpu["y"])
    for which, b in zip(("its own statistics", "float64 statistics"), got["bwd"]):
        rb, cb = ln_bwd_ref(c, t, b["mean32"], b["rstd32"]), ln_bwd_cpu32(c, t, b["mean32"], b["rstd32"])
        ckb(f"dz on {which}", b["dz"], *rb["dz"], out_dt=dt, cpu=cb["dz"])
        if c["drop_p"]:
            ckb(f"ddrop on {which}", b["ddrop"], *rb["ddrop"], out_dt=dt, cpu=cb["ddrop"], zero=~rb["keep"])
            if dt == "f32":                                         # a kept element is the kernel's own dz times the scale, to one rounding
                want = (np.asarray(b["dz"], dtype=np.float32) * np.float32(rb["scale"])).astype(np.float64)
                k = rb["keep"]
                assert np.array_equal(np.asarray(b["ddrop"], dtype=np.float64)[k], want[k]), f"{c['name']}: ddrop of a kept element is not dz * scale to one rounding"
        ckb(f"dgamma on {which}", b["dgamma"], *rb["dgamma"], cpu=cb["dgamma"])
        ckb(f"dbeta on {which}", b["dbeta"], *rb["dbeta"], cpu=cb["dbeta"])
        if c["dzsum"]:
            ckb(f"dzsum on {which}", b["dzsum"], *rb["dzsum"], cpu=cb["dzsum"])
    return [("ln_fwd", dt, ck.r, ck.r_cpu), ("ln_bwd", dt, ckb.r, ckb.r_cpu)]


def simulate_finish(c, t, defect=None):
    return finish_cpu32(c, t, defect)


def verify_finish(c, t, got):
    ck = Checked(c, "ln_finish")
    ref, cpu = finish_ref(c, t), finish_cpu32(c, t)
    for i in range(len(c["nparts"])):
        for q, what in enumerate(("dgamma", "dbeta", "dzsum")):
            if ref[i][q] is not None:
                ck(f"descriptor {i} {what}", got[i][q], *ref[i][q], cpu=cpu[i][q])
    return [("ln_finish", "f32", ck.r, ck.r_cpu)]


def simulate_switch(c, t, defect=None):
    s = switch_cpu32(c, t, defect)
    return dict(s=s["s"], dh=store(s["dh"], c["dt"]), dw=s["dw"], db=s["db"])


def verify_switch(c, t, got):
    ck, ckb = Checked(c, "switch_fwd"), Checked(c, "switch_bwd")
    ref, cpu = switch_ref(c, t), switch_cpu32(c, t)
    ck("s", got["s"], *ref["s"], cpu=cpu["s"])
    ckb("dh", got["dh"], *ref["dh"], out_dt=c["dt"], cpu=cpu["dh"])
    ckb("dw", got["dw"], *ref["dw"], cpu=cpu["dw"])
    ckb("db", np.reshape(got["db"], (1,)), *ref["db"], cpu=np.reshape(cpu["db"], (1,)))
    return [("switch_fwd", c["dt"], ck.r, ck.r_cpu), ("switch_bwd", c["dt"], ckb.r, ckb.r_cpu)]


def simulate_gelu(c, t, defect=None):
    s = gelu_cpu32(c, t, defect)
    return dict(y=store(s["y"], c["dt"]), dpre=store(s["dpre"], c["dt"]))


def verify_gelu(c, t, got):
    ck, ckb = Checked(c, "gelu_fwd"), Checked(c, "gelu_bwd")
    ref, cpu = gelu_ref(c, t), gelu_cpu32(c, t)
    ck("y", got["y"], *ref["y"], out_dt=c["dt"], cpu=cpu["y"], zero=ref["zero"])
    ckb("dpre", got["dpre"], *ref["dpre"], out_dt=c["dt"], cpu=cpu["dpre"], zero=ref["zero"])
    return [("gelu_fwd", c["dt"], ck.r, ck.r_cpu), ("gelu_bwd", c["dt"], ckb.r, ckb.r_cpu)]


NLL_BWD_FORMS = [("f32", 1.0, False), ("bf16", 0.25, False), ("f32", 0.25, True), ("bf16", 1.0, True)]    # (gradient dtype, gscale, upstream pointer)


def simulate_nll(c, t, defect=None):
    f = nll_fwd_cpu32(c, t, defect)
    got = dict(fwd=dict(stats=np.array([f["nll"], f["count"], f["hits"]]), lse=f["lse"]),
               fin=dict(stats=np.array([f["nll"], f["count"], f["hits"], 1.0, f["loss"], f["hits"] / (f["count"] + 1e-10)]), lse=f["lse"]), bwd=[])
    lse32, cnt = torch.from_numpy(f["lse"]), np.float32(f["count"])
    for odt, gscale, use_up in NLL_BWD_FORMS:
        up = np.float32(t["up"][0]) if use_up else np.float32(1.0)
        b = nll_bwd_cpu32(c, t, lse32, cnt, up, gscale, defect)
        got["bwd"].append(dict(lse32=lse32, count32=cnt, up32=up, dv=store(b["dv"], odt), dp=store(b["dp"], odt), dsw=b["dsw"]))
    return got


def verify_nll(c, t, got):
    ck, ckb = Checked(c, "nll_fwd"), Checked(c, "nll_bwd")
    cpu = nll_fwd_cpu32(c, t)
    for form in ("fwd", "fin"):
        ref = nll_fwd_ref(c, t, fixed=form == "fin")
        st = np.asarray(got[form]["stats"], dtype=np.float64)
        ck(f"{form}: row_lse", got[form]["lse"], *ref["lse"], cpu=cpu["lse"])
        # fwd: float atomics add the block partials in arrival order; fin: a fixed-point word, no order (nll_sum_yardstick)
        yard = nll_sum_yardstick(c, cpu, ref["nll"][0]) if form == "fwd" else cpu["nll"]
        ck(f"{form}: nll sum", st[:1], np.array([ref["nll"][0]]), np.array([ref["nll"][1]]), cpu=np.array([yard]))
        assert st[1] == ref["count"], f"{c['name']}: {form}: count {st[1]!r}, want {ref['count']}"
        assert st[2] == int(st[2]) and ref["hits"][0] <= st[2] <= ref["hits"][1], f"{c['name']}: {form}: hits {st[2]!r}, want {ref['hits']}"
        if form == "fin":
            assert st[3] == 1.0, f"{c['name']}: stats[3] = {st[3]!r}, want 1.0"
            ck("fin: loss", st[4:5], np.array([ref["loss"][0]]), np.array([ref["loss"][1]]), cpu=np.array([cpu["loss"]]))
            acc = ref["count"] and st[2] / ref["count"]
            assert abs(st[5] - acc) <= 4 * U24 * abs(acc), f"{c['name']}: accuracy {st[5]!r}, want {acc!r}"
    n = c["B"] * c["T"]
    for (odt, gscale, use_up), b in zip(NLL_BWD_FORMS, got["bwd"]):
        rb = nll_bwd_ref(c, t, b["lse32"], b["count32"], b["up32"], gscale)
        cb = nll_bwd_cpu32(c, t, b["lse32"], b["count32"], b["up32"], gscale)
        what = f"{odt} gscale {gscale} {'upstream' if use_up else 'stats[3]'}"
        ckb(f"dvocab {what}", b["dv"], *rb["dv"], out_dt=odt, cpu=cb["dv"], zero=rb["zero_v"])
        ckb(f"dptr {what}", b["dp"], *rb["dp"], out_dt=odt, cpu=cb["dp"], zero=rb["zero_p"])
        ckb(f"dsw {what}", b["dsw"], *rb["dsw"], cpu=cb["dsw"], zero=~nll_rows(c, t)["valid"])
    return [("nll_fwd", "f32", ck.r, ck.r_cpu), ("nll_bwd", "f32", ckb.r, ckb.r_cpu)]


def simulate_adam(c, t, defect=None):
    return adam_cpu32(c, t, defect)


def verify_adam(c, t, got):
    ck = Checked(c, "adam")
    ref, cpu = adam_ref(c, t), adam_cpu32(c, t)
    for k, (g, r, s) in enumerate(zip(got, ref, cpu)):
        for q in ("p", "m", "v"):
            ck(f"step {k + 1} {q}", f64(g[q]), *r[q], cpu=f64(s[q]))
        ck.exact(f"step {k + 1} p_bf16", g["pb"], rne_bf16_bits(torch.as_tensor(g["p"], dtype=torch.float32)))
    return [("adam", "f32", ck.r, ck.r_cpu)]


def simulate_cast(c, t, defect=None):
    return cast_want(c, t, defect)


def verify_cast(c, t, got):
    want = cast_want(c, t)
    assert got.dtype == want.dtype and same_bits_or_nan(got, want), f"{c['name']}: not the round-to-nearest-even image bit for bit"
    return [("cast", f"{c['src']}->{c['dst']}", 0.0, 0.0)]


def simulate_embed_in(c, t, defect=None):
    s = embed_in_cpu32(c, t, defect)
    return dict(out=store(s["out"], c["dt"]), grads=s["grads"])


def verify_embed_in(c, t, got):
    ck, ckb = Checked(c, "embed_in_fwd"), Checked(c, "embed_in_bwd")
    ref, cpu = embed_in_ref(c, t), embed_in_cpu32(c, t)
    ck("out", got["out"], *ref["out"], out_dt=c["dt"], cpu=cpu["out"])
    for k in range(len(c["rows"])):
        if ref["grads"][k] is not None:
            ckb(f"table {k} ({c['rows'][k]} rows) gradient", got["grads"][k], *ref["grads"][k], cpu=cpu["grads"][k])
    return [("embed_in_fwd", c["dt"], ck.r, ck.r_cpu), ("embed_in_bwd", c["dt"], ckb.r, ckb.r_cpu)]


def simulate_embed_out(c, t, defect=None):
    s = embed_out_cpu32(c, t, defect)
    return dict(out=store(s["out"], c["dt"]), grads=s["grads"])


def verify_embed_out(c, t, got):
    ck, ckb = Checked(c, "embed_out_fwd"), Checked(c, "embed_out_bwd")
    ref, cpu = embed_out_ref(c, t), embed_out_cpu32(c, t)
    ck("out", got["out"], *ref["out"], out_dt=c["dt"], cpu=cpu["out"], zero=ref["zero"])
    for k, what in enumerate(("value", "coord", "pos")):
        ckb(f"{what} gradient", got["grads"][k], *ref["grads"][k], cpu=cpu["grads"][k])
    return [("embed_out_fwd", c["dt"], ck.r, ck.r_cpu), ("embed_out_bwd", c["dt"], ckb.r, ckb.r_cpu)]


def simulate_seg(c, t, defect=None):
    return seg_cpu32(c, t, defect)


def verify_seg(c, t, got):
    ck = Checked(c, "embed_seg_bwd")
    ref, cpu = seg_ref(c, t), seg_cpu32(c, t)
    for k, r in enumerate(c["rows"]):
        ck(f"table {k} ({r} rows) gradient", got[k], *ref[k], cpu=cpu[k])
    return [("embed_seg_bwd", c["dt"], ck.r, ck.r_cpu)]


def simulate_pack(c, t, defect=None):
    return pack_want(c, t, defect)


def verify_pack(c, t, got):
    ck, want = Checked(c), pack_want(c, t)
    for k in ("cu", "rowmap", "order"):
        ck.exact(k, got[k], want[k])
    return [("pack_rows", "int32", 0.0, 0.0)]


def simulate_group(c, t, defect=None):
    return group_want(c, t, defect)


def verify_group(c, t, got):
    ck, want = Checked(c), group_want(c, t)
    for i, (g, w) in enumerate(zip(got, want)):
        ck.exact(f"table {i} seg", g["seg"], w["seg"])
        ck.exact(f"table {i} order", g["order"], w["order"])
    return [("group_rows", "int32", 0.0, 0.0)]


GROUPS = {  # kernel group -> (inputs, simulate, verify, the seeded defects its cases must catch)
    "ln": (ln_inputs, simulate_ln, verify_ln, ["one_pass_variance", "mean_skips_last_vector", "divide_by_d_minus_1", "dz_without_xhat_s2", "dgamma_misses_last_block",
                                             "dzsum_sums_dz", "finisher_overwrites", "dropout_without_scale", "dropout_hash_row_col_swapped"]),
    "ln_finish": (finish_inputs, simulate_finish, verify_finish, ["finisher_overwrites"]),
    "switch": (switch_inputs, simulate_switch, verify_switch, ["accumulate_ignored", "finisher_overwrites"]),
    "gelu": (gelu_inputs, simulate_gelu, verify_gelu, ["tanh_approximation", "gradient_without_x_phi", "dropout_without_scale", "dropout_hash_row_col_swapped"]),
    "nll": (nll_inputs, simulate_nll, verify_nll, ["lse_without_max", "pointer_mask_j_gt_i", "argmax_larger_index_on_tie", "switch_clamp_ignored", "gscale_left_out"]),
    "adam": (adam_inputs, simulate_adam, verify_adam, ["bias_correction_of_step_minus_1", "gscale_left_out", "bf16_by_truncation"]),
    "cast": (cast_inputs, simulate_cast, verify_cast, ["bf16_by_truncation"]),
    "embed_in": (embed_in_inputs, simulate_embed_in, verify_embed_in, ["rowmap_ignored"]),
    "embed_out": (embed_out_inputs, simulate_embed_out, verify_embed_out, ["token_not_shifted"]),
    "embed_seg": (seg_inputs, simulate_seg, verify_seg, ["tail_after_last_group_of_8_dropped"]),
    "pack_rows": (pack_inputs, simulate_pack, verify_pack, ["sort_not_stable"]),
    "group_rows": (group_inputs, simulate_group, verify_group, ["sort_not_stable"]),
}
