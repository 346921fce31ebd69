"""Float64 parity checker for the kernels csrc/decode.hip itself defines (TEST INFRASTRUCTURE; plain numpy / torch, no GPU):
dec_attn_kernel<T, DH> (pa_dec_attn), the distribution code row_dist_prepare / row_dist_visit behind the four step tails
(dec_row_dist_kernel, pa_dec_row_dist), dec_split_heads_kernel (pa_dec_split_heads) and dec_embed_kernel (pa_dec_embed).

One case table for tests/test_dec_step_parity_cpu.py (the checker tested on seeded defects) and tests/test_dec_step_float64_gpu.py (every
case through the C ABI on guarded windows).  The layout follows tests/dec_mq_parity.py and tests/rowops_parity.py, whose helpers it uses.
`dispatch(c)` restates the host side and the kernels' loop structure as a pure function of a case; every case names the `edge` it exists
for, and both test files assert that dispatch() puts it there.  `extents(c)` gives, per operand, the element behind the last one the
kernel may touch (clamped rows included); the GPU file asserts before every launch that it lies inside the operand's window.

u = 2^-24.  Every bound below is first order: n u sum |terms| for a sum of n float32 roundings; check() applies 2 x the bound (second
order), + half a bf16 ulp at max(|ref|, |got|) for a bf16 output (one round to nearest even), + 2^-126 (flushed denormals).  exp2f is taken
as v_exp_f32 with 1 ulp = 2 u (the ISA's figure, as DESIGN.md section 31 takes it); expf as 1 ulp = 2 u: profiles/logf_bias.txt measures
0.831 ulp at most on [-37, 0).  Inputs are exact in float64 (bf16 widened exactly).

dec_attn_kernel (scale = dh^-1/2; the kernel works in log2 units with sl = scale log2 e, rounded once):
    x_s = scale sum_j q_j k_sj   A_s = scale sum_j |q_j| |k_sj|   A_max = max_s A_s   P = softmax of x over the allowed keys   o_j = sum_s P_s v_sj
    score        dh products and sums, the product with sl, sl's own two roundings:              |dx_s| <= (dh + 3) u A_s
    p            the rounded subtraction s - m (|s - m| <= A_s + A_max in natural units) and exp2:  (A_s + A_max + 2) u relative
    rescales     a key's weight is multiplied by alpha = exp2f(m - m') once per iteration after its own and by exp2f(m_i - M) in the
                 merge: n_it + 1 factors, each one subtraction (<= 2 A_max u), one exp2 (2 u), one product (u)
    eps_s = (dh + 4) A_s + A_max + 2 + (n_it + 1) (2 A_max + 3)       ebar = sum_s P_s eps_s
    sums         l and acc meet ceil(Lk / NG) terms per partial group and NG partials in the merge: n_sum = ceil(Lk / NG) + NG in the
                 numerator and as much in the denominator; p v, w acc, num / den: 3 more
    E_j = u sum_s P_s (eps_s + ebar + 2 n_sum + 3) |v_sj|
    A row without an allowed key is +0.0 exactly.  The append of the self form is exact: row Lk - 1 of both caches holds the newkv
    slices, every other byte of the caches is as before.

row_dist_prepare / row_dist_visit (x_k = vmax - v_k, e_k = exp(-x_k); nv = ceil(V / 256) + 8 roundings on a term's way through the
per-thread sum, the 6 wave steps and the 2 block steps; nd = 4 ceil(d / 256) + 6 for a dot product of d columns):
    vmax         exact
    vsum         E = u sum_k e_k (x_k + 2) + nv u vsum
    z, prob      z = h . sw_w + b:  E_z = (nd + 1) u (sum |h| |w| + |b|);  prob = 1 / (1 + expf(-z)):  E_prob = prob ((1 - prob) (2 u + E_z) + 2 u)
    plog_j       (pfeat . cache_j) / d:  E_plog_j = (nd + 1) u sum |pfeat| |cache_j| / d;  pmax: max_j E_plog_j
    psum         y_j = pmax - plog_j, f_j = exp(-y_j), np = ceil(t / 256) + 8:  E = sum_j f_j (E_plog_j + E_pmax + u y_j + 2 u) + np u psum
    p vocab      e_k / vsum (x gate 1 - prob from sz = 6 on):  relative u (x_k + 2) + E_vsum / vsum + u (+ (E_prob + u (1 - prob)) / (1 - prob) + u),
                 applied as absolute bounds so that a gate that saturates to 0 in float32 stays inside
    p pointer    f_j / psum x prob where ptr_allowed(t, j) and j < t:  relative E_plog_j + u y_j + 2 u + sum_i pp_i (E_plog_i + u y_i + 2 u) + np u + u
                 + E_prob / prob + u;  exactly 0 where allowed and j = t, exactly float32(1e-6) where not allowed, nothing written behind j = t
    The stored cache row t equals h bit for bit; nothing else of the cache changes.

dec_split_heads_kernel, dec_embed_kernel: exact.  The split is index arithmetic; the embedding is (value + coord) + pos in float32 (no
product, so nothing to contract), its bf16 forms one round to nearest even of that; all zeros at t = 0.

tier 2: r(x) = max |x - ref| / E over the elements with E > 0; r(got) <= FACTOR[kernel] r(cpu32), cpu32 being the float32 restatement of
the kernel's own order in numpy (attn_cpu32, dist_cpu32: the partial groups, the 8-key iterations with their alpha rescale, the merge in
group order; the per-thread strided sums, the wave butterfly and the block sum).  profiles/dec_step_float64_parity.txt has the figures.

Inputs.  Attention: q ~ N(0, 1), keys 0.5 N(0, 1), values N(0, 1); per (row, head) one SPOT key k* at the position the case is named for
(slot 0 of a case: key Lk - 1; the other slots walk 0 and the first and last key of the first two passes and iterations): k* = g q /
(scale |q|^2) so that its score is g = ln(allowed keys) - 1 (at least 1.7 = 3.4 sigma at the 15 keys of the smallest case with more than one)
above the others' ~N(0, 1/4), and its value row is 8 further out.  It carries about a quarter of the weight and the other keys share the
rest, so that counting it twice shows as much as losing it - dropping, doubling or shifting k* is over a hundred bounds (half a bf16 ulp
included), and a wrong key elsewhere is still several.  Masked keys hold 2^20, cache rows from Lk on hold NaN, row Lk - 1 of a self cache holds stale
finite values the kernel must not read.  Distribution: vlog = scale N(0, 1) with NaN behind V, pointer logits of spread `scale` (1 or 30),
the gate mid-range or saturated by a bias of +-30; cache rows behind t hold NaN, row t the guard pattern.
"""
import math

import numpy as np
import torch

from gemm_parity import PATTERN, U24, half_ulp_bf16               # noqa: F401  (PATTERN: the guard pattern the GPU file looks for)
from rowops_parity import C6, seed_of

PA_F32, PA_BF16 = 0, 1
PA_EINVAL, PA_EALIGN, PA_ESHAPE = -1, -2, -3
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
PADT = {"f32": PA_F32, "bf16": PA_BF16}
TNAME = {"f32": "float", "bf16": "bf16"}
F = np.float32
UN, PUN, MAX_T = 8, 8, 2048                                         # decode.hip: key groups per iteration, cached rows per wave step, plog capacity
TINY = 2.0 ** -126
MASKED_ROW = 2.0 ** 20
NEG = F(-np.inf)
LOG2E_F = F(1.4426950408889634)
# The tier-2 factor in force per kernel: 16 unless a kernel that passes tier 1 was MEASURED above it on the MI355X (then twice its worst
# measured value); profiles/dec_step_float64_parity.txt.
FACTOR = {"attn": 16.0, "dist": 16.0}
SPOT_MIN_BOUNDS = 100.0


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _cdiv(a, b):
    return -(-a // b)


# ================================================================================================ restated dispatch
def geometry(dt, dh):
    """LPR lanes per key row, KPW keys per wave step, keys per block pass (= partial groups NG), keys per iteration."""
    EB = 8 if dt == "bf16" else 4
    LPR = dh // EB
    KPW = 64 // LPR
    return dict(EB=EB, LPR=LPR, KPW=KPW, pass_keys=4 * KPW, iter_keys=4 * KPW * UN)


def lk_label(Lk, g):
    P, I = g["pass_keys"], g["iter_keys"]
    return {0: "empty", 1: "one_key", P - 1: "pass-1", P: "pass", P + 1: "pass+1", I - 1: "iter-1", I: "iter", I + 1: "iter+1",
            2 * I + 3: "2iter+3"}.get(Lk, "other")


def ptr_allowed(i, j):
    if i < 6:
        return False
    return (j == i % 6) if j < 6 else ((j % 6) == ((i % 6) + 3) % 6)


def _attn_status(c):
    null, mis = c.get("null"), c.get("misalign")
    H, d, G = c["H"], c["H"] * c["dh"], c["G"]
    B = c.get("rows", c["Bd"] * max(G, 1))
    self_ = c["form"] == "self"
    if null in ("out", "q", "kc", "vc"):
        return PA_EINVAL
    if c["form"] not in ("packed",) and c.get("fixed_lk", 0) <= 0 and null == "t_dev":
        return PA_EINVAL
    if c["Lmax"] <= 0 or c.get("fixed_lk", 0) > c["Lmax"] or G < 1 or B % G:
        return PA_EINVAL
    if self_ and (c.get("with_cu") or c.get("with_kpm") or G > 1):
        return PA_EINVAL
    if c["dh"] not in (16, 32, 64):
        return PA_ESHAPE
    if mis or c["ldq"] < d or c["ldq"] % (8 if c["dt"] == "bf16" else 4):
        return PA_EALIGN
    return 0


def dispatch(c):
    """What the library and the kernel do with a case (module docstring)."""
    k = c["kernel"]
    if k == "attn":
        st = _attn_status(c)
        if st:
            return dict(status=st)
        g = geometry(c["dt"], c["dh"])
        lens = c["lens"]
        lab = {lk_label(L, g) for L in lens}
        return dict(status=0, kernel=f"dec_attn_kernel<{TNAME[c['dt']]}, {c['dh']}>", grid=(c["H"], c["Bd"] * c["G"]), **g,
                    passes=[_cdiv(L, g["pass_keys"]) for L in lens], iters=[_cdiv(L, g["iter_keys"]) for L in lens], labels=lab,
                    lk_source="cu" if c["form"] == "packed" else ("t_dev" if c["form"] == "self" else "fixed_lk"),
                    last_key="newkv" if c["form"] == "self" else "cache", group=c["G"] > 1, mask=c["form"] == "kpm")
    if k == "dist":
        d, t, V = c["d"], c["t"], c["V"]
        nch = d // 256 if d in (256, 512, 768, 1024) else 0
        gated = t + 1 >= 6
        return dict(status=0, kernel=f"dec_row_dist_kernel<{TNAME[c['dt']]}>", grid=c["rows"], nch=nch, gated=gated,
                    ptr_iters=(_cdiv(t, 4 * PUN) if nch else _cdiv(t, 4)) if gated else 0, ptr_tail=bool(gated and nch and t % PUN),
                    softmax_wrap=gated and t > 256, vocab_wrap=V > 256, phase=t % 6)
    if k == "embed":
        return dict(status=0, kernel=f"dec_embed_kernel<{TNAME[c['dt']]}>", grid=_cdiv(c["B"] * (c["d"] // 4), 256), zeros=c["t"] == 0,
                    coord_row=(c["t"] - 1) % c["dof"] if c["t"] else None, pos_row=(c["t"] - 1) // c["dof"] if c["t"] else None, lp=bool(c["lp"]))
    if k == "split":
        return dict(status=0, kernel=f"dec_split_heads_kernel<{TNAME[c['dt']]}>", grid=2048, packed=c["lens"] is not None)
    raise KeyError(k)


def on_edge(c):
    p = dispatch(c)
    if p["status"]:
        return False, p
    e = c["edge"]
    if c["kernel"] == "attn":
        ok = e["label"] in p["labels"] and p["lk_source"] == e["lk_source"] and p["last_key"] == e["last_key"] and \
            max(p["passes"]) == e["passes"] and max(p["iters"]) == e["iters"] and p["group"] == e["group"] and p["mask"] == e["mask"]
    elif c["kernel"] == "dist":
        ok = all(p[k] == v for k, v in e.items())
    else:
        ok = all(p[k] == v for k, v in e.items())
    return ok, p


# ================================================================================================ attention: cases
LK_LABELS = ("one_key", "pass-1", "pass", "pass+1", "iter-1", "iter", "iter+1", "2iter+3")


def lk_list(g):
    P, I = g["pass_keys"], g["iter_keys"]
    return [1, P - 1, P, P + 1, I - 1, I, I + 1, 2 * I + 3]


def _attn_case(name, dt, dh, H, form, lens, *, G=1, Lmax=None, label=None, steps=0):
    g = geometry(dt, dh)
    Lmax = Lmax or max(lens) + 3
    c = dict(kernel="attn", name=f"attn_{name}_{TNAME[dt]}_dh{dh}", dt=dt, dh=dh, H=H, Bd=len(lens), G=G, form=form, lens=list(lens), Lmax=Lmax,
             ldq=3 * H * dh if form == "self" else H * dh, steps=steps)
    if form in ("kpm", "dense"):
        c["fixed_lk"] = lens[0]
    L = max(lens)
    label = label or lk_label(L, g)
    c["edge"] = dict(label=label, lk_source={"packed": "cu", "self": "t_dev"}.get(form, "fixed_lk"), last_key="newkv" if form == "self" else "cache",
                     passes=_cdiv(L, g["pass_keys"]), iters=_cdiv(L, g["iter_keys"]), group=G > 1, mask=form == "kpm")
    return c


def attn_cases():
    cs = []
    i = 0
    for dt in ("f32", "bf16"):
        for dh in (16, 32, 64):
            g = geometry(dt, dh)
            P, I = g["pass_keys"], g["iter_keys"]
            for n, Lk in enumerate(lk_list(g)):                     # the self form at every key count (d 48 and 96: three heads of 16 / 32)
                B, H = (2, 3)[(i + n) % 2], (3, 2)[(i + n) % 2] if dh < 64 else (2, 3)[n % 2]
                cs.append(_attn_case(f"self_Lk{Lk}", dt, dh, H, "self", [Lk] * B, Lmax=Lk + (0 if n % 2 else 2)))
            for Lk, H in ((P + 1, 3), (I, 2), (2 * I + 3, 2)):      # dense with a key-padding mask (3 drawings: the last one fully masked)
                cs.append(_attn_case(f"kpm_S{Lk}", dt, dh, H, "kpm", [Lk] * 3))
            cs.append(_attn_case("packed_ragged_a", dt, dh, 3 if dh < 64 else 2, "packed", [I + 1, 0, 1]))
            cs.append(_attn_case("packed_ragged_b", dt, dh, 2, "packed", [P, I - 1]))
            cs.append(_attn_case("group2_dense", dt, dh, 2, "dense", [I + 1] * 2, G=2))
            cs.append(_attn_case("group3_packed", dt, dh, 3 if dh < 64 else 2, "packed", [P + 1, 2 * I + 3], G=3))
            cs.append(_attn_case("group2_kpm", dt, dh, 3 if dh < 64 else 2, "kpm", [P - 1] * 3, G=2))
            i += 1
    # the chain: t = 0 .. 9 on pattern-filled caches, t_dev advanced on the device, every step's K / V rows from its own newkv alone
    cs.append(_attn_case("chain_t0_9", "f32", 16, 3, "self", [10] * 2, Lmax=12, label="other", steps=10))
    cs.append(_attn_case("chain_t0_9", "bf16", 32, 3, "self", [10] * 3, Lmax=10, label="other", steps=10))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


def attn_rejections():
    """(case, status): launches pa_dec_attn refuses before anything reaches the device."""
    rs = []
    for dt in ("f32", "bf16"):
        base = dict(kernel="attn", dt=dt, dh=16, H=2, Bd=2, G=1, form="dense", lens=[8, 8], Lmax=8, fixed_lk=8, ldq=32, steps=0)

        def add(name, status, **kw):
            c = dict(base, name=f"reject_{name}_{dt}", **kw)
            assert _attn_status(c) == status, (c["name"], _attn_status(c), status)
            rs.append((c, status))
        for p in ("out", "q", "kc", "vc"):
            add(f"null_{p}", PA_EINVAL, null=p)
            add(f"{p}_off_8_bytes", PA_EALIGN, misalign=p)
        add("null_t_dev_without_a_key_count", PA_EINVAL, form="self", fixed_lk=0, ldq=96, null="t_dev")
        add("newkv_off_8_bytes", PA_EALIGN, form="self", fixed_lk=0, ldq=96, misalign="newkv")
        add("dh8", PA_ESHAPE, dh=8, ldq=16)
        add("dh24", PA_ESHAPE, dh=24, ldq=48)
        add("dh128", PA_ESHAPE, dh=128, ldq=256)
        add("ldq_no_vector_multiple", PA_EALIGN, ldq=32 + (4 if dt == "bf16" else 2))
        add("G0", PA_EINVAL, G=0)
        add("rows3_G2", PA_EINVAL, G=2, rows=3)
        add("newkv_with_cu", PA_EINVAL, form="self", fixed_lk=0, ldq=96, with_cu=1)
        add("newkv_with_kpm", PA_EINVAL, form="self", fixed_lk=0, ldq=96, with_kpm=1)
        add("newkv_with_G2", PA_EINVAL, form="self", fixed_lk=0, ldq=96, G=2)
        add("fixed_lk_above_Lmax", PA_EINVAL, fixed_lk=9)
    return rs


# ================================================================================================ attention: inputs
def attn_mask(c):
    """kpm uint8 [Bd, Lmax]: holes, a masked first key, a masked last key, the last drawing fully masked."""
    Bd, Lmax, S = c["Bd"], c["Lmax"], c["lens"][0]
    m = np.zeros((Bd, Lmax), dtype=np.uint8)
    g = geometry(c["dt"], c["dh"])
    for b in range(Bd):
        for x in (2, 5 + b, g["pass_keys"] - 2, g["pass_keys"] + 1, g["iter_keys"] + 2):
            if 0 < x < S - 1:
                m[b, x] = 1
    m[0, 0] = 1                                                     # a masked first key
    m[1 % Bd, S - 1] = 1                                            # a masked last key
    m[Bd - 1, :] = 1                                                # a drawing without an allowed key
    m[:, S:] = 0                                                    # (behind the keys: never read; a kernel that strides by Lk reads these)
    return m


def spot_edges(Lk, g):
    P, I = g["pass_keys"], g["iter_keys"]
    out = []
    for k in (Lk - 1, 0, P - 1, P, 2 * P - 1, 2 * P, I - 1, I, 2 * I - 1, 2 * I):
        if 0 <= k < Lk and k not in out:
            out.append(k)
    return out


def _nearest_allowed(ok, k):
    for dist in range(len(ok)):
        for q in (k - dist, k + dist):
            if 0 <= q < len(ok) and ok[q]:
                return q
    return None


class AttnTensors:
    """The operands of a case on the CPU as float32 arrays holding values of the case's type.  rows B = Bd G; cache sets nb = B (self) or Bd.
    q [B, H, dh]; K, V [nb, H, Lmax, dh]: the TRUE keys of every set (rows from Lk on NaN); kc0 / vc0: the caches as the launch finds them
    (self: row Lk - 1 stale); newkv [B, 3 d] (self); kpm, cu; allowed[bk]; spot[(r, h)].  A chain holds `steps` of newkv rows."""

    def __init__(self, c):
        self.c = c
        g = self.g = geometry(c["dt"], c["dh"])
        dh, H, Bd, G, Lmax, form = c["dh"], c["H"], c["Bd"], c["G"], c["Lmax"], c["form"]
        B = self.B = Bd * G
        nb = self.nb = B if form == "self" else Bd
        self.d = d = H * dh
        gen = torch.Generator().manual_seed(seed_of(c["name"]))
        rn = lambda *s: torch.randn(*s, generator=gen)
        bf = (lambda x: _bf(x)) if c["dt"] == "bf16" else (lambda x: x)
        scale = 1.0 / math.sqrt(dh)
        steps = max(c["steps"], 1)
        self.q_steps, self.new_steps = [], []
        kpm = attn_mask(c) if form == "kpm" else None
        self.allowed = [np.ones(c["lens"][bk], dtype=bool) & (True if kpm is None else kpm[bk, :c["lens"][bk]] == 0) for bk in range(nb)]
        K, V = 0.5 * rn(nb, H, Lmax, dh), rn(nb, H, Lmax, dh)
        self.spot = {}
        for step in range(steps):
            q = bf(rn(B, H, dh))
            self.q_steps.append(q)
            if c["steps"]:                                          # chain: the step's own key / value row, spot on the newest key at odd steps
                kn, vn = 0.5 * rn(B, H, dh), rn(B, H, dh)
                if step % 2:
                    gap = math.log(step + 1) + 1.0
                    kn = q * (gap / (scale * (q * q).sum(-1, keepdim=True)))
                    vn = vn + 4.0
                K[:, :, step], V[:, :, step] = kn, vn
        q = self.q_steps[0]
        if not c["steps"]:
            for r in range(B):
                bk = r if form == "self" else r // G
                ok = self.allowed[bk]
                if not ok.any():
                    continue
                ed = spot_edges(len(ok), g)
                gap = math.log(max(int(ok.sum()), 2)) - 1.0
                for h in range(H):
                    taken = [self.spot[(r2, h)] for r2 in range(bk * G, r)] if form != "self" else []      # rows of a group: one spot key each
                    free = ok.copy()
                    free[taken] = False
                    k = _nearest_allowed(free if free.any() else ok, ed[(r * H + h) % len(ed)])
                    self.spot[(r, h)] = k
                    K[bk, h, k] = q[r, h] * (gap / (scale * float((q[r, h] * q[r, h]).sum())))
                    V[bk, h, k] += 8.0 * (1 if (r + h) % 2 else -1)
        K, V = bf(K), bf(V)
        for bk in range(nb):
            Lk = len(self.allowed[bk])
            K[bk, :, Lk:], V[bk, :, Lk:] = float("nan"), float("nan")
            bad = torch.from_numpy(~self.allowed[bk])
            K[bk, :, :Lk][:, bad], V[bk, :, :Lk][:, bad] = MASKED_ROW, MASKED_ROW
        self.K, self.V = K, V
        self.kc0, self.vc0 = K.clone(), V.clone()
        self.newkv = None
        if form == "self":
            if c["steps"]:
                self.kc0[:], self.vc0[:] = PATTERN, PATTERN
                for step in range(steps):
                    self.new_steps.append(torch.cat([self.q_steps[step].reshape(B, d), K[:, :, step].reshape(B, d), V[:, :, step].reshape(B, d)], dim=1))
            else:
                Lk = c["lens"][0]
                self.newkv = torch.cat([q.reshape(B, d), K[:, :, Lk - 1].reshape(B, d), V[:, :, Lk - 1].reshape(B, d)], dim=1)
                self.kc0[:, :, Lk - 1], self.vc0[:, :, Lk - 1] = bf(0.5 * rn(nb, H, dh)), bf(rn(nb, H, dh) - 4.0)      # stale
        self.q = q
        self.kpm = torch.from_numpy(kpm) if kpm is not None else None
        self.cu = torch.tensor(np.concatenate(([0], np.cumsum(c["lens"]))), dtype=torch.int32) if form == "packed" else None

    def lk(self, bk, step=None):
        return (step + 1) if self.c["steps"] else len(self.allowed[bk])

    def ok(self, bk, step=None):
        return np.ones(step + 1, dtype=bool) if self.c["steps"] else self.allowed[bk]


def store(dt, x):
    """What a kernel stores of float32 values: themselves, or their round-to-nearest-even bf16 image (float64)."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float32))
    return (_bf(x) if dt == "bf16" else x).to(torch.float64).numpy()


# ================================================================================================ attention: float64 reference
def attn_reference(c, t, step=None):
    """ref, E [B, d] (float64; E in absolute units, u included) and has [B, H]."""
    g, dh, H = t.g, c["dh"], c["H"]
    NG, I = g["pass_keys"], g["iter_keys"]
    scale = 1.0 / math.sqrt(dh)
    ref, E, has = np.zeros((t.B, t.d)), np.zeros((t.B, t.d)), np.zeros((t.B, H), dtype=bool)
    q_all = (t.q_steps[step] if step is not None else t.q).to(torch.float64).numpy()
    for r in range(t.B):
        bk = r if c["form"] == "self" else r // c["G"]
        Lk, ok = t.lk(bk, step), t.ok(bk, step)
        if not ok.any():
            continue
        has[r] = True
        n_it, n_sum = _cdiv(Lk, I), _cdiv(Lk, NG) + NG
        for h in range(H):
            k = t.K[bk, h, :Lk].to(torch.float64).numpy()[ok]
            v = t.V[bk, h, :Lk].to(torch.float64).numpy()[ok]
            q = q_all[r, h]
            x = scale * (k @ q)
            A = scale * (np.abs(k) @ np.abs(q))
            p = np.exp(x - x.max())
            p /= p.sum()
            eps = (dh + 4) * A + A.max() + 2 + (n_it + 1) * (2 * A.max() + 3)
            w = p * (eps + float(p @ eps) + 2 * n_sum + 3)
            ref[r, h * dh:(h + 1) * dh] = p @ v
            E[r, h * dh:(h + 1) * dh] = U24 * (w @ np.abs(v))
    return dict(ref=ref, E=E, has=has)


# ================================================================================================ attention: float32 restatement
ATTN_DEFECTS = ("last_key_of_a_pass_dropped", "lk_minus_one", "lk_plus_one", "fresh_row_from_the_stale_cache", "clamped_key_counted",
                "mask_stride_lk", "mask_shifted_by_one", "group_row_b_for_b_div_g", "exp_for_exp2", "l_not_rescaled", "partial_merged_unweighted",
                "append_at_lk", "nan_for_an_empty_row", "output_rounded_twice")


def _dots32(q, K, g):
    """a = sum_e q_e k_e per key in the kernel's order: EB elements in sequence per lane, then the xor butterfly over the LPR lanes."""
    prod = (q[None, :] * K).astype(F).reshape(K.shape[0], g["LPR"], g["EB"])
    a = prod[..., 0]
    for e in range(1, g["EB"]):
        a = a + prod[..., e]
    while a.shape[1] > 1:
        a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0]


def _slot32(g, q, Kc, Vc, Lk, fresh, mask_flat, mask_off, sl, defect, edit):
    """One (row, head) of dec_attn_kernel in float32: (out [dh] float32, den)."""
    NG, IT, dh, Lmax = g["pass_keys"], g["iter_keys"], q.shape[0], Kc.shape[0]
    if Lk <= 0:
        return np.zeros(dh, dtype=F), F(0)
    n_it = _cdiv(Lk, IT)
    key = np.arange(n_it * IT)
    inn = key < Lk
    row = np.minimum(np.minimum(key, Lk - 1), Lmax - 1)
    Kr, Vr = Kc[row].copy(), Vc[row].copy()
    if fresh is not None and defect != "fresh_row_from_the_stale_cache":
        fr = key >= Lk - 1
        Kr[fr], Vr[fr] = fresh[0], fresh[1]
    ok = np.ones_like(inn) if defect == "clamped_key_counted" else inn.copy()
    if mask_flat is not None:
        mi = np.where(inn, key, 0) + (1 if defect == "mask_shifted_by_one" else 0)
        ok &= mask_flat[np.minimum(mask_off + mi, len(mask_flat) - 1)] == 0
    if defect == "last_key_of_a_pass_dropped":
        ok &= (key % NG) != NG - 1
    weight = np.ones(len(key), dtype=F)
    if edit is not None:
        how, ks = edit
        if how == "drop":
            ok[ks] = False
        elif how == "double":
            weight[ks] = 2
        elif how == "shift":
            nbr = ks + 1 if ks + 1 < Lk else ks - 1
            Kr[ks], Vr[ks] = Kr[nbr].copy(), Vr[nbr].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.where(ok, (_dots32(q, Kr, g) * sl).astype(F), NEG).reshape(n_it, UN, NG)
    Vr, weight = Vr.reshape(n_it, UN, NG, dh), weight.reshape(n_it, UN, NG)
    ex = np.exp if defect == "exp_for_exp2" else np.exp2
    m, l, acc = np.full(NG, NEG), np.zeros(NG, dtype=F), np.zeros((NG, dh), dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        for it in range(n_it):
            mn = np.maximum(m, s[it].max(axis=0))
            live = mn > NEG
            msafe = np.where(live, mn, F(0))
            alpha = np.where(live, ex((m - msafe).astype(F)), F(1)).astype(F)
            if defect != "l_not_rescaled":
                l = (l * alpha).astype(F)
            acc = (acc * alpha[:, None]).astype(F)
            for j in range(UN):
                p = np.where(live, ex((s[it, j] - msafe).astype(F)), F(0)).astype(F)
                pj = (p * weight[it, j]).astype(F)                  # (an edited key counted twice)
                l = (l + pj).astype(F)
                acc = (acc + (pj[:, None] * Vr[it, j]).astype(F)).astype(F)
            m = np.where(live, mn, m)
        M = m.max()
        num, den = np.zeros(dh, dtype=F), F(0)
        for i in range(NG):
            if m[i] == NEG:
                continue
            w = F(1) if defect == "partial_merged_unweighted" else ex(F(m[i] - M))
            den = F(den + F(l[i] * w))
            num = (num + (acc[i] * w).astype(F)).astype(F)
        if defect == "output_rounded_twice":
            num, den = _bf(torch.from_numpy(num)).numpy(), F(_bf(torch.tensor(float(den))).item())
        if den > 0:
            return (num / den).astype(F), den
    return np.full(dh, F(np.nan) if defect == "nan_for_an_empty_row" else F(0)), den


def attn_cpu32(c, t, defect=None, edit=None, step=None, caches=None):
    """dec_attn_kernel restated in float32 numpy (module docstring): dict(out [B, d] as stored (float64), kc, vc: the caches after the launch).
    edit = ("drop" | "double" | "shift"): applied to the spot key of every (row, head).  A chain passes `step` and the running `caches`."""
    g, dh, H, G, form = t.g, c["dh"], c["H"], c["G"], c["form"]
    sl = F(F(1.0 / np.sqrt(F(dh))) * LOG2E_F)
    kc, vc = caches if caches is not None else (t.kc0.numpy().copy(), t.vc0.numpy().copy())
    q_all = (t.q_steps[step] if step is not None else t.q).numpy()
    newkv = (t.new_steps[step] if step is not None else t.newkv)
    newkv = None if newkv is None else newkv.numpy()
    mask_flat = None if t.kpm is None else t.kpm.numpy().reshape(-1)
    out = np.zeros((t.B, t.d), dtype=F)
    appends = []
    d = t.d
    for r in range(t.B):
        bk = r if form == "self" else r // G
        if defect == "group_row_b_for_b_div_g":
            bk = min(r, t.nb - 1)
        Lk = t.lk(bk, step)
        Lk += {"lk_minus_one": -1, "lk_plus_one": 1}.get(defect, 0)
        for h in range(H):
            fresh = None
            if newkv is not None:
                fresh = (newkv[r, d + h * dh:d + (h + 1) * dh], newkv[r, 2 * d + h * dh:2 * d + (h + 1) * dh])
                dst = Lk - 1 + (1 if defect == "append_at_lk" else 0)
                if 0 <= dst < c["Lmax"]:
                    appends.append((bk, h, dst, fresh))
            moff = bk * (Lk if defect == "mask_stride_lk" else c["Lmax"])
            ed = None if edit is None or (r, h) not in t.spot else (edit, t.spot[(r, h)])
            o, _ = _slot32(g, q_all[r, h], kc[bk, h], vc[bk, h], Lk, fresh, mask_flat, moff, sl, defect, ed)
            out[r, h * dh:(h + 1) * dh] = o
    for bk, h, dst, fresh in appends:                               # (after the reads: no block reads the row it appends)
        kc[bk, h, dst], vc[bk, h, dst] = fresh
    return dict(out=store(c["dt"], out), kc=kc, vc=vc)


def attn_want_caches(c, t, step=None):
    """The caches after a correct launch: row Lk - 1 of every (row, head) holds the newkv slices, everything else is as before."""
    kc, vc = t.kc0.numpy().copy(), t.vc0.numpy().copy()
    if c["form"] == "self":
        steps = range(step + 1) if step is not None else [None]
        for s_ in steps:
            Lk = (s_ + 1) if s_ is not None else c["lens"][0]
            kc[:, :, Lk - 1], vc[:, :, Lk - 1] = t.K[:, :, Lk - 1].numpy(), t.V[:, :, Lk - 1].numpy()
    return kc, vc


def attn_applies(defect, c):
    g = geometry(c["dt"], c["dh"])
    if defect in ("mask_stride_lk", "mask_shifted_by_one"):
        return c["form"] == "kpm"
    if defect == "group_row_b_for_b_div_g":
        return c["G"] > 1
    if defect in ("fresh_row_from_the_stale_cache", "append_at_lk"):
        return c["form"] == "self" and not c["steps"]
    if defect == "last_key_of_a_pass_dropped":
        return max(c["lens"]) >= g["pass_keys"]
    if defect in ("l_not_rescaled",):
        return max(c["lens"]) > g["iter_keys"]
    if defect == "partial_merged_unweighted":
        return max(c["lens"]) > 1
    if defect == "nan_for_an_empty_row":
        return c["form"] == "kpm" or 0 in c["lens"]
    if defect == "output_rounded_twice":
        return c["dt"] == "bf16"
    if defect == "clamped_key_counted":
        return any(L % g["iter_keys"] for L in c["lens"])
    return not c["steps"]


# ================================================================================================ the checks
def ratio(x, ref, E):
    x = np.asarray(x, dtype=np.float64)
    ok = E > 0
    if not ok.any():
        return 0.0
    if not np.isfinite(x[ok]).all():
        return float("inf")
    return float((np.abs(x - ref)[ok] / (E[ok] + 0.5 * TINY)).max())


def check(name, kernel, what, got, ref, E, out_dt="f32", cpu=None, where=None):
    """Assert one output per element at tier 1, then tier 2 against the restatement `cpu`.  Returns (r(got), r(cpu32))."""
    got, ref, E = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(E, dtype=np.float64)
    assert got.shape == ref.shape == E.shape, (name, what, got.shape, ref.shape, E.shape)
    tag = f"{name}: {what} [{kernel}]"
    bound = 2.0 * E + TINY
    if out_dt == "bf16":
        bound = bound + half_ulp_bf16(np.maximum(np.abs(ref), np.abs(np.where(np.isfinite(got), got, 0.0))))
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - ref) <= bound)                         # (a NaN is never inside)
    if bad.any():
        err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            rel = np.where(bad, err / bound, 0.0)
        idx = np.unravel_index(int(np.argmax(rel)), rel.shape)
        at = where(idx) if where else tuple(int(i) for i in idx)
        raise AssertionError(f"{tag}: tier 1: {int(bad.sum())} of {bad.size} elements outside the bound; worst at {at}: got {got[idx]!r}, "
                             f"ref {ref[idx]!r}, |got - ref| = {rel[idx]:.3g} x the bound ({bound[idx]:.3g})")
    r = ratio(got, ref, E)
    r_cpu = None
    if cpu is not None:
        r_cpu = ratio(cpu, ref, E)
        f = FACTOR[kernel]
        if not r <= f * r_cpu:
            raise AssertionError(f"{tag}: tier 2: r(got) = {r:.4g} > {f:g} x r(cpu32) = {f:g} x {r_cpu:.4g}")
    return r, r_cpu


def same_bits(name, what, got, want):
    """Bit for bit: got, want float32 arrays holding the stored values, or integer arrays.  A NaN equals a NaN (the never-fetched rows: the
    payload of a NaN does not survive the widening from bf16)."""
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert a.shape == b.shape, (name, what, a.shape, b.shape)
    if a.dtype.kind == "f":
        both = np.isnan(a) & np.isnan(b)
        a, b = np.where(both, 0, a.astype(np.float32).view(np.int32)), np.where(both, 0, b.astype(np.float32).view(np.int32))
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{name}: exact: {what}: {len(bad)} of {a.size} element(s) differ, first at {tuple(int(i) for i in bad[0])}")


def attn_judge(c, t, got, kc, vc, ref, cpu, step=None):
    """Everything a launch of the attention is held to: tier 1, +0.0 on rows without keys, tier 2, the caches bit for bit."""
    def where(idx):
        r, j = int(idx[0]), int(idx[1])
        bk = r if c["form"] == "self" else r // c["G"]
        return f"(row, head, col) = ({r}, {j // c['dh']}, {j % c['dh']}): {t.lk(bk, step)} keys, spot key {t.spot.get((r, j // c['dh']))}"
    got = np.asarray(got, dtype=np.float64)
    out = check(c["name"], "attn", "out", got, ref["ref"], ref["E"], c["dt"], cpu["out"] if cpu is not None else None, where)
    keyless = np.repeat(~ref["has"], c["dh"], axis=1)
    if keyless.any():
        z = got[keyless]
        assert not (np.signbit(z).any() or (z != 0).any()), f"{c['name']}: exact: a row without an allowed key is not +0.0"
    wk, wv = attn_want_caches(c, t, step)
    same_bits(c["name"], "K cache after the launch (append at row Lk - 1, nothing else)", kc, wk)
    same_bits(c["name"], "V cache after the launch (append at row Lk - 1, nothing else)", vc, wv)
    return out


# ================================================================================================ distribution
D_ALL = (256, 512, 768, 1024, 48, 96)
T_FULL = (0, 4, 5, 6, 7, 8, 9, 10, 11, 31, 32, 33, 63, 64, 65, 255, 256, 257, 299)
T_SHORT = (5, 6, 31, 32, 33, 65, 257, 299)


def dist_cases():
    cs = []
    i = 0
    for dt in ("f32", "bf16"):
        for d in D_ALL:
            for t in (T_FULL if d in (768, 48) else T_SHORT):
                V = 514 if i % 5 else 200                            # (not a multiple of 256; one in five below 256)
                cs.append(dict(kernel="dist", name=f"dist_{TNAME[dt]}_d{d}_t{t}", dt=dt, d=d, t=t, Tmax=300, rows=2 + i % 2, V=V, ldv=(V + 8) // 8 * 8 + 8 * (i % 2),
                               scale=30.0 if i % 3 == 1 else 1.0, gate=("mid", "sat_hi", "mid", "sat_lo")[i % 4]))
                i += 1
        cs.append(dict(kernel="dist", name=f"dist_{TNAME[dt]}_d256_t2047", dt=dt, d=256, t=2047, Tmax=2048, rows=2, V=514, ldv=520, scale=1.0, gate="mid"))
    for c in cs:
        d, t = c["d"], c["t"]
        nch = d // 256 if d % 256 == 0 else 0
        gated = t >= 5
        c["edge"] = dict(nch=nch, gated=gated, ptr_iters=(_cdiv(t, 32) if nch else _cdiv(t, 4)) if gated else 0, ptr_tail=bool(gated and nch and t % 8),
                         softmax_wrap=gated and t > 256, phase=t % 6, vocab_wrap=c["V"] > 256)
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


class DistTensors:
    def __init__(self, c):
        d, t, V, rows, Tmax, sc = c["d"], c["t"], c["V"], c["rows"], c["Tmax"], c["scale"]
        gen = torch.Generator().manual_seed(seed_of(c["name"]))
        rn = lambda *s: torch.randn(*s, generator=gen)
        bf = (lambda x: _bf(x)) if c["dt"] == "bf16" else (lambda x: x)
        self.vlog = torch.full((rows, c["ldv"]), float("nan"))
        self.vlog[:, :V] = sc * rn(rows, V)
        self.pfeat = bf(sc * math.sqrt(d) * rn(rows, d))
        self.h = bf(rn(rows, d))
        self.cache0 = torch.full((Tmax, rows, d), float("nan"))
        self.cache0[:t] = bf(rn(t, rows, d))
        self.cache0[t] = PATTERN
        self.sw_w = rn(d) / math.sqrt(d)
        self.sw_b = torch.tensor([{"mid": 0.25, "sat_hi": 30.0, "sat_lo": -30.0}[c["gate"]]])


def dist_reference(c, t_):
    """p, E [rows, V + Tmax] (NaN where nothing is written), stats, Es [rows, 5] in float64."""
    d, t, V, rows, Tmax = c["d"], c["t"], c["V"], c["rows"], c["Tmax"]
    u = U24
    p = np.full((rows, V + Tmax), np.nan)
    E = np.zeros((rows, V + Tmax))
    st, Es = np.zeros((rows, 5)), np.zeros((rows, 5))
    nv, npt, nd = _cdiv(V, 256) + 8, _cdiv(max(t, 1), 256) + 8, 4 * _cdiv(d, 256) + 6
    for r in range(rows):
        v = t_.vlog[r, :V].to(torch.float64).numpy()
        x = v.max() - v
        e = np.exp(-x)
        vsum = e.sum()
        E_vsum = u * float(e @ (x + 2)) + nv * u * vsum
        pv = e / vsum
        E_pv = pv * (u * (x + 2) + E_vsum / vsum + u)
        st[r] = (v.max(), vsum, -np.inf, 0.0, 0.0)
        Es[r, 1] = E_vsum
        if t + 1 < 6:
            p[r, :V], E[r, :V] = pv, E_pv
            continue
        h, w, b = t_.h[r].to(torch.float64).numpy(), t_.sw_w.to(torch.float64).numpy(), float(t_.sw_b[0])
        z = float(h @ w) + b
        E_z = (nd + 1) * u * (float(np.abs(h) @ np.abs(w)) + abs(b))
        prob = 1.0 / (1.0 + math.exp(-z))
        E_prob = prob * ((1 - prob) * (2 * u + E_z) + 2 * u)
        gate = 1 - prob
        p[r, :V] = pv * gate
        E[r, :V] = E_pv * gate + pv * (E_prob + u * gate) + u * pv * gate
        pf, hc = t_.pfeat[r].to(torch.float64).numpy(), t_.cache0[:t, r].to(torch.float64).numpy()
        plog = (hc @ pf) / d
        E_pl = (nd + 1) * u * (np.abs(hc) @ np.abs(pf)) / d
        y = plog.max() - plog
        f = np.exp(-y)
        psum = f.sum()
        E_pm = float(E_pl.max())
        rel = E_pl + u * y + 2 * u
        pp = f / psum
        E_psum = float(f @ (rel + E_pm)) + npt * u * psum
        st[r, 2:], Es[r, 2:] = (plog.max(), psum, prob), (E_pm, E_psum, E_prob)
        for j in range(t + 1):
            if not ptr_allowed(t, j):
                p[r, V + j] = C6
            elif j < t:
                p[r, V + j] = pp[j] * prob
                E[r, V + j] = pp[j] * prob * (rel[j] + float(pp @ rel) + npt * u + u + u) + pp[j] * E_prob
            else:
                p[r, V + j] = 0.0
    return dict(p=p, E=E, stats=st, Es=Es)


DIST_DEFECTS = ("gate_inverted", "row_t_minus_1_missing_from_the_pointer_softmax", "clamped_tail_row_counted", "div_d_missing", "threshold_sz_lt_5",
                "threshold_sz_lt_7", "fill_before_gating", "ptr_allowed_phase_off_by_one", "vocab_tail_read_to_ldv")


def _wave_tree(a):
    """The xor butterfly of wave_sum over the last axis of 64 lanes."""
    o = 32
    while o:
        a = a[..., :o] + a[..., o:2 * o]
        o //= 2
    return a[..., 0]


def _block_sum32(terms):
    """block_sum of per-element terms [n] handed out k = tid, tid + 256, ...: per-thread sums in sequence, wave butterflies, (s0 + s1) + (s2 + s3)."""
    n = len(terms)
    pad = np.zeros(_cdiv(max(n, 1), 256) * 256, dtype=F)
    pad[:n] = terms
    pad = pad.reshape(-1, 256)
    acc = np.zeros(256, dtype=F)
    for row in pad:
        acc = (acc + row).astype(F)
    s = _wave_tree(acc.reshape(4, 64)).astype(F)
    return F(F(s[0] + s[1]) + F(s[2] + s[3]))


def _dot256(a, B):
    """Rows of B [n, d] against a [d] in the order of ptr_logits / the gate: per lane and 256-column chunk ((a0 b0 + a1 b1) + a2 b2) + a3 b3,
    chunks in sequence, then the wave butterfly (columns behind d count as lanes that add 0)."""
    n, d = B.shape
    nch = _cdiv(d, 256)
    pa, pb = np.zeros(nch * 256, dtype=F), np.zeros((n, nch * 256), dtype=F)
    pa[:d], pb[:, :d] = a, B
    pr = (pa[None, :] * pb).astype(F).reshape(n, nch, 64, 4)
    ch = (((pr[..., 0] + pr[..., 1]).astype(F) + pr[..., 2]).astype(F) + pr[..., 3]).astype(F)
    acc = np.zeros((n, 64), dtype=F)
    for q in range(nch):
        acc = (acc + ch[:, q]).astype(F)
    return _wave_tree(acc).astype(F)


def dist_cpu32(c, t_, defect=None):
    """dec_row_dist_kernel restated in float32 numpy: dict(p [rows, V + Tmax] float32 (NaN: not written), stats [rows, 5], cache after)."""
    d, t, V, rows, Tmax = c["d"], c["t"], c["V"], c["rows"], c["Tmax"]
    p = np.full((rows, V + Tmax), np.nan, dtype=F)
    st = np.zeros((rows, 5), dtype=F)
    cache = t_.cache0.numpy().copy()
    cache[t] = t_.h.numpy()
    thr = {"threshold_sz_lt_5": 5, "threshold_sz_lt_7": 7}.get(defect, 6)
    Vr = c["ldv"] if defect == "vocab_tail_read_to_ldv" else V
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r in range(rows):
            v = t_.vlog[r, :Vr].numpy()
            vmax = v.max() if not np.isnan(v).any() else F(np.nan)
            e = np.exp((v - vmax).astype(F)).astype(F)
            vsum = _block_sum32(e)
            pv = (np.exp((t_.vlog[r, :V].numpy() - vmax).astype(F)).astype(F) / vsum).astype(F)
            st[r] = (vmax, vsum, NEG, 0, 0)
            if t + 1 < thr:
                p[r, :V] = pv
                continue
            n = t - 1 if defect == "row_t_minus_1_missing_from_the_pointer_softmax" else t
            plog = _dot256(t_.pfeat[r].numpy(), t_.cache0[:t, r].numpy()) if t else np.zeros(0, dtype=F)
            if defect != "div_d_missing":
                plog = (plog / F(d)).astype(F)
            z = F(_dot256(t_.sw_w.numpy(), t_.h[r:r + 1].numpy())[0] + t_.sw_b.numpy()[0])
            prob = F(F(1) / F(F(1) + np.exp(F(-z))))
            if defect == "gate_inverted":
                prob = F(F(1) - prob)
            pl = plog[:n]
            if defect == "clamped_tail_row_counted" and t % PUN:
                pl = np.concatenate([plog, np.full(PUN - t % PUN, plog[t - 1], dtype=F)])
            pmax = pl.max() if len(pl) else NEG
            f = np.exp((pl - pmax).astype(F)).astype(F)
            psum = _block_sum32(f)
            st[r, 2:] = (pmax, psum, prob)
            p[r, :V] = (pv * F(F(1) - prob)).astype(F)
            ph = 1 if defect == "ptr_allowed_phase_off_by_one" else 0
            for j in range(t + 1):
                if not ptr_allowed(t + ph, j):
                    p[r, V + j] = F(C6) * prob if defect == "fill_before_gating" else F(C6)
                elif j < t:
                    p[r, V + j] = F(F(np.exp(F(plog[j] - pmax)) / psum) * prob)
                else:
                    p[r, V + j] = 0
    return dict(p=p, stats=st, cache=cache)


def dist_judge(c, t_, got_p, got_stats, got_cache, ref, cpu):
    """Tier 1 and 2 on p and on the statistics; the written set, the exact values (0, the 1e-6 fill, vmax, the -inf / 0 statistics of an
    un-gated step) and the stored cache row bit for bit.  got_p: float32 with NaN where the guard pattern stayed."""
    name, V = c["name"], c["V"]
    got_p, got_stats = np.asarray(got_p, dtype=np.float64), np.asarray(got_stats, dtype=np.float64)
    wr, wr_ref = ~np.isnan(got_p), ~np.isnan(ref["p"])
    if not np.array_equal(wr, wr_ref):
        bad = np.argwhere(wr != wr_ref)[0]
        raise AssertionError(f"{name}: exact: the set of candidates written differs, first at row {int(bad[0])} index {int(bad[1])} "
                             f"({'written' if wr[tuple(bad)] else 'not written'}; V = {V}, t = {c['t']})")
    m = wr_ref

    def where(idx):
        i = int(np.flatnonzero(m.reshape(-1))[idx[0]])
        r, k = divmod(i, m.shape[1])
        return f"row {r}, " + (f"vocab entry {k}" if k < V else f"pointer {k - V} of step {c['t']}")
    r1 = check(name, "dist", "p", got_p[m], ref["p"][m], ref["E"][m], "f32", None if cpu is None else np.asarray(cpu["p"], dtype=np.float64)[m], where)
    exact = m & (ref["E"] == 0)
    same_bits(name, "the exact candidates (0 and the 1e-6 fill)", got_p[exact].astype(np.float32), ref["p"][exact].astype(np.float32))
    fin = np.isfinite(ref["stats"]) & (ref["Es"] > 0)
    r2 = check(name, "dist", "stats", got_stats[fin], ref["stats"][fin], ref["Es"][fin], "f32", None if cpu is None else np.asarray(cpu["stats"], dtype=np.float64)[fin])
    ex = ~fin
    same_bits(name, "vmax and the statistics of an un-gated step", got_stats[ex].astype(np.float32), ref["stats"][ex].astype(np.float32))
    want = t_.cache0.numpy().copy()
    want[c["t"]] = t_.h.numpy()
    same_bits(name, "hidden cache after the launch (row t = h, nothing else)", got_cache, want)
    return max(r1[0], r2[0]), (None if cpu is None else max(r1[1], r2[1]))


# ================================================================================================ the copies: exact
def embed_cases():
    cs = []
    for i, (dt, lp) in enumerate((("f32", 0), ("bf16", 0), ("f32", 1))):
        for d, B in ((48, 3), (512, 3), (64, 2)):
            for dof, Tmax in ((6, 20), (7, 16)):
                for t in (0, 1, dof - 1, dof, dof + 1, 2 * dof, Tmax - 1):
                    c = dict(kernel="embed", name=f"embed_{TNAME[dt]}{'_lp' if lp else ''}_d{d}_dof{dof}_t{t}", dt=dt, lp=lp, d=d, B=B, dof=dof, Tmax=Tmax, t=t, nval=11)
                    c["edge"] = dict(zeros=t == 0, coord_row=(t - 1) % dof if t else None, pos_row=(t - 1) // dof if t else None, lp=bool(lp),
                                     grid=_cdiv(B * d // 4, 256))
                    cs.append(c)
    return cs


class EmbedTensors:
    def __init__(self, c):
        gen = torch.Generator().manual_seed(seed_of(c["name"]))
        d, npos = c["d"], _cdiv(c["Tmax"], c["dof"])
        self.value, self.coord, self.pos = (torch.randn(n, d, generator=gen) * s for n, s in ((c["nval"], 1.0), (c["dof"], 3.0), (npos, 0.1)))
        self.tokens = torch.randint(0, c["nval"], (c["B"], c["Tmax"]), generator=gen)       # (every position a valid token: a wrong read shows as wrong values)
        for b in range(c["B"]):                                     # neighbours of t - 1 differ from it
            for k in range(1, c["Tmax"]):
                if self.tokens[b, k] == self.tokens[b, k - 1]:
                    self.tokens[b, k] = (self.tokens[b, k] + 1 + b) % c["nval"]


def embed_want(c, t_, defect=None):
    """(x as stored, x_lp or None): float32 (value + coord) + pos, all zeros at t = 0; the bf16 forms one RNE of that."""
    t, dof = c["t"], c["dof"]
    if t == 0:
        acc = torch.zeros(c["B"], c["d"])
    else:
        tc = t if defect == "t_mod_dof_for_t_minus_1" else t - 1
        acc = (t_.value[t_.tokens[:, t - 1]] + t_.coord[tc % dof][None, :]) + t_.pos[(t - 1) // dof][None, :]
    x = _bf(acc) if c["dt"] == "bf16" else acc
    return x.numpy(), (_bf(acc).numpy() if c["lp"] else None)


def split_cases():
    cs = []
    for dt in ("f32", "bf16"):
        for d, H in ((48, 3), (64, 2), (96, 3), (512, 8)):
            cs.append(dict(kernel="split", name=f"split_{TNAME[dt]}_dense_d{d}_H{H}", dt=dt, d=d, H=H, B=3, S=5, lens=None, edge=dict(packed=False)))
            cs.append(dict(kernel="split", name=f"split_{TNAME[dt]}_packed_d{d}_H{H}", dt=dt, d=d, H=H, B=4, S=5, lens=[3, 0, 5, 1], edge=dict(packed=True)))
    cs.append(dict(kernel="split", name="split_float_dense_grid_stride", dt="f32", d=64, H=2, B=3, S=11000, lens=None, edge=dict(packed=False)))   # > 2048 x 256 vectors
    return cs


class SplitTensors:
    def __init__(self, c):
        gen = torch.Generator().manual_seed(seed_of(c["name"]))
        lens = c["lens"]
        self.rows = sum(lens) if lens else c["B"] * c["S"]
        kv = torch.randn(self.rows, 2 * c["d"], generator=gen)
        self.kv = _bf(kv) if c["dt"] == "bf16" else kv
        self.cu = self.rowmap = None
        if lens:
            self.cu = torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int32)
            self.rowmap = torch.tensor([b * c["S"] + s for b, n in enumerate(lens) for s in range(n)], dtype=torch.int32)


def split_want(c, t_, defect=None):
    """kc, vc [B, H, S, dh] float32 by index arithmetic; positions no row maps to keep the guard pattern."""
    B, H, S, d = c["B"], c["H"], c["S"], c["d"]
    dh = d // H
    kc = np.full((B, H, S, dh), PATTERN, dtype=np.float32)
    vc = kc.copy()
    kv = t_.kv.numpy()
    rows = np.arange(t_.rows)
    if c["lens"]:
        b = t_.rowmap.numpy() // S
        s = rows - t_.cu.numpy()[b + (1 if defect == "cu_offset_of_the_wrong_element" else 0)]
    else:
        b, s = rows // S, rows % S
    ok = (s >= 0) & (s < S)                                         # (a defect's writes outside the window are dropped here)
    kc[b[ok], :, s[ok]] = kv[ok, :d].reshape(-1, H, dh)
    vc[b[ok], :, s[ok]] = kv[ok, d:].reshape(-1, H, dh)
    return kc, vc


COPY_DEFECTS = ("t_mod_dof_for_t_minus_1", "cu_offset_of_the_wrong_element")


# ================================================================================================ extents: the last element + 1 a launch may touch
def extents(c):
    k = c["kernel"]
    if k == "attn":
        H, dh, Lmax, G = c["H"], c["dh"], c["Lmax"], c["G"]
        d, B = H * dh, c["Bd"] * G
        nb = B if c["form"] == "self" else c["Bd"]
        lens = c["lens"] if c["form"] != "self" else [c["lens"][0]] * nb
        hi = max((((bk * H + H - 1) * Lmax + max(L, 1) - 1) * dh + dh) for bk, L in enumerate(lens))      # (row min(key, Lk - 1), clamped)
        ex = dict(out=B * d, q=(B - 1) * c["ldq"] + d, kc=hi, vc=hi)
        if c["form"] == "self":
            ex["newkv"] = B * 3 * d
        if c["form"] == "kpm":
            ex["kpm"] = (c["Bd"] - 1) * Lmax + c["lens"][0]
        if c["form"] == "packed":
            ex["cu"] = c["Bd"] + 1
        assert max(lens) <= Lmax
        return ex
    if k == "dist":
        rows, d, t, V, Tmax = c["rows"], c["d"], c["t"], c["V"], c["Tmax"]
        assert 0 <= t < Tmax <= MAX_T
        nch = _cdiv(d, 256) if d % 256 == 0 else 0
        assert nch * 256 == d or nch == 0                            # (the unrolled loads cover exactly d columns)
        return dict(vlog=(rows - 1) * c["ldv"] + V, pfeat=rows * d, h=rows * d, cache=(t * rows + rows - 1) * d + d, p=(rows - 1) * (V + Tmax) + V + t + 1,
                    stats=rows * 5, sw_w=d, sw_b=1)
    if k == "embed":
        t, d, dof = c["t"], c["d"], c["dof"]
        ex = dict(x=c["B"] * d, tokens=(c["B"] - 1) * c["Tmax"] + max(t, 1))
        if t:
            ex.update(value=c["nval"] * d, coord=((t - 1) % dof + 1) * d, pos=((t - 1) // dof + 1) * d)
        return ex
    if k == "split":
        n = c["B"] * c["H"] * c["S"] * (c["d"] // c["H"])
        rows = sum(c["lens"]) if c["lens"] else c["B"] * c["S"]
        return dict(kc=n, vc=n, kv=rows * 2 * c["d"])
    raise KeyError(k)


def all_cases():
    return attn_cases() + dist_cases() + embed_cases() + split_cases()
