"""Float64 parity checker for the GEMM companion kernels at the end of csrc/gemm.hip (TEST INFRASTRUCTURE; plain numpy / torch, no GPU):
pa_colsum, pa_colsum_many, pa_splitk_reduce_many, pa_transpose_many, pa_segment_tail, pa_ln_fold_weights(_f32), pa_gemm_norm_a, pa_gemm_ln.

One case table for tests/test_gemm_aux_parity_cpu.py (the checker tested on seeded defects) and tests/test_gemm_aux_float64_gpu.py (every
entry point held to it at every branch of its host code).  Guarded buffers, the guard pattern, the poison, half a bf16 ulp, the LayerNorm
forward and finisher bounds and the per-element check come from gemm_parity.py / rowops_parity.py; this file adds what is new.

A case is run in three steps that both test files share: build(c, t) lays every operand out as a window of a guarded buffer (outputs
prefilled with the pattern, accumulated outputs seeded, input padding 2^60, the gap between `cols` and `ld` inside the guarded area);
an implementation - the device, or simulate(): the float32 restatement on the CPU, with or without a seeded defect - turns the buffers
into the buffers AFTER the call; verify(c, t, G, after, env) checks every guard, every input bit for bit, and every output per ELEMENT
against float64 computed from the STORED operand values (bf16 widened exactly; a later kernel's check takes the stored outputs of the
earlier one).

dispatch(c, env) restates the host code of each entry point as a pure function of the arguments and the switches: ordered or atomic
(pa_device.h pa_ordered_reductions: dtype, bf16x3 mode, PA_DETERMINISTIC), vector or scalar pa_colsum, colsum_blocks, chunks / nbx / nby
of the LayerNorm finish, vector or scalar reduce, wide or scalar transpose per descriptor.  pa_gemm_norm_a alone has a plan call; its family
comes from pa_gemm_plan(args, ext).  A case names the `branch` it exists for and the tests assert that dispatch() puts it there.

  tier 1 (derived)   |got - ref| <= 2 e + 2^-126 (+ half a bf16 ulp at max(|ref|, |got|) for a bf16 output), u = 2^-24:
      column sums      out[n] = init[n] + sum_m X[m][n]:  e = (M + 3) u (|init| + sum_m |X|), ordered and atomic alike
      split-K reduce   out = sum_s ws[s]:  e = (splitk + 1) u sum|ws|; the sum is ordered in every branch, so it also equals the float32
                       left-to-right sum BIT FOR BIT
      LayerNorm finish out = init + sum of nparts partials met in `chunks` atomics:  e = (nparts + chunks + 1) u (|init| + sum|partial|)
      transposes       bit for bit src^T
      weight fold      Wf = the correctly rounded product W[n][k] gamma[k], bit for bit;  u[n] against sum_k Wf[n][k] of the STORED Wf:
                       e = (K + 3) u sum|Wf|;  v[n] = bias[n] + sum_k W beta:  e = (K + 3) u (|bias| + sum|W beta|)
      pa_gemm_norm_a   ref = epi(rstd (A . Wf - mean u) + v), mean / rstd the float64 statistics of the statistic source rows (zf, else A):
                       e = rstd (K + 6) u (|A| @ |Wf| + |mean| |u|) + e_mean rstd |u| + e_rstd |A . Wf - mean u| + 2 u |v|, e_mean / e_rstd the
                       LayerNorm-forward terms of rowops_parity.py.  The rows carry a common offset of four standard deviations, so
                       acc - mean u cancels most of acc: the bound follows S.  y = LayerNorm(Z): rowops' e_y.  ReLU: compared after the clamp.
      pa_gemm_ln       (a) Z against R + keep scale (A . W + bias):  e = (K + 6) u S, S = scale (|A| @ |W| + |bias|) + |R|; a dropped element is
                       exactly R (or 0);  (b) Y, mean, rstd against the float64 LayerNorm of the STORED Z with rowops' forward bound: no
                       rounding flip of z leaks into y.
  tier 2 (measured)  f32 outputs: r(x) = max |x - ref| / e;  r(got) <= FACTOR[kernel] r(cpu32), cpu32 the same operation restated in float32 on
                     the CPU.  An output that meets in float atomics has no order: its yardstick is the worst r of the restatement over the natural
                     order and ORDERS = 64 seeded permutations of the block partials, built as the kernel builds them.
"""
import ctypes as C
import contextlib

import numpy as np
import torch

import dropout_masks as dm
import rowops_parity as rp
from gemm_parity import KINDS, POISON, U24
from rowops_parity import DT, PADT, TINY, Guarded, LnFinishDesc, f64, randn, seed_of

PA_F32, PA_BF16 = 0, 1
PA_EINVAL, PA_EALIGN, PA_ESHAPE = -1, -2, -3
F32, BF16 = torch.float32, torch.bfloat16
ORDERS = 64
CS_ROWS, LN_CHUNKS = 128, 8                                         # csrc/gemm.hip
MAX_COLSUM, MAX_REDUCE, MAX_LN_FINISH = 8, 16, 4                    # include/plank_hip.h PA_MAX_*

# The tier-2 factor in force per kernel (profiles/gemm_aux_float64_parity.txt holds the measurements behind it).  16 unless a kernel that
# passes tier 1 was MEASURED above it on the hardware: then twice its worst measured value, never above 256.
KERNELS = ["colsum", "colsum_many", "reduce", "transpose", "tail_ln", "tail_colsum", "tail_reduce", "fold", "norm_a_small", "norm_a_skinny",
           "norm_a_f32", "gemm_ln"]
FACTOR = {k: 16.0 for k in KERNELS}

ENTRY_POINTS = {  # kernel group of a case (c["kernel"]) -> the entry points of include/plank_hip.h its runner calls
    "colsum": ["pa_colsum", "pa_colsum_ws_floats"], "colsum_many": ["pa_colsum_many"], "reduce": ["pa_splitk_reduce_many"],
    "transpose": ["pa_transpose_many"], "tail": ["pa_segment_tail", "pa_splitk_reduce_many"],
    "fold": ["pa_ln_fold_weights", "pa_ln_fold_weights_f32"], "norm_a": ["pa_gemm_norm_a", "pa_gemm_plan"],
    "gemm_ln": ["pa_gemm_ln", "pa_gemm", "pa_layernorm_fwd"]}
TABLE = ["pa_gemm_ln", "pa_gemm_norm_a", "pa_ln_fold_weights", "pa_ln_fold_weights_f32", "pa_colsum", "pa_colsum_many", "pa_splitk_reduce_many",
         "pa_transpose_many", "pa_segment_tail"]                    # the entry points this checker exists for


class ColsumDesc(C.Structure):                                      # include/plank_hip.h pa_colsum_desc
    _fields_ = [("X", C.c_void_p), ("out", C.c_void_p), ("M", C.c_int32), ("N", C.c_int32), ("ldx", C.c_int32), ("pad_", C.c_int32)]


class ReduceDesc(C.Structure):                                      # pa_reduce_desc
    _fields_ = [("ws", C.c_void_p), ("out", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("ld_out", C.c_int32), ("splitk", C.c_int32)]


class TrDesc(C.Structure):                                          # pa_tr_desc
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("ld_src", C.c_int32), ("ld_dst", C.c_int32),
                ("tile_begin", C.c_int32), ("pad_", C.c_int32)]


def _up(n, q):
    return -(-n // q) * q


def _eb(dt):
    return 8 if dt == "bf16" else 4


# ------------------------------------------------------------------------------------------------ the dispatch, restated
SWITCHES = ("PA_DETERMINISTIC",)
BUNDLES = {"deterministic_1": {"PA_DETERMINISTIC": "1"}, "deterministic_0": {"PA_DETERMINISTIC": "0"}}


def ordered_reductions(dt, x3, env):
    """pa_device.h pa_ordered_reductions: PA_DETERMINISTIC decides when set; else exact f32 outside the bf16x3 mode is ordered."""
    det = rp._env_int(env or {}, "PA_DETERMINISTIC")
    return (dt == "f32" and not x3) if det is None else det != 0


def colsum_blocks(M, N, eb, ordered):
    return -(-N // (4 * eb)) if ordered else -(-N // (64 * eb)) * -(-M // CS_ROWS)


def _reduce_plan(descs):
    return dict(vector=[cols % 4 == 0 for _, cols, _, _ in descs], blocks=[-(-rows * cols // 1024) for rows, cols, _, _ in descs])


def _colsum_many_plan(descs, dt, ordered):
    return dict(ordered=ordered, blocks=[colsum_blocks(M, N, _eb(dt), ordered) for M, N in descs])


def dispatch(c, env=None):
    """The host code of the entry point behind a case, restated: a pure function of the case's arguments and of the process's switches."""
    k = c["kernel"]
    if k == "colsum":
        eb, es = _eb(c["dt"]), 4 if c["dt"] == "f32" else 2
        ordered = ordered_reductions(c["dt"], c.get("x3"), env)
        lead, ldx = colsum_layout(c)
        vec = (lead * es) % 16 == 0 and ldx % eb == 0 and ldx >= _up(c["N"], eb)
        return dict(ordered=ordered, vec=vec, grid=(-(-c["N"] // (64 * eb)), 1 if ordered else -(-c["M"] // CS_ROWS)), rows_per_block=c["M"] if ordered else CS_ROWS)
    if k == "colsum_many":
        return _colsum_many_plan(c["descs"], c["dt"], ordered_reductions(c["dt"], c.get("x3"), env))
    if k == "reduce":
        return _reduce_plan(c["descs"])
    if k == "transpose":
        es, wide, tiles = 4 if c["dt"] == "f32" else 2, [], []
        for rows, cols, xs, xd, lead in c["descs"]:
            wide.append(c["dt"] == "bf16" and ((cols + xs) | (rows + xd) | cols) % 4 == 0 and (lead * es) % 8 == 0)
            tiles.append(-(-rows // 64) * -(-cols // 64))
        return dict(wide=wide, tiles=tiles, total_tiles=sum(tiles))
    if k == "tail":
        ordered = ordered_reductions(c["dt"], c.get("x3"), env)
        chunks, nbx, nby = (1 if ordered else LN_CHUNKS), -(-c["d"] // 64), (3 if any(dz for _, dz in c["ln"]) else 2)
        per = [-(-n // chunks) for n, _ in c["ln"]]
        return dict(ordered=ordered, chunks=chunks, nbx=nbx, nby=nby, ln_blocks=nbx * nby * len(c["ln"]) * chunks if c["ln"] else 0,
                    empty_chunks=[sum(ch * p >= n for ch in range(chunks)) for p, (n, _) in zip(per, c["ln"])],
                    colsum=_colsum_many_plan(c["cs"], c["dt"], ordered), reduce=_reduce_plan(c["rd"]))
    if k == "fold":
        return dict(kernel="bf16" if c["dt"] == "bf16" else "f32", strides=-(-c["K"] // 256))
    if k == "norm_a":
        return dict(form=c["form"])                                 # (the family itself: pa_gemm_plan)
    if k == "gemm_ln":
        nt = c["K"] // 32
        return dict(grid=-(-c["M"] // 32), k_tiles=nt, prologue=min(3, nt), steady=max(0, nt - 3))
    raise KeyError(k)


def on_branch(c, env=None):
    got = dispatch(c, env)
    return all(got[k] == v for k, v in c["branch"].items()), got


# ------------------------------------------------------------------------------------------------ float32 restatements of the block sums
def lanes4_sum(x32):
    """float32 [N]: rows summed as colsum_block / ln_finish_block do - four row lanes (row i on lane i % 4, in sequence), (l0 + l1) + (l2 + l3)."""
    x = np.asarray(x32, dtype=np.float32)
    x = np.concatenate([x, np.zeros((-x.shape[0] % 4,) + x.shape[1:], dtype=np.float32)]).reshape(-1, 4, *x.shape[1:])
    l = np.add.accumulate(x, axis=0, dtype=np.float32)[-1]          # (accumulate adds in sequence; a trailing 0 changes nothing)
    return (l[0] + l[1]) + (l[2] + l[3])


def lanes64_sum(x32):
    """float32 [N]: colsum_block_ordered - 64 row lanes walk all rows, the lanes' sums are added in lane order from 0."""
    x = np.asarray(x32, dtype=np.float32)
    x = np.concatenate([x, np.zeros((-x.shape[0] % 64,) + x.shape[1:], dtype=np.float32)]).reshape(-1, 64, *x.shape[1:])
    l = np.add.accumulate(x, axis=0, dtype=np.float32)[-1]
    return np.add.accumulate(l, axis=0, dtype=np.float32)[-1]


def order_sums(start32, parts, seed, orders=ORDERS):
    """float32 [1 + orders][N]: the contributions `parts` [n][N] added one by one to `start32` as float atomics do - in the natural order, then
    in `orders` seeded permutations.  Every entry is a value a correct kernel may return.  One contribution or none: one entry."""
    start = np.asarray(start32, dtype=np.float32)
    parts = np.asarray(parts, dtype=np.float32).reshape(-1, start.shape[0])
    n = len(parts)
    rng = np.random.default_rng(seed)
    perms = [np.arange(n)] + ([rng.permutation(n) for _ in range(orders)] if n > 1 else [])
    out = []
    for p in perms:
        out.append(np.add.accumulate(np.concatenate([start[None], parts[p]]), axis=0, dtype=np.float32)[-1])
    return np.stack(out)


def colsum32(x32, init32, ordered, many, seed, defect=None):
    """What pa_colsum / pa_colsum_many leave in `out` (float32 [1 + orders][N]): the block partials as the kernels form them, met in `out`."""
    x = np.asarray(x32, dtype=np.float32)
    M = x.shape[0]
    if ordered and many:
        return (np.asarray(init32, dtype=np.float32) + lanes64_sum(x))[None]
    rpb = M if ordered else CS_ROWS
    starts = list(range(0, M, rpb))
    if defect == "last_row_block_dropped" and M % rpb and M > rpb:
        starts = starts[:-1]                                        # the last, partial block of rows never arrives
    parts = [lanes4_sum(x[r0:r0 + rpb]) for r0 in starts]
    return order_sums(init32, np.stack(parts) if parts else np.zeros((0, x.shape[1]), dtype=np.float32), seed)


# ------------------------------------------------------------------------------------------------ the checks
class Checked:
    """The checks of one case: per output tier 1 (rowops_parity.check), then tier 2 against the float32 restatement(s); the worst r(got) /
    r(cpu32) per kernel for the report."""

    def __init__(self, c):
        self.c, self.fig = c, {}

    def __call__(self, kernel, what, got, ref, e, out_dt="f32", cpu=None, zero=None, where=None):
        name = self.c["name"]
        got, ref, e = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(e, dtype=np.float64)
        try:
            r, _ = rp.check(name, what, kernel, got, ref, e, out_dt, None, zero)
        except AssertionError as err:
            raise AssertionError(f"{err}{self._where(where, got, ref, e)}") from None
        r_cpu = None
        if cpu is not None:
            cands = cpu if isinstance(cpu, (list, tuple)) or (isinstance(cpu, np.ndarray) and cpu.ndim == ref.ndim + 1) else [cpu]
            eu = e + 0.5 * TINY
            r_cpu = max(rp.ratio(np.asarray(x, dtype=np.float64), ref, eu) for x in cands)
            if out_dt == "f32" and not r <= FACTOR[kernel] * r_cpu:
                raise AssertionError(f"{name}: {what} [{kernel}]: tier 2: r(got) = {r:.4g} > {FACTOR[kernel]:g} x r_cpu = {FACTOR[kernel]:g} x {r_cpu:.4g}"
                                     f"{self._where(where, got, ref, e)}")
        if out_dt == "f32":
            f = self.fig.get(kernel) or [0.0, 0.0]
            self.fig[kernel] = [max(f[0], r), max(f[1], r_cpu or 0.0)]
        else:
            self.fig.setdefault(kernel, None)
        return r, r_cpu

    @staticmethod
    def _where(where, got, ref, e):
        if where is None:
            return ""
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(got - ref) / np.maximum(e, 1e-300)
        rel = np.where(np.isfinite(rel), rel, np.inf)
        return "; worst element: " + where(tuple(int(i) for i in np.unravel_index(int(np.argmax(rel)), rel.shape)))

    def exact(self, kernel, what, got, want):
        got, want = torch.as_tensor(got), torch.as_tensor(want)
        assert got.shape == want.shape, (self.c["name"], what, got.shape, want.shape)
        self.fig.setdefault(kernel, None)
        if not torch.equal(got, want):
            bad = torch.nonzero(got != want)
            idx = tuple(int(i) for i in bad[0])
            raise AssertionError(f"{self.c['name']}: {what} [{kernel}]: {len(bad)} of {got.numel()} element(s) differ bit for bit, first at {idx}, tile "
                                 f"{tuple(i // 64 for i in idx)} of 64: got {got[idx].item()!r}, want {want[idx].item()!r}")

    def rows(self, dt):
        return [(k, dt) + ((None, None) if f is None else (f[0], f[1])) for k, f in self.fig.items()]


def bits(x):
    x = x.contiguous()
    return x.view({2: torch.int16, 4: torch.int32}[x.element_size()])


def check_guards(c, G, after):
    for key, g in G.items():
        g.check(after[key], f"{c['name']}: {key}")


def win(G, after, key):
    return G[key].view(after[key])


def _out(shape, dtype, init=None, **kw):
    g = Guarded(shape=shape, dtype=dtype, out=True, **kw)
    if init is not None:
        g.view().copy_(init.reshape(g.rows, g.cols))
    return g


def _clone(G):
    return {k: g.buf.clone() for k, g in G.items()}


def _put(G, after, key, values):
    win(G, after, key).copy_(torch.as_tensor(np.ascontiguousarray(values)).reshape(G[key].rows, G[key].cols))


# ================================================================================================ pa_colsum
def colsum_layout(c):
    """(lead, ldx): pad - the round-up of N (vector path, poisoned pad columns inside the last vector); odd - an odd ldx (scalar path);
    off - X one element off its 16-byte boundary (scalar path)."""
    N, eb = c["N"], _eb(c["dt"])
    return {"pad": (0, _up(N, eb)), "odd": (0, N if N % 2 else N + 1), "off": (1, _up(N, eb))}[c["lay"]]


def _colsum_case(dt, M, N, lay, acc, x3=0):
    return dict(kernel="colsum", name=f"colsum_{dt}_{M}x{N}_{lay}_acc{acc}" + ("_x3" if x3 else ""), dt=dt, M=M, N=N, lay=lay, acc=acc, x3=x3,
                branch=dict(vec=lay == "pad", ordered=dt == "f32" and not x3))


def colsum_cases():
    cs = []
    for i, M in enumerate([1, 3, 127, 128, 129, 300]):
        for j, N in enumerate([1, 7, 8, 260, 516]):
            k = 5 * i + j                                           # k % 6 walks every (dtype, layout); acc flips every six cases
            cs.append(_colsum_case(("f32", "bf16")[k % 2], M, N, ("pad", "odd", "off")[k % 3], (k // 6) % 2))
    # several row blocks AND several column blocks (64 x EB columns, 128 rows) on the vector path, both dtypes, both accumulate settings
    cs += [_colsum_case("bf16", 300, 516, "pad", 1), _colsum_case("bf16", 129, 516, "pad", 0), _colsum_case("f32", 300, 516, "pad", 0),
           _colsum_case("f32", 129, 260, "pad", 1)]
    # the f32 atomic form, as the bf16x3 step runs it
    cs += [_colsum_case("f32", 300, 516, "pad", 0, x3=1), _colsum_case("f32", 129, 260, "pad", 1, x3=1), _colsum_case("f32", 129, 7, "odd", 1, x3=1)]
    return cs


def colsum_inputs(c):
    s = seed_of(c["name"])
    return dict(X=randn((c["M"], c["N"]), s + 1, DT[c["dt"]]), init=randn((c["N"],), s + 2, shift=0.5))


def colsum_build(c, t):
    lead, ldx = colsum_layout(c)
    return dict(X=Guarded(t["X"], ld=ldx, lead=lead), out=_out((c["N"],), F32, init=t["init"]))


def _colsum_ref(X, init):
    x, i0 = f64(X), f64(init)
    return i0 + x.sum(0), (x.shape[0] + 3) * U24 * (np.abs(i0) + np.abs(x).sum(0))


def colsum_simulate(c, t, G, defect=None, env=None):
    after, plan = _clone(G), dispatch(c, env)
    init = t["init"].numpy() if (c["acc"] or defect == "keeps_init") else np.zeros(c["N"], dtype=np.float32)
    out = colsum32(t["X"].float().numpy(), init, plan["ordered"], False, seed_of(c["name"]), defect)[0].copy()
    if defect == "pad_column_added":                                # the poisoned element behind every row's end goes into column N - 1
        out[-1] = np.float32(out[-1] + np.float32(POISON) * c["M"])
    _put(G, after, "out", out)
    return after


def colsum_verify(c, t, G, after, env=None):
    check_guards(c, G, after)
    ck, plan = Checked(c), dispatch(c, env)
    init = t["init"] if c["acc"] else torch.zeros(c["N"])           # accumulate = 0: the seeded init must be gone
    ref, e = _colsum_ref(t["X"], init)
    cpu = colsum32(t["X"].float().numpy(), init.numpy(), plan["ordered"], False, seed_of(c["name"]))
    eb = _eb(c["dt"])
    ck("colsum", "out", f64(win(G, after, "out")).reshape(-1), ref, e, cpu=cpu,
       where=lambda i: f"column {i[0]}, column block {i[0] // (64 * eb)} of {64 * eb}, {-(-c['M'] // plan['rows_per_block'])} row block(s) of {plan['rows_per_block']}")
    return ck.rows(c["dt"])


# ================================================================================================ pa_colsum_many
MANY8 = [(1, 4), (63, 20), (64, 36), (65, 520), (200, 4), (129, 36), (300, 520), (200, 20)]


def _many_case(dt, descs, x3=0):
    return dict(kernel="colsum_many", name=f"colsum_many_{dt}_{len(descs)}desc" + ("_x3" if x3 else ""), dt=dt, descs=descs, x3=x3,
                branch=dict(ordered=dt == "f32" and not x3))


def colsum_many_cases():
    cs = []
    for dt in ("f32", "bf16"):
        cs += [_many_case(dt, [(300, 520)] if dt == "bf16" else [(65, 20)]), _many_case(dt, [(1, 4), (129, 36), (300, 520)]), _many_case(dt, MANY8)]
    cs += [_many_case("f32", [(1, 4), (129, 36), (300, 520)], x3=1), _many_case("f32", MANY8, x3=1)]
    return cs


def _many_ldx(i, N, dt):
    return _up(N, _eb(dt)) + (_eb(dt) if i % 2 else 0)              # every other descriptor: one more (poisoned) vector per row


def many_inputs(descs, dt, s):
    return dict(X=[randn((M, N), s + 10 * i + 1, DT[dt]) for i, (M, N) in enumerate(descs)],
                init=[randn((N,), s + 10 * i + 2, shift=0.5) for i, (M, N) in enumerate(descs)])


def colsum_many_inputs(c):
    return many_inputs(c["descs"], c["dt"], seed_of(c["name"]))


def many_build(descs, dt, t, pre=""):
    G = {}
    for i, (M, N) in enumerate(descs):
        G[f"{pre}X{i}"], G[f"{pre}out{i}"] = Guarded(t["X"][i], ld=_many_ldx(i, N, dt)), _out((N,), F32, init=t["init"][i])
    return G


def colsum_many_build(c, t):
    return many_build(c["descs"], c["dt"], t)


def many_simulate(c, descs, t, G, after, ordered, defect=None, pre=""):
    for i, (M, N) in enumerate(descs):
        out = colsum32(t["X"][i].float().numpy(), t["init"][i].numpy(), ordered, True, seed_of(c["name"], i), defect)[0].copy()
        if defect == "pad_column_added":
            out[-1] = np.float32(out[-1] + np.float32(POISON) * M)
        _put(G, after, f"{pre}out{i}", out)


def many_verify(c, ck, kernel, descs, t, G, after, ordered, pre=""):
    eb = _eb(c["dt"])
    for i, (M, N) in enumerate(descs):
        ref, e = _colsum_ref(t["X"][i], t["init"][i])
        cpu = colsum32(t["X"][i].float().numpy(), t["init"][i].numpy(), ordered, True, seed_of(c["name"], i))
        cb = 4 * eb if ordered else 64 * eb
        ck(kernel, f"descriptor {i} ({M} x {N}) out", f64(win(G, after, f"{pre}out{i}")).reshape(-1), ref, e, cpu=cpu,
           where=lambda j, cb=cb, M=M: f"column {j[0]}, column block {j[0] // cb} of {cb}" + ("" if ordered else f", {-(-M // CS_ROWS)} row block(s) of {CS_ROWS}"))


def colsum_many_simulate(c, t, G, defect=None, env=None):
    after = _clone(G)
    many_simulate(c, c["descs"], t, G, after, dispatch(c, env)["ordered"], defect)
    return after


def colsum_many_verify(c, t, G, after, env=None):
    check_guards(c, G, after)
    ck = Checked(c)
    many_verify(c, ck, "colsum_many", c["descs"], t, G, after, dispatch(c, env)["ordered"])
    return ck.rows(c["dt"])


# ================================================================================================ pa_splitk_reduce_many
RED5 = [(64, 36, 44, 1), (5, 37, 37, 3), (33, 31, 35, 8), (32, 33, 33, 3), (16, 8, 8, 8)]         # rows, cols, ld_out, splitk
# vector path with ld_out > cols; scalar: 5 x 37, 33 x 31 (1023 elements: the last thread partial), 32 x 33 (1056: a second block of 32 elements)


def reduce_cases():
    d16 = [(r, c_, ld + (4 if i >= 10 else 0), (1, 3, 8)[i % 3]) for i, (r, c_, ld, _) in enumerate((RED5 * 4)[:16])]
    return [dict(kernel="reduce", name=f"reduce_{len(d)}desc", descs=d, branch=dict(vector=[q[1] % 4 == 0 for q in d]))
            for d in ([(64, 36, 44, 3)], RED5, d16)]


def reduce_inputs_of(descs, s):
    return dict(ws=[randn((sk, rows * cols), s + 10 * i + 5) for i, (rows, cols, ld, sk) in enumerate(descs)])


def reduce_inputs(c):
    return reduce_inputs_of(c["descs"], seed_of(c["name"]))


def reduce_build_of(descs, t, pre=""):
    G = {}
    for i, (rows, cols, ld, sk) in enumerate(descs):
        G[f"{pre}ws{i}"], G[f"{pre}red{i}"] = Guarded(t["ws"][i]), _out((rows, cols), F32, ld=ld)
    return G


def reduce_build(c, t):
    return reduce_build_of(c["descs"], t)


def reduce32(ws, skip=None):
    """float32 left-to-right sum of the slabs from 0 (the order of both branches of reduce_block)."""
    x = ws.numpy()
    if skip is not None:
        x = np.delete(x, skip, axis=0)
    return np.add.accumulate(np.concatenate([np.zeros((1, x.shape[1]), dtype=np.float32), x]), axis=0, dtype=np.float32)[-1]


def reduce_simulate_of(descs, t, G, after, defect=None, pre=""):
    for i, (rows, cols, ld, sk) in enumerate(descs):
        v = reduce32(t["ws"][i], skip=1 if (defect == "slab_skipped" and sk > 1) else None)
        if defect == "cols_as_ld" and ld > cols:                    # rows written `cols` apart: behind row 0 they land beside their place
            torch.as_strided(after[f"{pre}red{i}"], (rows, cols), (cols, 1), G[f"{pre}red{i}"].off).copy_(torch.from_numpy(v).reshape(rows, cols))
        else:
            _put(G, after, f"{pre}red{i}", v)


def reduce_verify_of(c, ck, kernel, descs, t, G, after, pre=""):
    for i, (rows, cols, ld, sk) in enumerate(descs):
        ws = f64(t["ws"][i])
        got = win(G, after, f"{pre}red{i}")
        what = f"descriptor {i} ({rows} x {cols}, ld {ld}, {sk} slab(s)) out"
        ck(kernel, what, f64(got), ws.sum(0).reshape(rows, cols), ((sk + 1) * U24 * np.abs(ws).sum(0)).reshape(rows, cols), cpu=reduce32(t["ws"][i]).reshape(rows, cols),
           where=lambda j, cols=cols: f"(m, n) = {j}, element {j[0] * cols + j[1]}, block {(j[0] * cols + j[1]) // 1024} of 1024")
        ck.exact(kernel, what + " against the float32 left-to-right sum", bits(got), bits(torch.from_numpy(reduce32(t["ws"][i])).reshape(rows, cols)))


def reduce_simulate(c, t, G, defect=None, env=None):
    after = _clone(G)
    reduce_simulate_of(c["descs"], t, G, after, defect)
    return after


def reduce_verify(c, t, G, after, env=None):
    check_guards(c, G, after)
    ck = Checked(c)
    reduce_verify_of(c, ck, "reduce", c["descs"], t, G, after)
    return ck.rows("f32")


# ================================================================================================ pa_transpose_many
# rows, cols, ld_src - cols, ld_dst - rows, destination lead (elements).  bf16 wide path: ld_src, ld_dst and cols multiples of 4, both ends 8-byte aligned.
TR = [(1, 1, 0, 0, 0), (64, 64, 0, 0, 0), (65, 63, 1, 3, 0), (130, 72, 8, 6, 0), (30, 18, 2, 2, 0), (130, 72, 8, 6, 4), (130, 72, 8, 6, 1), (64, 64, 4, 4, 4)]
TR_WIDE = [False, True, False, True, False, True, False, True]


def transpose_cases():
    return [dict(kernel="transpose", name=f"transpose_{dt}_{len(TR)}desc", dt=dt, descs=TR, branch=dict(wide=TR_WIDE if dt == "bf16" else [False] * len(TR)))
            for dt in ("bf16", "f32")]


def transpose_inputs(c):
    s = seed_of(c["name"])
    return dict(src=[randn((rows, cols), s + i, DT[c["dt"]]) for i, (rows, cols, *_) in enumerate(c["descs"])])


def transpose_build(c, t):
    G = {}
    for i, (rows, cols, xs, xd, lead) in enumerate(c["descs"]):
        G[f"src{i}"], G[f"dst{i}"] = Guarded(t["src"][i], ld=cols + xs), _out((cols, rows), DT[c["dt"]], ld=rows + xd, lead=lead)
    return G


def transpose_simulate(c, t, G, defect=None, env=None):
    after = _clone(G)
    for i, (rows, cols, xs, xd, lead) in enumerate(c["descs"]):
        d = t["src"][i].t().clone()
        last = defect and i == 3                                    # 130 x 72: edge tiles in both directions
        if last and defect == "edge_swapped":
            d[cols - 1, rows - 1], d[cols - 1, rows - 2] = d[cols - 1, rows - 2].clone(), d[cols - 1, rows - 1].clone()
        win(G, after, f"dst{i}").copy_(d)
        if last and defect == "one_past_the_block":
            after[f"dst{i}"][G[f"dst{i}"].off + (cols - 1) * (rows + xd) + rows] = d[cols - 1, rows - 1]
    return after


def transpose_verify(c, t, G, after, env=None):
    check_guards(c, G, after)
    ck = Checked(c)
    for i, (rows, cols, *_) in enumerate(c["descs"]):
        ck.exact("transpose", f"descriptor {i} ({rows} x {cols}) dst", bits(win(G, after, f"dst{i}")), bits(t["src"][i].t()))
    return ck.rows(c["dt"])


# ================================================================================================ pa_segment_tail
TAIL_CS = [(129, 36), (300, 520), (1, 4)]
TAIL_RD = [(64, 36, 44, 3), (33, 31, 35, 8), (32, 33, 33, 1)]


def _tail_case(dt, what, d, ln, cs, rd, x3=0):
    ordered = dt == "f32" and not x3
    return dict(kernel="tail", name=f"tail_{dt}_{what}_d{d}" + ("_x3" if x3 else ""), dt=dt, d=d, ln=ln, cs=cs, rd=rd, x3=x3,
                branch=dict(ordered=ordered, chunks=1 if ordered else 8, nbx=-(-d // 64), nby=3 if any(dz for _, dz in ln) else 2))


def tail_cases():
    cs = []
    for dt in ("f32", "bf16"):
        cs += [_tail_case(dt, "ln", 64, [(1, 1), (3, 0), (8, 1), (9, 1)], [], []),                 # 9 partials in 8 chunks of 2: chunks 5 .. 7 are empty
               _tail_case(dt, "ln_no_dzsum", 96, [(37, 0), (9, 0)], [], []),                       # nby = 2; a partial last column block
               _tail_case(dt, "colsum", 64, [], TAIL_CS, []), _tail_case(dt, "reduce", 64, [], [], TAIL_RD),
               _tail_case(dt, "all", 512, [(37, 1), (9, 0), (3, 1)], TAIL_CS, TAIL_RD)]
    cs += [_tail_case("f32", "ln", 64, [(1, 1), (3, 0), (8, 1), (9, 1)], [], [], x3=1), _tail_case("f32", "all", 512, [(37, 1), (9, 0), (3, 1)], TAIL_CS, TAIL_RD, x3=1)]
    return cs


def tail_inputs(c):
    s, d = seed_of(c["name"]), c["d"]
    t = dict(partial=[randn((n, 3 * d), s + 100 * i + 50) for i, (n, _) in enumerate(c["ln"])],
             ln_init=[[randn((d,), s + 100 * i + 60 + q, shift=0.5) for q in range(3)] for i in range(len(c["ln"]))])
    t.update(many_inputs(c["cs"], c["dt"], s))
    t.update(reduce_inputs_of(c["rd"], s))
    return t


def tail_build(c, t):
    G = {}
    for i, (n, dz) in enumerate(c["ln"]):
        G[f"partial{i}"] = Guarded(t["partial"][i])
        for q in range(3):                                          # (q = 2 without dzsum: the call is handed NULL, the buffer must keep its seeded values)
            G[f"ln{i}_{q}"] = _out((c["d"],), F32, init=t["ln_init"][i][q])
    G.update(many_build(c["cs"], c["dt"], t))
    G.update(reduce_build_of(c["rd"], t))
    G.update(reduce_build_of(c["rd"], t, pre="alone_"))            # the same slabs through pa_splitk_reduce_many: the tail's bits must equal these
    return G


def ln_finish32(partial, q, d, nparts, init32, chunks, seed, defect=None):
    p = partial.numpy().reshape(nparts, 3, d)[:, q]
    per = -(-nparts // chunks)
    parts = [lanes4_sum(p[ch * per:min(nparts, (ch + 1) * per)]) for ch in range(chunks) if ch * per < nparts]
    if defect == "last_chunk_dropped" and len(parts) > 1:
        parts = parts[:-1]
    return order_sums(init32, np.stack(parts), seed)


def tail_simulate(c, t, G, defect=None, env=None):
    after, plan = _clone(G), dispatch(c, env)
    for i, (n, dz) in enumerate(c["ln"]):
        for q in range(3 if dz else 2):
            src = 2 if (defect == "dzsum_into_dbeta" and q == 1 and dz) else q
            _put(G, after, f"ln{i}_{q}", ln_finish32(t["partial"][i], src, c["d"], n, t["ln_init"][i][q].numpy(), plan["chunks"], seed_of(c["name"], 3 * i + q), defect)[0])
    many_simulate(c, c["cs"], t, G, after, plan["ordered"], defect)
    for pre in ("", "alone_"):
        reduce_simulate_of(c["rd"], t, G, after, defect if pre == "" else None, pre)
    return after


def tail_verify(c, t, G, after, env=None):
    check_guards(c, G, after)
    ck, plan, d = Checked(c), dispatch(c, env), c["d"]
    for i, (n, dz) in enumerate(c["ln"]):
        p = f64(t["partial"][i]).reshape(n, 3, d)
        for q, what in enumerate(("dgamma", "dbeta", "dzsum")):
            got, i0 = win(G, after, f"ln{i}_{q}").reshape(-1), t["ln_init"][i][q]
            if q == 2 and not dz:
                ck.exact("tail_ln", f"LayerNorm {i}: the buffer behind a NULL dzsum", bits(got), bits(i0))
                continue
            cpu = ln_finish32(t["partial"][i], q, d, n, i0.numpy(), plan["chunks"], seed_of(c["name"], 3 * i + q))
            ck("tail_ln", f"LayerNorm {i} ({n} partials) {what}", f64(got), f64(i0) + p[:, q].sum(0), (n + plan["chunks"] + 1) * U24 * (np.abs(f64(i0)) + np.abs(p[:, q]).sum(0)),
               cpu=cpu, where=lambda j: f"column {j[0]}, column block {j[0] // 64} of 64, {plan['chunks']} chunk(s) of {-(-n // plan['chunks'])} partial(s)")
    many_verify(c, ck, "tail_colsum", c["cs"], t, G, after, plan["ordered"])
    reduce_verify_of(c, ck, "tail_reduce", c["rd"], t, G, after)
    for i in range(len(c["rd"])):
        ck.exact("tail_reduce", f"reduce descriptor {i}: pa_segment_tail against pa_splitk_reduce_many", bits(win(G, after, f"red{i}")), bits(win(G, after, f"alone_red{i}")))
    return ck.rows(c["dt"])


# ================================================================================================ pa_ln_fold_weights(_f32)
def fold_cases():
    cs = []
    for i, N in enumerate([1, 32, 96]):
        for j, K in enumerate([64, 200, 256, 512, 520]):
            for dt in ("bf16", "f32"):
                bias = (i + j + (dt == "f32")) % 2
                cs.append(dict(kernel="fold", name=f"fold_{dt}_{N}x{K}_bias{bias}", dt=dt, N=N, K=K, bias=bias, branch=dict(kernel=dt, strides=-(-K // 256))))
    return cs


def fold_inputs(c):
    s, N, K = seed_of(c["name"]), c["N"], c["K"]
    return dict(W=randn((N, K), s + 1, scale=K ** -0.5), gamma=randn((K,), s + 2, scale=0.5, shift=1.0), beta=randn((K,), s + 3),
                bias=randn((N,), s + 4) if c["bias"] else None)


def fold_build(c, t):
    G = dict(W=Guarded(t["W"]), gamma=Guarded(t["gamma"]), beta=Guarded(t["beta"]), Wf=_out((c["N"], c["K"]), DT[c["dt"]]),
             u=_out((c["N"],), F32), v=_out((c["N"],), F32))
    if c["bias"]:
        G["bias"] = Guarded(t["bias"])
    return G


def fold_sum32(x32):
    """float32 [N]: the row sums of x [N][K] as ln_fold_weights_kernel forms them - thread t adds k = t, t + 256, ... in sequence, wave_sum
    (lanes i and i ^ 32, then 16, ... 1), (w0 + w1) + (w2 + w3)."""
    x = np.asarray(x32, dtype=np.float32)
    x = np.concatenate([x, np.zeros((x.shape[0], -x.shape[1] % 256), dtype=np.float32)], axis=1).reshape(x.shape[0], -1, 256)
    l = np.add.accumulate(x, axis=1, dtype=np.float32)[:, -1].reshape(-1, 4, 64)
    while l.shape[2] > 1:
        h = l.shape[2] // 2
        l = l[:, :, :h] + l[:, :, h:]
    return (l[:, 0, 0] + l[:, 1, 0]) + (l[:, 2, 0] + l[:, 3, 0])


def fold32(W, gamma, beta, bias, dt, defect=None):
    """The float32 restatement of the fold: (Wf as stored, u, v)."""
    prod = W * gamma
    wf = prod.to(DT[dt])
    if defect == "wf_truncated" and dt == "bf16":
        wf = (prod.view(torch.int32) & -65536).view(F32).to(BF16)  # the low 16 bits cut off, not rounded
    u = fold_sum32((prod if defect == "u_unrounded" else wf.float()).numpy())
    v = fold_sum32((W * beta).numpy())
    if bias is not None and defect != "v_without_bias":
        v = bias.numpy() + v
    return wf, u, v


def fold_simulate(c, t, G, defect=None, env=None):
    after = _clone(G)
    wf, u, v = fold32(t["W"], t["gamma"], t["beta"], t["bias"], c["dt"], defect)
    win(G, after, "Wf").copy_(wf)
    _put(G, after, "u", u)
    _put(G, after, "v", v)
    return after


def fold_verify(c, t, G, after, env=None):
    check_guards(c, G, after)
    ck, K = Checked(c), c["K"]
    wf_got = win(G, after, "Wf")
    wf32, u32, v32 = fold32(t["W"], t["gamma"], t["beta"], t["bias"], c["dt"])
    ck.exact("fold", "Wf against the correctly rounded W gamma", bits(wf_got), bits(wf32))
    wf = f64(wf_got)                                                # u is held to the STORED Wf
    ck("fold", "u", f64(win(G, after, "u")).reshape(-1), wf.sum(1), (K + 3) * U24 * np.abs(wf).sum(1), cpu=fold_sum32(wf_got.float().numpy()), where=lambda i: f"n = {i[0]}")
    wb, b0 = f64(t["W"]) * f64(t["beta"]), (f64(t["bias"]) if c["bias"] else 0.0)
    ck("fold", "v", f64(win(G, after, "v")).reshape(-1), b0 + wb.sum(1), (K + 3) * U24 * (np.abs(b0) + np.abs(wb).sum(1)), cpu=v32, where=lambda i: f"n = {i[0]}")
    return ck.rows(c["dt"])


# ================================================================================================ pa_gemm_norm_a
FAMILY = {"small": "SMALL", "skinny": "SKINNY", "f32": "SKINNY"}


def _norm_case(form, M, N, K, y, relu, out_dt, eps, zf=0, y_f32=0):
    if form == "f32":
        zf, y_f32, out_dt = 1, 1, "f32"
    name = f"norm_a_{form}_{M}x{N}x{K}_y{y}" + ("_f32y" if (y and y_f32 and form != "f32") else "") + ("_zf" if (zf and form != "f32") else "") + \
           ("_relu" if relu else "") + f"_{out_dt}out_eps{eps:g}"
    return dict(kernel="norm_a", name=name, form=form, M=M, N=N, K=K, y=y, relu=relu, out_dt=out_dt, eps=eps, zf=zf, y_f32=y_f32, branch=dict(form=form))


def norm_a_cases():
    cs, k = [], 0
    for K in (64, 128, 192):
        for M in (1, 63, 64, 65, 130):
            for N in (32, 96, 160, 192):
                y = int(k % 2 == 0 and _up(N, 64) >= K)             # (y needs its columns among the column tiles)
                cs.append(_norm_case("small", M, N, K, y, (k // 2) % 2, ("bf16", "f32")[(k // 3) % 2], (1e-5, 1.0)[(k // 5) % 2]))
                k += 1
    cs.append(_norm_case("small", 513, 512, 512, 1, 0, "bf16", 1e-5))                              # the first row count past the skinny form
    cs.append(_norm_case("small", 513, 96, 512, 0, 1, "f32", 1.0))
    modes = [(1, 0, 0), (1, 1, 0), (1, 1, 1), (0, 0, 0), (0, 1, 0)]                                # (y, zf, y_f32): y bf16; zf with y bf16 / f32; no y
    k = 0
    for M in (1, 31, 33, 512):
        for N in (32, 512, 544):
            for q in range(2):
                y, zf, yf = modes[(k + q * 2) % 5]
                if N < 512 and y:
                    y, yf = 0, 0
                cs.append(_norm_case("skinny", M, N, 512, y, (k + q) % 2, ("bf16", "f32")[(k // 2 + q) % 2], (1e-5, 1.0)[(k + q) % 2], zf, yf))
            k += 1
    k = 0
    for M in (1, 33, 512):
        for N in (512, 544):
            cs.append(_norm_case("f32", M, N, 512, k % 2, (k // 2) % 2, "f32", (1.0, 1e-5)[k % 2]))
            k += 1
    names = {}
    for c in cs:                                                    # (two modes of one shape can collapse to the same case: keep one)
        names.setdefault(c["name"], c)
    return list(names.values())


def norm_a_inputs(c):
    s, M, N, K = seed_of(c["name"]), c["M"], c["N"], c["K"]
    rows = randn((M, K), s + 1, shift=4.0)                          # a common offset of four standard deviations
    W, gamma, beta, bias = randn((N, K), s + 2, scale=K ** -0.5), randn((K,), s + 3, scale=0.5, shift=1.0), randn((K,), s + 4), randn((N,), s + 5)
    wf, u, v = fold32(W, gamma, beta, bias, "f32" if c["form"] == "f32" else "bf16")
    t = dict(W=W, bias=bias, A=rows if c["form"] == "f32" else rows.to(BF16), zf=rows if c["zf"] else None, Wf=wf, u=torch.from_numpy(u), v=torch.from_numpy(v), gamma=gamma, beta=beta)
    t["src"] = t["zf"] if c["zf"] else t["A"]                       # the rows the statistics are taken from
    return t


def norm_a_build(c, t):
    M, N, K = c["M"], c["N"], c["K"]
    G = dict(A=Guarded(t["A"], ld=K + 8), Wf=Guarded(t["Wf"], ld=K + 8), u=Guarded(t["u"]), v=Guarded(t["v"]), gamma=Guarded(t["gamma"]), beta=Guarded(t["beta"]),
             C=_out((M, N), DT[c["out_dt"]], ld=N + 8))
    if c["zf"] and c["form"] != "f32":                              # (exact f32: zf IS A)
        G["zf"] = Guarded(t["zf"], ld=K + 4)
    if c["y"]:
        G["y"] = _out((M, K), F32 if c["y_f32"] else BF16, ld=K + 8)
    return G


def norm_a_args(L, c, G, ptr):
    """(pa_gemm_args, pa_gemm_norm_ext) of a case; ptr(key) -> address of the window."""
    g, x = L.GemmArgs(), L.GemmNormExt()
    g.A, g.B, g.C, g.bias = ptr("A"), ptr("Wf"), ptr("C"), ptr("v")
    g.M, g.N, g.K = c["M"], c["N"], c["K"]
    g.lda, g.ldb, g.ldc = G["A"].ld, G["Wf"].ld, G["C"].ld
    g.batch, g.a_kcontig, g.b_kcontig = 1, 1, 1
    g.in_dtype, g.out_dtype = (PA_F32 if c["form"] == "f32" else PA_BF16), PADT[c["out_dt"]]
    g.alpha, g.relu, g.aux_scale, g.splitk = 1.0, int(c["relu"]), 1.0, 1
    x.u, x.gamma, x.beta, x.eps = ptr("u"), ptr("gamma"), ptr("beta"), c["eps"]
    if c["y"]:
        x.y, x.ldy, x.y_f32 = ptr("y"), G["y"].ld, c["y_f32"]
    if c["zf"]:
        key = "A" if c["form"] == "f32" else "zf"
        x.zf, x.ldzf = ptr(key), G[key].ld
    return g, x


def fake_ptr(G):
    keys = sorted(G)
    return lambda key: 0x10000000 * (keys.index(key) + 1) + G[key].byte_offset()


def norm_a_plan(L, c, G, ptr=None):
    g, x = norm_a_args(L, c, G, ptr or fake_ptr(G))
    info = L.GemmPlanInfo()
    rc = L.lib().pa_gemm_plan(C.byref(g), C.byref(x), C.byref(info))
    return rc, (KINDS[info.kind] if rc == 0 else None), info


def _ln_case(c, K):
    return dict(d=K, eps=c["eps"])


def norm_a32(c, t, defect=None):
    """The float32 restatement: (C float32 [M][N] before the store, y float32 or None)."""
    K, N = c["K"], c["N"]
    src = t["A"] if (defect == "stats_from_bf16_rows" and c["zf"]) else t["src"]
    ln = rp.ln_fwd_cpu32(dict(d=K, eps=0.0 if defect == "rstd_without_eps" else c["eps"]), dict(z=src, gamma=t["gamma"], beta=t["beta"]))
    mu, rs = torch.from_numpy(ln["mean"])[:, None], torch.from_numpy(ln["rstd"])[:, None]
    acc = t["A"].float() @ t["Wf"].float().t()
    mu_u = mu * t["u"][None]
    if defect == "mean_u_skipped_in_a_tile":
        mu_u[:, (N - 1) // 64 * 64:] = 0.0                          # the last 64-column tile
    out = rs * (acc - mu_u) + t["v"][None]
    if c["relu"]:
        out = torch.relu(out)
    return out.numpy(), ln["y"]


def norm_a_simulate(c, t, G, defect=None, env=None):
    after = _clone(G)
    out, y = norm_a32(c, t, defect)
    win(G, after, "C").copy_(torch.from_numpy(out).to(DT[c["out_dt"]]))
    if c["y"]:
        win(G, after, "y").copy_(torch.from_numpy(y).to(G["y"].dtype))
    return after


def norm_a_verify(c, t, G, after, env=None):
    check_guards(c, G, after)
    ck, K, kern = Checked(c), c["K"], "norm_a_" + c["form"]
    ln = rp.ln_fwd_ref(_ln_case(c, K), dict(z=t["src"], gamma=t["gamma"], beta=t["beta"]))
    (mu, e_mu), (rs, e_rs) = ln["mean"], ln["rstd"]
    a, wf, u, v = f64(t["A"]), f64(t["Wf"]), f64(t["u"]), f64(t["v"])
    acc = a @ wf.T
    D = acc - mu[:, None] * u[None]
    ref = rs[:, None] * D + v[None]
    e = rs[:, None] * (K + 6) * U24 * (np.abs(a) @ np.abs(wf).T + np.abs(mu)[:, None] * np.abs(u)[None]) + (e_mu * rs)[:, None] * np.abs(u)[None] + \
        e_rs[:, None] * np.abs(D) + 2 * U24 * np.abs(v)[None]
    if c["relu"]:
        ref = np.maximum(ref, 0.0)                                  # compared after the clamp (1-Lipschitz: the bound stays absolute)
    cpu, y32 = norm_a32(c, t)
    ck(kern, "C", f64(win(G, after, "C")), ref, e, out_dt=c["out_dt"], cpu=cpu,
       where=lambda i: f"(m, n) = {i}, 64 x 64 tile ({i[0] // 64}, {i[1] // 64}), 32 x 32 tile ({i[0] // 32}, {i[1] // 32})")
    if c["y"]:
        ck(kern, "y = LayerNorm(Z)", f64(win(G, after, "y")), *ln["y"], out_dt="f32" if c["y_f32"] else "bf16", cpu=y32, where=lambda i: f"(m, k) = {i}")
    return ck.rows(("f32" if c["form"] == "f32" else "bf16") + "->" + c["out_dt"])


# ================================================================================================ pa_gemm_ln
GL_SEED = 20251


def gemm_ln_cases():
    cs, k = [], 0
    for K in (64, 128, 192, 512):                                   # 2, 4, 6 and 16 K tiles of 32 against a prologue of three tiles ahead
        for M in (1, 31, 32, 33, 77):
            R, bias, Z, stats, drop = int(k % 3 != 0), int(k % 4 != 1), int(k % 2 == 0), int(k % 5 != 2), (0.3 if (k // 2) % 2 == 0 else 0.0)
            nt = K // 32
            cs.append(dict(kernel="gemm_ln", name=f"gemm_ln_{M}x{K}_R{R}_b{bias}_Z{Z}_st{stats}_p{drop:g}", M=M, K=K, R=R, bias=bias, Z=Z, stats=stats, drop=drop, eps=1e-5,
                           branch=dict(grid=-(-M // 32), k_tiles=nt, prologue=min(3, nt), steady=max(0, nt - 3))))
            k += 1
    return cs


def gemm_ln_inputs(c):
    s, M, K = seed_of(c["name"]), c["M"], c["K"]
    return dict(A=randn((M, K), s + 1, BF16), W=randn((512, K), s + 2, BF16, scale=K ** -0.5), bias=randn((512,), s + 3) if c["bias"] else None,
                R=randn((M, 512), s + 4, BF16, shift=0.5) if c["R"] else None, gamma=randn((512,), s + 5, scale=0.5, shift=1.0), beta=randn((512,), s + 6))


def gemm_ln_build(c, t):
    M, K = c["M"], c["K"]
    G = dict(A=Guarded(t["A"], ld=K + 8), W=Guarded(t["W"], ld=K + 8), gamma=Guarded(t["gamma"]), beta=Guarded(t["beta"]),
             Z=_out((M, 512), BF16, ld=516), Y=_out((M, 512), BF16, ld=516), mean=_out((M,), F32), rstd=_out((M,), F32),
             Y2=_out((M, 512), BF16, ld=516))                       # Y of the call with Z / mean / rstd NULL as the case says
    if c["bias"]:
        G["bias"] = Guarded(t["bias"])
    if c["R"]:
        G["R"] = Guarded(t["R"], ld=516)
    if c["Z"]:
        G["Z2"] = _out((M, 512), BF16, ld=516)
    if c["stats"]:
        G["mean2"], G["rstd2"] = _out((M,), F32), _out((M,), F32)
    if c["drop"]:                                                   # pa_gemm + pa_layernorm_fwd: bit-identical where the Linear has dropout
        G.update(Z0=_out((M, 512), BF16), Y0=_out((M, 512), BF16), mean0=_out((M,), F32), rstd0=_out((M,), F32))
    return G


def gemm_ln_keep(c):
    if not c["drop"]:
        return None, 1.0
    return dm.linear_keep(GL_SEED, np.arange(c["M"]), 512, c["drop"]), dm.linear_scale(c["drop"])


def gemm_ln32(c, t, defect=None):
    M, K = c["M"], c["K"]
    a = t["A"].float()
    acc = a @ t["W"].float().t()
    if defect == "k_tile_zeroed":                                   # the second-to-last 32-wide K tile of the last 32-row block never lands
        r0, k0 = (M - 1) // 32 * 32, K - 64
        a2 = a.clone()
        a2[r0:, k0:k0 + 32] = 0.0
        acc[r0:] = (a2 @ t["W"].float().t())[r0:]
    z = acc + t["bias"][None] if c["bias"] else acc
    keep, scale = gemm_ln_keep(c)
    if keep is not None:
        kept = z * np.float32(scale)
        dropped = (t["bias"][None].expand_as(z) if (defect == "dropped_keeps_bias" and c["bias"]) else torch.zeros_like(z))
        z = torch.where(torch.from_numpy(keep), kept, dropped)
    if c["R"]:
        z = z + t["R"].float()
    zb = z.to(BF16)
    ln = rp.ln_fwd_cpu32(dict(d=512, eps=c["eps"]), dict(z=z if defect == "stats_from_unrounded_z" else zb, gamma=t["gamma"], beta=t["beta"]))
    return zb, torch.from_numpy(ln["y"]).to(BF16), torch.from_numpy(ln["mean"]), torch.from_numpy(ln["rstd"])


def gemm_ln_simulate(c, t, G, defect=None, env=None):
    after = _clone(G)
    z, y, mean, rstd = gemm_ln32(c, t, defect)
    for key, val in (("Z", z), ("Z2", z), ("Z0", z), ("Y", y), ("Y2", y), ("Y0", y), ("mean", mean), ("mean2", mean), ("mean0", mean), ("rstd", rstd),
                     ("rstd2", rstd), ("rstd0", rstd)):
        if key in G:
            win(G, after, key).copy_(val.reshape(G[key].rows, G[key].cols))
    return after


def gemm_ln_verify(c, t, G, after, env=None):
    check_guards(c, G, after)
    ck, M, K = Checked(c), c["M"], c["K"]
    a, w = f64(t["A"]), f64(t["W"])
    keep, scale = gemm_ln_keep(c)
    b0 = f64(t["bias"])[None] if c["bias"] else 0.0
    r0 = f64(t["R"]) if c["R"] else np.zeros((M, 512))
    mult = np.where(keep, scale, 0.0) if keep is not None else 1.0
    ref = r0 + mult * (a @ w.T + b0)
    S = scale * (np.abs(a) @ np.abs(w).T + np.abs(b0)) + np.abs(r0)
    zgot = win(G, after, "Z")
    where = lambda i: f"(m, n) = {i}, row block {i[0] // 32} of 32, wave {i[1] // 64} of 64 columns, {K // 32} K tile(s)"
    ck("gemm_ln", "Z", f64(zgot), ref, (K + 6) * U24 * S, out_dt="bf16", where=where)
    if keep is not None:                                            # a dropped element is exactly the stored R (or exactly 0)
        want = torch.where(torch.from_numpy(keep), zgot, t["R"] if c["R"] else torch.zeros_like(zgot))
        ck.exact("gemm_ln", "Z at the dropped elements against R", bits(zgot), bits(want))
    tz = dict(z=zgot.clone(), gamma=t["gamma"], beta=t["beta"])     # (b): everything behind z against the STORED z
    ln, cpu = rp.ln_fwd_ref(dict(d=512, eps=c["eps"]), tz), rp.ln_fwd_cpu32(dict(d=512, eps=c["eps"]), tz)
    ck("gemm_ln", "mean", f64(win(G, after, "mean")).reshape(-1), *ln["mean"], cpu=cpu["mean"], where=lambda i: f"row {i[0]}")
    ck("gemm_ln", "rstd", f64(win(G, after, "rstd")).reshape(-1), *ln["rstd"], cpu=cpu["rstd"], where=lambda i: f"row {i[0]}")
    ck("gemm_ln", "Y", f64(win(G, after, "Y")), *ln["y"], out_dt="bf16", where=where)
    ck.exact("gemm_ln", f"Y with Z {'given' if c['Z'] else 'NULL'}, mean / rstd {'given' if c['stats'] else 'NULL'} against Y of the full call",
             bits(win(G, after, "Y2")), bits(win(G, after, "Y")))
    for key in ("Z", "mean", "rstd"):
        if key + "2" in G:
            ck.exact("gemm_ln", f"{key} of the second call", bits(win(G, after, key + "2")), bits(win(G, after, key)))
        if key + "0" in G:
            ck.exact("gemm_ln", f"{key} against pa_gemm + pa_layernorm_fwd", bits(win(G, after, key + "0")), bits(win(G, after, key)))
    if "Y0" in G:
        ck.exact("gemm_ln", "Y against pa_gemm + pa_layernorm_fwd", bits(win(G, after, "Y0")), bits(win(G, after, "Y")))
    return ck.rows("bf16")


# ================================================================================================ the table
GROUPS = {  # kernel group -> (cases, inputs, build, simulate, verify)
    "colsum": (colsum_cases, colsum_inputs, colsum_build, colsum_simulate, colsum_verify),
    "colsum_many": (colsum_many_cases, colsum_many_inputs, colsum_many_build, colsum_many_simulate, colsum_many_verify),
    "reduce": (reduce_cases, reduce_inputs, reduce_build, reduce_simulate, reduce_verify),
    "transpose": (transpose_cases, transpose_inputs, transpose_build, transpose_simulate, transpose_verify),
    "tail": (tail_cases, tail_inputs, tail_build, tail_simulate, tail_verify),
    "fold": (fold_cases, fold_inputs, fold_build, fold_simulate, fold_verify),
    "norm_a": (norm_a_cases, norm_a_inputs, norm_a_build, norm_a_simulate, norm_a_verify),
    "gemm_ln": (gemm_ln_cases, gemm_ln_inputs, gemm_ln_build, gemm_ln_simulate, gemm_ln_verify),
}


def all_cases():
    cs = [c for g in GROUPS.values() for c in g[0]()]
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cs


def switch_cases(env):
    """The cases whose restated dispatch a switch setting changes (what a bundle's child process runs)."""
    return [c for c in all_cases() if not c.get("x3") and dispatch(c, env) != dispatch(c)]


# ------------------------------------------------------------------------------------------------ the bf16x3 mode around a call
@contextlib.contextmanager
def x3_mode(lib, ws_ptr, ws_bytes):
    """pa_gemm_split_config(1, ..) inside a split context of the caller's own, as the bf16x3 train step enters one around its calls; off and
    left again on the way out.  pa_gemm_split_active() is asserted on both sides."""
    ctx = C.c_void_p()
    assert lib.pa_split_ctx_create(C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.pa_split_ctx_enter(ctx) == 0
        assert lib.pa_gemm_split_active() == 0
        assert lib.pa_gemm_split_config(1, C.c_void_p(ws_ptr), C.c_int64(ws_bytes)) == 0
        assert lib.pa_gemm_split_active() == 1
        yield
    finally:
        lib.pa_gemm_split_config(0, None, 0)
        active = lib.pa_gemm_split_active()
        lib.pa_split_ctx_enter(None)
        lib.pa_split_ctx_destroy(ctx)
        assert active == 0 and lib.pa_gemm_split_active() == 0


# ------------------------------------------------------------------------------------------------ rejections (all return before any launch)
def _descs(cls, rows):
    arr = (cls * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = cls(*r)
    return arr


def rejections(L):
    """[(name, call() -> status, status wanted)]: made-up addresses with the alignment named; every call returns before a launch."""
    lib, P = L.lib(), 0x10000000
    out = []
    # ---- pa_colsum_many (f32: EB = 4)
    cm = lambda rows, dt=PA_F32: (lambda: lib.pa_colsum_many(C.cast(_descs(ColsumDesc, rows), C.c_void_p), len(rows), dt, None))
    out += [("colsum_many_9_descriptors", cm([(P, 2 * P, 5, 8, 8, 0)] * 9), PA_EINVAL),
            ("colsum_many_ldx_not_a_vector", cm([(P, 2 * P, 5, 8, 10, 0)]), PA_EALIGN),
            ("colsum_many_X_unaligned", cm([(P + 4, 2 * P, 5, 8, 8, 0)]), PA_EALIGN),
            ("colsum_many_ldx_below_round_up", cm([(P, 2 * P, 5, 20, 16, 0)], PA_BF16), PA_EALIGN)]
    # ---- pa_splitk_reduce_many
    rd = lambda rows: (lambda: lib.pa_splitk_reduce_many(C.cast(_descs(ReduceDesc, rows), C.c_void_p), len(rows), None))
    out += [("reduce_ld_out_below_cols", rd([(P, 2 * P, 8, 36, 32, 2)]), PA_EINVAL), ("reduce_ws_unaligned", rd([(P + 4, 2 * P, 8, 36, 36, 2)]), PA_EALIGN),
            ("reduce_out_unaligned", rd([(P, 2 * P + 8, 8, 36, 36, 2)]), PA_EALIGN), ("reduce_vector_cols_scalar_ld", rd([(P, 2 * P, 8, 36, 38, 2)]), PA_EALIGN),
            ("reduce_17_descriptors", rd([(P, 2 * P, 8, 36, 36, 2)] * 17), PA_EINVAL)]
    # ---- pa_segment_tail
    def tail(n_ln=0, n_cs=0, n_rd=0, dtype=PA_F32):
        ln = _descs(LnFinishDesc, [(P, 2 * P, 3 * P, None, 3, 0)] * max(n_ln, 1))
        cs = _descs(ColsumDesc, [(P, 2 * P, 5, 8, 8, 0)] * max(n_cs, 1))
        r = _descs(ReduceDesc, [(P, 2 * P, 8, 36, 36, 2)] * max(n_rd, 1))
        return lambda: lib.pa_segment_tail(C.cast(ln, C.c_void_p), n_ln, 64, C.cast(cs, C.c_void_p), n_cs, dtype, C.cast(r, C.c_void_p), n_rd, None)
    out += [("tail_all_lists_empty", tail(), PA_EINVAL), ("tail_bad_dtype", tail(1, 1, 1, dtype=2), PA_EINVAL),
            ("tail_5_layernorms", tail(n_ln=MAX_LN_FINISH + 1), PA_EINVAL), ("tail_9_colsums", tail(n_cs=MAX_COLSUM + 1), PA_EINVAL),
            ("tail_17_reduces", tail(n_rd=MAX_REDUCE + 1), PA_EINVAL)]
    # ---- pa_gemm_norm_a: from the dry run and from the real call
    def norm(c, edit=None):
        G = _norm_layout(c)

        def both():
            g, x = norm_a_args(L, c, G, fake_ptr(G))
            if edit:
                edit(g, x)
            info = L.GemmPlanInfo()
            dry = lib.pa_gemm_plan(C.byref(g), C.byref(x), C.byref(info))
            real = lib.pa_gemm_norm_a(C.byref(g), C.byref(x), None)
            assert dry == real, (c["name"], dry, real)
            return real
        return both
    def no_bias(g, x):
        g.bias = None
    def u_off(g, x):
        x.u = x.u + 4
    out += [("norm_a_zf_at_513_rows", norm(_norm_case("skinny", 513, 512, 512, 1, 0, "bf16", 1e-5, zf=1, y_f32=1)), PA_ESHAPE),
            ("norm_a_y_columns_beyond_the_tiles", norm(_norm_case("small", 64, 32, 128, 1, 0, "bf16", 1e-5)), PA_ESHAPE),
            ("norm_a_more_units_than_2_per_cu", norm(_norm_case("small", 64 * 33, 1024, 64, 0, 0, "bf16", 1e-5)), PA_ESHAPE),
            ("norm_a_N_not_a_multiple_of_32", norm(_norm_case("small", 64, 40, 64, 0, 0, "bf16", 1e-5)), PA_ESHAPE),
            ("norm_a_null_bias", norm(_norm_case("small", 64, 64, 64, 0, 0, "bf16", 1e-5), no_bias), PA_EINVAL),
            ("norm_a_u_misaligned", norm(_norm_case("small", 64, 64, 64, 0, 0, "bf16", 1e-5), u_off), PA_EALIGN)]
    # ---- pa_gemm_ln
    def gl(**kw):
        def call():
            a = L.GemmLnArgs()
            a.A, a.W, a.bias, a.R, a.Z, a.Y, a.gamma, a.beta, a.mean, a.rstd = [P * (i + 1) for i in range(10)]
            a.M, a.N, a.K, a.lda, a.ldw, a.ldr, a.ldz, a.ldy, a.eps, a.drop_p, a.drop_seed = 33, 512, 128, 136, 136, 516, 516, 516, 1e-5, 0.0, 1
            for k, v in kw.items():
                setattr(a, k, v)
            return lib.pa_gemm_ln(C.byref(a), None)
        return call
    out += [("gemm_ln_N_not_512", gl(N=256), PA_EINVAL), ("gemm_ln_K_not_a_multiple_of_64", gl(K=96), PA_EINVAL), ("gemm_ln_drop_p_1", gl(drop_p=1.0), PA_EINVAL),
            ("gemm_ln_drop_p_negative", gl(drop_p=-0.1), PA_EINVAL), ("gemm_ln_lda_not_a_multiple_of_8", gl(lda=132), PA_EALIGN),
            ("gemm_ln_R_4_bytes_off", gl(R=4 * P + 4), PA_EALIGN)]
    return out


class _Layout:
    """Strides and offsets of a Guarded window without its buffer (the dry runs need no values)."""

    def __init__(self, rows, cols, dtype, ld=None, lead=0):
        self.rows, self.cols, self.dtype, self.ld, self.off = rows, cols, dtype, ld or cols, rp.GUARD + lead

    def byte_offset(self):
        return self.off * torch.empty(0, dtype=self.dtype).element_size()


def _norm_layout(c):
    M, N, K = c["M"], c["N"], c["K"]
    idt = F32 if c["form"] == "f32" else BF16
    G = dict(A=_Layout(M, K, idt, K + 8), Wf=_Layout(N, K, idt, K + 8), u=_Layout(1, N, F32), v=_Layout(1, N, F32), gamma=_Layout(1, K, F32), beta=_Layout(1, K, F32),
             C=_Layout(M, N, DT[c["out_dt"]], N + 8))
    if c["zf"] and c["form"] != "f32":
        G["zf"] = _Layout(M, K, F32, K + 4)
    if c["y"]:
        G["y"] = _Layout(M, K, F32 if c["y_f32"] else BF16, K + 8)
    return G


def norm_a_dry_run(L, c):
    """pa_gemm_plan(args, ext) of a case on made-up addresses with the real windows' alignment: (status, family, info)."""
    return norm_a_plan(L, c, _norm_layout(c))
