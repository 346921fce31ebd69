"""Thin torch-tensor wrappers over the op-level C ABI (include/plank_hip.h).

Used by the kernel parity tests and by host code that needs a single op.  The model-level
path (plankassembly_amd.models) drives the same kernels through the C++ runtime entry points.
All tensors must live on the GPU; everything enqueues on torch's current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L


def _f32(*shape, device):
    return torch.empty(*shape, dtype=torch.float32, device=device)


def gemm(a, b, *, a_kcontig=True, b_kcontig=True, bias=None, residual=None, aux=None, aux_scale=1.0,
         relu=False, alpha=1.0, drop_p=0.0, drop_seed=0, out_dtype=None, splitk=1, out=None, defer=False, out_lp=None):
    """C[b] = epi(alpha * A[b] @ B[b]).  a: [batch?, M, K] (or [K, M] if not a_kcontig);
    b: [batch?, N, K] if b_kcontig (Linear weight layout) else [K, N]."""
    batched = a.dim() == 3
    A3 = a if batched else a[None]
    B3 = b if b.dim() == 3 else b[None]
    batch = A3.shape[0]
    M, K = (A3.shape[1], A3.shape[2]) if a_kcontig else (A3.shape[2], A3.shape[1])
    N = B3.shape[1] if b_kcontig else B3.shape[2]
    assert (B3.shape[2] if b_kcontig else B3.shape[1]) == K
    assert A3.stride(2) == 1 and B3.stride(2) == 1
    out_dtype = out_dtype or a.dtype
    if out is None:
        out = torch.empty((batch, M, N) if batched else (M, N), dtype=out_dtype, device=a.device)
    O3 = out if out.dim() == 3 else out[None]
    g = L.GemmArgs()
    g.A, g.B, g.C = a.data_ptr(), b.data_ptr(), out.data_ptr()
    g.bias = bias.data_ptr() if bias is not None else None
    g.R = residual.data_ptr() if residual is not None else None
    g.aux = aux.data_ptr() if aux is not None else None
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = A3.stride(1), B3.stride(1), O3.stride(1)
    g.ldr = (residual if residual is not None else O3).stride(-2)
    g.ldaux = aux.stride(-2) if aux is not None else 0
    g.sA = A3.stride(0) if batch > 1 else 0
    g.sB = B3.stride(0) if (b.dim() == 3 and B3.shape[0] > 1) else 0
    g.sC = O3.stride(0) if batch > 1 else 0
    g.sR = residual.stride(0) if (residual is not None and residual.dim() == 3 and batch > 1) else 0
    g.sAux = aux.stride(0) if (aux is not None and aux.dim() == 3 and batch > 1) else 0
    g.sBias = bias.stride(0) if (bias is not None and bias.dim() == 2 and batch > 1) else 0     # [batch, N]: one bias per member
    g.batch = batch
    g.a_kcontig, g.b_kcontig = int(a_kcontig), int(b_kcontig)
    g.in_dtype, g.out_dtype = L.dt(a), L.dt(out)
    g.alpha, g.relu, g.aux_scale = alpha, int(relu), aux_scale
    g.drop_p, g.drop_seed = drop_p, drop_seed
    if out_lp is not None:                    # bf16 copy of an f32 output (skinny kernel: the f32-residual decode step's form)
        g.C_lp, g.ldc_lp = out_lp.data_ptr(), out_lp.stride(-2)
    splitk = int(L.lib().pa_gemm_effective_splitk(K, L.dt(a), splitk))       # slabs actually written
    g.splitk = splitk
    ws = None
    if splitk > 1:
        ws = _f32(splitk * batch * M * N, device=a.device)
        g.ws = ws.data_ptr()
        g.splitk_defer = int(defer)
    L.check(L.lib().pa_gemm(C.byref(g), L.stream()), "pa_gemm")
    if defer and splitk > 1:
        return out, ws, splitk  # slabs only: reduce with splitk_reduce_many([(ws, out, splitk), ...])
    return out


def dw_group(items):
    """Weight gradients dW_i = dY_i^T @ X_i for [(dY[rows, M], X[rows, N], splitk)], bf16 in / f32 out: ONE ring-kernel
    launch for all products (pa_gemm_group) plus one reduction launch for the split ones."""
    n = len(items)
    args = (L.GemmArgs * n)()
    outs, keep, red = [], [], []
    for i, (dy, x, sk) in enumerate(items):
        rows, M = dy.shape
        N = x.shape[1]
        sk = int(L.lib().pa_gemm_effective_splitk(rows, L.dt(dy), sk))
        out = torch.empty(M, N, dtype=torch.float32, device=dy.device)
        g = args[i]
        g.A, g.B, g.C = dy.data_ptr(), x.data_ptr(), out.data_ptr()
        g.M, g.N, g.K = M, N, rows
        g.lda, g.ldb, g.ldc = dy.stride(0), x.stride(0), out.stride(0)
        g.batch, g.a_kcontig, g.b_kcontig = 1, 0, 0
        g.in_dtype, g.out_dtype = L.dt(dy), L.dt(out)
        g.alpha, g.aux_scale, g.splitk = 1.0, 1.0, sk
        if sk > 1:
            ws = _f32(sk * M * N, device=dy.device)
            g.ws, g.splitk_defer = ws.data_ptr(), 1
            keep.append(ws)
            red.append((ws, out, sk))
        outs.append(out)
    L.check(L.lib().pa_gemm_group(C.cast(args, C.c_void_p), n, L.stream()), "pa_gemm_group")
    if red:
        splitk_reduce_many(red)
    return outs


class ColsumDesc(C.Structure):          # mirrors pa_colsum_desc
    _fields_ = [("X", C.c_void_p), ("out", C.c_void_p), ("M", C.c_int32), ("N", C.c_int32), ("ldx", C.c_int32),
                ("pad_", C.c_int32)]


def colsum_many(items):
    """items: [(x[M, N], out[N] f32)]: out += column sums of x, one launch for all items."""
    n = len(items)
    descs = (ColsumDesc * n)()
    for i, (x, out) in enumerate(items):
        descs[i].X, descs[i].out = x.data_ptr(), out.data_ptr()
        descs[i].M, descs[i].N, descs[i].ldx = x.shape[0], x.shape[1], x.stride(0)
    L.check(L.lib().pa_colsum_many(C.cast(descs, C.c_void_p), n, L.dt(items[0][0]), L.stream()), "pa_colsum_many")


class ReduceDesc(C.Structure):          # mirrors pa_reduce_desc
    _fields_ = [("ws", C.c_void_p), ("out", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32),
                ("ld_out", C.c_int32), ("splitk", C.c_int32)]


def splitk_reduce_many(items):
    """items: [(ws, out[rows, cols] f32, splitk)]: out = sum of the splitk slabs in ws, one launch for all items."""
    n = len(items)
    descs = (ReduceDesc * n)()
    for i, (ws, out, sk) in enumerate(items):
        descs[i].ws, descs[i].out = ws.data_ptr(), out.data_ptr()
        descs[i].rows, descs[i].cols, descs[i].ld_out, descs[i].splitk = out.shape[0], out.shape[1], out.stride(0), sk
    L.check(L.lib().pa_splitk_reduce_many(C.cast(descs, C.c_void_p), n, L.stream()), "pa_splitk_reduce_many")


def colsum(x, out=None, accumulate=False):
    M, N = x.shape
    if out is None:
        out = torch.zeros(N, dtype=torch.float32, device=x.device)
    part = _f32(int(L.lib().pa_colsum_ws_floats(M, N)), device=x.device)
    L.check(L.lib().pa_colsum(L.ptr(x), L.dt(x), M, N, x.stride(0), L.ptr(out), int(accumulate), L.ptr(part),
                              L.stream()), "pa_colsum")
    return out


def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr() if t is not None else None
    return arr


def embed_input_fwd(tables, idx, dtype=torch.float32, rowmap=None, n_rows=None):
    n_tok = n_rows if n_rows is not None else next(i for i in idx if i is not None).numel()
    d = tables[0].shape[1]
    out = torch.empty(n_tok, d, dtype=dtype, device=tables[0].device)
    L.check(L.lib().pa_embed_input_fwd(L.ptr(out), L.dt(out), _ptr_array(tables), _ptr_array(idx), L.ptr(rowmap), len(tables),
                                       C.c_int64(n_tok), d, L.stream()), "pa_embed_input_fwd")
    return out


def pack_rows(mask):
    """mask: bool/uint8 [B, S] (True = PAD).  Returns (cu int32 [B+1], rowmap int32 [n_valid], n_valid); cu is a view of
    the [2B+1] buffer whose tail holds the batch elements by descending row count (``pack_order(cu)``)."""
    B, S = mask.shape
    m8 = mask.to(torch.uint8).contiguous()
    cu = torch.empty(2 * B + 1, dtype=torch.int32, device=mask.device)
    rowmap = torch.empty(B * S, dtype=torch.int32, device=mask.device)
    L.check(L.lib().pa_pack_rows(L.ptr(m8), B, S, L.ptr(cu), L.ptr(rowmap), L.stream()), "pa_pack_rows")
    n = int(cu[B])
    return cu[: B + 1], rowmap[:n], n


def pack_order(cu):
    """The dispatch order pa_pack_rows left behind cu (int32 [B]: batch elements, longest first)."""
    base = cu._base if cu._base is not None else cu           # the [B+1] view pack_rows returns, or the whole buffer
    if base.numel() % 2 == 0:
        raise ValueError("pack_order needs the [2B+1] buffer of pa_pack_rows (or a view of it)")
    B = (base.numel() - 1) // 2
    return base[B + 1: 2 * B + 1]


def embed_input_bwd(dout, dtables, idx, rowmap=None):
    n_tok, d = dout.shape
    rows = (C.c_int32 * len(dtables))(*[t.shape[0] for t in dtables])
    L.check(L.lib().pa_embed_input_bwd(L.ptr(dout), L.dt(dout), _ptr_array(dtables), _ptr_array(idx), L.ptr(rowmap), rows,
                                       len(dtables), C.c_int64(n_tok), d, L.stream()), "pa_embed_input_bwd")


def embed_output_fwd(value, coord, pos, tok, T, dof=6, dtype=torch.float32):
    B = tok.shape[0]
    d = value.shape[1]
    out = torch.empty(B, T, d, dtype=dtype, device=value.device)
    L.check(L.lib().pa_embed_output_fwd(L.ptr(out), L.dt(out), L.ptr(value), L.ptr(coord), L.ptr(pos), L.ptr(tok),
                                        tok.stride(0), B, T, d, dof, L.stream()), "pa_embed_output_fwd")
    return out


def embed_output_bwd(dout, dvalue, dcoord, dpos, tok, dof=6):
    B, T, d = dout.shape
    L.check(L.lib().pa_embed_output_bwd(L.ptr(dout), L.dt(dout), L.ptr(dvalue), L.ptr(dcoord), L.ptr(dpos),
                                        L.ptr(tok), tok.stride(0), B, T, d, dof, L.stream()), "pa_embed_output_bwd")


def gemm_ln(x, w, gamma, beta, eps, *, bias=None, residual=None, drop_p=0.0, drop_seed=0, want_z=True):
    """z = residual + drop(x @ w.T + bias), y = LayerNorm(z) in one launch (bf16, w: [512, K]).  Returns (z | None, y, mean, rstd)
    - bit-identical to gemm(..., bias, residual, drop_p) followed by layernorm_fwd."""
    M, K = x.shape
    assert w.shape[1] == K and x.stride(1) == 1 and w.stride(1) == 1
    y = torch.empty(M, w.shape[0], dtype=x.dtype, device=x.device)
    z = torch.empty_like(y) if want_z else None
    mean, rstd = _f32(M, device=x.device), _f32(M, device=x.device)
    g = L.GemmLnArgs()
    g.A, g.W, g.Y, g.Z = x.data_ptr(), w.data_ptr(), y.data_ptr(), (z.data_ptr() if want_z else None)
    g.bias = bias.data_ptr() if bias is not None else None
    g.R = residual.data_ptr() if residual is not None else None
    g.gamma, g.beta, g.mean, g.rstd = gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    g.M, g.N, g.K = M, w.shape[0], K
    g.lda, g.ldw, g.ldy = x.stride(0), w.stride(0), y.stride(0)
    g.ldz = z.stride(0) if want_z else 0
    g.ldr = residual.stride(0) if residual is not None else 0
    g.eps, g.drop_p, g.drop_seed = eps, drop_p, drop_seed
    L.check(L.lib().pa_gemm_ln(C.byref(g), L.stream()), "pa_gemm_ln")
    return z, y, mean, rstd


def gemm_norm_a(z, w, bias, gamma, beta, eps, *, relu=False, want_y=True, out_dtype=None, zf=None):
    """epi(LayerNorm(z) @ w.T + bias) with the LayerNorm folded into the product (pa_ln_fold_weights + pa_gemm_norm_a; the
    greedy-decode step's form).  z: bf16 [M, K]; w, bias, gamma, beta: f32 master parameters.  Returns (out, y | None).
    zf: the f32 rows of which z is the bf16 copy - statistics and y (then f32) come from them (f32 residual stream)."""
    M, K = z.shape
    N = w.shape[0]
    dev = z.device
    wf = torch.empty(N, K, dtype=torch.bfloat16, device=dev)
    u, v = _f32(N, device=dev), _f32(N, device=dev)
    L.check(L.lib().pa_ln_fold_weights(L.ptr(wf), L.ptr(u), L.ptr(v), L.ptr(w), L.ptr(bias), L.ptr(gamma), L.ptr(beta), N, K,
                                       L.stream()), "pa_ln_fold_weights")
    out = torch.empty(M, N, dtype=out_dtype or z.dtype, device=dev)
    y = torch.empty(M, K, dtype=(torch.float32 if zf is not None else z.dtype), device=dev) if want_y else None
    g = L.GemmArgs()
    g.A, g.B, g.C, g.bias = z.data_ptr(), wf.data_ptr(), out.data_ptr(), v.data_ptr()
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = z.stride(0), K, N
    g.batch, g.a_kcontig, g.b_kcontig = 1, 1, 1
    g.in_dtype, g.out_dtype = L.dt(z), L.dt(out)
    g.alpha, g.relu, g.aux_scale, g.splitk = 1.0, int(relu), 1.0, 1
    x = L.GemmNormExt()
    x.u, x.gamma, x.beta = u.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    x.y, x.ldy, x.eps = (y.data_ptr() if want_y else None), K, eps
    if zf is not None:
        x.zf, x.ldzf, x.y_f32 = zf.data_ptr(), zf.stride(0), 1
    L.check(L.lib().pa_gemm_norm_a(C.byref(g), C.byref(x), L.stream()), "pa_gemm_norm_a")
    return out, y


def layernorm_fwd(z, gamma, beta, eps):
    rows, d = z.numel() // z.shape[-1], z.shape[-1]
    y = torch.empty_like(z)
    mean, rstd = _f32(rows, device=z.device), _f32(rows, device=z.device)
    L.check(L.lib().pa_layernorm_fwd(L.ptr(y), L.ptr(z), L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(rstd),
                                     C.c_int64(rows), d, C.c_float(eps), L.dt(z), L.stream()), "pa_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, z, gamma, mean, rstd, dgamma, dbeta, dzsum=None, drop_p=0.0, drop_seed=0):
    rows, d = z.numel() // z.shape[-1], z.shape[-1]
    dz = torch.empty_like(z)
    ddrop = torch.empty_like(z) if drop_p > 0 else None
    part = _f32(int(L.lib().pa_layernorm_ws_floats(rows, d)), device=z.device)
    L.check(L.lib().pa_layernorm_bwd(L.ptr(dz), L.ptr(ddrop), L.ptr(dy), L.ptr(z), L.ptr(gamma), L.ptr(mean),
                                     L.ptr(rstd), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dzsum), L.ptr(part),
                                     C.c_int64(rows), d, L.dt(z), C.c_float(drop_p), C.c_uint32(drop_seed),
                                     L.stream()), "pa_layernorm_bwd")
    return dz, ddrop


def _attn_args(q, k, v, o, lse, kpm, causal, scale, drop_p, drop_seed, H, cu_q=None, cu_k=None, B=None, Lq=None, Lk=None, order=None):
    if B is None:
        B, Lq = q.shape[0], q.shape[1]
        Lk = k.shape[1]
    dh = q.shape[-1] // H
    a = L.AttnArgs()
    a.q, a.k, a.v, a.o, a.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr()
    a.kpm = kpm.data_ptr() if kpm is not None else None
    a.B, a.H, a.Lq, a.Lk, a.dh = B, H, Lq, Lk, dh
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(-2), k.stride(-2), v.stride(-2), o.stride(-2)
    a.cu_q = cu_q.data_ptr() if cu_q is not None else None
    a.cu_k = cu_k.data_ptr() if cu_k is not None else None
    a.order = order.data_ptr() if order is not None else None        # int32 [B] dispatch order (pa_pack_rows)
    a.causal = int(causal)
    a.scale = scale if scale is not None else 1.0 / math.sqrt(dh)
    a.drop_p, a.drop_seed = drop_p, drop_seed
    a.dtype = L.dt(q)
    return a


def mask_order(kpm):
    """Dispatch order for a padded batch with a key-padding mask: int32 [B], batch elements by descending number of unmasked
    keys (what pa_pack_rows leaves behind `cu` for packed batches).  A block's duration is proportional to its element's key
    count (tiles past the last unmasked key are skipped) and the hardware hands out blocks in index order as slots free up, so
    longest-first is list scheduling's LPT rule: the launch no longer ends with a long element that started late.  Computed
    once per batch (the mask is the same for every layer, forward and backward); results do not depend on it."""
    return torch.argsort((kpm == 0).sum(dim=1), descending=True, stable=True).to(torch.int32)


def attn_fwd(q, k, v, H, kpm=None, causal=False, scale=None, drop_p=0.0, drop_seed=0, order=None):
    """q: [B, Lq, H*dh] (may be a strided view of a packed projection), k/v: [B, Lk, H*dh];
    kpm: uint8/bool [B, Lk] (1 = PAD); order: optional int32 [B] dispatch order (mask_order).
    Returns (o [B, Lq, H*dh], lse [B, H, Lq])."""
    B, Lq, dm = q.shape
    o = torch.empty(B, Lq, dm, dtype=q.dtype, device=q.device)
    lse = _f32(B, H, Lq, device=q.device)
    if kpm is not None:
        kpm = kpm.to(torch.uint8).contiguous()
    a = _attn_args(q, k, v, o, lse, kpm, causal, scale, drop_p, drop_seed, H, order=order)
    L.check(L.lib().pa_attn_fwd(C.byref(a), L.stream()), "pa_attn_fwd")
    return o, lse


def attn_bwd(dout, q, k, v, o, lse, H, kpm=None, causal=False, scale=None, drop_p=0.0, drop_seed=0, order=None):
    if kpm is not None:
        kpm = kpm.to(torch.uint8).contiguous()
    a = _attn_args(q, k, v, o, lse, kpm, causal, scale, drop_p, drop_seed, H, order=order)
    dq = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    dk = torch.empty(k.shape, dtype=k.dtype, device=k.device)
    dv = torch.empty(v.shape, dtype=v.dtype, device=v.device)
    delta = _f32(lse.shape, device=q.device)
    a.dout, a.dq, a.dk, a.dv, a.delta = dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr()
    a.lddo, a.lddq, a.lddk, a.lddv = dout.stride(1), dq.stride(1), dk.stride(1), dv.stride(1)
    L.check(L.lib().pa_attn_bwd(C.byref(a), L.stream()), "pa_attn_bwd")
    return dq, dk, dv


def pack_lengths(lengths, device):
    """int lengths [B] -> (cu int32 [B+1] on `device`, order int32 [B] = batch elements by descending length) - the
    layout pa_pack_rows leaves behind (cu[0..B], cu[B+1..2B])."""
    ln = torch.as_tensor(lengths, dtype=torch.int64)
    cu = torch.zeros(len(ln) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(ln, 0).to(torch.int32)
    order = torch.argsort(ln, descending=True, stable=True).to(torch.int32)
    return cu.to(device), order.to(device)


def switch_fwd(h, w, b):
    rows, d = h.numel() // h.shape[-1], h.shape[-1]
    s = _f32(rows, device=h.device)
    L.check(L.lib().pa_switch_fwd(L.ptr(s), L.ptr(h), L.dt(h), L.ptr(w), L.ptr(b), C.c_int64(rows), d, L.stream()),
            "pa_switch_fwd")
    return s


def switch_bwd(ds, h, w, dw, db, dh=None):
    rows, d = h.numel() // h.shape[-1], h.shape[-1]
    acc = dh is not None
    if dh is None:
        dh = torch.empty_like(h)
    # one [2][d] partial per backward block; the block height is the library's (it changed from 32 to 8 rows once
    # and a hard-coded 32 here wrote past this buffer), so ask it
    part = _f32(int(L.lib().pa_layernorm_bwd_nparts(C.c_int64(rows))) * 2 * d, device=h.device)
    L.check(L.lib().pa_switch_bwd(L.ptr(dh), int(acc), L.ptr(dw), L.ptr(db), L.ptr(ds), L.ptr(h), L.dt(h), L.ptr(w),
                                  L.ptr(part), C.c_int64(rows), d, L.stream()), "pa_switch_bwd")
    return dh


def mixture_nll_fwd(vocab, ptr, sw, label, V, pad):
    """vocab [B,T,ldv] f32, ptr [B,T,T] f32 (scaled), sw [B*T] f32, label int64 [B,T].
    Returns stats (sum_nll, n_valid, n_correct) and per-row lse."""
    B, T = label.shape
    stats = torch.zeros(4, dtype=torch.float32, device=vocab.device)
    row_lse = _f32(B * T, 2, device=vocab.device)
    L.check(L.lib().pa_mixture_nll_fwd(L.ptr(stats), L.ptr(row_lse), L.ptr(vocab), vocab.stride(-2), L.ptr(ptr),
                                       L.ptr(sw), L.ptr(label), B, T, V, pad, L.stream()), "pa_mixture_nll_fwd")
    return stats, row_lse


def mixture_nll_bwd(stats, row_lse, vocab, ptr, sw, label, V, pad, gscale=1.0, out_dtype=torch.float32):
    B, T = label.shape
    dvocab = torch.empty(vocab.shape, dtype=out_dtype, device=vocab.device)
    dptr = torch.empty(ptr.shape, dtype=out_dtype, device=vocab.device)
    dsw = torch.empty_like(sw)
    L.check(L.lib().pa_mixture_nll_bwd(L.ptr(dvocab), L.ptr(dptr), L.dt(dvocab), L.ptr(dsw), L.ptr(stats), L.ptr(row_lse),
                                       L.ptr(vocab), vocab.stride(-2), L.ptr(ptr), L.ptr(sw), L.ptr(label), B, T, V,
                                       pad, C.c_float(gscale), L.stream()), "pa_mixture_nll_bwd")
    return dvocab, dptr, dsw


def loss_weight_layout(weight, B, T):
    """0 for a per-drawing weight [B], 1 for a per-token weight [B, T] (pa_loss_ext.weight_per_token); ValueError for anything else."""
    if not torch.is_tensor(weight) or not weight.is_floating_point() or tuple(weight.shape) not in ((B,), (B, T)):
        shape = tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__
        raise ValueError(f"loss_weight must be a float tensor of shape [{B}] or [{B}, {T}], got {shape}")
    return weight.dim() - 1


def loss_ext_block(smoothing, weight, B, T, token_nll, ext_stats):
    """The pa_loss_ext of one call; ``weight`` f32 contiguous on the device (or None), ``token_nll`` f32 [B, T] (or None)."""
    per_token = 0 if weight is None else loss_weight_layout(weight, B, T)
    return L.LossExt(float(smoothing), per_token, L.ptr(weight).value if weight is not None else None,
                     L.ptr(token_nll).value if token_nll is not None else None, L.ptr(ext_stats).value)


def mixture_nll_ext_fwd(vocab, ptr, sw, label, V, pad, smoothing=0.0, weight=None, token_nll=False, out=None):
    """The extended objective (include/plank_hip.h pa_loss_ext).  Operands as mixture_nll_fwd; ``weight`` f32 [B] or [B, T] or None.
    Returns (stats8, row_lse, ext_stats, token_nll or None): stats8[4] the loss, ext_stats[2] the plain mean NLL.  ``out``: buffers to
    write into instead of fresh ones, by the same names (``token_nll`` included)."""
    B, T = label.shape
    out = out or {}
    dev = vocab.device
    stats = out["stats8"] if "stats8" in out else torch.empty(8, dtype=torch.float32, device=dev)
    row_lse = out["row_lse"] if "row_lse" in out else _f32(B * T, 2, device=dev)
    ext = out["ext_stats"] if "ext_stats" in out else torch.empty(4, dtype=torch.float32, device=dev)
    tok = out["token_nll"] if "token_nll" in out else (_f32(B, T, device=dev) if token_nll else None)
    e = loss_ext_block(smoothing, weight, B, T, tok, ext)
    L.check(L.lib().pa_mixture_nll_fwd_ext(L.ptr(stats), L.ptr(row_lse), L.ptr(vocab), vocab.stride(-2), L.ptr(ptr), L.ptr(sw),
                                           L.ptr(label), B, T, V, pad, C.byref(e), L.stream()), "pa_mixture_nll_fwd_ext")
    return stats, row_lse, ext, tok


def mixture_nll_ext_bwd(stats, row_lse, ext_stats, vocab, ptr, sw, label, V, pad, smoothing=0.0, weight=None, gscale=1.0,
                        out_dtype=torch.float32, upstream=None, out=None):
    """Gradients of the extended objective from the forward's stats8 and row_lse: (dvocab, dptr, dsw).  ``upstream``: device f32
    scalar d(loss), None = stats8[3]."""
    B, T = label.shape
    out = out or {}
    dvocab = out["dvocab"] if "dvocab" in out else torch.empty(vocab.shape, dtype=out_dtype, device=vocab.device)
    dptr = out["dptr"] if "dptr" in out else torch.empty(ptr.shape, dtype=out_dtype, device=vocab.device)
    dsw = out["dsw"] if "dsw" in out else torch.empty_like(sw)
    e = loss_ext_block(smoothing, weight, B, T, None, ext_stats)
    L.check(L.lib().pa_mixture_nll_bwd_ext(L.ptr(dvocab), L.ptr(dptr), L.dt(dvocab), L.ptr(dsw), L.ptr(stats), L.ptr(row_lse),
                                           L.ptr(vocab), vocab.stride(-2), L.ptr(ptr), L.ptr(sw), L.ptr(label), B, T, V, pad,
                                           C.c_float(gscale), L.ptr(upstream), C.byref(e), L.stream()), "pa_mixture_nll_bwd_ext")
    return dvocab, dptr, dsw


def adam_step(p, g, m, v, step, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0, p_bf16=None):
    L.check(L.lib().pa_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(p_bf16), C.c_int64(p.numel()),
                                 C.c_float(lr), C.c_float(b1), C.c_float(b2), C.c_float(eps), int(step),
                                 C.c_float(gscale), L.stream()), "pa_adam_step")


def grad_guard_ws(device, step0=0):
    """A workspace of the gradient guard (include/plank_hip.h pa_grad_guard), counters zeroed, Adam step count = ``step0``."""
    ws = torch.empty(L.ws_bytes("pa_grad_guard_ws_bytes"), dtype=torch.uint8, device=device)
    L.check(L.lib().pa_grad_guard_init(L.ptr(ws), C.c_int64(ws.numel()), int(step0), L.stream()), "pa_grad_guard_init")
    return ws


def grad_guard(g, ws, gscale=1.0, max_norm=0.0, skip_nonfinite=False, lr=1e-4, b1=0.9, b2=0.999):
    """Enqueue the norm of ``g * gscale`` and the step decision into ``ws`` (two launches, nothing read back)."""
    L.check(L.lib().pa_grad_guard(L.ptr(g), C.c_int64(g.numel()), C.c_float(gscale), C.c_float(max_norm or 0.0),
                                  int(bool(skip_nonfinite)), C.c_float(lr), C.c_float(b1), C.c_float(b2), L.ptr(ws),
                                  C.c_int64(ws.numel()), L.stream()), "pa_grad_guard")


def grad_guard_ctl(ws):
    """The guard's control block as a dict.  SYNCHRONISES (a device-to-host copy of 64 bytes)."""
    raw = ws[L.GRAD_GUARD_CTL_OFFSET:L.GRAD_GUARD_WS_BYTES].cpu().numpy().tobytes()
    c = L.GradGuardCtl.from_buffer_copy(raw)
    return {k: getattr(c, k) for k, _ in L.GradGuardCtl._fields_ if k != "pad_"}


def adam_step_guarded(p, g, m, v, ws, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0, clip_value=0.0, p_bf16=None):
    """pa_adam_step with step size, bias correction, clip coefficient and the apply flag taken from the guard's ``ws``."""
    ctl = C.c_void_p(ws.data_ptr() + L.GRAD_GUARD_CTL_OFFSET)
    L.check(L.lib().pa_adam_step_guarded(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(p_bf16), C.c_int64(p.numel()),
                                         C.c_float(b1), C.c_float(b2), C.c_float(eps), C.c_float(gscale),
                                         C.c_float(clip_value or 0.0), ctl, L.stream()), "pa_adam_step_guarded")


def adam_step_ext(p, g, m, v, step=0, ws=None, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0, clip_value=0.0,
                  weight_decay=0.0, decay_bits=None, ema=None, ema_decay=0.0, ema_warmup=False, p_bf16=None):
    """pa_adam_step_ext: Adam with decoupled weight decay (``decay_bits``: uint8 bitmask of the elements that decay, None: all)
    and a weight EMA in the same pass.  ``ws`` (a guard workspace pa_grad_guard has just written): the guarded form, ``step``
    ignored; else ``step`` >= 1 is this step's Adam step count."""
    ad = lambda t: None if t is None else t.data_ptr()
    a = L.AdamExtArgs(p=ad(p), g=ad(g), m=ad(m), v=ad(v), p_bf16=ad(p_bf16), ema=ad(ema), decay_bits=ad(decay_bits),
                      n=p.numel(), lr=lr, b1=b1, b2=b2, eps=eps, gscale=gscale, clip_value=clip_value or 0.0,
                      weight_decay=weight_decay, ema_decay=ema_decay, step=int(step), ema_warmup=int(bool(ema_warmup)),
                      ctl=None if ws is None else ws.data_ptr() + L.GRAD_GUARD_CTL_OFFSET)
    L.check(L.lib().pa_adam_step_ext(C.byref(a), L.stream()), "pa_adam_step_ext")


def cast(src, dtype):
    dst = torch.empty(src.shape, dtype=dtype, device=src.device)
    L.check(L.lib().pa_cast(L.ptr(dst), L.dt(dst), L.ptr(src), L.dt(src), C.c_int64(src.numel()), L.stream()),
            "pa_cast")
    return dst


def attn_split_ws(rows_total, B, H, device, L_max=1 << 20):
    """Scratch for the range blocks of packed self-attention launches (include/plank_hip.h pa_attn_args.ws), zeroed as its
    contract asks, or None when the library would not use one."""
    n = int(L.lib().pa_attn_ws_bytes(int(rows_total), int(B), int(H), int(L_max)))
    return torch.zeros(n, dtype=torch.uint8, device=device) if n > 0 else None


def attn_varlen_fwd(q, k, v, H, cu_q, cu_k, B, Lq_max, Lk_max, causal=False, scale=None, drop_p=0.0, drop_seed=0, order=None, ws=None):
    """Packed ("unpadded") attention: q [Nq, H*dh], k/v [Nk, H*dh] with int32 row offsets cu_q / cu_k [B+1]
    (either may be None = dense [B*L] rows).  Returns (o [Nq, H*dh], lse [B, H, Lq_max]).  ``ws``: attn_split_ws()."""
    o = torch.empty(q.shape[0], q.shape[1], dtype=q.dtype, device=q.device)
    lse = _f32(B, H, Lq_max, device=q.device)
    a = _attn_args(q, k, v, o, lse, None, causal, scale, drop_p, drop_seed, H, cu_q, cu_k, B, Lq_max, Lk_max, order)
    if ws is not None:
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    L.check(L.lib().pa_attn_fwd(C.byref(a), L.stream()), "pa_attn_fwd")
    return o, lse


def attn_varlen_bwd(dout, q, k, v, o, lse, H, cu_q, cu_k, B, Lq_max, Lk_max, causal=False, scale=None, drop_p=0.0, drop_seed=0, order=None, ws=None):
    a = _attn_args(q, k, v, o, lse, None, causal, scale, drop_p, drop_seed, H, cu_q, cu_k, B, Lq_max, Lk_max, order)
    if ws is not None:
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    dq = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    dk = torch.empty(k.shape, dtype=k.dtype, device=k.device)
    dv = torch.empty(v.shape, dtype=v.dtype, device=v.device)
    delta = _f32(lse.shape, device=q.device)
    a.dout, a.dq, a.dk, a.dv, a.delta = dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr()
    a.lddo, a.lddq, a.lddk, a.lddv = dout.stride(-2), dq.stride(-2), dk.stride(-2), dv.stride(-2)
    L.check(L.lib().pa_attn_bwd(C.byref(a), L.stream()), "pa_attn_bwd")
    return dq, dk, dv


def dec_cross_mq(qt, mem, *, kpm=None, cu=None, S=None, ws=None):
    """Absorbed ("multi-query") cross-attention of one decode step (csrc/decode_mq.h, pa_dec_cross_mq): qt [B, H, 512] bf16 (already
    carrying scale * log2 e), mem dense [B, S, 512] (optional kpm [B, S] uint8, 1 = PAD) or packed [rows, 512] with cu int32 [B + 1].
    Returns ctx [B, H, 512] bf16: per head the softmax-weighted sum of the element's memory rows."""
    B, H, d = qt.shape
    if cu is None:
        S = mem.shape[1]
    if qt.dtype == torch.float32:                      # the exact-f32 form (pa_dec_cross_mq32)
        ctx = torch.empty(B, H, d, dtype=torch.float32, device=qt.device)
        if ws is not None:
            L.check(L.lib().pa_dec_cross_mq32_ws(L.ptr(ctx), L.ptr(qt), L.ptr(mem), L.ptr(kpm), L.ptr(cu), B, int(S), H, d, L.ptr(ws),
                                                 C.c_int64(ws.numel()), L.stream()), "pa_dec_cross_mq32_ws")
            return ctx
        L.check(L.lib().pa_dec_cross_mq32(L.ptr(ctx), L.ptr(qt), L.ptr(mem), L.ptr(kpm), L.ptr(cu), B, int(S), H, d, L.stream()),
                "pa_dec_cross_mq32")
        return ctx
    ctx = torch.empty(B, H, d, dtype=torch.bfloat16, device=qt.device)
    if ws is not None:                                 # range blocks (pa_dec_cross_mq_ws); ws = dec_cross_mq_ws(B, S, device)
        L.check(L.lib().pa_dec_cross_mq_ws(L.ptr(ctx), L.ptr(qt), L.ptr(mem), L.ptr(kpm), L.ptr(cu), B, int(S), H, d, L.ptr(ws),
                                           C.c_int64(ws.numel()), L.stream()), "pa_dec_cross_mq_ws")
        return ctx
    L.check(L.lib().pa_dec_cross_mq(L.ptr(ctx), L.ptr(qt), L.ptr(mem), L.ptr(kpm), L.ptr(cu), B, int(S), H, d, L.stream()),
            "pa_dec_cross_mq")
    return ctx


def dec_cross_mq_group(qt, mem, group, *, kpm=None, cu=None, S=None, rows_per_block=1, nparts=0, ws=None):
    """dec_cross_mq for a decode group (pa_dec_cross_mq_group / pa_dec_cross_mq32_group): qt [B * group, H, 512],
    mem / kpm / cu of B drawings - row r attends over drawing r // group.  ``rows_per_block`` 1 or 2 rows of a drawing per block;
    ``nparts`` 0 = range blocks by the rule, n = n per unit; ``ws``: zeroed uint8 scratch that holds them (None: one block per unit)."""
    R, H, d = qt.shape
    if R % int(group):
        raise ValueError(f"{R} rows are no multiple of the group {group}")
    if cu is None:
        S = mem.shape[1]
    ctx = torch.empty_like(qt)
    name = "pa_dec_cross_mq32_group" if qt.dtype == torch.float32 else "pa_dec_cross_mq_group"
    L.check(getattr(L.lib(), name)(L.ptr(ctx), L.ptr(qt), L.ptr(mem), L.ptr(kpm), L.ptr(cu), R // int(group), int(group), int(S), H, d,
                                   int(rows_per_block), int(nparts), L.ptr(ws), C.c_int64(ws.numel() if ws is not None else 0),
                                   L.stream()), name)
    return ctx


def dec_cross_mq_ws(B, S, device):
    """Zeroed scratch for dec_cross_mq(..., ws=): None when the library would launch one block per element anyway."""
    n = int(L.lib().pa_dec_cross_mq_ws_bytes(int(B), int(S)))
    return torch.zeros(n, dtype=torch.uint8, device=device) if n > 0 else None


def dec_self_mq32(qt, xcache, t_dev):
    """Self-attention form of the absorbed decode attention (pa_dec_self_mq32): qt [B, H, 512] f32, xcache [B, Tmax, 512] f32, t_dev int32
    device scalar (element b attends over rows 0 .. t).  Returns ctx [B, H, 512] f32."""
    B, H, d = qt.shape
    ctx = torch.empty(B, H, d, dtype=torch.float32, device=qt.device)
    L.check(L.lib().pa_dec_self_mq32(L.ptr(ctx), L.ptr(qt), L.ptr(xcache), L.ptr(t_dev), B, xcache.shape[1], H, d, L.stream()),
            "pa_dec_self_mq32")
    return ctx


def dec_self_mq(qt, xcache, t_dev, *, nparts=0, ws=None):
    """The self-attention form in both types (pa_dec_self_mq_ws): qt [B, H, 512] and xcache [B, Tmax, 512] f32 or bf16, t_dev int32 device
    scalar.  ``nparts`` 0 = one block per row, n = n range blocks per row in ``ws`` (zeroed uint8 scratch; None: one block per row)."""
    B, H, d = qt.shape
    ctx = torch.empty_like(qt)
    L.check(L.lib().pa_dec_self_mq_ws(L.ptr(ctx), L.ptr(qt), L.ptr(xcache), L.ptr(t_dev), B, xcache.shape[1], H, d,
                                      0 if qt.dtype == torch.float32 else 1, int(nparts), L.ptr(ws),
                                      C.c_int64(ws.numel() if ws is not None else 0), L.stream()), "pa_dec_self_mq_ws")
    return ctx


def _padt(t):
    return 0 if t.dtype == torch.float32 else 1


def dec_attn(q, kc, vc, *, H, d=None, kpm=None, fixed_lk=0, t_dev=None, cu=None, newkv=None, group=1):
    """The single-query attention of the decode step over per-head caches (pa_dec_attn): q [B, ldq] rows of which the first d columns
    are the query (``d`` defaults to ldq), kc / vc [B // group, H, Lmax, dh].  Key count: ``cu`` int32 [B // group + 1], else
    ``fixed_lk`` > 0, else ``t_dev`` + 1 read on the device.  ``newkv`` [B, 3 d] (the self form): key Lk - 1 comes from it and is
    appended to both caches in place.  Returns out [B, d]."""
    B, ldq = q.shape
    d = int(d or ldq)
    out = torch.empty(B, d, dtype=q.dtype, device=q.device)
    L.check(L.lib().pa_dec_attn(L.ptr(out), L.ptr(q), ldq, L.ptr(kc), L.ptr(vc), kc.shape[2], L.ptr(kpm), int(fixed_lk), L.ptr(t_dev), B, int(H),
                                d, _padt(q), L.ptr(cu), L.ptr(newkv), int(group), L.stream()), "pa_dec_attn")
    return out


def dec_split_heads(kv, B, S, H, *, cu=None, rowmap=None):
    """kv [rows, 2 d] (k | v) -> K, V [B, H, S, dh] (pa_dec_split_heads): dense rows b S + s, or packed rows with ``cu`` [B + 1] and
    ``rowmap`` [rows].  Positions no row maps to are left as allocated (zeros here)."""
    rows, d = kv.shape[0], kv.shape[1] // 2
    kc = torch.zeros(B, H, S, d // H, dtype=kv.dtype, device=kv.device)
    vc = torch.zeros_like(kc)
    L.check(L.lib().pa_dec_split_heads(L.ptr(kc), L.ptr(vc), L.ptr(kv), C.c_int64(rows), int(S), d, int(H), _padt(kv), L.ptr(cu), L.ptr(rowmap),
                                       L.stream()), "pa_dec_split_heads")
    return kc, vc


def dec_embed(value, coord, pos, tokens, t_dev, dof, *, dtype=torch.float32, low_precision_copy=False):
    """The decode step's input embedding (pa_dec_embed): value / coord / pos f32 tables [*, d], tokens int64 [B, Tmax], t_dev int32 device
    scalar.  Returns x [B, d] of ``dtype`` (and its bf16 copy with ``low_precision_copy``)."""
    B, Tmax = tokens.shape
    d = value.shape[1]
    x = torch.empty(B, d, dtype=dtype, device=value.device)
    x_lp = torch.empty(B, d, dtype=torch.bfloat16, device=value.device) if low_precision_copy else None
    L.check(L.lib().pa_dec_embed(L.ptr(x), L.ptr(x_lp), L.ptr(value), L.ptr(coord), L.ptr(pos), L.ptr(tokens), Tmax, L.ptr(t_dev), B, d, int(dof),
                                 _padt(x), L.stream()), "pa_dec_embed")
    return (x, x_lp) if low_precision_copy else x


def dec_row_dist(vlog, V, pfeat, h, hid_cache, sw_w, sw_b, t_dev, *, fill=0.0):
    """The distribution the decode tails choose from (pa_dec_row_dist): vlog f32 [rows, ldv], pfeat / h [rows, d], hid_cache
    [Tmax, rows, d] (row t is written in place), sw_w [d], sw_b [1] f32, t_dev int32 device scalar.  Returns p [rows, V + Tmax] (vocab k at
    k, pointer j <= t at V + j; what the kernel does not write holds ``fill``) and stats [rows, 5] = vmax, vsum, pmax, psum, prob."""
    rows, d = h.shape
    Tmax = hid_cache.shape[0]
    p = torch.full((rows, int(V) + Tmax), float(fill), dtype=torch.float32, device=h.device)
    stats = torch.empty(rows, 5, dtype=torch.float32, device=h.device)
    L.check(L.lib().pa_dec_row_dist(L.ptr(p), L.ptr(stats), L.ptr(vlog), vlog.stride(0), L.ptr(pfeat), L.ptr(h), L.ptr(hid_cache), L.ptr(sw_w),
                                    L.ptr(sw_b), L.ptr(t_dev), rows, Tmax, d, int(V), _padt(h), L.stream()), "pa_dec_row_dist")
    return p, stats


def plank_match(seq_a, seq_b, pairs=None, *, end_token, filter_a, filter_b, threshold, check_pairs=True):
    """Token rows compared as sets of planks, one launch for all pairs (pa_plank_match, csrc/match.hip).

    seq_a [Ra, len_a], seq_b [Rb, len_b]: int64 device tensors, last dimension contiguous, any row stride (a slice such as
    ``samples[:, :n]`` works as it is).  ``pairs``: None - rows i of both (Ra == Rb) - or an integer tensor / sequence [n, 2] of
    (row of a, row of b).  Pairs given on the host are range-checked there; pairs that already live on the device are checked
    with one read-back unless ``check_pairs=False`` (the kernel cannot know how many rows exist).  ``filter_x``: drop the
    zero-extent planks of that side.  Returns int32 [n, 4] on the device: tp, n_a, n_b, ties (include/plank_hip.h)."""
    for name, t in (("seq_a", seq_a), ("seq_b", seq_b)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int64 and t.dim() == 2):
            raise TypeError(f"{name} must be a 2-D int64 device tensor")
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError(f"{name}: the tokens of a row must be contiguous (stride {t.stride(1)})")
    if seq_b.device != seq_a.device:
        raise ValueError("seq_a and seq_b must be on the same device")
    dev = seq_a.device
    pa = pb = None
    if pairs is None:
        if seq_a.shape[0] != seq_b.shape[0]:
            raise ValueError(f"without pairs both sides need the same number of rows ({seq_a.shape[0]} != {seq_b.shape[0]})")
        n = seq_a.shape[0]
    else:
        p = torch.as_tensor(pairs)
        if p.numel() == 0 and p.dim() == 1:                   # an empty list: no pairs
            p = torch.empty(0, 2, dtype=torch.int32)
        if p.dim() != 2 or p.shape[1] != 2 or p.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64):
            raise ValueError("pairs must be an integer [n, 2] tensor")
        n = p.shape[0]
        if n and (not p.is_cuda or check_pairs):
            lo, hi = p.amin(0).tolist(), p.amax(0).tolist()
            if min(lo) < 0 or hi[0] >= seq_a.shape[0] or hi[1] >= seq_b.shape[0]:
                raise IndexError(f"pairs name rows outside seq_a ({seq_a.shape[0]} rows) / seq_b ({seq_b.shape[0]} rows)")
        p = p.to(device=dev, dtype=torch.int32)
        pa, pb = p[:, 0].contiguous(), p[:, 1].contiguous()
    out = torch.empty(n, 4, dtype=torch.int32, device=dev)
    if n == 0:
        return out
    sa = seq_a.stride(0) if seq_a.shape[0] > 1 else seq_a.shape[1]
    sb = seq_b.stride(0) if seq_b.shape[0] > 1 else seq_b.shape[1]
    with torch.cuda.device(dev):
        L.check(L.lib().pa_plank_match(L.ptr(seq_a), C.c_int64(sa), int(seq_a.shape[1]), L.ptr(seq_b), C.c_int64(sb),
                                       int(seq_b.shape[1]), L.ptr(pa), L.ptr(pb), int(n), int(end_token), 6, int(bool(filter_a)),
                                       int(bool(filter_b)), float(threshold), L.ptr(out), L.stream()), "pa_plank_match")
    return out


def plank_volume(seq_a, seq_b=None, pairs=None, *, end_token, check_pairs=True):
    """Token rows compared as solids - the unions of their planks - one launch for all pairs (pa_plank_volume, csrc/volume.hip;
    DESIGN.md section 33): the counts behind shape IoU, self-overlap and the volume consensus.

    seq_a [Ra, len_a], seq_b [Rb, len_b]: int64 device tensors as for ``plank_match``; ``seq_b=None``: every b side is empty
    (the self-overlap-only call; a pair's row of b is then not read).  ``pairs`` / ``check_pairs``: as for ``plank_match``
    (without ``seq_b`` only the rows of a are range-checked; a 1-D list then names rows of a).  Returns int64 [n, 8] on the device:
    union_a, sum_a, union_b, sum_b, inter, union_ab, n_a, n_b (include/plank_hip.h); nothing is read back."""
    sides = (("seq_a", seq_a),) if seq_b is None else (("seq_a", seq_a), ("seq_b", seq_b))
    for name, t in sides:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int64 and t.dim() == 2):
            raise TypeError(f"{name} must be a 2-D int64 device tensor")
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError(f"{name}: the tokens of a row must be contiguous (stride {t.stride(1)})")
    if seq_b is not None and seq_b.device != seq_a.device:
        raise ValueError("seq_a and seq_b must be on the same device")
    dev = seq_a.device
    rows_b = seq_a.shape[0] if seq_b is None else seq_b.shape[0]
    pa = pb = None
    if pairs is None:
        if seq_a.shape[0] != rows_b:
            raise ValueError(f"without pairs both sides need the same number of rows ({seq_a.shape[0]} != {rows_b})")
        n = seq_a.shape[0]
    else:
        p = torch.as_tensor(pairs)
        if p.numel() == 0 and p.dim() == 1:                   # an empty list: no pairs
            p = torch.empty(0, 2, dtype=torch.int32)
        if seq_b is None and p.dim() == 1:                    # rows of a alone
            p = torch.stack((p, p), 1)
        if p.dim() != 2 or p.shape[1] != 2 or p.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64):
            raise ValueError("pairs must be an integer [n, 2] tensor")
        n = p.shape[0]
        if n and (not p.is_cuda or check_pairs):
            lo, hi = p.amin(0).tolist(), p.amax(0).tolist()
            if min(lo) < 0 or hi[0] >= seq_a.shape[0] or (seq_b is not None and hi[1] >= rows_b):
                raise IndexError(f"pairs name rows outside seq_a ({seq_a.shape[0]} rows) / seq_b ({rows_b} rows)")
        p = p.to(device=dev, dtype=torch.int32)
        pa, pb = p[:, 0].contiguous(), p[:, 1].contiguous()
    out = torch.empty(n, 8, dtype=torch.int64, device=dev)
    if n == 0:
        return out
    sa = seq_a.stride(0) if seq_a.shape[0] > 1 else seq_a.shape[1]
    sb = lb = 0
    if seq_b is not None:
        sb, lb = (seq_b.stride(0) if seq_b.shape[0] > 1 else seq_b.shape[1]), int(seq_b.shape[1])
    with torch.cuda.device(dev):
        L.check(L.lib().pa_plank_volume(L.ptr(seq_a), C.c_int64(sa), int(seq_a.shape[1]), L.ptr(seq_b), C.c_int64(sb), lb, L.ptr(pa),
                                        L.ptr(pb), int(n), int(end_token), 6, L.ptr(out), L.stream()), "pa_plank_volume")
    return out


OVERLAP_MODES = {"ignore": 0, "match": 1, "visible": 2}       # include/plank_hip.h PA_OVERLAP_*


def _overlap_side(name, side):
    """``side`` - a batch dict or a (value, view[, type]) tuple - as three 2-D int64 device tensors of one shape and one row
    stride (copied only where they are not that already) and the stride."""
    if isinstance(side, dict):
        side = (side.get("input_value"), side.get("input_view"), side.get("input_type"))
    if not isinstance(side, (tuple, list)) or len(side) not in (2, 3):
        raise TypeError(f"{name} must be a dict with input_value / input_view / optional input_type, or a tuple of those")
    rows = [side[0], side[1], side[2] if len(side) == 3 else None]
    for key, t in zip(("value", "view", "type"), rows):
        if t is None and key == "type":
            continue
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int64 and t.dim() == 2):
            raise TypeError(f"{name}: {key} must be a 2-D int64 device tensor")
        if t.shape != rows[0].shape or t.device != rows[0].device:
            raise ValueError(f"{name}: {key} {tuple(t.shape)} on {t.device} against value {tuple(rows[0].shape)} on {rows[0].device}")
    have = [t for t in rows if t is not None]
    if any((t.shape[1] > 1 and t.stride(1) != 1) or t.stride(0) != have[0].stride(0) for t in have):
        rows = [None if t is None else t.contiguous() for t in rows]
    v = rows[0]
    return rows, (v.stride(0) if v.shape[0] > 1 else v.shape[1])


def line_overlap(a, b, pairs=None, *, end_token, num_bits, tol=1, types="ignore", check_pairs=True):
    """Encoder rows compared as sets of axis-aligned lines, one launch for all pairs (pa_line_overlap, csrc/overlap.hip; DESIGN.md
    section 30): the counts behind the reprojection score.

    ``a`` (the given drawings) and ``b`` (the renderings): a dict with ``input_value`` / ``input_view`` / optional ``input_type``
    or a tuple ``(value, view[, type])`` of int64 device tensors [Ra, Sa] / [Rb, Sb], last dimension contiguous; the rows of a
    side share one row stride (they are copied where they do not).  Line drawings only: the tokens of a sideface input are
    faces, not lines.  ``pairs`` / ``check_pairs``: as for ``plank_match``.  ``tol``: the tolerance in quantisation levels, 0 ..
    255.  ``types``: ``ignore`` (no type is read), ``match`` (lines match at equal type only; both sides need a type row, else
    ValueError) or ``visible`` (only the type-0 lines of ``b`` take part).  Returns int32 [n, 8] on the device: cov(A|B), len(A),
    cov(B|A), len(B), kept_A, kept_B, skipped_A, skipped_B (include/plank_hip.h); nothing is read back."""
    if types not in OVERLAP_MODES:
        raise ValueError(f"types must be one of {tuple(OVERLAP_MODES)}, not {types!r}")
    (va, wa, ta), sa = _overlap_side("a", a)
    (vb, wb, tb), sb = _overlap_side("b", b)
    if types == "match" and (ta is None or tb is None):
        raise ValueError("types='match' needs a type row on both sides")
    if vb.device != va.device:
        raise ValueError("a and b must be on the same device")
    dev = va.device
    pa = pb = None
    if pairs is None:
        if va.shape[0] != vb.shape[0]:
            raise ValueError(f"without pairs both sides need the same number of rows ({va.shape[0]} != {vb.shape[0]})")
        n = va.shape[0]
    else:
        p = torch.as_tensor(pairs)
        if p.numel() == 0 and p.dim() == 1:                   # an empty list: no pairs
            p = torch.empty(0, 2, dtype=torch.int32)
        if p.dim() != 2 or p.shape[1] != 2 or p.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64):
            raise ValueError("pairs must be an integer [n, 2] tensor")
        n = p.shape[0]
        if n and (not p.is_cuda or check_pairs):
            lo, hi = p.amin(0).tolist(), p.amax(0).tolist()
            if min(lo) < 0 or hi[0] >= va.shape[0] or hi[1] >= vb.shape[0]:
                raise IndexError(f"pairs name rows outside a ({va.shape[0]} rows) / b ({vb.shape[0]} rows)")
        p = p.to(device=dev, dtype=torch.int32)
        pa, pb = p[:, 0].contiguous(), p[:, 1].contiguous()
    out = torch.empty(n, 8, dtype=torch.int32, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        L.check(L.lib().pa_line_overlap(L.ptr(va), L.ptr(wa), L.ptr(ta), C.c_int64(sa), int(va.shape[1]), L.ptr(vb), L.ptr(wb), L.ptr(tb),
                                        C.c_int64(sb), int(vb.shape[1]), L.ptr(pa), L.ptr(pb), int(n), int(end_token), int(num_bits),
                                        int(tol), OVERLAP_MODES[types], L.ptr(out), L.stream()), "pa_line_overlap")
    return out


RENDER_MAX_PLANKS = 32                # include/plank_hip.h PA_RENDER_MAX_PLANKS


def render_drawings(coords, n_planks=None, *, max_input_length, num_bits, end_token, pad_token, skip_first=True, with_type=True,
                    augmentation=False, aug_ratio=0.0, noise_ratio=0.0, noise_length=0.0, seed=0, epoch=0, lines=True):
    """The three-view line drawing of every row's planks, rendered and tokenised by one launch (pa_render_drawings,
    csrc/render.h).

    ``coords`` float64 [B, P, 6] on the device (lo xyz, hi xyz per plank, in [-1, 1]); ``n_planks`` integer [B] on the device
    (default: P for every row) - the planks of row b are ``coords[b, :n_planks[b]]``; plank 0 is not drawn with ``skip_first``.
    P above PA_RENDER_MAX_PLANKS raises PA_ESHAPE; nothing is read back.  The noise draws of an augmented call are keyed by
    the row number.  Returns the encoder rows of the batch contract (``input_value`` / ``input_pos`` / ``input_coord`` /
    ``input_view`` / ``input_type`` int64 [B, S], ``input_mask`` bool [B, S], S = ``max_input_length`` - 1), ``_n_tokens`` int32
    [B], ``_render_flags`` int32 [B] (PA_RENDER_* bits) and - with ``lines`` - ``_lines`` float64 [B, F, 4] (xmin ymin xmax
    ymax), ``_views`` / ``_types`` uint8 [B, F] and ``_n_lines`` int32 [B], F = (S - 1) // 4: the lines before the noise in the
    canonical order, zero behind each row's count."""
    if not (torch.is_tensor(coords) and coords.is_cuda and coords.dtype == torch.float64 and coords.dim() == 3 and coords.shape[2] == 6):
        raise TypeError("coords must be a float64 [B, P, 6] device tensor")
    B, P, dev = int(coords.shape[0]), int(coords.shape[1]), coords.device
    S = int(max_input_length) - 1
    F = max((S - 1) // 4, 0)
    if B == 0 or S <= 0:
        raise ValueError("render_drawings needs at least one row and MAX_INPUT_LENGTH >= 2")
    coords = coords.contiguous()
    if P == 0:                                         # never an empty allocation: the ABI takes no NULL arrays
        coords = torch.zeros(B, 1, 6, dtype=torch.float64, device=dev)
    stride = int(coords.shape[1])
    if n_planks is None:
        cnt = torch.full((B,), P, dtype=torch.int32, device=dev)
    else:
        if not (torch.is_tensor(n_planks) and n_planks.is_cuda and n_planks.shape == (B,)):
            raise TypeError("n_planks must be an integer [B] device tensor")
        cnt = n_planks.to(torch.int32).clamp(0, P).contiguous()
    off = torch.arange(B + 1, dtype=torch.int32, device=dev) * stride
    index = torch.arange(B, dtype=torch.int32, device=dev)
    out = {k: torch.empty(B, S, dtype=torch.int64, device=dev) for k in ("input_value", "input_pos", "input_coord", "input_view")}
    if with_type:
        out["input_type"] = torch.empty(B, S, dtype=torch.int64, device=dev)
    out["input_mask"] = torch.empty(B, S, dtype=torch.bool, device=dev)
    n_tokens = torch.empty(B, dtype=torch.int32, device=dev)
    flags = torch.empty(B, dtype=torch.int32, device=dev)
    ln = vw = ty = nl = None
    if lines:
        ln = torch.empty(B, max(F, 1), 4, dtype=torch.float64, device=dev)
        vw = torch.empty(B, max(F, 1), dtype=torch.uint8, device=dev)
        ty = torch.empty(B, max(F, 1), dtype=torch.uint8, device=dev)
        nl = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().pa_render_drawings(
            L.ptr(off), L.ptr(cnt), L.ptr(coords), None, B, L.ptr(index), B, P, int(bool(skip_first)), S, 0, int(num_bits),
            int(end_token), int(pad_token), 0, int(bool(with_type)), int(bool(augmentation)), float(aug_ratio), float(noise_ratio),
            float(noise_length), int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, L.ptr(out["input_value"]), L.ptr(out["input_pos"]),
            L.ptr(out["input_coord"]), L.ptr(out["input_view"]), L.ptr(out.get("input_type")), L.ptr(out["input_mask"]), None, None, None,
            L.ptr(n_tokens), L.ptr(ln), L.ptr(vw), L.ptr(ty), L.ptr(nl), L.ptr(flags), L.stream()), "pa_render_drawings")
    out["_n_tokens"], out["_render_flags"] = n_tokens, flags
    if lines:
        out["_lines"], out["_views"], out["_types"], out["_n_lines"] = ln[:, :F], vw[:, :F], ty[:, :F], nl
    return out


SEQ_OBJECTIVES = ("reinforce", "risk")
SEQ_BASELINES = ("none", "mean", "greedy")


def sequence_batch(tokens, attach, first_end, scores, counts, output_value, output_label, *, num_samples, vocab_size, end_token,
                   pad_token, objective="reinforce", baseline="mean", alpha=1.0, nll_weight=0.0, base_counts=None):
    """The sample decoder's buffers and their match counts -> a teacher-forced, weighted training batch, one launch, nothing read
    back (pa_sequence_batch, csrc/seqtrain.hip; include/plank_hip.h has the row and weight rules).

    tokens / attach int64 [B*N, Tmax] (last dimension contiguous, the same row stride), first_end int32 [B*N], scores f32 [B*N],
    counts int32 [B*N, 4] (``plank_match`` of the sample rows against their drawing's ground truth), base_counts int32 [B, 4]
    (baseline ``greedy``), output_value / output_label int64 [B, T] with T >= Tmax; all on one device.  ``objective``
    ``reinforce`` | ``risk``; ``baseline`` ``none`` | ``mean`` | ``greedy``.  TypeError for a wrong dtype or device, ValueError for
    a wrong shape or value, before the call.  Returns (output_value, output_label int64 [B*G, T], output_mask bool [B*G, T],
    loss_weight f32 [B*G], reward f32 [B, N]) with G = N + (nll_weight != 0)."""
    N = num_samples
    if isinstance(N, bool) or not isinstance(N, int) or not 1 <= N <= 64:
        raise ValueError(f"num_samples must be an integer in [1, 64], got {N!r}")
    if objective not in SEQ_OBJECTIVES:
        raise ValueError(f"objective must be one of {SEQ_OBJECTIVES}, got {objective!r}")
    if baseline not in SEQ_BASELINES:
        raise ValueError(f"baseline must be one of {SEQ_BASELINES}, got {baseline!r}")
    for name, v in (("alpha", alpha), ("nll_weight", nll_weight)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if objective == "risk" and not alpha > 0:
        raise ValueError(f"alpha must be > 0 under objective 'risk', got {alpha!r}")
    if baseline == "mean" and N < 2:
        raise ValueError("baseline 'mean' needs num_samples >= 2")
    if (base_counts is None) != (baseline != "greedy"):
        raise ValueError("base_counts goes with baseline 'greedy', and only with it")
    spec = [("tokens", tokens, torch.int64, 2), ("attach", attach, torch.int64, 2), ("first_end", first_end, torch.int32, 1),
            ("scores", scores, torch.float32, 1), ("counts", counts, torch.int32, 2), ("output_value", output_value, torch.int64, 2),
            ("output_label", output_label, torch.int64, 2)]
    if base_counts is not None:
        spec.append(("base_counts", base_counts, torch.int32, 2))
    for name, t, dtype, dim in spec:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype):
            raise TypeError(f"{name} must be a {dtype} device tensor")
        if t.device != tokens.device:
            raise TypeError(f"{name} must be on the device of tokens ({tokens.device}), got {t.device}")
        if t.dim() != dim:
            raise ValueError(f"{name} must have {dim} dimension(s), got shape {tuple(t.shape)}")
    rows, Tmax = tokens.shape
    B, T = output_value.shape
    if rows != B * N:
        raise ValueError(f"tokens has {rows} rows for {B} drawings of {N} samples")
    if attach.shape != tokens.shape or output_label.shape != output_value.shape:
        raise ValueError("attach / output_label must have the shape of tokens / output_value")
    if first_end.shape != (rows,) or scores.shape != (rows,) or counts.shape != (rows, 4):
        raise ValueError(f"first_end / scores / counts must be [{rows}] / [{rows}] / [{rows}, 4]")
    if base_counts is not None and base_counts.shape != (B, 4):
        raise ValueError(f"base_counts must be [{B}, 4], got {tuple(base_counts.shape)}")
    if Tmax > T:
        raise ValueError(f"the samples are longer (Tmax {Tmax}) than the ground-truth rows (T {T})")

    def strided(a, b):                                 # two row-major views with one row stride: read in place when they are that
        ok = all(t.shape[1] <= 1 or t.stride(1) == 1 for t in (a, b)) and (a.shape[0] <= 1 or a.stride(0) == b.stride(0))
        if not ok:
            a, b = a.contiguous(), b.contiguous()
        return a, b, (a.stride(0) if a.shape[0] > 1 else a.shape[1])
    tokens, attach, s_stride = strided(tokens, attach)
    output_value, output_label, g_stride = strided(output_value, output_label)
    first_end, scores, counts = first_end.contiguous(), scores.contiguous(), counts.contiguous()
    base_counts = None if base_counts is None else base_counts.contiguous()
    dev = tokens.device
    G = N + (1 if float(nll_weight) != 0.0 else 0)
    out_value = torch.empty(B * G, T, dtype=torch.int64, device=dev)
    out_label = torch.empty(B * G, T, dtype=torch.int64, device=dev)
    out_mask = torch.empty(B * G, T, dtype=torch.uint8, device=dev)
    out_weight = torch.empty(B * G, dtype=torch.float32, device=dev)
    reward = torch.empty(B, N, dtype=torch.float32, device=dev)
    a = L.SeqBatchArgs(tokens.data_ptr(), attach.data_ptr(), first_end.data_ptr(), scores.data_ptr(), counts.data_ptr(),
                       None if base_counts is None else base_counts.data_ptr(), output_value.data_ptr(), output_label.data_ptr(),
                       out_value.data_ptr(), out_label.data_ptr(), out_mask.data_ptr(), out_weight.data_ptr(), reward.data_ptr(),
                       s_stride, g_stride, B, N, Tmax, T, SEQ_OBJECTIVES.index(objective), SEQ_BASELINES.index(baseline),
                       float(alpha), float(nll_weight), int(vocab_size), int(end_token), int(pad_token), 0)
    if B > 0:
        with torch.cuda.device(dev):
            L.check(L.lib().pa_sequence_batch(C.byref(a), L.stream()), "pa_sequence_batch")
    return out_value, out_label, out_mask.view(torch.bool), out_weight, reward
