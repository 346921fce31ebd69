"""What the mixture NLL (one forward, one finish and one backward kernel behind the plain and the _ext entries)
costs at the headline head shape: the entries alone, back to back, hip-event time per call, every variant in alternating blocks in ONE
process.

    python tools/time_loss_ext.py [--parent-lib PATH/libplank_hip.so] [--blocks 6] [--reps 200] [--out profiles/loss_ext_time.txt]

Shape: B 16 x T 128 rows, V 514 with the model's row stride ldv = 576.  Forward = the memsets, the row kernel and the one-wave finish;
backward with f32 and with bf16 gradients.  Variants: pa_mixture_nll_fwd_fin / pa_mixture_nll_bwd_up twice (an A/A pair: the session's
spread), the same two entries of the library given with --parent-lib (a build of the parent commit), and the _ext entries with everything
off - the plain entries' backward kernel, and the forward's EXT instantiation with its second memset -, eps 0.1, per-drawing weights, and
eps 0.1 + per-token weights + token_nll."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from plankassembly_amd import _lib as L
from plankassembly_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--blocks", type=int, default=6)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--out", default=None)
args = ap.parse_args()

B, T, V, LDV, PAD = 16, 128, 514, 576, 513
n = B * T
gen = torch.Generator(device="cuda").manual_seed(1)
vocab = torch.randn(n, LDV, device="cuda", generator=gen)[:, :V]
ptr = torch.randn(n, T, device="cuda", generator=gen)
sw = torch.randn(n, device="cuda", generator=gen)
i = torch.arange(n, device="cuda") % T
u = torch.rand(n, device="cuda", generator=gen)
label = torch.where(u < 0.6, (torch.rand(n, device="cuda", generator=gen) * 512).long(), V + (torch.rand(n, device="cuda", generator=gen) * i).long())
label = torch.where(i >= 100, torch.full_like(label, PAD), label).view(B, T)                      # a PAD tail: 78 % of the rows are valid
w_b = torch.rand(B, device="cuda", generator=gen) + 0.5
w_bt = torch.rand(B, T, device="cuda", generator=gen) + 0.5
lib, st = L.lib(), L.stream()
stats, lse, ext = torch.empty(8, device="cuda"), torch.empty(n, 2, device="cuda"), torch.empty(4, device="cuda")
tok = torch.empty(B, T, device="cuda")
dsw = torch.empty(n, device="cuda")
grads = {dt: (torch.empty(n, LDV, device="cuda", dtype=dt), torch.empty(n, T, device="cuda", dtype=dt)) for dt in (torch.float32, torch.bfloat16)}


def plain_fwd(lib):
    fn = lib.pa_mixture_nll_fwd_fin
    fn.restype = C.c_int32
    a = (L.ptr(stats), L.ptr(lse), L.ptr(vocab), C.c_int32(LDV), L.ptr(ptr), L.ptr(sw), L.ptr(label), C.c_int32(B), C.c_int32(T), C.c_int32(V),
         C.c_int32(PAD), st)
    return lambda: L.check(fn(*a), "fwd_fin")


def plain_bwd(lib, dt):
    dv, dp = grads[dt]
    fn = lib.pa_mixture_nll_bwd_up
    fn.restype = C.c_int32
    a = (L.ptr(dv), L.ptr(dp), C.c_int32(L.dt(dv)), L.ptr(dsw), L.ptr(stats), L.ptr(lse), L.ptr(vocab), C.c_int32(LDV), L.ptr(ptr), L.ptr(sw),
         L.ptr(label), C.c_int32(B), C.c_int32(T), C.c_int32(V), C.c_int32(PAD), C.c_float(1.0), None, st)
    return lambda: L.check(fn(*a), "bwd_up")


old_fwd = plain_fwd(lib)
parent = C.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None


def ext_fwd(eps, weight, token):
    e = ops.loss_ext_block(eps, weight, B, T, tok if token else None, ext)                        # (built once: the loop times the entry, not the wrapper)
    a = (L.ptr(stats), L.ptr(lse), L.ptr(vocab), LDV, L.ptr(ptr), L.ptr(sw), L.ptr(label), B, T, V, PAD, C.byref(e), st)
    return lambda: L.check(lib.pa_mixture_nll_fwd_ext(*a), "fwd_ext")


def ext_bwd(eps, weight, dt):
    dv, dp = grads[dt]
    e = ops.loss_ext_block(eps, weight, B, T, None, ext)
    a = (L.ptr(dv), L.ptr(dp), L.dt(dv), L.ptr(dsw), L.ptr(stats), L.ptr(lse), L.ptr(vocab), LDV, L.ptr(ptr), L.ptr(sw), L.ptr(label), B, T, V, PAD,
         C.c_float(1.0), None, C.byref(e), st)
    return lambda: L.check(lib.pa_mixture_nll_bwd_ext(*a), "bwd_ext")


SETTINGS = [("ext, everything off", 0.0, None, False), ("ext, eps 0.1", 0.1, None, False), ("ext, weights [B]", 0.0, w_b, False),
            ("ext, eps 0.1 + weights [B,T] + token_nll", 0.1, w_bt, True)]
variants = {"fwd  plain entries (A)": old_fwd, "fwd  plain entries (A again)": old_fwd}
if parent:
    variants["fwd  plain entries (parent build)"] = plain_fwd(parent)
variants.update({f"fwd  {k}": ext_fwd(e, w, t) for k, e, w, t in SETTINGS})
for dt, tag in ((torch.float32, "f32 "), (torch.bfloat16, "bf16")):
    variants[f"bwd {tag} plain entries (A)"] = plain_bwd(lib, dt)
    variants[f"bwd {tag} plain entries (A again)"] = plain_bwd(lib, dt)
    if parent:
        variants[f"bwd {tag} plain entries (parent build)"] = plain_bwd(parent, dt)
    variants.update({f"bwd {tag} {k}": ext_bwd(e, w, dt) for k, e, w, t in SETTINGS})


def block(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps * 1e3


old_fwd()
for fn in variants.values():
    block(fn, 10)
times = {k: [] for k in variants}
for _ in range(args.blocks):
    for k, fn in variants.items():
        if k.startswith("bwd") and "plain" in k:
            old_fwd()                                            # (the statistics a backward reads are those of its own forward)
        times[k].append(block(fn, args.reps))
torch.cuda.synchronize()
assert torch.isfinite(stats[:6]).all() and torch.isfinite(grads[torch.float32][0][:, :V]).all()

mean = {k: statistics.mean(t) for k, t in times.items()}
lines = [f"device: {torch.cuda.get_device_name(0)}; B {B} x T {T} = {n} rows, V {V}, ldv {LDV}, {int((label != PAD).sum())} non-PAD rows; {args.blocks} "
         f"alternating blocks of {args.reps} back-to-back calls per variant, hip-event time per block / calls (host launch cost included)"]
for k, t in times.items():
    ref = mean[k.split("plain")[0].split("ext,")[0] + "plain entries (A)"]
    lines.append(f"{k:56s}: mean {mean[k]:6.2f} us  min {min(t):6.2f}  max {max(t):6.2f}  x{mean[k] / ref:.3f} of (A)")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
