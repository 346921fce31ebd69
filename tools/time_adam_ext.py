"""What the Adam pass (the one kernel behind pa_adam_step / pa_adam_step_guarded / pa_adam_step_ext) costs at
the headline parameter count: the kernel alone, back to back, hip-event time per call, every variant in alternating blocks in ONE process.

    python tools/time_adam_ext.py [--parent-lib PATH/libplank_hip.so] [--blocks 6] [--reps 100] [--out profiles/adam_ext_time.txt]

Variants: pa_adam_step of this tree twice (an A/A pair: the session's spread) and pa_adam_step_guarded; both entries of the library
given with --parent-lib (a build of the parent commit); and pa_adam_step_ext with (a) everything off - the same kernel instantiation as
pa_adam_step, through the struct entry -, (b) decay with the 1-D mask, (c) EMA, (d) both, (e) both under the guard's control block.
Bytes per call are counted from the buffer widths the kernel must move."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from plankassembly_amd import _lib as L
from plankassembly_amd import ops
from plankassembly_amd.optim import decay_bitmask

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--blocks", type=int, default=6)
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--out", default=None)
args = ap.parse_args()

model = bench.build("bf16", bench.S_IN + 1, bench.T_OUT, 0.2)
n = model.flat_params.numel()
bits = torch.from_numpy(decay_bitmask(model, "1d")).cuda()
gen = torch.Generator(device="cuda").manual_seed(1)
p = model.flat_params.detach().clone()
g = torch.randn(n, device="cuda", generator=gen) * 1e-3
m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
pb = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
ws = ops.grad_guard_ws("cuda")
ops.grad_guard(g, ws, max_norm=1.0, skip_nonfinite=True)
del model


def plain(lib):
    fn = lib.pa_adam_step
    fn.restype = C.c_int32
    a = (L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(pb), C.c_int64(n), C.c_float(1e-4), C.c_float(0.9), C.c_float(0.999),
         C.c_float(1e-8), C.c_int32(1000), C.c_float(1.0), L.stream())
    return lambda: L.check(fn(*a), "pa_adam_step")


def guarded(lib):
    fn = lib.pa_adam_step_guarded
    fn.restype = C.c_int32
    a = (L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(pb), C.c_int64(n), C.c_float(0.9), C.c_float(0.999), C.c_float(1e-8),
         C.c_float(1.0), C.c_float(0.0), C.c_void_p(ws.data_ptr() + L.GRAD_GUARD_CTL_OFFSET), L.stream())
    return lambda: L.check(fn(*a), "pa_adam_step_guarded")


def ext(**kw):
    return lambda: ops.adam_step_ext(p, g, m, v, step=1000, p_bf16=pb, **kw)


base, with_ema, with_mask = 30 * n, 8 * n, bits.numel()            # 4 f32 reads + 3 f32 writes + the bf16 shadow; e read + write
variants = {"pa_adam_step (A)": (plain(L.lib()), base), "pa_adam_step (A again)": (plain(L.lib()), base)}
variants["pa_adam_step_guarded"] = (guarded(L.lib()), base)
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    variants["pa_adam_step (parent build)"] = (plain(parent), base)
    variants["pa_adam_step_guarded (parent build)"] = (guarded(parent), base)
variants.update({
    "ext (a) off: pa_adam_step's kernel": (ext(), base),
    "ext (b) decay + mask": (ext(weight_decay=0.01, decay_bits=bits), base + with_mask),
    "ext (c) EMA": (ext(ema=ema, ema_decay=0.999), base + with_ema),
    "ext (d) decay + mask + EMA": (ext(weight_decay=0.01, decay_bits=bits, ema=ema, ema_decay=0.999), base + with_mask + with_ema),
    "ext (e) (d) under the guard": (ext(weight_decay=0.01, decay_bits=bits, ema=ema, ema_decay=0.999, ws=ws, clip_value=0.0),
                                    base + with_mask + with_ema),
})


def block(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps * 1e3


for fn, _ in variants.values():
    block(fn, 10)
times = {k: [] for k in variants}
for _ in range(args.blocks):
    for k, (fn, _) in variants.items():
        times[k].append(block(fn, args.reps))
assert torch.isfinite(p).all() and torch.isfinite(ema).all()

mean = {k: statistics.mean(t) for k, t in times.items()}
ref = mean["pa_adam_step (A)"]
lines = [f"device: {torch.cuda.get_device_name(0)}; n = {n} parameters ({4 * n / 1e6:.1f} MB per f32 buffer); {args.blocks} alternating "
         f"blocks of {args.reps} back-to-back calls per variant, hip-event time per block / calls (launch gaps included)"]
for k, t in times.items():
    nbytes = variants[k][1]
    lines.append(f"{k:36s}: mean {mean[k]:7.1f} us  min {min(t):7.1f}  max {max(t):7.1f}  x{mean[k] / ref:.3f} of (A)  "
                 f"{nbytes / 1e6:7.1f} MB -> {nbytes / mean[k] / 1e6:.2f} TB/s")
lines.append(f"A/A spread: |A - A again| {abs(mean['pa_adam_step (A)'] - mean['pa_adam_step (A again)']):.1f} us; block-to-block range "
             f"of (A): {max(times['pa_adam_step (A)']) - min(times['pa_adam_step (A)']):.1f} us")
lines.append(f"byte ratio of (d) to pa_adam_step: {(base + with_mask + with_ema) / base:.3f}")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
