"""What FusedAdam's gradient guard costs per training step: the headline config (bf16, B 16, S 1024, T 128) stepped with the
guard off and with it on (max_grad_norm 1.0 + skip_nonfinite), in alternating blocks in ONE process, hip-event times.

    python tools/time_grad_guard.py [--blocks 6] [--steps 40] [--out profiles/grad_guard_time.txt]

Both optimizers drive the same model (each keeps its own moments), so the blocks differ in nothing but the optimizer's step.
Also times the guard's two launches alone (pa_grad_guard over the model's flat gradient buffer)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from plankassembly_amd import ops
from plankassembly_amd.data import spec_for, synth_batch
from plankassembly_amd.optim import FusedAdam

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=6, help="blocks per variant (off, on, off, on, ...)")
ap.add_argument("--steps", type=int, default=40, help="steps per block")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--out", default=None)
args = ap.parse_args()

model = bench.build("bf16", bench.S_IN + 1, bench.T_OUT, 0.2).train()
opts = {"guard off": FusedAdam(model, lr=1e-4),
        "guard on": FusedAdam(model, lr=1e-4, max_grad_norm=1.0, skip_nonfinite=True)}
pool = []
for i in range(4):
    b = synth_batch(args.batch, spec_for("headline"), seed=2022 + i, device="cuda")
    b.pop("name")
    pool.append(model.prepare_batch(b))


def block(opt, n):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(n):
        opt.zero_grad()
        model(pool[i % len(pool)])["loss"].backward()
        opt.step()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n


for opt in opts.values():                            # warm-up: both paths, every shape
    block(opt, 10)
times = {k: [] for k in opts}
for _ in range(args.blocks):
    for k, opt in opts.items():
        times[k].append(block(opt, args.steps))

g = model.flat_grads
ws = ops.grad_guard_ws(g.device)
for _ in range(5):
    ops.grad_guard(g, ws, max_norm=1.0, skip_nonfinite=True)
start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
reps = 200
start.record()
for _ in range(reps):
    ops.grad_guard(g, ws, max_norm=1.0, skip_nonfinite=True)
end.record()
end.synchronize()
alone_us = start.elapsed_time(end) / reps * 1e3

stats = opts["guard on"].guard_stats()
lines = [f"headline config: bf16, B {args.batch}, S {bench.S_IN}, T {bench.T_OUT}; {args.blocks} alternating blocks of {args.steps} steps "
         f"per variant, hip-event time per block / steps",
         f"device: {torch.cuda.get_device_name(0)}; parameters: {g.numel()} ({g.numel() * 4 / 1e6:.1f} MB of f32 gradients)"]
for k, v in times.items():
    lines.append(f"{k:9s}: mean {statistics.mean(v):.4f} ms/step  (blocks: {' '.join(f'{x:.4f}' for x in v)})")
d = statistics.mean(times["guard on"]) - statistics.mean(times["guard off"])
lines.append(f"guard on - guard off: {d * 1e3:+.1f} us/step ({100 * d / statistics.mean(times['guard off']):+.2f} %); spread of the "
             f"guard-off blocks: {(max(times['guard off']) - min(times['guard off'])) * 1e3:.1f} us")
lines.append(f"pa_grad_guard alone (sum of squares + finish, back to back, gradient resident in the cache hierarchy or not as the "
             f"hardware decides): {alone_us:.1f} us per call = {g.numel() * 4 / alone_us / 1e6:.2f} TB/s of gradient read")
lines.append(f"guard-on optimizer after the run: {stats}")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
