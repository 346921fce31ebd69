"""Beam-search step against the greedy step at the same row count, in one process.

For each shape (B drawings x K beams, Tmax 128, bf16, the bench decode model): greedy on B*K rows and beam B x K, eager and
graph replay; the time is that of the Tmax steps alone (encoder and pa_decode_begin excluded), best of `REPS` runs.
`python tools/beam_time.py [BxK ...]` (default: 16x4 16x8 64x4).  One shape under
`rocprofv3 --kernel-trace --stats -- python tools/beam_time.py 16x8` gives the per-kernel breakdown."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from plankassembly_amd.data import spec_for, synth_batch
from plankassembly_amd.decode import BeamDecoder, GreedyDecoder

TMAX, REPS = 128, 3
shapes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]] or [(16, 4), (16, 8), (64, 4)]
dm = bench.apply_gains(bench.build("bf16", 1025, TMAX, 0.0), bench.DECODE_GAINS).eval()
dm._ensure_handle()
dm._refresh_shadow()


def timed(dec, batch):
    best = float("inf")
    with torch.no_grad():
        for _ in range(REPS + 1):                      # (the first run captures the graph)
            dec.begin(batch, TMAX)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.steps(TMAX)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
    return best / TMAX


for B, K in shapes:
    db = synth_batch(B, spec_for("decode"), seed=7, device="cuda")
    db.pop("name")
    rep = dm.prepare_batch({k: v.repeat_interleave(K, dim=0) for k, v in db.items()})
    for graph in (False, True):
        g = timed(GreedyDecoder(dm, use_graph=graph, strict_graph=graph, lanes=1), rep)
        b = timed(BeamDecoder(dm, K, use_graph=graph, strict_graph=graph), db)
        print(f"B {B} x K {K} ({B * K} rows), Tmax {TMAX}, {'graph' if graph else 'eager'}: greedy {g * 1e3:.3f} ms/step "
              f"({1 / g:.0f} steps/s), beam {b * 1e3:.3f} ms/step ({1 / b:.0f} steps/s), ratio {b / g:.3f}", flush=True)
