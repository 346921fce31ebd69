"""Sampling step against the greedy step at the same row count, in one process.

For each shape (B drawings x N samples, Tmax 128, bf16, the bench decode model) and each setting (tau 1 with no filter; tau 0.8,
top_k 50, top_p 0.95): greedy on B*N rows and sampling B x N under graph replay; the time is that of the Tmax steps alone (encoder
and pa_decode_begin excluded), best of `REPS` runs, greedy and sampling alternating.  `python tools/sample_time.py [BxN ...]`
(default: 16x8 64x4 256x1).  One shape under `rocprofv3 --kernel-trace --stats -- python tools/sample_time.py 16x8` gives the
per-kernel breakdown."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from plankassembly_amd.data import spec_for, synth_batch
from plankassembly_amd.decode import GreedyDecoder, SampleDecoder

TMAX, REPS = 128, 5
SETTINGS = [("tau 1, no filter", dict()), ("tau 0.8, top_k 50, top_p 0.95", dict(temperature=0.8, top_k=50, top_p=0.95))]
shapes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]] or [(16, 8), (64, 4), (256, 1)]
dm = bench.apply_gains(bench.build("bf16", 1025, TMAX, 0.0), bench.DECODE_GAINS).eval()
dm._ensure_handle()
dm._refresh_shadow()


def once(dec, batch):
    with torch.no_grad():
        dec.begin(batch, TMAX)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.steps(TMAX)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / TMAX


for B, N in shapes:
    db = synth_batch(B, spec_for("decode"), seed=7, device="cuda")
    db.pop("name")
    rep = dm.prepare_batch({k: v.repeat_interleave(N, dim=0) for k, v in db.items()})
    g_dec = GreedyDecoder(dm, use_graph=True, strict_graph=True, lanes=1)
    decs = [SampleDecoder(dm, N, use_graph=True, strict_graph=True, seed=1, **kw) for _, kw in SETTINGS]
    once(g_dec, rep)                                   # (the first run captures the graph)
    for d in decs:
        once(d, db)
    g = float("inf")
    s = [float("inf")] * len(decs)
    for _ in range(REPS):
        g = min(g, once(g_dec, rep))
        for i, d in enumerate(decs):
            s[i] = min(s[i], once(d, db))
    for (name, _), t in zip(SETTINGS, s):
        print(f"B {B} x N {N} ({B * N} rows), Tmax {TMAX}, graph, {name}: greedy {g * 1e3:.3f} ms/step, sampling {t * 1e3:.3f} "
              f"ms/step, ratio {t / g:.3f}", flush=True)
