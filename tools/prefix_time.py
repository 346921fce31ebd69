"""Greedy step without a prefix table, with an all-free table, and fully forced (the scorer), in one process.

For each row count (B rows, Tmax 128, bf16, the bench decode model) under graph replay: greedy without a table (the step as it was
before prefixes existed), greedy with a table of plen = 0 (what carrying the table costs) and every position
forced to the table-less run's own output (what PlankModel.score runs); the time is that of the Tmax steps alone (encoder,
pa_decode_begin and pa_decode_prefix_begin excluded), best of `REPS` runs, the three alternating.
`python tools/prefix_time.py [B ...]` (default: 16 64 256).  One row count under
`rocprofv3 --kernel-trace --stats -- python tools/prefix_time.py 16` gives the per-kernel census of the three."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from plankassembly_amd.data import spec_for, synth_batch
from plankassembly_amd.decode import GreedyDecoder, prefix_table

TMAX, REPS = 128, 5
sizes = [int(a) for a in sys.argv[1:]] or [16, 64, 256]
dm = bench.apply_gains(bench.build("bf16", 1025, TMAX, 0.0), bench.DECODE_GAINS).eval()
dm._ensure_handle()
dm._refresh_shadow()


def once(dec, batch, table):
    with torch.no_grad():
        B, _ = dec.begin(batch, TMAX)
        dec._prefix_begin(table, 1, B, TMAX)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.steps(TMAX)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / TMAX


for B in sizes:
    db = synth_batch(B, spec_for("decode"), seed=7, device="cuda")
    db.pop("name")
    db = dm.prepare_batch(db)
    decs = [GreedyDecoder(dm, use_graph=True, strict_graph=True, lanes=1) for _ in range(3)]
    with torch.no_grad():
        s, a = decs[0].run(db, max_len=TMAX, early_stop=False)
    mk = lambda n: prefix_table({"tokens": s, "attach": a, "lengths": [n] * B}, B, TMAX, dm.vocab_size, dm.token.END, dm.token.PAD)
    tables = [None, mk(0), mk(TMAX)]
    for d, t in zip(decs, tables):
        once(d, db, t)                                 # (the first run captures the graph)
    with torch.no_grad():                              # the forced run reproduces the tokens it was given
        tok, att, _ = decs[2]._lanes[0].buffers(B, TMAX)
        assert torch.equal(tok, s) and torch.equal(att, a)
    best = [float("inf")] * 3
    for _ in range(REPS):
        for i, (d, t) in enumerate(zip(decs, tables)):
            best[i] = min(best[i], once(d, db, t))
    g, e, f = best
    print(f"B {B} rows, Tmax {TMAX}, graph: greedy without a table {g * 1e3:.3f} ms/step, with a table of plen 0 {e * 1e3:.3f} "
          f"({e / g:.3f}x), fully forced {f * 1e3:.3f} ({f / g:.3f}x)", flush=True)
