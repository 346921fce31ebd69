"""Decode step without and with the plank grammar, in one process.

Under graph replay (Tmax 128, bf16, the bench decode model), the two forms alternating, best of `REPS` runs, the time that of the Tmax
steps alone (encoder, pa_decode_begin and the mode's begin excluded):
  * greedy at each row count B, constraint off against on;
  * beam K 4 and sampling N 4 (tau 0.8, top_k 50, top_p 0.95) at B 16 drawings, off against on.
`python tools/constraint_time.py [B ...]` (default: 16 64 256; beam and sampling run when 16 is among them).
`--off-only` prints the constraint-off greedy step alone and touches nothing of the constraint interface: copied into a checkout of
another commit it times that commit's step, for the parent-commit comparison (alternate the two processes in one session).
One row count under `rocprofv3 --kernel-trace --stats -- python tools/constraint_time.py 16` gives the per-kernel census."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from plankassembly_amd.data import spec_for, synth_batch
from plankassembly_amd.decode import BeamDecoder, GreedyDecoder, SampleDecoder

TMAX, REPS = 128, 5
args = sys.argv[1:]
off_only = "--off-only" in args
sizes = [int(a) for a in args if not a.startswith("--")] or [16, 64, 256]
dm = bench.apply_gains(bench.build("bf16", 1025, TMAX, 0.0), bench.DECODE_GAINS).eval()
dm._ensure_handle()
dm._refresh_shadow()


def once(dec, batch, grammar):
    with torch.no_grad():
        dec.begin(batch, TMAX)
        if not off_only:
            dec._constraint_begin(grammar)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.steps(TMAX)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / TMAX


def batch_of(B):
    db = synth_batch(B, spec_for("decode"), seed=7, device="cuda")
    db.pop("name")
    return dm.prepare_batch(db)


def first_ends(dec, rows):
    tok, _, _ = dec._lanes[0].buffers(rows, TMAX)
    e = tok.cpu() == dm.token.END
    return torch.where(e.any(1), e.long().argmax(1), torch.full((rows,), TMAX))


def compare(what, make, db, rows):
    """Two decoders of one kind, one never constrained and one always: a decoder keeps its captured graph across its runs."""
    from plankassembly_amd.decode import check_planks, plank_grammar
    decs, grammars = [make(), make()], [None, plank_grammar()]
    for d, g in zip(decs, grammars):
        once(d, db, g)                                 # (the first run captures the graph)
    fe = first_ends(decs[1], rows)
    tok, _, _ = decs[1]._lanes[0].buffers(rows, TMAX)
    valid = int(check_planks(tok, dm.token.END, min(dm.token.END, dm.token.PAD)).sum())
    best = [float("inf")] * 2
    for _ in range(REPS):
        for i, (d, g) in enumerate(zip(decs, grammars)):
            best[i] = min(best[i], once(d, db, g))
    off, on = best
    print(f"{what}, Tmax {TMAX}, graph: constraint off {off * 1e3:.3f} ms/step, on {on * 1e3:.3f} ms/step, ratio {on / off:.3f} "
          f"(on: {valid} of {rows} rows valid programs, first END {int(fe.min())}-{int(fe.max())})", flush=True)


for B in sizes:
    db = batch_of(B)
    if off_only:
        dec = GreedyDecoder(dm, use_graph=True, strict_graph=True, lanes=1)
        once(dec, db, None)
        t = min(once(dec, db, None) for _ in range(REPS))
        print(f"greedy B {B} rows, Tmax {TMAX}, graph: constraint off {t * 1e3:.3f} ms/step", flush=True)
        continue
    compare(f"greedy B {B} rows", lambda: GreedyDecoder(dm, use_graph=True, strict_graph=True, lanes=1), db, B)
    if B == 16:
        compare("beam B 16 x K 4 (64 rows)", lambda: BeamDecoder(dm, 4, use_graph=True, strict_graph=True), db, 64)
        compare("sampling B 16 x N 4 (64 rows), tau 0.8, top_k 50, top_p 0.95",
                lambda: SampleDecoder(dm, 4, temperature=0.8, top_k=50, top_p=0.95, seed=1, use_graph=True, strict_graph=True), db, 64)
