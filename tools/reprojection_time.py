"""What the reprojection score costs, in one process.

1. The overlap launch alone (`ops.line_overlap`), between HIP events, at 128 and 256 pairs: the renderer's generated drawings
   (tests/render_reference.py `generated`, 6 - 20 planks, rows of 1199 tokens) against the rendering of the same program with one
   plank moved by 3 levels; then one pair at 1024 lines a side, the widest row the entry takes.
2. The render launch of the same rows (`decode._redraw`), between HIP events, for the share of the two.
3. `PlankModel.sample(select="reprojection")` against `select=None` and `select="consensus"` at B 16 x N 8 and B 64 x N 4: Tmax 128,
   bf16, the bench decode model under the plank grammar, parse=False; the three alternate, best of `REPS`.
Every step runs under a time limit of its own (`LIMIT` seconds: a watchdog thread ends the process, whatever it is blocked in).
`python tools/reprojection_time.py [--no-sample]`."""
import faulthandler
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import render_reference as RR
import reprojection_reference as R
from plankassembly_amd import ops
from plankassembly_amd.decode import _redraw

REPS, LIMIT, END, PAD, BITS = 5, 120, 512, 513, 9
TOKEN = types.SimpleNamespace(END=END, PAD=PAD)
args = sys.argv[1:]
assert torch.cuda.is_available(), "tools/reprojection_time.py measures on the GPU"


class step:
    """One measured step under its own time limit."""

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        faulthandler.dump_traceback_later(LIMIT, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()
        return False


def between_events(fn, launches=50):
    for _ in range(3):
        fn()
    best = float("inf")
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / launches)
    return best * 1e3                                           # us per launch


def programs(n, width=128):
    """n program rows of the renderer's generated drawings and the same rows with the last plank moved by 3 levels along x."""
    rows = np.stack([R.program_row(RR.generated(500 + i, 5 + i % 15), width) for i in range(n)])
    moved = rows.copy()
    for r in moved:
        last = (int(np.nonzero(r == END)[0][0]) // 6 - 1) * 6
        r[last], r[last + 3] = min(r[last] + 3, 511), min(r[last + 3] + 3, 511)
    return torch.from_numpy(rows).cuda(), torch.from_numpy(moved).cuda()


print(f"# tools/reprojection_time.py ({torch.cuda.get_device_name(0)}; best of {REPS}; every step under a limit of {LIMIT} s)")
for n_pairs in (128, 256):
    with step(f"overlap {n_pairs}"):
        rows, moved = programs(n_pairs)
        given, drawn = (_redraw(t, END, PAD, BITS, 6, 1200) for t in (rows, moved))
        kw = dict(end_token=END, num_bits=BITS, tol=1)
        counts = ops.line_overlap(given, drawn, **kw)
        c = counts.cpu().numpy()
        f1 = R.scores(c)[2]
        us = {mode: between_events(lambda: ops.line_overlap(given, drawn, types=mode, **kw)) for mode in ("ignore", "match", "visible")}
        render = between_events(lambda: _redraw(moved, END, PAD, BITS, 6, 1200), launches=20)
        print(f"overlap, {n_pairs} pairs of generated drawings (rows of 1199 tokens, {c[:, 4].mean():.0f} lines a side on average, "
              f"{c[:, 4].max()} at most; mean F1 {f1.mean():.3f}): ignore {us['ignore']:.1f} us, match {us['match']:.1f} us, visible "
              f"{us['visible']:.1f} us per launch between HIP events (50 back-to-back launches: launch cadence included); "
              f"_redraw of the same rows (torch ops + the render launch) {render:.1f} us", flush=True)

with step("overlap 1024 lines"):
    _, a, b, _ = R.large_case()
    a, b = (tuple(torch.from_numpy(x[None]).cuda() for x in s) for s in (a, b))
    us = between_events(lambda: ops.line_overlap(a, b, end_token=END, num_bits=BITS, tol=1))
    print(f"overlap, 1 pair at 1024 lines a side (rows of 4097 tokens): {us:.1f} us per launch between HIP events", flush=True)

if "--no-sample" not in args:
    import bench
    from plankassembly_amd.data import spec_for, synth_batch
    from plankassembly_amd.decode import plank_grammar
    with step("model"):
        dm = bench.apply_gains(bench.build("bf16", 1025, 128, 0.0), bench.DECODE_GAINS).eval()
    for B, N in ((16, 8), (64, 4)):
        with step(f"sample {B} x {N}"):
            db = synth_batch(B, spec_for("decode"), seed=7, device="cuda")
            db.pop("name")
            db = dm.prepare_batch(db)

            def sample(select):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.no_grad():
                    out = dm.sample(db, N, temperature=0.8, top_k=50, top_p=0.95, seed=3, constraint=plank_grammar(), parse=False,
                                    select=select)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out

            t = {None: float("inf"), "consensus": float("inf"), "reprojection": float("inf")}
            for sel in t:
                sample(sel)
            for _ in range(REPS):
                for sel in t:
                    dt, out = sample(sel)
                    t[sel] = min(t[sel], dt)
            f1 = out["reprojection_f1"]
            print(f"sample B {B} x N {N}, Tmax 128, bf16, grammar on, parse=False: select=None {t[None] * 1e3:.2f} ms, 'consensus' "
                  f"{t['consensus'] * 1e3:.2f} ms (+{(t['consensus'] - t[None]) * 1e3:.2f} ms), 'reprojection' "
                  f"{t['reprojection'] * 1e3:.2f} ms (+{(t['reprojection'] - t[None]) * 1e3:.2f} ms, ratio "
                  f"{t['reprojection'] / t[None]:.4f}); reprojection_f1 of the winners {float(f1.max(1).values.mean()):.3f}, index != 0 in "
                  f"{int((out['reprojection_index'] != 0).sum())} of {B} drawings, render flags seen "
                  f"{sorted(set(out['reprojection_flags'].reshape(-1).cpu().tolist()))}", flush=True)
