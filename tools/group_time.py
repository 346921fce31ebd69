"""Decode groups against repeated drawings, in one process at the bench decode model (d 512, 6 + 6 layers, S 1024,
Tmax 128, bf16, graph replay): per shape the decode step and the `begin` call (encoder + pa_decode_group_begin + the mode's begin) with
``share_encoder`` off and on, forms alternating, best of REPS; then one ``seq_train_step`` + backward at B 16 x N 4 and N 8, off and on.

Two rows of a drawing per block of the absorbed cross launch is a switch read once per process, so the pairing-off column is a second
process.  Every GPU step under its own time limit, chained:

    timeout -k 10 600 python tools/group_time.py && PLANK_DECODE_MQ_PAIR=0 timeout -k 10 600 python tools/group_time.py --decode-only

`python tools/group_time.py [--decode-only] [--census off|on] [sBxN | bBxK ...]` (default: s16x4 s16x8 s64x4 b16x4; s = sampling, b =
beam search).  `--census FORM` runs ONE decode of the first shape in that form and nothing else: under
`rocprofv3 --kernel-trace --stats -- python tools/group_time.py --census on s16x8` (a run of its own, no counters) the per-kernel call
counts of the two forms can be laid side by side."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from plankassembly_amd.data import spec_for, synth_batch
from plankassembly_amd.decode import BeamDecoder, SampleDecoder, plank_grammar

TMAX, REPS = 128, 5
census = sys.argv[sys.argv.index("--census") + 1] if "--census" in sys.argv else None
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in ("off", "on")]
decode_only = "--decode-only" in sys.argv or census is not None
shapes = [(a[0], *(int(v) for v in a[1:].split("x"))) for a in args] or [("s", 16, 4), ("s", 16, 8), ("s", 64, 4), ("b", 16, 4)]
assert torch.cuda.is_available(), "tools/group_time.py measures on the GPU"
pair = os.environ.get("PLANK_DECODE_MQ_PAIR", "1") != "0"
print(f"# tools/group_time.py ({torch.cuda.get_device_name(0)}; S 1024, Tmax {TMAX}, bf16, graph replay, best of {REPS}, forms alternating; "
      f"two rows per block {'on' if pair else 'off (PLANK_DECODE_MQ_PAIR=0)'})", flush=True)
dm = bench.apply_gains(bench.build("bf16", 1025, TMAX, 0.0), bench.DECODE_GAINS).eval()
dm._ensure_handle()
dm._refresh_shadow()


def once(dec, batch):
    """(seconds of begin, seconds per step) of one decode of TMAX steps."""
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.begin(batch, TMAX)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        dec.steps(TMAX)
        torch.cuda.synchronize()
    return t1 - t0, (time.perf_counter() - t1) / TMAX


for mode, B, N in shapes:
    db = synth_batch(B, spec_for("decode"), seed=7, device="cuda")
    db.pop("name")
    db = dm.prepare_batch(db)
    make = (lambda share: SampleDecoder(dm, N, temperature=0.8, top_k=50, top_p=0.95, seed=1, use_graph=True, strict_graph=True,
                                        share_encoder=share)) if mode == "s" else \
           (lambda share: BeamDecoder(dm, N, use_graph=True, strict_graph=True, share_encoder=share))
    if census is not None:
        once(make(census == "on"), db)
        print(f"census: one decode of B {B} x {N}, Tmax {TMAX}, share_encoder {census}")
        break
    decs = [make(False), make(True)]
    for d in decs:
        once(d, db)                                    # (the first run captures the graph)
    best = [[float("inf")] * 2 for _ in decs]
    for _ in range(REPS):
        for i, d in enumerate(decs):
            best[i] = [min(a, b) for a, b in zip(best[i], once(d, db))]
    (b0, s0), (b1, s1) = best
    what = "sampling" if mode == "s" else "beam search"
    print(f"{what} B {B} x {'N' if mode == 's' else 'K'} {N} ({B * N} rows): step off {s0 * 1e3:.3f} ms, on {s1 * 1e3:.3f} ms (ratio "
          f"{s1 / s0:.3f}); begin off {b0 * 1e3:.2f} ms, on {b1 * 1e3:.2f} ms (ratio {b1 / b0:.3f})", flush=True)

if not decode_only:
    model = bench.apply_gains(bench.build("bf16", 1025, TMAX, 0.0), bench.DECODE_GAINS).train()
    batch = synth_batch(16, spec_for("headline"), seed=7, device="cuda")
    batch.pop("name")
    batch = model.prepare_batch(batch)
    grammar = plank_grammar()

    def whole(N, share):
        for p in model._params.values():
            p.grad = None
        model.seq_train_step(batch, N, temperature=1.0, top_k=50, top_p=0.95, seed=3, objective="reinforce", baseline="mean", nll_weight=0.5,
                             constraint=grammar, share_encoder=share)["loss"].backward()

    for N in (4, 8):
        fns = [lambda: whole(N, False), lambda: whole(N, True)]
        for fn in fns:
            fn()
        best = [float("inf")] * 2
        for _ in range(REPS):
            for i, fn in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                best[i] = min(best[i], time.perf_counter() - t0)
        print(f"seq_train_step + backward B 16 x N {N}: off {best[0] * 1e3:.2f} ms, on {best[1] * 1e3:.2f} ms (ratio {best[1] / best[0]:.3f})",
              flush=True)
