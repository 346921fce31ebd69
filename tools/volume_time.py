"""What the assembly volume costs, in one process.

1. The volume launch alone (`ops.plank_volume`), between HIP events, at 128 and 256 pairs of generated programs of 8 - 21 planks a
   side (rows of 132 tokens, the Tmax-128 decode), next to `ops.plank_match` on the same pairs; then one pair at 170 planks a
   side, the widest row the entry takes.
2. `PlankModel.sample(select="volume")` against `select=None` and `select="consensus"` at B 16 x N 8 and B 64 x N 4: Tmax 128,
   bf16, the bench decode model under the plank grammar, parse=False; the three alternate, best of `REPS`.
Every step runs under a time limit of its own (`LIMIT` seconds: a watchdog thread ends the process, whatever it is blocked in).
`python tools/volume_time.py [--no-sample]`."""
import faulthandler
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import volume_reference as R
from plankassembly_amd import ops

REPS, LIMIT, END = 5, 120, R.END
args = sys.argv[1:]
assert torch.cuda.is_available(), "tools/volume_time.py measures on the GPU"


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


def programs(n, length=132, size=256):
    """n pairs of program rows of 8 - 21 random planks each, coordinates of 8 bits."""
    rng = np.random.default_rng(33)
    rows = [[R.row_of([R.random_box(rng, size - 1, 4, 96) for _ in range(int(rng.integers(8, 22)))], length) for _ in range(n)]
            for _ in range(2)]
    return torch.from_numpy(np.stack(rows[0])).cuda(), torch.from_numpy(np.stack(rows[1])).cuda()


print(f"# tools/volume_time.py ({torch.cuda.get_device_name(0)}; best of {REPS}; every step under a limit of {LIMIT} s)")
for n_pairs in (128, 256):
    with step(f"volume {n_pairs}"):
        a, b = programs(n_pairs)
        c = ops.plank_volume(a, b, end_token=END).cpu().numpy()
        iou = R.scores(c)["volume_iou"]
        vol = between_events(lambda: ops.plank_volume(a, b, end_token=END))
        own = between_events(lambda: ops.plank_volume(a, None, end_token=END))
        match = between_events(lambda: ops.plank_match(a, b, end_token=END, filter_a=True, filter_b=True, threshold=0.5))
        print(f"volume, {n_pairs} pairs of generated programs (rows of 132 tokens, {c[:, 6:].mean():.1f} planks a side on average, "
              f"{c[:, 6:].max()} at most; mean IoU {iou.mean():.3f}): {vol:.1f} us per launch, without a b side {own:.1f} us, "
              f"pa_plank_match on the same pairs {match:.1f} us, between HIP events (50 back-to-back launches: launch cadence "
              f"included)", flush=True)

with step("volume 170 planks"):
    a, b = (torch.from_numpy(x).cuda() for x in R.ceiling_pairs())
    for i, name in enumerate(("dense random", "all disjoint", "all identical", "against an empty b")):
        us = between_events(lambda: ops.plank_volume(a[i:i + 1], b[i:i + 1], end_token=END), launches=10)
        print(f"volume, 1 pair at 170 planks a side (rows of 1026 tokens), {name}: {us:.1f} us per launch between HIP events", flush=True)

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

            t = {None: float("inf"), "consensus": float("inf"), "volume": float("inf")}
            outs = {}
            for sel in t:
                sample(sel)
            for _ in range(REPS):
                for sel in t:
                    dt, outs[sel] = sample(sel)
                    t[sel] = min(t[sel], dt)
            v, f = outs["volume"], outs["consensus"]
            print(f"sample B {B} x N {N}, Tmax 128, bf16, grammar on, parse=False: select=None {t[None] * 1e3:.2f} ms, 'consensus' "
                  f"{t['consensus'] * 1e3:.2f} ms (+{(t['consensus'] - t[None]) * 1e3:.2f} ms), 'volume' {t['volume'] * 1e3:.2f} ms "
                  f"(+{(t['volume'] - t[None]) * 1e3:.2f} ms, ratio {t['volume'] / t[None]:.4f}); mean volume_iou of the winners "
                  f"{float(v['volume_iou'].max(1).values.mean()):.4f}, volume_index != 0 in {int((v['volume_index'] != 0).sum())} of {B} "
                  f"drawings, mean self_overlap {float(v['self_overlap'].mean()):.4f}; consensus_f1 of the winners "
                  f"{float(f['consensus_f1'].max(1).values.mean()):.4f}, consensus_index != 0 in {int((f['consensus_index'] != 0).sum())}",
                  flush=True)
