"""Scoring decoded programs on the host against on the device, in one process.

1. Per batch of B decoded drawings (device tensors, programs of 10 - 20 planks, rows of 128 tokens): the host path of the validation
   hook - `PlankModel._eval_dict` (two `parse_sequence` per drawing) and the `validation_step` loop (`_valid_pred`, D2H,
   `HungarianMatcher`) - against `DevicePlankScorer.add_batch` plus its share of `means()` (one read-back for `BATCHES` batches).
   Host and device alternate, best of `REPS`; the two paths' means are compared for equality in the same run.
2. The matching kernel alone, between HIP events, at 256 pairs (one batch against its truth) and 448 pairs (16 x 8 samples pairwise).
3. `PlankModel.sample(select="consensus")` against `select=None`, B 16 x N 8, the bench decode model under the plank grammar.
`python tools/match_time.py [B ...] [--no-sample]` (default B: 16 64 256)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import match_reference as R
from plankassembly_amd import metric as M
from plankassembly_amd import ops
from plankassembly_amd.trainer import Trainer

REPS, BATCHES, END = 5, 8, 512
args = sys.argv[1:]
sizes = [int(a) for a in args if not a.startswith("--")] or [16, 64, 256]
assert torch.cuda.is_available(), "tools/match_time.py measures on the GPU"


def free_planks(rng, n):
    """Boxes with free integer coordinates in the 9-bit vocabulary (no lattice: a pair at IoU == 0.5 exactly is rare)."""
    lo = rng.integers(0, 400, size=(n, 3))
    return np.concatenate([lo, lo + rng.integers(5, 112, size=(n, 3))], axis=1).astype(np.int64)


def programs(B, seed, lattice=False):
    """B prediction / truth rows of 10 - 20 planks each: about 60 % of a prediction's planks are copies of the truth's, a third of
    them with one face moved.  ``lattice``: the boxes of the tests' tie-heavy family (8-lattice: exact halves are common)."""
    rng = np.random.default_rng(seed)
    pred, truth = [], []
    for _ in range(B):
        if lattice:
            gt = R.random_planks(rng, int(rng.integers(10, 21)), jitter=False)
            pr = R.random_planks(rng, int(rng.integers(10, 21)))
        else:
            gt, pr = free_planks(rng, int(rng.integers(10, 21))), free_planks(rng, int(rng.integers(10, 21)))
        for i in range(len(pr)):
            if rng.random() < 0.6:
                pr[i] = gt[rng.integers(0, len(gt))]
                if rng.random() < 0.3:
                    pr[i, rng.integers(0, 3)] += (8 if lattice else 3) * int(rng.integers(-1, 2))
        pred.append(pr); truth.append(gt)
    return torch.from_numpy(R.rows_of(pred, 128)).cuda(), torch.from_numpy(R.rows_of(truth, 128)).cuda()


class _Parser:
    """The two attributes `PlankModel.parse_sequence` / `_eval_dict` read: the timing needs no weights."""
    from plankassembly_amd.models import PlankModel as _P
    token, num_output_dof = type("T", (), {"END": END})(), 6
    parse_sequence, _eval_dict = _P.parse_sequence, _P._eval_dict


def host_batches(batches):
    scorer, parser = M.PlankScorer(0.5), _Parser()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for samples, truth in batches:
        out = parser._eval_dict({"output_value": truth}, samples, samples)
        for pred, gt in zip(out["predicts"], out["groundtruths"]):
            scorer.add(Trainer._valid_pred(None, pred), gt)
    means = scorer.means(sync=False)
    return (time.perf_counter() - t0) / len(batches), means


def device_batches(batches):
    scorer = M.DevicePlankScorer(0.5, END)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for samples, truth in batches:
        scorer.add_batch(samples, truth)
    means = scorer.means(sync=False)
    return (time.perf_counter() - t0) / len(batches), means, scorer.fallbacks


print(f"# tools/match_time.py ({torch.cuda.get_device_name(0)}; best of {REPS}, host and device alternating in one process; "
      f"{BATCHES} batches per epoch end)")
for B, lattice in [(B, lat) for lat in (False, True) for B in sizes]:
    batches = [programs(B, 100 + i, lattice) for i in range(BATCHES)]
    host_batches(batches[:1]); device_batches(batches[:1])                     # warm-up of both paths
    h = d = float("inf")
    for _ in range(REPS):
        th, mh = host_batches(batches)
        td, md, fb = device_batches(batches)
        assert md == mh, (md, mh)
        h, d = min(h, th), min(d, td)
    print(f"scoring B {B}{' (8-lattice boxes, tie-heavy)' if lattice else ''}: host path {h * 1e3:.2f} ms/batch ({h / B * 1e6:.0f} us/drawing), device scorer {d * 1e3:.3f} ms/batch "
          f"({fb} of {B * BATCHES} drawings re-scored on the host for ties), ratio {h / d:.1f} x; means equal {mh == md}", flush=True)

for n_pairs, what in ((256, "256 rows against their truth"), (448, "16 x 8 samples pairwise")):
    a, b = programs(256, 7)
    pairs = None
    if n_pairs == 448:
        from plankassembly_amd.decode import _consensus_pairs
        a = b = a[:128].contiguous()
        pairs = _consensus_pairs(16, 8, a.device)[0]
    kw = dict(end_token=END, filter_a=True, filter_b=pairs is not None, threshold=0.5, check_pairs=False)
    for _ in range(3):
        ops.plank_match(a, b, pairs, **kw)
    best = float("inf")
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            ops.plank_match(a, b, pairs, **kw)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / 50)
    print(f"kernel, {n_pairs} pairs ({what}), 128-token rows: {best * 1e3:.1f} us per launch between HIP events "
          f"(50 back-to-back launches: launch cadence included)", flush=True)

if "--no-sample" not in args:
    import bench
    from plankassembly_amd.data import spec_for, synth_batch
    from plankassembly_amd.decode import plank_grammar
    dm = bench.apply_gains(bench.build("bf16", 1025, 128, 0.0), bench.DECODE_GAINS).eval()
    db = synth_batch(16, spec_for("decode"), seed=7, device="cuda")
    db.pop("name")
    db = dm.prepare_batch(db)

    def sample(select):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = dm.sample(db, 8, temperature=0.8, top_k=50, top_p=0.95, seed=3, constraint=plank_grammar(), parse=False, select=select)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    sample(None); sample("consensus")
    t = {None: float("inf"), "consensus": float("inf")}
    for _ in range(REPS):
        for sel in t:
            dt, out = sample(sel)
            t[sel] = min(t[sel], dt)
    f1 = out["consensus_f1"]
    print(f"sample B 16 x N 8, Tmax 128, bf16, grammar on, parse=False: select=None {t[None] * 1e3:.2f} ms, select='consensus' "
          f"{t['consensus'] * 1e3:.2f} ms (+{(t['consensus'] - t[None]) * 1e3:.2f} ms, ratio {t['consensus'] / t[None]:.4f}); "
          f"consensus_f1 of the winners {float(f1.max(1).values.mean()):.3f}, index != 0 in "
          f"{int((out['consensus_index'] != 0).sum())} of 16 drawings", flush=True)
