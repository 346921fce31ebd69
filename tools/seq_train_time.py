"""What a sequence-level training step costs, in one process at the headline model (d 512, 6 + 6 layers, S 1024,
T 128, bf16, grammar-constrained sampling so that rows end like a trained model's):

1. `pa_sequence_batch` alone against the same work with torch ops and the host F1 (tests/seq_train_reference.py's rules on device
   tensors: a read-back of the counts, `prf_from_counts`, the weights in numpy, an upload, and torch ops for the rows) - alternating,
   best of REPS, from the buffers of one sampled decode;
2. sampling, matching, batch build and train step (forward + backward) as shares of one `seq_train_step`, each stage synchronised on
   its own (so the shares add up to a little more than the unsynchronised step, which is timed too);
3. one `seq_train_step` + backward against a plain `train_step` + backward at `B * G` rows.
`python tools/seq_train_time.py [N ...]` (default N: 4 8; B 16)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import bench
import seq_train_reference as R
from plankassembly_amd import ops
from plankassembly_amd.data import spec_for, synth_batch
from plankassembly_amd.decode import _repeat_batch, plank_grammar

REPS, B, NLL_WEIGHT = 5, 16, 0.5
sizes = [int(a) for a in sys.argv[1:]] or [4, 8]
assert torch.cuda.is_available(), "tools/seq_train_time.py measures on the GPU"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def best_of(fns):
    """Best of REPS for each function, the functions alternating inside every repetition."""
    best = [float("inf")] * len(fns)
    for fn in fns:
        fn()
    for _ in range(REPS):
        for i, fn in enumerate(fns):
            best[i] = min(best[i], timed(fn)[0])
    return best


def torch_batch(tokens, attach, first_end, counts, truth, label, N, nll_weight):
    """The batch build without the kernel: counts to the host, F1 and weights there, weights back, rows with torch ops."""
    rows, Tmax = tokens.shape
    Bq, T = truth.shape
    reward = R.rewards(counts.cpu().numpy()).reshape(Bq, N)
    w = np.stack([R.reinforce_weights(r, "mean") for r in reward])
    G = N + 1
    weight = torch.from_numpy(np.concatenate([w, np.full((Bq, 1), nll_weight, dtype=np.float32)], 1).reshape(-1)).cuda()
    L = torch.where(first_end >= 0, first_end + 1, torch.full_like(first_end, Tmax)).long()
    live = torch.arange(T, device=tokens.device)[None, :] < L[:, None]
    pad = torch.full((rows, T), R.PAD, dtype=torch.int64, device=tokens.device)
    value, lab = pad.clone(), pad.clone()
    value[:, :Tmax] = tokens
    lab[:, :Tmax] = torch.where(attach >= 0, attach + R.VOCAB, tokens)
    value, lab = torch.where(live, value, pad), torch.where(live, lab, pad)
    ov = torch.cat([value.view(Bq, N, T), truth[:, None]], 1).reshape(Bq * G, T)
    ol = torch.cat([lab.view(Bq, N, T), label[:, None]], 1).reshape(Bq * G, T)
    om = torch.cat([~live.view(Bq, N, T), (truth == R.PAD)[:, None]], 1).reshape(Bq * G, T)
    return ov, ol, om, weight, torch.from_numpy(reward).cuda()


print(f"# tools/seq_train_time.py ({torch.cuda.get_device_name(0)}; B {B}, S 1024, T 128, bf16, headline model with the decode gains; "
      f"best of {REPS}, alternatives alternating in one process)")
model = bench.apply_gains(bench.build("bf16", 1025, 128, 0.0), bench.DECODE_GAINS).train()
batch = synth_batch(B, spec_for("headline"), seed=7, device="cuda")
batch.pop("name")
batch = model.prepare_batch(batch)
grammar = plank_grammar()
for N in sizes:
    kw = dict(temperature=1.0, top_k=50, top_p=0.95, seed=3, objective="reinforce", baseline="mean", nll_weight=NLL_WEIGHT,
              constraint=grammar)
    G = N + 1
    sb = model.sequence_batch(batch, N, **kw)
    dec = model._mode_decoders[("sample", N, 1.0, 50, 0.95, 0.0)]
    tokens, attach, first_end = dec._lanes[0].buffers(B * N, 128)
    scores, counts = dec._scores(B * N), sb["counts"]
    truth, label = batch["output_value"], batch["output_label"]
    args = (tokens, attach, first_end, scores, counts, truth, label)
    okw = dict(num_samples=N, vocab_size=R.VOCAB, end_token=R.END, pad_token=R.PAD, baseline="mean", nll_weight=NLL_WEIGHT)
    a, b = ops.sequence_batch(*args, **okw), torch_batch(tokens, attach, first_end, counts, truth, label, N, NLL_WEIGHT)
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    t_kernel, t_torch = best_of([lambda: ops.sequence_batch(*args, **okw),
                                 lambda: torch_batch(tokens, attach, first_end, counts, truth, label, N, NLL_WEIGHT)])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        ops.sequence_batch(*args, **okw)
    e1.record()
    torch.cuda.synchronize()
    print(f"B {B} x N {N}: batch build, one launch {t_kernel * 1e6:.1f} us per call (host-timed, output allocation included; "
          f"{e0.elapsed_time(e1) / 50 * 1e3:.1f} us between HIP events over 50 back-to-back calls), torch ops + host F1 "
          f"{t_torch * 1e6:.1f} us, ratio {t_torch / t_kernel:.1f} x; outputs equal {same}; mean reward "
          f"{float(sb['reward'].mean()):.3f}, rows ended {int((first_end >= 0).sum())} of {B * N}", flush=True)

    # ---- the stages of one step, each synchronised on its own
    pairs = model._seq_pairs(B, N, tokens.device)

    def stage_sample():
        with torch.no_grad():
            return dec.run_device(batch, seed=3, constraint=grammar)

    def stage_match():
        return ops.plank_match(tokens, truth, pairs, end_token=R.END, filter_a=True, filter_b=False, threshold=0.5, check_pairs=False)

    def stage_build():
        out = ops.sequence_batch(*args, **okw)
        rep = _repeat_batch({k: v for k, v in batch.items() if k.startswith("input_")}, G)
        rep.update(output_value=out[0], output_label=out[1], output_mask=out[2], loss_weight=out[3], _n_valid=batch["_pack"][2] * G)
        return model.prepare_batch(rep)

    def zero():
        for p in model._params.values():
            p.grad = None

    def stage_train(b=None):
        zero()
        model.train_step(sb if b is None else b)["loss"].backward()

    def whole():
        zero()
        model.seq_train_step(batch, N, **kw)["loss"].backward()

    plain = _repeat_batch({k: v for k, v in batch.items() if not k.startswith("_")}, G)
    plain = model.prepare_batch(plain)
    t_s, t_m, t_b, t_t, t_w, t_p = best_of([stage_sample, stage_match, stage_build, stage_train, whole, lambda: stage_train(plain)])
    total = t_s + t_m + t_b + t_t
    print(f"B {B} x N {N}: seq_train_step + backward {t_w * 1e3:.2f} ms; stages sampled decode {t_s * 1e3:.2f} ms "
          f"({t_s / total:.1%}), matching {t_m * 1e3:.3f} ms ({t_m / total:.2%}), batch build with the input repeat and packing "
          f"{t_b * 1e3:.3f} ms ({t_b / total:.2%}), train step + backward on {B * G} rows {t_t * 1e3:.2f} ms ({t_t / total:.1%}); "
          f"plain train_step + backward on {B * G} ground-truth rows {t_p * 1e3:.2f} ms: ratio {t_w / t_p:.2f} x", flush=True)
