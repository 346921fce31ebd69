"""Sequence-level training on the GPU (csrc/seqtrain.hip, include/plank_hip.h pa_sequence_batch, ops.sequence_batch,
SampleDecoder.run_device, PlankModel.sequence_batch / seq_train_step, the trainer's SEQ_TRAIN block) against
the numpy restatement tests/seq_train_reference.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import match_reference as MR
import seq_train_reference as R
from decode_logprob_cases import F32_TOKEN_BOUND
from test_beam_gpu import TOKEN, dev, make

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"b3n5t13": (3, 5, 13, 13), "b1n2t36": (1, 2, 36, 36), "b4n64t7T130": (4, 64, 7, 130), "b2n1t9T11": (2, 1, 9, 11)}
MODES = {"none": ("reinforce", "none"), "mean": ("reinforce", "mean"), "greedy": ("reinforce", "greedy"), "risk": ("risk", "none")}
ALPHA = 0.5
_INPUTS = {}


def inputs(shape):
    """One synthetic input set per shape, shared by every mode (first_end -1 / 0 / Tmax - 1, n_a == 0, n_b == 0, ties > 0; the
    drawing without ground-truth planks and, where there is a third one, drawing 2 have all-equal rewards)."""
    if shape not in _INPUTS:
        B, N, Tmax, T = SHAPES[shape]
        _INPUTS[shape] = R.synthetic(B, N, Tmax, T, seed=sum(SHAPES[shape]), equal_drawing=2 if B > 2 else None)
    return _INPUTS[shape]


def gpu_batch(x, N, objective, baseline, alpha, nll_weight):
    from plankassembly_amd import ops
    d = {k: torch.from_numpy(v).cuda() for k, v in x.items()}
    out = ops.sequence_batch(d["tokens"], d["attach"], d["first_end"], d["scores"], d["counts"], d["gt_value"], d["gt_label"],
                             num_samples=N, vocab_size=R.VOCAB, end_token=R.END, pad_token=R.PAD, objective=objective,
                             baseline=baseline, alpha=alpha, nll_weight=nll_weight,
                             base_counts=d["base_counts"] if baseline == "greedy" else None)
    assert [t.dtype for t in out] == [torch.int64, torch.int64, torch.bool, torch.float32, torch.float32] and all(t.is_cuda for t in out)
    return dict(zip(("out_value", "out_label", "out_mask", "out_weight", "reward"), (t.cpu().numpy() for t in out)))


def assert_batch_equal(got, want, objective, where):
    """Integer outputs and rewards bit for bit; weights bit for bit under reinforce, within one f32 ulp of the reference under risk.
    Returns the largest weight difference in ulps of the reference."""
    for k in ("out_value", "out_label"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (where, k)
    assert np.array_equal(got["out_mask"].astype(np.uint8), want["out_mask"]), where
    assert np.array_equal(got["reward"].view(np.uint32), want["reward"].view(np.uint32)), where
    gw, ww = got["out_weight"], want["out_weight"]
    assert gw.shape == ww.shape and gw.dtype == np.float32 and ww.dtype == np.float32
    if objective == "reinforce":
        assert np.array_equal(gw.view(np.uint32), ww.view(np.uint32)), (where, gw, ww)
        return 0.0
    ulp = np.spacing(np.abs(ww))                                    # one f32 ulp of the reference value
    diff = np.abs(gw.astype(np.float64) - ww.astype(np.float64))
    assert bool(np.all(diff <= ulp)), (where, gw[diff > ulp], ww[diff > ulp])
    return float(np.max(diff / ulp))


# ------------------------------------------------------------------------------------------------ 1. the kernel
# every shape in every mode with and without the ground-truth row; one sample per drawing has no "others": no mean baseline there
KERNEL_CASES = [(s, m, w) for s in SHAPES for m in MODES for w in (0.0, 0.5) if not (SHAPES[s][1] == 1 and m == "mean")]


@pytest.mark.parametrize("shape,mode,nll_weight", KERNEL_CASES)
def test_kernel_equals_the_restatement(shape, mode, nll_weight):
    B, N, Tmax, T = SHAPES[shape]
    objective, baseline = MODES[mode]
    x = inputs(shape)
    want = R.sequence_batch(x["tokens"], x["attach"], x["first_end"], x["scores"], x["counts"], x["gt_value"], x["gt_label"], N,
                            objective, baseline, ALPHA, nll_weight, x["base_counts"] if baseline == "greedy" else None)
    got = gpu_batch(x, N, objective, baseline, ALPHA, nll_weight)
    worst = assert_batch_equal(got, want, objective, (shape, mode, nll_weight))
    G = N + (nll_weight != 0)
    assert got["out_value"].shape == (B * G, T) and got["out_weight"].shape == (B * G,) and got["reward"].shape == (B, N)
    print(f"{shape} {mode} nll_weight {nll_weight}: largest weight difference {worst:.3f} ulp of the reference")
    # the inputs really hold the edge cases
    fe, c = x["first_end"], x["counts"]
    assert fe[0] == -1 and (B * N < 2 or fe[1] == 0) and c[0, 1] == 0 and c[0, 3] > 0 and (B < 2 or bool((c[N:2 * N, 2] == 0).all()))
    if baseline == "mean":
        flat = want["out_weight"].reshape(B, G)[:, :N]
        equal = [b for b in range(B) if len(set(want["reward"][b].tolist())) == 1]
        assert (equal or B == 1) and all(np.array_equal(flat[b].view(np.uint32), np.zeros(N, dtype=np.uint32)) for b in equal)   # exact +0.0
        assert bool((got["out_weight"].reshape(B, G)[equal, :N].view(np.uint32) == 0).all())


def test_strided_inputs_are_read_in_place():
    """Column slices of wider buffers (row stride > Tmax, > T), as a decoder's or a dataset's views can be."""
    from plankassembly_amd import ops
    B, N, Tmax, T = SHAPES["b3n5t13"]
    x = inputs("b3n5t13")
    wide = {k: torch.full((x[k].shape[0], x[k].shape[1] + 5), -3, dtype=torch.int64).cuda() for k in ("tokens", "attach", "gt_value", "gt_label")}
    for k, t in wide.items():
        t[:, :x[k].shape[1]] = torch.from_numpy(x[k]).cuda()
    d = {k: torch.from_numpy(v).cuda() for k, v in x.items()}
    out = ops.sequence_batch(wide["tokens"][:, :Tmax], wide["attach"][:, :Tmax], d["first_end"], d["scores"], d["counts"],
                             wide["gt_value"][:, :T], wide["gt_label"][:, :T], num_samples=N, vocab_size=R.VOCAB, end_token=R.END,
                             pad_token=R.PAD, baseline="mean", nll_weight=0.5)
    got = dict(zip(("out_value", "out_label", "out_mask", "out_weight", "reward"), (t.cpu().numpy() for t in out)))
    want = R.sequence_batch(x["tokens"], x["attach"], x["first_end"], x["scores"], x["counts"], x["gt_value"], x["gt_label"], N,
                            "reinforce", "mean", 1.0, 0.5)
    assert_batch_equal(got, want, "reinforce", "strided")


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_every_refusal_returns_einval_and_launches_nothing():
    from plankassembly_amd import _lib as L
    from plankassembly_amd import ops
    B, N, Tmax, T = 2, 3, 8, 10
    x = {k: torch.from_numpy(v).cuda() for k, v in R.synthetic(B, N, Tmax, T, seed=5).items()}
    G = N + 1
    outs = {"out_value": torch.full((B * G, T), -7, dtype=torch.int64), "out_label": torch.full((B * G, T), -7, dtype=torch.int64),
            "out_mask": torch.full((B * G, T), 7, dtype=torch.uint8), "out_weight": torch.full((B * G,), -7.0),
            "reward": torch.full((B, N), -7.0)}
    outs = {k: v.cuda() for k, v in outs.items()}

    def args(**over):
        a = dict(tokens=x["tokens"].data_ptr(), attach=x["attach"].data_ptr(), first_end=x["first_end"].data_ptr(),
                 scores=x["scores"].data_ptr(), counts=x["counts"].data_ptr(), base_counts=x["base_counts"].data_ptr(),
                 gt_value=x["gt_value"].data_ptr(), gt_label=x["gt_label"].data_ptr(), sample_stride=Tmax, gt_stride=T,
                 B=B, N=N, Tmax=Tmax, T=T, objective=0, baseline=1, alpha=1.0, nll_weight=0.5, vocab_size=R.VOCAB, end_token=R.END,
                 pad_token=R.PAD, pad_=0, **{k: v.data_ptr() for k, v in outs.items()})
        a.update(over)
        return L.SeqBatchArgs(**a)

    def call(**over):
        a = args(**over)
        return L.lib().pa_sequence_batch(C.byref(a), L.stream())

    refusals = [dict(tokens=None), dict(attach=None), dict(first_end=None), dict(scores=None), dict(counts=None), dict(gt_value=None),
                dict(gt_label=None), dict(out_value=None), dict(out_label=None), dict(out_mask=None), dict(out_weight=None),
                dict(reward=None),                                                        # a null required pointer
                dict(N=0), dict(N=65), dict(N=-1),                                        # N outside [1, 64]
                dict(N=1, baseline=1),                                                    # baseline mean with N < 2
                dict(baseline=2, base_counts=None),                                       # baseline greedy without base_counts
                dict(Tmax=T + 1),                                                         # Tmax > T
                dict(objective=1, alpha=float("nan")), dict(objective=1, alpha=float("inf")), dict(objective=1, alpha=0.0),
                dict(objective=1, alpha=-1.0),                                            # alpha under risk
                dict(sample_stride=-1), dict(gt_stride=-1),                               # a negative stride
                dict(objective=2), dict(baseline=3), dict(B=-1), dict(nll_weight=float("nan"))]
    for over in refusals:
        rc = call(**over)
        assert rc == -1, (over, rc)                                                       # PA_EINVAL
        with pytest.raises(L.PlankHipError, match="PA_EINVAL"):
            L.check(rc, "pa_sequence_batch")
    assert L.lib().pa_sequence_batch(None, L.stream()) == -1
    assert call(B=0) == 0                                                                 # nothing to do, nothing launched
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == (7 if k == "out_mask" else -7)).all()), k                      # every buffer still as it was filled
    # alpha is not looked at under reinforce, base_counts may be NULL without the greedy baseline: these run
    assert call(alpha=float("nan"), base_counts=None) == 0
    torch.cuda.synchronize()
    assert not bool((outs["out_value"] == -7).any()) and not bool((outs["out_weight"] == -7).any())
    # the Python layer refuses the same before the call, by type and by value
    kw = dict(num_samples=N, vocab_size=R.VOCAB, end_token=R.END, pad_token=R.PAD)
    pos = [x[k] for k in ("tokens", "attach", "first_end", "scores", "counts", "gt_value", "gt_label")]
    with pytest.raises(TypeError, match="first_end"):
        ops.sequence_batch(*pos[:2], x["first_end"].long(), *pos[3:], **kw)
    with pytest.raises(TypeError, match="tokens"):
        ops.sequence_batch(x["tokens"].cpu(), *pos[1:], **kw)
    with pytest.raises(ValueError, match="rows"):
        ops.sequence_batch(*pos, **dict(kw, num_samples=2))
    with pytest.raises(ValueError, match="Tmax"):
        ops.sequence_batch(*pos[:5], x["gt_value"][:, :Tmax - 1], x["gt_label"][:, :Tmax - 1], **kw)
    with pytest.raises(ValueError, match="baseline"):
        ops.sequence_batch(*pos, baseline="median", **kw)
    with pytest.raises(ValueError, match="base_counts"):
        ops.sequence_batch(*pos, baseline="greedy", **kw)
    with pytest.raises(ValueError, match="alpha"):
        ops.sequence_batch(*pos, objective="risk", baseline="none", alpha=0.0, **kw)


# ------------------------------------------------------------------------------------------------ 3. run_device
def test_run_device_is_run_before_the_ranking(small_fixture):
    import plankassembly_amd.decode as D
    sd, batch, _ = small_fixture
    m = make(sd)
    N = 4
    dec = D.SampleDecoder(m, N, temperature=1.5, seed=3)
    with torch.no_grad():
        r = {k: v.cpu() for k, v in dec.run(dev(batch)).items()}
        tok, att, fe, sc = dec.run_device(dev(batch))
        assert tok.is_cuda and tok.shape == (4 * N, 36) and att.shape == tok.shape and fe.dtype == torch.int32 and sc.dtype == torch.float32
        tok, att, fe, sc = tok.cpu(), att.cpu(), fe.cpu().long(), sc.cpu()
    n = r["sample_tokens"].shape[2]
    order = torch.sort(sc.view(4, N), dim=1, descending=True, stable=True).indices          # run's ranking (length_penalty 0)
    pick = lambda t: t.view(4, N, -1)[:, :, :n].gather(1, order[:, :, None].expand(4, N, n))
    assert torch.equal(pick(tok), r["sample_tokens"]) and torch.equal(pick(att), r["sample_attach"])
    assert torch.equal(sc.view(4, N).gather(1, order).view(torch.int32), r["scores"].view(torch.int32))
    lengths = torch.where(fe >= 0, fe + 1, torch.full_like(fe, 36)).view(4, N).gather(1, order)
    assert torch.equal(lengths, r["lengths"])
    # a seed of the call's own, as run takes it
    with torch.no_grad():
        other = dec.run_device(dev(batch), seed=4)[0].cpu()
        again = dec.run_device(dev(batch), seed=3)[0].cpu()
    assert torch.equal(again, tok) and not torch.equal(other, tok)


# ------------------------------------------------------------------------------------------------ 4. sequence_batch
def decoder_buffers(m, N, B, temperature):
    dec = m._mode_decoders[("sample", N, float(temperature), 0, 1.0, 0.0)]
    Tmax = dec._lanes[0].key[2]
    tok, att, fe = dec._lanes[0].buffers(B * N, Tmax)
    return tok.cpu().numpy(), att.cpu().numpy(), fe.cpu().numpy(), dec._scores(B * N).cpu().numpy()


_FITTED = {}


def fitted(small_fixture):
    """(state dict, batch) of the small model after 200 plain steps on the fixture's inputs with a ground truth of VALID planks
    (tests/match_reference.py's lattice boxes).  The fixture's own ground truth is random tokens - inverted boxes, IoU 0 even against
    themselves, so every reward on it is 0; on this batch samples at temperature 1.5 earn rewards all over [0, 1].  Fitted once."""
    if not _FITTED:
        from plankassembly_amd.optim import FusedAdam
        sd, batch, _ = small_fixture
        rng = np.random.default_rng(24)
        rows = torch.from_numpy(MR.rows_of([MR.random_planks(rng, n, jitter=False) for n in (5, 4, 5, 3)], 36))
        batch = dict(batch, output_value=rows, output_label=rows.clone(), output_mask=rows == TOKEN.PAD)
        m = make(sd).train()
        gb = m.prepare_batch(batch)
        opt = FusedAdam(m, lr=2e-3)
        for _ in range(200):
            opt.zero_grad()
            m(gb)["loss"].backward()
            opt.step()
        _FITTED["sd"] = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        _FITTED["batch"] = batch
    return _FITTED["sd"], _FITTED["batch"]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("N", [4, 3])
def test_sequence_batch_on_the_small_fixture(small_fixture, N, mode):
    sd, batch, _ = small_fixture
    check_sequence_batch(sd, batch, N, mode)


@pytest.mark.parametrize("mode", list(MODES))
def test_sequence_batch_with_rewards_that_differ(small_fixture, mode):
    sd, batch = fitted(small_fixture)
    reward = check_sequence_batch(sd, batch, 4, mode)
    assert len(set(reward.reshape(-1).tolist())) >= 4 and 0.0 < reward.mean() < 1.0, reward.tolist()


def check_sequence_batch(sd, batch, N, mode):
    objective, baseline = MODES[mode]
    m = make(sd)
    gb = dev(batch)
    nll_weight = 0.5 if N == 3 else 0.0
    sb = m.sequence_batch(gb, N, temperature=1.5, seed=3, objective=objective, baseline=baseline, alpha=ALPHA, nll_weight=nll_weight)
    tok, att, fe, sc = decoder_buffers(m, N, 4, 1.5)                                       # the decoder's own buffers, still in place
    truth, label = batch["output_value"].numpy(), batch["output_label"].numpy()
    counts = MR.plank_match(tok, truth, [(r, r // N) for r in range(4 * N)], end_token=TOKEN.END, filter_a=True, filter_b=False,
                            threshold=0.5)
    assert sb["counts"].dtype == torch.int32 and np.array_equal(sb["counts"].cpu().numpy(), counts)
    base = None
    if baseline == "greedy":
        with torch.no_grad():
            greedy = m.eval_step(gb, parse=False)["samples"].cpu().numpy()
        base = MR.plank_match(greedy, truth, end_token=TOKEN.END, filter_a=True, filter_b=False, threshold=0.5)
    want = R.sequence_batch(tok, att, fe, sc, counts, truth, label, N, objective, baseline, ALPHA, nll_weight, base, vocab=514, pad=TOKEN.PAD)
    got = {"out_value": sb["output_value"], "out_label": sb["output_label"], "out_mask": sb["output_mask"], "out_weight": sb["loss_weight"],
           "reward": sb["reward"]}
    assert sb["output_mask"].dtype == torch.bool and all(v.is_cuda for v in got.values())
    worst = assert_batch_equal({k: v.cpu().numpy() for k, v in got.items()}, want, objective, (N, mode))
    print(f"N {N} {mode}: rewards {want['reward'].tolist()}, largest weight difference {worst:.3f} ulp")
    G = N + (nll_weight != 0)
    assert np.array_equal(sb["sample_scores"].cpu().numpy().view(np.uint32), sc.reshape(4, N).view(np.uint32))
    for k in ("input_value", "input_pos", "input_coord", "input_view", "input_type", "input_mask"):
        assert torch.equal(sb[k].cpu(), batch[k].repeat_interleave(G, dim=0)), k
    assert sb["output_value"].shape == (4 * G, 36) and sb["loss_weight"].shape == (4 * G,)
    return want["reward"]


def test_sequence_batch_needs_six_output_dof(small_fixture):
    sd, batch, _ = small_fixture
    m = make(sd)
    m.num_output_dof = 5
    with pytest.raises(ValueError, match="six"):
        m.sequence_batch(dev(batch), 2)
    m.num_output_dof = 6
    with pytest.raises(ValueError, match="objective"):
        m.sequence_batch(dev(batch), 2, objective="mle")


# ------------------------------------------------------------------------------------------------ 5. the train step
def no_grads(m):
    for p in m._params.values():
        p.grad = None


def long_way_batch(m, batch, sb, N, **kw):
    """The restatement's batch, uploaded: what seq_train_step must have trained on, built on the host from the decoder's buffers."""
    from plankassembly_amd.decode import _repeat_batch
    tok, att, fe, sc = decoder_buffers(m, N, 4, kw["temperature"])
    want = R.sequence_batch(tok, att, fe, sc, sb["counts"].cpu().numpy(), batch["output_value"].numpy(), batch["output_label"].numpy(), N,
                            kw["objective"], kw["baseline"], kw["alpha"], kw["nll_weight"], vocab=514, pad=TOKEN.PAD)
    G = N + (kw["nll_weight"] != 0)
    out = _repeat_batch({k: v for k, v in dev(batch).items() if k.startswith("input_")}, G)
    out.update(output_value=torch.from_numpy(want["out_value"]).cuda(), output_label=torch.from_numpy(want["out_label"]).cuda(),
               output_mask=torch.from_numpy(want["out_mask"]).cuda().bool(), loss_weight=torch.from_numpy(want["out_weight"]).cuda())
    return m.prepare_batch(out)


@pytest.mark.parametrize("which", ["fixture", "fitted"])
def test_seq_train_step_equals_the_long_way_round(small_fixture, which):
    sd, batch = small_fixture[:2] if which == "fixture" else fitted(small_fixture)
    N = 4
    kw = dict(temperature=1.5, seed=3, objective="reinforce", baseline="mean", alpha=1.0, nll_weight=0.5)
    m = make(sd).train()                                                                   # (dropout 0: a step is a function of its batch)
    out = m.seq_train_step(dev(batch), N, **kw)
    assert sorted(out) == ["accuracy", "batch", "loss", "nll", "reward"] and out["loss"].requires_grad
    out["loss"].backward()
    grads = m.flat_grads.clone()
    loss = out["loss"].item()
    assert out["reward"].item() == out["batch"]["reward"].mean().item() and 0.0 <= out["reward"].item() <= 1.0
    lw = long_way_batch(m, batch, out["batch"], N, **kw)
    assert torch.equal(lw["loss_weight"].view(torch.int32), out["batch"]["loss_weight"].view(torch.int32))
    if which == "fitted":                                                                  # the sample rows really pull: weights of both signs
        w = out["batch"]["loss_weight"].view(4, N + 1)[:, :N]
        assert bool((w > 0).any()) and bool((w < 0).any()), w.tolist()
    runs = []
    for _ in range(2):                                                                     # the existing path, twice on the same batch
        no_grads(m)
        o = m.train_step(lw)
        o["loss"].backward()
        runs.append((o["loss"].item(), m.flat_grads.clone()))
    assert loss == runs[0][0] == runs[1][0], (loss, runs[0][0], runs[1][0])              # bit-identical loss
    repeat = float((runs[0][1] - runs[1][1]).abs().max())
    diff = float((grads - runs[0][1]).abs().max())
    print(f"flat_grads: existing path run to run {repeat!r}, seq_train_step against it {diff!r} (max |g| {float(grads.abs().max())!r})")
    if repeat == 0.0:
        assert torch.equal(grads.view(torch.int32), runs[0][1].view(torch.int32))
    else:
        assert diff <= 2 * repeat, (diff, repeat)
    assert float(grads.abs().max()) > 0


def test_second_step_samples_under_the_updated_weights(small_fixture):
    """The decode reads low-precision / transposed shadows of the weights: after a FusedAdam step the samples' log-likelihoods must be
    those of the new weights.  PlankModel.score (the forced greedy step, float64 sums of its per-token values) is the yardstick; the
    sampler's score is an f32 running sum of the same per-token values, each within the per-token bound of the parity tests."""
    from plankassembly_amd.optim import FusedAdam
    sd, batch, _ = small_fixture
    N, G = 3, 4
    kw = dict(temperature=1.5, objective="reinforce", baseline="mean", nll_weight=0.5)     # (the ground-truth row: an update whatever the rewards)
    m = make(sd).train()
    opt = FusedAdam(m, lr=1e-2)
    opt.zero_grad()
    first = m.seq_train_step(dev(batch), N, seed=1, **kw)
    first["loss"].backward()
    before = m.flat_params.clone()
    opt.step()
    assert not torch.equal(before, m.flat_params)
    opt.zero_grad()
    second = m.seq_train_step(dev(batch), N, seed=1, **kw)
    sb = second["batch"]
    rows = torch.tensor([b * G + n for b in range(4) for n in range(N)])                   # the sample rows of the expanded batch
    tokens = sb["output_value"].cpu()[rows]
    label = sb["output_label"].cpu()[rows]
    lengths = (~sb["output_mask"].cpu()[rows]).sum(1)
    attach = torch.where(label >= 514, label - 514, torch.full_like(label, -1))
    inputs_rep = {k: v[rows.cuda()] for k, v in sb.items() if k.startswith("input_")}
    m.eval()
    with torch.no_grad():
        sc = m.score(inputs_rep, tokens=tokens, attach=attach, lengths=lengths)
    got = sb["sample_scores"].cpu().reshape(-1)
    bound = F32_TOKEN_BOUND * lengths.double()
    diff = (got.double() - sc["scores"].double()).abs()
    print(f"sample scores against score(): largest difference {float(diff.max()):.3e}, bound per row {bound.tolist()}")
    assert bool(torch.isfinite(got).all()) and bool((diff <= bound).all()), (diff.tolist(), bound.tolist())
    # and the update was large enough to tell: under the weights of the first step the same samples score differently
    old = first["batch"]["sample_scores"].cpu().reshape(-1)
    assert not torch.equal(old, got)


# ------------------------------------------------------------------------------------------------ 6. the trainer
def small_hparams(**over):
    from test_trainer_surface import small_hparams as base
    hp = base(SYNTHETIC_SAMPLES=8, **over)
    hp["MODEL"].update(DROPOUT=0.0)
    return hp


def fit_two_steps(hp, step=None):
    """The loop of trainer.run for one epoch of two batches, on synthetic drawings; ``step``: what to call for a batch (default: the
    trainer's own training_step).  Returns (trainer, the two losses)."""
    from plankassembly_amd.trainer import Trainer
    torch.manual_seed(2022)
    t = Trainer(hp)
    t.model.cuda().train()
    opt = t.configure_optimizers()["optimizer"]
    losses = []
    for i, b in enumerate(t.train_dataloader()):
        b = t.model.prepare_batch(b)
        opt.zero_grad()
        loss = t.training_step(b, i) if step is None else step(t, b)
        loss.backward()
        opt.step()
        t.global_step += 1
        losses.append(loss.item())
    assert len(losses) == 2
    return t, losses


def test_trainer_without_the_block_is_the_parents_loop():
    def parent_step(t, b):                                                                 # training_step as it was: one call of the model
        outputs = t.model(b)
        assert sorted(outputs) == ["accuracy", "loss"]                                     # no nll key: the reference-parity calls
        return torch.mean(outputs["loss"])
    _, want = fit_two_steps(small_hparams(), parent_step)
    t, got = fit_two_steps(small_hparams())
    assert got == want and t._train_nll is None and t._train_reward is None, (got, want)


def test_trainer_with_a_seq_train_block(tmp_path, monkeypatch):
    import yaml
    from plankassembly_amd.trainer import Trainer, cli
    monkeypatch.chdir(tmp_path)
    with open(os.path.join(REPO, "configs", "train_complete.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["trainer"].update(max_epochs=1, check_val_every_n_epoch=5, devices=1)
    hp = small_hparams(SEQ_TRAIN={"NUM_SAMPLES": 3, "TEMPERATURE": 1.2, "NLL_WEIGHT": 0.5, "SEED": 11})
    cfg["model"]["hparams"] = hp
    path = tmp_path / "train_seq.yaml"
    path.write_text(yaml.safe_dump(cfg))
    mod = cli(Trainer, ["fit", "--config", str(path)])
    assert mod.global_step == 2 and mod.seq_train["step"]["num_samples"] == 3
    hist = {name: v for _, name, v in mod.logger.history}
    assert np.isfinite(hist["train/loss"]) and np.isfinite(hist["train/nll"]) and 0.0 <= hist["train/reward"] <= 1.0
    torch.manual_seed(int(cfg["seed_everything"]))
    fresh = Trainer(hp).model.state_dict()
    moved = [k for k, v in mod.model.state_dict().items() if not torch.equal(v.cpu(), fresh[k])]
    assert len(moved) > len(fresh) // 2, (len(moved), len(fresh))
