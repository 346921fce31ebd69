"""The extended objective at model level: PlankModel(label_smoothing=), batch["loss_weight"] and
train_step(token_nll=) on the small fixture (d 64, 2+2 layers, T 36, dropout 0) against float64 autograd through oracle/plank_oracle.py,
the default model's calls, gradient accumulation, and a short fit that logs train/nll."""
import os
import types

import numpy as np
import pytest
import torch

import loss_ext_reference as R

pytestmark = pytest.mark.gpu

TOKEN = types.SimpleNamespace(END=512, PAD=513)
NEW_ENTRIES = ("pa_mixture_nll_fwd_ext", "pa_mixture_nll_bwd_ext", "pa_model_set_loss")
EPS = 0.1
WEIGHT = [1.25, 0.0, -0.5, 0.75]                                    # per drawing: one 0, one negative


def make(sd, dtype="f32", **kw):
    from plankassembly_amd.models import PlankModel
    m = PlankModel(64, 4, 128, 0.0, "relu", True, 2, 2, 3, 2, 4, 6, 65, 36, 514, TOKEN, compute_dtype=dtype, **kw)
    m.load_state_dict(sd)
    return m.cuda()


def to_dev(batch, **extra):
    return dict({k: v.cuda() for k, v in batch.items()}, **extra)


_ORACLE = {}


def oracle(sd, batch, eps, weight):
    """Loss, plain mean and every parameter gradient in float64: autograd through the oracle's log-probabilities and the definition
    (loss_ext_reference.loss_from_dists).  Computed once per setting and shared."""
    key = (eps, None if weight is None else tuple(float(x) for x in weight.reshape(-1)))
    if key not in _ORACLE:
        from oracle import plank_oracle as O
        cfg = O.OracleCfg(d_model=64, n_head=4, d_ff=128, n_enc=2, n_dec=2, max_input_length=65, max_output_length=36)
        p = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
        dists = O.train_forward(p, cfg, batch, return_all=True)["dists"]
        assert dists.dtype == torch.float64
        loss, mean, token = R.loss_from_dists(dists, batch["output_label"], cfg.pad, eps, weight)
        loss.backward()
        _ORACLE[key] = (float(loss.detach()), float(mean.detach()), token.detach(), {k: v.grad.clone() for k, v in p.items()})
    return _ORACLE[key]


def gate(m, grads, scale=1.0):
    """The project's f32 model gate (tests/test_model_gpu.py): each gradient within 1e-5 + 1e-4 max|ref|."""
    for k, p in m.named_parameters():
        ref = grads[k] * scale
        assert p.grad is not None, k
        err = float((p.grad.cpu().double() - ref).abs().max())
        assert err <= 1e-5 + 1e-4 * float(ref.abs().max()), (k, err, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ 8
def test_default_model_never_enters_the_new_entries(small_fixture, monkeypatch):
    from plankassembly_amd import _lib as L
    sd, batch, _ = small_fixture
    lib = L.lib()
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name not in NEW_ENTRIES:
                return fn
            return lambda *a: (calls.append(name), fn(*a))[1]

    m, ms = make(sd).train(), make(sd, label_smoothing=EPS).train()
    monkeypatch.setattr(L, "lib", lambda: Counting())
    out = m(to_dev(batch))
    out["loss"].backward()
    m.prepare_batch(batch)
    with torch.no_grad():
        m.train_step(to_dev(batch))
    assert calls == [] and sorted(out) == ["accuracy", "loss"]
    # (the counter does see the extended path.  Python reaches the two kernel entries only through the runtime, which calls them if and only
    # if pa_model_set_loss armed the handle: the plain mean below exists only where pa_mixture_nll_fwd_ext wrote it.)
    outs = ms(to_dev(batch))
    outs["loss"].backward()
    assert calls == ["pa_model_set_loss"] and sorted(outs) == ["accuracy", "loss", "nll"]
    assert abs(outs["nll"].item() - out["loss"].item()) <= 4 * 2.0 ** -24 * abs(out["loss"].item()) and outs["loss"].item() != out["loss"].item()
    # and a model that used the block once goes back to the present calls: one pa_model_set_loss(NULL), then nothing
    del calls[:]
    ms.label_smoothing = 0.0
    ms(to_dev(batch))["loss"].backward()
    ms(to_dev(batch))["loss"].backward()
    assert calls == ["pa_model_set_loss"]


# ------------------------------------------------------------------------------------------------ 9, 10
def test_smoothing_and_weights_match_float64_autograd(small_fixture):
    sd, batch, g = small_fixture
    w = torch.tensor(WEIGHT)
    loss64, mean64, token64, grads = oracle(sd, batch, EPS, w)
    m = make(sd, label_smoothing=EPS).train()
    out = m.train_step(to_dev(batch, loss_weight=w), token_nll=True)
    assert sorted(out) == ["accuracy", "loss", "nll", "token_nll"] and out["token_nll"].shape == batch["output_label"].shape
    print(f"loss {out['loss'].item()!r} (float64 {loss64!r}), nll {out['nll'].item()!r} (float64 {mean64!r})")
    assert abs(out["loss"].item() - loss64) <= 1e-4 and abs(out["nll"].item() - mean64) <= 1e-4
    assert abs(out["accuracy"].item() - float(g["g1::accuracy"])) < 1e-6                # unweighted, from the unsmoothed arg-max
    out["loss"].backward()
    gate(m, grads)
    # ---- nll is the default model's loss on the same batch (4 ulp); token_nll sums to it; PAD positions hold 0
    plain = make(sd).train()(to_dev(batch))["loss"].item()
    assert abs(out["nll"].item() - plain) <= 4 * 2.0 ** -24 * abs(plain), (out["nll"].item(), plain)
    n = int((batch["output_label"] != TOKEN.PAD).sum())
    assert abs(out["token_nll"].double().sum().item() / n - out["nll"].item()) <= 1e-6
    tok = out["token_nll"].cpu()
    assert not bool(tok[batch["output_label"] == TOKEN.PAD].any())
    assert float((tok.double() - token64).abs().max()) <= 1e-4
    # ---- 10: eval mode under no_grad returns the same token_nll bits (dropout 0)
    m.eval()
    with torch.no_grad():
        ev = m.train_step(to_dev(batch, loss_weight=w), token_nll=True)
    assert not ev["loss"].requires_grad
    assert torch.equal(ev["token_nll"].view(torch.int32), out["token_nll"].view(torch.int32))
    assert ev["loss"].item() == out["loss"].item() and ev["nll"].item() == out["nll"].item()


def test_token_nll_alone_and_per_token_weights(small_fixture):
    """token_nll=True on a default model: the loss is the default one; [B, T] weights that repeat a [B] vector give its loss bits; a
    prepared batch carries loss_weight through."""
    sd, batch, _ = small_fixture
    m = make(sd).train()
    base = m(to_dev(batch))["loss"].item()
    out = m.train_step(to_dev(batch), token_nll=True)
    assert out["loss"].item() == base and out["nll"].item() == base
    w = torch.tensor(WEIGHT)
    a = m.train_step(to_dev(batch, loss_weight=w))["loss"].item()
    b = m.train_step(to_dev(batch, loss_weight=w[:, None].expand(4, 36).contiguous().double()))["loss"].item()
    pb = m.prepare_batch(dict(batch, loss_weight=w))
    assert pb["loss_weight"].is_cuda and pb["loss_weight"].dtype == torch.float32
    c = m.train_step(pb)["loss"].item()
    assert a == b == c and a != base
    with pytest.raises(ValueError, match="loss_weight"):
        m.train_step(to_dev(batch, loss_weight=torch.ones(36)))


# ------------------------------------------------------------------------------------------------ 11
def test_bf16_gate(small_fixture):
    sd, batch, _ = small_fixture
    w = torch.tensor(WEIGHT)
    loss64, _, _, grads = oracle(sd, batch, EPS, w)
    m = make(sd, "bf16", label_smoothing=EPS).train()
    out = m.train_step(to_dev(batch, loss_weight=w))
    print(f"bf16 loss {out['loss'].item()!r} (float64 {loss64!r})")
    assert abs(out["loss"].item() - loss64) <= 0.02 * abs(loss64)
    out["loss"].backward()
    got = torch.cat([p.grad.detach().cpu().double().flatten() for _, p in m.named_parameters()])
    ref = torch.cat([grads[k].flatten() for k, _ in m.named_parameters()])
    cos = float(got @ ref) / (float(got.norm()) * float(ref.norm()) + 1e-300)
    print("bf16 flat gradient cosine", cos)
    assert cos > 0.995, cos


# ------------------------------------------------------------------------------------------------ 12
def test_gradient_accumulation_with_different_weights(small_fixture):
    sd, batch, _ = small_fixture
    w1, w2 = torch.tensor(WEIGHT), torch.tensor([0.5, 2.0, 0.0, -1.0])
    _, _, _, g1 = oracle(sd, batch, EPS, w1)
    _, _, _, g2 = oracle(sd, batch, EPS, w2)
    m = make(sd, label_smoothing=EPS).train()
    m.train_step(to_dev(batch, loss_weight=w1))["loss"].backward()
    m.train_step(to_dev(batch, loss_weight=w2))["loss"].backward()
    gate(m, {k: g1[k] + g2[k] for k in g1})


# ------------------------------------------------------------------------------------------------ 13
def test_short_fit_logs_nll_and_keeps_the_key(tmp_path, monkeypatch):
    import yaml
    from plankassembly_amd.trainer import Trainer, cli
    from test_cli_gpu import _write_config
    monkeypatch.chdir(tmp_path)
    config, n_files = _write_config(tmp_path, max_epochs=1)
    with open(config) as f:
        cfg = yaml.safe_load(f)
    cfg["model"]["hparams"]["MODEL"]["LABEL_SMOOTHING"] = 0.1
    with open(config, "w") as f:
        f.write(yaml.safe_dump(cfg))
    mod = cli(Trainer, ["fit", "--config", config])
    assert mod.global_step == 2 and mod.model.label_smoothing == 0.1                 # two optimizer steps
    hist = {name: v for _, name, v in mod.logger.history}
    assert np.isfinite(hist["train/loss"]) and np.isfinite(hist["train/nll"]) and hist["train/nll"] > 0
    assert hist["train/loss"] != hist["train/nll"]
    ck = torch.load(os.path.join(mod.logger.log_dir, "checkpoints", "last.ckpt"), map_location="cpu", weights_only=True)
    assert ck["hyper_parameters"]["hparams"]["MODEL"]["LABEL_SMOOTHING"] == 0.1
