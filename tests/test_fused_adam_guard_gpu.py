"""FusedAdam's gradient guard at model level (d 64 model of tests/test_model_gpu.py on the small golden fixture): a skipped
step leaves no trace, clipping reaches the moments, step() never waits for the device, checkpoints taken after a skipped step
resume with the right bias correction, and two data-parallel ranks skip the same step.  GPU only (`-m gpu`)."""
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

TOKEN = types.SimpleNamespace(END=512, PAD=513)


def make(sd, dtype="f32", d=64, h=4, ff=128, ne=2, nd=2, max_in=65, max_out=36, dropout=0.0):
    from plankassembly_amd.models import PlankModel
    m = PlankModel(d, h, ff, dropout, "relu", True, ne, nd, 3, 2, 4, 6, max_in, max_out, 514, TOKEN,
                   compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.cuda()


def to_dev(batch):
    return {k: v.cuda() for k, v in batch.items()}


def backward(m, opt, batch):
    opt.zero_grad()
    m(to_dev(batch))["loss"].backward()


def bits(t):
    return t.detach().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def test_a_skipped_step_leaves_no_trace(small_fixture):
    """Twins A and B (bf16 compute, so the Adam kernel also writes the shadow), both with skip_nonfinite.  A takes an extra step
    on a gradient with one inf in it; afterwards A must be B, bit for bit, in parameters, moments, shadow and step count.
    Two backward passes of one model differ in the last bits (f32 atomics in a few small reductions), so B steps on a COPY of
    A's gradient buffer after its own backward: what is compared is the optimizers."""
    from plankassembly_amd.optim import FusedAdam
    sd, batch, _ = small_fixture
    A, B = make(sd, "bf16").train(), make(sd, "bf16").train()
    oa, ob = FusedAdam(A, lr=1e-4, skip_nonfinite=True), FusedAdam(B, lr=1e-4, skip_nonfinite=True)

    def both_step():
        backward(A, oa, batch)
        backward(B, ob, batch)
        with torch.no_grad():
            B.flat_grads.copy_(A.flat_grads)
        oa.step()
        ob.step()

    both_step()
    backward(A, oa, batch)
    with torch.no_grad():
        A.flat_grads[A.flat_grads.numel() // 2] = float("inf")
    oa.step()
    both_step()
    torch.cuda.synchronize()
    assert torch.isfinite(A.flat_params).all()
    for a, b in ((A.flat_params, B.flat_params), (oa._m, ob._m), (oa._v, ob._v), (A._shadow, B._shadow)):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(A._shadow), bits(A.flat_params.to(torch.bfloat16)))
    sa, sb = oa.guard_stats(), ob.guard_stats()
    assert sa["skipped_steps"] == 1 and sa["attempts"] == 3 and sa["applied_steps"] == 2 and sa["first_skipped_attempt"] == 2
    assert sb["skipped_steps"] == 0 and sb["attempts"] == 2 and sb["applied_steps"] == 2
    assert float(oa.torch_state_dict()["state"][0]["step"]) == 2 == float(ob.torch_state_dict()["state"][0]["step"])


def test_clipping_reaches_the_moments(small_fixture):
    """max_grad_norm = half of the fixture's true norm (float64, from the golden g2:: gradients): after one step from zero
    moments m = (1 - b1) * 0.5 * g, within 1e-4 of the largest entry - the gate test_g1_g2 puts on the gradient itself."""
    from plankassembly_amd.optim import FusedAdam
    sd, batch, g = small_fixture
    m = make(sd).train()
    ref = torch.zeros(m.flat_params.numel(), dtype=torch.float64)
    for k, p in m.named_parameters():
        ref[m._offsets[k]:m._offsets[k] + p.numel()] = torch.from_numpy(g["g2::" + k]).double().flatten()
    true_norm = float(ref.norm())
    opt = FusedAdam(m, lr=1e-4, max_grad_norm=0.5 * true_norm)
    backward(m, opt, batch)
    opt.step()
    st = opt.guard_stats()
    want = 0.1 * 0.5 * ref
    err = float((opt._m.cpu().double() - want).abs().max())
    print(f"true norm {true_norm:.6e} device norm {st['norm']:.6e} coef {st['coef']!r} |dm| {err:.3e} of {float(want.abs().max()):.3e}")
    assert err <= 1e-4 * float(want.abs().max())
    assert abs(st["coef"] - 0.5) <= 1e-4
    assert st["applied_steps"] == 1 and st["skipped_steps"] == 0


def test_guarded_step_never_waits_for_the_device(small_fixture):
    from plankassembly_amd.optim import FusedAdam
    sd, batch, _ = small_fixture
    m = make(sd, "bf16").train()
    opt = FusedAdam(m, lr=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
    for _ in range(2):                               # the first step also makes the workspace and the moments
        backward(m, opt, batch)
        torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert opt.guard_stats()["attempts"] == 2


@pytest.mark.parametrize("layout", ["flat", "torch"])
def test_checkpoint_after_a_skipped_step_resumes_bit_equal(small_fixture, layout):
    """One applied step, one skipped step, then the checkpoint: the loaded optimizer must continue with Adam step 2 (not 3,
    the number of attempts) - its next step on the same gradient equals the original's bit for bit."""
    from plankassembly_amd.optim import FusedAdam
    sd, batch, _ = small_fixture
    kw = dict(lr=1e-4, max_grad_norm=0.01, skip_nonfinite=True)
    m = make(sd).train()
    opt = FusedAdam(m, **kw)
    backward(m, opt, batch)
    opt.step()
    backward(m, opt, batch)
    with torch.no_grad():
        m.flat_grads[7] = float("nan")
    opt.step()
    ck = opt.state_dict() if layout == "flat" else opt.torch_state_dict()
    step = ck["step"] if layout == "flat" else int(ck["state"][0]["step"])
    assert step == 1
    weights = m.flat_params.detach().clone()
    backward(m, opt, batch)
    grad = m.flat_grads.detach().clone()
    opt.step()

    m2 = make(sd).train()
    with torch.no_grad():
        m2.flat_params.copy_(weights)
    m2.invalidate_shadow()
    opt2 = FusedAdam(m2, **kw)
    opt2.load_state_dict(ck)
    with torch.no_grad():
        m2.flat_grads.copy_(grad)
    opt2.step()
    torch.cuda.synchronize()
    for a, b in ((m.flat_params, m2.flat_params), (opt._m, opt2._m), (opt._v, opt2._v)):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(bits(m.flat_params), bits(weights))               # (the compared step did move the weights)
    assert opt2.guard_stats()["applied_steps"] == 2 == opt.guard_stats()["applied_steps"]


def test_two_ranks_skip_the_same_step(tmp_path):
    """Two processes on one GPU over gloo, each with its own half batch; on step 2 rank 1 alone writes a NaN into its gradient
    buffer before the exchange.  The summed buffer is what both guards see, so both skip step 2 - without a collective of
    their own - and the ranks stay in lock step."""
    import socket
    import subprocess
    import sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = str(tmp_path / "rank")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ddp_guard_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", str(port), out], env=env) for r in range(2)]
    try:
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    r0, r1 = (torch.load(f"{out}.{r}", weights_only=True) for r in range(2))
    for r in (r0, r1):
        assert r["stats"]["skipped_steps"] == 1 and r["stats"]["applied_steps"] == 2 and r["stats"]["attempts"] == 3
        assert r["stats"]["first_skipped_attempt"] == 2 and r["finite"]
    assert torch.equal(bits(r0["params"]), bits(r1["params"]))


def test_trainer_loop_skips_logs_and_raises(tmp_path, monkeypatch):
    """The loop end to end on the small CLI model of tests/test_cli_gpu.py (two steps per epoch); the training step at global
    step 1 returns a NaN loss, so every gradient of that step is NaN.  `skip_nonfinite_steps`: the run goes on, logs the count
    and its checkpoint stores ONE Adam step; `detect_anomaly`: RuntimeError at the epoch boundary, weights finite."""
    from test_cli_gpu import _write_config
    from plankassembly_amd.trainer import Trainer, cli
    monkeypatch.chdir(tmp_path)
    config, n_files = _write_config(tmp_path, max_epochs=1)
    assert n_files // 4 == 2
    made = []

    class Poisoned(Trainer):
        def __init__(self, hparams):
            super().__init__(hparams)
            made.append(self)

        def training_step(self, batch, batch_idx):
            loss = super().training_step(batch, batch_idx)
            return loss * float("nan") if self.global_step == 1 else loss

    mod = cli(Poisoned, ["fit", "--config", config, "--trainer.skip_nonfinite_steps", "true", "--trainer.gradient_clip_val", "0.5"])
    assert mod.optimizer.max_grad_norm == 0.5 and mod.optimizer.skip_nonfinite
    assert mod.global_step == 2 and mod._logged["train/skipped_steps"] == 1.0 and mod._logged["train/grad_norm"] != mod._logged["train/grad_norm"]
    assert mod.optimizer.guard_stats()["applied_steps"] == 1 and torch.isfinite(mod.model.flat_params).all()
    ck = torch.load(os.path.join(mod.logger.log_dir, "checkpoints", "last.ckpt"), map_location="cpu", weights_only=True)
    assert float(ck["optimizer_states"][0]["state"][0]["step"]) == 1.0 and ck["global_step"] == 2

    with pytest.raises(RuntimeError, match=r"detect_anomaly: 1 optimizer step\(s\).*first at global step 1 "):
        cli(Poisoned, ["fit", "--config", config, "--trainer.detect_anomaly", "true"])
    bad = made[-1]
    assert bad is not mod and torch.isfinite(bad.model.flat_params).all()
    assert bad.optimizer.guard_stats()["skipped_steps"] == 1 and bad.optimizer.max_grad_norm is None
