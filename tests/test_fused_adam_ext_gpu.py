"""FusedAdam's recipe extensions at model level (d 64 model on the small golden fixture): decoupled decay
with the 1-D exemption and the EMA against torch.optim.AdamW with two parameter groups, ema_weights(), the default path against ops.adam_step,
and `fit` with a schedule, decay and EMA through the command line, resumed.  GPU only (`-m gpu`)."""
import os

import numpy as np
import pytest
import torch

import adam_ext_reference as R
from test_fused_adam_guard_gpu import backward, bits, make, to_dev

pytestmark = pytest.mark.gpu
EPS24 = 2.0 ** -24


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def test_three_train_steps_match_adamw_with_two_groups_and_a_float64_ema(small_fixture):
    """FusedAdam(lr 1e-4, weight_decay 0.01, no_decay "1d", ema_decay 0.99) against a CPU copy of the parameters under
    torch.optim.AdamW with two groups (1-D parameters at weight_decay 0), fed the device's own gradients each step.  Bounds: the
    kernel test's (p 2e-7 plus half an ulp of max|p| per step, m 2e-5 rel, v 1.2e-4 rel); the EMA per step within
    4 * 2^-24 (|p| + |e|) of the float64 rule fed the device's p."""
    from plankassembly_amd.optim import FusedAdam
    sd, batch, _ = small_fixture
    m = make(sd, "bf16").train()
    opt = FusedAdam(m, lr=1e-4, weight_decay=0.01, no_decay="1d", ema_decay=0.99)
    names = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
    cpu = {k: torch.nn.Parameter(p.detach().cpu().clone()) for k, p in names}
    topt = torch.optim.AdamW([{"params": [cpu[k] for k, p in names if p.ndim >= 2], "weight_decay": 0.01},
                              {"params": [cpu[k] for k, p in names if p.ndim < 2], "weight_decay": 0.0}], lr=1e-4)
    assert any(p.ndim < 2 for _, p in names) and any(p.ndim >= 2 for _, p in names)
    p_max = max(float(p.detach().abs().max()) for _, p in names)
    e_prev = m.flat_params.detach().cpu().double().numpy()
    for t in (1, 2, 3):
        backward(m, opt, batch)
        for k, p in names:
            cpu[k].grad = p.grad.detach().cpu().clone()
        opt.step()
        topt.step()
        p_now = m.flat_params.detach().cpu().double().numpy()
        e_now = opt._ema.detach().cpu().double().numpy()
        want = R.ema_step(e_prev, p_now, 0.99, t)
        assert (np.abs(e_now - want) <= 4 * EPS24 * (np.abs(p_now) + np.abs(e_prev))).all()
        assert np.abs(e_now - e_prev).max() > 0
        e_prev = e_now
    torch.cuda.synchronize()
    bound = 2e-7 + 3 * 0.5 * float(np.spacing(np.float32(p_max)))
    dp = 0.0
    m_ref, v_ref = torch.zeros_like(opt._m, device="cpu"), torch.zeros_like(opt._v, device="cpu")
    for k, p in names:
        off, n = m._offsets[k], p.numel()
        st = topt.state[cpu[k]]
        dp = max(dp, float((p.detach().cpu() - cpu[k].detach()).abs().max()))
        m_ref[off:off + n], v_ref[off:off + n] = st["exp_avg"].reshape(-1), st["exp_avg_sq"].reshape(-1)
    dm, dv = rel_err(opt._m, m_ref), rel_err(opt._v, v_ref)             # (over the flat buffer, as the kernel test measures)
    print(f"three train steps: |dp| {dp:.3e} (bound {bound:.3e})  m rel {dm:.3e}  v rel {dv:.3e}")
    assert dp <= bound and dm <= 2e-5 and dv <= 1.2e-4
    assert opt.ema_updates == 3 and opt.state_dict()["ema_updates"] == 3
    assert torch.equal(bits(m._shadow), bits(m.flat_params.to(torch.bfloat16)))
    assert opt.torch_state_dict()["param_groups"][0]["weight_decay"] == 0.01


def test_ema_weights_swaps_in_and_restores_bit_for_bit(small_fixture):
    from plankassembly_amd.optim import FusedAdam
    sd, batch, _ = small_fixture
    m = make(sd, "bf16").train()
    opt = FusedAdam(m, lr=1e-2, ema_decay=0.5, skip_nonfinite=True)
    for _ in range(2):
        backward(m, opt, batch)
        opt.step()
    assert opt.ema_updates == 2                                     # (read from the device control block)
    raw, shadow = m.flat_params.detach().clone(), m._shadow.detach().clone()
    ema_sd = opt.ema_state_dict()
    assert not torch.equal(opt._ema, raw)
    twin = make({k: v.clone() for k, v in ema_sd.items()}, "bf16").eval()
    m.eval()
    with torch.no_grad():
        want = twin.eval_step(to_dev(batch), parse=False)["samples"]
        raw_tokens = m.eval_step(to_dev(batch), parse=False)["samples"]
        with opt.ema_weights():
            assert torch.equal(bits(m.flat_params), bits(opt._ema))
            assert all(torch.equal(v.cpu(), ema_sd[k]) for k, v in m.state_dict().items())
            got = m.eval_step(to_dev(batch), parse=False)["samples"]
            with pytest.raises(RuntimeError, match="inside ema_weights"):
                opt.step()
        assert torch.equal(got, want)
        assert torch.equal(bits(m.flat_params), bits(raw))
        assert torch.equal(m.eval_step(to_dev(batch), parse=False)["samples"], raw_tokens)
        assert torch.equal(bits(m._shadow), bits(shadow))
        with pytest.raises(ZeroDivisionError):
            with opt.ema_weights():
                m.eval_step(to_dev(batch), parse=False)
                1 / 0
        m.eval_step(to_dev(batch), parse=False)                     # (re-derives the shadow if the exit had not)
    torch.cuda.synchronize()
    assert torch.equal(bits(m.flat_params), bits(raw)) and torch.equal(bits(m._shadow), bits(shadow))
    m.train()
    backward(m, opt, batch)
    opt.step()                                                      # and training goes on
    assert opt.ema_updates == 3


def test_default_fused_adam_step_equals_ops_adam_step_bit_for_bit(small_fixture):
    """No new argument: one step equals a twin stepped through ops.adam_step, bit for bit in parameters, moments and shadow
    (B steps on a copy of A's gradient buffer: two backward passes differ in the last bits).  Every FusedAdam step and
    ops.adam_step run the one Adam kernel, so this holds the optimizer's marshalling to the entry's.  That the default step's
    RESULT is untouched - what counting the calls of pa_adam_step_ext used to guarantee here - is the stricter comparison with
    the bits recorded from the build before the kernels were folded: tests/test_rowops_family_bits_gpu.py."""
    from plankassembly_amd import ops
    from plankassembly_amd.optim import FusedAdam
    sd, batch, _ = small_fixture
    A, B = make(sd, "bf16").train(), make(sd, "bf16").train()
    oa, ob = FusedAdam(A, lr=1e-4), FusedAdam(B, lr=1e-4)
    backward(A, oa, batch)
    backward(B, ob, batch)                                          # (binds B to the runtime: its shadow exists from here on)
    oa.step()
    mB, vB = torch.zeros_like(B.flat_params), torch.zeros_like(B.flat_params)
    ops.adam_step(B.flat_params, A.flat_grads, mB, vB, 1, lr=1e-4, p_bf16=B._shadow)
    torch.cuda.synchronize()
    assert torch.equal(bits(A.flat_params), bits(B.flat_params)) and torch.equal(bits(A._shadow), bits(B._shadow))
    assert torch.equal(bits(oa._m), bits(mB)) and torch.equal(bits(oa._v), bits(vB))


def test_fit_with_schedule_decay_and_ema_resumes_bit_equal(tmp_path, monkeypatch):
    """`fit` on the small CLI model of tests/test_cli_gpu.py (two steps per epoch) with LR_SCHEDULE cosine, WARMUP_STEPS 2,
    EMA_DECAY 0.9, WEIGHT_DECAY 0.01: the logged train/lr follows lr_factor, last.ckpt carries the EMA and the scheduler record,
    and two epochs + `fit --ckpt_path last.ckpt` for a third equal an uninterrupted three-epoch run bit for bit in weights,
    moments, EMA and the next learning rate.  Two backward passes differ in the last bits, so - the pattern of
    test_checkpoint_after_a_skipped_step_resumes_bit_equal - the uninterrupted run records the gradient buffer of each step and
    the other two runs step on those: what is compared is everything between the gradient and the checkpoint."""
    import yaml
    from test_cli_gpu import _write_config
    from plankassembly_amd.trainer import Trainer, cli
    monkeypatch.chdir(tmp_path)
    config, n_files = _write_config(tmp_path, max_epochs=3)
    assert n_files // 4 == 2
    with open(config) as f:
        cfg = yaml.safe_load(f)
    cfg["model"]["hparams"].update(LR_SCHEDULE="cosine", WARMUP_STEPS=2, EMA_DECAY=0.9, WEIGHT_DECAY=0.01, LR_TOTAL_STEPS=6)
    with open(config, "w") as f:
        yaml.safe_dump(cfg, f)
    base_lr = cfg["model"]["hparams"]["LR"]
    tape = []

    class Taped(Trainer):
        replay = False

        def configure_optimizers(self):
            out = super().configure_optimizers()
            opt, trainer = out["optimizer"], self
            inner = opt.step

            def step(closure=None):
                g = trainer.model.flat_grads
                if trainer.replay:
                    with torch.no_grad():
                        g.copy_(tape[trainer.global_step])
                else:
                    tape.append(g.detach().clone())
                return inner(closure)

            opt.step = step
            return out

    def end_state(mod):
        o = mod.optimizer
        return [mod.model.flat_params, o._m, o._v, o._ema]

    full = cli(Taped, ["fit", "--config", config])
    assert full.global_step == 6 and len(tape) == 6 and full.optimizer.ema_updates == 6
    lrs = [v for _, name, v in full.logger.history if name == "train/lr"]
    want = [base_lr * R.lr_factor("cosine", s, 2, 6, 0.0) for s in (1, 3, 5)]           # the rate of each epoch's last step
    assert lrs == pytest.approx(want, rel=1e-12) and lrs[0] == base_lr and lrs[2] < lrs[1] < lrs[0]
    full_ck = torch.load(os.path.join(full.logger.log_dir, "checkpoints", "last.ckpt"), map_location="cpu", weights_only=True)

    Taped.replay = True
    two = cli(Taped, ["fit", "--config", config, "--trainer.max_epochs", "2"])
    last = os.path.join(two.logger.log_dir, "checkpoints", "last.ckpt")
    ck = torch.load(last, map_location="cpu", weights_only=True)
    assert ck["global_step"] == 4 and ck["ema_updates"] == 4 and list(ck["ema_state_dict"]) == list(ck["state_dict"])
    (rec,) = ck["lr_schedulers"]
    assert rec["last_epoch"] == 4 and rec["base_lrs"] == [base_lr]
    assert rec["_last_lr"] == [base_lr * R.lr_factor("cosine", 4, 2, 6, 0.0)]
    assert ck["optimizer_states"][0]["param_groups"][0]["weight_decay"] == 0.01
    assert all(torch.equal(v, two.model.state_dict()[k[6:]].cpu()) for k, v in ck["state_dict"].items())     # raw weights
    assert any(not torch.equal(v, ck["state_dict"][k]) for k, v in ck["ema_state_dict"].items())

    resumed = cli(Taped, ["fit", "--config", config, "--ckpt_path", last])
    assert resumed.resume_epoch == 2 and resumed.global_step == 6 and resumed.optimizer.ema_updates == 6
    torch.cuda.synchronize()
    for a, b in zip(end_state(full), end_state(resumed)):
        assert torch.equal(bits(a), bits(b))
    res_ck = torch.load(os.path.join(resumed.logger.log_dir, "checkpoints", "last.ckpt"), map_location="cpu", weights_only=True)
    assert res_ck["lr_schedulers"] == full_ck["lr_schedulers"] and res_ck["ema_updates"] == full_ck["ema_updates"] == 6
    assert all(torch.equal(v, full_ck["ema_state_dict"][k]) for k, v in res_ck["ema_state_dict"].items())
    assert full.optimizer.param_groups[0]["lr"] == resumed.optimizer.param_groups[0]["lr"]

    # ---- `test --ckpt_path` evaluates the EMA weights when the file has them (EVAL_EMA defaults to true with EMA_DECAY)
    tested = cli(Trainer, ["test", "--config", config, "--ckpt_path", last])
    for k, v in tested.model.state_dict().items():
        assert torch.equal(v.cpu(), ck["ema_state_dict"]["model." + k])
