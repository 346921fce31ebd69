"""CPU checks of the gradient guard's host side: the `trainer:` keys -> FusedAdam arguments (trainer.optimizer_options), a
reference-shaped YAML, FusedAdam's own argument checks (before it touches the library) and the control-block mirror."""
import ctypes

import pytest
import torch

from plankassembly_amd import _lib as L
from plankassembly_amd.config import load_cli_config
from plankassembly_amd.optim import FusedAdam
from plankassembly_amd.trainer import cli, optimizer_options


@pytest.mark.parametrize("block,kwargs,raises", [
    ({}, {}, False),
    ({"max_epochs": 3, "strategy": "ddp"}, {}, False),
    ({"gradient_clip_val": 0.5}, {"max_grad_norm": 0.5}, False),
    ({"gradient_clip_val": 2, "gradient_clip_algorithm": "norm"}, {"max_grad_norm": 2.0}, False),
    ({"gradient_clip_val": 0.5, "gradient_clip_algorithm": "value"}, {"clip_value": 0.5}, False),
    ({"gradient_clip_val": 0}, {}, False),
    ({"gradient_clip_val": 0.0, "gradient_clip_algorithm": "value"}, {}, False),
    ({"gradient_clip_val": None, "gradient_clip_algorithm": None}, {}, False),
    ({"detect_anomaly": True}, {"skip_nonfinite": True}, True),
    ({"detect_anomaly": False}, {}, False),
    ({"skip_nonfinite_steps": True}, {"skip_nonfinite": True}, False),
    ({"skip_nonfinite_steps": True, "detect_anomaly": True, "gradient_clip_val": 1.0},
     {"skip_nonfinite": True, "max_grad_norm": 1.0}, True),
    ({"detect_anomaly": "True"}, {"skip_nonfinite": True}, True),                # as `--trainer.detect_anomaly True` arrives
])
def test_optimizer_options(block, kwargs, raises):
    assert optimizer_options(block) == (kwargs, raises)


@pytest.mark.parametrize("block", [
    {"gradient_clip_val": 0.5, "gradient_clip_algorithm": "agc"},
    {"gradient_clip_algorithm": "NORM"},
    {"gradient_clip_val": -1.0},
    {"gradient_clip_val": float("nan")},
    {"gradient_clip_val": float("inf")},
    {"gradient_clip_val": "lots"},
    {"gradient_clip_val": True},
    {"detect_anomaly": "yes please"},
    {"skip_nonfinite_steps": 1},
])
def test_optimizer_options_rejects(block):
    with pytest.raises(ValueError):
        optimizer_options(block)


REFERENCE_SHAPED_YAML = """\
seed_everything: 2022

trainer:
  callbacks:
    - class_path: pytorch_lightning.callbacks.RichProgressBar
  benchmark: True
  detect_anomaly: True
  num_sanity_val_steps: 0
  max_epochs: 400
  check_val_every_n_epoch: 20
  strategy: ddp
  devices: 4
  accelerator: gpu

model:
  hparams:
    LR: 1e-4
"""


def test_reference_shaped_yaml_turns_skip_and_raise_on(tmp_path):
    path = tmp_path / "train_reference_shaped.yaml"
    path.write_text(REFERENCE_SHAPED_YAML)
    _, tkw, _ = load_cli_config(str(path))
    assert optimizer_options(tkw) == ({"skip_nonfinite": True}, True)
    path.write_text(REFERENCE_SHAPED_YAML.replace("  detect_anomaly: True\n", "  gradient_clip_val: 0.5\n"))
    assert optimizer_options(load_cli_config(str(path))[1]) == ({"max_grad_norm": 0.5}, False)


def test_shipped_configs_leave_the_guard_off():
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("train_complete", "train_visible", "train_sideface", "train_headline_seq1024"):
        assert optimizer_options(load_cli_config(os.path.join(repo, "configs", name + ".yaml"))[1]) == ({}, False)


def test_cli_override_reaches_optimizer_options(monkeypatch):
    """`--trainer.gradient_clip_val 1.0 --trainer.gradient_clip_algorithm value` through the existing override parser."""
    from plankassembly_amd import trainer as T
    seen = {}
    monkeypatch.setattr(T, "run", lambda cls, sub, config, ckpt, over: seen.update(over))
    cli(T.Trainer, ["fit", "--config", "x.yaml", "--trainer.gradient_clip_val", "1.0", "--trainer.gradient_clip_algorithm",
                    "value", "--trainer.detect_anomaly=true"])
    assert optimizer_options(seen) == ({"clip_value": 1.0, "skip_nonfinite": True}, True)


class _CpuModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(8))


@pytest.mark.parametrize("kw", [
    {"max_grad_norm": 0}, {"max_grad_norm": -1.0}, {"max_grad_norm": float("inf")}, {"max_grad_norm": float("nan")},
    {"max_grad_norm": "1"}, {"clip_value": 0.0}, {"clip_value": -3}, {"clip_value": float("nan")}, {"clip_value": True},
    {"max_grad_norm": 1.0, "clip_value": 1.0},
])
def test_fused_adam_rejects_bad_guard_arguments_before_touching_the_library(kw, monkeypatch):
    monkeypatch.setattr(L, "lib", lambda: pytest.fail("FusedAdam touched the library before checking its arguments"))
    with pytest.raises(ValueError):
        FusedAdam(_CpuModel(), **kw)


def test_fused_adam_guard_flags(monkeypatch):
    monkeypatch.setattr(L, "lib", lambda: pytest.fail("the constructor needs no library"))
    plain = FusedAdam(_CpuModel())
    assert not plain.guarded and plain.max_grad_norm is None and plain.clip_value is None and not plain.skip_nonfinite
    with pytest.raises(RuntimeError):
        plain.guard_stats()
    for kw in ({"max_grad_norm": 2}, {"clip_value": 0.5}, {"skip_nonfinite": True}):
        opt = FusedAdam(_CpuModel(), **kw)
        assert opt.guarded
        assert opt.guard_stats() == {"norm": 0.0, "coef": 1.0, "applied_steps": 0, "skipped_steps": 0, "attempts": 0,
                                     "first_skipped_attempt": -1}
        assert opt.state_dict()["step"] == 0


def test_control_block_mirror_matches_the_header():
    """include/plank_hip.h: 2048 f32 partials, then a 64-byte control block of four floats, five counters and padding."""
    assert ctypes.sizeof(L.GradGuardCtl) == 64 and L.GRAD_GUARD_CTL_OFFSET == 8192 and L.GRAD_GUARD_WS_BYTES == 8256
    names = [n for n, _ in L.GradGuardCtl._fields_]
    assert names == ["norm", "coef", "step_size", "inv_sqrt_bc2", "apply", "applied", "skipped", "attempts",
                     "first_skipped_attempt", "pad_"]
    assert L.GradGuardCtl.first_skipped_attempt.offset == 32
