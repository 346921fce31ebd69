"""Scoring on the device (metric.DevicePlankScorer, trainer hparam DEVICE_METRIC, eval_step(parse=False)) on
the fixture_f1 weights: the numbers and files of the host path, bit for bit and byte for byte."""
import os
import types

import numpy as np
import pytest
import torch

import match_reference as R
from conftest import REPO, load_fixture
from plankassembly_amd import metric as M

pytestmark = pytest.mark.gpu


def f1_trainer(**extra):
    from plankassembly_amd.config import load_cli_config
    from plankassembly_amd.trainer import Trainer
    _, _, hp = load_cli_config(os.path.join(REPO, "configs", "train_complete.yaml"))
    hp["MODEL"].update(NUM_MODEL=64, NUM_HEAD=4, NUM_FEEDFORWARD=128, NUM_ENCODER_LAYERS=2, NUM_DECODER_LAYERS=2,
                       DROPOUT=0.0, COMPUTE_DTYPE="f32")
    hp["DATA"].update(MAX_INPUT_LENGTH=65, MAX_OUTPUT_LENGTH=36)
    hp.update(extra)
    sd, batch, g = load_fixture("fixture_f1.npz")
    t = Trainer(hp)
    t.model.load_state_dict(sd)
    t.model.cuda().eval()
    return t, t.model.prepare_batch(batch), g


def host_means(t, outputs):
    scorer = M.PlankScorer(0.5)
    dicts = [scorer.add(t._valid_pred(p), g) for p, g in zip(outputs["predicts"], outputs["groundtruths"])]
    return dicts, scorer.means(sync=False)


def test_greedy_decode_into_the_device_scorer_equals_the_host_scorer():
    t, gb, g = f1_trainer()
    with torch.no_grad():
        out = t.model(gb)
    assert np.array_equal(out["samples"].cpu().numpy(), g["samples"])
    want_dicts, want = host_means(t, out)
    dev = M.DevicePlankScorer(0.5, 512)
    assert dev.add_batch(out["samples"], gb["output_value"]) is None
    got = dev.means(sync=False)
    assert got == want and np.allclose(got, g["epoch_prf"], atol=1e-7), (got, want)
    assert 0.5 < got[2] < 1.0 and dev.fallbacks == 0
    assert dev.add_batch(out["samples"], gb["output_value"], scores=True) == want_dicts      # read back at once, as test_step does
    assert dev.means(sync=False) == want


def test_exact_half_pairs_go_through_the_fallback():
    rng = np.random.default_rng(41)
    pairs = []
    while len(pairs) < 64:
        pred, gt = R.random_pair(rng, 12)
        pairs.append((pred, gt))
    samples = torch.from_numpy(R.rows_of([p for p, _ in pairs], 96)).cuda()
    truth = torch.from_numpy(R.rows_of([q for _, q in pairs], 128)).cuda()
    ties = R.plank_match(samples.cpu().numpy(), truth.cpu().numpy())[:, 3]
    assert int((ties > 0).sum()) >= 10 and int((ties == 0).sum()) >= 10

    def parse(seq):
        valid = seq[torch.cumsum(seq == 512, 0) == 0]
        return valid[: len(valid) // 6 * 6].reshape(-1, 6)

    t = types.SimpleNamespace()
    from plankassembly_amd.trainer import Trainer
    host = M.PlankScorer(0.5)
    want_dicts = [host.add(Trainer._valid_pred(t, parse(s)), parse(q)) for s, q in zip(samples.cpu(), truth.cpu())]
    want = host.means(sync=False)
    dev = M.DevicePlankScorer(0.5, 512)
    got_dicts = dev.add_batch(samples[:40], truth[:40], scores=True)
    dev.add_batch(samples[40:], truth[40:])
    assert got_dicts == want_dicts[:40]
    assert dev.means(sync=False) == want
    assert dev.fallbacks == int((ties > 0).sum())


def test_eval_step_without_parse_carries_the_same_tokens():
    t, gb, g = f1_trainer()
    with torch.no_grad():
        full = t.model.eval_step(gb)
        lean = t.model.eval_step(gb, parse=False)
    assert sorted(lean) == ["attach", "samples"] and "predicts" in full and "groundtruths" in full
    assert torch.equal(lean["samples"], full["samples"]) and torch.equal(lean["attach"], full["attach"])


def test_trainer_with_device_metric_logs_and_writes_what_the_host_path_does(tmp_path):
    logged, files = {}, {}
    for key in ("host", "device"):
        t, gb, g = f1_trainer(**({"DEVICE_METRIC": True} if key == "device" else {}))
        assert isinstance(t.scorer, M.DevicePlankScorer) == (key == "device")
        out_dir = tmp_path / key
        t.logger = types.SimpleNamespace(log_dir=str(out_dir), log=lambda *a: None)
        n = int(g["n"])
        with torch.no_grad():
            t.validation_step(gb, 0)
            t.validation_step(gb, 1)
            t.validation_epoch_end()
            t.test_step(dict(gb, name=[f"f1case{i}" for i in range(n)]), 0)
            t.test_epoch_end()
        logged[key] = dict(t._logged)
        files[key] = {f: open(out_dir / "pred_jsons" / f, "rb").read() for f in sorted(os.listdir(out_dir / "pred_jsons"))}
    assert sorted(logged["host"]) == ["test/fmeasure", "test/precision", "test/recall", "val/fmeasure", "val/precision", "val/recall"]
    assert logged["device"] == logged["host"]
    assert len(files["host"]) == 6 and files["device"] == files["host"]
    assert np.allclose([logged["device"][f"val/{k}"] for k in ("precision", "recall", "fmeasure")], g["epoch_prf"], atol=1e-7)


def test_sideface_trainer_with_device_metric_and_an_empty_input(tmp_path):
    """SidefaceTrainer.test_step: a drawing without side faces (input = [END, PAD ...]) scores 0, writes an empty prediction and
    takes no part in the means - on the device path (`keep=`) as on the host path, byte for byte."""
    from plankassembly_amd.config import load_cli_config
    from plankassembly_amd.trainer import SidefaceTrainer
    sd, batch, g = load_fixture("fixture_f1.npz")
    batch = {k: v.clone() for k, v in batch.items() if k != "input_type"}
    batch["input_value"][2] = 513
    batch["input_value"][2, 0] = 512
    batch["input_mask"][2] = True
    batch["input_mask"][2, 0] = False
    n = int(g["n"])
    logged, files = {}, {}
    for key in ("host", "device"):
        _, _, hp = load_cli_config(os.path.join(REPO, "configs", "train_sideface.yaml"))
        hp["MODEL"].update(NUM_MODEL=64, NUM_HEAD=4, NUM_FEEDFORWARD=128, NUM_ENCODER_LAYERS=2, NUM_DECODER_LAYERS=2,
                           DROPOUT=0.0, COMPUTE_DTYPE="f32")
        hp["DATA"].update(MAX_INPUT_LENGTH=65, MAX_OUTPUT_LENGTH=36)
        if key == "device":
            hp["DEVICE_METRIC"] = True
        t = SidefaceTrainer(hp)
        t.model.load_state_dict(sd)
        t.model.cuda().eval()
        gb = t.model.prepare_batch(batch)
        out_dir = tmp_path / key
        t.logger = types.SimpleNamespace(log_dir=str(out_dir), log=lambda *a: None)
        with torch.no_grad():
            t.validation_step(gb, 0)
            t.validation_epoch_end()
            t.test_step(dict(gb, name=[f"side{i}" for i in range(n)]), 0)
            t.test_epoch_end()
        logged[key] = dict(t._logged)
        files[key] = {f: open(out_dir / "pred_jsons" / f, "rb").read() for f in sorted(os.listdir(out_dir / "pred_jsons"))}
    assert logged["device"] == logged["host"] and files["device"] == files["host"] and len(files["host"]) == n
    import json
    empty = json.loads(files["device"]["side2.json"])
    assert empty["prediction"] == [] and empty["fmeasure"] == 0.0 and len(empty["groundtruth"]) > 0
    assert sum(bool(json.loads(v)["prediction"]) for v in files["device"].values()) >= 3
    # five drawings count for test/*, six for val/*: the empty one is left out of the test means only
    per = [json.loads(files["host"][f"side{i}.json"])["fmeasure"] for i in range(n) if i != 2]
    assert abs(logged["device"]["test/fmeasure"] - sum(per) / 5) < 1e-6 and logged["device"]["test/fmeasure"] > 0
