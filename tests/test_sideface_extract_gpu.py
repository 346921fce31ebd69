"""Side-face extraction on the GPU (csrc/sideface.h `pa_tokenise_sideface_drawings`, plankassembly_amd/device_data.py; DESIGN.md
section 26).  Augmentation off: the device batch IS the batch `DataLoader` collates from `SidefaceDataset` extracting on the host, and
the merged boxes equal the host's as float64 bits.  Augmentation on: the numpy restatement (tests/sideface_reference.py `sample`) fed
the same counter-based draws, bit for bit.  Then the flags, a drawing outside the domain handed straight to the entry, and two
optimiser steps through `fit`."""
import os
import types

import numpy as np
import pytest
import torch
import yaml

import device_data_reference as R
import sideface_reference as SR
from plankassembly_amd import datasets as D

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKEN = types.SimpleNamespace(END=512, PAD=513)
NO_PLANKS = (np.zeros((1, 6)), np.full((1, 6), -1))
KEYS = ("input_value", "input_pos", "input_coord", "input_view", "input_mask", "output_value", "output_label", "output_mask")


def _info(name, segs, views, planks=NO_PLANKS):
    return R.make_info(name, np.asarray(segs, dtype=np.float64).reshape(-1, 4), views, [0] * len(views), *planks)


def _dangles(n, x=0.5, y=0.9):
    """A chain of n segments that bounds nothing."""
    return [[round(x + 0.01 * k, 3), y, round(x + 0.01 * (k + 1), 3), y] for k in range(n)]


def _edge_infos():
    """0 lines; 1 line; one rectangle; a generated drawing of about 60 lines; 257 lines (one more than the block has threads) and
    1024 lines (the kernel's capacity) of tiled thin cells; the last one's 15 rows + 32 columns = 47 boxes fill the row exactly."""
    rng = np.random.default_rng(7)
    gen = SR.render_drawing(rng, 4, "generated")
    assert 40 <= len(gen["svgs"]) <= 90
    t257, v257 = SR.tiled_cells(16, 7, 0.03, 0.03)
    t1024, v1024 = SR.tiled_cells(32, 15, 0.03, 0.03, view=2)
    s257, s1024 = t257.tolist() + _dangles(10), t1024.tolist() + _dangles(17)
    assert len(s257) == 257 and len(s1024) == 1024
    return [_info("no_lines", np.zeros((0, 4)), []), _info("one_line", [[0.0, 0.0, 0.5, 0.0]], [1]),
            _info("one_rectangle", [[0.0, 0.0, 0.5, 0.0], [0.5, 0.0, 0.5, 0.02], [0.5, 0.02, 0.0, 0.02], [0.0, 0.02, 0.0, 0.0]], [1] * 4,
                  R.random_planks(rng, 3)),
            gen, _info("tiles257", s257, list(v257) + [0] * 10, R.random_planks(rng, 5)),
            _info("tiles1024", s1024, list(v1024) + [2] * 17, R.random_planks(rng, 9))]


@pytest.fixture(scope="module")
def edge_set(tmp_path_factory):
    from plankassembly_amd.device_data import DeviceDrawings, pack_infos
    root = str(tmp_path_factory.mktemp("sideface_edges"))
    files = R.write_infos(root, _edge_infos())
    cfg = SR.make_data_cfg(4 * 47 + 2, 60)                                   # a row of exactly 47 faces
    packed = pack_infos(root, files, "sideface", extract=True, data_cfg=cfg)
    assert packed["n_faces"].tolist()[:3] == [0, 0, 1] and packed["n_faces"][-1] == 47 == (cfg.MAX_INPUT_LENGTH - 2) // 4
    return root, files, cfg, packed, DeviceDrawings(packed, TOKEN, cfg, "cuda")


def _batch(dd, index, **kw):
    index = np.asarray(index, dtype=np.int32)
    return dd.batch(torch.from_numpy(index).cuda(), host_index=index, **kw)


def _same_rows(got, want, rows=None):
    for k in KEYS:
        w = torch.from_numpy(np.asarray(want[k])) if not torch.is_tensor(want[k]) else want[k]
        g = got[k].cpu() if rows is None else got[k].cpu()[rows]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g, w), (k, (g != w).nonzero()[:4].tolist())


def test_batches_equal_the_cpu_dataset_and_boxes_equal_the_hosts_bits(edge_set):
    root, files, cfg, packed, dd = edge_set
    index = [0, 1, 2, 3, 4, 5, 3, 3, 2, 0]                                    # every drawing; some twice
    got = _batch(dd, index)
    ds = D.SidefaceDataset(root, files, TOKEN, cfg)
    cpu = next(iter(torch.utils.data.DataLoader(torch.utils.data.Subset(ds, index), batch_size=len(index), shuffle=False)))
    assert [k for k in got if not k.startswith("_")] == list(cpu) and got["name"] == list(cpu["name"])
    _same_rows(got, cpu)
    assert not got["_extract_flags"].any()
    n_faces = got["_n_faces"].cpu().numpy()
    assert torch.equal(got["_n_tokens"].cpu(), (~cpu["input_mask"]).sum(1).to(torch.int32))
    assert got["_n_valid"] == int((4 * n_faces + 1).sum()) == int((~cpu["input_mask"]).sum())
    faces_dev, views_dev = got["_faces"].cpu().numpy(), got["_faceviews"].cpu().numpy()
    for r, i in enumerate(index):
        faces, fviews = D.extract_sideface(*SR.info_segments(_edge_infos()[i]), *SR.THRESHOLDS)
        order = SR.row_order(faces, fviews, cfg.NUM_BITS)
        assert n_faces[r] == len(faces) == packed["n_faces"][i]
        assert np.array_equal(faces_dev[r, :len(faces)].view(np.int64), faces[order].view(np.int64).reshape(-1, 4)), files[i]
        assert np.array_equal(views_dev[r, :len(faces)], fviews[order]) and not faces_dev[r, len(faces):].any()
    assert n_faces.tolist()[:6] == [0, 0, 1, n_faces[3], 23, 47] and n_faces[3] > 0
    row = got["input_value"][0].cpu()
    assert row[0] == TOKEN.END and bool((row[1:] == TOKEN.PAD).all())


@pytest.fixture(scope="module")
def aug_set(tmp_path_factory):
    from plankassembly_amd.device_data import DeviceDrawings, pack_infos
    root = str(tmp_path_factory.mktemp("sideface_aug"))
    infos = [SR.render_drawing(np.random.default_rng(100 + s), 2 + s % 7, f"aug{s:02d}") for s in range(12)]
    files = R.write_infos(root, infos)
    cfg = SR.make_data_cfg(4 * 60 + 2, 60, aug_ratio=1.0, noise_ratio=0.15, noise_length=0.02)
    packed = pack_infos(root, files, "sideface", extract=True, data_cfg=cfg)
    return cfg, packed, DeviceDrawings(packed, TOKEN, cfg, "cuda")


def _check_against_restatement(dd, packed, cfg, index, epoch, seed=7):
    got = _batch(dd, index, epoch=epoch, augmentation=True, seed=seed)
    assert "_n_valid" not in got
    flags, n_faces = got["_extract_flags"].cpu().numpy(), got["_n_faces"].cpu().numpy()
    faces_dev = got["_faces"].cpu().numpy()
    for r, i in enumerate(index):
        want, wflags, wfaces, _ = SR.sample(packed, i, cfg, TOKEN, True, seed, epoch)
        _same_rows(got, {k: want[k][None] for k in KEYS}, rows=slice(r, r + 1))
        assert flags[r] == wflags and n_faces[r] == len(wfaces), (i, epoch, flags[r], wflags)
        assert np.array_equal(faces_dev[r, :len(wfaces)].view(np.int64), wfaces.view(np.int64).reshape(-1, 4))
    return got, flags


def test_augmented_batches_equal_the_restatement(aug_set):
    cfg, packed, dd = aug_set
    clean = _batch(dd, range(len(dd)))
    changed = 0
    for epoch in (0, 1):
        got, flags = _check_against_restatement(dd, packed, cfg, list(range(len(dd))), epoch)
        changed += int((got["input_value"] != clean["input_value"]).any(1).sum())
    assert changed >= 4                                                       # the noise reaches the side faces


def test_a_row_does_not_depend_on_its_batch(aug_set):
    cfg, packed, dd = aug_set
    full = _batch(dd, range(len(dd)), epoch=3, augmentation=True, seed=7)
    perm = np.random.default_rng(1).permutation(len(dd))
    for bs in (1, 5):
        for lo in range(0, len(perm), bs):
            idx = perm[lo:lo + bs]
            part = _batch(dd, idx, epoch=3, augmentation=True, seed=7)
            for k in KEYS + ("_extract_flags", "_n_faces", "_faces"):
                assert torch.equal(part[k], full[k][torch.from_numpy(idx).cuda()]), (k, bs, lo)


def test_fallback_and_capacity_flags(tmp_path):
    from plankassembly_amd.device_data import DeviceDrawings, pack_infos
    rect = [[0.0, 0.0, 0.5, 0.0], [0.5, 0.0, 0.5, 0.02], [0.5, 0.02, 0.0, 0.02], [0.0, 0.02, 0.0, 0.0]]
    row, rviews = SR.tiled_cells(8, 1, 0.1, 0.02)                             # eight thin cells in a row: one merged box
    files = R.write_infos(str(tmp_path), [_info("rect", rect, [0] * 4), _info("row", row, rviews)])
    # NOISE_RATIO 1.0 on the rectangle: whenever a line is deleted or shortened its only face is gone -> the clean drawing
    cfg = SR.make_data_cfg(4 * 1 + 2, 20, aug_ratio=1.0, noise_ratio=1.0, noise_length=0.3)
    packed = pack_infos(str(tmp_path), files, "sideface", extract=True, data_cfg=cfg)
    assert packed["n_faces"].tolist() == [1, 1]                               # each fills the row of ONE face
    dd = DeviceDrawings(packed, TOKEN, cfg, "cuda")
    clean = _batch(dd, [0, 1])
    seen = 0
    for epoch in range(6):
        got, flags = _check_against_restatement(dd, packed, cfg, [0], epoch)
        assert torch.equal(got["input_value"], clean["input_value"][:1])      # intact or fallen back: the clean row either way
        seen |= int(flags[0])
    assert seen == D.EXTRACT_FELL_BACK
    # the row of cells under a little noise: a deleted piece of its boundary splits the merged box in two, one more than fits
    cfg2 = SR.make_data_cfg(4 * 1 + 2, 20, aug_ratio=1.0, noise_ratio=0.1, noise_length=0.3)
    dd2 = DeviceDrawings(packed, TOKEN, cfg2, "cuda")
    seen = 0
    for epoch in range(12):
        got, flags = _check_against_restatement(dd2, packed, cfg2, [1], epoch)
        assert int(got["_n_faces"][0]) <= 1
        seen |= int(flags[0])
    assert seen & D.EXTRACT_TRUNCATED


def test_a_drawing_outside_the_domain_sets_its_flag(edge_set):
    from plankassembly_amd.device_data import DeviceDrawings
    root, files, cfg, packed, _ = edge_set
    bad = dict(packed, seg=packed["seg"].copy())
    lo = packed["line_off"]
    bad["seg"][lo[2]] = [0.0, 0.0, 0.5, 0.3]                                  # the rectangle gets a diagonal ...
    bad["seg"][lo[4] + 1] = bad["seg"][lo[4]]                                 # ... tiles257 a duplicate line ...
    bad["seg"][lo[5]] = [0.0, 0.0, float("nan"), 0.0]                         # ... and tiles1024 a NaN: none went through pack_infos
    dd = DeviceDrawings(bad, TOKEN, cfg, "cuda")
    got = _batch(dd, [2, 3, 4, 5])
    torch.cuda.synchronize()
    assert got["_extract_flags"].cpu().tolist() == [1, 0, 1, 1] and got["_n_faces"].cpu().tolist()[0::2] == [0, 0]
    for r in (0, 2, 3):
        row = got["input_value"][r].cpu()
        assert row[0] == TOKEN.END and bool((row[1:] == TOKEN.PAD).all()) and bool(got["input_mask"][r, 1:].all())
        assert not got["input_pos"][r].any() and int(got["_n_tokens"][r]) == 1
    want = SR.sample(packed, 3, cfg, TOKEN)[0]
    _same_rows(got, {k: want[k][None] for k in KEYS}, rows=slice(1, 2))      # the drawing between them is untouched


# ---------------------------------------------------------------------------------------------- the trainer
def _write_config(tmp_path, device, aug_ratio, n=9):
    root = str(tmp_path / "data" / "infos")
    names = R.write_infos(root, [SR.render_drawing(np.random.default_rng(40 + i), 3 + i % 5, f"drawing{i:02d}") for i in range(n)])
    split = tmp_path / "all.txt"
    split.write_text("\n".join(names))
    with open(os.path.join(REPO, "configs", "train_sideface.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["trainer"].update(max_epochs=1, check_val_every_n_epoch=1, devices=1)
    hp = cfg["model"]["hparams"]
    hp.update(ROOT=root, DATASETS_TRAIN=str(split), DATASETS_VALID=str(split), DATASETS_TEST=str(split), BATCH_SIZE=4,
              NUM_WORKERS=0, LR=2e-3, DEVICE_DATASET=device)
    hp["DATA"].update(MAX_INPUT_LENGTH=4 * 50 + 2, MAX_OUTPUT_LENGTH=60, AUG_RATIO=aug_ratio, NOISE_RATIO=0.15, NOISE_LENGTH=0.02)
    hp["MODEL"].update(NUM_MODEL=64, NUM_HEAD=4, NUM_FEEDFORWARD=128, NUM_ENCODER_LAYERS=2, NUM_DECODER_LAYERS=2, DROPOUT=0.0,
                       COMPUTE_DTYPE="f32")
    path = tmp_path / f"sideface_{'device' if device else 'cpu'}_{aug_ratio}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path), hp


def test_fit_two_steps_on_extracted_augmented_data(tmp_path, monkeypatch):
    from plankassembly_amd.device_data import DeviceLoader
    from plankassembly_amd.trainer import SidefaceTrainer, cli
    monkeypatch.chdir(tmp_path)
    config, _ = _write_config(tmp_path, True, 1.0)
    mod = cli(SidefaceTrainer, ["fit", "--config", config, "--trainer.max_steps", "2"])
    loader = mod.train_dataloader()
    assert isinstance(loader, DeviceLoader) and loader.augmentation and loader.drawings.extract and loader.drawings.augments(True)
    assert mod.global_step == 2
    losses = [v for _, name, v in mod.logger.history if name == "train/loss"]
    assert len(losses) == 1 and np.isfinite(losses[0])
    batch = next(iter(loader))
    assert "_extract_flags" in batch and batch["input_value"].shape == (4, 201)
    # without augmentation the device loader's batch gives the loss bits of the CPU loader's
    results = []
    for device in (True, False):
        _, hp = _write_config(tmp_path, device, 0.0)
        torch.manual_seed(5)
        m = SidefaceTrainer(hp)
        m.model.cuda().train()
        loader = m.val_dataloader()
        assert isinstance(loader, DeviceLoader) == device
        out = m.model(m.model.prepare_batch(next(iter(loader))))
        results.append(out["loss"].detach().float().cpu())
    assert torch.isfinite(results[0]).all() and results[0].view(torch.int32).equal(results[1].view(torch.int32)), results
