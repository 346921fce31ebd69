"""The device dataset on the GPU (plankassembly_amd/device_data.py, csrc/tokenise.hip `pa_tokenise_drawings`; DESIGN.md section
17).  Augmentation off: the device batch IS the batch `DataLoader` collates from the CPU dataset - every key, dtype, shape and
value.  Augmentation on: it is the numpy restatement (tests/device_data_reference.py, pinned to the CPU classes by
tests/test_device_data_cpu.py) bit for bit.  Then the loader's order, `_n_valid`, a train step, and the command line."""
import json
import os
import types

import numpy as np
import pytest
import torch
import yaml

import device_data_reference as R
from conftest import GOLDEN
from plankassembly_amd import datasets as D

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKEN = types.SimpleNamespace(END=512, PAD=513)
INFOS = os.path.join(GOLDEN, "infos")
GOLDEN_FILES = ["item0.json", "item1.json", "item2.json"]


def _drawings(root, files, cfg, kind="line"):
    from plankassembly_amd.device_data import DeviceDrawings, pack_infos
    packed = pack_infos(root, files, kind)
    return DeviceDrawings(packed, TOKEN, cfg, "cuda"), packed


def _all(dd, **kw):
    return dd.batch(torch.arange(len(dd), dtype=torch.int32, device="cuda"), **kw)


def _public(batch):
    return {k: v for k, v in batch.items() if not k.startswith("_")}


def _cpu_batch(kind, root, files, cfg):
    cls = D.LineDataset if kind == "line" else D.SidefaceDataset
    return next(iter(torch.utils.data.DataLoader(cls(root, files, TOKEN, cfg), batch_size=len(files), shuffle=False)))


def _same_batch(got, want):
    """Keys, order, dtypes, shapes, values; ``want`` holds torch tensors (DataLoader) or numpy arrays (the restatement)."""
    got = _public(got)
    assert list(got) == list(want)
    for k, w in want.items():
        if k == "name":
            assert list(got[k]) == list(w)
            continue
        w = torch.from_numpy(w) if isinstance(w, np.ndarray) else w
        g = got[k]
        assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        bad = (g.cpu() != w).nonzero()
        assert len(bad) == 0, (k, bad[:4].tolist())


def _check_counts(batch):
    n = (~batch["input_mask"]).sum(1).to(torch.int32)
    assert torch.equal(batch["_n_tokens"], n)
    if "_n_valid" in batch:
        assert batch["_n_valid"] == int(n.sum())


@pytest.mark.parametrize("kind", ["line", "sideface"])
def test_golden_infos_equal_the_cpu_dataset(kind):
    cfg = R.make_data_cfg(120, 60)
    dd, _ = _drawings(INFOS, GOLDEN_FILES, cfg, kind)
    got = _all(dd)
    _same_batch(got, _cpu_batch(kind, INFOS, GOLDEN_FILES, cfg))
    assert ("input_type" in got) == (kind == "line") and isinstance(got["_n_valid"], int)
    _check_counts(got)


def _info(name, lines, views, types_, coords, attach, faces=False):
    """An info dict whose ``lines`` are exactly ``lines`` (R.make_info would order each box)."""
    info = R.make_info(name, lines, views, types_, coords, attach, faces)
    info["lines"] = np.asarray(lines, dtype=np.float64).reshape(-1, 4).tolist()
    if faces:
        info["faces"] = info["lines"]
    return info


def _quantiser_edges(ks):
    """Per k: 2k/511 - 1 rounded to three decimals, itself, and the nearest float64 on either side (inside [-1, 1])."""
    rows = []
    for k in ks:
        v = 2.0 * k / 511.0 - 1.0
        rows.append(np.clip([round(v, 3), v, np.nextafter(v, -2.0), np.nextafter(v, 2.0)], -1.0, 1.0))
    return np.asarray(rows)


def _edge_infos(max_lines, max_planks, faces=False):
    """The shapes at which the tokeniser can go wrong, for a row of ``4 * max_lines + 1`` tokens and ``max_planks`` planks."""
    rng = np.random.default_rng(23)
    nopt = (np.zeros((1, 6)), np.full((1, 6), -1))
    full_c, full_a = R.random_planks(rng, max_planks)
    assert (full_a != -1).any()
    one = rng.uniform(-1, 1, size=(1, 4)).round(3)
    full = rng.uniform(-1, 1, size=(max_lines, 4)).round(3)
    twin = np.repeat(rng.uniform(-1, 1, size=(3, 4)).round(3), 4, axis=0)          # three boxes, four copies each
    edges = _quantiser_edges([0, 1, 2, 3, 127, 128, 255, 256, 257, 383, 509, 510, 511] + list(range(40, 40 + max_lines - 13)))
    ends = np.array([[-1.0, -1.0, 1.0, 1.0], [1.0, 1.0, -1.0, -1.0], [-1.0, 1.0, -1.0, 1.0]])
    infos = [
        _info("one_line", one, [2], [1], *nopt, faces),
        _info("fills_row", full, rng.integers(0, 3, max_lines), rng.integers(0, 2, max_lines), full_c, full_a, faces),
        _info("equal_boxes_types", twin, [1] * 12, [0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0], *R.random_planks(rng, 3), faces),
        _info("equal_boxes_views", twin, [2, 0, 1, 0, 1, 1, 0, 2, 0, 2, 2, 1], [0] * 12, *R.random_planks(rng, 2), faces),
        _info("quantiser_edges", edges[:max_lines], rng.integers(0, 3, max_lines), rng.integers(0, 2, max_lines),
              np.clip(_quantiser_edges(range(300, 306)).T.reshape(-1, 6), -1, 1), np.full((4, 6), -1), faces),
        _info("ends", ends, [0, 0, 1], [0, 1, 0], [[-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]], [[-1] * 6], faces),
    ]
    if faces:
        infos.append(_info("no_faces", np.zeros((0, 4)), [], [], *R.random_planks(rng, 2), True))
    return infos


@pytest.mark.parametrize("kind", ["line", "sideface"])
def test_edge_shapes_equal_the_cpu_dataset(kind, tmp_path):
    """One line; a row filled exactly (4 n + 1 == MAX_INPUT_LENGTH - 1); equal boxes with different types / in different views;
    coordinates at the quantiser's edges and at -1 / 1; 1 plank and (T - 1) // 6 planks; pointers present and absent; for
    side faces the empty drawing."""
    cfg = R.make_data_cfg(122, 60)                                           # 30 lines fill the row; (60 - 1) // 6 = 9 planks
    files = R.write_infos(str(tmp_path), _edge_infos(30, 9, kind == "sideface"))
    dd, packed = _drawings(str(tmp_path), files, cfg, kind)
    assert 4 * int(np.diff(packed["line_off"]).max()) + 1 == cfg.MAX_INPUT_LENGTH - 1
    got = _all(dd)
    _same_batch(got, _cpu_batch(kind, str(tmp_path), files, cfg))
    _check_counts(got)
    if kind == "sideface":
        row = got["input_value"][-1].cpu()
        assert row[0] == TOKEN.END and bool((row[1:] == TOKEN.PAD).all()) and not got["input_pos"][-1].any()


@pytest.fixture(scope="module")
def long_set(tmp_path_factory):
    """MAX_INPUT_LENGTH 1200: a drawing of 280 lines (a thread of the block takes more than one) among shorter ones, 21 planks."""
    root = str(tmp_path_factory.mktemp("long"))
    rng = np.random.default_rng(29)
    infos = [R.random_info(rng, "long280", (280, 280), (21, 21)), R.random_info(rng, "long299", (299, 299), (2, 2)),
             R.random_info(rng, "mid", (257, 257), (5, 5)), R.random_info(rng, "short", (3, 3), (1, 1))]
    return root, R.write_infos(root, infos), R.make_data_cfg(1200, 128)


def test_more_lines_than_threads(long_set):
    root, files, cfg = long_set
    dd, _ = _drawings(root, files, cfg)
    got = _all(dd)
    _same_batch(got, _cpu_batch("line", root, files, cfg))
    _check_counts(got)


@pytest.fixture(scope="module")
def aug_set(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("aug"))
    infos, cfg = R.augmentation_set()
    files = R.write_infos(root, infos)
    dd, packed = _drawings(root, files, cfg)
    want = {e: [R.sample(packed, i, cfg, TOKEN, True, 7, e) for i in range(len(files))] for e in range(3)}
    return dd, packed, cfg, want


def test_augmented_batches_equal_the_restatement(aug_set):
    dd, packed, cfg, want = aug_set
    seen = set()
    for epoch, samples in want.items():
        got = _all(dd, epoch=epoch, augmentation=True, seed=7)
        assert "_n_valid" not in got                                          # the count depends on the deleted lines
        _same_batch(got, R.collate([s for s, _ in samples]))
        _check_counts(got)
        for i, (_, dec) in enumerate(samples):
            seen |= R.branches_of(dec, int(packed["line_off"][i + 1] - packed["line_off"][i]))
    assert seen == set(R.BRANCHES)
    off = _all(dd, epoch=0, augmentation=False)
    assert "_n_valid" in off and not torch.equal(off["input_value"], got["input_value"])


def test_augmentation_is_a_function_of_seed_epoch_and_drawing(aug_set):
    dd, packed, cfg, want = aug_set
    full = {e: _all(dd, epoch=e, augmentation=True, seed=7) for e in (0, 1)}
    again = _all(dd, epoch=0, augmentation=True, seed=7)
    perm = np.random.default_rng(1).permutation(len(dd)).astype(np.int32)
    for bs in (3, 5):
        for lo in range(0, len(perm), bs):
            idx = perm[lo:lo + bs]
            part = dd.batch(torch.from_numpy(idx).cuda(), epoch=0, augmentation=True, seed=7, host_index=idx)
            for k, v in _public(part).items():
                if k != "name":
                    assert torch.equal(v, full[0][k][torch.from_numpy(idx).long().cuda()]), (k, bs, lo)
    augmented = [i for i, (_, dec) in enumerate(want[0]) if dec.augmented and want[1][i][1].augmented]
    assert augmented and any(not torch.equal(full[0]["input_value"][i], full[1]["input_value"][i]) for i in augmented)
    other_seed = _all(dd, epoch=0, augmentation=True, seed=8)
    assert not torch.equal(other_seed["input_value"], full[0]["input_value"])
    for k, v in _public(again).items():
        if k != "name":
            assert torch.equal(v, full[0][k]), k


def test_loader_order_length_and_batches(aug_set):
    from plankassembly_amd.device_data import DeviceLoader
    dd, packed, cfg, _ = aug_set
    n, names = len(dd), list(packed["names"])
    train = DeviceLoader(dd, 5, shuffle=True, drop_last=True, augmentation=False, seed=3)
    assert len(train) == n // 5
    orders = []
    for epoch in (0, 1, 0):
        train.set_epoch(epoch)
        batches = list(train)
        assert len(batches) == len(train) and all(b["input_value"].shape[0] == 5 for b in batches)
        order = [names.index(x) for b in batches for x in b["name"]]
        assert len(set(order)) == len(order) == 5 * (n // 5)                  # a permutation, cut by drop_last
        orders.append(order)
    assert orders[0] == orders[2] and orders[0] != orders[1] and orders[0] != sorted(orders[0])
    whole = _all(dd)
    for b in batches[:3]:
        rows = torch.tensor([names.index(x) for x in b["name"]], device="cuda")
        assert torch.equal(b["input_value"], whole["input_value"][rows]) and torch.equal(b["output_label"], whole["output_label"][rows])
        _check_counts(b)
    evalu = DeviceLoader(dd, 5, shuffle=False, drop_last=False)
    batches = list(evalu)
    assert len(evalu) == len(batches) == -(-n // 5) and batches[-1]["input_value"].shape[0] == n - 5 * (n // 5)
    assert [x for b in batches for x in b["name"]] == names                   # sequential, last partial batch kept
    assert torch.equal(torch.cat([b["input_value"] for b in batches]), whole["input_value"])


def test_train_step_equals_the_cpu_collated_batch(long_set, tiny_fixture):
    """Same loss bits and same gradients from the device batch (its host-known `_n_valid`) and from the CPU-collated batch moved
    to the device: tiny_fixture's model (d 128, 2 + 2 layers, MAX_INPUT_LENGTH 1200), f32, dropout 0."""
    from plankassembly_amd.models import PlankModel
    root, files, cfg = long_set
    sd, _, _ = tiny_fixture
    m = PlankModel(128, 8, 256, 0.0, "relu", True, 2, 2, 3, 2, 4, 6, 1200, 128, 514, TOKEN, compute_dtype="f32")
    m.load_state_dict(sd)
    m = m.cuda().train()
    dd, _ = _drawings(root, files, cfg)
    cpu = _cpu_batch("line", root, files, cfg)
    results = []
    for batch in (_all(dd), cpu):
        for p in m.parameters():
            p.grad = None
        out = m(m.prepare_batch(batch))
        out["loss"].backward()
        torch.cuda.synchronize()
        results.append((out["loss"].detach().cpu(), {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}))
    (l_dev, g_dev), (l_cpu, g_cpu) = results
    assert torch.isfinite(l_dev).all() and l_dev.view(torch.int32).equal(l_cpu.view(torch.int32)), (l_dev, l_cpu)
    for k in g_cpu:
        assert torch.equal(g_dev[k], g_cpu[k]), k
    assert any(bool(g.any()) for g in g_dev.values())


# ---------------------------------------------------------------------------------------------- command line
def _write_config(tmp_path, device, aug_ratio=0.0, n=9):
    rng = np.random.default_rng(11)
    root = str(tmp_path / "data" / "infos")
    names = R.write_infos(root, [R.random_info(rng, f"drawing{i:02d}", (3, 25), (2, 8)) for i in range(n)])
    split = tmp_path / "all.txt"
    split.write_text("\n".join(names))
    with open(os.path.join(REPO, "configs", "train_complete.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["trainer"].update(max_epochs=1, check_val_every_n_epoch=1, devices=1)
    hp = cfg["model"]["hparams"]
    hp.update(ROOT=root, DATASETS_TRAIN=str(split), DATASETS_VALID=str(split), DATASETS_TEST=str(split), BATCH_SIZE=4,
              NUM_WORKERS=0, LR=2e-3, DEVICE_DATASET=device)
    hp["DATA"].update(MAX_INPUT_LENGTH=129, MAX_OUTPUT_LENGTH=60, AUG_RATIO=aug_ratio, NOISE_RATIO=0.5, NOISE_LENGTH=0.3)
    hp["MODEL"].update(NUM_MODEL=64, NUM_HEAD=4, NUM_FEEDFORWARD=128, NUM_ENCODER_LAYERS=2, NUM_DECODER_LAYERS=2, DROPOUT=0.0,
                       COMPUTE_DTYPE="f32")
    path = tmp_path / f"small_{'device' if device else 'cpu'}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


def test_cli_test_writes_the_same_predictions(tmp_path, monkeypatch):
    from plankassembly_amd.device_data import DeviceLoader
    from plankassembly_amd.trainer import Trainer, cli
    monkeypatch.chdir(tmp_path)
    runs = {}
    for device in (False, True):
        mod = cli(Trainer, ["test", "--config", _write_config(tmp_path, device)])
        assert isinstance(mod.test_dataloader(), DeviceLoader) == device
        out_dir = os.path.join(mod.logger.log_dir, "pred_jsons")
        preds = {}
        for fn in sorted(os.listdir(out_dir)):
            with open(os.path.join(out_dir, fn)) as f:
                preds[fn] = json.load(f)
        runs[device] = (preds, {k: v for k, v in mod._logged.items() if k.startswith("test/")})
    assert len(runs[True][0]) == 9 and runs[True][0] == runs[False][0]
    assert len(runs[True][1]) == 3 and runs[True][1] == runs[False][1]


def test_cli_fit_two_steps_with_augmentation(tmp_path, monkeypatch):
    from plankassembly_amd.device_data import DeviceLoader
    from plankassembly_amd.trainer import Trainer, cli
    monkeypatch.chdir(tmp_path)
    config = _write_config(tmp_path, True, aug_ratio=0.5)
    mod = cli(Trainer, ["fit", "--config", config, "--trainer.max_steps", "2"])
    loader = mod.train_dataloader()
    assert isinstance(loader, DeviceLoader) and loader.augmentation and loader.drawings.augments(True) and len(loader) == 2
    assert mod.global_step == 2
    losses = [v for _, name, v in mod.logger.history if name == "train/loss"]
    assert len(losses) == 1 and np.isfinite(losses[0])
    assert os.path.exists(os.path.join(mod.logger.log_dir, "checkpoints", "last.ckpt"))
