"""The device dataset on the host (plankassembly_amd/device_data.py): ``pack_infos`` against the info
files, the numpy restatement (tests/device_data_reference.py) against the CPU classes it must equal, its augmentation arithmetic
against ``datasets.add_noise`` fed the same decisions, the branches the generated augmentation set takes, and the quality of the
counter-based draws.  tests/test_device_data_gpu.py then pins the kernel to the restatement."""
import json
import math
import os
import types

import numpy as np
import pytest

import device_data_reference as R
from conftest import GOLDEN
from plankassembly_amd import datasets as D
from plankassembly_amd.device_data import DeviceDrawings, pack_infos

TOKEN = types.SimpleNamespace(END=512, PAD=513)
INFOS = os.path.join(GOLDEN, "infos")
GOLDEN_FILES = ["item0.json", "item1.json", "item2.json"]


def _same_sample(got, want):
    assert list(got) == list(want)
    for k in want:
        if k == "name":
            assert got[k] == want[k]
        else:
            a, b = np.asarray(got[k]), np.asarray(want[k])
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k


@pytest.mark.parametrize("kind", ["line", "sideface"])
def test_pack_round_trips_the_golden_infos(kind):
    packed = pack_infos(INFOS, GOLDEN_FILES, kind)
    assert packed["line_off"].dtype == np.int32 and packed["plank_off"].dtype == np.int32
    assert packed["box"].dtype == np.float64 and packed["coords"].dtype == np.float64
    assert packed["view"].dtype == np.uint8 and packed["attach"].dtype == np.int32
    for i, fn in enumerate(GOLDEN_FILES):
        with open(os.path.join(INFOS, fn)) as f:
            info = json.load(f)
        lo, hi = packed["line_off"][i], packed["line_off"][i + 1]
        plo, phi = packed["plank_off"][i], packed["plank_off"][i + 1]
        assert packed["names"][i] == info["name"]
        assert np.array_equal(packed["box"][lo:hi], np.array(info["lines" if kind == "line" else "faces"], dtype=float).reshape(-1, 4))
        assert np.array_equal(packed["view"][lo:hi], np.array(info["views" if kind == "line" else "faceviews"]))
        assert np.array_equal(packed["coords"][plo:phi], np.array(info["coords"], dtype=float))
        assert np.array_equal(packed["attach"][plo:phi], np.array(info["attach"]))
        if kind == "line":
            assert packed["type"].dtype == np.uint8 and np.array_equal(packed["type"][lo:hi], np.array(info["types"]))
            segs = np.stack([D._segment_points(s).reshape(4) for s in info["svgs"]])
            assert np.array_equal(packed["seg"][lo:hi], segs)
        else:
            assert "seg" not in packed and "type" not in packed


def test_pack_and_construction_errors(tmp_path):
    rng = np.random.default_rng(0)
    info = R.random_info(rng, "d0", (5, 5), (3, 3))
    files = R.write_infos(str(tmp_path), [info])
    # side faces not stored: the CPU class's error
    with pytest.raises(NotImplementedError, match="side-face extraction"):
        pack_infos(str(tmp_path), files, "sideface")
    packed = pack_infos(str(tmp_path), files, "line")
    DeviceDrawings(packed, TOKEN, R.make_data_cfg(22, 19), "cpu")                        # 4 * 5 + 1 = 21 rows, 6 * 3 + 1 = 19: both fit exactly
    with pytest.raises(ValueError, match=r"d0\.json: 20 input tokens do not fit MAX_INPUT_LENGTH=21"):
        DeviceDrawings(packed, TOKEN, R.make_data_cfg(21, 19), "cpu")
    with pytest.raises(ValueError):                                                      # ... as LineDataset does
        D.LineDataset(str(tmp_path), files, TOKEN, R.make_data_cfg(21, 19))[0]
    with pytest.raises(ValueError, match=r"d0\.json: 18 output tokens do not fit MAX_OUTPUT_LENGTH=18"):
        DeviceDrawings(packed, TOKEN, R.make_data_cfg(22, 18), "cpu")
    with pytest.raises(ValueError):
        D.LineDataset(str(tmp_path), files, TOKEN, R.make_data_cfg(22, 18))[0]
    # a polyline: straight segments only, the message names the CPU class
    bent = dict(info, name="bent")
    bent["svgs"] = list(info["svgs"])
    bent["svgs"][2] = {"type": "LineString", "coordinates": [[0.0, 0.0], [0.1, 0.0], [0.1, 0.2]]}
    files = R.write_infos(str(tmp_path), [bent])
    with pytest.raises(ValueError, match=r"bent\.json.*LineDataset"):
        pack_infos(str(tmp_path), files, "line")


def _generated(tmp_path, faces):
    rng = np.random.default_rng(3)
    infos = [R.random_info(rng, f"g{i:02d}", (0, 29) if faces else (1, 29), (1, 9), faces) for i in range(12)]
    return R.write_infos(str(tmp_path), infos)


@pytest.mark.parametrize("kind", ["line", "sideface"])
def test_restatement_equals_the_cpu_dataset(kind, tmp_path):
    cls = D.LineDataset if kind == "line" else D.SidefaceDataset
    for root, files in ((INFOS, GOLDEN_FILES), (str(tmp_path), _generated(tmp_path, kind == "sideface"))):
        cfg = R.make_data_cfg(120, 60)
        ds = cls(root, files, TOKEN, cfg)
        packed = pack_infos(root, files, kind)
        for i in range(len(files)):
            got, dec = R.sample(packed, i, cfg, TOKEN)
            assert dec is None
            _same_sample(got, ds[i])


class _QueueRng:
    """``rng`` of datasets.add_noise that replays recorded decisions."""

    def __init__(self, num_select, indices, randoms):
        self.num_select, self.indices, self.randoms = num_select, indices, list(randoms)

    def randint(self, low, high):
        assert low <= self.num_select < high, (low, self.num_select, high)
        return self.num_select

    def choice(self, n, size, replace):
        assert size == self.num_select == len(self.indices) and not replace and self.indices.max() < n
        return self.indices

    def random(self):
        return self.randoms.pop(0)


def test_augmentation_arithmetic_equals_add_noise_and_covers_every_branch():
    infos, cfg = R.augmentation_set()
    seen = set()
    for epoch in range(3):
        for d, info in enumerate(infos):
            segs = np.stack([D._segment_points(s).reshape(4) for s in info["svgs"]])
            out, keep, dec = R.augment(segs, 7, epoch, d, cfg.AUG_RATIO, cfg.NOISE_RATIO, cfg.NOISE_LENGTH)
            seen |= R.branches_of(dec, len(segs))
            if not dec.augmented:
                assert keep.all() and np.array_equal(out, segs)
                continue
            assert 1 <= dec.num_select <= math.ceil(len(segs) * cfg.NOISE_RATIO)
            rng = _QueueRng(*dec.queue())
            lines, views, typs = D.add_noise([D._segment_points(s) for s in info["svgs"]], list(info["views"]), list(info["types"]),
                                             cfg.NOISE_RATIO, cfg.NOISE_LENGTH, rng=rng)
            assert not rng.randoms                                          # every exported decision was consumed
            assert views == [v for v, k in zip(info["views"], keep) if k] and typs == [t for t, k in zip(info["types"], keep) if k]
            want = np.stack([ln.reshape(4) for ln in lines]) if lines else np.zeros((0, 4))
            assert want.tobytes() == out[keep].tobytes()                    # bit for bit
            if lines:
                assert np.array_equal(D._bounds(lines), R.bounds(out[keep]))
    assert seen == set(R.BRANCHES), set(R.BRANCHES) - seen


def test_draw_quality():
    """Over 4 096 drawings of 1-40 lines: each share within 5 standard deviations of a binomial at the nominal probability,
    5 * sqrt(p (1 - p) / n)."""
    rng = np.random.default_rng(17)
    n_draw, aug_ratio, noise_ratio = 4096, 0.5, 0.5
    augmented = selected = by_coin = reached_end = tail = 0
    for d in range(n_draw):
        n = int(rng.integers(1, 41))
        p0 = rng.uniform(-1, 1, size=(n, 2))
        segs = np.concatenate([p0, np.clip(p0 + rng.uniform(-0.6, 0.6, size=(n, 2)), -1, 1)], axis=1)
        _, keep, dec = R.augment(segs, 2022, d % 5, d, aug_ratio, noise_ratio, 0.3)
        if not dec.augmented:
            continue
        augmented += 1
        assert 1 <= dec.num_select <= math.ceil(n * noise_ratio) and len(set(dec.indices)) == dec.num_select
        for i in dec.indices:
            selected += 1
            by_coin += dec.branch[i] == "deleted_by_coin"
            if dec.end_u[i] is not None:
                reached_end += 1
                tail += dec.branch[i] == "shortened_tail"

    def within(k, n, p):
        assert n > 1000 and abs(k / n - p) <= 5 * math.sqrt(p * (1 - p) / n), (k, n, p)

    within(augmented, n_draw, aug_ratio)
    within(by_coin, selected, 0.5)
    within(tail, reached_end, 0.5)
