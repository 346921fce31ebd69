"""Side-face extraction on the host (plankassembly_amd/datasets.py `extract_sideface`): hand-written
drawings with their boxes written out, generated drawings against the flood-fill oracle of tests/sideface_reference.py, the
invariances the defined candidate order gives, and the pack / dataset / trainer surface."""
import itertools
import types

import numpy as np
import pytest
import torch

import device_data_reference as R
import sideface_reference as SR
from plankassembly_amd import datasets as D

TOKEN = types.SimpleNamespace(END=512, PAD=513)
MAXT, MINT, TOL = 0.04, 0.004, 0.004                      # thresholds of the hand-written cases (already over SCALE)


def rect(x0, y0, x1, y1):
    return [[x0, y0, x1, y0], [x1, y0, x1, y1], [x1, y1, x0, y1], [x0, y1, x0, y0]]


def extract(segs, views=None, thresholds=(MAXT, MINT, TOL)):
    segs = np.asarray(segs, dtype=np.float64).reshape(-1, 4)
    faces, fviews = D.extract_sideface(segs, [0] * len(segs) if views is None else views, *thresholds)
    assert faces.shape == (len(fviews), 4) and faces.dtype == np.float64
    return faces.tolist(), list(fviews)


# ------------------------------------------------------------------------------------------------ hand-written drawings
def test_one_thin_rectangle():
    assert extract(rect(0.0, 0.0, 0.5, 0.02)) == ([[0.0, 0.0, 0.5, 0.02]], [0])
    assert extract(rect(0.25, -0.5, 0.27, 0.5), [2] * 4) == ([[0.25, -0.5, 0.27, 0.5]], [2])


def test_a_thick_square_gives_nothing():
    assert extract(rect(0.0, 0.0, 0.5, 0.5)) == ([], [])


def test_a_row_of_thin_cells_merges_into_one_box():
    segs, views = SR.tiled_cells(3, 1, 0.1, 0.02, x0=0.0, y0=0.0)
    assert extract(segs, views) == ([[0.0, 0.0, 0.3, 0.02]], [0])


def test_rows_whose_widths_differ_by_the_tolerance_do_not_merge():
    # two cells side by side at the same centre line, widths 0.02 and 0.028 (the second is taller, centred alike)
    segs = rect(0.0, 0.0, 0.1, 0.02) + [[0.1, -0.004, 0.2, -0.004], [0.2, -0.004, 0.2, 0.024], [0.2, 0.024, 0.1, 0.024],
                                        [0.1, 0.024, 0.1, 0.02], [0.1, 0.0, 0.1, -0.004]]
    faces, _ = extract(segs)
    assert sorted(faces) == [[0.0, 0.0, 0.1, 0.02], [0.1, -0.004, 0.2, 0.024]]
    # ... and merge once the tolerance exceeds the difference: the later candidate's width is kept
    faces, _ = extract(segs, thresholds=(MAXT, MINT, 0.009))
    assert faces == [[0.0, 0.01 - 0.014, 0.2, 0.01 + 0.014]]
    # two adjacent rows (stacked; binary fractions, so the boxes are exact): different centre lines never merge
    a, b = 0.015625, 0.0234375
    faces, _ = extract(rect(0.0, 0.0, 0.5, a) + [[0.5, a, 0.5, b], [0.5, b, 0.0, b], [0.0, b, 0.0, a]])
    assert sorted(faces) == [[0.0, 0.0, 0.5, a], [0.0, a, 0.5, b]]


def test_a_small_square_gives_a_box_of_each_type():
    assert extract(rect(0.0, 0.0, 0.01, 0.01)) == ([[0.0, 0.0, 0.01, 0.01], [0.0, 0.0, 0.01, 0.01]], [0, 0])


def test_a_width_below_the_minimum_is_dropped():
    assert extract(rect(0.0, 0.0, 0.5, 0.003)) == ([], [])
    assert extract(rect(0.0, 0.0, 0.5, 0.004)) == ([[0.0, 0.0, 0.5, 0.004]], [0])


def test_dangles_are_pruned():
    thin = rect(0.0, 0.0, 0.5, 0.02)
    want = ([[0.0, 0.0, 0.5, 0.02]], [0])
    assert extract(thin + [[0.5, 0.02, 0.7, 0.02]]) == want
    chain = [[0.5, 0.02, 0.7, 0.02], [0.7, 0.02, 0.7, 0.3], [0.7, 0.3, 0.6, 0.3], [0.0, 0.0, -0.2, 0.0], [-0.2, 0.0, -0.2, -0.1]]
    assert extract(thin + chain) == want
    assert extract(chain) == ([], [])                             # a drawing of dangles alone


A, B = 0.015625, 0.03125                                  # 1/64 and 1/32: binary fractions, so the written boxes are exact


def test_two_rectangles_joined_by_a_bridge():
    # the bridge starts and ends at corners: a cut edge with the outer ring on both sides
    segs = rect(0.0, 0.0, 0.25, A) + [[0.25, A, 0.5, A]] + rect(0.5, A, 0.875, B)
    faces, _ = extract(segs)
    assert sorted(faces) == [[0.0, 0.0, 0.25, A], [0.5, A, 0.875, B]]
    assert SR.faces_by_flood_fill(segs) == [(0.0, 0.0, 0.25, A), (0.5, A, 0.875, B)]
    assert len(D.view_faces(segs, [0] * 9, 0)[0]) == 2


def test_two_rectangles_sharing_only_a_corner():
    faces, _ = extract(rect(0.0, 0.0, 0.25, A) + rect(0.25, A, 0.5, B))
    assert sorted(faces) == [[0.0, 0.0, 0.25, A], [0.25, A, 0.5, B]]


def test_a_rectangle_with_an_island():
    # the thick outer face keeps its outer bounds (nothing thin); the island is a thin face of its own
    faces, _ = extract(rect(0.0, 0.0, 0.5, 0.5) + rect(0.125, 0.125, 0.375, 0.125 + A))
    assert faces == [[0.125, 0.125, 0.375, 0.125 + A]]
    # a thin frame around an island: the frame's face has the outer bounds, the hole's ring is discarded
    segs = rect(0.0, 0.0, 0.5, B) + rect(0.125, A / 2, 0.375, A)
    assert sorted(extract(segs)[0]) == [[0.0, 0.0, 0.5, B], [0.125, A / 2, 0.375, A]]
    assert sorted(map(tuple, D.view_faces(segs, [0] * 8, 0)[0].tolist())) == SR.faces_by_flood_fill(segs)


def test_an_un_noded_t_junction_divides_nothing():
    # the stem ends on the interior of the top edge: no node there, so the stem is a dangle and the cell is one face
    segs = rect(0.0, 0.0, 0.5, 0.02) + [[0.25, 0.0, 0.25, 0.02]]
    assert extract(segs) == ([[0.0, 0.0, 0.5, 0.02]], [0])
    # noded (the edges split at the stem's ends) the two cells are two faces - merged again, being collinear
    noded = [[0.0, 0.0, 0.25, 0.0], [0.25, 0.0, 0.5, 0.0], [0.5, 0.0, 0.5, 0.02], [0.5, 0.02, 0.25, 0.02], [0.25, 0.02, 0.0, 0.02],
             [0.0, 0.02, 0.0, 0.0], [0.25, 0.0, 0.25, 0.02]]
    assert len(D.view_faces(noded, [0] * 7, 0)[0]) == 2 and extract(noded) == ([[0.0, 0.0, 0.5, 0.02]], [0])


def test_views_beyond_two_empty_views_and_no_lines():
    thin = rect(0.0, 0.0, 0.5, 0.02)
    assert extract(thin + rect(0.0, 0.0, 0.3, 0.01), [1] * 4 + [3] * 4) == ([[0.0, 0.0, 0.5, 0.02]], [1])     # view 3 ignored
    assert extract(thin + rect(-0.5, 0.0, -0.2, 0.01), [2] * 4 + [0] * 4) == ([[-0.5, 0.0, -0.2, 0.01], [0.0, 0.0, 0.5, 0.02]], [0, 2])
    faces, fviews = D.extract_sideface(np.zeros((0, 4)), [], MAXT, MINT, TOL)
    assert faces.shape == (0, 4) and len(fviews) == 0
    assert extract(thin + [[0.1, 0.1, 0.1, 0.1]]) == ([[0.0, 0.0, 0.5, 0.02]], [0])                            # zero length dropped


def test_out_of_domain_drawings_are_refused():
    thin = rect(0.0, 0.0, 0.5, 0.02)
    for extra in ([[0.0, 0.0, 0.3, 0.3]], [thin[0]], [[0.0, 0.0, 0.2, 0.0]], [[0.5, 0.0, 1.5, 0.0]], [[0.5, 0.0, float("nan"), 0.0]]):
        with pytest.raises(ValueError, match="axis-aligned"):
            extract(thin + extra)
        faces, fviews, flags = D.extract_sideface_flags(np.asarray(thin + extra), [0] * 5, MAXT, MINT, TOL)
        assert len(faces) == 0 and len(fviews) == 0 and flags & D.EXTRACT_OUT_OF_DOMAIN
    assert extract(thin + [[0.2, -0.1, 0.2, 0.1]]) == ([[0.0, 0.0, 0.5, 0.02]], [0])      # a crossing away from end points is in
    assert extract(thin + [[-0.0, 0.0, -0.0, -0.3]]) == ([[0.0, 0.0, 0.5, 0.02]], [0])    # -0.0 is the node 0.0


# ------------------------------------------------------------------------------------------------ generated drawings
# Seeds 0 .. 39: every one passes the merge-order condition below, none had to be skipped.
SEEDS = list(range(40))


@pytest.fixture(scope="module")
def drawings():
    out = []
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        out.append(SR.info_segments(SR.render_drawing(rng, int(rng.integers(2, 13)), f"gen{seed:02d}")))
    assert max(len(s) for s, _ in out) > 150 and sum(len(D.extract_sideface(s, v, *SR.THRESHOLDS)[0]) for s, v in out) > 300
    return out


NOISE_SEEDS_SKIPPED = {0.15: 0, 0.5: 0}                    # filled by _noisy, printed below


def _noisy(seg, views, noise_ratio, seed):
    """``add_noise`` under the first generator seed (seed, seed + 100, ...) that leaves the drawing inside the ORACLE's domain
    (sideface_reference.meet_only_at_end_points: a drawn noise length of 0 can move an end point by an ulp)."""
    for attempt in range(20):
        rng = np.random.RandomState(seed + 100 * attempt)
        lines, v, _ = D.add_noise([s.reshape(2, 2) for s in seg], list(views), list(views), noise_ratio, 0.02, rng)
        lines, v = np.asarray(lines, dtype=np.float64).reshape(-1, 4), np.asarray(v, dtype=np.int64)
        if all(SR.meet_only_at_end_points(lines[v == k]) for k in range(3)):
            return lines, v
        NOISE_SEEDS_SKIPPED[noise_ratio] += 1
    raise AssertionError("no noise seed leaves the drawing inside the oracle's domain")


@pytest.mark.parametrize("noise_ratio", [0.0, 0.15, 0.5])
def test_faces_equal_the_flood_fill(drawings, noise_ratio):
    total = 0
    for k, (seg, views) in enumerate(drawings):
        if noise_ratio:
            seg, views = _noisy(seg, views, noise_ratio, k)
        for view in range(3):
            faces, flags = D.view_faces(seg, views, view)
            assert flags == 0
            assert sorted(map(tuple, faces.tolist())) == SR.faces_by_flood_fill(seg[views == view]), (k, view)
            total += len(faces)
    assert total > 500
    # measured: 11 generator seeds skipped over the 40 drawings at NOISE_RATIO 0.15, 24 at 0.5 - a drawn noise length of 0
    # (2.5 % of the selected lines at NOISE_LENGTH 0.02) recomputes an end point and may move it by an ulp
    print("noise seeds skipped:", NOISE_SEEDS_SKIPPED)


def test_extraction_ignores_the_order_and_direction_of_the_lines(drawings):
    rng = np.random.default_rng(1)
    for seg, views in drawings:
        want_f, want_v = D.extract_sideface(seg, views, *SR.THRESHOLDS)
        perm = rng.permutation(len(seg))
        for s, v in ((seg[perm], views[perm]), (seg[:, [2, 3, 0, 1]], views)):
            got_f, got_v = D.extract_sideface(s, v, *SR.THRESHOLDS)
            assert np.array_equal(got_f.view(np.int64), want_f.view(np.int64)) and np.array_equal(got_v, want_v)


def _candidates(seg, views, view):
    return D.parse_sideface_candidates(D.view_faces(seg, views, view)[0], SR.THRESHOLDS[0])


def test_merged_set_does_not_depend_on_the_candidate_order(drawings):
    """A condition on the fixtures (the reference's merge is sequential, and GEOS's polygon order is not knowable here): for these
    drawings any order of the candidates merges to the same set."""
    rng = np.random.default_rng(2)
    for k, (seg, views) in enumerate(drawings):
        for view in range(3):
            cands = _candidates(seg, views, view)
            if not cands:
                continue
            want = sorted(D.merge_colinear_sidefaces(cands, SR.THRESHOLDS[2]))
            for _ in range(8):
                shuffled = [cands[i] for i in rng.permutation(len(cands))]
                assert sorted(D.merge_colinear_sidefaces(shuffled, SR.THRESHOLDS[2])) == want, (k, view)


def test_literal_and_reduced_merge_predicates_agree(drawings):
    pairs = merged = 0
    for seg, views in drawings:
        for view in range(3):
            cands = _candidates(seg, views, view)
            for q, m in itertools.permutations(cands, 2):
                lit = D.merges_literal(q, m, SR.THRESHOLDS[2])
                assert lit == D.merges_reduced(q, m, SR.THRESHOLDS[2]), (q, m)
                pairs, merged = pairs + 1, merged + lit
            if cands:
                want = D.merge_colinear_sidefaces(cands, SR.THRESHOLDS[2])
                assert D.merge_colinear_sidefaces(cands, SR.THRESHOLDS[2], D.merges_reduced) == want
    assert pairs > 1000 and merged > 20
    for tol in (0.0, -1.0):                                       # nothing merges under a tolerance that is not positive
        q = (0.0, 0.01, 0.5, 0.01, 0.02, 1)
        assert not D.merges_literal(q, q, tol) and not D.merges_reduced(q, q, tol)


# ------------------------------------------------------------------------------------------------ pack, dataset, trainer
@pytest.fixture(scope="module")
def info_set(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("sideface_infos"))
    infos = [SR.render_drawing(np.random.default_rng(s), 3 + s, f"gen{s}") for s in range(4)]
    return root, R.write_infos(root, infos), infos


def test_pack_infos_extracting(info_set):
    from plankassembly_amd.device_data import DeviceDrawings, pack_infos
    root, files, infos = info_set
    with pytest.raises(NotImplementedError, match="side-face extraction"):
        pack_infos(root, files, "sideface")
    cfg = SR.make_data_cfg(300, 80, 0.5, 0.15, 0.02)
    packed = pack_infos(root, files, "sideface", extract=True, data_cfg=cfg)
    assert packed["kind"] == "sideface" and packed["extract"] is True and packed["seg"].dtype == np.float64
    for i, info in enumerate(infos):
        lo, hi = packed["line_off"][i], packed["line_off"][i + 1]
        seg, views = SR.info_segments(info)
        assert np.array_equal(packed["seg"][lo:hi], seg) and np.array_equal(packed["view"][lo:hi], views)
        assert packed["n_faces"][i] == len(D.extract_sideface(seg, views, *SR.THRESHOLDS)[0])
    assert pack_infos(root, files, "sideface", extract="auto")["extract"] is True
    dd = DeviceDrawings(pack_infos(root, files, "sideface", extract=True), TOKEN, cfg, "cpu")   # counts made at construction
    assert np.array_equal(dd.n_prims, packed["n_faces"]) and dd.augments(True) and not dd.augments(False)
    assert dd.thresholds == SR.THRESHOLDS
    with pytest.raises(ValueError, match="extract=True is for kind='sideface'"):
        pack_infos(root, files, "line", extract=True)
    with pytest.raises(ValueError, match="MAX_THICKNESS"):
        DeviceDrawings(pack_infos(root, files, "sideface", extract=True), TOKEN, R.make_data_cfg(300, 80), "cpu")


def test_pack_infos_refuses_what_is_outside_the_domain(tmp_path):
    from plankassembly_amd.device_data import DeviceDrawings, pack_infos
    thin = rect(0.0, 0.0, 0.5, 0.02)
    none = (np.zeros((1, 6)), np.full((1, 6), -1))
    cases = {"diagonal": thin + [[0.0, 0.0, 0.3, 0.3]], "duplicate": thin + [thin[1]]}
    for name, segs in cases.items():
        files = R.write_infos(str(tmp_path), [R.make_info(name, segs, [0] * 5, [0] * 5, *none)])
        with pytest.raises(ValueError, match=rf"{name}\.json: .*axis-aligned"):
            pack_infos(str(tmp_path), files, "sideface", extract=True)
    segs, views = SR.tiled_cells(1, 6, 0.5, 0.02)                  # six stacked rows: six faces
    files = R.write_infos(str(tmp_path), [R.make_info("crowded", segs, views, [0] * len(segs), *none)])
    assert pack_infos(str(tmp_path), files, "sideface", extract=True, data_cfg=SR.make_data_cfg(26, 20))["n_faces"][0] == 6
    with pytest.raises(ValueError, match=r"crowded\.json: 6 side faces .* do not fit MAX_INPUT_LENGTH=25"):
        pack_infos(str(tmp_path), files, "sideface", extract=True, data_cfg=SR.make_data_cfg(25, 20))
    with pytest.raises(ValueError, match=r"crowded\.json: 6 side faces"):
        DeviceDrawings(pack_infos(str(tmp_path), files, "sideface", extract=True), TOKEN, SR.make_data_cfg(25, 20), "cpu")
    bent = R.make_info("bent", thin, [0] * 4, [0] * 4, *none)
    bent["svgs"][0]["coordinates"].append([0.6, 0.1])
    files = R.write_infos(str(tmp_path), [bent])
    with pytest.raises(ValueError, match=r"bent\.json: svg 0 has 3 vertices"):
        pack_infos(str(tmp_path), files, "sideface", extract=True)


def test_dataset_extracts_where_no_faces_are_stored(info_set):
    root, files, infos = info_set
    cfg = SR.make_data_cfg(300, 80)
    ds = D.SidefaceDataset(root, files, TOKEN, cfg)
    assert ds.extract == "auto"
    plain = D.SidefaceDataset(root, files, TOKEN, R.make_data_cfg(300, 80), extract="false")
    for i, info in enumerate(infos):
        faces, fviews = D.extract_sideface(*SR.info_segments(info), *SR.THRESHOLDS)
        assert len(faces) or i == 0
        want = {"name": info["name"], **plain.prepare_input_sequence(faces, fviews),
                **plain.prepare_output_sequence(np.array(info["coords"]).flatten(), np.array(info["attach"]).flatten())}
        got = ds[i]
        assert list(got) == list(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
    with pytest.raises(NotImplementedError, match="EXTRACT_SIDEFACE is false"):
        plain[0]
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=4)))
    assert batch["input_value"].shape == (4, 299) and "input_type" not in batch


def test_dataset_modes_stored_faces_and_augmentation(tmp_path):
    thin = rect(0.0, 0.0, 0.5, 0.02)
    info = R.make_info("stored", thin, [0] * 4, [0] * 4, np.zeros((1, 6)), np.full((1, 6), -1))
    info["faces"], info["faceviews"] = [[-0.5, -0.5, 0.5, -0.48]], [1]                   # NOT what the lines give
    files = R.write_infos(str(tmp_path), [info])
    cfg = SR.make_data_cfg(30, 20, aug_ratio=1.0, noise_ratio=1.0, noise_length=0.0)
    stored = D.quantize_values(np.array([-0.5, -0.5, 0.5, -0.48])).tolist()
    lines = D.quantize_values(np.array([0.0, 0.0, 0.5, 0.02])).tolist()
    for mode, want in (("auto", stored), ("false", stored), ("true", lines), (True, lines), (False, stored), (None, stored)):
        got = D.SidefaceDataset(str(tmp_path), files, TOKEN, cfg, extract=mode)[0]
        assert got["input_value"][:5].tolist() == want + [TOKEN.END], mode
        assert got["input_view"][0] == (0 if want is lines else 1)
    # augmented: NOISE_LENGTH 0 shortens by nothing, so a kept line stays and a deleted one opens the only face -> the fallback
    np.random.seed(0)
    seen = set()
    for _ in range(12):
        got = D.SidefaceDataset(str(tmp_path), files, TOKEN, cfg, augmentation=True, extract="auto")[0]
        seen.add(tuple(got["input_value"][:4].tolist()))
    assert seen <= {tuple(stored), tuple(lines)} and tuple(stored) in seen       # noisy faces come from the lines, the fallback is stored
    with pytest.raises(ValueError, match="EXTRACT_SIDEFACE must be one of"):
        D.SidefaceDataset(str(tmp_path), files, TOKEN, cfg, extract="sometimes")
    cfg["EXTRACT_SIDEFACE"] = "true"
    assert D.SidefaceDataset(str(tmp_path), files, TOKEN, cfg).extract == "true"


def test_extract_mode_values():
    assert [D.extract_mode(v) for v in (None, "auto", "TRUE", "false", True, False)] == ["auto", "auto", "true", "false", "true", "false"]
    for bad in ("yes", 1, 0.5, []):
        with pytest.raises(ValueError, match="EXTRACT_SIDEFACE"):
            D.extract_mode(bad)


def test_trainer_validates_extract_sideface_and_requests_augmentation():
    import os

    import yaml

    from plankassembly_amd.trainer import SidefaceTrainer, extract_option
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "configs", "train_sideface.yaml")) as f:
        hp = yaml.safe_load(f)["model"]["hparams"]
    assert extract_option(hp) == "auto" and SidefaceTrainer.train_augmentation is True
    hp["DATA"]["EXTRACT_SIDEFACE"] = True
    assert extract_option(hp) == "true"
    hp["DATA"]["EXTRACT_SIDEFACE"] = "never"
    with pytest.raises(ValueError, match="DATA.EXTRACT_SIDEFACE must be one of"):
        extract_option(hp)
