"""Rendering the three-view drawing from the planks, on the host (plankassembly_amd/datasets.py `render_drawing`; DESIGN.md section
27): the interval-algebra renderer equals the raster oracle (tests/render_reference.py) - lines and types exactly - on the named
cases of the definition and on 40 generated drawings; then the decisions of the definition one by one, the flags, the datasets
that render on access, `pack_infos(render=True)`, the option parsing and `redraw`'s row cutting."""
import json
import types

import numpy as np
import pytest
import torch

import device_data_reference as R
import render_reference as RR
import sideface_reference as SR
from plankassembly_amd import datasets as D

TOKEN = types.SimpleNamespace(END=512, PAD=513)


def _equal(got, want):
    return (got[3] == want[3] and np.array_equal(got[0].view(np.int64), want[0].view(np.int64)) and np.array_equal(got[1], want[1])
            and np.array_equal(got[2], want[2]))


def _render(name):
    return D.render_drawing(RR.named_boxes(name) / 1000.0)


def _view(r, view):
    """{(xmin, ymin, xmax, ymax): type} of one view."""
    lines = [tuple(ln) for ln, v in zip(r[0].tolist(), r[1]) if v == view]
    assert len(set(lines)) == len(lines), "a line twice"
    return dict(zip(lines, r[2][r[1] == view].tolist()))


@pytest.fixture(scope="module")
def generated():
    """(integer planks, host rendering, oracle rendering) of the 40 generated drawings: rendered once, shared."""
    return [(b, D.render_drawing(b / 1000.0), RR.render_oracle(b)) for b in RR.generated_set(40)]


@pytest.mark.parametrize("name", sorted(RR.NAMED))
def test_named_case_equals_the_oracle(name):
    assert len(RR.NAMED[name]) <= 4
    assert _equal(_render(name), RR.render_oracle(RR.named_boxes(name)))


def test_generated_drawings_equal_the_oracle_and_some_line_is_hidden(generated):
    assert len(generated) == 40 and {len(b) - 1 for b, _, _ in generated} >= {1, 20}
    for b, host, oracle in generated:
        assert _equal(host, oracle), len(b)
    assert sum(int(h[2].sum()) for _, h, _ in generated) > 0, "no generated drawing has a hidden line: the type path is vacuous"
    assert all(h[3] == 0 for _, h, _ in generated)


def test_lines_without_types_are_the_noded_rectangles(generated):
    for b, host, _ in generated[::4]:
        for view, (ua, va, _, _) in enumerate(RR.VIEWS):
            rects = [(int(x[ua]), int(-x[va + 3]), int(x[ua + 3]), int(-x[va])) for x in b[1:]]
            want = sorted((min(s[0], s[2]) / 1000 + 0.0, min(s[1], s[3]) / 1000 + 0.0, max(s[0], s[2]) / 1000 + 0.0,
                           max(s[1], s[3]) / 1000 + 0.0) for s in SR.noded_segments(rects))
            assert sorted(_view(host, view)) == want


def test_order_of_the_planks_does_not_matter(generated):
    rng = np.random.default_rng(3)
    for b, host, _ in generated[::5]:
        shuffled = np.concatenate([b[:1], b[1:][rng.permutation(len(b) - 1)]])
        assert _equal(D.render_drawing(shuffled / 1000.0), host)


def test_tokens_dequantised_equal_the_oracle():
    """Any doubles, not only thousandths: token planks through ``dequantize_values``."""
    rng = np.random.default_rng(11)
    for _ in range(6):
        lo = rng.integers(0, 400, size=(6, 3)) // 8 * 8
        q = np.concatenate([lo, lo + rng.integers(1, 110, size=(6, 3)) // 4 * 4 + 1], axis=1)
        host = D.render_drawing(D.dequantize_values(q))
        assert _equal(host, RR.render_oracle(q, lambda k: float(D.dequantize_values(k))))


def test_single_box_has_four_visible_lines_per_view():
    lines, views, types, flags = _render("single")
    assert flags == 0 and len(lines) == 12 and not types.any() and np.bincount(views).tolist() == [4, 4, 4]
    assert len({(v,) + tuple(ln) for v, ln in zip(views, lines.tolist())}) == 12
    assert ((lines[:, 0] != lines[:, 2]) | (lines[:, 1] != lines[:, 3])).all(), "a point"
    assert sorted(_view((lines, views, types, flags), 0)) == [(-0.5, -0.1, -0.5, 0.2), (-0.5, -0.1, 0.4, -0.1), (-0.5, 0.2, 0.4, 0.2),
                                                              (0.4, -0.1, 0.4, 0.2)]


def test_a_box_behind_another_is_hidden_and_in_front_of_it_visible():
    small = [(-0.2, -0.2, -0.2, 0.2), (-0.2, -0.2, 0.2, -0.2), (-0.2, 0.2, 0.2, 0.2), (0.2, -0.2, 0.2, 0.2)]
    behind, in_front = _view(_render("behind"), 0), _view(_render("in_front"), 0)
    assert [behind[s] for s in small] == [1, 1, 1, 1] and sum(behind.values()) == 4
    assert [in_front[s] for s in small] == [0, 0, 0, 0] and sum(in_front.values()) == 0
    # the opposite sense: seen from the side (view 2) and from above (view 1) the two do not overlap, nothing is hidden
    assert not any(_view(_render("behind"), 1).values()) and not any(_view(_render("behind"), 2).values())


def test_partial_occlusion_splits_the_edge_at_the_occluders_boundary():
    v = _view(_render("partial"), 0)
    for y in (-0.2, 0.2):
        assert v[(-0.2, y, 0.0, y)] == 1 and v[(0.0, y, 0.3, y)] == 0        # hidden up to the occluder's right edge x = 0
    assert v[(-0.2, -0.2, -0.2, 0.2)] == 1 and v[(0.3, -0.2, 0.3, 0.2)] == 0
    assert [v[s] for s in ((0.0, -0.5, 0.0, -0.2), (0.0, -0.2, 0.0, 0.2), (0.0, 0.2, 0.0, 0.5))] == [0, 0, 0]   # noded there


def test_seam_outer_boundary_and_equal_depth():
    seam = _view(_render("seam"), 0)
    for y in (-0.2, 0.2):                                          # behind the seam x = 0 of two abutting planks: hidden, cut at the seam
        assert seam[(-0.2, y, 0.0, y)] == 1 and seam[(0.0, y, 0.3, y)] == 1
    assert seam[(-0.2, -0.2, -0.2, 0.2)] == 1 and seam[(0.3, -0.2, 0.3, 0.2)] == 1
    outer = _view(_render("outer_boundary"), 0)
    assert outer[(0.0, -0.2, 0.0, 0.2)] == 0                       # behind the occluder's outer boundary: visible
    assert outer[(-0.3, -0.2, -0.3, 0.2)] == 1 and outer[(-0.3, 0.2, 0.0, 0.2)] == 1
    equal = _view(_render("equal_depth"), 0)
    assert not any(equal.values())                                 # in the occluder's near-face plane: visible


def test_far_face_edge_behind_a_neighbour():
    """The far-face edge at x = 0 of the left plank is hidden as an edge (its own box on one side, the nearer neighbour on the
    other); the near-face edge over it is visible, and visible wins."""
    rects, _ = D.project_planks(RR.named_boxes("far_face_neighbour") / 1000.0)
    left = rects[0][0]
    assert (left[2], left[4], left[5]) == (0.0, 0.6, 0.4)
    v = _view(_render("far_face_neighbour"), 0)
    assert v[(0.0, -0.5, 0.0, 0.5)] == 0 and not any(v.values())


def test_coincident_edges_give_one_visible_line():
    v = _view(_render("coincident"), 0)
    assert v[(-0.2, -0.2, -0.2, 0.2)] == 0                         # the hidden box's left edge under the front box's: once, visible
    assert v[(0.2, -0.2, 0.2, 0.2)] == 1


def test_a_hidden_line_crossing_a_visible_one_splits_both():
    v = _view(_render("hidden_crosses_visible"), 0)
    for y in (-0.2, 0.2):
        assert [v[(a, y, b, y)] for a, b in ((-0.2, -0.1), (-0.1, 0.0), (0.0, 0.2))] == [1, 1, 1]
    for x in (-0.1, 0.0):
        assert [v[(x, a, x, b)] for a, b in ((-0.3, -0.2), (-0.2, 0.2), (0.2, 0.3))] == [0, 0, 0]


def test_t_junction_cuts_the_line_it_ends_on():
    v = _view(_render("t_junction"), 0)
    assert [(0.0, a, 0.0, b) in v for a, b in ((-0.5, -0.2), (-0.2, 0.2), (0.2, 0.5))] == [True] * 3
    assert (0.0, -0.5, 0.0, 0.5) not in v and not any(v.values())


def test_flags_and_the_empty_drawing():
    r = _render("degenerate")
    assert r[3] == D.RENDER_DEGENERATE and _equal(r, (*_render("single")[:3], D.RENDER_DEGENERATE))
    for bad in (np.nan, 1.5, -np.inf):
        c = RR.named_boxes("behind") / 1000.0
        c[2, 4] = bad
        lines, views, types, flags = D.render_drawing(c)
        assert flags == D.RENDER_OUT_OF_DOMAIN and lines.shape == (0, 4) and len(views) == len(types) == 0
    lines, views, types, flags = _render("only_plank0")
    assert flags == 0 and len(lines) == 0
    row = R.input_rows(lines, views, types, 29, 9, TOKEN.END, TOKEN.PAD)       # the row the device writes: [END, PAD, ...]
    assert row["input_value"][0] == TOKEN.END and (row["input_value"][1:] == TOKEN.PAD).all() and not row["input_mask"][0]


def test_negative_zero_does_not_come_out():
    c = np.asarray([RR.PLANK0, (-500, -300, -200, 0, 300, 0)], dtype=np.float64) / 1000.0
    c[1, 3], c[1, 5] = -0.0, -0.0
    lines = D.render_drawing(c)[0]
    assert (lines == 0).any() and not np.signbit(lines[lines == 0]).any()
    assert _equal(D.render_drawing(c), D.render_drawing(c + 0.0))


def test_capacity_keeps_the_first_lines_in_token_order(tmp_path):
    from plankassembly_amd.device_data import pack_infos
    b = RR.named_boxes("partial")
    full = D.render_drawing(b / 1000.0)
    n = len(full[0])
    cut = D.render_drawing(b / 1000.0, max_lines=n - 1)
    assert cut[3] == D.RENDER_TRUNCATED and len(cut[0]) == n - 1 and D.render_drawing(b / 1000.0, max_lines=n)[3] == 0
    keep = sorted(D.render_token_order(full[0], full[1], 9)[:n - 1])
    assert np.array_equal(cut[0], full[0][keep]) and np.array_equal(cut[2], full[2][keep])
    files = R.write_infos(str(tmp_path), [RR.plank_info("over", b)])
    with pytest.raises(ValueError, match=r"over\.json.*%d lines" % n):
        pack_infos(str(tmp_path), files, "line", render=True, data_cfg=R.make_data_cfg(4 * (n - 1) + 2, 40))
    packed = pack_infos(str(tmp_path), files, "line", render=True, data_cfg=R.make_data_cfg(4 * n + 2, 40))
    assert packed["render"] and packed["n_lines"].tolist() == [n] and "seg" not in packed


def test_pack_infos_names_the_file_outside_the_domain(tmp_path):
    from plankassembly_amd.device_data import RENDER_MAX_PLANKS, pack_infos
    cfg = R.make_data_cfg(1200, 400)
    bad = RR.plank_info("bad", RR.named_boxes("single"))
    bad["coords"][1][0] = -1.5
    many = RR.plank_info("many", np.concatenate([RR.generated(5, 20), RR.generated(6, 12)]))
    assert len(many["coords"]) == RENDER_MAX_PLANKS + 2
    for info, pattern in ((bad, r"bad\.json"), (many, r"many\.json.*34 planks")):
        files = R.write_infos(str(tmp_path), [info])
        with pytest.raises(ValueError, match=pattern):
            pack_infos(str(tmp_path), files, "line", render=True, data_cfg=cfg)
    stored = R.write_infos(str(tmp_path), [D.render_info("stored", np.asarray(RR.plank_info("s", RR.named_boxes("seam"))["coords"]),
                                                         np.full((4, 6), -1))])
    assert "render" not in pack_infos(str(tmp_path), stored, "line", render="auto")
    with pytest.raises(ValueError, match="kind='line'"):
        pack_infos(str(tmp_path), stored, "sideface", render=True)


def test_render_info_round_trips_through_the_line_dataset(tmp_path, generated):
    cfg = R.make_data_cfg(4 * 500 + 2, 128)
    b, host, _ = generated[5]
    coords, attach = b / 1000.0, np.full(b.shape, -1)
    info = D.render_info("full", coords, attach)
    assert sorted(info) == ["attach", "coords", "lines", "name", "svgs", "types", "views"]
    assert all(isinstance(s, str) and len(json.loads(s)["coordinates"]) == 2 for s in info["svgs"])
    files = R.write_infos(str(tmp_path), [info, RR.plank_info("planks_only", b)])
    direct = D.LineDataset("", [], TOKEN, cfg).prepare_input_sequence(*host[:3])
    ds = D.LineDataset(str(tmp_path), files, TOKEN, cfg)
    assert ds.render == "auto"
    for i in range(2):                                             # stored lines, and rendered on access
        item = ds[i]
        for k, w in direct.items():
            assert np.array_equal(item[k], w), (i, k)
    assert int(direct["input_type"].sum()) > 0
    with pytest.raises(KeyError):
        D.LineDataset(str(tmp_path), files, TOKEN, cfg, render="false")[1]
    always = D.LineDataset(str(tmp_path), files, TOKEN, cfg, render=True)[0]
    assert all(np.array_equal(always[k], w) for k, w in direct.items())
    side = D.SidefaceDataset(str(tmp_path), files, TOKEN, SR.make_data_cfg(4 * 500 + 2, 128))
    a, b2 = side[0], side[1]                                       # side faces extracted from stored and from rendered lines
    assert all(np.array_equal(a[k], b2[k]) for k in a if k != "name")


def test_render_drawings_option_parsing():
    from plankassembly_amd.trainer import render_option
    assert [D.render_mode(v) for v in (None, True, False, "auto", "TRUE", "false")] == ["auto", "true", "false", "auto", "true", "false"]
    for bad in ("yes", 1, 0.5, []):
        with pytest.raises(ValueError, match="RENDER_DRAWINGS"):
            D.render_mode(bad)
    assert render_option({}) == "auto" and render_option({"DATA": {"RENDER_DRAWINGS": False}}) == "false"
    with pytest.raises(ValueError, match="RENDER_DRAWINGS"):
        render_option({"DATA": {"RENDER_DRAWINGS": "sometimes"}})
    cfg = R.make_data_cfg(30, 20)
    cfg["RENDER_DRAWINGS"] = True
    assert D.LineDataset("", [], TOKEN, cfg).render == "true"


def test_redraw_cuts_rows_like_the_numpy_restatement():
    from plankassembly_amd.decode import redraw_planks
    rng = np.random.default_rng(5)
    tokens = rng.integers(0, 512, size=(9, 37))
    for row, end in enumerate((0, 1, 5, 6, 7, 12, 35, 36)):
        tokens[row, end] = TOKEN.END
        tokens[row, end + 1:] = TOKEN.PAD
    tokens[2, 20] = TOKEN.END                                      # a second END behind the first changes nothing
    coords, n = redraw_planks(torch.from_numpy(tokens), TOKEN.END, 9)
    assert n.tolist() == RR.cut_rows(tokens, TOKEN.END).tolist() == [0, 0, 0, 1, 1, 2, 5, 6, 6]
    assert coords.shape == (9, 6, 6) and coords.dtype == torch.float64
    want = D.dequantize_values(tokens[:, :36]).reshape(9, 6, 6)
    assert np.array_equal(coords.numpy().view(np.int64), want.view(np.int64))
    empty, n0 = redraw_planks(torch.zeros(2, 0, dtype=torch.int64), TOKEN.END, 9)
    assert empty.shape == (2, 0, 6) and n0.tolist() == [0, 0]


def _same_item(a, b):
    assert list(a) == list(b)
    for k in a:
        assert (a[k] == b[k]) if k == "name" else np.array_equal(a[k], b[k]), k


def test_auto_leaves_files_that_store_their_input_as_they_are(tmp_path):
    """``RENDER_DRAWINGS: auto`` (the default) renders only where the data the dataset consumes is absent.  A line file with
    boxes but no ``svgs`` and a sideface file with faces but no lines give the tokens they gave before - their stored drawing is
    NOT the rendering of their planks here, so a silent re-rendering would show - and nothing is synthesised beside them."""
    from plankassembly_amd.device_data import pack_infos
    rng = np.random.default_rng(2)
    coords = RR.named_boxes("partial") / 1000.0
    other = R.random_info(rng, "other", (9, 9), (3, 3))                        # some drawing that is not these planks' rendering
    boxes_only = {k: other[k] for k in ("lines", "views", "types")}
    boxes_only.update(name="boxes_only", coords=coords.tolist(), attach=np.full(coords.shape, -1).tolist())
    faces_only = {"name": "faces_only", "faces": other["lines"][:5], "faceviews": other["views"][:5],
                  "coords": coords.tolist(), "attach": np.full(coords.shape, -1).tolist()}
    planks_only = RR.plank_info("planks_only", RR.named_boxes("partial"))
    files = R.write_infos(str(tmp_path), [boxes_only, faces_only, planks_only])
    assert D.stores_input(boxes_only, "line") and D.stores_input(faces_only, "sideface") and not D.stores_input(faces_only, "line")
    assert not D.stores_input(planks_only, "line") and not D.stores_input(planks_only, "sideface")
    assert D.rendered(boxes_only, "auto", "line") is boxes_only and D.rendered(faces_only, "auto", "sideface") is faces_only
    cfg, scfg = R.make_data_cfg(4 * 60 + 2, 40), SR.make_data_cfg(4 * 60 + 2, 40, aug_ratio=1.0, noise_ratio=0.5, noise_length=0.3)
    # the line kind: stored boxes, whatever the mode short of "true"
    before = D.LineDataset(str(tmp_path), files, TOKEN, cfg, render="false")[0]
    _same_item(D.LineDataset(str(tmp_path), files, TOKEN, cfg)[0], before)
    want = D.LineDataset("", [], TOKEN, cfg).prepare_input_sequence(np.array(other["lines"]), other["views"], other["types"])
    assert all(np.array_equal(before[k], w) for k, w in want.items())
    assert not np.array_equal(D.LineDataset(str(tmp_path), files, TOKEN, cfg, render="true")[0]["input_value"], before["input_value"])
    # the sideface kind: stored faces, also under augmentation (no ``svgs`` appear, so the noise has nothing to act on and no
    # draw is taken from the generator)
    for aug in (False, True):
        np.random.seed(3)
        was = D.SidefaceDataset(str(tmp_path), files, TOKEN, scfg, aug, render="false")[1]
        state = np.random.get_state()[1].copy()
        np.random.seed(3)
        _same_item(D.SidefaceDataset(str(tmp_path), files, TOKEN, scfg, aug)[1], was)
        assert np.array_equal(np.random.get_state()[1], state)
    # the device dataset's packing: the same arrays as without the option, file by file in one pass
    plain, auto = pack_infos(str(tmp_path), files[:1], "line"), pack_infos(str(tmp_path), files[:1], "line", render="auto", data_cfg=cfg)
    assert list(plain) == list(auto) and "render" not in auto and auto["seg"] is None
    assert all(np.array_equal(plain[k], auto[k]) for k in ("line_off", "box", "view", "type", "plank_off", "coords", "attach"))
    splain = pack_infos(str(tmp_path), files[1:2], "sideface")
    sauto = pack_infos(str(tmp_path), files[1:2], "sideface", render="auto")
    assert list(splain) == list(sauto) and all(np.array_equal(splain[k], sauto[k]) for k in ("line_off", "box", "view"))
    with pytest.raises(ValueError, match=r"planks_only\.json.*DEVICE_DATASET: false"):
        pack_infos(str(tmp_path), files[2:], "sideface", render="auto", extract=True)
    # a mixed line set: the stored file as stored, the plank-only file rendered on the host beside it
    mixed = pack_infos(str(tmp_path), [files[0], files[2]], "line", render="auto", data_cfg=cfg)
    lines, views, types, _ = D.render_drawing(coords)
    assert "render" not in mixed and mixed["seg"] is None and mixed["line_off"].tolist() == [0, 9, 9 + len(lines)]
    assert np.array_equal(mixed["box"][:9], plain["box"]) and np.array_equal(mixed["box"][9:], lines)
    assert np.array_equal(mixed["type"][9:], types) and np.array_equal(mixed["view"][9:], views)
    only = pack_infos(str(tmp_path), files[2:], "line", render="auto", data_cfg=cfg)
    assert only["render"] and only["n_lines"].tolist() == [len(lines)] and "box" not in only
