"""Rendering the three-view drawing from the planks: an independent raster oracle, the named cases,
generated drawings, and the device kernel's numpy restatement (TEST INFRASTRUCTURE).

* ``render_oracle``   planks with INTEGER coordinates -> lines and types by a plain raster on the integer grid: a nearest-depth
                      map per unit cell (one slice-maximum per box), unit pieces of every box edge hidden iff the cells on both
                      sides are nearer than the edge, nodes at piece end points and proper crossings, runs between nodes.  No
                      compressed coordinates, no intervals: it shares no code and no formulation with ``datasets.render_drawing``
                      (interval algebra on the values) or csrc/render.h (compressed grid, per-segment rule).  Valid for every
                      integer-grid input, so no generated case is ever skipped;
* ``NAMED``           the fixtures of the definition's decisions, at most 4 planks besides plank 0, thousandths;
* ``generated``       the coarse-lattice generator of tests/sideface_reference.py, planks only;
* ``sample``          what ``pa_render_drawings`` computes for one row: host rendering, capacity, counter-based noise keyed by
                      the canonical line number (tests/device_data_reference.py), tokens.
"""
from __future__ import annotations

import numpy as np

import device_data_reference as R
import sideface_reference as SR
from plankassembly_amd import datasets as D

# the oracle's own statement of the views: (first 2D axis, negated second 2D axis, depth axis, sign of nearness)
VIEWS = ((0, 2, 1, -1), (0, 1, 2, 1), (1, 2, 0, 1))
_NONE = np.iinfo(np.int64).min


def thousandths(k):
    return k / 1000.0


def _runs(present, visible, node, along_value, across_value, vertical):
    """Runs of present unit pieces between nodes on every grid line -> [(xmin, ymin, xmax, ymax, type)]."""
    out = []
    for j in np.nonzero(present.any(axis=0))[0]:
        cells = np.nonzero(present[:, j])[0]
        start = prev = int(cells[0])
        for i in list(cells[1:]) + [None]:
            if i is None or i != prev + 1 or node[i, j]:
                vis = visible[start:prev + 1, j]
                assert vis.all() or not vis.any(), "visibility changed between two nodes"
                a, b, c = along_value(start), along_value(prev + 1), across_value(int(j))
                out.append((c, a, c, b, int(not vis.any())) if vertical else (a, c, b, c, int(not vis.any())))
                start = i
            prev = i
    return out


def render_oracle(iboxes, to_float=thousandths, skip_first=True):
    """``iboxes`` integer [P, 6] -> (lines float64 [n, 4], views [n], types [n], flags) in the canonical order.  A coordinate
    k stands for ``to_float(k)``; the negated axis of a view is -to_float(k)."""
    b = np.asarray(iboxes, dtype=np.int64).reshape(-1, 6)[1 if skip_first else 0:]
    good = (b[:, :3] < b[:, 3:]).all(axis=1)
    flags = 0 if good.all() else D.RENDER_DEGENERATE
    b = b[good]
    rows = []
    for view, (ua, va, da, sign) in enumerate(VIEWS):
        if len(b) == 0:
            continue
        u0, u1, v0, v1 = b[:, ua], b[:, ua + 3], -b[:, va + 3], -b[:, va]
        near = np.maximum(sign * b[:, da], sign * b[:, da + 3])
        far = np.minimum(sign * b[:, da], sign * b[:, da + 3])
        ou, ov = int(u0.min()) - 1, int(v0.min()) - 1                          # one empty cell all around
        W, H = int(u1.max()) - ou + 1, int(v1.max()) - ov + 1
        depth = np.full((W, H), _NONE, dtype=np.int64)                         # cell (i, j): [ou + i, ou + i + 1] x [ov + j, ov + j + 1]
        for k in range(len(b)):
            cell = depth[u0[k] - ou:u1[k] - ou, v0[k] - ov:v1[k] - ov]
            np.maximum(cell, near[k], out=cell)
        hp, hv = np.zeros((W, H + 1), bool), np.zeros((W, H + 1), bool)        # horizontal piece (i, j): u in [ou+i, ou+i+1] at v = ov+j
        vp, vv = np.zeros((H, W + 1), bool), np.zeros((H, W + 1), bool)        # vertical piece (j, i): v in [ov+j, ov+j+1] at u = ou+i
        node = np.zeros((W + 1, H + 1), bool)
        for k in range(len(b)):
            i0, i1, j0, j1 = int(u0[k] - ou), int(u1[k] - ou), int(v0[k] - ov), int(v1[k] - ov)
            for d in (near[k], far[k]):
                for j in (j0, j1):
                    hid = (depth[i0:i1, j] > d) & (depth[i0:i1, j - 1] > d)
                    hp[i0:i1, j] = True
                    hv[i0:i1, j] |= ~hid
                    node[i0, j] = node[i1, j] = True
                    node[i0 + 1 + np.nonzero(hid[1:] != hid[:-1])[0], j] = True
                for i in (i0, i1):
                    hid = (depth[i, j0:j1] > d) & (depth[i - 1, j0:j1] > d)
                    vp[j0:j1, i] = True
                    vv[j0:j1, i] |= ~hid
                    node[i, j0] = node[i, j1] = True
                    node[i, j0 + 1 + np.nonzero(hid[1:] != hid[:-1])[0]] = True
        cross = np.zeros_like(node)
        cross[1:-1, 1:-1] = hp[:-1, 1:-1] & hp[1:, 1:-1] & vp[:-1, 1:-1].T & vp[1:, 1:-1].T
        node |= cross

        def fu(i):
            return to_float(ou + i) + 0.0

        def fv(j):
            return -to_float(-(ov + j)) + 0.0

        rows += [(view,) + r for r in _runs(hp, hv, node, fu, fv, False)]
        rows += [(view,) + r for r in _runs(vp, vv, node.T, fv, fu, True)]
    rows.sort()
    return (np.asarray([r[1:5] for r in rows], dtype=np.float64).reshape(-1, 4), np.asarray([r[0] for r in rows], dtype=np.int64),
            np.asarray([r[5] for r in rows], dtype=np.int64), flags)


# ------------------------------------------------------------------------------------------------ the named cases
PLANK0 = (-950, -950, -950, 950, 950, 950)
FRONT = (-500, -600, -500, 500, -400, 500)            # a wide plank near the viewer of view 0 (small y)
LEFT = (-500, -600, -500, 0, -400, 500)               # its left half
RIGHT = (0, -600, -500, 500, -400, 500)               # its right half
SMALL = (-200, 0, -200, 300, 200, 200)                # a small plank, behind FRONT in view 0
NAMED = {
    "single": [(-500, -300, -200, 400, 300, 100)],
    "behind": [FRONT, (-200, 0, -200, 200, 200, 200)],
    "in_front": [(-500, 400, -500, 500, 600, 500), (-200, 0, -200, 200, 200, 200)],
    "partial": [LEFT, SMALL],
    "seam": [LEFT, RIGHT, SMALL],
    "outer_boundary": [LEFT, (-300, 0, -200, 0, 200, 200)],
    "equal_depth": [LEFT, (-200, -600, -200, 300, -500, 200)],
    "far_face_neighbour": [LEFT, (0, -800, -500, 500, -700, 500)],
    "coincident": [FRONT, (-200, 0, -200, 200, 200, 200), (-200, -900, -200, 0, -800, 200)],
    "hidden_crosses_visible": [FRONT, (-200, 0, -200, 200, 200, 200), (-100, -900, -300, 0, -800, 300)],
    "t_junction": [LEFT, (0, -600, -200, 300, -400, 200)],
    "degenerate": [(-500, -300, -200, 400, 300, 100), (100, 100, 100, 100, 300, 300), (200, 200, 200, 100, 300, 300)],
    "only_plank0": [],
}


def named_boxes(name):
    """Integer [P, 6] with plank 0 in front."""
    return np.asarray([PLANK0] + list(NAMED[name]), dtype=np.int64).reshape(-1, 6)


def generated(seed, n_planks):
    """Integer planks [1 + n_planks, 6] of the coarse-lattice generator (planks touch and align often), plank 0 = their bounds."""
    info = SR.render_drawing(np.random.default_rng(seed), n_planks, f"gen{seed}")
    b = np.rint(np.asarray(info["coords"], dtype=np.float64) * 1000.0).astype(np.int64).reshape(-1, 6)
    return np.concatenate([np.concatenate([b[:, :3].min(0), b[:, 3:].max(0)])[None], b])


def generated_set(n=40, seed=100):
    """``n`` generated drawings of 1 .. 20 planks besides plank 0 - 2 .. 21 planks in all, 21 being the planks of T = 128; the plank
    counts cycle so every size occurs."""
    return [generated(seed + i, 1 + (i * 7) % 20) for i in range(n)]


def crossing_bars(n_x=15, n_z=16):
    """Integer planks [1 + n_x + n_z, 6]: n_x bars along x and n_z bars along z, each at a depth of its own, so that in view 0
    every bar of one kind crosses every bar of the other - far more lines (about 2000 in view 0 at 15 + 16 bars) than the render
    kernel's 1024 sort keys hold."""
    bars = [(-900, -900 + 20 * i, -800 + 100 * i, 900, -890 + 20 * i, -770 + 100 * i) for i in range(n_x)]
    bars += [(-800 + 100 * j, 100 + 20 * j, -900, -770 + 100 * j, 110 + 20 * j, 900) for j in range(n_z)]
    return np.asarray([PLANK0] + bars, dtype=np.int64)


def plank_info(name, iboxes):
    """An info dict that stores planks only: ``name``, ``coords``, ``attach``."""
    b = np.asarray(iboxes, dtype=np.int64).reshape(-1, 6)
    return {"name": name, "coords": (b / 1000.0).tolist(), "attach": np.full(b.shape, -1).tolist()}


# ------------------------------------------------------------------------------------------------ the kernel, restated
def sample(coords, attach, drawing, name, data_cfg, token, augmentation=False, seed=0, epoch=0):
    """One row of ``pa_render_drawings`` -> (the sample dict, flags, lines [n, 4], views, types as the row keeps them, in the
    canonical order).  The noise acts on the kept lines as two-point segments (xmin, ymin) -> (xmax, ymax), with the draws
    of tests/device_data_reference.py keyed by the canonical line number."""
    S, n_bits = int(data_cfg.MAX_INPUT_LENGTH) - 1, int(data_cfg.NUM_BITS)
    lines, views, types, flags = D.render_drawing(coords, True, (S - 1) // 4, n_bits)
    box, v, t = lines, views, types
    if augmentation and float(data_cfg.AUG_RATIO) > 0.0:
        seg, keep, dec = R.augment(lines, seed, epoch, drawing, float(data_cfg.AUG_RATIO), float(data_cfg.NOISE_RATIO),
                                   float(data_cfg.NOISE_LENGTH))
        if dec.augmented:
            box, v, t = R.bounds(seg)[keep], views[keep], types[keep]
    out = {"name": name}
    out.update(R.input_rows(box, v, t, S, n_bits, token.END, token.PAD))
    out.update(R.output_rows(coords, attach, int(data_cfg.MAX_OUTPUT_LENGTH), n_bits, token.END, token.PAD, int(data_cfg.VOCAB_SIZE)))
    return out, flags, lines, views, types


def cut_rows(tokens, end, dof=6):
    """``redraw``'s row cutting in numpy: per row the tokens before the first ``end`` -> the number of whole planks."""
    tokens = np.asarray(tokens)
    counts = []
    for row in tokens:
        hit = np.nonzero(row == end)[0]
        counts.append((int(hit[0]) if len(hit) else len(row)) // dof)
    return np.asarray(counts, dtype=np.int64)
