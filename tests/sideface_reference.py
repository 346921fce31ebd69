"""Side-face extraction: generated drawings, an independent oracle, and the device kernel's numpy
restatement (TEST INFRASTRUCTURE).

* ``render_drawing``       random planks projected to three views, their rectangle edges split at every crossing and end point,
                           duplicates and overlaps removed - what the reference's dataset/data_utils.py does to the real renders;
* ``faces_by_flood_fill``  the bounded faces of a view WITHOUT a graph: compressed coordinates, unit walls, flood fill.  Valid where
                           segments meet only at end points - the generator's drawings, with or without noise;
* ``sample``               what csrc/sideface.h computes for one drawing of ``pack_infos(..., extract=True)``: the counter-based
                           noise of tests/device_data_reference.py, ``datasets.extract_sideface_flags``, the fallback, the row's
                           order and capacity, the tokens.
"""
from __future__ import annotations

import numpy as np

import device_data_reference as R
from plankassembly_amd import datasets as D

SCALE, MAX_THICKNESS, MIN_THICKNESS, MERGE_TOLERANCE = 1280, 50, 5, 5         # configs/train_sideface.yaml
THRESHOLDS = (MAX_THICKNESS / SCALE, MIN_THICKNESS / SCALE, MERGE_TOLERANCE / SCALE)


def make_data_cfg(max_input_length, max_output_length, aug_ratio=0.0, noise_ratio=0.0, noise_length=0.0, **extra):
    cfg = R.make_data_cfg(max_input_length, max_output_length, aug_ratio, noise_ratio, noise_length)
    for k, v in dict(SCALE=SCALE, MAX_THICKNESS=MAX_THICKNESS, MIN_THICKNESS=MIN_THICKNESS, MERGE_TOLERANCE=MERGE_TOLERANCE,
                     **extra).items():
        cfg[k] = v
    return cfg


# ------------------------------------------------------------------------------------------------ generated drawings
def _union(intervals):
    out = []
    for lo, hi in sorted(intervals):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return out


def noded_segments(rects):
    """Integer rectangles (x0, y0, x1, y1) -> their edges as integer segments that meet only at end points: collinear overlaps
    united, every segment split where a perpendicular one crosses, touches or ends on it."""
    rows, cols = {}, {}                                            # y -> x intervals, x -> y intervals
    for x0, y0, x1, y1 in rects:
        for y in (y0, y1):
            rows.setdefault(y, []).append((x0, x1))
        for x in (x0, x1):
            cols.setdefault(x, []).append((y0, y1))
    rows = {y: _union(iv) for y, iv in rows.items()}
    cols = {x: _union(iv) for x, iv in cols.items()}
    segs = []
    for y, ivs in rows.items():
        for lo, hi in ivs:
            cuts = sorted({lo, hi} | {x for x, civ in cols.items() if lo < x < hi and any(a <= y <= b for a, b in civ)})
            segs += [(a, y, b, y) for a, b in zip(cuts[:-1], cuts[1:])]
    for x, ivs in cols.items():
        for lo, hi in ivs:
            cuts = sorted({lo, hi} | {y for y, riv in rows.items() if lo < y < hi and any(a <= x <= b for a, b in riv)})
            segs += [(x, a, x, b) for a, b in zip(cuts[:-1], cuts[1:])]
    return segs


def render_drawing(rng, n_planks, name="drawing"):
    """The info dict of dataset/prepare_info.py for ``n_planks`` random axis-aligned planks on the 0.001 grid: one thin axis
    each - mostly between MIN and MAX_THICKNESS / SCALE (0.004 .. 0.039), some below, some thick - three orthographic views."""
    boxes = []
    for _ in range(n_planks):
        kind = rng.random()
        thin = int(rng.integers(5, 39)) if kind < 0.6 else (int(rng.integers(1, 4)) if kind < 0.8 else int(rng.integers(45, 200)))
        size = [int(rng.integers(60, 700)) for _ in range(3)]
        size[int(rng.integers(0, 3))] = thin
        lo = [int(rng.integers(-950, 950 - s)) // 10 * 10 for s in size]         # a coarse lattice: planks touch and align often
        boxes.append(lo + [l + s for l, s in zip(lo, size)])
    segs, views = [], []
    for view, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
        got = noded_segments([(bx[a], bx[b], bx[a + 3], bx[b + 3]) for bx in boxes])
        order = rng.permutation(len(got))
        for k in order:
            s = got[k] if rng.random() < 0.5 else (got[k][2], got[k][3], got[k][0], got[k][1])
            segs.append([v / 1000.0 for v in s])
            views.append(view)
    coords = np.asarray(boxes, dtype=np.float64) / 1000.0
    return R.make_info(name, np.asarray(segs, dtype=np.float64).reshape(-1, 4), views, [0] * len(segs), coords,
                       np.full((n_planks, 6), -1))


def info_segments(info):
    return D.two_point_segments(info["svgs"]), np.asarray(info["views"], dtype=np.int64)


def tiled_cells(nx, ny, dx=0.03, dy=0.03, x0=-0.9, y0=-0.9, view=0):
    """An nx x ny grid of cells as unit segments: nx (ny + 1) + ny (nx + 1) lines, nx ny faces."""
    xs = [round(x0 + i * dx, 3) for i in range(nx + 1)]
    ys = [round(y0 + j * dy, 3) for j in range(ny + 1)]
    segs = [[xs[i], y, xs[i + 1], y] for y in ys for i in range(nx)] + [[x, ys[j], x, ys[j + 1]] for x in xs for j in range(ny)]
    return np.asarray(segs, dtype=np.float64), np.full(len(segs), view, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the oracle
def meet_only_at_end_points(segments):
    """The oracle's condition, checked pair by pair: two axis-aligned segments share nothing, or one point that is an end point
    of both.  (``add_noise`` with a drawn length of 0 moves an end point by an ulp - x0 + 1.0 * (x1 - x0) - and a segment that
    overshoots its neighbour by that ulp crosses it away from the end points: such a drawing is outside the oracle, not outside
    the extraction, whose nodes are end points compared by value.)"""
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 4)
    seg = seg[(seg[:, 0] != seg[:, 2]) | (seg[:, 1] != seg[:, 3])]             # zero-length segments are dropped by both sides
    xlo, xhi = np.minimum(seg[:, 0], seg[:, 2]), np.maximum(seg[:, 0], seg[:, 2])
    ylo, yhi = np.minimum(seg[:, 1], seg[:, 3]), np.maximum(seg[:, 1], seg[:, 3])
    ixlo, ixhi = np.maximum(xlo[:, None], xlo[None]), np.minimum(xhi[:, None], xhi[None])
    iylo, iyhi = np.maximum(ylo[:, None], ylo[None]), np.minimum(yhi[:, None], yhi[None])
    touch = (ixlo <= ixhi) & (iylo <= iyhi) & ~np.eye(len(seg), dtype=bool)
    point = (ixlo == ixhi) & (iylo == iyhi)

    def is_end(x, y, s):
        return ((x == s[..., 0]) & (y == s[..., 1])) | ((x == s[..., 2]) & (y == s[..., 3]))

    ends = is_end(ixlo, iylo, seg[:, None, :]) & is_end(ixlo, iylo, seg[None, :, :])
    return bool(np.all(~touch | (point & ends)))


def faces_by_flood_fill(segments):
    """Bounds [xmin, ymin, xmax, ymax] of the bounded faces of axis-aligned ``segments`` [n, 4] that meet only at end points,
    sorted.  No graph: the cells of the compressed grid are joined across every unit wall no segment covers; a region that
    does not reach the frame around the drawing is a bounded face."""
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 4)
    seg = seg[(seg[:, 0] != seg[:, 2]) | (seg[:, 1] != seg[:, 3])]
    if len(seg) == 0:
        return []
    xs = sorted(set(seg[:, 0]) | set(seg[:, 2]))
    ys = sorted(set(seg[:, 1]) | set(seg[:, 3]))
    xi, yi = {v: k for k, v in enumerate(xs)}, {v: k for k, v in enumerate(ys)}
    nx, ny = len(xs) + 1, len(ys) + 1                               # cell (i, j): between xs[i-1], xs[i] and ys[j-1], ys[j]
    wall_v = np.zeros((len(xs), ny), dtype=bool)                    # wall at xs[i] between cells (i, j) and (i + 1, j)
    wall_h = np.zeros((nx, len(ys)), dtype=bool)                    # wall at ys[j] between cells (i, j) and (i, j + 1)
    for x0, y0, x1, y1 in seg:
        if x0 == x1:
            wall_v[xi[x0], yi[min(y0, y1)] + 1:yi[max(y0, y1)] + 1] = True
        else:
            assert y0 == y1, "axis-aligned segments only"
            wall_h[xi[min(x0, x1)] + 1:xi[max(x0, x1)] + 1, yi[y0]] = True
    region = -np.ones((nx, ny), dtype=np.int64)
    faces = []
    for si in range(nx):
        for sj in range(ny):
            if region[si, sj] != -1:
                continue
            region[si, sj] = len(faces)
            stack, cells, outside = [(si, sj)], [], False
            while stack:
                i, j = stack.pop()
                cells.append((i, j))
                outside |= i in (0, nx - 1) or j in (0, ny - 1)
                for ni, nj, blocked in ((i + 1, j, i < nx - 1 and wall_v[i, j]), (i - 1, j, i > 0 and wall_v[i - 1, j]),
                                        (i, j + 1, j < ny - 1 and wall_h[i, j]), (i, j - 1, j > 0 and wall_h[i, j - 1])):
                    if 0 <= ni < nx and 0 <= nj < ny and not blocked and region[ni, nj] == -1:
                        region[ni, nj] = region[si, sj]
                        stack.append((ni, nj))
            if outside:
                faces.append(None)
            else:
                ci, cj = [c[0] for c in cells], [c[1] for c in cells]
                faces.append((xs[min(ci) - 1], ys[min(cj) - 1], xs[max(ci)], ys[max(cj)]))
    return sorted(f for f in faces if f is not None)


# ------------------------------------------------------------------------------------------------ the kernel, restated
def row_order(box, view, n_bits):
    """The order of the row's tokens: (view, column 0, column 2, column 1, column 3, number) of the quantised boxes."""
    q = R.quantise(np.asarray(box, dtype=np.float64).reshape(-1, 4), n_bits)
    return sorted(range(len(q)), key=lambda i: (int(view[i]), int(q[i, 0]), int(q[i, 2]), int(q[i, 1]), int(q[i, 3]), i))


def sample(packed, i, data_cfg, token, augmentation=False, seed=0, epoch=0):
    """Drawing ``i`` of ``pack_infos(..., "sideface", extract=True)`` -> (the sample dict, flags, faces [n, 4] and faceviews
    [n] in the row's order, after the capacity cut)."""
    lo, hi = int(packed["line_off"][i]), int(packed["line_off"][i + 1])
    plo, phi = int(packed["plank_off"][i]), int(packed["plank_off"][i + 1])
    seg, view = packed["seg"][lo:hi], packed["view"][lo:hi].astype(np.int64)
    thresholds = D.sideface_thresholds(data_cfg)
    flags, faces, fviews = 0, np.zeros((0, 4)), np.zeros(0, dtype=np.int64)
    augmented = False
    if augmentation and float(data_cfg.AUG_RATIO) > 0.0:
        noisy, keep, dec = R.augment(seg, seed, epoch, i, float(data_cfg.AUG_RATIO), float(data_cfg.NOISE_RATIO),
                                     float(data_cfg.NOISE_LENGTH))
        augmented = dec.augmented
        if augmented:
            # (a deleted line keeps its number: the kernel's half-edge numbers are those of the drawing's lines)
            faces, fviews, flags = D.extract_sideface_flags(noisy[keep], view[keep], *thresholds)
            if len(faces) == 0:
                flags |= D.EXTRACT_FELL_BACK
    if len(faces) == 0 and (not augmented or flags & D.EXTRACT_FELL_BACK):
        faces, fviews, f = D.extract_sideface_flags(seg, view, *thresholds)
        flags |= f
    S, n_bits = int(data_cfg.MAX_INPUT_LENGTH) - 1, int(data_cfg.NUM_BITS)
    order = row_order(faces, fviews, n_bits)
    if len(order) > (S - 1) // 4:
        order, flags = order[:(S - 1) // 4], flags | D.EXTRACT_TRUNCATED
    faces, fviews = faces[order], fviews[order]
    out = {"name": packed["names"][i]}
    out.update(R.input_rows(faces, fviews, None, S, n_bits, token.END, token.PAD))
    out.update(R.output_rows(packed["coords"][plo:phi], packed["attach"][plo:phi], int(data_cfg.MAX_OUTPUT_LENGTH), n_bits,
                             token.END, token.PAD, int(data_cfg.VOCAB_SIZE)))
    return out, flags, faces, fviews
