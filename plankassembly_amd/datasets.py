"""Tokenisers of the reference's dataloaders: ``infos/<name>.json`` -> the batch
contract the model consumes.  Drop-in for ``plankassembly/datasets`` (same class names, constructor arguments and
method names), numpy only - shapely / PythonOCC are not needed to READ the prepared info files.

* ``quantize_values`` / ``dequantize_values``            reference plankassembly/datasets/data_utils.py:6-21
* ``LineDataset.prepare_input_sequence``                  reference line_data.py:34-83   (pinned: tests/golden/data_tokens.npz)
* ``LineDataset.prepare_output_sequence``                 reference line_data.py:85-109  (pinned)
* ``LineDataset.__getitem__``                             reference line_data.py:111-142 (info JSON schema: SURVEY appendix B)
* ``SidefaceDataset.prepare_input_sequence``              reference sideface_data.py:137-189 incl. the empty case (pinned)

* ``extract_sideface`` / ``SidefaceDataset.__getitem__``   reference sideface_data.py:22-135, 215-254

The shapely line-noise augmentation (data_utils.py:24-75) is restated here for the straight 2-point segments the info
files hold (``add_noise``; unpinned - there is no shapely to compare with).  Side-face extraction from the line drawing
(sideface_data.py:21-135: polygonize + STRtree merge) is restated for the same domain - two-point, axis-aligned segments
that meet at end points - as a face trace with comparisons only (``extract_sideface``; DESIGN.md section 26 fixes the
semantics, csrc/sideface.h runs them on the device).  It is pinned to an independent flood-fill oracle
(tests/sideface_reference.py), not to GEOS.  ``SidefaceDataset`` extracts when the info file stores no ``faces`` /
``faceviews`` and whenever it augments; stored faces without augmentation are read as before.

* ``render_drawing`` / ``render_info``                     reference dataset/data_utils.py:49-205, prepare_info.py:36-70

The drawing itself (PythonOCC hidden-line removal of a compound of boxes, shapely noding) is restated for what the planks are -
axis-aligned boxes seen along the axes - as interval algebra on the coordinate values (``render_drawing``; section 27 fixes the
semantics, csrc/render.h runs them on the device).  It is pinned to an independent raster oracle (tests/render_reference.py), not
to OpenCASCADE / GEOS.  ``LineDataset`` renders on access where the info file stores no ``lines``, ``SidefaceDataset``
where it stores neither ``faces`` / ``faceviews`` nor ``svgs`` (``DATA.RENDER_DRAWINGS``: auto | true | false; ``stores_input``); a
file that stores what the dataset consumes - boxes without ``svgs``, faces without lines - is read exactly as before.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch


def quantize_values(verts, n_bits=9):
    """[-1, 1] floats -> integers in [0, 2**n_bits - 1] (truncation, as the reference's ``astype('long')``)."""
    rq = 2 ** n_bits - 1
    return ((np.asarray(verts) - (-1)) * rq / 2).astype("long")


def dequantize_values(quantized_verts, n_bits=9):
    rq = 2 ** n_bits - 1
    return (np.asarray(quantized_verts) * 2 / rq + (-1)).astype("float")


def parse_splits_list(splits):
    """reference dataset/data_utils.py:28-46: '.json' entries are info files, '.txt' entries list one per line."""
    if isinstance(splits, str):
        splits = splits.split()
    info_files = []
    for split in splits:
        ext = os.path.splitext(split)[1]
        if ext == ".json":
            info_files.append(split)
        elif ext == ".txt":
            with open(split) as f:
                info_files += [ln.rstrip() for ln in f]
        else:
            raise NotImplementedError("%s not a valid info_file type" % split)
    return info_files


def _segment_points(svg):
    """GeoJSON LineString (string or dict) -> float [n, 2] vertices."""
    g = json.loads(svg) if isinstance(svg, str) else svg
    return np.asarray(g["coordinates"], dtype=float).reshape(-1, 2)


def _interpolate(pts, dist):
    """Point at arc length ``dist`` along the polyline (negative: from the end), clamped - shapely's
    line_interpolate_point."""
    seg = np.linalg.norm(np.diff(pts, axis=0), axis=1)
    total = float(seg.sum())
    if dist < 0:
        dist = total + dist
    dist = min(max(dist, 0.0), total)
    acc = 0.0
    for i, s in enumerate(seg):
        if dist <= acc + s or i == len(seg) - 1:
            t = 0.0 if s == 0 else (dist - acc) / s
            return pts[i] + t * (pts[i + 1] - pts[i])
        acc += s
    return pts[-1]


def add_noise(lines, views, types, noise_ratio, noise_length, rng=np.random):
    """The reference's drawing noise (data_utils.py:24-75) on vertex arrays instead of shapely geometries: a random
    subset of the lines is deleted or shortened from one end by up to ``noise_length``; same sequence of draws from
    numpy's global generator."""
    lines = list(lines)
    num_select = rng.randint(low=1, high=np.ceil(len(lines) * noise_ratio) + 1)
    indices = rng.choice(len(lines), num_select, replace=False)
    for index in indices:
        if rng.random() > 0.5:
            lines[index] = None
            continue
        pts = lines[index]
        length = float(np.linalg.norm(np.diff(pts, axis=0), axis=1).sum())
        noise = np.round(rng.random() * noise_length, 3)
        if length <= noise:
            lines[index] = None
        elif rng.random() > 0.5:
            lines[index] = np.stack([_interpolate(pts, 0.0), _interpolate(pts, -noise)])
        else:
            lines[index] = np.stack([_interpolate(pts, noise), _interpolate(pts, length)])
    keep = [i for i, ln in enumerate(lines) if ln is not None]
    return [lines[i] for i in keep], [views[i] for i in keep], [types[i] for i in keep]


def _bounds(lines):
    """[xmin, ymin, xmax, ymax] per vertex array (shapely.bounds)."""
    return np.array([[p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()] for p in lines], dtype=float).reshape(-1, 4)


# ---------------------------------------------------------------------------------- side faces
EXTRACT_OUT_OF_DOMAIN, EXTRACT_TRUNCATED, EXTRACT_FELL_BACK, EXTRACT_DEGENERATE = 1, 2, 4, 8
_DEGENERATE_AREA2 = 1e-12
_DOMAIN = ("side-face extraction takes straight two-point, axis-aligned segments with finite coordinates in [-1, 1], "
           "no two of one view leaving a common end point in the same direction (DESIGN.md section 26); "
           "for anything else store the extracted boxes in the info file as 'faces' / 'faceviews'")


def _trace_faces(seg, numbers):
    """The bounded faces of ONE view.  ``seg`` float [n, 4] (x0 y0 x1 y1; no zero-length row), ``numbers`` the line number of
    each row (half-edge 2i / 2i + 1 is line i forward / backward).  Returns ([(xmin, ymin, xmax, ymax, smallest half-edge)],
    flags).  Nodes are end points compared by value; a node has at most one half-edge per direction E, N, W, S."""
    n = len(seg)
    origin, direction, node_of, table = [], [], {}, {}
    for i in range(n):
        x0, y0, x1, y1 = (float(v) for v in seg[i])
        if x0 != x1 and y0 != y1:
            return [], EXTRACT_OUT_OF_DOMAIN
        fwd = (0 if x1 > x0 else 2) if y0 == y1 else (1 if y1 > y0 else 3)
        origin += [(x0, y0), (x1, y1)]
        direction += [fwd, (fwd + 2) % 4]
    node = [node_of.setdefault(p, len(node_of)) for p in origin]
    for h in range(2 * n):
        if (node[h], direction[h]) in table:
            return [], EXTRACT_OUT_OF_DOMAIN
        table[node[h], direction[h]] = h
    alive = [True] * n

    def drop(i):
        alive[i] = False
        del table[node[2 * i], direction[2 * i]], table[node[2 * i + 1], direction[2 * i + 1]]

    def degree(v):
        return sum((v, d) in table for d in range(4))

    for _ in range(n):                                             # dangles: at most one round per edge
        dangles = [i for i in range(n) if alive[i] and (degree(node[2 * i]) == 1 or degree(node[2 * i + 1]) == 1)]
        if not dangles:
            break
        for i in dangles:
            drop(i)

    def rings():
        """ring label (its smallest half-edge) per surviving half-edge; next(u -> v): clockwise at v from the direction v -> u"""
        nxt, label = {}, {}
        for h in range(2 * n):
            if alive[h >> 1]:
                v, back = node[h ^ 1], direction[h ^ 1]
                nxt[h] = next(table[v, (back - k) % 4] for k in (1, 2, 3, 4) if (v, (back - k) % 4) in table)
        for h in sorted(nxt):
            g = h
            while g not in label:
                label[g] = h
                g = nxt[g]
        return nxt, label

    nxt, label = rings()
    cuts = [i for i in range(n) if alive[i] and label[2 * i] == label[2 * i + 1]]
    if cuts:                                                       # an edge with the same ring on both sides bounds no face
        for i in cuts:
            drop(i)
        nxt, label = rings()
    faces, flags = [], 0
    for rep in sorted(set(label.values())):
        area2, g = 0.0, rep
        xs, ys = [], []
        while True:
            (xu, yu), (xv, yv) = origin[g], origin[g ^ 1]
            area2 = area2 + (xu * yv - xv * yu)                    # float64 shoelace from the ring's smallest half-edge
            xs.append(xu); ys.append(yu)
            g = nxt[g]
            if g == rep:
                break
        if abs(area2) < _DEGENERATE_AREA2:
            flags |= EXTRACT_DEGENERATE
        elif area2 > 0.0:                                          # the face is on the left: positive = bounded
            faces.append((min(xs), min(ys), max(xs), max(ys), 2 * int(numbers[rep >> 1]) + (rep & 1)))
    return faces, flags


def parse_sideface_candidates(faces, max_thickness):
    """reference parse_sideface_from_polygons (sideface_data.py:22-38) on face bounds: centre lines (x0, y0, x1, y1, width,
    type), horizontal (type 1) before vertical (type 0)."""
    out = []
    for xmin, ymin, xmax, ymax in (tuple(float(v) for v in f) for f in faces):
        h, w = ymax - ymin, xmax - xmin
        if h < max_thickness:
            yc = (ymin + ymax) / 2
            out.append((xmin, yc, xmax, yc, h, 1))
        if w < max_thickness:
            xc = (xmin + xmax) / 2
            out.append((xc, ymin, xc, ymax, w, 0))
    return out


def _segments_intersect(a, b):
    """Closed segments (x0, y0, x1, y1) share a point (shapely ``intersects``): orientation test with the collinear cases."""
    def orient(px, py, qx, qy, rx, ry):
        v = (qx - px) * (ry - py) - (qy - py) * (rx - px)
        return int(v > 0) - int(v < 0)

    def within(px, py, qx, qy, rx, ry):                            # r inside the box of p q
        return min(px, qx) <= rx <= max(px, qx) and min(py, qy) <= ry <= max(py, qy)

    ax0, ay0, ax1, ay1 = a[:4]
    bx0, by0, bx1, by1 = b[:4]
    o1, o2 = orient(ax0, ay0, ax1, ay1, bx0, by0), orient(ax0, ay0, ax1, ay1, bx1, by1)
    o3, o4 = orient(bx0, by0, bx1, by1, ax0, ay0), orient(bx0, by0, bx1, by1, ax1, ay1)
    if o1 != o2 and o3 != o4:
        return True
    return ((o1 == 0 and within(ax0, ay0, ax1, ay1, bx0, by0)) or (o2 == 0 and within(ax0, ay0, ax1, ay1, bx1, by1)) or
            (o3 == 0 and within(bx0, by0, bx1, by1, ax0, ay0)) or (o4 == 0 and within(bx0, by0, bx1, by1, ax1, ay1)))


def merges_literal(q, m, merge_tolerance):
    """The reference's test (sideface_data.py:47-60) on two centre lines (x0, y0, x1, y1, width, type)."""
    xs, ys = (q[0], q[2], m[0], m[2]), (q[1], q[3], m[1], m[3])
    return (_segments_intersect(q, m)
            and (max(xs) - min(xs) < merge_tolerance or max(ys) - min(ys) < merge_tolerance)
            and abs(q[4] - m[4]) < merge_tolerance and q[5] == m[5])


def merges_reduced(q, m, merge_tolerance):
    """The same test as the kernel states it for axis-aligned centre lines: same type, the same centre coordinate exactly,
    ranges that overlap or touch, widths closer than the tolerance (which then is positive)."""
    if q[5] != m[5] or not abs(q[4] - m[4]) < merge_tolerance:
        return False
    if q[5] == 1:
        return q[1] == m[1] and q[0] <= m[2] and m[0] <= q[2]
    return q[0] == m[0] and q[1] <= m[3] and m[1] <= q[3]


def merge_colinear_sidefaces(cands, merge_tolerance, merges=merges_literal):
    """reference merge_colinaer_sidefaces (sideface_data.py:41-76), literally and in that order, on centre lines."""
    merged = [cands[0]]
    for q in cands[1:]:
        hit = [j for j, m in enumerate(merged) if merges(q, m, merge_tolerance)]
        if hit:
            xs = [q[0], q[2]] + [merged[j][k] for j in hit for k in (0, 2)]
            ys = [q[1], q[3]] + [merged[j][k] for j in hit for k in (1, 3)]
            q = (min(xs), min(ys), max(xs), max(ys), q[4], q[5])
            for j in reversed(hit):
                merged.pop(j)
        merged.append(q)
    return merged


def sideface_boxes(merged, min_thickness):
    """The flat-capped buffer of each kept centre line (sideface_data.py:18-19, 78) as its bounds."""
    out = []
    for x0, y0, x1, y1, width, kind in merged:
        if width >= min_thickness:
            half = width / 2
            out.append([x0, y0 - half, x1, y0 + half] if kind == 1 else [x0 - half, y0, x0 + half, y1])
    return out


def view_faces(segments, views, view):
    """Face bounds [n, 4] of one view in the defined candidate order (xmin, ymin, xmax, ymax, smallest half-edge), and flags."""
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 4) + 0.0          # -0.0 -> 0.0: nodes compare by value
    views = np.asarray(views, dtype=np.int64).reshape(-1)
    if len(views) != len(seg):
        raise ValueError(f"{len(views)} views for {len(seg)} segments")
    pick = [i for i in range(len(seg)) if views[i] == view and (seg[i, 0] != seg[i, 2] or seg[i, 1] != seg[i, 3])]
    if pick and not (np.isfinite(seg[pick]).all() and seg[pick].min() >= -1.0 and seg[pick].max() <= 1.0):
        return np.zeros((0, 4)), EXTRACT_OUT_OF_DOMAIN
    faces, flags = _trace_faces(seg[pick], pick)
    return np.asarray([f[:4] for f in sorted(faces)], dtype=np.float64).reshape(-1, 4), flags


def extract_sideface_flags(segments, views, max_thickness, min_thickness, merge_tolerance):
    """``extract_sideface`` that never raises: (faces [n, 4], faceviews [n], flags).  A drawing outside the domain yields no
    face at all and EXTRACT_OUT_OF_DOMAIN, as the kernel reports it."""
    boxes, faceviews, flags = [], [], 0
    for view in range(3):                                          # the reference loops range(3); other views are ignored
        faces, f = view_faces(segments, views, view)
        flags |= f
        cands = parse_sideface_candidates(faces, max_thickness)
        if cands:
            got = sideface_boxes(merge_colinear_sidefaces(cands, merge_tolerance), min_thickness)
            boxes += got
            faceviews += [view] * len(got)
    if flags & EXTRACT_OUT_OF_DOMAIN:
        boxes, faceviews = [], []
    return np.asarray(boxes, dtype=np.float64).reshape(-1, 4), np.asarray(faceviews, dtype=np.int64), flags


def extract_sideface(segments, views, max_thickness, min_thickness, merge_tolerance):
    """reference SidefaceDataset.extract_sideface (sideface_data.py:109-135) for two-point axis-aligned segments
    ``segments`` [n, 4] (x0 y0 x1 y1) with their ``views``: per view 0, 1, 2 the bounded faces of the drawing (dangles
    pruned, faces traced with the face on the left, cut edges removed), thin faces as centre lines, collinear ones merged
    in the defined order, buffered back to boxes.  Returns (faces float64 [n, 4], faceviews int64 [n]).  Raises ValueError
    outside the domain.  DESIGN.md section 26."""
    faces, faceviews, flags = extract_sideface_flags(segments, views, max_thickness, min_thickness, merge_tolerance)
    if flags & EXTRACT_OUT_OF_DOMAIN:
        raise ValueError(_DOMAIN)
    return faces, faceviews


def two_point_segments(svgs, where=""):
    """``svgs`` of an info file -> float [n, 4]; a polyline is refused."""
    seg = np.zeros((len(svgs), 4))
    for i, svg in enumerate(svgs):
        pts = _segment_points(svg)
        if len(pts) != 2:
            raise ValueError(f"{where}svg {i} has {len(pts)} vertices; {_DOMAIN}")
        seg[i] = pts.reshape(4)
    return seg


# ------------------------------------------------------------------- the drawing from the planks
RENDER_OUT_OF_DOMAIN, RENDER_TRUNCATED, RENDER_DEGENERATE = 1, 2, 8
RENDER_OVERFLOW = 16                   # the device only: more lines than the kernel sorts, the kept ones are not the defined ones
RENDER_MODES = ("auto", "true", "false")
# THE view table (reference dataset/data_utils.py:15-25, 104-110; unverified against OpenCASCADE): per view the axis of the 2D
# point's first coordinate, the axis whose NEGATION is its second coordinate, the depth axis, and the sign that turns a depth
# coordinate into nearness (larger = nearer to the viewer).
#   view 0 (f): (x, -z), smaller y nearer;  view 1 (t): (x, -y), larger z nearer;  view 2 (s): (y, -z), larger x nearer
RENDER_VIEWS = ((0, 2, 1, -1.0), (0, 1, 2, 1.0), (1, 2, 0, 1.0))


def render_mode(value):
    """``DATA.RENDER_DRAWINGS``: ``auto`` (default; render only where a file stores nothing the dataset consumes, ``stores_input``), ``true`` (always render from
    ``coords``), ``false`` (stored lines only).  YAML booleans are accepted for true / false."""
    if value is None:
        return "auto"
    if isinstance(value, bool):
        return "true" if value else "false"
    if isinstance(value, str) and value.lower() in RENDER_MODES:
        return value.lower()
    raise ValueError(f"DATA.RENDER_DRAWINGS must be one of {RENDER_MODES}, got {value!r}")


def _merge_closed(intervals):
    """Union of closed intervals; intervals that touch become one."""
    out = []
    for lo, hi in sorted(intervals):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return out


def project_planks(coords, skip_first=True):
    """``coords`` [P, 6] (lo xyz, hi xyz) -> (per view a list of rectangles (u0, v0, u1, v1, near, far) with near / far as
    nearness, flags).  A plank with lo >= hi on an axis is dropped (RENDER_DEGENERATE); any coordinate that is not finite or
    not in [-1, 1] puts the whole drawing out of the domain (RENDER_OUT_OF_DOMAIN, no rectangle)."""
    c = np.asarray(coords, dtype=np.float64).reshape(-1, 6)[1 if skip_first else 0:] + 0.0
    if c.size and not (np.isfinite(c).all() and c.min() >= -1.0 and c.max() <= 1.0):
        return [[], [], []], RENDER_OUT_OF_DOMAIN
    flags, views = 0, [[], [], []]
    for box in c:
        lo, hi = [float(v) for v in box[:3]], [float(v) for v in box[3:]]
        if any(l >= h for l, h in zip(lo, hi)):
            flags |= RENDER_DEGENERATE
            continue
        for view, (ua, va, da, sign) in enumerate(RENDER_VIEWS):
            d0, d1 = sign * lo[da] + 0.0, sign * hi[da] + 0.0
            views[view].append((lo[ua], -hi[va] + 0.0, hi[ua], -lo[va] + 0.0, max(d0, d1), min(d0, d1)))
    return views, flags


def _render_view(rects):
    """The noded arrangement of one view's rectangle edges with the type of every atomic segment: [(xmin, ymin, xmax, ymax,
    type)].  Interval algebra on the coordinate values: collinear edges are united, a line is cut where a perpendicular line
    has a point of it, and a segment is hidden (1) unless an edge covering it is visible there."""
    lines = ({}, {})                                               # [0] horizontal: v -> u intervals; [1] vertical: u -> v intervals
    for u0, v0, u1, v1, _, _ in rects:
        for v in (v0, v1):
            lines[0].setdefault(v, []).append((u0, u1))
        for u in (u0, u1):
            lines[1].setdefault(u, []).append((v0, v1))
    lines = tuple({c: _merge_closed(iv) for c, iv in side.items()} for side in lines)
    hidden_spans = {}

    def hidden(vertical, c, depth):
        """The open spans of the line at ``c`` that lie inside the union of the rectangles nearer than ``depth``: where the
        union covers the strip on both sides of the line."""
        if (vertical, c, depth) not in hidden_spans:
            sides = ([], [])
            for r in rects:
                if r[4] > depth:
                    lo, hi, a0, a1 = (r[1], r[3], r[0], r[2]) if vertical else (r[0], r[2], r[1], r[3])
                    if a0 <= c < a1:
                        sides[0].append((lo, hi))
                    if a0 < c <= a1:
                        sides[1].append((lo, hi))
            one, two = _merge_closed(sides[0]), _merge_closed(sides[1])
            hidden_spans[vertical, c, depth] = [(max(p, r), min(q, s)) for p, q in one for r, s in two if max(p, r) < min(q, s)]
        return hidden_spans[vertical, c, depth]

    out = []
    for vertical in (0, 1):
        for c, spans in lines[vertical].items():
            for lo, hi in spans:
                cuts = sorted({lo, hi} | {x for x, other in lines[1 - vertical].items()
                                          if lo < x < hi and any(a <= c <= b for a, b in other)})
                for a, b in zip(cuts[:-1], cuts[1:]):
                    visible = False
                    for r in rects:
                        rlo, rhi, a0, a1 = (r[1], r[3], r[0], r[2]) if vertical else (r[0], r[2], r[1], r[3])
                        if c in (a0, a1) and rlo <= a and b <= rhi:          # both faces of the box have this edge
                            visible = visible or any(not any(p <= a and b <= q for p, q in hidden(vertical, c, depth))
                                                     for depth in (r[4], r[5]))
                    out.append((c, a, c, b, int(not visible)) if vertical else (a, c, b, c, int(not visible)))
    return sorted(out)


def render_token_order(lines, views, num_bits):
    """The order of the row's tokens over lines in canonical order: (view, column 0, column 2, column 1, column 3, number)."""
    q = quantize_values(np.asarray(lines, dtype=np.float64).reshape(-1, 4), num_bits)
    return sorted(range(len(q)), key=lambda i: (int(views[i]), int(q[i, 0]), int(q[i, 2]), int(q[i, 1]), int(q[i, 3]), i))


def render_drawing(coords, skip_first=True, max_lines=None, num_bits=9):
    """The three-view line drawing of a plank program: ``coords`` [P, 6] -> (lines float64 [n, 4]
    bounds xmin ymin xmax ymax, views int64 [n], types int64 [n] (0 visible, 1 hidden), flags) in the canonical order
    (view, xmin, ymin, xmax, ymax).  Plank 0 (the overall bounding box) is skipped as the reference's ``build`` does.
    ``max_lines``: the row's capacity; a longer drawing keeps the lines that sort first in the order of the row's tokens
    (``num_bits`` quantisation) and gets RENDER_TRUNCATED.  Never raises on the geometry."""
    rects, flags = project_planks(coords, skip_first)
    rows = [(view,) + seg for view in range(3) for seg in _render_view(rects[view])]
    lines = np.asarray([r[1:5] for r in rows], dtype=np.float64).reshape(-1, 4)
    views = np.asarray([r[0] for r in rows], dtype=np.int64)
    types = np.asarray([r[5] for r in rows], dtype=np.int64)
    if max_lines is not None and len(lines) > max_lines:
        keep = sorted(render_token_order(lines, views, num_bits)[:max(int(max_lines), 0)])
        lines, views, types, flags = lines[keep], views[keep], types[keep], flags | RENDER_TRUNCATED
    return lines, views, types, flags


def render_info(name, coords, attach):
    """The info dict of the reference's dataset/prepare_info.py:59-70 with the drawing rendered from ``coords``."""
    lines, views, types, flags = render_drawing(coords)
    if flags & RENDER_OUT_OF_DOMAIN:
        raise ValueError(f"{name}: plank coordinates must be finite and in [-1, 1] (DESIGN.md section 27)")
    return {"name": name, "lines": lines.tolist(), "views": [int(v) for v in views], "types": [int(t) for t in types],
            "svgs": [json.dumps({"type": "LineString", "coordinates": [[ln[0], ln[1]], [ln[2], ln[3]]]}) for ln in lines.tolist()],
            "coords": np.asarray(coords, dtype=np.float64).reshape(-1, 6).tolist(),
            "attach": np.asarray(attach, dtype=np.int64).reshape(-1, 6).tolist()}


def stores_input(info, kind):
    """Whether an info dict stores what the dataset of ``kind`` consumes: ``lines`` for the line kind; ``faces`` / ``faceviews``,
    or the ``svgs`` to extract them from, for the sideface kind.  (``svgs`` alone is not asked of a line file: a file with
    boxes only is read as it is and merely cannot be augmented.)"""
    if kind == "sideface":
        return ("faces" in info and "faceviews" in info) or "svgs" in info
    return "lines" in info


def rendered(info, mode, kind="line", where=""):
    """``info`` with ``lines`` / ``views`` / ``types`` / ``svgs`` rendered from its planks where ``mode`` (``render_mode``)
    says so: ``true`` always (stored ``faces`` are dropped with the stored drawing), ``auto`` only where the file stores
    nothing the dataset of ``kind`` consumes (``stores_input``), ``false`` never.  A file that stores its input is returned
    as it is: nothing is synthesised beside stored data."""
    if mode == "true" or (mode == "auto" and not stores_input(info, kind)):
        kept = {k: v for k, v in info.items() if k not in ("faces", "faceviews")}
        return {**kept, **render_info(where + str(info.get("name", "")), info["coords"], info["attach"]), "name": info["name"]}
    return info


class _TokenisedDataset(torch.utils.data.Dataset):
    render = "false"                                               # the classes that render set it from DATA.RENDER_DRAWINGS
    kind = "line"                                                  # what ``stores_input`` asks of an info file

    def __init__(self, root, info_files, token, cfg, augmentation=False):
        self.root = root
        self.info_files = info_files
        self.augmentation = augmentation
        self.token = token
        self.vocab_size = cfg.VOCAB_SIZE
        self.num_input_dof = cfg.NUM_INPUT_DOF
        self.max_input_length = cfg.MAX_INPUT_LENGTH
        self.max_output_length = cfg.MAX_OUTPUT_LENGTH
        self.num_bits = cfg.NUM_BITS
        self.aug_ratio = cfg.get("AUG_RATIO", 0.0) if hasattr(cfg, "get") else getattr(cfg, "AUG_RATIO", 0.0)
        self.noise_ratio = cfg.get("NOISE_RATIO", 0.0) if hasattr(cfg, "get") else getattr(cfg, "NOISE_RATIO", 0.0)
        self.noise_length = cfg.get("NOISE_LENGTH", 0.0) if hasattr(cfg, "get") else getattr(cfg, "NOISE_LENGTH", 0.0)

    def __len__(self):
        return len(self.info_files)

    def _sorted_tokens(self, boxes, views, extra=None):
        """Shared by lines and side faces: quantise, sort by (view, xmin, xmax, ymin, ymax), position within the view,
        coordinate index, 4 tokens per primitive."""
        value = quantize_values(np.array(boxes), self.num_bits)
        view = np.array(views, dtype="long")
        with_view = np.concatenate((value, view[..., np.newaxis]), axis=1)
        order = np.lexsort(with_view.T[[3, 1, 2, 0, 4]])          # last key is primary: view, then column 0, 2, 1, 3
        value = value[order].flatten()
        view = view[order]
        extra = None if extra is None else np.array(extra)[order]
        _, counts = np.unique(view, return_counts=True)
        pos = np.concatenate([np.arange(c) for c in counts])
        coord = np.arange(len(value)) % self.num_input_dof
        return value, np.repeat(pos, 4), coord, np.repeat(view, 4), None if extra is None else np.repeat(extra, 4)

    def _pad_inputs(self, value, ids):
        """END, then PAD up to MAX_INPUT_LENGTH - 1 value tokens; id rows are zero at END / PAD (line_data.py:58-72:
        the value row gets ``pad_length - 1`` PADs after END, the id rows ``pad_length`` zeros)."""
        value = np.append(value, self.token.END)
        pad_length = self.max_input_length - len(value)
        if pad_length < 1:
            raise ValueError(f"{len(value) - 1} input tokens do not fit MAX_INPUT_LENGTH={self.max_input_length}")
        value = np.pad(value, (0, pad_length - 1), constant_values=self.token.PAD)
        out = {"input_value": value}
        for k, v in ids.items():
            out[k] = np.pad(v, (0, pad_length))
        out["input_mask"] = value == self.token.PAD
        return out

    def prepare_output_sequence(self, planks, attach):
        """reference line_data.py:85-109 / sideface_data.py:191-213."""
        value = quantize_values(planks, self.num_bits)
        value = np.append(value, self.token.END)
        value = np.pad(value, (0, self.max_output_length - len(value)), constant_values=self.token.PAD)
        label = np.pad(np.asarray(attach, dtype="long"), (0, self.max_output_length - len(attach)), constant_values=-1)
        ptr = label != -1
        label[ptr] += self.vocab_size
        label[~ptr] = value[~ptr]
        return {"output_value": value, "output_label": label, "output_mask": value == self.token.PAD}

    def _read_info(self, index):
        with open(os.path.join(self.root, self.info_files[index]), "r") as f:
            info = json.loads(f.read())
        return info if self.render == "false" else rendered(info, self.render, self.kind, f"{self.info_files[index]}: ")


class LineDataset(_TokenisedDataset):
    """reference plankassembly/datasets/line_data.py:12-142.  ``render`` (default: ``DATA.RENDER_DRAWINGS``, else ``auto``):
    see ``render_mode`` - the drawing is rendered from the planks on access where the info file stores no ``lines``."""

    def __init__(self, root, info_files, token, cfg, augmentation=False, render=None):
        super().__init__(root, info_files, token, cfg, augmentation)
        if render is None:
            render = cfg.get("RENDER_DRAWINGS", None) if hasattr(cfg, "get") else getattr(cfg, "RENDER_DRAWINGS", None)
        self.render = render_mode(render)

    def prepare_input_sequence(self, lines, views, types):
        value, pos, coord, view, typ = self._sorted_tokens(lines, views, types)
        return self._pad_inputs(value, {"input_pos": pos, "input_coord": coord, "input_view": view, "input_type": typ})

    def __getitem__(self, index):
        info = self._read_info(index)
        lines = np.array(info["lines"], dtype="float")
        views = np.array(info["views"], dtype="long")
        types = np.array(info["types"], dtype="long")
        planks = np.array(info["coords"]).flatten()
        attach = np.array(info["attach"]).flatten()
        if self.augmentation and np.random.random() < self.aug_ratio:
            segs, views, types = add_noise([_segment_points(s) for s in info["svgs"]], list(views), list(types),
                                           self.noise_ratio, self.noise_length)
            lines = _bounds(segs)
        inputs = self.prepare_input_sequence(lines, views, types)
        outputs = self.prepare_output_sequence(planks, attach)
        return {"name": info["name"], **inputs, **outputs}


def sideface_thresholds(cfg):
    """(max_thickness, min_thickness, merge_tolerance) of a ``DATA`` node: MAX_THICKNESS, MIN_THICKNESS, MERGE_TOLERANCE over
    SCALE (reference sideface_data.py:102-104), as Python floats."""
    get = (lambda k: cfg.get(k, None)) if hasattr(cfg, "get") else (lambda k: getattr(cfg, k, None))
    vals = {k: get(k) for k in ("MAX_THICKNESS", "MIN_THICKNESS", "MERGE_TOLERANCE", "SCALE")}
    missing = [k for k, v in vals.items() if v is None]
    if missing:
        raise ValueError(f"side-face extraction needs DATA.{', DATA.'.join(missing)} (configs/train_sideface.yaml)")
    return tuple(vals[k] / vals["SCALE"] for k in ("MAX_THICKNESS", "MIN_THICKNESS", "MERGE_TOLERANCE"))


EXTRACT_MODES = ("auto", "true", "false")


def extract_mode(value):
    """``DATA.EXTRACT_SIDEFACE``: ``auto`` (default; extract where a file stores no faces), ``true`` (always extract from
    ``svgs`` - what augmentation needs), ``false`` (stored faces only).  YAML booleans are accepted for true / false."""
    if value is None:
        return "auto"
    if isinstance(value, bool):
        return "true" if value else "false"
    if isinstance(value, str) and value.lower() in EXTRACT_MODES:
        return value.lower()
    raise ValueError(f"DATA.EXTRACT_SIDEFACE must be one of {EXTRACT_MODES}, got {value!r}")


class SidefaceDataset(_TokenisedDataset):
    """reference plankassembly/datasets/sideface_data.py:85-254.  ``extract`` (default: ``DATA.EXTRACT_SIDEFACE``, else
    ``auto``): see ``extract_mode``.  The input is extracted from ``svgs`` when the mode says so, and - mode ``auto`` or
    ``true`` - whenever the sample is augmented (the noise acts on the lines, sideface_data.py:233-245)."""
    kind = "sideface"

    def __init__(self, root, info_files, token, cfg, augmentation=False, extract=None, render=None):
        super().__init__(root, info_files, token, cfg, augmentation)
        if extract is None:
            extract = cfg.get("EXTRACT_SIDEFACE", None) if hasattr(cfg, "get") else getattr(cfg, "EXTRACT_SIDEFACE", None)
        self.extract = extract_mode(extract)
        if render is None:
            render = cfg.get("RENDER_DRAWINGS", None) if hasattr(cfg, "get") else getattr(cfg, "RENDER_DRAWINGS", None)
        self.render = render_mode(render)
        self._cfg = cfg

    def extract_sideface(self, segments, views):
        """(faces, faceviews, flags) under the thresholds of the ``DATA`` node; never raises on the geometry."""
        return extract_sideface_flags(segments, views, *sideface_thresholds(self._cfg))

    def prepare_input_sequence(self, faces, views):
        if len(faces) != 0:
            value, pos, coord, view, _ = self._sorted_tokens(faces, views)
        else:                                                      # no side face detected: input = [END, PAD, ...]
            value = quantize_values(np.array(faces), self.num_bits)
            view = np.array(views, dtype="long")
            pos = np.zeros_like(view, dtype="long")
            coord = np.zeros_like(view, dtype="long")
        return self._pad_inputs(value, {"input_pos": pos, "input_coord": coord, "input_view": view})

    def __getitem__(self, index):
        info = self._read_info(index)
        stored = "faces" in info and "faceviews" in info
        if self.extract == "false" and not stored:
            raise NotImplementedError(
                "this info file stores no side faces ('faces' [[xmin, ymin, xmax, ymax]] and 'faceviews' [0|1|2]) and "
                "DATA.EXTRACT_SIDEFACE is false; 'auto' or 'true' extracts them from the line drawing ('svgs')")
        planks = np.array(info["coords"]).flatten()
        attach = np.array(info["attach"]).flatten()
        where = f"{self.info_files[index]}: "
        faces, faceviews = [], []
        if (self.augmentation and self.extract != "false" and len(info.get("svgs") or [])
                and np.random.random() < self.aug_ratio):
            views = list(np.array(info["views"], dtype="long"))
            segs, noisy_views, _ = add_noise([_segment_points(s) for s in info["svgs"]], views, views, self.noise_ratio,
                                             self.noise_length)
            faces, faceviews, _ = self.extract_sideface(np.array(segs, dtype=float).reshape(-1, 4), noisy_views)
        if len(faces) == 0:                                        # not augmented, or the noise left no face
            if stored and self.extract != "true":
                faces, faceviews = np.array(info["faces"], dtype="float").reshape(-1, 4), info["faceviews"]
            else:
                faces, faceviews, flags = self.extract_sideface(two_point_segments(info["svgs"], where), info["views"])
                if flags & EXTRACT_OUT_OF_DOMAIN:
                    raise ValueError(where + _DOMAIN)
        inputs = self.prepare_input_sequence(faces, faceviews)
        outputs = self.prepare_output_sequence(planks, attach)
        return {"name": info["name"], **inputs, **outputs}
