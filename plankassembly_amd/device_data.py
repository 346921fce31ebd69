"""Device-resident dataset: the prepared drawings live in HBM and every batch is tokenised,
augmented and padded there by ONE launch of ``pa_tokenise_drawings`` (csrc/tokenise.hip) - the batch contract of
``data.py`` / ``datasets.py`` (reference line_data.py:34-142, sideface_data.py:137-213) without a CPU tokeniser, a
DataLoader worker or a host -> device copy per step.  Opt-in: hparams key ``DEVICE_DATASET`` (trainer.py).

* ``pack_infos``      info JSONs -> plain numpy arrays in CSR form (read once, on the host);
* ``DeviceDrawings``  those arrays in HBM; ``batch(index, epoch, augmentation)`` is the one launch;
* ``DeviceLoader``    the iteration order of torch's own samplers, uploaded once per epoch.

What differs from the CPU classes, all of it in the augmentation (``LineDataset`` with ``augmentation=True``):
  - the draws are counter-based (``mix32`` of seed, epoch, drawing, line, slot - tests/device_data_reference.py restates
    them), not numpy's global generator: the same drawing in the same epoch gets the same noise whatever the batch size,
    the position in the batch or the number of ranks, and no two runs of the CPU class can be compared draw for draw;
  - straight two-point segments only (all the info files hold, ``datasets.py`` docstring): ``pack_infos`` refuses a
    polyline and points to ``LineDataset``;
  - side faces: with ``pack_infos(..., "sideface", extract=True)`` the LINES are packed and
    ``pa_tokenise_sideface_drawings`` (csrc/sideface.h) extracts the side faces of every batch row on the device - faces
    of each view, centre lines, merge, boxes - then tokenises them; such a set can be augmented (the noise acts on the
    lines) and returns ``_extract_flags``; stored ``faces`` (the default) are tokenised as they are and never augmented;
  - rendered drawings: with ``pack_infos(..., "line", render=True)`` only the PLANKS are packed and
    ``pa_render_drawings`` (csrc/render.h) draws the three views of every batch row on the device - hidden-line rendering,
    then the same noise (draws keyed by the canonical line number) and tokens; such a batch returns ``_render_flags``.  A
    drawing of plank 0 alone tokenises as the empty case ``[END, PAD, ...]``, where ``LineDataset`` raises;
  - a drawing whose every line the noise deleted tokenises as the empty case ``[END, PAD, ...]`` - ``LineDataset`` (and
    the reference) raise there, a kernel cannot; ``num_select`` is capped at the number of lines (``NOISE_RATIO`` > 1
    raises in numpy's ``choice``), and ``NOISE_RATIO`` 0 leaves a drawing as it is (numpy's ``randint(1, 1)`` raises).
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch
import torch.distributed as dist

from . import _lib as L
from .datasets import (EXTRACT_OUT_OF_DOMAIN, RENDER_OUT_OF_DOMAIN, RENDER_TRUNCATED, _DOMAIN, _segment_points,
                       extract_sideface_flags, render_drawing, rendered, sideface_thresholds, stores_input, two_point_segments,
                       view_faces)

MAX_LINES = 1024                      # include/plank_hip.h PA_TOKENISE_MAX_LINES: the kernel's LDS key array
RENDER_MAX_PLANKS = 32                # include/plank_hip.h PA_RENDER_MAX_PLANKS: the render kernel's box arrays
_SIDEFACE_RENDER = ("rendering on the device (render=True / DATA.RENDER_DRAWINGS) is for kind='line': a sideface file that stores neither "
                    "'faces' / 'faceviews' nor 'svgs' is rendered and extracted on the host (datasets.SidefaceDataset) - DEVICE_DATASET: false")
_SIDEFACE_MISSING = (
    "this info file stores no side faces ('faces' [[xmin, ymin, xmax, ymax]] and 'faceviews' [0|1|2]); side-face extraction "
    "from the line drawing (reference sideface_data.py:21-135) is pack_infos(..., 'sideface', extract=True) / "
    "DATA.EXTRACT_SIDEFACE auto or true")


def _in_unit_range(a):
    return a.size == 0 or (np.isfinite(a).all() and a.min() >= -1.0 and a.max() <= 1.0)


def sideface_count(seg, view, data_cfg, where=""):
    """The number of side faces ``extract_sideface`` finds in one drawing's clean lines, checked against the row: what
    the host knows of an extracting set without augmentation.  Raises ValueError naming ``where`` beyond (S - 1) / 4."""
    faces, _, flags = extract_sideface_flags(seg, view, *sideface_thresholds(data_cfg))
    if flags & EXTRACT_OUT_OF_DOMAIN:
        raise ValueError(f"{where}{_DOMAIN}")
    room = (int(data_cfg.MAX_INPUT_LENGTH) - 2) // 4
    if len(faces) > room:
        raise ValueError(f"{where}{len(faces)} side faces ({4 * len(faces)} input tokens) do not fit "
                         f"MAX_INPUT_LENGTH={int(data_cfg.MAX_INPUT_LENGTH)} ({room} faces)")
    return len(faces)


def _check_rendered(where, n_planks, n_lines, data_cfg):
    """A drawing the device is to render, against the render kernel's plank cap and - with ``data_cfg`` - the row."""
    if n_planks > RENDER_MAX_PLANKS:
        raise ValueError(f"{where}{n_planks} planks, the render kernel draws at most {RENDER_MAX_PLANKS} (PA_RENDER_MAX_PLANKS)")
    if data_cfg is not None:
        room = (int(data_cfg.MAX_INPUT_LENGTH) - 2) // 4
        if n_lines > room:
            raise ValueError(f"{where}the rendered drawing has {n_lines} lines ({4 * n_lines} input tokens), which do not fit "
                             f"MAX_INPUT_LENGTH={int(data_cfg.MAX_INPUT_LENGTH)} ({room} lines)")


def render_count(coords, data_cfg, where=""):
    """The number of lines ``render_drawing`` draws for one drawing's planks, checked against the render kernel's domain and
    the row: what the host knows of a rendering set without augmentation.  Raises ValueError naming ``where``."""
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, 6)
    if len(coords) > RENDER_MAX_PLANKS:
        raise ValueError(f"{where}{len(coords)} planks, the render kernel draws at most {RENDER_MAX_PLANKS} (PA_RENDER_MAX_PLANKS)")
    room = (int(data_cfg.MAX_INPUT_LENGTH) - 2) // 4
    lines, _, _, flags = render_drawing(coords, True, room, int(data_cfg.NUM_BITS))
    if flags & RENDER_OUT_OF_DOMAIN:
        raise ValueError(f"{where}plank coordinates must be finite and in [-1, 1] to be rendered (DESIGN.md section 27)")
    if flags & RENDER_TRUNCATED:
        n = len(render_drawing(coords)[0])
        raise ValueError(f"{where}the rendered drawing has {n} lines ({4 * n} input tokens), which do not fit "
                         f"MAX_INPUT_LENGTH={int(data_cfg.MAX_INPUT_LENGTH)} ({room} lines)")
    return len(lines)


def pack_infos(root, info_files, kind="line", extract=False, data_cfg=None, render=False):
    """Read every info JSON once -> dict of numpy arrays, CSR over the drawings: ``line_off`` int32 [N+1], ``box`` f64
    [L,4] (``lines`` / ``faces`` as stored), ``seg`` f64 [L,4] (x0 y0 x1 y1 of ``svgs``; lines only, None when the files
    carry no svgs), ``view`` u8 [L], ``type`` u8 [L] (lines only), ``plank_off`` int32 [N+1], ``coords`` f64 [P,6],
    ``attach`` int32 [P,6], ``names`` and ``files`` (lists), ``kind``.

    ``kind="sideface"`` with ``extract=True``: ``seg`` / ``view`` / ``line_off`` hold the LINES of
    ``svgs`` (``box`` their bounds) and the side faces are extracted on the device, batch by batch; every drawing is
    checked against the extraction's domain here, by file name.  With ``data_cfg`` (the ``DATA`` node) the extraction
    also runs once per drawing on the host: ``n_faces`` int64 [N], checked against the row; without it
    ``DeviceDrawings`` does that.  ``extract="auto"``: True unless every file stores ``faces`` / ``faceviews``.

    ``kind="line"`` with ``render=True``: only the PLANKS are packed (``name``, ``coords``, ``attach`` are
    all a file needs) and ``pa_render_drawings`` (csrc/render.h) draws the three views of every batch row on the device.  Every
    drawing is rendered once on the host here when ``data_cfg`` is given (else by ``DeviceDrawings``): its domain and its line
    count against the row, by file name -> ``n_lines`` int64 [N].  ``render="auto"`` renders only where a file stores nothing the
    kind consumes (``datasets.stores_input``), decided file by file in the one packing pass: a file that stores ``lines`` - with
    or without ``svgs`` - is packed exactly as with ``render=False``; when NO file stores lines the planks-only set above is
    returned; in a mixed set the files without lines are rendered once here, on the host, and packed beside the stored ones.
    For ``kind="sideface"`` ``auto`` only refuses, by name, a file that stores neither faces nor ``svgs``."""
    if kind not in ("line", "sideface"):
        raise ValueError(f"kind must be 'line' or 'sideface', got {kind!r}")
    if render is True and kind != "line":
        raise ValueError(_SIDEFACE_RENDER)
    if render is True:
        return _pack_rendering(root, info_files, data_cfg)
    auto = render == "auto"
    if extract == "auto":
        def stored(fn):
            with open(os.path.join(root, fn), "r") as f:
                info = json.loads(f.read())
            return "faces" in info and "faceviews" in info
        extract = kind == "sideface" and not all(stored(fn) for fn in info_files)
    if extract and kind != "sideface":
        raise ValueError("extract=True is for kind='sideface'")
    if extract:
        return _pack_extracting(root, info_files, data_cfg, auto)
    line_off, plank_off = [0], [0]
    box, seg, view, typ, coords, attach, names = [], [], [], [], [], [], []
    have_seg = kind == "line"
    n_rendered = 0
    for fn in info_files:
        with open(os.path.join(root, fn), "r") as f:
            info = json.loads(f.read())
        if auto and not stores_input(info, kind):
            if kind == "sideface":
                raise ValueError(f"{fn}: {_SIDEFACE_RENDER}")
            info = rendered(info, "auto", kind, f"{fn}: ")         # (raises by name outside the renderer's domain)
            n_rendered += 1
        if kind == "sideface":
            if "faces" not in info or "faceviews" not in info:
                raise NotImplementedError(_SIDEFACE_MISSING)
            b = np.array(info["faces"], dtype="float").reshape(-1, 4)
            v = np.array(info["faceviews"], dtype="long").reshape(-1)
        else:
            b = np.array(info["lines"], dtype="float").reshape(-1, 4)
            v = np.array(info["views"], dtype="long").reshape(-1)
            t = np.array(info["types"], dtype="long").reshape(-1)
            if len(t) != len(b) or (len(t) and (t.min() < 0 or t.max() > 255)):
                raise ValueError(f"{fn}: {len(t)} types in [0, 255] expected for {len(b)} lines")
            typ.append(t.astype(np.uint8))
            svgs = info.get("svgs") or []
            if len(svgs) == 0 and len(b):
                have_seg = False                                   # boxes only: such a dataset cannot be augmented
            elif have_seg:
                if len(svgs) != len(b):
                    raise ValueError(f"{fn}: {len(svgs)} svgs for {len(b)} lines")
                s = np.zeros((len(b), 4))
                for i, svg in enumerate(svgs):
                    pts = _segment_points(svg)
                    if len(pts) != 2:
                        raise ValueError(f"{fn}: svg {i} has {len(pts)} vertices; the device dataset augments straight "
                                         f"two-point segments only - use datasets.LineDataset (DEVICE_DATASET: false)")
                    s[i] = pts.reshape(4)
                seg.append(s)
        if len(v) != len(b) or (len(v) and (v.min() < 0 or v.max() > 254)):
            raise ValueError(f"{fn}: {len(v)} views in [0, 254] expected for {len(b)} boxes")
        c = np.array(info["coords"], dtype="float").reshape(-1)
        a = np.array(info["attach"], dtype="long").reshape(-1)
        if len(c) % 6 or len(a) != len(c):
            raise ValueError(f"{fn}: coords ({len(c)} values) and attach ({len(a)}) must hold 6 values per plank")
        if not (_in_unit_range(b) and _in_unit_range(c) and (not (have_seg and len(b)) or _in_unit_range(seg[-1]))):
            raise ValueError(f"{fn}: coordinates outside [-1, 1]")
        box.append(b); view.append(v.astype(np.uint8)); coords.append(c.reshape(-1, 6)); attach.append(a.reshape(-1, 6))
        line_off.append(line_off[-1] + len(b)); plank_off.append(plank_off[-1] + len(c) // 6)
        names.append(info["name"])

    def cat(parts, width, dtype):
        return np.concatenate(parts).astype(dtype) if parts else np.zeros((0, width) if width else (0,), dtype)

    if n_rendered and n_rendered == len(info_files):               # no file stores a drawing: the device renders every batch
        n_lines = np.diff(line_off).astype(np.int64)
        for i, fn in enumerate(info_files):
            _check_rendered(f"{fn}: ", len(coords[i]), int(n_lines[i]), data_cfg)
        out = {"kind": "line", "render": True, "names": names, "files": list(info_files),
               "plank_off": np.asarray(plank_off, np.int32), "coords": cat(coords, 6, np.float64), "attach": cat(attach, 6, np.int32)}
        if data_cfg is not None:
            out["n_lines"] = n_lines
        return out
    out = {"kind": kind, "names": names, "files": list(info_files),
           "line_off": np.asarray(line_off, np.int32), "box": cat(box, 4, np.float64), "view": cat(view, 0, np.uint8),
           "plank_off": np.asarray(plank_off, np.int32), "coords": cat(coords, 6, np.float64),
           "attach": cat(attach, 6, np.int32)}
    if kind == "line":
        out["seg"] = cat(seg, 4, np.float64) if have_seg else None
        out["type"] = cat(typ, 0, np.uint8)
    return out


def _pack_extracting(root, info_files, data_cfg, auto_render=False):
    line_off, plank_off = [0], [0]
    seg, view, coords, attach, names, n_faces = [], [], [], [], [], []
    for fn in info_files:
        with open(os.path.join(root, fn), "r") as f:
            info = json.loads(f.read())
        if auto_render and not stores_input(info, "sideface"):
            raise ValueError(f"{fn}: {_SIDEFACE_RENDER}")
        s = two_point_segments(info.get("svgs") or [], f"{fn}: ")
        v = np.array(info["views"], dtype="long").reshape(-1)
        if len(v) != len(s) or (len(v) and (v.min() < 0 or v.max() > 254)):
            raise ValueError(f"{fn}: {len(v)} views in [0, 254] expected for {len(s)} svgs")
        if len(s) > MAX_LINES:
            raise ValueError(f"{fn}: {len(s)} lines, the extraction kernel holds at most {MAX_LINES}")
        if any(view_faces(s, v, k)[1] & EXTRACT_OUT_OF_DOMAIN for k in range(3)):
            raise ValueError(f"{fn}: {_DOMAIN}")
        c = np.array(info["coords"], dtype="float").reshape(-1)
        a = np.array(info["attach"], dtype="long").reshape(-1)
        if len(c) % 6 or len(a) != len(c):
            raise ValueError(f"{fn}: coords ({len(c)} values) and attach ({len(a)}) must hold 6 values per plank")
        if not _in_unit_range(c):
            raise ValueError(f"{fn}: coordinates outside [-1, 1]")
        if data_cfg is not None:
            n_faces.append(sideface_count(s, v, data_cfg, f"{fn}: "))
        seg.append(s); view.append(v.astype(np.uint8)); coords.append(c.reshape(-1, 6)); attach.append(a.reshape(-1, 6))
        line_off.append(line_off[-1] + len(s)); plank_off.append(plank_off[-1] + len(c) // 6)
        names.append(info["name"])

    def cat(parts, width, dtype):
        return np.concatenate(parts).astype(dtype) if parts else np.zeros((0, width) if width else (0,), dtype)

    segs = cat(seg, 4, np.float64)
    box = np.stack([np.minimum(segs[:, 0], segs[:, 2]), np.minimum(segs[:, 1], segs[:, 3]),
                    np.maximum(segs[:, 0], segs[:, 2]), np.maximum(segs[:, 1], segs[:, 3])], axis=1)
    out = {"kind": "sideface", "extract": True, "names": names, "files": list(info_files),
           "line_off": np.asarray(line_off, np.int32), "box": box, "seg": segs, "view": cat(view, 0, np.uint8),
           "plank_off": np.asarray(plank_off, np.int32), "coords": cat(coords, 6, np.float64),
           "attach": cat(attach, 6, np.int32)}
    if data_cfg is not None:
        out["n_faces"] = np.asarray(n_faces, np.int64)
    return out


def _pack_rendering(root, info_files, data_cfg):
    plank_off, coords, attach, names, n_lines = [0], [], [], [], []
    for fn in info_files:
        with open(os.path.join(root, fn), "r") as f:
            info = json.loads(f.read())
        c = np.array(info["coords"], dtype="float").reshape(-1)
        a = np.array(info["attach"], dtype="long").reshape(-1)
        if len(c) % 6 or len(a) != len(c):
            raise ValueError(f"{fn}: coords ({len(c)} values) and attach ({len(a)}) must hold 6 values per plank")
        if not _in_unit_range(c):
            raise ValueError(f"{fn}: coordinates outside [-1, 1]")
        if len(c) // 6 > RENDER_MAX_PLANKS:
            raise ValueError(f"{fn}: {len(c) // 6} planks, the render kernel draws at most {RENDER_MAX_PLANKS} (PA_RENDER_MAX_PLANKS)")
        if data_cfg is not None:
            n_lines.append(render_count(c, data_cfg, f"{fn}: "))
        coords.append(c.reshape(-1, 6)); attach.append(a.reshape(-1, 6))
        plank_off.append(plank_off[-1] + len(c) // 6)
        names.append(info["name"])
    out = {"kind": "line", "render": True, "names": names, "files": list(info_files),
           "plank_off": np.asarray(plank_off, np.int32),
           "coords": np.concatenate(coords).astype(np.float64) if coords else np.zeros((0, 6), np.float64),
           "attach": np.concatenate(attach).astype(np.int32) if attach else np.zeros((0, 6), np.int32)}
    if data_cfg is not None:
        out["n_lines"] = np.asarray(n_lines, np.int64)
    return out


def _get(cfg, key, default):
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


class DeviceDrawings:
    """The packed arrays of ``pack_infos`` in HBM.  ``token``: END / PAD; ``data_cfg``: the ``DATA`` node the CPU classes
    take (VOCAB_SIZE, NUM_INPUT_DOF, MAX_INPUT_LENGTH, MAX_OUTPUT_LENGTH, NUM_BITS, AUG_RATIO, NOISE_RATIO, NOISE_LENGTH)."""

    def __init__(self, packed, token, data_cfg, device, seed=0):
        self.kind = packed["kind"]
        self.names = list(packed["names"])
        self.token = token
        self.vocab_size = int(data_cfg.VOCAB_SIZE)
        self.max_input_length = int(data_cfg.MAX_INPUT_LENGTH)
        self.max_output_length = int(data_cfg.MAX_OUTPUT_LENGTH)
        self.num_bits = int(data_cfg.NUM_BITS)
        self.aug_ratio = float(_get(data_cfg, "AUG_RATIO", 0.0))
        self.noise_ratio = float(_get(data_cfg, "NOISE_RATIO", 0.0))
        self.noise_length = float(_get(data_cfg, "NOISE_LENGTH", 0.0))
        self.seed = int(seed)
        if int(data_cfg.NUM_INPUT_DOF) != 4:
            raise ValueError(f"the device dataset writes 4 tokens per primitive, NUM_INPUT_DOF is {data_cfg.NUM_INPUT_DOF}")
        n_planks = np.diff(packed["plank_off"]).astype(np.int64)
        files = packed.get("files") or self.names
        self.render = bool(packed.get("render", False))                # the drawing from the planks, on the device (section 27)
        if not self.render:
            self.n_lines = np.diff(packed["line_off"]).astype(np.int64)
        elif packed.get("n_lines") is not None:
            self.n_lines = np.asarray(packed["n_lines"], dtype=np.int64)
        else:
            off = packed["plank_off"]
            self.n_lines = np.asarray([render_count(packed["coords"][off[i]:off[i + 1]], data_cfg, f"{files[i]}: ")
                                       for i in range(len(self.names))], np.int64)
        self.max_planks = int(n_planks.max()) if len(n_planks) else 0
        self.extract = bool(packed.get("extract", False))              # side faces from the lines, on the device (section 26)
        self.n_prims = self.n_lines                                    # primitives in a row without augmentation
        if self.extract:
            self.thresholds = tuple(float(t) for t in sideface_thresholds(data_cfg))
            if packed.get("n_faces") is not None:
                self.n_prims = np.asarray(packed["n_faces"], dtype=np.int64)
            else:
                off = packed["line_off"]
                self.n_prims = np.asarray([sideface_count(packed["seg"][off[i]:off[i + 1]], packed["view"][off[i]:off[i + 1]],
                                                          data_cfg, f"{files[i]}: ") for i in range(len(self.names))], np.int64)
        for i in np.nonzero(4 * self.n_prims + 1 > self.max_input_length - 1)[0]:
            raise ValueError(f"{files[i]}: {4 * self.n_prims[i]} input tokens do not fit MAX_INPUT_LENGTH={self.max_input_length}")
        for i in np.nonzero(self.n_lines > MAX_LINES)[0]:
            raise ValueError(f"{files[i]}: {self.n_lines[i]} lines, the tokenise kernel sorts at most {MAX_LINES}")
        for i in np.nonzero(6 * n_planks + 1 > self.max_output_length)[0]:
            raise ValueError(f"{files[i]}: {6 * n_planks[i]} output tokens do not fit MAX_OUTPUT_LENGTH={self.max_output_length}")
        self.device = torch.device(device)

        def up(a):                                  # never an empty allocation: the ABI takes no NULL arrays
            if a.shape[0] == 0:
                a = np.zeros((1,) + a.shape[1:], a.dtype)
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

        self._plank_off = up(packed["plank_off"])
        self._coords, self._attach = up(packed["coords"]), up(packed["attach"])
        if self.render:                                                # planks only: there are no stored lines
            self._line_off = self._box = self._view = self._seg = self._type = None
            return
        self._line_off = up(packed["line_off"])
        self._box, self._view = up(packed["box"]), up(packed["view"])
        self._seg = up(packed["seg"]) if packed.get("seg") is not None else None
        self._type = up(packed["type"]) if self.kind == "line" else None

    def __len__(self):
        return len(self.names)

    def augments(self, augmentation):
        """Whether ``batch(..., augmentation)`` draws noise at all: lines, or side faces extracted from the lines, with
        ``AUG_RATIO`` > 0 (stored side faces cannot be augmented - the noise acts on the lines)."""
        return bool(augmentation) and (self.kind == "line" or self.extract) and self.aug_ratio > 0.0

    def batch(self, index, epoch=0, augmentation=False, host_index=None, seed=None):
        """``index``: int32 [B] on the device, drawing numbers.  One launch on the current stream -> the collated batch
        dict of the CPU dataset (same keys, order, dtypes, shapes).  ``host_index``: the same numbers on the host, when
        the caller has them (``DeviceLoader`` does) - names and ``_n_valid`` then need no device -> host read.  ``seed``
        (default: the constructor's) keys the augmentation draws together with ``epoch``.
        Without augmentation the unmasked encoder rows are known on the host, sum(4 n_i + 1): ``_n_valid`` (the cheap
        branch of ``PlankModel.prepare_batch``); with it the count depends on the deleted lines and is left out."""
        if index.dtype != torch.int32 or not index.is_cuda or index.dim() != 1:
            raise ValueError("index must be a 1-d int32 tensor on the device")
        index = index.contiguous()
        if host_index is None:
            host_index = index.cpu().numpy()
        host_index = np.asarray(host_index, dtype=np.int64)
        if len(host_index) != index.numel() or (len(host_index) and (host_index.min() < 0 or host_index.max() >= len(self))):
            raise IndexError(f"drawing numbers must be {index.numel()} values in [0, {len(self)})")
        aug = self.augments(augmentation)
        if aug and self._seg is None and not self.render:
            raise ValueError("augmentation needs the segments of the info files ('svgs'), which this dataset does not hold")
        B, S, T, dev = index.numel(), self.max_input_length - 1, self.max_output_length, self.device
        with_type = self.kind == "line"
        out = {"name": [self.names[i] for i in host_index]}
        keys = ["input_value", "input_pos", "input_coord", "input_view"] + (["input_type"] if with_type else [])
        for k in keys:
            out[k] = torch.empty(B, S, dtype=torch.int64, device=dev)
        out["input_mask"] = torch.empty(B, S, dtype=torch.bool, device=dev)
        out["output_value"] = torch.empty(B, T, dtype=torch.int64, device=dev)
        out["output_label"] = torch.empty(B, T, dtype=torch.int64, device=dev)
        out["output_mask"] = torch.empty(B, T, dtype=torch.bool, device=dev)
        n_tokens = torch.empty(B, dtype=torch.int32, device=dev)
        if self.extract:
            return self._extract_batch(out, index, host_index, n_tokens, aug, epoch, seed)
        if self.render:
            return self._render_batch(out, index, host_index, n_tokens, aug, epoch, seed)
        L.check(L.lib().pa_tokenise_drawings(
            L.ptr(self._line_off), L.ptr(self._box), L.ptr(self._seg), L.ptr(self._view), L.ptr(self._type),
            L.ptr(self._plank_off), L.ptr(self._coords), L.ptr(self._attach), len(self), L.ptr(index), B, S, T,
            self.num_bits, int(self.token.END), int(self.token.PAD), self.vocab_size, int(with_type), int(aug),
            self.aug_ratio, self.noise_ratio, self.noise_length, int(self.seed if seed is None else seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF,
            L.ptr(out["input_value"]), L.ptr(out["input_pos"]), L.ptr(out["input_coord"]), L.ptr(out["input_view"]),
            L.ptr(out.get("input_type")), L.ptr(out["input_mask"]), L.ptr(out["output_value"]), L.ptr(out["output_label"]),
            L.ptr(out["output_mask"]), L.ptr(n_tokens), L.stream()), "pa_tokenise_drawings")
        out["_n_tokens"] = n_tokens
        if not aug:
            out["_n_valid"] = int((4 * self.n_lines[host_index] + 1).sum())
        return out

    def _render_batch(self, out, index, host_index, n_tokens, aug, epoch, seed):
        """The rendering line set: one launch of ``pa_render_drawings``.  Beside the batch: ``_render_flags`` int32 [B]
        (include/plank_hip.h PA_RENDER_*); the host has checked every drawing, so they are 0 or PA_RENDER_DEGENERATE."""
        B, S, T, dev = index.numel(), self.max_input_length - 1, self.max_output_length, self.device
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        L.check(L.lib().pa_render_drawings(
            L.ptr(self._plank_off), None, L.ptr(self._coords), L.ptr(self._attach), len(self), L.ptr(index), B, self.max_planks, 1,
            S, T, self.num_bits, int(self.token.END), int(self.token.PAD), self.vocab_size, 1, int(aug),
            self.aug_ratio, self.noise_ratio, self.noise_length, int(self.seed if seed is None else seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF,
            L.ptr(out["input_value"]), L.ptr(out["input_pos"]), L.ptr(out["input_coord"]), L.ptr(out["input_view"]),
            L.ptr(out["input_type"]), L.ptr(out["input_mask"]), L.ptr(out["output_value"]), L.ptr(out["output_label"]),
            L.ptr(out["output_mask"]), L.ptr(n_tokens), None, None, None, None, L.ptr(flags), L.stream()), "pa_render_drawings")
        out["_n_tokens"], out["_render_flags"] = n_tokens, flags
        if not aug:
            out["_n_valid"] = int((4 * self.n_lines[host_index] + 1).sum())
        return out

    def _extract_batch(self, out, index, host_index, n_tokens, aug, epoch, seed):
        """The extracting sideface set: one launch of ``pa_tokenise_sideface_drawings``.  Beside the batch: ``_extract_flags``
        int32 [B] (include/plank_hip.h PA_EXTRACT_*), ``_faces`` f64 [B, F, 4] / ``_faceviews`` u8 [B, F] / ``_n_faces`` int32
        [B]: the merged boxes before quantisation, in the order of the row's tokens."""
        B, S, T, dev = index.numel(), self.max_input_length - 1, self.max_output_length, self.device
        F = (S - 1) // 4
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        faces = torch.empty(B, max(F, 1), 4, dtype=torch.float64, device=dev)
        faceviews = torch.empty(B, max(F, 1), dtype=torch.uint8, device=dev)
        n_faces = torch.empty(B, dtype=torch.int32, device=dev)
        L.check(L.lib().pa_tokenise_sideface_drawings(
            L.ptr(self._line_off), None, L.ptr(self._seg), L.ptr(self._view), None,
            L.ptr(self._plank_off), L.ptr(self._coords), L.ptr(self._attach), len(self), L.ptr(index), B, S, T,
            self.num_bits, int(self.token.END), int(self.token.PAD), self.vocab_size, 0, int(aug),
            self.aug_ratio, self.noise_ratio, self.noise_length, int(self.seed if seed is None else seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF,
            L.ptr(out["input_value"]), L.ptr(out["input_pos"]), L.ptr(out["input_coord"]), L.ptr(out["input_view"]),
            None, L.ptr(out["input_mask"]), L.ptr(out["output_value"]), L.ptr(out["output_label"]),
            L.ptr(out["output_mask"]), L.ptr(n_tokens), *self.thresholds, L.ptr(faces), L.ptr(faceviews), L.ptr(n_faces),
            L.ptr(flags), L.stream()), "pa_tokenise_sideface_drawings")
        out["_n_tokens"], out["_extract_flags"] = n_tokens, flags
        out["_faces"], out["_faceviews"], out["_n_faces"] = faces[:, :F], faceviews[:, :F], n_faces
        if not aug:
            out["_n_valid"] = int((4 * self.n_prims[host_index] + 1).sum())
        return out


class DeviceLoader:
    """Batches of a ``DeviceDrawings`` in the order of torch's own samplers over ``range(N)`` - ``RandomSampler`` /
    ``SequentialSampler`` on one rank, ``DistributedSampler`` under a process group of more than one - so sharding,
    padding and ``drop_last`` are torch's rules.  The epoch's order is uploaded once; a batch's ``index`` is a slice of it.

    The launches go to a stream of the loader's own, so a batch never queues behind the train step in flight.  Every batch
    carries its completion event as ``_ready``; the stream that is current when the batch is handed out already waits for
    it (a device-side dependency, no host synchronisation), and ``data.DevicePrefetcher`` makes its side stream wait too."""

    def __init__(self, drawings, batch_size, shuffle=False, drop_last=False, augmentation=False, seed=0):
        self.drawings, self.batch_size, self.drop_last = drawings, int(batch_size), bool(drop_last)
        self.augmentation, self.seed, self.epoch = bool(augmentation), int(seed), 0
        src = range(len(drawings))
        self._gen = None
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            self.sampler = torch.utils.data.distributed.DistributedSampler(src, shuffle=shuffle, drop_last=drop_last,
                                                                           seed=self.seed)
        elif shuffle:
            self._gen = torch.Generator()
            self.sampler = torch.utils.data.RandomSampler(src, generator=self._gen)
        else:
            self.sampler = torch.utils.data.SequentialSampler(src)
        self.batch_sampler = torch.utils.data.BatchSampler(self.sampler, self.batch_size, self.drop_last)
        self._stream = None

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        if hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(self.epoch)

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        if self._gen is not None:
            self._gen.manual_seed(self.seed + self.epoch)
        order = np.fromiter(iter(self.sampler), dtype=np.int32)
        dev = self.drawings.device
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(self._stream):
            order_dev = torch.from_numpy(order).to(dev)
        for k in range(len(self)):
            lo, hi = k * self.batch_size, min((k + 1) * self.batch_size, len(order))
            with torch.cuda.stream(self._stream):
                batch = self.drawings.batch(order_dev[lo:hi], self.epoch, self.augmentation, host_index=order[lo:hi],
                                            seed=self.seed)
                ready = torch.cuda.Event()
                ready.record(self._stream)
            cur = torch.cuda.current_stream(dev)
            cur.wait_event(ready)
            for v in batch.values():
                if torch.is_tensor(v):
                    v.record_stream(cur)
            batch["_ready"] = ready
            yield batch
