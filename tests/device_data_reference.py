"""The device dataset's tokeniser and augmentation, restated in numpy (TEST INFRASTRUCTURE).

csrc/tokenise.hip is pinned to this module bit for bit (tests/test_device_data_gpu.py); this module is pinned to the CPU classes
(tests/test_device_data_cpu.py): with augmentation off it equals ``LineDataset`` / ``SidefaceDataset`` key for key, and its
augmentation arithmetic equals ``datasets.add_noise`` when that function is fed this module's decisions through a stub generator.

The draws.  h(line, slot) = mix32(slot ^ mix32(line ^ base)), base = mix32(drawing ^ mix32(epoch ^ mix32(seed + 0x9e3779b9))) with
``mix32`` of csrc/pa_device.h (tests/dropout_masks.py); u = (h >> 8) 2^-24 in [0, 1).
  per drawing (line = 0xffffffff):  slot 0: augmented <=> u < AUG_RATIO;
                                    slot 1: num_select = 1 + ((h * max_sel) >> 32), max_sel = min(n, ceil(n * NOISE_RATIO));
  per line:  slot 0: the selected lines are those with the num_select smallest (h, line) pairs;
             slot 1: u > 0.5 deletes the line;
             slot 2: noise = rint(u * NOISE_LENGTH * 1000) / 1000; length <= noise deletes the line;
             slot 3: u > 0.5 shortens the line at the tail, else at the head.
Every decision is exported in the order ``datasets.add_noise`` consumes its generator (``Decisions.queue``).
"""
from __future__ import annotations

import math

import numpy as np

from dropout_masks import mix32

DRAWING = 0xFFFFFFFF
SLOT_SELECT, SLOT_DELETE, SLOT_NOISE, SLOT_END = 0, 1, 2, 3
SLOT_AUGMENT, SLOT_COUNT = 0, 1
BRANCHES = ("not_augmented", "not_selected", "deleted_by_coin", "deleted_too_short", "shortened_head", "shortened_tail",
            "every_line_deleted")


def _u32(v):
    return np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF)


def draw_base(seed, epoch, drawing):
    return mix32(_u32(drawing) ^ mix32(_u32(epoch) ^ mix32(_u32(int(seed) + 0x9E3779B9))))


def draw_hash(seed, epoch, drawing, line, slot):
    """uint64 numpy holding the uint32 hash; broadcasts over its arguments."""
    return mix32(_u32(slot) ^ mix32(_u32(line) ^ draw_base(seed, epoch, drawing)))


def unit(h):
    return (np.asarray(h, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


class Decisions:
    """What the draws decided for one drawing.  ``augmented``; ``num_select``; ``indices`` (the selected lines, ascending
    (hash, line)); per selected line ``coin`` (u of the delete draw), ``noise_u`` and ``end_u`` (None where ``add_noise``
    does not reach that draw).  ``queue()``: (randint value, choice value, [random values...]) in ``add_noise``'s order."""

    def __init__(self):
        self.augmented, self.num_select, self.max_select, self.indices = False, 0, 0, []
        self.coin, self.noise_u, self.end_u, self.branch = {}, {}, {}, {}

    def queue(self):
        randoms = []
        for i in self.indices:
            randoms.append(self.coin[i])
            if self.noise_u[i] is not None:
                randoms.append(self.noise_u[i])
            if self.end_u[i] is not None:
                randoms.append(self.end_u[i])
        return self.num_select, np.asarray(self.indices, dtype=np.int64), randoms


def augment(seg, seed, epoch, drawing, aug_ratio, noise_ratio, noise_length):
    """``seg`` float64 [n, 4] (x0 y0 x1 y1).  Returns (segments float64 [n, 4], keep bool [n], Decisions).  Plain Python floats:
    one rounding per operation."""
    seg = np.asarray(seg, dtype=np.float64).reshape(-1, 4)
    n = len(seg)
    out, keep, dec = seg.copy(), np.ones(n, dtype=bool), Decisions()
    if n == 0:
        return out, keep, dec
    if not float(unit(draw_hash(seed, epoch, drawing, DRAWING, SLOT_AUGMENT))) < aug_ratio:
        return out, keep, dec
    max_sel = min(int(math.ceil(float(n) * float(noise_ratio))), n)
    if max_sel < 1:
        return out, keep, dec
    dec.augmented, dec.max_select = True, max_sel
    dec.num_select = 1 + ((int(draw_hash(seed, epoch, drawing, DRAWING, SLOT_COUNT)) * max_sel) >> 32)
    lines = np.arange(n)
    sel = draw_hash(seed, epoch, drawing, lines, SLOT_SELECT)
    order = np.lexsort((lines, sel))                                    # ascending (hash, line)
    dec.indices = [int(i) for i in order[:dec.num_select]]
    for i in lines:
        dec.branch[int(i)] = "not_selected"
    for i in dec.indices:
        coin = float(unit(draw_hash(seed, epoch, drawing, i, SLOT_DELETE)))
        dec.coin[i], dec.noise_u[i], dec.end_u[i] = coin, None, None
        if coin > 0.5:
            keep[i], dec.branch[i] = False, "deleted_by_coin"
            continue
        x0, y0, x1, y1 = (float(v) for v in seg[i])
        dx, dy = x1 - x0, y1 - y0
        length = math.sqrt(dx * dx + dy * dy)
        u = float(unit(draw_hash(seed, epoch, drawing, i, SLOT_NOISE)))
        dec.noise_u[i] = u
        noise = float(np.rint(u * noise_length * 1000.0)) / 1000.0
        if length <= noise:
            keep[i], dec.branch[i] = False, "deleted_too_short"
            continue
        end = float(unit(draw_hash(seed, epoch, drawing, i, SLOT_END)))
        dec.end_u[i] = end
        if end > 0.5:
            d0, d1, dec.branch[i] = 0.0, length - noise, "shortened_tail"
        else:
            d0, d1, dec.branch[i] = noise, length, "shortened_head"
        t0, t1 = d0 / length, d1 / length
        out[i] = [x0 + t0 * dx, y0 + t0 * dy, x0 + t1 * dx, y0 + t1 * dy]
    return out, keep, dec


def bounds(seg):
    seg = np.asarray(seg, dtype=np.float64).reshape(-1, 4)
    return np.stack([np.minimum(seg[:, 0], seg[:, 2]), np.minimum(seg[:, 1], seg[:, 3]),
                     np.maximum(seg[:, 0], seg[:, 2]), np.maximum(seg[:, 1], seg[:, 3])], axis=1)


def quantise(v, n_bits):
    rq = float(2 ** n_bits - 1)
    return (((np.asarray(v, dtype=np.float64) + 1.0) * rq) / 2.0).astype(np.int64)          # truncation toward zero


def _padded(body, length, fill):
    out = np.full(length, fill, dtype=np.int64)
    out[:len(body)] = body
    return out


def input_rows(box, view, typ, S, n_bits, END, PAD):
    """Sorted by (view, col 0, col 2, col 1, col 3, line number) through ONE integer key, as the kernel does."""
    q = quantise(np.asarray(box, dtype=np.float64).reshape(-1, 4), n_bits)
    view = np.asarray(view, dtype=np.int64)
    n = len(q)
    key = [(int(view[i]), int(q[i, 0]), int(q[i, 2]), int(q[i, 1]), int(q[i, 3]), i) for i in range(n)]
    order = np.asarray(sorted(range(n), key=lambda i: key[i]), dtype=np.int64)
    q, view = q[order], view[order]
    pos = np.asarray([int(np.sum(view[:r] == view[r])) for r in range(n)], dtype=np.int64)
    value = _padded(np.append(q.reshape(-1), END), S, PAD)
    out = {"input_value": value, "input_pos": _padded(np.repeat(pos, 4), S, 0),
           "input_coord": _padded(np.arange(4 * n) % 4, S, 0), "input_view": _padded(np.repeat(view, 4), S, 0)}
    if typ is not None:
        out["input_type"] = _padded(np.repeat(np.asarray(typ, dtype=np.int64)[order], 4), S, 0)
    out["input_mask"] = value == PAD
    return out


def output_rows(coords, attach, T, n_bits, END, PAD, vocab):
    q = quantise(np.asarray(coords, dtype=np.float64).reshape(-1), n_bits)
    value = _padded(np.append(q, END), T, PAD)
    at = _padded(np.asarray(attach, dtype=np.int64).reshape(-1), T, -1)
    return {"output_value": value, "output_label": np.where(at != -1, at + vocab, value), "output_mask": value == PAD}


def sample(packed, i, data_cfg, token, augmentation=False, seed=0, epoch=0):
    """Drawing ``i`` of ``pack_infos``' arrays -> (the dict ``__getitem__`` of the CPU dataset returns, Decisions | None)."""
    lo, hi = int(packed["line_off"][i]), int(packed["line_off"][i + 1])
    plo, phi = int(packed["plank_off"][i]), int(packed["plank_off"][i + 1])
    box, view = packed["box"][lo:hi], packed["view"][lo:hi]
    typ = packed["type"][lo:hi] if packed["kind"] == "line" else None
    dec = None
    if augmentation and packed["kind"] == "line" and float(data_cfg.AUG_RATIO) > 0.0:
        seg, keep, dec = augment(packed["seg"][lo:hi], seed, epoch, i, float(data_cfg.AUG_RATIO), float(data_cfg.NOISE_RATIO),
                                 float(data_cfg.NOISE_LENGTH))
        if dec.augmented:
            box, view, typ = bounds(seg)[keep], view[keep], typ[keep]
    out = {"name": packed["names"][i]}
    out.update(input_rows(box, view, typ, int(data_cfg.MAX_INPUT_LENGTH) - 1, int(data_cfg.NUM_BITS), token.END, token.PAD))
    out.update(output_rows(packed["coords"][plo:phi], packed["attach"][plo:phi], int(data_cfg.MAX_OUTPUT_LENGTH),
                           int(data_cfg.NUM_BITS), token.END, token.PAD, int(data_cfg.VOCAB_SIZE)))
    return out, dec


def collate(samples):
    """What ``torch.utils.data.DataLoader`` makes of the samples, as numpy."""
    out = {"name": [s["name"] for s in samples]}
    for k in samples[0]:
        if k != "name":
            out[k] = np.stack([s[k] for s in samples])
    return out


def branches_of(dec, n):
    """The set of BRANCHES one drawing of ``n`` lines took."""
    if dec is None or not dec.augmented:
        return {"not_augmented"}
    got = set(dec.branch.values())
    if n and all(b.startswith("deleted") for b in dec.branch.values()):
        got.add("every_line_deleted")
    return got


# ------------------------------------------------------------------------------------------ generated info files
def make_data_cfg(max_input_length, max_output_length, aug_ratio=0.0, noise_ratio=0.0, noise_length=0.0):
    from plankassembly_amd.config import CfgNode
    return CfgNode({"NUM_INPUT_DOF": 4, "NUM_OUTPUT_DOF": 6, "VOCAB_SIZE": 514, "NUM_VIEW": 3, "NUM_TYPE": 2,
                    "MAX_INPUT_LENGTH": max_input_length, "MAX_OUTPUT_LENGTH": max_output_length, "NUM_BITS": 9,
                    "AUG_RATIO": aug_ratio, "NOISE_RATIO": noise_ratio, "NOISE_LENGTH": noise_length})


def make_info(name, segs, views, types, coords, attach, faces=False):
    """One info dict in the reference's schema (dataset/prepare_info.py:59-70) from two-point segments [n, 4]."""
    segs = np.asarray(segs, dtype=np.float64).reshape(-1, 4)
    info = {"name": name, "lines": bounds(segs).tolist(), "views": [int(v) for v in views], "types": [int(t) for t in types],
            "svgs": [{"type": "LineString", "coordinates": [[float(s[0]), float(s[1])], [float(s[2]), float(s[3])]]} for s in segs],
            "coords": np.asarray(coords, dtype=np.float64).reshape(-1, 6).tolist(),
            "attach": np.asarray(attach, dtype=np.int64).reshape(-1, 6).tolist()}
    if faces:
        info["faces"], info["faceviews"] = info["lines"], info["views"]
    return info


def random_planks(rng, npk):
    """``npk`` planks (plank 0 = the overall bounding box) with the pointer attachments the reference's pointer mask allows."""
    from plankassembly_amd.data import pointer_mask_row
    grid = np.round(rng.uniform(-1, 0.95, size=10), 3)
    lo, hi = rng.choice(grid, size=(npk, 3)), rng.choice(grid, size=(npk, 3))
    coords = np.concatenate([np.minimum(lo, hi), np.maximum(lo, hi) + 0.05], axis=1).round(3)
    coords[0] = np.concatenate([coords[:, :3].min(0), coords[:, 3:].max(0)])
    flat, attach = coords.reshape(-1), np.full(npk * 6, -1)
    for t in range(6, npk * 6):
        cand = np.nonzero(pointer_mask_row(t, t))[0]
        cand = cand[np.isclose(flat[cand], flat[t])]
        if len(cand):
            attach[t] = int(cand[0])
    return coords, attach


def random_info(rng, name, n_lines, n_planks, faces=False):
    """Segments on a 3-decimal grid: a third axis-aligned, a third short (below 0.3 long), some of zero length."""
    nl, npk = int(rng.integers(n_lines[0], n_lines[1] + 1)), int(rng.integers(n_planks[0], n_planks[1] + 1))
    p0 = np.round(rng.uniform(-1, 1, size=(nl, 2)), 3)
    p1 = np.round(rng.uniform(-1, 1, size=(nl, 2)), 3)
    style = rng.integers(0, 6, size=nl)
    for i in range(nl):
        if style[i] == 0:
            p1[i, 0] = p0[i, 0]
        elif style[i] == 1:
            p1[i, 1] = p0[i, 1]
        elif style[i] in (2, 3):
            p1[i] = np.clip(np.round(p0[i] + rng.uniform(-0.15, 0.15, size=2), 3), -1, 1)
        elif style[i] == 4 and rng.random() < 0.3:
            p1[i] = p0[i]
    coords, attach = random_planks(rng, npk)
    return make_info(name, np.concatenate([p0, p1], axis=1), rng.integers(0, 3, nl), rng.integers(0, 2, nl), coords, attach, faces)


def write_infos(root, infos):
    import json
    import os
    os.makedirs(root, exist_ok=True)
    files = []
    for info in infos:
        with open(os.path.join(root, info["name"] + ".json"), "w") as f:
            json.dump(info, f)
        files.append(info["name"] + ".json")
    return files


def augmentation_set(n=64, seed=5, n_lines=(1, 40)):
    """The generated set of the augmentation tests (64 drawings of 1-40 lines) and its DATA node: AUG_RATIO 0.5, NOISE_RATIO
    0.5, NOISE_LENGTH 0.3 - a third of the segments are shorter than that."""
    rng = np.random.default_rng(seed)
    # (the first eight have one line: only there can the noise delete EVERY line, NOISE_RATIO 0.5 selects at most half)
    infos = [random_info(rng, f"aug{i:04d}", (1, 1) if i < 8 else n_lines, (1, 6)) for i in range(n)]
    return infos, make_data_cfg(4 * n_lines[1] + 2, 40, 0.5, 0.5, 0.3)
