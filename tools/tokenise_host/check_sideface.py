"""csrc/sideface.h on the host, as tools/tokenise_host/check.py does for the line kind: the kernel source compiled by the host
compiler (one OS thread per GPU thread) and compared with the numpy restatement (tests/sideface_reference.py `sample`) on generated
drawings - clean, augmented at two noise ratios, a tiled drawing of 1024 lines, a row cut at its capacity, drawings outside the domain.
A check of the kernel's logic and float64 arithmetic where there is no GPU; the GPU tests pin the device.
`python tools/tokenise_host/check_sideface.py`"""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
CXX = os.environ.get("CXX") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++")

import device_data_reference as R
import sideface_reference as SR
from plankassembly_amd.device_data import pack_infos

TOKEN = types.SimpleNamespace(END=512, PAD=513)
TMP = tempfile.mkdtemp(prefix="sideface_host_")
os.makedirs(os.path.join(TMP, "a", "b"))
os.makedirs(os.path.join(TMP, "include"))
for name in ("tokenise.hip", "sideface.h"):
    shutil.copy(os.path.join(REPO, "plankassembly_amd", "csrc", name), os.path.join(TMP, "a", "b", name.replace(".hip", ".cpp")))
shutil.copy(os.path.join(HERE, "pa_device.h"), os.path.join(TMP, "a", "b", "pa_device.h"))
shutil.copy(os.path.join(REPO, "include", "plank_hip.h"), os.path.join(TMP, "include", "plank_hip.h"))
subprocess.run([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-o", "libtok_host.so",
                os.path.join("a", "b", "tokenise.cpp")], cwd=TMP, check=True)
lib = C.CDLL(os.path.join(TMP, "libtok_host.so"))
P, I, Dd, U = C.c_void_p, C.c_int32, C.c_double, C.c_uint32
lib.pa_tokenise_sideface_drawings.restype = I
lib.pa_tokenise_sideface_drawings.argtypes = [P] * 8 + [I, P] + [I] * 9 + [Dd] * 3 + [U, U] + [P] * 10 + [Dd] * 3 + [P] * 5


def ptr(a):
    return None if a is None else a.ctypes.data


def batch(packed, cfg, index, epoch=0, aug=False, seed=0):
    B, S, T = len(index), cfg.MAX_INPUT_LENGTH - 1, cfg.MAX_OUTPUT_LENGTH
    F = (S - 1) // 4
    up = lambda a: np.ascontiguousarray(a if a.shape[0] else np.zeros((1,) + a.shape[1:], a.dtype))
    arrs = {k: up(packed[k]) for k in ("line_off", "seg", "view", "plank_off", "coords", "attach")}
    index = np.ascontiguousarray(index, dtype=np.int32)
    out = {k: np.full((B, S), -7, np.int64) for k in ("input_value", "input_pos", "input_coord", "input_view")}
    out["input_mask"] = np.full((B, S), 9, np.uint8)
    out["output_value"] = np.full((B, T), -7, np.int64); out["output_label"] = np.full((B, T), -7, np.int64)
    out["output_mask"] = np.full((B, T), 9, np.uint8)
    nt, nf, flags = np.zeros(B, np.int32), np.zeros(B, np.int32), np.full(B, -1, np.int32)
    faces, fviews = np.full((B, F, 4), 7.0), np.full((B, F), 9, np.uint8)
    th = SR.D.sideface_thresholds(cfg)
    rc = lib.pa_tokenise_sideface_drawings(
        ptr(arrs["line_off"]), None, ptr(arrs["seg"]), ptr(arrs["view"]), None, ptr(arrs["plank_off"]), ptr(arrs["coords"]),
        ptr(arrs["attach"]), len(packed["names"]), ptr(index), B, S, T, cfg.NUM_BITS, 512, 513, 514, 0, int(aug and cfg.AUG_RATIO > 0),
        float(cfg.AUG_RATIO), float(cfg.NOISE_RATIO), float(cfg.NOISE_LENGTH), seed, epoch,
        ptr(out["input_value"]), ptr(out["input_pos"]), ptr(out["input_coord"]), ptr(out["input_view"]), None, ptr(out["input_mask"]),
        ptr(out["output_value"]), ptr(out["output_label"]), ptr(out["output_mask"]), ptr(nt), *th, ptr(faces), ptr(fviews), ptr(nf),
        ptr(flags), None)
    assert rc == 0, rc
    out["input_mask"] = out["input_mask"].astype(bool); out["output_mask"] = out["output_mask"].astype(bool)
    assert np.array_equal(nt, (~out["input_mask"]).sum(1)) and np.array_equal(nt, 4 * nf + 1), (nt, nf)
    return out, flags, faces, fviews, nf


def check(packed, cfg, index, epoch=0, aug=False, seed=0):
    out, flags, faces, fviews, nf = batch(packed, cfg, index, epoch, aug, seed)
    seen = 0
    for r, i in enumerate(index):
        want, wflags, wfaces, wviews = SR.sample(packed, i, cfg, TOKEN, aug, seed, epoch)
        for k, w in want.items():
            if k != "name":
                assert np.array_equal(out[k][r], w), (i, k, np.argwhere(out[k][r] != w)[:4].tolist())
        assert flags[r] == wflags, (i, flags[r], wflags)
        assert nf[r] == len(wfaces) and np.array_equal(faces[r, :nf[r]].view(np.int64), wfaces.view(np.int64).reshape(-1, 4)), i
        assert np.array_equal(fviews[r, :nf[r]], wviews) and not faces[r, nf[r]:].any()
        seen |= int(flags[r])
    return seen


rng = np.random.default_rng(3)
infos = [SR.render_drawing(np.random.default_rng(s), int(rng.integers(2, 13)), f"gen{s:02d}") for s in range(24)]
seg, views = SR.tiled_cells(3, 1, 0.1, 0.02)
infos.append(R.make_info("row", seg, views, [0] * len(seg), np.zeros((1, 6)), np.full((1, 6), -1)))
infos.append(R.make_info("empty", np.zeros((0, 4)), [], [], np.zeros((1, 6)), np.full((1, 6), -1)))
seg, views = SR.tiled_cells(1, 1, 0.5, 0.02)
infos.append(R.make_info("one", seg, views, [0] * 4, np.zeros((1, 6)), np.full((1, 6), -1)))
seg, views = SR.tiled_cells(31, 15, 0.03, 0.03)                             # 31 * 16 + 15 * 32 = 976 lines, 465 faces
infos.append(R.make_info("tiles", seg, views, [0] * len(seg), np.zeros((1, 6)), np.full((1, 6), -1)))
d = tempfile.mkdtemp()
files = R.write_infos(d, infos)
cfg = SR.make_data_cfg(4 * 500 + 2, 80)
packed = pack_infos(d, files, "sideface", extract=True, data_cfg=cfg)
print("clean flags", check(packed, cfg, np.arange(len(files))))
for ratio, length in ((0.15, 0.02), (0.5, 0.3), (1.0, 0.3)):
    cfg = SR.make_data_cfg(4 * 500 + 2, 80, 1.0, ratio, length)
    for epoch in range(2):
        print("aug", ratio, "epoch", epoch, "flags", check(packed, cfg, np.arange(len(files)), epoch, True, 7))
small = SR.make_data_cfg(4 * 5 + 2, 80)                                     # a row of 5 faces: the cut
print("cut flags", check(packed, small, np.arange(8)))
bad = dict(packed)
bad["seg"] = packed["seg"].copy()
bad["seg"][int(packed["line_off"][3])] = [0.0, 0.0, 0.5, 0.5]               # a diagonal
bad["seg"][int(packed["line_off"][4]) + 1] = bad["seg"][int(packed["line_off"][4])]      # a duplicate
bad["seg"][int(packed["line_off"][5])] = [0.0, 0.0, 1.5, 0.0]               # outside [-1, 1]
bad["seg"][int(packed["line_off"][6])] = [np.nan, 0.0, 0.5, 0.0]
cfg = SR.make_data_cfg(4 * 500 + 2, 80)
print("out of domain flags", check(bad, cfg, np.arange(3, 8)))
print("ok")
