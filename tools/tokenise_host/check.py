"""csrc/tokenise.hip on the host: the kernel source compiled by the host compiler against tools/tokenise_host/pa_device.h (one OS thread per
GPU thread) and compared with the CPU datasets and the numpy restatement on the sets of tests/test_device_data_gpu.py - golden infos,
edge shapes, more lines than threads, three epochs of the augmentation set.  A check of the kernel's logic and float64 arithmetic
(-ffp-contract=off) where there is no GPU; it says nothing about the device's rounding, which the GPU tests pin.
`python tools/tokenise_host/check.py [--sanitize]`; --sanitize instead builds a stand-alone program with AddressSanitizer + UBSan
that runs drawings longer than the row, above the kernel's line maximum and out-of-range drawing numbers."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
CXX = os.environ.get("CXX") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++")


def stage():
    """The kernel source next to the stand-in header, with the ABI header where its relative include expects it."""
    tmp = tempfile.mkdtemp(prefix="tokenise_host_")
    os.makedirs(os.path.join(tmp, "a", "b"))
    os.makedirs(os.path.join(tmp, "include"))
    shutil.copy(os.path.join(REPO, "plankassembly_amd", "csrc", "tokenise.hip"), os.path.join(tmp, "a", "b", "tokenise.cpp"))
    shutil.copy(os.path.join(REPO, "plankassembly_amd", "csrc", "sideface.h"), os.path.join(tmp, "a", "b", "sideface.h"))
    shutil.copy(os.path.join(HERE, "pa_device.h"), os.path.join(tmp, "a", "b", "pa_device.h"))
    shutil.copy(os.path.join(REPO, "include", "plank_hip.h"), os.path.join(tmp, "include", "plank_hip.h"))
    return tmp


if "--sanitize" in sys.argv:
    tmp = stage()
    shutil.copy(os.path.join(HERE, "bounds_main.cpp"), os.path.join(tmp, "main.cpp"))
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I.", "-o", "bounds", "main.cpp"], cwd=tmp, check=True)
    raise SystemExit(subprocess.run([os.path.join(tmp, "bounds")]).returncode)

TMP = stage()
subprocess.run([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-o", "libtok_host.so",
                os.path.join("a", "b", "tokenise.cpp")], cwd=TMP, check=True)
import device_data_reference as R
import test_device_data_gpu as G
from plankassembly_amd.device_data import pack_infos

lib = C.CDLL(os.path.join(TMP, "libtok_host.so"))
P, I, Dd, U = C.c_void_p, C.c_int32, C.c_double, C.c_uint32
lib.pa_tokenise_drawings.restype = I
lib.pa_tokenise_drawings.argtypes = [P]*8 + [I, P] + [I]*9 + [Dd]*3 + [U, U] + [P]*11
TOKEN = G.TOKEN
def ptr(a): return None if a is None else a.ctypes.data
def batch(packed, cfg, index, epoch=0, aug=False, seed=0):
    kind = packed["kind"]; wt = kind == "line"
    B, S, T = len(index), cfg.MAX_INPUT_LENGTH - 1, cfg.MAX_OUTPUT_LENGTH
    def up(a): return np.ascontiguousarray(a if a.shape[0] else np.zeros((1,) + a.shape[1:], a.dtype))
    arrs = {k: up(packed[k]) for k in ("line_off", "box", "view", "plank_off", "coords", "attach")}
    seg = up(packed["seg"]) if packed.get("seg") is not None else None
    typ = up(packed["type"]) if wt else None
    index = np.ascontiguousarray(index, dtype=np.int32)
    out = {"name": [packed["names"][i] for i in index]}
    for k in ["input_value", "input_pos", "input_coord", "input_view"] + (["input_type"] if wt else []):
        out[k] = np.full((B, S), -7, np.int64)
    out["input_mask"] = np.full((B, S), 9, np.uint8)
    out["output_value"] = np.full((B, T), -7, np.int64); out["output_label"] = np.full((B, T), -7, np.int64)
    out["output_mask"] = np.full((B, T), 9, np.uint8)
    nt = np.zeros(B, np.int32)
    aug = bool(aug) and wt and cfg.AUG_RATIO > 0
    rc = lib.pa_tokenise_drawings(ptr(arrs["line_off"]), ptr(arrs["box"]), ptr(seg), ptr(arrs["view"]), ptr(typ), ptr(arrs["plank_off"]),
        ptr(arrs["coords"]), ptr(arrs["attach"]), len(packed["names"]), ptr(index), B, S, T, cfg.NUM_BITS, 512, 513, 514, int(wt), int(aug),
        float(cfg.AUG_RATIO), float(cfg.NOISE_RATIO), float(cfg.NOISE_LENGTH), seed, epoch,
        ptr(out["input_value"]), ptr(out["input_pos"]), ptr(out["input_coord"]), ptr(out["input_view"]), ptr(out.get("input_type")),
        ptr(out["input_mask"]), ptr(out["output_value"]), ptr(out["output_label"]), ptr(out["output_mask"]), ptr(nt), None)
    assert rc == 0, rc
    assert set(np.unique(out["input_mask"])) <= {0, 1} and set(np.unique(out["output_mask"])) <= {0, 1}
    out["input_mask"] = out["input_mask"].astype(bool); out["output_mask"] = out["output_mask"].astype(bool)
    assert np.array_equal(nt, (~out["input_mask"]).sum(1)), nt
    return out
def same(got, want):
    assert list(got) == list(want), (list(got), list(want))
    for k, w in want.items():
        if k == "name": assert list(got[k]) == list(w); continue
        w = w.numpy() if torch.is_tensor(w) else w
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
        bad = np.argwhere(got[k] != w)
        assert len(bad) == 0, (k, bad[:5], got[k][tuple(bad[0])], w[tuple(bad[0])])
# golden + edges
for kind in ("line", "sideface"):
    cfg = R.make_data_cfg(120, 60)
    packed = pack_infos(G.INFOS, G.GOLDEN_FILES, kind)
    same(batch(packed, cfg, np.arange(3)), G._cpu_batch(kind, G.INFOS, G.GOLDEN_FILES, cfg))
    d = tempfile.mkdtemp(); cfg = R.make_data_cfg(122, 60)
    files = R.write_infos(d, G._edge_infos(30, 9, kind == "sideface"))
    packed = pack_infos(d, files, kind)
    same(batch(packed, cfg, np.arange(len(files))), G._cpu_batch(kind, d, files, cfg))
    print(kind, "golden + edges ok")
# long
d = tempfile.mkdtemp(); rng = np.random.default_rng(29)
infos = [R.random_info(rng, "long280", (280, 280), (21, 21)), R.random_info(rng, "long299", (299, 299), (2, 2)),
         R.random_info(rng, "mid", (257, 257), (5, 5)), R.random_info(rng, "short", (3, 3), (1, 1))]
files = R.write_infos(d, infos); cfg = R.make_data_cfg(1200, 128)
packed = pack_infos(d, files, "line")
same(batch(packed, cfg, np.arange(4)), G._cpu_batch("line", d, files, cfg)); print("long ok")
# augmentation
d = tempfile.mkdtemp(); infos, cfg = R.augmentation_set(); files = R.write_infos(d, infos)
packed = pack_infos(d, files, "line")
for e in range(3):
    want = R.collate([R.sample(packed, i, cfg, TOKEN, True, 7, e)[0] for i in range(len(files))])
    same(batch(packed, cfg, np.arange(len(files)), e, True, 7), want)
    print("aug epoch", e, "ok")
idx = np.array([5, 63, 0, 17, 99999, -1], dtype=np.int32)   # out-of-range drawing numbers: the empty drawing
packed2 = dict(packed); o = batch(packed2, cfg, idx[:4], 1, True, 7)
full = batch(packed, cfg, np.arange(len(files)), 1, True, 7)
assert all(np.array_equal(o[k], full[k][idx[:4]]) for k in o if k != "name"); print("batch independence ok")
