"""What side-face extraction costs, at the sideface config's batch: B 64, MAX_INPUT_LENGTH 300 (S 299).

`--drawings N` (default 256) generated drawings of 4-12 planks (tests/sideface_reference.py `render_drawing`):
  1. host `extract_sideface` ms per drawing, one thread (no GPU needed: `--host-only`);
  2. one `pa_tokenise_sideface_drawings` launch between HIP events on an idle stream, augmentation off and on (AUG_RATIO 1 so that
     every row is augmented: the worst case - the config's 0.1 augments a tenth of them);
  3. in the same session `pa_tokenise_drawings` (unchanged from before the extraction existed) on the same drawings' pre-extracted
     faces, the stored-faces sideface path;
  4. `--step-ms X`: the sideface train step of the same session (`python bench.py --gpus 1 --config sideface`, its step time at B 64)
     to report the ratio launch / step against; below 1 the loader's stream never holds the step back.
`python tools/sideface_rate.py --out profiles/sideface_extract_time.txt [--step-ms X]`"""
import argparse
import os
import shutil
import sys
import tempfile
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np

import device_data_reference as R
import sideface_reference as SR
from plankassembly_amd import datasets as D

TOKEN = types.SimpleNamespace(END=512, PAD=513)
BATCH, MAX_INPUT_LENGTH, MAX_OUTPUT_LENGTH = 64, 300, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drawings", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--step-ms", type=float, default=None)
    args = ap.parse_args()
    sink = open(args.out, "w") if args.out else None

    def say(line=""):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    infos = []
    for i in range(args.drawings):
        rng = np.random.default_rng(5000 + i)
        infos.append(SR.render_drawing(rng, int(rng.integers(4, 13)), f"d{i:05d}"))
    segs = [SR.info_segments(info) for info in infos]
    lines = np.array([len(s) for s, _ in segs])
    say(f"side-face extraction: {args.drawings} generated drawings of 4-12 planks, {lines.min()}-{lines.max()} lines (median "
        f"{int(np.median(lines))}), B {BATCH}, MAX_INPUT_LENGTH {MAX_INPUT_LENGTH}")

    # ---- 1. the host
    t0 = time.perf_counter()
    faces = [D.extract_sideface(s, v, *SR.THRESHOLDS) for s, v in segs]
    dt = time.perf_counter() - t0
    counts = np.array([len(f) for f, _ in faces])
    say(f"\n1. host extract_sideface, one thread: {dt / len(segs) * 1e3:.2f} ms / drawing ({counts.min()}-{counts.max()} side faces, "
        f"median {int(np.median(counts))})")
    if args.host_only:
        say("\n2.-4. not measured (--host-only)")
        return

    import torch
    from plankassembly_amd.device_data import DeviceDrawings, pack_infos
    tmp = tempfile.mkdtemp(prefix="sideface_rate_")
    say(f"   {torch.cuda.get_device_name(0)}")
    cfg = SR.make_data_cfg(MAX_INPUT_LENGTH, MAX_OUTPUT_LENGTH, 1.0, 0.15, 0.02)
    files = R.write_infos(os.path.join(tmp, "lines"), infos)
    t0 = time.perf_counter()
    packed = pack_infos(os.path.join(tmp, "lines"), files, "sideface", extract=True, data_cfg=cfg)
    say(f"   pack_infos(extract=True): {time.perf_counter() - t0:.1f} s once")
    stored = []
    for info, (f, v) in zip(infos, faces):
        stored.append(dict(info, faces=f.tolist(), faceviews=[int(x) for x in v]))
    sfiles = R.write_infos(os.path.join(tmp, "faces"), stored)
    sets = {"extract": DeviceDrawings(packed, TOKEN, cfg, "cuda"),
            "stored": DeviceDrawings(pack_infos(os.path.join(tmp, "faces"), sfiles, "sideface"), TOKEN, cfg, "cuda")}

    def launch_us(dd, aug):
        rng = np.random.default_rng(1)
        out = []
        for rep in range(40):
            host = rng.choice(len(dd), BATCH, replace=False).astype(np.int32)
            idx = torch.from_numpy(host).cuda()
            dd.batch(idx, rep, aug, host_index=host)            # (warms the allocator: the timed call reuses these blocks)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); dd.batch(idx, rep, aug, host_index=host); b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
        out.sort()
        return out[len(out) // 2], out[0], out[-1]

    say("\n2. pa_tokenise_sideface_drawings, one launch of 64 drawings between HIP events (median / min / max of 40 batches)")
    results = {}
    for aug in (False, True):
        results[aug] = launch_us(sets["extract"], aug)
        say(f"   augmentation {str(aug):5}: {results[aug][0]:8.1f} / {results[aug][1]:8.1f} / {results[aug][2]:8.1f} us")
    say("\n3. pa_tokenise_drawings on the same drawings' pre-extracted faces (the stored-faces path)")
    base = launch_us(sets["stored"], False)
    say(f"   {base[0]:8.1f} / {base[1]:8.1f} / {base[2]:8.1f} us; extraction / stored = {results[False][0] / base[0]:.1f} (clean), "
        f"{results[True][0] / base[0]:.1f} (augmented)")
    if args.step_ms:
        say(f"\n4. sideface train step of this session: {args.step_ms:.3f} ms at B {BATCH}; launch / step = "
            f"{results[False][0] / 1e3 / args.step_ms:.3f} (clean), {results[True][0] / 1e3 / args.step_ms:.3f} (every row augmented)")
    else:
        say("\n4. train step: not measured (pass --step-ms from `python bench.py --gpus 1 --config sideface`)")
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
