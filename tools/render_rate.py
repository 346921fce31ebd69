"""What rendering the drawing from the planks costs, at the complete config's row: B 64, MAX_INPUT_LENGTH 1200
(S 1199, 299 lines to a row), MAX_OUTPUT_LENGTH 128.

`--drawings N` (default 256) generated drawings of 4-12 planks (tests/render_reference.py `generated`: random boxes on a coarse lattice
that cross as often as boxes can - their line counts are NOT the dataset's):
  1. host `render_drawing` ms per drawing, one thread (no GPU needed: `--host-only`);
  2. one rendering `DeviceDrawings.batch()` (`pa_render_drawings`) between HIP events on an idle stream, augmentation off and on
     (AUG_RATIO 1 so that every row is augmented: the worst case);
  3. in the same session `pa_tokenise_drawings` on the same drawings' host-rendered lines, stored in the info files;
  4. `--step-ms X`: the complete train step of the same session (`python bench.py --gpus 1 --config complete --batch 64`, its step time)
     to report the ratio launch / step against; below 1 the loader's stream never holds the step back.
`python tools/render_rate.py --out profiles/render_time.txt [--step-ms X]`"""
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
import render_reference as RR
from plankassembly_amd import datasets as D

TOKEN = types.SimpleNamespace(END=512, PAD=513)
BATCH, MAX_INPUT_LENGTH, MAX_OUTPUT_LENGTH = 64, 1200, 128


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

    planks = [RR.generated(5000 + i, 4 + i % 9) for i in range(args.drawings)]

    # ---- 1. the host
    t0 = time.perf_counter()
    drawn = [D.render_drawing(b / 1000.0) for b in planks]
    dt = time.perf_counter() - t0
    lines = np.array([len(r[0]) for r in drawn])
    hidden = np.array([int(r[2].sum()) for r in drawn])
    say(f"rendering from the planks: {args.drawings} generated drawings of 4-12 planks besides plank 0 (random, maximally crossing boxes - "
        f"not the dataset's line counts), {lines.min()}-{lines.max()} lines (median {int(np.median(lines))}), {hidden.min()}-{hidden.max()} "
        f"of them hidden (median {int(np.median(hidden))}), B {BATCH}, MAX_INPUT_LENGTH {MAX_INPUT_LENGTH}")
    say(f"\n1. host render_drawing, one thread: {dt / len(planks) * 1e3:.2f} ms / drawing")
    if args.host_only:
        say("\n2.-4. not measured (--host-only)")
        return

    import torch
    from plankassembly_amd.device_data import DeviceDrawings, pack_infos
    tmp = tempfile.mkdtemp(prefix="render_rate_")
    say(f"   {torch.cuda.get_device_name(0)}")
    cfg = R.make_data_cfg(MAX_INPUT_LENGTH, MAX_OUTPUT_LENGTH, 1.0, 0.15, 0.02)
    room = (MAX_INPUT_LENGTH - 2) // 4
    keep = [i for i in range(len(planks)) if lines[i] <= room]
    if len(keep) < len(planks):
        say(f"   {len(planks) - len(keep)} drawings have more than the row's {room} lines and are left out (the host refuses them)")
    pfiles = R.write_infos(os.path.join(tmp, "planks"), [RR.plank_info(f"d{i:05d}", planks[i]) for i in keep])
    t0 = time.perf_counter()
    packed = pack_infos(os.path.join(tmp, "planks"), pfiles, "line", render=True, data_cfg=cfg)
    say(f"   pack_infos(render=True): {time.perf_counter() - t0:.1f} s once")
    stored = [D.render_info(f"d{i:05d}", planks[i] / 1000.0, np.full(planks[i].shape, -1)) for i in keep]
    sfiles = R.write_infos(os.path.join(tmp, "lines"), stored)
    sets = {"render": DeviceDrawings(packed, TOKEN, cfg, "cuda"),
            "stored": DeviceDrawings(pack_infos(os.path.join(tmp, "lines"), sfiles, "line"), TOKEN, cfg, "cuda")}

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

    say("\n2. pa_render_drawings, one launch of 64 drawings between HIP events (median / min / max of 40 batches)")
    results = {}
    for aug in (False, True):
        results[aug] = launch_us(sets["render"], aug)
        say(f"   augmentation {str(aug):5}: {results[aug][0]:8.1f} / {results[aug][1]:8.1f} / {results[aug][2]:8.1f} us")
    say("\n3. pa_tokenise_drawings on the same drawings' stored host-rendered lines")
    for aug in (False, True):
        base = launch_us(sets["stored"], aug)
        say(f"   augmentation {str(aug):5}: {base[0]:8.1f} / {base[1]:8.1f} / {base[2]:8.1f} us; rendering / stored = "
            f"{results[aug][0] / base[0]:.1f}")
    if args.step_ms:
        say(f"\n4. complete train step of this session: {args.step_ms:.3f} ms at B {BATCH}; launch / step = "
            f"{results[False][0] / 1e3 / args.step_ms:.3f} (clean), {results[True][0] / 1e3 / args.step_ms:.3f} (every row augmented)")
    else:
        say("\n4. train step: not measured (pass --step-ms from `python bench.py --gpus 1 --config complete --batch 64`)")
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
