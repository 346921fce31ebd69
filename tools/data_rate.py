"""What feeds the train step: the CPU tokeniser, the DataLoader over it, and the device dataset.

One session on one MI355X, headline config (d_model 512, 6 + 6 layers, MAX_INPUT_LENGTH 1025, MAX_OUTPUT_LENGTH 128, batch 16,
bf16), `--drawings N` (default 4 096) generated info files of 8-255 lines:
  1. `LineDataset.__getitem__` drawings/s in one process at AUG_RATIO 0, 0.1 and 1;
  2. `DataLoader` batches/s at NUM_WORKERS 4 and 16 (AUG_RATIO 0.1);
  3. `DeviceLoader` batches/s alone and the tokenise kernel's time from HIP events, augmentation off and on;
  4. `fit`: the epoch's printed samples/s with the CPU loader (NUM_WORKERS 4) and with DEVICE_DATASET, three epochs each;
  5. the ceiling: `python bench.py --gpus 1`'s `value` (synthetic batches already in HBM).
`python tools/data_rate.py --out profiles/device_data_rate.txt`; every line is written as soon as it is measured."""
import argparse
import contextlib
import io
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch
import yaml

import device_data_reference as R
from plankassembly_amd import datasets as D

TOKEN = types.SimpleNamespace(END=512, PAD=513)
BATCH = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drawings", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-bench", action="store_true")
    args = ap.parse_args()
    sink = open(args.out, "w") if args.out else None

    def say(line=""):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    tmp = tempfile.mkdtemp(prefix="data_rate_")
    root = os.path.join(tmp, "infos")
    rng = np.random.default_rng(2022)
    t0 = time.perf_counter()
    files = R.write_infos(root, [R.random_info(rng, f"d{i:05d}", (8, 255), (2, 21)) for i in range(args.drawings)])
    split = os.path.join(tmp, "all.txt")
    with open(split, "w") as f:
        f.write("\n".join(files))
    say(f"device dataset feed rates: {args.drawings} generated drawings of 8-255 lines, MAX_INPUT_LENGTH 1025, MAX_OUTPUT_LENGTH 128, "
        f"batch {BATCH}; {torch.cuda.get_device_name(0) if torch.cuda.is_available() else 'no GPU'}; {len(os.sched_getaffinity(0))} CPUs visible "
        f"(files written in {time.perf_counter() - t0:.0f} s)")

    def cfg_of(aug):
        return R.make_data_cfg(1025, 128, aug, 0.15, 0.02)

    # ---- 1. the CPU tokeniser, one process
    say("\n1. LineDataset.__getitem__, one process")
    for aug in (0.0, 0.1, 1.0):
        ds = D.LineDataset(root, files, TOKEN, cfg_of(aug), augmentation=aug > 0)
        np.random.seed(1)
        n = min(1024, len(ds))
        t0 = time.perf_counter()
        for i in range(n):
            ds[i]
        dt = time.perf_counter() - t0
        say(f"   AUG_RATIO {aug:<4}: {dt / n * 1e3:6.2f} ms / drawing, {n / dt:8.0f} drawings/s")

    # ---- 2. DataLoader
    say("\n2. DataLoader(LineDataset, batch 16, shuffle, drop_last), AUG_RATIO 0.1, collated CPU batches only")
    for workers in (4, 16):
        ds = D.LineDataset(root, files, TOKEN, cfg_of(0.1), augmentation=True)
        dl = torch.utils.data.DataLoader(ds, batch_size=BATCH, shuffle=True, drop_last=True, num_workers=workers)
        t0 = time.perf_counter()
        nb = sum(1 for _ in dl)
        dt = time.perf_counter() - t0
        say(f"   NUM_WORKERS {workers:2d}: {nb / dt:8.1f} batches/s = {nb * BATCH / dt:8.0f} drawings/s (one epoch of {nb} batches, worker start included)")

    # ---- 3. the device loader alone
    from plankassembly_amd.device_data import DeviceDrawings, DeviceLoader, pack_infos
    say("\n3. DeviceLoader alone")
    t0 = time.perf_counter()
    packed = pack_infos(root, files, "line")
    t_pack = time.perf_counter() - t0
    dd = DeviceDrawings(packed, TOKEN, cfg_of(0.1), "cuda")
    hbm = sum(t.numel() * t.element_size() for t in (dd._line_off, dd._plank_off, dd._box, dd._seg, dd._view, dd._type, dd._coords, dd._attach))
    say(f"   pack_infos: {t_pack:.1f} s once; {hbm / 2**20:.1f} MiB in HBM")
    for aug in (False, True):
        dl = DeviceLoader(dd, BATCH, shuffle=True, drop_last=True, augmentation=aug, seed=1)
        for _ in dl:
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nb = sum(1 for _ in dl)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        idx = torch.arange(BATCH, dtype=torch.int32, device="cuda")
        host = np.arange(BATCH)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
        for a, b in evs:
            dd.batch(idx, 0, aug, host_index=host)              # (warms the allocator: the timed call below reuses these blocks)
            a.record(); dd.batch(idx, 0, aug, host_index=host); b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        say(f"   augmentation {str(aug):5}: {nb / dt:8.0f} batches/s = {nb * BATCH / dt:9.0f} drawings/s (host loop, one epoch of {nb}); "
            f"batch() between HIP events: median {ms[len(ms) // 2] * 1e3:.1f} us, min {ms[0] * 1e3:.1f} us")

    # ---- 4. fit
    say("\n4. trainer fit, headline model, 3 epochs, no validation: the epoch's printed samples/s")
    from plankassembly_amd.trainer import Trainer, run
    with open(os.path.join(REPO, "configs", "train_headline_seq1024.yaml")) as f:
        cfg = yaml.safe_load(f)
    fit = {}
    for device in (False, True):
        cfg["trainer"].update(max_epochs=3, check_val_every_n_epoch=1000, devices=1)
        cfg["model"]["hparams"].update(ROOT=root, DATASETS_TRAIN=split, DATASETS_VALID=split, DATASETS_TEST=split, BATCH_SIZE=BATCH,
                                       NUM_WORKERS=4, DEVICE_DATASET=device)
        path = os.path.join(tmp, f"fit_{int(device)}.yaml")
        with open(path, "w") as f:
            yaml.safe_dump(cfg, f)
        buf = io.StringIO()
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(buf):
                run(Trainer, "fit", path)
        finally:
            os.chdir(cwd)
        rates = [float(x) for x in re.findall(r"([0-9.]+) samples/s", buf.getvalue())]
        fit[device] = rates
        say(f"   DEVICE_DATASET {str(device):5} (NUM_WORKERS 4{' ignored' if device else ''}): " + ", ".join(f"{r:.0f}" for r in rates) + " samples/s per epoch")
        torch.cuda.empty_cache()

    # ---- 5. the ceiling
    ceiling = None
    if not args.no_bench:
        say("\n5. python bench.py --gpus 1 --steps 200 --warmup 20")
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20"],
                           capture_output=True, text=True, cwd=REPO)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode == 0 and lines:
            ceiling = float(json.loads(lines[-1])["value"])
            say(f"   value {ceiling:.0f} samples/s (synthetic batches already in HBM)")
        else:
            say(f"   bench.py failed (exit {r.returncode}): {r.stderr[-400:]}")
    cpu, dev = fit[False][-1], fit[True][-1]
    say(f"\nlast epochs: device-loader fit {dev:.0f} samples/s, CPU-loader fit {cpu:.0f} samples/s: ratio {dev / cpu:.2f}")
    if ceiling:
        say(f"against the synthetic ceiling {ceiling:.0f}: device-loader fit {dev / ceiling:.3f}, CPU-loader fit {cpu / ceiling:.3f}")
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
