#!/usr/bin/env python
"""Per-kernel HBM traffic from two rocprofv3 PMC passes (FETCH_SIZE and WRITE_SIZE cannot share a pass on gfx950).

    rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d gpurun_out/pmc_fetch -o t -- python bench.py ...
    rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d gpurun_out/pmc_write -o t -- python bench.py ...
    python tools/pmc_summary.py gpurun_out/pmc_fetch gpurun_out/pmc_write [out.json]

Both counters are in KiB per dispatch.  MI355X_MICROARCH.md (HBM section) warns that FETCH_SIZE can under-report
wide streaming reads by 2x on gfx950 and tells us to calibrate on a known byte count in the same run: the table
therefore prints torch's f32->bf16 copy kernels of known size first (bytes read = 4 B x elements, written = 2 B x
elements) and the derived correction factors, which are then applied to every kernel."""
import csv
import glob
import json
import os
import re
import sys

KEYS = [  # json key -> regex on the demangled kernel name
    ("gemm_ring_tt", r"gemm3_kernel<true, true, .*GemmP>"),
    ("gemm_ring_nn", r"gemm3_kernel<false, false, .*GemmP>"),
    ("gemm_group_nn", r"gemm3_kernel<false, false, .*GemmGroup>"),
    ("gemm_small_tt", r"gemm3s_kernel"),
    ("gemm_wide_tt", r"gemm3w_kernel"),
    ("dec_attn", r"dec_attn_kernel"),
    ("dec_cross_mq", r"dec_cross_mq_kernel"),
    ("dec_cross_mq32", r"dec_cross_mq32(w8)?_kernel"),
    ("dec_sample", r"dec_sample_kernel"),
    # (rocprofv3's demangler leaves names with the __bf16 template argument mangled)
    ("gemm_pair_tt", r"gemm_kernel<__bf16, 64, 2, true, true, true, true, false, 2>|gemm_kernelIDF16bLi64ELi2ELb1ELb1ELb1ELb1ELb0ELi2E"),
    ("gemm_pair_nn", r"gemm_kernel<__bf16, 64, 2, false, false, true, true, true, 2>|gemm_kernelIDF16bLi64ELi2ELb0ELb0ELb1ELb1ELb1ELi2E"),
    ("attn_fwd", r"attn_fwd_bf16_kernel<64|attn4_fwd_kernel"),
    ("attn_bwd_dq", r"attn_bwd_dq_bf16_kernel<64|attn4_bwd_dq_kernel"),
    ("attn_bwd_dkv", r"attn_bwd_dkv_bf16_kernel<64|attn4_bwd_dkv_kernel"),
    ("layernorm_bwd", r"layernorm_bwd_kernel<__bf16"),
    ("layernorm_fwd", r"layernorm_fwd_kernel<__bf16"),
    ("splitk_reduce", r"splitk_reduce_kernel"),
    ("splitk_reduce_many", r"splitk_reduce_many_kernel"),
    ("adam", r"adam_ext_kernel"),
]


def load(d, counter):
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] != counter:
                continue
            a = out.setdefault(r["Kernel_Name"], [0, 0.0, 0])
            a[0] += 1
            a[1] += float(r["Counter_Value"]) * 1024.0
            a[2] = int(r["Grid_Size"])
    return out


def main():
    fetch, write = load(sys.argv[1], "FETCH_SIZE"), load(sys.argv[2], "WRITE_SIZE")
    # calibration on a kernel of KNOWN traffic in the same run: the library's own flat f32 -> bf16 cast of the parameter
    # buffer (cast_kernel<bf16, float>, one launch when the model's shadow is first built: reads 4 B and writes 2 B per
    # element) or torch's vectorised f32 -> bf16 copy.  MI355X_MICROARCH.md (HBM): on gfx950 FETCH_SIZE reports half the
    # bytes of a wide coalesced streaming read - the factor measured here is applied to every kernel's FETCH below
    # (`fetch_bytes_corrected`), the raw numbers are kept next to it.
    cf = None
    fcorr = wcorr = 1.0
    # PMC_FETCH_FACTOR: a run without a calibration kernel (the exact-f32 decode never casts parameters) takes the factor measured by
    # the same script on the same box in the pass next to it
    if os.environ.get("PMC_FETCH_FACTOR"):
        fcorr = float(os.environ["PMC_FETCH_FACTOR"])
        print(f"# no calibration kernel in this run: FETCH correction factor {fcorr:.3f} taken from PMC_FETCH_FACTOR (measured in the bf16 pass of the same session)")
    for name, (n, tot, grid) in fetch.items():
        is_cast = "cast_kernel" in name
        is_torch = "bfloat16_copy_kernel_cuda" in name and "lambda(float)" in name
        if (is_cast or is_torch) and tot / n > 8e6:
            w = write.get(name)
            if w:
                rd, wr = tot / n, w[1] / w[0]
                print(f"# calibration kernel ({'cast_kernel' if is_cast else 'torch f32->bf16 copy'}): FETCH {rd / 1e6:.2f} MB, "
                      f"WRITE {wr / 1e6:.2f} MB per launch; ideal read/write ratio 2.0, measured {rd / wr:.3f}")
                cf = (rd, wr)
                if rd / wr < 1.5:                                    # the documented under-count: reads tallied at half
                    fcorr = 2.0 * wr / rd if rd > 0 else 2.0
                    fcorr = min(max(fcorr, 1.0), 2.2)
                print(f"# FETCH correction factor applied below: {fcorr:.3f} (WRITE taken as is)")
            break
    res = {}
    print(f"{'kernel':16s} {'launches':>9s} {'fetch_MB':>10s} {'write_MB':>10s} {'hbm_MB/launch':>14s}")
    for key, rx in KEYS:
        fs = [(n, t) for name, (n, t, g) in fetch.items() if re.search(rx, name)]
        ws = [(n, t) for name, (n, t, g) in write.items() if re.search(rx, name)]
        if not fs or not ws:
            continue
        nf, tf = sum(a for a, _ in fs), sum(b for _, b in fs)
        nw, tw = sum(a for a, _ in ws), sum(b for _, b in ws)
        f1, w1 = tf / nf, tw / nw
        res[key] = dict(launches=nf, fetch_bytes_per_launch=f1, write_bytes_per_launch=w1, fetch_bytes_corrected=f1 * fcorr,
                        hbm_bytes_per_launch=f1 * fcorr + w1, hbm_bytes_per_launch_raw=f1 + w1)
        print(f"{key:16s} {nf:9d} {f1 / 1e6:10.3f} {w1 / 1e6:10.3f} {(f1 * fcorr + w1) / 1e6:14.3f}   (raw {(f1 + w1) / 1e6:.3f})")
    # bench.py's attention families are forward / backward (dQ + dK,dV together): per-launch bytes of a family member
    for fam, keys in (("attn_enc_self_fwd", ["attn_fwd"]), ("attn_enc_self_bwd", ["attn_bwd_dq", "attn_bwd_dkv"])):
        if all(k in res for k in keys):
            res[fam] = dict(launches=sum(res[k]["launches"] for k in keys),
                            hbm_bytes_per_launch=sum(res[k]["hbm_bytes_per_launch"] * res[k]["launches"] for k in keys) /
                            sum(res[k]["launches"] for k in keys),
                            note="mean over ALL attention launches of these kernels in the step (self, cross and causal)")
    if len(sys.argv) > 3:
        json.dump(dict(source="rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes), KiB x 1024, per-launch mean",
                       calibration=dict(copy_fetch_bytes=cf[0], copy_write_bytes=cf[1]) if cf else None, kernels=res),
                  open(sys.argv[3], "w"), indent=1)


if __name__ == "__main__":
    main()
