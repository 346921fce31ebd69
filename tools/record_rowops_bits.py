"""Record the bits of the Adam and mixture-NLL entries (csrc/rowops.hip) as a build of one commit gives them on the device.

    PLANK_HIP_LIB=<that build>/libplank_hip.so python tools/record_rowops_bits.py --commit <hash> [--out tests/golden/rowops_family_bits.json]

Per case of tests/rowops_parity.py's adam_cases() and nll_cases(): the sha256 of every input buffer and of every output buffer of every
entry and configuration tests/rowops_family_bits.py runs.  The file also names the commit the library was built from and the compiler.
tests/test_rowops_family_bits_gpu.py holds later trees to this record, so it is taken ONCE, from the parent of a change that folds
kernels together, and not refreshed from the tree under test."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch                                                        # noqa: E402

import rowops_family_bits as fb                                     # noqa: E402
from plankassembly_amd import _lib as L                             # noqa: E402
from plankassembly_amd.build import _hipcc                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit", required=True, help="the commit the loaded library was built from")
ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "rowops_family_bits.json"))
args = ap.parse_args()

try:
    hipcc = subprocess.run([_hipcc(), "--version"], capture_output=True, text=True, check=True).stdout.strip()
except (OSError, subprocess.CalledProcessError, RuntimeError) as e:
    hipcc = f"unknown ({e})"
record = dict(commit=args.commit, hipcc_version=hipcc, device=torch.cuda.get_device_name(0), library=os.path.basename(L.LIB_PATH),
              adam=fb.adam_records(), nll=fb.nll_records())
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(record['adam'])} Adam cases, {len(record['nll'])} NLL cases, "
      f"{sum(len(o) for r in record['adam'] + record['nll'] for o in r['outputs'].values())} output hashes -> {args.out}")
