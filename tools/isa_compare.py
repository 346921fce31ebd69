"""Device code of two versions of one HIP source, kernel by kernel, without a GPU (the method of profiles/decode_refactor_isa.txt,
profiles/gemm_dispatch_refactor.txt and profiles/attn_dispatch_refactor.txt, section 1).

    python tools/isa_compare.py BEFORE.hip AFTER.hip        (each next to the headers it includes)

Both are compiled with the project's flags plus `--cuda-device-only -S`; kernels are matched by mangled name.  The instruction stream
of a kernel is everything between its label and its last s_endpgm with comments, blank lines and .loc / .cfi / .p2align / .file
directives dropped and the function number of local labels (.LBB<n>_<m>, .Ltmp<n>) masked.  Register and memory figures are the
kernel's metadata: .vgpr_count / .agpr_count / .sgpr_count / private_segment_fixed_size (scratch) / group_segment_fixed_size (LDS).
`--diff NAME` prints the first differing lines of one kernel, `--order` the order in which each version emits its kernels (hipcc's
register numbering can follow it)."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plankassembly_amd.build import FLAGS, _hipcc


def assembly(src):
    out = os.path.join(tempfile.mkdtemp(), "k.s")
    subprocess.run([_hipcc(), *FLAGS, "--cuda-device-only", "-S", "-x", "hip", os.path.abspath(src), "-o", out], check=True,
                   cwd=os.path.dirname(os.path.abspath(src)), stderr=subprocess.DEVNULL)
    return open(out).read()


def parse(txt):
    """-> (kernel names in emission order, {name: figures}, {name: instruction stream})"""
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M)
    figures = {}
    for m in re.finditer(r"- \.agpr_count:\s*(\d+).*?(?=\n  - \.agpr_count|\namdhsa\.target|\Z)", txt, re.S):
        field = lambda k: int(re.search(r"\." + k + r":\s*(\d+)", m.group(0)).group(1))
        figures[re.search(r"\.name:\s*(\S+)", m.group(0)).group(1)] = tuple(
            field(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"))
    lines = txt.split("\n")
    label = {ln.split(":")[0]: i for i, ln in enumerate(lines) if ln.startswith("_Z") and ":" in ln}
    streams = {}
    for k in kernels:
        body, end = [], None
        for ln in lines[label[k] + 1:]:
            if ln.startswith(("\t.section", ".Lfunc_end")):
                break
            s = ln.split(";")[0].strip()
            if not s or s.startswith((".loc", ".cfi", ".p2align", ".file")):
                continue
            body.append(re.sub(r"\.Ltmp\d+", ".Ltmpn", re.sub(r"\.LBB\d+_", ".LBBn_", s)))
            if s.startswith("s_endpgm"):
                end = len(body)
        streams[k] = body[:end]
    return kernels, figures, streams


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    (kb, fb, sb), (ka, fa, sa) = parse(assembly(args[0])), parse(assembly(args[1]))
    names = sorted(set(kb) | set(ka))
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = {k: re.sub(r"^void |\(anonymous namespace\)::", "", d).rsplit("(", 1)[0].replace("__hip_bfloat16", "bf16") for k, d in zip(names, dem)}
    print(f"before: {len(kb)} kernels    after: {len(ka)} kernels")
    print("gone:", ", ".join(short[k] for k in kb if k not in ka) or "none")
    print("new:", ", ".join(short[k] for k in ka if k not in kb) or "none")
    both = [k for k in ka if k in kb]
    same = {k: sb[k] == sa[k] and fb[k] == fa[k] for k in both}
    print(f"identical instruction streams AND identical figures: {sum(same.values())} of {len(both)}")
    fmt = lambda f: "%3d /%3d /%3d /%4d /%6d" % f
    print(f"{'kernel':<50} before VGPR/AGPR/SGPR/scratch/LDS   after VGPR/AGPR/SGPR/scratch/LDS   instr. before after")
    for k in both:
        print(f"{short[k]:<50} {fmt(fb[k])}   {fmt(fa[k])}   {len(sb[k]):>6} {len(sa[k]):>6}  {'same' if same[k] else 'DIFFERENT'}")
    if "--order" in sys.argv:
        for tag, ks in (("before", kb), ("after", ka)):
            print(f"emission order {tag}:\n  " + "\n  ".join(short[k] for k in ks))
    if "--diff" in sys.argv:
        k = next(k for k in both if short[k] == sys.argv[sys.argv.index("--diff") + 1])
        print("\n".join(list(difflib.unified_diff(sb[k], sa[k], lineterm="", n=2))[:80]))


if __name__ == "__main__":
    main()
