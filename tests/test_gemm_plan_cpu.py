"""The GEMM dispatch rule ("which kernel, which grid") pinned without a GPU, through pa_gemm_plan - the dry run of pa_gemm /
pa_gemm_norm_a (include/plank_hip.h).  The expected status and kernel family of every case under every switch setting are in
tests/golden/gemm_plan.json; they were recorded from the library of the commit BEFORE plan_gemm existed (pa_gemm_record + pa_gemm on
a machine without a device: the family is recorded before the launch fails; rejected blocks return their PA_E* code), so this file
holds the refactored selection function to the rule the hand-grown dispatch had.  pa_gemm_norm_a recorded no family there: its
accepted cases are pinned as accepted, its family on the GPU (test_kernels_gpu.py).

The switches are read once per process, so every setting runs in a child process (this file run as a script) that prints one JSON
line; the parent process asserts.
"""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "gemm_plan.json")

PA_F32, PA_BF16 = 0, 1
KINDS = ["PAIR", "RING", "WIDE", "SMALL", "SKINNY", "BIG"]          # PA_GEMM_KIND_* by value
# one character per case: the family's number, or the rejection; 'o': accepted, family not pinned (pa_gemm_norm_a)
CODE_OF_STATUS = {-1: "I", -2: "A", -3: "S"}

MS = [2, 37, 250, 256, 512, 513, 2048, 2049, 4096, 7940, 8192, 8300, 8704, 9736, 12288, 16385]
NS = [96, 384, 512, 514, 1024, 1100, 1536, 2048]
KS = [64, 512, 520, 1024, 2048]
DTYPES = [PA_BF16, PA_F32]
LAYOUTS = [(1, 1), (1, 0), (0, 1), (0, 0)]                          # (a_kcontig, b_kcontig)
SPLITKS = [1, 4]
BATCHES = [1, 8]
EPILOGUES = ["none", "residual", "aux", "dropout", "C_lp"]
ALIGNMENTS = [0, 1]                                                 # 1: A two bytes off a 16-byte boundary
N_SAMPLED = 1200

SETTINGS = {
    "default": {},
    "TALL=1": {"PA_GEMM_TALL": "1"},
    "BIG=1": {"PA_GEMM_BIG": "1"},
    "BIG=2": {"PA_GEMM_BIG": "2"},
    "WIDE=0": {"PA_GEMM_WIDE": "0"},
    "WIDE=1": {"PA_GEMM_WIDE": "1"},
    "SKINNY=0": {"PA_GEMM_SKINNY": "0"},
    "SKINNY=1": {"PA_GEMM_SKINNY": "1"},
    "V3=0": {"PA_GEMM_V3": "0"},
    "V3=2": {"PA_GEMM_V3": "2"},
    "SMALL=0": {"PA_GEMM_SMALL": "0"},
    "RESERVE_CUS=32": {"PA_RESERVE_CUS": "32"},
}


def cases():
    """The case list, in a fixed order.  ("gemm", M, N, K, dtype, a_kcontig, b_kcontig, splitk, batch, epilogue, misaligned) and
    ("norm", M, N, K, dtype, y, zf, y_f32).  The whole cross product of the pa_gemm dimensions is 204 800 blocks; pinned are
      - every (M, N, K, dtype) as a plain Linear (both operands k-contiguous, no split, one batch, no epilogue, aligned): 1 280,
      - N_SAMPLED blocks drawn from the whole product by a fixed linear congruential sequence (invalid combinations stay in),
      - every pa_gemm_norm_a form: 320."""
    out = [("gemm", M, N, K, dt, 1, 1, 1, 1, "none", 0) for dt, M, N, K in itertools.product(DTYPES, MS, NS, KS)]
    dims = [MS, NS, KS, DTYPES, LAYOUTS, SPLITKS, BATCHES, EPILOGUES, ALIGNMENTS]
    x = 12345
    for _ in range(N_SAMPLED):
        pick = []
        for d in dims:
            x = (x * 1103515245 + 12345) % (1 << 31)
            pick.append(d[(x >> 8) % len(d)])
        M, N, K, dt, (akc, bkc), sk, nb, epi, mis = pick
        out.append(("gemm", M, N, K, dt, akc, bkc, sk, nb, epi, mis))
    for dt, M, N, K, y, zf, yf in itertools.product(DTYPES, [37, 256, 512, 513, 4096], [512, 1536], [512, 1024], [0, 1], [0, 1], [0, 1]):
        out.append(("norm", M, N, K, dt, y, zf, yf))
    return out


# made-up operand addresses: 16-byte aligned, never dereferenced by the dry run
ADDR = {k: 0x10000000 * (i + 1) for i, k in enumerate(["A", "B", "C", "bias", "R", "aux", "ws", "C_lp", "u", "gamma", "beta", "y", "zf"])}


def gemm_args(L, case):
    """The pa_gemm_args block (and the pa_gemm_norm_ext, or None) of a case."""
    g = L.GemmArgs()
    if case[0] == "gemm":
        _, M, N, K, dt, akc, bkc, sk, nb, epi, mis = case
        out_dt = PA_F32 if epi == "C_lp" else dt
    else:
        _, M, N, K, dt, y, zf, yf = case
        akc = bkc = sk = nb = 1
        epi, mis = "none", 0
        out_dt = PA_F32 if (dt == PA_F32 or yf) else dt             # (the f32 residual stream keeps its outputs in f32)
    g.A, g.B, g.C = ADDR["A"] + 2 * mis, ADDR["B"], ADDR["C"]
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = (K if akc else M), (K if bkc else N), N
    g.batch, g.sA, g.sB, g.sC = nb, M * K, N * K, M * N
    g.a_kcontig, g.b_kcontig = akc, bkc
    g.in_dtype, g.out_dtype = dt, out_dt
    g.alpha, g.aux_scale, g.splitk = 1.0, 1.0, sk
    if sk > 1:
        g.ws = ADDR["ws"]
    if epi == "residual":
        g.R, g.ldr, g.sR = ADDR["R"], N, M * N
    elif epi == "aux":
        g.aux, g.ldaux, g.sAux = ADDR["aux"], N, M * N
    elif epi == "dropout":
        g.drop_p, g.drop_seed = 0.1, 7
    elif epi == "C_lp":
        g.C_lp, g.ldc_lp = ADDR["C_lp"], N
    if case[0] == "gemm":
        return g, None
    g.bias = ADDR["bias"]
    x = L.GemmNormExt()
    x.u, x.eps = ADDR["u"], 1e-5
    if y:
        x.gamma, x.beta, x.y, x.ldy = ADDR["gamma"], ADDR["beta"], ADDR["y"], K
    if zf:
        x.zf, x.ldzf = ADDR["zf"], K
    x.y_f32 = yf
    return g, x


def child():
    """Plan every case under this process's environment; one JSON line: [[code, grid, block, units, splitk, effective], ...]."""
    sys.path.insert(0, REPO)
    lib_path = os.path.join(REPO, "plankassembly_amd", "libplank_hip.so")
    if not os.path.exists(lib_path):
        from plankassembly_amd.build import build
        build()
    from plankassembly_amd import _lib as L
    lib = L.lib()
    rows = []
    for case in cases():
        g, x = gemm_args(L, case)
        info = L.GemmPlanInfo()
        rc = lib.pa_gemm_plan(C.byref(g), C.byref(x) if x is not None else None, C.byref(info))
        if rc:
            rows.append([CODE_OF_STATUS[rc], 0, 0, 0, 0, 0])
        else:
            eff = lib.pa_gemm_effective_splitk(g.K, g.in_dtype, g.splitk)
            rows.append([str(info.kind), info.grid, info.block, info.units, info.splitk, eff])
    print(json.dumps(rows))


_RUNS = {}


def plan_under(setting):
    if setting not in _RUNS:
        env = {k: v for k, v in os.environ.items() if not k.startswith(("PA_GEMM_", "PA_RESERVE_CUS", "PLANK_HIP_LIB"))}
        env.update(SETTINGS[setting])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        _RUNS[setting] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("[")][-1])
    return _RUNS[setting]


def test_case_list_matches_the_golden_file():
    gold = json.load(open(GOLDEN))
    cs = cases()
    assert gold["cases"] == len(cs) and len(set(cs)) > 2400
    assert sorted(gold["codes"]) == sorted(SETTINGS)
    for name, codes in gold["codes"].items():
        assert len(codes) == len(cs), name
    assert os.path.getsize(GOLDEN) < 64 * 1024


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_status_and_family_of_every_case(setting):
    gold = json.load(open(GOLDEN))["codes"][setting]
    rows = plan_under(setting)
    cs = cases()
    assert len(rows) == len(cs) == len(gold)
    wrong = []
    for case, row, want in zip(cs, rows, gold):
        got = "o" if (case[0] == "norm" and row[0] in "012345") else row[0]
        if got != want:
            wrong.append((case, got, want))
    assert not wrong, f"{len(wrong)} of {len(cs)} cases differ from the recorded dispatch, first: {wrong[:8]}"


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_grid_block_and_split_of_every_accepted_case(setting):
    cus = 256 - int(SETTINGS[setting].get("PA_RESERVE_CUS", 0))
    n_ok = 0
    for case, (code, grid, block, units, splitk, eff) in zip(cases(), plan_under(setting)):
        if code not in "012345":
            continue
        n_ok += 1
        fam = KINDS[int(code)]
        assert 1 <= grid <= units, (case, grid, units)
        assert block == (512 if fam == "BIG" else 256), (case, fam, block)
        assert splitk == eff >= 1, (case, splitk, eff)
        if fam in ("RING", "WIDE", "BIG"):
            assert grid <= cus, (case, fam, grid)               # one block per CU that the launch may use
        if fam == "SMALL":
            assert grid <= 2 * cus, (case, grid)
        if fam not in ("RING", "PAIR"):
            assert splitk == 1, (case, fam, splitk)             # only the 128 x 128 kernels split the contraction
    assert n_ok > 1000


def test_spot_checks_default_setting():
    """Readable anchors: the model's own shapes, read off the library before the refactor."""
    want = {(256, 512, 512): ("SKINNY", "SKINNY"), (2048, 512, 512): ("SMALL", "SKINNY"), (2048, 1536, 512): ("SMALL", "SKINNY"),
            (2048, 1536, 1024): ("RING", "SKINNY"), (7940, 1024, 512): ("WIDE", "PAIR"), (7940, 1536, 512): ("PAIR", "PAIR"),
            (8704, 512, 512): ("PAIR", "PAIR")}
    got = {}
    for case, row in zip(cases(), plan_under("default")):
        if case[0] == "gemm" and case[5:] == (1, 1, 1, 1, "none", 0) and case[1:4] in want and row[0] in "012345":
            got[(case[1:4], case[4])] = KINDS[int(row[0])]
    for shape, (bf, f32) in want.items():
        assert got[(shape, PA_BF16)] == bf, (shape, "bf16", got[(shape, PA_BF16)])
        assert got[(shape, PA_F32)] == f32, (shape, "f32", got[(shape, PA_F32)])


if __name__ == "__main__":
    child()
