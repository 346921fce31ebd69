"""The attention dispatch rule ("which kernels, which grids, which AttnP") pinned without a GPU, through pa_attn_plan - the dry run of
pa_attn_fwd / pa_attn_bwd (include/plank_hip.h).  tests/golden/attn_plan.json holds, for every case under every switch setting, the
status or the launches (kernel, grid, block, LDS bytes, extra argument, in order) and the five AttnP fields the dispatch decides.

How the golden file was made: from the commit BEFORE plan_attn existed, not from the code under test.  In a scratch copy of that
commit's csrc/attention.hip, PA_LAUNCH was redefined to append (the stringified kernel expression, the enclosing function's
__PRETTY_FUNCTION__, grid, block, lds, extra argument or 0) to a thread-local list and to keep the AttnP it was given, set_lds was
made to return 0 (no device to take the attribute), and one export returned and cleared the list.  That library, built with the
project's flags, ran pa_attn_fwd / pa_attn_bwd on cases() of this file under every entry of SETTINGS.  Kernel names are the recorded
expressions with the parentheses stripped, whitespace normalised, and the two template parameters the old launchers left symbolic
(`T`, `DH`) replaced by their values from the recorded __PRETTY_FUNCTION__.

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
GOLDEN = os.path.join(REPO, "tests", "golden", "attn_plan.json")

PA_F32, PA_BF16 = 0, 1
CODE_OF_STATUS = {-1: "I", -2: "A", -3: "S"}

DTYPES = [PA_F32, PA_BF16]
DHS = [16, 32, 64, 48]
BS = [1, 2, 16, 64, 65]
HS = [2, 8]
LS = [(36, 36), (128, 128), (128, 300), (128, 1199), (129, 300), (300, 300), (1024, 1024), (2049, 2049)]
DROPS = [0.0, 1e-11, 0.2, 1.0]
# dense; packed self-attention (cu_q == cu_k, with order); the same with scratch of pa_attn_ws_bytes size / of 1 KiB / 16 bytes off its
# alignment; packed keys only
LAYOUTS = ["dense", "self", "self_ws", "self_ws1k", "self_ws_mis", "keys"]
# misaligned q; ldk no multiple of the vector width; no dout (a defect of a backward call only).  "none" five times: most sampled
# cases should get as far as the selection rule
DEFECTS = ["none"] * 5 + ["q_mis", "ldk", "no_dout"]
N_SAMPLED = 700

SETTINGS = {
    "default": {},
    "V4=0": {"PA_ATTN_V4": "0"},
    "V4=2": {"PA_ATTN_V4": "2"},
    "V5=0": {"PA_ATTN_V5": "0"},
    "V5=2": {"PA_ATTN_V5": "2"},
    "V5_OCC=2": {"PA_ATTN_V5_OCC": "2"},
    "KSPLIT=0": {"PA_ATTN_KSPLIT": "0"},
    "KSPLIT=2": {"PA_ATTN_KSPLIT": "2"},
    "KSPLIT_MIN=2,MIN2=6": {"PA_ATTN_KSPLIT_MIN": "2", "PA_ATTN_KSPLIT_MIN2": "6"},
    "BWD_MERGE=0,X3_DKV_OCC=2": {"PA_ATTN_BWD_MERGE": "0", "PA_X3_DKV_OCC": "2"},
    "BWD_MERGE_MAX=256": {"PA_ATTN_BWD_MERGE_MAX": "256"},
    "OCC=43,V4=0": {"PA_ATTN_OCC": "43", "PA_ATTN_V4": "0"},
    "BALANCED=0": {"PA_ATTN_BALANCED": "0"},
    "SPLIT=1": {"PA_ATTN_SPLIT": "1"},
    "SPLIT=1,KMAX=4,PMAX=4": {"PA_ATTN_SPLIT": "1", "PA_ATTN_SPLIT_KMAX": "4", "PA_ATTN_SPLIT_PMAX": "4"},
    "SPLIT=1,KMAX=0,PMAX=9": {"PA_ATTN_SPLIT": "1", "PA_ATTN_SPLIT_KMAX": "0", "PA_ATTN_SPLIT_PMAX": "9"},     # (the clamps: 1, 8)
    "X3_PARTS=2,PARTS_MIN=128": {"PA_X3_PARTS": "2", "PA_X3_PARTS_MIN": "128"},
}

# (dtype, dh, B, H, (Lq, Lk), kpm, causal, drop_p, layout, bwd, x3, defect); the model's own launches, looked up by the anchors test
ENCODER_SELF = (PA_BF16, 64, 16, 8, (1024, 1024), 0, 0, 0.2, "self", 0, 0, "none")
DECODER_CROSS = (PA_BF16, 64, 16, 8, (128, 1199), 0, 0, 0.2, "keys", 0, 0, "none")
DECODER_CAUSAL = (PA_BF16, 64, 16, 8, (128, 128), 1, 1, 0.2, "dense", 0, 0, "none")


def _bwd(case):
    return case[:9] + (1,) + case[10:]


def cases():
    """The case list, in a fixed order.  The whole cross product is 1.5 million argument blocks; pinned are
      - every (dtype, dh 16 / 32 / 64, L pair, causal, direction) as a plain dense launch of B 2 x H 8: 192,
      - the bf16x3 mode on f32 dh 64: every (L pair, drop 0 / 0.2, direction): 32,
      - every packed layout of bf16 dh 64 x H 8 on the self-attention L pairs, B 16 / 64 / 65, both directions: 90,
      - the model's three attention launches, both directions: 6,
      - N_SAMPLED blocks drawn from the whole product by a fixed linear congruential sequence (invalid combinations stay in)."""
    out = [(dt, dh, 2, 8, L, 0, ca, 0.0, "dense", bw, 0, "none") for dt, dh, L, ca, bw in itertools.product(DTYPES, [16, 32, 64], LS, [0, 1], [0, 1])]
    out += [(PA_F32, 64, 2, 8, L, 0, 0, dp, "dense", bw, 1, "none") for L, dp, bw in itertools.product(LS, [0.0, 0.2], [0, 1])]
    out += [(PA_BF16, 64, B, 8, L, 0, 0, 0.0, lay, bw, 0, "none")
            for lay, B, L, bw in itertools.product(LAYOUTS[1:], [16, 64, 65], [(300, 300), (1024, 1024), (2049, 2049)], [0, 1])]
    for c in (ENCODER_SELF, DECODER_CROSS, DECODER_CAUSAL):
        out += [c, _bwd(c)]
    dims = [DTYPES, DHS, BS, HS, LS, [0, 1], [0, 1], DROPS, LAYOUTS, [0, 1], [0, 1], DEFECTS]
    x = 12345
    for _ in range(N_SAMPLED):
        pick = []
        for d in dims:
            x = (x * 1103515245 + 12345) % (1 << 31)
            pick.append(d[(x >> 8) % len(d)])
        out.append(tuple(pick))
    return out


# made-up operand addresses: 256-byte aligned, never dereferenced by the dry run
ADDR = {k: 0x10000000 * (i + 1) for i, k in enumerate(
    ["q", "k", "v", "o", "lse", "kpm", "dout", "dq", "dk", "dv", "delta", "cu", "order", "ws"])}


def attn_args(L, lib, case):
    """The pa_attn_args block of a case (lib: for pa_attn_ws_bytes, which sizes the scratch of the "self_ws" layouts)."""
    dt, dh, B, H, (Lq, Lk), kpm, causal, drop_p, layout, bwd, x3, defect = case
    a = L.AttnArgs()
    for f in ("q", "k", "v", "o", "lse", "dout", "dq", "dk", "dv", "delta"):
        setattr(a, f, ADDR[f])
    a.B, a.H, a.Lq, a.Lk, a.dh = B, H, Lq, Lk, dh
    a.ldq = a.ldk = a.ldv = a.ldo = a.lddo = a.lddq = a.lddk = a.lddv = H * dh
    a.causal, a.scale, a.drop_p, a.drop_seed, a.dtype = causal, dh ** -0.5, drop_p, 7, dt
    if kpm:
        a.kpm = ADDR["kpm"]
    if layout == "keys":
        a.cu_k = ADDR["cu"]
    elif layout != "dense":
        a.cu_q = a.cu_k = ADDR["cu"]
        a.order = ADDR["order"]
        if layout != "self":
            a.ws = ADDR["ws"] + (16 if layout == "self_ws_mis" else 0)
            a.ws_bytes = 1024 if layout == "self_ws1k" else lib.pa_attn_ws_bytes(B * Lq, B, H, Lq)
    if defect == "q_mis":
        a.q = ADDR["q"] + 4
    elif defect == "ldk":
        a.ldk = H * dh + 2
    elif defect == "no_dout":
        a.dout = None
    return a


def child(plan_case=None):
    """Plan every case under this process's environment; one JSON line: {"rows": [status letter, or
    [[kernel, gx, gy, gz, block, lds, extra], ..., [balanced, ks_min, parts_q, parts_kv, sp_slots]], ...], "ws": the largest answer
    of pa_attn_ws_bytes over the cases' shapes}.  plan_case(L, lib, args, bwd) -> row: how a case is planned (the recording of the
    golden file put the instrumented library of the earlier commit here)."""
    sys.path.insert(0, REPO)
    from plankassembly_amd import _lib as L
    lib = L.lib()

    def dry_run(L, lib, a, bwd):
        info = L.AttnPlanInfo()
        rc = lib.pa_attn_plan(C.byref(a), bwd, C.byref(info))
        if rc:
            return CODE_OF_STATUS[rc]
        row = [[ln.kernel.decode(), *ln.grid, ln.block, ln.lds_bytes, ln.extra] for ln in info.launch[:info.n_launches]]
        return row + [[info.balanced, info.ks_min, info.parts_q, info.parts_kv, info.sp_slots]]

    rows, ws = [], 0
    for case in cases():
        a = attn_args(L, lib, case)
        ws = max(ws, lib.pa_attn_ws_bytes(case[2] * case[4][0], case[2], case[3], case[4][0]))
        L.check(lib.pa_attn_split_config(case[10]), "pa_attn_split_config")
        rows.append((plan_case or dry_run)(L, lib, a, case[9]))
        L.check(lib.pa_attn_split_config(0), "pa_attn_split_config")
    print(json.dumps({"rows": rows, "ws": ws}))


_RUNS = {}


def plan_under(setting):
    if not _RUNS:                                               # all children at once: short single-threaded processes
        if not os.path.exists(os.path.join(REPO, "plankassembly_amd", "libplank_hip.so")):
            sys.path.insert(0, REPO)
            from plankassembly_amd.build import build
            build()
        procs = {}
        for s, switches in SETTINGS.items():
            env = {k: v for k, v in os.environ.items() if not k.startswith(("PA_ATTN_", "PA_X3_", "PLANK_HIP_LIB"))}
            env.update(switches, OMP_NUM_THREADS="1")
            procs[s] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], cwd=REPO, env=env, stdout=subprocess.PIPE,
                                        stderr=subprocess.PIPE, text=True)
        for s, pr in procs.items():
            out, err = pr.communicate(timeout=600)
            _RUNS[s] = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1]) if pr.returncode == 0 else err[-4000:]
    assert isinstance(_RUNS[setting], dict), _RUNS[setting]
    return _RUNS[setting]


def golden_rows(gold, setting):
    """Decode the golden file's compact form: "launches" are unique [name index, gx, gy, gz, block, lds, extra], "outcomes" unique
    status letters or [[launch indices], [the five AttnP fields]], "default" one outcome index per case, "diff"[setting] a flat
    list (case index, outcome index, ...) of the cases that differ from the default setting."""
    idx = list(gold["default"])
    d = gold["diff"].get(setting, [])
    for i in range(0, len(d), 2):
        idx[d[i]] = d[i + 1]
    rows = []
    for o in idx:
        o = gold["outcomes"][o]
        if isinstance(o, str):
            rows.append(o)
        else:
            launches = [gold["launches"][k] for k in o[0]]
            rows.append([[gold["names"][ln[0]], *ln[1:]] for ln in launches] + [o[1]])
    return rows


def test_case_list_matches_the_golden_file():
    gold = json.load(open(GOLDEN))
    cs = cases()
    assert gold["cases"] == len(cs) and len(set(cs)) > 900
    assert sorted(gold["diff"]) == sorted(s for s in SETTINGS if s != "default")
    assert len(gold["default"]) == len(cs)
    assert os.path.getsize(GOLDEN) < 64 * 1024
    switches = {k for env in SETTINGS.values() for k in env}
    assert len(switches) == 16, switches                        # every switch of AttnSwitches has a non-default setting


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_status_launches_and_params_of_every_case(setting):
    want = golden_rows(json.load(open(GOLDEN)), setting)
    rows = plan_under(setting)["rows"]
    cs = cases()
    assert len(rows) == len(cs) == len(want)
    wrong = [(case, got, w) for case, got, w in zip(cs, rows, want) if got != w]
    assert not wrong, f"{len(wrong)} of {len(cs)} cases differ from the recorded dispatch, first: {wrong[:4]}"


def test_every_kernel_is_reached_by_some_setting():
    """The names seen across all settings are the golden file's list: the 82 kernels of the object, each reachable."""
    gold = json.load(open(GOLDEN))
    seen = {ln[0] for s in SETTINGS for row in plan_under(s)["rows"] if not isinstance(row, str) for ln in row[:-1]}
    assert seen == set(gold["names"]), (sorted(seen - set(gold["names"])), sorted(set(gold["names"]) - seen))
    assert len(gold["names"]) == len(set(gold["names"])) == 82


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_launch_shapes_independent_of_the_golden_file(setting):
    env = SETTINGS[setting]
    res = plan_under(setting)
    if env.get("PA_ATTN_SPLIT") != "1":
        assert res["ws"] == 0
    n_ok = 0
    for case, row in zip(cases(), res["rows"]):
        dt, dh, B, H, (Lq, Lk), kpm, causal, drop_p, layout, bwd, x3, defect = case
        if isinstance(row, str):
            continue
        n_ok += 1
        launches, (balanced, ks_min, parts_q, parts_kv, sp_slots) = row[:-1], row[-1]
        assert len(launches) == 1 if not bwd else 1 <= len(launches) <= 3, (case, row)
        for name, gx, gy, gz, block, lds, extra in launches:
            assert block in (256, 512, 1024), (case, row)
            assert 0 <= lds <= 160 * 1024, (case, row)
            if dt == PA_BF16:
                assert gy == gz == 1, (case, row)
            if name.startswith("attn_delta_kernel"):
                assert (gx, gy, gz) == ((B * H * Lq + 255) // 256, 1, 1), (case, row)
            elif name.startswith("attn4_bwd_merged_kernel"):
                assert gx * gy * gz == (-(-Lq // 128) + -(-Lk // 128)) * H * B and extra == -(-Lq // 128) * H * B, (case, row)
            elif balanced != 2 and parts_q == parts_kv == 1:
                owned = Lk if "dkv" in name else Lq
                assert gx * gy * gz == -(-owned // 128) * H * B, (case, row)
            if "merged" not in name:
                assert extra == 0, (case, row)
        if balanced == 2:
            assert sp_slots >= 1 and env.get("PA_ATTN_SPLIT") == "1" and layout == "self_ws", (case, row)
        if parts_q > 1 or parts_kv > 1:
            assert "PA_X3_PARTS" in env and x3 and dt == PA_F32 and dh == 64 and bwd, (case, row)
    assert n_ok > 400


def test_anchors_default_setting():
    """Readable anchors: the model's own attention launches, read off the library before the refactor."""
    rows = dict(zip(cases(), plan_under("default")["rows"]))
    names = lambda c: [ln[0] for ln in rows[c][:-1]]
    # packed encoder self-attention, B 16 x S 1024, H 8: v5 forward; 16-row-wave dQ then dK/dV, one block per (tile, head, element)
    assert names(ENCODER_SELF) == ["attn5_fwd_kernel<true, 3, 3>"] and rows[ENCODER_SELF][0][1:4] == [1024, 1, 1]
    assert names(_bwd(ENCODER_SELF)) == ["attn4_bwd_dq_kernel<true, 1>", "attn4_bwd_dkv_kernel<true, false>"]
    assert rows[ENCODER_SELF][-1][0] == 1                                                   # length-balanced block order
    # decoder cross-attention 128 x 1199: key split in the block (ks_min 4, 1 024 threads); dQ and dK/dV merged into one launch
    assert names(DECODER_CROSS) == ["attn4_fwd_kernel<true, 2>"] and rows[DECODER_CROSS][0][1:5] == [128, 1, 1, 1024]
    assert rows[DECODER_CROSS][-1][1] == 4
    assert names(_bwd(DECODER_CROSS)) == ["attn4_bwd_merged_kernel<true, false>"]
    assert rows[_bwd(DECODER_CROSS)][0][1] == 128 + 10 * 128 and rows[_bwd(DECODER_CROSS)][0][6] == 128
    # decoder causal self-attention 128 x 128 with a key-padding mask: no key split; merged causal backward
    assert names(DECODER_CAUSAL) == ["attn4_fwd_kernel<true, 1>"]
    assert names(_bwd(DECODER_CAUSAL)) == ["attn4_bwd_merged_kernel<true, true>"]


if __name__ == "__main__":
    child()
