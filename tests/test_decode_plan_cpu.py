"""The decode dispatch rule ("which forms the step takes, how many range blocks, how many bytes") pinned without a GPU, through
pa_decode_plan - the dry run of pa_decode_begin / pa_decode_ws_bytes / pa_decode_beam_ws_bytes (include/plank_hip.h).
tests/golden/decode_plan.json holds, for every case under every switch setting, the status or the eleven numbers of the plan: the six
form bits, the range blocks of the absorbed cross- and self-attention launch, mq_sp_bytes, ws_bytes and scr_row.

How the golden file was made: from the commit BEFORE plan_decode existed, not from the code under test.  In a scratch copy of that
commit's csrc/decode.hip one throwaway export was appended that, for a cfg and (B, S, Tmax), called that commit's decode_modes,
step_form, dec_layout(base = NULL), mq_parts, mq_split_bytes and beam_segments(L = NULL) and returned: fold / f32res / mq (decode_modes),
mq_contract / mq_self / mq_self_bf (step_form), mq_parts(B, S) where mq is set and 0 elsewhere, mq_parts(B, Tmax) where mq_self or
mq_self_bf is set and 0 elsewhere, the layout's mq_sp_bytes, dec_layout + 256, and beam_segments' scratch bytes per row.  That library,
built with the project's flags, ran cases() of this file under every entry of SETTINGS (child() below with its `plan_case` hook); the
status of a case is what that commit's pa_model_create answered for the cfg and, for a cfg it accepted, what its pa_decode_ws_bytes
answered for the handle.  The recording also checked, on that commit alone, that dec_layout + 256 equals pa_decode_ws_bytes and that
pa_decode_beam_ws_bytes(rows, K = 1) is the K = 1 beam layout over the recorded scr_row.  The scratch export is not committed.

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
GOLDEN = os.path.join(REPO, "tests", "golden", "decode_plan.json")

PA_F32, PA_BF16 = 0, 1
CODE_OF_STATUS = {-1: "I", -2: "A", -3: "S"}
VOCAB = 514
MQ_MAXS, MQ32_MAXS, MAX_T = 16384, 16000, 2048                 # csrc/decode_mq.h, csrc/decode.hip

DTYPES = [PA_BF16, PA_F32]
DS = [64, 256, 512, 768]
HS = [1, 2, 8, 16, 12]                                         # (12: the one head count of this list d_model 768 can run with)
FFS = [256, 520, 544, 512, 2048, 1024]                         # below d_model 512; no multiple of 32; of 32 but not of 512; 512; 2048; 1024
# (d_model, heads) the sampled cases draw from: head dims 64 / 32 / 16 at every width, and three that no handle can have
WIDTHS = [(64, 1), (64, 2), (256, 8), (256, 16), (512, 8), (512, 16), (768, 12), (512, 2), (768, 16), (64, 16)]
NDECS = [1, 6]
BS = [1, 31, 199, 200, 256, 512, 513]
SS = [1, 1024, 1199, MQ32_MAXS - 1, MQ32_MAXS, MQ32_MAXS + 1, MQ_MAXS, MQ_MAXS + 1]
TS = [1, 12, 1024, 1199, MAX_T]                                # (Tmax beyond MAX_T is an invalid argument: INVALID below)
N_SAMPLED = 400

# (dtype, d_model, n_head, d_ff, n_dec, B, S, Tmax); an invalid argument of each kind
HEADLINE_BF16 = (PA_BF16, 512, 8, 2048, 6, 256, 1199, 1024)
HEADLINE_F32 = (PA_F32, 512, 8, 2048, 6, 256, 1199, 1024)
INVALID = [
    (PA_BF16, 512, 8, 2048, 6, 0, 1199, 1024), (PA_BF16, 512, 8, 2048, 6, -4, 1199, 1024),      # B
    (PA_BF16, 512, 8, 2048, 6, 256, 0, 1024),                                                    # S
    (PA_F32, 512, 8, 2048, 6, 256, 1199, 0), (PA_F32, 512, 8, 2048, 6, 256, 1199, MAX_T + 1),     # Tmax
    (PA_F32, 512, 8, 2048, 6, 256, 1199, MQ32_MAXS + 1), (PA_BF16, 512, 8, 2048, 6, 256, 1199, MQ_MAXS + 1),
    (PA_BF16, 512, 0, 2048, 6, 256, 1199, 1024), (PA_BF16, 512, 3, 2048, 6, 256, 1199, 1024),    # no heads; heads that do not divide
    (PA_BF16, 0, 8, 2048, 6, 256, 1199, 1024),                                                   # d_model
    (PA_BF16, 512, 4, 2048, 6, 256, 1199, 1024), (PA_F32, 768, 16, 2048, 6, 256, 1199, 1024),    # head dims 128 and 48
    (PA_BF16, 512, 8, 2044, 6, 256, 1199, 1024),                                                 # d_ff no multiple of 8
    (7, 512, 8, 2048, 6, 256, 1199, 1024),                                                       # dtype
]

SETTINGS = {
    "default": {},
    "FOLD_LN=0": {"PLANK_DECODE_FOLD_LN": "0"},
    "FOLD_LN=1": {"PLANK_DECODE_FOLD_LN": "1"},
    "F32_RESID=0": {"PLANK_DECODE_F32_RESID": "0"},
    "MQ=0": {"PLANK_DECODE_MQ": "0"},
    "MQ_F32=0": {"PLANK_DECODE_MQ_F32": "0"},
    "MQ_CONTRACT=0": {"PLANK_DECODE_MQ_CONTRACT": "0"},
    "MQ_CONTRACT=1": {"PLANK_DECODE_MQ_CONTRACT": "1"},
    "MQ_SELF=0": {"PLANK_DECODE_MQ_SELF": "0"},
    "MQ_SELF_BF16=0": {"PLANK_DECODE_MQ_SELF_BF16": "0"},
    "MQ_SELF_BF16=1": {"PLANK_DECODE_MQ_SELF_BF16": "1"},
    "MQ_SELF_MINB=32": {"PLANK_DECODE_MQ_SELF_MINB": "32"},
    "MQ_PARTS=1": {"PLANK_DECODE_MQ_PARTS": "1"},
    "MQ_PARTS=4": {"PLANK_DECODE_MQ_PARTS": "4"},
    "MQ_PARTS=65": {"PLANK_DECODE_MQ_PARTS": "65"},              # (the clamp: 64)
    "MQ_MINT=0": {"PLANK_DECODE_MQ_MINT": "0"},
    "MQ_MINT=2": {"PLANK_DECODE_MQ_MINT": "2"},
    "MQ_NT=0": {"PLANK_DECODE_MQ_NT": "0"},
    "MQ_SWAP=0": {"PLANK_DECODE_MQ_SWAP": "0"},
    "MQ32_W8=0": {"PLANK_DECODE_MQ32_W8": "0"},
    # the bundles of tests/test_decode_logprob_gpu.py and tests/test_decode_mq_gpu.py (bench.py sets none: it reads seven switches to
    # describe the step it measured); the two single-switch ones are the entries of the same name above
    "MQ=0,MQ_F32=0": {"PLANK_DECODE_MQ": "0", "PLANK_DECODE_MQ_F32": "0"},
    "FOLD_LN=1,MQ_SELF_BF16=1,MQ_CONTRACT=0": {"PLANK_DECODE_FOLD_LN": "1", "PLANK_DECODE_MQ_SELF_BF16": "1", "PLANK_DECODE_MQ_CONTRACT": "0"},
}
VARIANT_SWITCHES = ("PLANK_DECODE_MQ_NT", "PLANK_DECODE_MQ_SWAP", "PLANK_DECODE_MQ32_W8")


def cases():
    """The case list, in a fixed order.  The whole cross product is 0.8 million shapes; pinned are
      - every (dtype, d_model, heads, d_ff, n_dec 6) at the headline batch (B 256, S 1199, Tmax 1024): 240 (most head counts do not
        fit most widths: those are statuses),
      - d_model 512 x 8 heads and x 16 heads (dh 32), d_ff 2048, both dtypes and both depths: every B at S 1199, Tmax 1024: 56,
      - the headline model in both dtypes: every (B, S) at Tmax 12 and 1199, and every (B, Tmax) at S 1199: 294,
      - an invalid argument of each kind: 14,
      - N_SAMPLED shapes drawn from the product over WIDTHS by a fixed linear congruential sequence (invalid combinations stay in)."""
    out = [(dt, d, H, ff, 6, 256, 1199, 1024) for dt, d, H, ff in itertools.product(DTYPES, DS, HS, FFS)]
    out += [(dt, 512, H, 2048, nd, B, 1199, 1024) for dt, H, nd, B in itertools.product(DTYPES, [8, 16], NDECS, BS)]
    for dt in DTYPES:
        out += [(dt, 512, 8, 2048, 6, B, S, T) for B, S, T in itertools.product(BS, SS, [12, 1199])]
        out += [(dt, 512, 8, 2048, 6, B, 1199, T) for B, T in itertools.product(BS, TS)]
    out += INVALID
    dims = [DTYPES, WIDTHS, FFS, NDECS, BS + [0], SS + [0], TS + [MAX_T + 1]]
    x = 12345
    for _ in range(N_SAMPLED):
        pick = []
        for d in dims:
            x = (x * 1103515245 + 12345) % (1 << 31)
            pick.append(d[(x >> 8) % len(d)])
        out.append((pick[0], *pick[1], *pick[2:]))
    return out


def model_cfg(case):
    """The pa_model_cfg of a case (what the plan does not read is the shipped configuration's)."""
    sys.path.insert(0, REPO)
    from plankassembly_amd.models import _ModelCfg
    dt, d, H, ff, nd = case[:5]
    c = _ModelCfg()
    c.d_model, c.n_head, c.d_ff, c.n_enc, c.n_dec, c.vocab, c.out_dof = d, H, ff, 6, nd, VOCAB, 6
    c.eps_layer, c.eps_final, c.has_enc_norm, c.dropout, c.pad, c.end, c.dtype, c.activation = 1.0, 1e-5, 1, 0.0, 513, 512, dt, 1
    return c


def plan_row(info):
    return [info.fold, info.f32res, info.mq, info.mq_contract, info.mq_self, info.mq_self_bf, info.parts_cross, info.parts_self,
            info.mq_sp_bytes, info.ws_bytes, info.scr_row]


def child(plan_case=None, extra=None):
    """Plan every case under this process's environment; one JSON line: {"rows": [status letter, or the eleven numbers of the plan,
    ...], "variants": [mq_nt, mq_swap, mq32_w8]}.  plan_case(cfg, B, S, Tmax) -> row: how a case is planned (the recording of the
    golden file put the instrumented library of the earlier commit here)."""
    variants = None
    if plan_case is None:
        sys.path.insert(0, REPO)
        from plankassembly_amd import _lib as L
        lib = L.lib()

        def plan_case(cfg, B, S, Tmax):
            nonlocal variants
            info = L.DecodePlanInfo()
            rc = lib.pa_decode_plan(C.byref(cfg), B, S, Tmax, C.byref(info))
            if rc:
                return CODE_OF_STATUS[rc]
            assert variants in (None, [info.mq_nt, info.mq_swap, info.mq32_w8]) and info.pad_ == 0
            variants = [info.mq_nt, info.mq_swap, info.mq32_w8]
            return plan_row(info)

    rows = [plan_case(model_cfg(case), *case[5:]) for case in cases()]
    print(json.dumps(dict({"rows": rows, "variants": variants}, **(extra() if extra else {}))))


_RUNS = {}


def plan_under(setting):
    if not _RUNS:                                               # all children at once: short single-threaded processes
        if not os.path.exists(os.path.join(REPO, "plankassembly_amd", "libplank_hip.so")):
            sys.path.insert(0, REPO)
            from plankassembly_amd.build import build
            build()
        procs = {}
        for s, switches in SETTINGS.items():
            env = {k: v for k, v in os.environ.items() if not k.startswith(("PLANK_DECODE_", "PLANK_HIP_LIB"))}
            env.update(switches, OMP_NUM_THREADS="1")
            procs[s] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], cwd=REPO, env=env, stdout=subprocess.PIPE,
                                        stderr=subprocess.PIPE, text=True)
        for s, pr in procs.items():
            out, err = pr.communicate(timeout=600)
            _RUNS[s] = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1]) if pr.returncode == 0 else err[-4000:]
    assert isinstance(_RUNS[setting], dict), _RUNS[setting]
    return _RUNS[setting]


def golden_rows(gold, setting):
    """Decode the golden file's compact form: "outcomes" are the unique rows (a status letter or the eleven numbers), "default" one
    outcome index per case, "diff"[setting] a flat list (case index, outcome index, ...) of the cases that differ from the default
    setting."""
    idx = list(gold["default"])
    d = gold["diff"].get(setting, [])
    for i in range(0, len(d), 2):
        idx[d[i]] = d[i + 1]
    return [gold["outcomes"][o] for o in idx]


def test_case_list_matches_the_golden_file():
    gold = json.load(open(GOLDEN))
    cs = cases()
    assert gold["cases"] == len(cs) and len(set(cs)) > 900
    assert sorted(gold["diff"]) == sorted(s for s in SETTINGS if s != "default")
    assert len(gold["default"]) == len(cs)
    assert os.path.getsize(GOLDEN) < 128 * 1024
    switches = {k for env in SETTINGS.values() for k in env}
    assert len(switches) == 13, switches                        # every switch of DecodeSwitches has a non-default setting
    for s in SETTINGS:
        if s != "default" and not set(SETTINGS[s]) <= set(VARIANT_SWITCHES):
            assert gold["diff"][s], f"{s} changes no case"


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_status_forms_parts_and_bytes_of_every_case(setting):
    want = golden_rows(json.load(open(GOLDEN)), setting)
    rows = plan_under(setting)["rows"]
    cs = cases()
    assert len(rows) == len(cs) == len(want)
    wrong = [(case, got, w) for case, got, w in zip(cs, rows, want) if got != w]
    assert not wrong, f"{len(wrong)} of {len(cs)} cases differ from the recorded rule, first: {wrong[:4]}"


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_kernel_variant_switches_are_reported_as_set(setting):
    env = SETTINGS[setting]
    assert plan_under(setting)["variants"] == [int(env.get(k, "1")) for k in VARIANT_SWITCHES]


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_plans_are_consistent_independent_of_the_golden_file(setting):
    n_ok = 0
    for case, row in zip(cases(), plan_under(setting)["rows"]):
        dt, d, H, ff, nd, B, S, T = case
        if isinstance(row, str):
            continue
        n_ok += 1
        fold, f32res, mq, contract, mq_self, self_bf, pc, ps, sp, ws, scr = row
        assert fold or not (f32res or mq), (case, row)
        assert mq or not (contract or mq_self or self_bf), (case, row)
        assert not (mq_self and self_bf) and (not mq_self or dt == PA_F32) and (not (self_bf or f32res) or dt == PA_BF16), (case, row)
        assert (pc >= 1) == bool(mq) and (ps >= 1) == bool(mq_self or self_bf) and pc <= 64 and ps <= 64, (case, row)
        tickets = -(-B * 4 // 256) * 256                        # range blocks: one ticket word per row, then the partials
        assert (sp > tickets and mq) if max(pc, ps) > 1 else (sp == 0 or mq), (case, row)
        e = 2 if dt == PA_BF16 else 4
        caches = nd * 2 * B * T * d * e + (B * S * d * e if mq else nd * 2 * B * S * d * e)
        assert ws > caches + sp, (case, row)
        per_layer = T * d * e if (mq_self or self_bf) else 2 * T * d * e
        assert scr >= nd * per_layer + T * d * e + 2 * T * 8 and scr % 256 == 0, (case, row)
    assert n_ok > 600


def test_anchors_default_setting():
    """Readable anchors: the headline decode (B 256, S 1199, Tmax 1024), read off the library before the refactor."""
    rows = dict(zip(cases(), plan_under("default")["rows"]))
    # bf16: folded, f32 residual stream, absorbed cross-attention and - from 200 rows - self-attention, no range blocks at 256 rows
    assert rows[HEADLINE_BF16][:8] == [1, 1, 1, 0, 0, 1, 1, 1] and rows[HEADLINE_BF16][8] == 0
    assert rows[HEADLINE_BF16[:5] + (199, 1199, 1024)][:8] == [1, 1, 1, 0, 0, 0, 1, 0]
    # exact f32: folded, absorbed with W_v as its own launch, self-attention absorbed
    assert rows[HEADLINE_F32][:8] == [1, 0, 1, 1, 1, 0, 1, 1]
    # one row: 256 / 1 blocks would fit, 75 key tiles / 8 allow 9 (cross), 64 tiles / 8 allow 8 (self)
    assert rows[HEADLINE_F32[:5] + (1, 1199, 1024)][6:8] == [9, 8]
    # 513 rows: nothing folds, nothing is absorbed
    assert rows[HEADLINE_BF16[:5] + (513, 1199, 1024)][:8] == [0] * 8


def test_null_arguments():
    sys.path.insert(0, REPO)
    from plankassembly_amd import _lib as L
    info = L.DecodePlanInfo()
    cfg = model_cfg(HEADLINE_BF16)
    assert L.lib().pa_decode_plan(None, 4, 40, 12, C.byref(info)) == -1
    assert L.lib().pa_decode_plan(C.byref(cfg), 4, 40, 12, None) == -1


def test_sim_mode_of_the_logprob_cases_agrees_with_the_plan():
    """tests/decode_logprob_cases.py::sim_mode restates the f32res rule by hand for its cases A to F: it must be the plan's."""
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import decode_logprob_cases as DL
    from plankassembly_amd import _lib as L
    for cid, spec in sorted(DL.CASES.items()):
        c = DL.case_dict(cid)
        ocfg = c["cfg"] if "cfg" in c else DL.LC.case_oracle_cfg(c)
        case = (PA_BF16, c["d"], ocfg.n_head, c["ff"], ocfg.n_dec, spec["B"], ocfg.max_input_length - 1, spec["n"])
        info = L.DecodePlanInfo()
        L.check(L.lib().pa_decode_plan(C.byref(model_cfg(case)), *case[5:], C.byref(info)), "pa_decode_plan")
        assert DL.sim_mode(cid) == ("step_f32res" if info.f32res else "step_all_bf16"), (cid, case, plan_row(info))


if __name__ == "__main__":
    child()
