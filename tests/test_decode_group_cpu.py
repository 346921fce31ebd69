"""Decode groups without a GPU: the plan of a decode of B * G rows over B drawings (pa_decode_group_plan - pure,
no handle, no device) and the host-side validation of the ``share_encoder`` setting.

The PLANK_DECODE_* switches are read once per process, so the plans are made in child processes (this file run as a script, the
environment cleared of the switches as tests/test_decode_plan_cpu.py does) that print one JSON line; the parent asserts."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import test_decode_plan_cpu as P

REPO = P.REPO
HEADLINE = (P.PA_BF16, 512, 8, 2048, 6, 16, 1024, 128)            # (dtype, d_model, heads, d_ff, n_dec, B drawings, S, Tmax)
HEADLINE_F32 = (P.PA_F32,) + HEADLINE[1:]
SMALL = (P.PA_F32, 64, 4, 128, 2, 4, 64, 36)                      # the small fixture's model: d 64, the K / V-cache form
PLAN_FIELDS = ("fold", "f32res", "mq", "mq_contract", "mq_self", "mq_self_bf", "parts_cross", "parts_self", "mq_nt", "mq_swap", "mq32_w8",
               "pad_", "mq_sp_bytes", "ws_bytes", "scr_row")
GROUP_FIELDS = ("rows", "rows_per_block", "units", "pad_", "mem_rows")


def child():
    sys.path.insert(0, REPO)
    from plankassembly_amd import _lib as L
    lib = L.lib()

    def plain(case):
        info = L.DecodePlanInfo()
        rc = lib.pa_decode_plan(C.byref(P.model_cfg(case)), *case[5:], C.byref(info))
        return rc, [getattr(info, f) for f in PLAN_FIELDS]

    def group(case, G):
        info, g = L.DecodePlanInfo(), L.DecodeGroupInfo()
        rc = lib.pa_decode_group_plan(C.byref(P.model_cfg(case)), case[5], G, case[6], case[7], C.byref(info), C.byref(g))
        return rc, [getattr(info, f) for f in PLAN_FIELDS], [getattr(g, f) for f in GROUP_FIELDS]

    out = {"ungrouped_differ": [], "ungrouped_ok": 0}
    for case in P.cases():
        rc, row = plain(case)
        grc, grow, g = group(case, 1)
        want_g = [case[5], 1, case[5], 0, case[5] * case[6]] if rc == 0 else [0, 0, 0, 0, 0]
        if (rc, row) != (grc, grow) or g != want_g:
            out["ungrouped_differ"].append([list(case), rc, row, grc, grow, g])
        out["ungrouped_ok"] += rc == 0
    out["headline"] = {str(G): group(HEADLINE, G) for G in (1, 2, 3, 8, 64)}
    out["headline_f32_g8"] = group(HEADLINE_F32, 8)
    out["headline_rows128"] = plain(HEADLINE[:5] + (128,) + HEADLINE[6:])
    out["heads16_g8"] = group((P.PA_BF16, 512, 16, 2048, 6, 16, 1024, 128), 8)
    out["small"] = {str(G): group(SMALL, G) for G in (1, 2, 4)}
    out["small_rows8"] = plain(SMALL[:5] + (8,) + SMALL[6:])
    out["errors"] = [group(HEADLINE, 0)[0], group(HEADLINE, 65)[0], group(HEADLINE[:5] + (0,) + HEADLINE[6:], 2)[0],
                     group(HEADLINE, -1)[0], group(HEADLINE[:5] + (2 ** 30,) + HEADLINE[6:], 4)[0]]
    info, g = L.DecodePlanInfo(), L.DecodeGroupInfo()
    cfg = P.model_cfg(HEADLINE)
    out["nulls"] = [lib.pa_decode_group_plan(None, 16, 2, 1024, 128, C.byref(info), C.byref(g)),
                    lib.pa_decode_group_plan(C.byref(cfg), 16, 2, 1024, 128, None, C.byref(g)),
                    lib.pa_decode_group_plan(C.byref(cfg), 16, 2, 1024, 128, C.byref(info), None)]
    out["sizes"] = [C.sizeof(L.DecodePlanInfo), C.sizeof(L.DecodeGroupInfo)]
    print(json.dumps(out))


_RUNS = {}


def plans(setting="default"):
    if setting not in _RUNS:
        env = {k: v for k, v in os.environ.items() if not k.startswith(("PLANK_DECODE_", "PLANK_HIP_LIB"))}
        env.update({"default": {}, "PAIR=0": {"PLANK_DECODE_MQ_PAIR": "0"}, "PAIR=1": {"PLANK_DECODE_MQ_PAIR": "1"}}[setting], OMP_NUM_THREADS="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        _RUNS[setting] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return _RUNS[setting]


def mq_parts(units, S, mint=8):
    """csrc/decode_mq.h mq_parts restated (no forced count): enough range blocks to fill 256 CUs, at least `mint` key tiles each."""
    ntiles = (S + 15) // 16
    p = min(256 // units, ntiles // mint)
    return max(1, min(64, p))


def as_plan(row):
    return dict(zip(PLAN_FIELDS, row))


def as_group(row):
    return dict(zip(GROUP_FIELDS, row))


@pytest.mark.parametrize("setting", ["default", "PAIR=0"])
def test_ungrouped_plan_is_pa_decode_plan_field_by_field(setting):
    """G = 1 over every case the plan test walks (tests/golden/decode_plan.json): status and all fifteen fields of pa_decode_plan; the
    group is B rows, one per block, B units, B * S memory rows."""
    r = plans(setting)
    assert r["ungrouped_differ"] == [] and r["ungrouped_ok"] > 600
    assert r["sizes"] == [72, 24]


def test_headline_groups():
    r = plans()
    _, B, S, T = HEADLINE[4:]
    rc, plan8, g8 = r["headline"]["8"]
    plan8, g8 = as_plan(plan8), as_group(g8)
    assert rc == 0 and g8 == dict(rows=128, rows_per_block=2, units=64, pad_=0, mem_rows=16 * 1024)
    assert plan8["mq"] == 1 and plan8["parts_cross"] == mq_parts(64, S) == 4
    rc, plan3, g3 = r["headline"]["3"]
    assert rc == 0 and as_group(g3) == dict(rows=48, rows_per_block=1, units=48, pad_=0, mem_rows=16 * 1024)
    assert as_plan(plan3)["parts_cross"] == mq_parts(48, S) == 5
    rc, plan2, g2 = r["headline"]["2"]
    assert rc == 0 and as_group(g2)["rows_per_block"] == 2 and as_group(g2)["units"] == 16 and as_plan(plan2)["parts_cross"] == mq_parts(16, S) == 8
    # the row-count decisions use the rows: 16 x 64 = 1024 rows are beyond the 512-row forms - nothing folds, nothing is absorbed
    rc, plan64, g64 = r["headline"]["64"]
    assert rc == 0 and as_plan(plan64)["fold"] == 0 and as_plan(plan64)["mq"] == 0 and as_group(g64) == dict(
        rows=1024, rows_per_block=1, units=1024, pad_=0, mem_rows=16 * 1024)
    # one memory per drawing: the workspace of 128 rows over 16 drawings is smaller than that of 128 repeated drawings by at least
    # the 112 memory copies
    rc, rows128 = r["headline_rows128"]
    rows128 = as_plan(rows128)
    assert rc == 0 and rows128["ws_bytes"] - plan8["ws_bytes"] >= (128 - 16) * S * 512 * 2
    for f in ("fold", "f32res", "mq", "mq_contract", "mq_self", "mq_self_bf", "parts_self", "scr_row"):      # decided by the 128 rows
        assert plan8[f] == rows128[f], f
    # exact f32: the self launches stay per row (128 rows: 2 range blocks of the 8 Tmax tiles allow 1)
    rc, p32, g32 = r["headline_f32_g8"]
    assert rc == 0 and as_group(g32)["rows_per_block"] == 2 and as_plan(p32)["mq_self"] == 1
    assert as_plan(p32)["parts_cross"] == mq_parts(64, S) and as_plan(p32)["parts_self"] == mq_parts(128, T) == 1
    # 16 heads (dh 32) fill the 16 slots alone - and are beyond the absorbed form's 8 heads anyway
    rc, p16, g16 = r["heads16_g8"]
    assert rc == 0 and as_group(g16)["rows_per_block"] == 1


def test_pairing_switch():
    off, on = plans("PAIR=0"), plans("PAIR=1")
    assert on["headline"] == plans()["headline"]                                 # unset = 1
    _, plan8, g8 = off["headline"]["8"]
    assert as_group(g8) == dict(rows=128, rows_per_block=1, units=128, pad_=0, mem_rows=16 * 1024)
    assert as_plan(plan8)["parts_cross"] == mq_parts(128, 1024) == 2
    assert off["headline"]["3"] == on["headline"]["3"]


def test_small_cfg_is_never_paired():
    r = plans()
    for G in ("1", "2", "4"):
        rc, plan, g = r["small"][G]
        assert rc == 0 and as_plan(plan)["mq"] == 0 and as_group(g)["rows_per_block"] == 1 and as_group(g)["units"] == 4 * int(G)
        assert as_group(g)["mem_rows"] == 4 * 64
    # K / V-cache form: the per-layer cross-attention caches and the projection scratch are per drawing too
    rc, rows8 = r["small_rows8"]
    e, d, S, nd = 4, 64, 64, 2
    assert as_plan(rows8)["ws_bytes"] - as_plan(r["small"]["2"][1])["ws_bytes"] >= (8 - 4) * S * d * e * (2 * nd + 2)


def test_plan_errors():
    r = plans()
    assert r["errors"] == [-1, -1, -1, -1, -1]                                  # G 0, G 65, B 0, G -1, B * G beyond int32: PA_EINVAL
    assert r["nulls"] == [-1, -1, -1]


def test_abi_is_declared_and_bound():
    sys.path.insert(0, REPO)
    from plankassembly_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "plank_hip.h")).read()
    for name in ("pa_decode_group_ws_bytes", "pa_decode_group_begin", "pa_decode_group_plan", "pa_dec_cross_mq_group", "pa_dec_cross_mq32_group"):
        assert f"{name}(" in hdr and hasattr(L.lib(), name) and getattr(L.lib(), name).argtypes is not None, name
    assert "} pa_decode_group_info;" in hdr


def _cfg(**model):
    from plankassembly_amd.config import CfgNode
    base = dict(NUM_MODEL=64, NUM_HEAD=4, NUM_FEEDFORWARD=128, DROPOUT=0.0, ACTIVATION="relu", NORMALIZE_BEFORE=True,
                NUM_ENCODER_LAYERS=2, NUM_DECODER_LAYERS=2, COMPUTE_DTYPE="f32")
    data = dict(NUM_VIEW=3, NUM_TYPE=2, NUM_INPUT_DOF=4, NUM_OUTPUT_DOF=6, MAX_INPUT_LENGTH=65, MAX_OUTPUT_LENGTH=36, VOCAB_SIZE=514)
    return CfgNode(dict(MODEL=dict(base, **model), DATA=data, TOKEN=dict(END=512, PAD=513)))


def test_share_encoder_setting_is_validated_on_the_host():
    sys.path.insert(0, REPO)
    import types
    from plankassembly_amd.models import PlankModel, build_model
    from plankassembly_amd.trainer import seq_train_options
    assert build_model(_cfg()).share_encoder is False
    assert build_model(_cfg(SHARE_ENCODER=True)).share_encoder is True and build_model(_cfg(SHARE_ENCODER=False)).share_encoder is False
    for bad in ("yes", 1, 0, "true"):
        with pytest.raises(ValueError, match="SHARE_ENCODER"):
            build_model(_cfg(SHARE_ENCODER=bad))
    tok = types.SimpleNamespace(END=512, PAD=513)
    mk = lambda **kw: PlankModel(64, 4, 128, 0.0, "relu", True, 2, 2, 3, 2, 4, 6, 65, 36, 514, tok, **kw)
    assert mk().share_encoder is False and mk(share_encoder=True).share_encoder is True
    with pytest.raises(ValueError, match="SHARE_ENCODER"):
        mk(share_encoder="yes")
    m = mk(share_encoder=True)
    assert m._share(None) is True and m._share(False) is False and mk()._share(None) is False and mk()._share(True) is True
    with pytest.raises(ValueError, match="SHARE_ENCODER"):
        m._share(1)
    # the SEQ_TRAIN block: absent = the model's setting (no key in the step's arguments), a bool is passed through, anything else raises
    assert "share_encoder" not in seq_train_options({"SEQ_TRAIN": {"NUM_SAMPLES": 4}})["step"]
    assert seq_train_options({"SEQ_TRAIN": {"NUM_SAMPLES": 4, "SHARE_ENCODER": True}})["step"]["share_encoder"] is True
    assert seq_train_options({"SEQ_TRAIN": {"NUM_SAMPLES": 4, "SHARE_ENCODER": False}})["step"]["share_encoder"] is False
    for bad in ("yes", 1):
        with pytest.raises(ValueError, match="SHARE_ENCODER"):
            seq_train_options({"SEQ_TRAIN": {"NUM_SAMPLES": 4, "SHARE_ENCODER": bad}})


def test_decoders_take_and_check_the_flag():
    """The decoders' share_encoder is checked before anything touches a device; two lanes refuse a group."""
    sys.path.insert(0, REPO)
    import plankassembly_amd.decode as D
    with pytest.raises(ValueError, match="SHARE_ENCODER"):
        D._share_flag("yes")
    assert D._share_flag(True) is True and D.GreedyDecoder.share_encoder is False
    import inspect
    for cls in (D.BeamDecoder, D.SampleDecoder):
        assert inspect.signature(cls.__init__).parameters["share_encoder"].default is False
    assert inspect.signature(D._Lane.begin).parameters["group"].default == 1


if __name__ == "__main__":
    child()
