"""pa_decode_plan (the dry run of the decode dispatch, tests/test_decode_plan_cpu.py) pinned to the real path: under each switch bundle,
in a fresh child process (the switches are read once per process), the bytes the plan reports are the bytes the handle asks for, the
beam workspace is the beam layout over the plan's scr_row, and a 12-step greedy decode of the planned form runs.

The smallest shapes that reach every form: d_model 512, 8 heads (head dim 64), d_ff 512, 2 decoder layers, seeded random weights,
S 40 with ragged lengths, Tmax 12; B 4, and B 200 once - the default bf16 step absorbs its self-attention from 200 rows on."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_IN, TMAX = 40, 12
# bundle -> (dtype, switches, batch sizes, the form bits the plan must report: fold, f32res, mq, mq_contract, mq_self, mq_self_bf per size)
BUNDLES = {
    "default_bf16": ("bf16", {}, {4: [1, 1, 1, 0, 0, 0], 200: [1, 1, 1, 0, 0, 1]}),
    "default_f32": ("f32", {}, {4: [1, 0, 1, 1, 1, 0]}),
    "MQ=0": ("bf16", {"PLANK_DECODE_MQ": "0"}, {4: [1, 1, 0, 0, 0, 0]}),
    "FOLD_LN=0": ("bf16", {"PLANK_DECODE_FOLD_LN": "0"}, {4: [0, 0, 0, 0, 0, 0]}),
    "F32_RESID=0": ("bf16", {"PLANK_DECODE_F32_RESID": "0"}, {4: [1, 0, 1, 0, 0, 0]}),
    "MQ_SELF_BF16=1": ("bf16", {"PLANK_DECODE_MQ_SELF_BF16": "1"}, {4: [1, 1, 1, 0, 0, 1]}),
}


def child(dtype, sizes):
    import torch
    sys.path.insert(0, REPO)
    import plankassembly_amd.decode as D
    from plankassembly_amd import _lib as L
    from plankassembly_amd.data import SynthSpec, synth_batch
    from plankassembly_amd.models import PlankModel
    torch.manual_seed(20)
    m = PlankModel(512, 8, 512, 0.0, "relu", True, 2, 2, 3, 2, 4, 6, S_IN + 1, TMAX, 514, types.SimpleNamespace(END=512, PAD=513),
                   compute_dtype=dtype).cuda().eval()
    m._ensure_handle()
    m._refresh_shadow()
    lib, out = L.lib(), {}
    for B in sizes:
        batch = synth_batch(B, SynthSpec(S_IN + 1, TMAX, (1, 10), (1, 1), True), seed=7 + B)
        batch.pop("name")
        dec = D.GreedyDecoder(m, use_graph=False, lanes=1)
        with torch.no_grad():
            dec.begin({k: v.cuda() for k, v in batch.items()})
            h, S = dec._lanes[0].h(), dec._lanes[0].keep[0].S
            info = L.DecodePlanInfo()
            L.check(lib.pa_decode_plan(C.byref(m._cfg_struct()), B, S, TMAX, C.byref(info)), "pa_decode_plan")
            n_steps = dec._loop(TMAX, False, lambda: False)     # (every pa_decode_step answered 0: L.check in the lane)
            torch.cuda.synchronize()
            tokens, _, _ = dec._lanes[0].buffers(B, TMAX)
            out[B] = dict(S=S, bits=[info.fold, info.f32res, info.mq, info.mq_contract, info.mq_self, info.mq_self_bf],
                          plan_ws=info.ws_bytes, ws=int(lib.pa_decode_ws_bytes(h, B, S, TMAX)), scr_row=info.scr_row,
                          beam_ws={K: int(lib.pa_decode_beam_ws_bytes(h, B, S, TMAX, K)) for K in (1, 2, 4)},
                          steps=int(n_steps), in_vocab=bool(((tokens >= 0) & (tokens < 514)).all()))
    print(json.dumps(out))


def beam_ws_bytes(rows, K, scr_row):
    """pa_decode_beam_ws_bytes over a given scr_row (csrc/decode.hip beam_layout): three f32 / int32 [rows], three [rows][K], the
    reorder scratch [rows][scr_row]; every region starts 256-byte aligned; 256 bytes of slack."""
    off = 0
    for n in [rows * 4] * 3 + [rows * 4 * K] * 3 + [rows * scr_row]:
        off = -(-off // 256) * 256 + n
    return off + 256


_DONE = {}


def run_bundle(name):
    """Children run one after the other, each under its own time limit; after the first failure nothing further is started."""
    if "failed" in _DONE:
        pytest.fail(f"not started: the child of bundle {_DONE['failed']} failed")
    dtype, switches, sizes = BUNDLES[name]
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PLANK_DECODE_", "PLANK_HIP_LIB"))}
    env.update(switches)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--child", dtype, *map(str, sizes)],
                       cwd=REPO, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        _DONE["failed"] = name
        pytest.fail(f"child of {name} ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    return {int(k): v for k, v in json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]).items()}


@pytest.mark.parametrize("name", list(BUNDLES))
def test_plan_is_what_the_handle_does(name):
    res = run_bundle(name)
    for B, bits in BUNDLES[name][2].items():
        r = res[B]
        assert r["S"] == S_IN and r["bits"] == bits, (B, r)
        assert r["ws"] == r["plan_ws"] > 0, (B, r)
        assert r["scr_row"] > 0 and r["beam_ws"] == {str(K): beam_ws_bytes(B, K, r["scr_row"]) for K in (1, 2, 4)}, (B, r)
        assert r["steps"] == TMAX and r["in_vocab"], (B, r)


if __name__ == "__main__":
    child(sys.argv[2], [int(x) for x in sys.argv[3:]])
