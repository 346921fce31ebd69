"""Teacher-forced log-probability parity of the decode step at full size.

PlankModel.score with every position forced to a RANDOM candidate (tests/decode_logprob_cases.py) against the float64 oracle, per
token and per row, in every form the step takes: range blocks at 8 and 6 parts per element (cases A, B), one block per element and
the bf16 absorbed self-attention (C, B 256), 1024 cached keys (D), the generic step at d_model 512 beyond 512 rows (E), the generic
bf16 step on the small fixture (F), eager against graph replay (G) and, in child processes, the forms the environment switches of
csrc/decode.hip select.  No token is left out of a comparison; a non-finite value on either side fails.

Bounds (none is measured on the device; the device's values are printed next to them):
  f32   per token |lp - lp64| <= 1e-4 (the project's parity bound) while the CPU's own float32 evaluation of the same rows stays
        below 2.5e-5; per row |score - score64| <= 15 x the CPU float32 evaluation's cumulative deviation on the same row set
  bf16  against the rounding simulation (tests/bf16_decode_sim.py, the step_* mode of the device's form) on the same tokens:
        mean |lp - lp64| <= 2 x the simulation's (3 x below 1 000 scored tokens), max <= 3 x the simulation's max,
        |mean(lp - lp_sim)| <= half the simulation's mean |lp_sim - lp64|
  D     each step range [0,6) [6,128) [128,512) [512,1024) on its own: f32 1e-4 per token, bf16 range mean <= 2 x the simulation's
        mean of that range
Measured on MI355X: profiles/decode_logprob_parity.txt."""
import os
import subprocess
import sys
import time

import pytest
import torch

import decode_logprob_cases as DL
import large_cases as LC
from test_beam_gpu import make

pytestmark = pytest.mark.gpu

SEED = 2027
CASES, case_dict, sim_mode = DL.CASES, DL.case_dict, DL.sim_mode
_CACHE = {}          # per case id: batch, forced sequences, float64 / float32 references; (id, mode): the simulation; (id, dtype): device lp
T0 = time.time()


def disk(name):
    """File of a CPU reference in the directory the parent process hands its children (PLANK_LOGPROB_CACHE), or None."""
    d = os.environ.get("PLANK_LOGPROB_CACHE")
    return os.path.join(d, name) if d else None


def ref_file(cid):
    return disk(f"ref_{cid}_{len(CASES[cid]['rows'])}rows_seed{SEED}.pt")


def save_refs():
    """Write what this process has computed on the CPU where the next child process finds it."""
    for key, val in list(_CACHE.items()):
        if isinstance(key, str) and ref_file(key) and not os.path.exists(ref_file(key)):
            torch.save(dict(rows=CASES[key]["rows"], tokens=val["tokens"], attach=val["attach"], ref=val["ref"]), ref_file(key))
        if isinstance(key, tuple) and len(key) == 2 and key[0] != "model":
            f = disk(f"sim_{key[0]}_{len(CASES[key[0]]['rows'])}rows_seed{SEED}_{key[1]}.pt")
            if f and not os.path.exists(f):
                torch.save(dict(rows=CASES[key[0]]["rows"], lp=val), f)


def prepared(cid):
    """The case's batch, forced sequences of ALL rows and the CPU references of the scored rows (computed once per process)."""
    if cid not in _CACHE:
        spec, c = CASES[cid], case_dict(cid)
        batch = c["batch"] if "batch" in c else LC.case_batch(c, decode=True, batch_size=spec["B"])
        assert batch["input_value"].shape[0] == spec["B"]
        rows = spec["rows"]
        f = ref_file(cid)
        if f and os.path.exists(f):                      # computed by the parent process or an earlier child on the same inputs
            z = torch.load(f)
            assert z["rows"] == rows and z["tokens"].shape == (spec["B"], spec["n"])
            _CACHE[cid] = dict(c=c, batch=batch, tokens=z["tokens"], attach=z["attach"], ref=z["ref"])
            print(f"    [{cid}] references of rows {rows} taken from the files of the parent process")
            return _CACHE[cid]
        tokens, attach = DL.random_forced(range(spec["B"]), spec["n"], SEED)
        t0 = time.time()
        ref = DL.reference(c, batch, rows, tokens[rows], attach[rows])
        print(f"    [{cid}] float64 reference of rows {rows} x {spec['n']} steps (+ float32 on the same rows): {time.time() - t0:.0f} s; "
              f"log p in [{float(ref['lp'].min()):.1f}, {float(ref['lp'].max()):.1f}], pointers {float((attach[rows] >= 0).double().mean()):.2f}")
        _CACHE[cid] = dict(c=c, batch=batch, tokens=tokens, attach=attach, ref=ref)
        save_refs()
    return _CACHE[cid]


def model(cid, dtype):
    key = ("model", CASES[cid]["case"], dtype)
    if key not in _CACHE:
        for k in [k for k in _CACHE if k[0] == "model" and k[1] != key[1]]:      # one case's models at a time on the device
            del _CACHE[k]
        c = case_dict(cid)
        if "sd" in c:
            _CACHE[key] = make(c["sd"], dtype)
        else:
            _CACHE[key] = make(LC.case_state_dict(c), dtype, c["d"], c["h"], c["ff"], c["ne"], c["nd"], c["max_in"], c["max_out"])
    return _CACHE[key]


def device_score(cid, dtype, graph=True):
    import plankassembly_amd.decode as D
    p, spec = prepared(cid), CASES[cid]
    m = model(cid, dtype)
    m._decoder = D.GreedyDecoder(m, use_graph=graph, strict_graph=graph)
    with torch.no_grad():
        got = m.score(m.prepare_batch(p["batch"]), p["tokens"], p["attach"], torch.full((spec["B"],), spec["n"]))
    torch.cuda.synchronize()
    assert (m._decoder._graph is not None) == graph
    got["running"] = m._decoder.last_prefix_scores           # the step's own f32 running sum (what complete / beam / sampling report)
    m._decoder = None
    assert got["logprobs"].shape == (spec["B"], spec["n"]) and got["logprobs"].dtype == got["scores"].dtype == torch.float32
    return got


def simulated(cid, mode):
    if (cid, mode) not in _CACHE:
        p, rows = prepared(cid), CASES[cid]["rows"]
        f = disk(f"sim_{cid}_{len(rows)}rows_seed{SEED}_{mode}.pt")
        if f and os.path.exists(f):
            z = torch.load(f)
            assert z["rows"] == rows
            _CACHE[(cid, mode)] = z["lp"]
            return _CACHE[(cid, mode)]
        t0 = time.time()
        _CACHE[(cid, mode)] = DL.simulated(p["c"], p["batch"], rows, p["tokens"][rows], p["attach"][rows], mode)
        print(f"    [{cid}] simulation {mode}: {time.time() - t0:.0f} s")
        save_refs()
    return _CACHE[(cid, mode)]


def fmt(st):
    return f"max {st[0]:.3e} mean {st[1]:.3e} signed {st[2]:+.3e} (n {st[3]})"


def report(cid, dtype, what, diff, yard=None):
    """Per-case printout: max / mean / signed mean of the per-token difference, the same by step range, against the yardstick."""
    st = DL.range_stats(diff)
    ys = DL.range_stats(yard) if yard is not None else {}
    for key in st:
        name = "all steps" if key == "all" else f"steps [{key[0]},{min(key[1], diff.shape[1])})"
        line = f"    [{cid} {dtype}] {what} {name}: {fmt(st[key])}"
        if key in ys:
            line += f" | yardstick max {ys[key][0]:.3e} mean {ys[key][1]:.3e}: ratio max {st[key][0] / ys[key][0]:.2f} mean {st[key][1] / ys[key][1]:.2f}"
        print(line)
    return st, ys


def switches():
    on = {k: v for k, v in os.environ.items() if k.startswith("PLANK_DECODE_")}
    return f" switches {on}" if on else ""


def check_scores(cid, dtype, got):
    """What PlankModel.score guarantees, on every row of the device batch: `scores` is the float64 sum of its own per-token values
    rounded ONCE to f32 (no position forced here is END, so every position is summed) - an f32 running sum does not pass this.  The
    step's own running sum, which the decoders keep reporting, stays within the worst case of n sequential f32 additions,
    n * 2^-24 * the largest partial sum, of the same float64 sum."""
    lp = got["logprobs"].double()
    total = lp.sum(1)
    assert torch.equal(got["scores"], total.float()), float((got["scores"].double() - total).abs().max())
    n = lp.shape[1]
    worst = n * 2.0 ** -24 * lp.cumsum(1).abs().max(1).values
    drift = (got["running"].double() - total).abs()
    r = int((drift / worst).argmax())
    print(f"    [{cid} {dtype}] scores = float32(float64 sum of the per-token values) on all {lp.shape[0]} rows: exact; the step's f32 running sum is "
          f"up to {float(drift.max()):.3e} from that sum (row {int(drift.argmax())}; largest share of its worst case n 2^-24 |sum|: "
          f"{float(drift[r] / worst[r]):.3f}, row {r})")
    assert bool((drift <= worst).all()), (r, float(drift[r]), float(worst[r]))


def check_f32(cid, got):
    check_scores(cid, "f32", got)
    p, rows = prepared(cid), CASES[cid]["rows"]
    ref = p["ref"]
    lp, lp64 = got["logprobs"][rows].double(), ref["lp"]
    assert bool(torch.isfinite(got["logprobs"]).all()) and bool(torch.isfinite(got["scores"]).all()), "non-finite log p on the device"
    own = (ref["lp32"] - lp64[ref["rows32"]])
    print(f"    [{cid} f32]{switches()} rows {rows}: bound per token {DL.F32_TOKEN_BOUND:.0e}; the CPU's float32 evaluation of rows "
          f"{[rows[i] for i in ref['rows32']]}: {fmt(DL.range_stats(own)['all'])}")
    st, _ = report(cid, "f32", "device - float64", lp - lp64)
    cum_own = float(own.sum(1).abs().max())
    cum = (got["scores"][rows].double() - lp64.sum(1))
    cum_bound = DL.F32_CUM_FACTOR * cum_own
    print(f"    [{cid} f32] cumulative per row (device score - float64): {[f'{float(x):+.2e}' for x in cum]}; max {float(cum.abs().max()):.3e} "
          f"against {DL.F32_CUM_FACTOR:.0f} x the CPU float32 evaluation's {cum_own:.3e} = {cum_bound:.3e} (ratio {float(cum.abs().max()) / cum_bound:.2f}); "
          f"per token max {st['all'][0]:.3e} = {st['all'][0] / DL.F32_TOKEN_BOUND:.2f} of the bound; the device's per-token values "
          f"summed in float64 deviate {float((lp.sum(1) - lp64.sum(1)).abs().max()):.3e}, one float32 rounding of the score is up to "
          f"{float(torch.finfo(torch.float32).eps * lp64.sum(1).abs().max() / 2):.1e}")
    d, mag = lp - lp64, lp64.abs()
    octaves = [(lo, d[(mag >= lo) & (mag < 2 * lo)]) for lo in (1, 2, 4, 8, 16, 32)]
    print(f"    [{cid} f32] signed mean of device - float64 by |log p| in [x, 2x): "
          + ", ".join(f"{lo}: {float(v.mean()):+.2e} (n {v.numel()})" for lo, v in octaves if v.numel()))
    assert float(own.abs().max()) <= DL.F32_CPU_FLOAT32_MAX, float(own.abs().max())
    fails = DL.f32_per_token_failures(lp, lp64)                       # (every step range is held to the same bound: nothing drifts)
    assert len(fails) == 0, [(rows[int(r)], int(t), float(lp[r, t] - lp64[r, t])) for r, t in fails[:8]]
    assert float(cum.abs().max()) <= cum_bound, (float(cum.abs().max()), cum_bound)


def check_bf16(cid, got):
    check_scores(cid, "bf16", got)
    p, rows = prepared(cid), CASES[cid]["rows"]
    mode = sim_mode(cid)
    lp64, sim = p["ref"]["lp"], simulated(cid, mode)
    lp = got["logprobs"][rows].double()
    assert bool(torch.isfinite(got["logprobs"]).all()) and bool(torch.isfinite(got["scores"]).all()), "non-finite log p on the device"
    assert bool(torch.isfinite(sim).all()), "non-finite log p in the simulation"
    n_tok = lp.numel()
    k_mean, k_max = (2.0 if n_tok >= 1000 else 3.0), 3.0
    print(f"    [{cid} bf16]{switches()} rows {rows}: yardstick = simulation '{mode}' against float64; mean x {k_mean:.0f}, max x {k_max:.0f}, "
          f"bias 0.5 x its mean")
    st, ys = report(cid, "bf16", "device - float64", lp - lp64, sim - lp64)
    bias = float((lp - sim).mean())
    cum = got["scores"][rows].double() - lp64.sum(1)
    print(f"    [{cid} bf16] bias mean(device - simulation) {bias:+.3e} against {0.5 * ys['all'][1]:.3e} (ratio {abs(bias) / (0.5 * ys['all'][1]):.2f}); "
          f"cumulative per row (device score - float64): {[f'{float(x):+.2e}' for x in cum]}, simulation: "
          f"{[f'{float(x):+.2e}' for x in (sim - lp64).sum(1)]}")
    assert st["all"][1] <= k_mean * ys["all"][1], (st["all"][1], ys["all"][1])
    assert st["all"][0] <= k_max * ys["all"][0], (st["all"][0], ys["all"][0])
    assert abs(bias) <= 0.5 * ys["all"][1], (bias, ys["all"][1])
    if cid == "D":                                                    # no drift with the cache length
        for key in st:
            assert st[key][1] <= 2.0 * ys[key][1], (key, st[key][1], ys[key][1])


# (F in f32: tests/test_prefix_gpu.py::test_score_matches_float64 holds the small f32 step to float64 already)
RUNS = [(cid, dtype) for cid in "ABCDE" for dtype in ("f32", "bf16")] + [("F", "bf16")]


@pytest.mark.parametrize("cid,dtype", RUNS, ids=[f"{c}-{d}" for c, d in RUNS])
def test_forced_logprobs_against_float64(cid, dtype):
    got = device_score(cid, dtype)
    _CACHE[(cid, dtype, "lp")] = got["logprobs"]
    (check_f32 if dtype == "f32" else check_bf16)(cid, got)
    print(f"    [{cid} {dtype}] {time.time() - T0:.0f} s since the module was imported")


def test_eager_step_is_bit_identical_to_graph_replay():
    """G: case A, f32, eager launches against the captured graph."""
    if ("A", "f32", "lp") not in _CACHE:
        _CACHE[("A", "f32", "lp")] = device_score("A", "f32")["logprobs"]
    eager = device_score("A", "f32", graph=False)
    same = torch.equal(eager["logprobs"], _CACHE[("A", "f32", "lp")])
    print(f"    [G f32] eager launches against graph replay, case A, {eager['logprobs'].numel()} log p of all 16 rows: "
          f"{'bit-identical' if same else 'DIFFERENT'}")
    assert same


def test_score_of_zero_lengths_and_of_an_early_end():
    """PlankModel.score on the small fixture where its host-side sum has edges: every length 0 and a table of no positions give zero
    scores and [B, 0] log p (no step runs); a forced END stops a row's sum at that position (END's own log p included) while the
    positions behind it are still scored per token, as the step's own prefix score does."""
    import plankassembly_amd.decode as D
    c = case_dict("F")
    m = model("F", "f32")
    db = m.prepare_batch(c["batch"])
    tok, att = DL.random_forced(range(4), 36, SEED)
    for tokens, lengths in ((tok, torch.zeros(4, dtype=torch.long)), (tok[:, :0], None)):
        m._decoder = None
        with torch.no_grad():
            got = m.score(db, tokens, None if lengths is None else att, lengths)
        assert got["scores"].shape == (4,) and got["scores"].dtype == torch.float32 and float(got["scores"].abs().max()) == 0.0
        assert got["logprobs"].shape == (4, 0) and got["lengths"].tolist() == [0, 0, 0, 0]
    tok, att = tok.clone(), att.clone()
    tok[1, 20], att[1, 20] = 512, -1                                  # END at step 20 of row 1, length 30: positions 21 .. 29 are not summed
    att[1, 21:] = -1                                                  # (no pointer behind it may copy the END)
    lengths = torch.tensor([36, 30, 7, 0])
    m._decoder = D.GreedyDecoder(m, use_graph=True, strict_graph=True)
    with torch.no_grad():
        got = m.score(db, tok, att, lengths)
    running = m._decoder.last_prefix_scores
    m._decoder = None
    lp = got["logprobs"].double()
    assert bool(torch.isfinite(lp).all()) and bool((lp[1, 21:30] < 0).all()) and bool((lp[1, 30:] == 0).all()) and bool((lp[3] == 0).all())
    want = torch.stack([lp[0].sum(), lp[1, :21].sum(), lp[2, :7].sum(), lp[3].sum()])
    assert torch.equal(got["scores"], want.float()), (got["scores"], want)
    assert float((running.double() - want).abs().max()) <= 36 * 2.0 ** -24 * float(want.abs().max())
    import prefix_reference as PR
    with torch.no_grad():
        ref_sc, ref_lp = PR.score(c["sd"], c["cfg"], c["batch"], tok, att, lengths)
    assert float((got["scores"].double() - ref_sc).abs().max()) <= 1e-3 and float((lp - ref_lp).abs().max()) <= 1e-3   # (check_score's bound)


CHILDREN = {      # switches csrc/decode.hip reads once per process -> the cases whose step form they change
    "kv_cache_cross_attention": (dict(PLANK_DECODE_MQ="0", PLANK_DECODE_MQ_F32="0"), "A-f32 or A-bf16 or C-f32 or C-bf16"),
    "absorbed_bf16_self_attention_at_B16": (dict(PLANK_DECODE_MQ_SELF_BF16="1"), "A-bf16"),
    "all_bf16_step_at_d512": (dict(PLANK_DECODE_F32_RESID="0"), "A-bf16 or C-bf16"),
}


@pytest.mark.parametrize("name", list(CHILDREN))
def test_step_forms_behind_environment_switches(name, tmp_path_factory):
    """One child pytest process per setting (never two at a time), the cases above under the same bounds; the child takes its
    simulation mode from the same switches (sim_mode) and the CPU references this process and the children before it have
    computed from files in pytest's temporary directory (case C's 16 rows are evaluated once, not three times)."""
    import re
    env_add, keys = CHILDREN[name]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if "PLANK_LOGPROB_CACHE" not in os.environ:
        os.environ["PLANK_LOGPROB_CACHE"] = str(tmp_path_factory.mktemp("logprob_refs"))
    save_refs()
    env = dict(os.environ, PLANK_LOGPROB_TWO_ROWS="1", **env_add)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "tests/test_decode_logprob_gpu.py", "-k",
                        f"test_forced_logprobs_against_float64 and ({keys})"], cwd=root, env=env, capture_output=True, text=True, timeout=1500)
    print("\n".join(ln.lstrip(".") for ln in r.stdout.splitlines() if ln.lstrip(".").startswith("    [")))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    n = len(keys.split(" or "))
    assert re.search(rf"(?<![0-9]){n} passed", r.stdout) and "skipped" not in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]
