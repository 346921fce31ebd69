"""Seeded top-k / top-p sampling on the GPU (decode.SampleDecoder, include/plank_hip.h pa_decode_sample_*)."""
import ctypes as C

import pytest
import torch

import large_cases as LC
import beam_reference as BR
import sample_reference as SR
from oracle import plank_oracle as O
from test_beam_gpu import SMALL, case_model, dev, greedy, make, tiny_case

pytestmark = pytest.mark.gpu

SETTINGS = {"plain": dict(), "t0.7k8": dict(temperature=0.7, top_k=8), "p0.9": dict(top_p=0.9),
            "t1.3k50p0.95": dict(temperature=1.3, top_k=50, top_p=0.95)}


def sampler(m, N, graph=True, **kw):
    import plankassembly_amd.decode as D
    return D.SampleDecoder(m, N, use_graph=graph, strict_graph=graph, **kw)


def run(dec, batch, max_len=None, early_stop=True, seed=None):
    """The ranked result dict plus the per-row buffers (row b*N + n, before the ranking): rows_tokens / rows_attach [R, n],
    rows_scores [R]."""
    with torch.no_grad():
        r = dec.run(batch, max_len=max_len, early_stop=early_stop, seed=seed)
        n = r["sample_tokens"].shape[2]
        rows = r["sample_tokens"].shape[0] * dec.num_samples
        tok, att, _ = dec._lanes[0].buffers(rows, dec._lanes[0].key[2])          # (key[2]: the decode's Tmax)
        out = {k: v.cpu() for k, v in r.items()}
        out["rows_tokens"], out["rows_attach"] = tok[:, :n].cpu(), att[:, :n].cpu()
        out["rows_scores"] = dec._scores(rows).cpu().clone()
    return out


def assert_greedy_prefix(s, a, tok, att, N, end=512, pad=513):
    """Row b*N + n equals the greedy row b up to its first END, then PAD / -1."""
    for row in range(tok.shape[0]):
        i = row // N
        e = (s[i] == end).nonzero()
        n = int(e[0]) + 1 if len(e) else s.shape[1]
        assert torch.equal(tok[row, :n], s[i, :n]) and torch.equal(att[row, :n], a[i, :n]), (row, n)
        assert bool((tok[row, n:] == pad).all()) and bool((att[row, n:] == -1).all()), row


# ------------------------------------------------------------------------------------------ 1. top_k = 1 is greedy, bit for bit
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("graph", [False, True])
def test_top_k1_equals_greedy_small(small_fixture, dtype, graph):
    sd, batch, _ = small_fixture
    m = make(sd, dtype)
    s, a = greedy(m, dev(batch), graph)
    for tau, seed in ((0.5, 1), (2.0, 2)):
        r = run(sampler(m, 2, graph, temperature=tau, top_k=1, top_p=0.9, seed=seed), dev(batch), early_stop=False)
        assert_greedy_prefix(s, a, r["rows_tokens"], r["rows_attach"], 2)
        assert bool((r["rows_attach"] >= 0).any())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_top_k1_equals_greedy_ragged_sideface(ragged_fixture, dtype):
    sd, batch, _ = ragged_fixture
    m = make(sd, dtype)
    s, a = greedy(m, dev(batch))
    for tau, seed in ((0.5, 3), (2.0, 4)):
        r = run(sampler(m, 2, temperature=tau, top_k=1, seed=seed), dev(batch), early_stop=False)
        assert_greedy_prefix(s, a, r["rows_tokens"], r["rows_attach"], 2)


# ------------------------------------------------------------------------------------------ 2. exact f32 against float64
def compare_to_reference(r, ref, N, min_full=0.9):
    """Rows equal the reference up to their first near-boundary step; at least `min_full` of the rows have none and compare over
    their full length."""
    tok, att = r["rows_tokens"], r["rows_attach"]
    n = min(tok.shape[1], ref["tokens"].shape[1])
    R = tok.shape[0]
    full = 0
    for row in range(R):
        nz = ref["near"][row, :n].nonzero()
        stop = int(nz[0]) if len(nz) else n
        assert torch.equal(tok[row, :stop], ref["tokens"][row, :stop]) and torch.equal(att[row, :stop], ref["attach"][row, :stop]), \
            (row, stop, tok[row], ref["tokens"][row])
        full += stop == n
    assert full >= min_full * R, (full, R)


def check_scores_teacher_forced(sd, cfg, batch, r, N, atol):
    tok, att = r["rows_tokens"], r["rows_attach"]
    R, n = tok.shape
    with torch.no_grad():
        tf = BR.teacher_forced_logprob(sd, cfg, batch, tok.view(R // N, N, n), att.view(R // N, N, n))
    d = (tf.view(-1) - r["rows_scores"].double()).abs()
    assert float(d.max()) <= atol, (float(d.max()), tf.view(-1), r["rows_scores"])
    return d


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_f32_matches_float64_reference_small(small_fixture, setting):
    sd, batch, _ = small_fixture
    m = make(sd, "f32")
    cfg = O.OracleCfg(**SMALL)
    for seed in (1, 2):
        r = run(sampler(m, 4, seed=seed, **SETTINGS[setting]), dev(batch), early_stop=False)
        with torch.no_grad():
            ref = SR.sample_decode(sd, cfg, batch, 4, seed=seed, max_steps=36, early_stop=False, **SETTINGS[setting])
        compare_to_reference(r, ref, 4)
        check_scores_teacher_forced(sd, cfg, batch, r, 4, 1e-3)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_f32_matches_float64_reference_tiny(setting):
    """The tiny fixture is untrained: its distribution is close to uniform over ~600 candidates, each ~1.6e-3 of W, so the 1e-4 W
    margin around u W of section 13 flags ~12 % of its draws and nearly every row of 24 steps (measured on the reference, seeds 1
    and 2: 49 of 64 rows).  Its near-boundary margin is 1e-6 instead: at that margin the reference flags 2 of those 64 rows, and the
    f32 p and prefix sums of the exact-f32 step agree with float64 far below it."""
    sd, batch, cfg = tiny_case()
    m = make(sd, "f32", 128, 8, 256, 2, 2, 1200, 128)
    db = m.prepare_batch(batch)
    for seed in (1, 2):
        r = run(sampler(m, 2, seed=seed, **SETTINGS[setting]), db, max_len=24, early_stop=False)
        with torch.no_grad():
            ref = SR.sample_decode(sd, cfg, batch, 2, seed=seed, max_steps=24, early_stop=False, tol=1e-6, **SETTINGS[setting])
        compare_to_reference(r, ref, 2, min_full=0.85)
        check_scores_teacher_forced(sd, cfg, batch, r, 2, 1e-3)


# ------------------------------------------------------------------------------------------ 3. determinism
def test_determinism_and_seed_change_without_recapture():
    sd, batch, _ = tiny_case()
    m = make(sd, "f32", 128, 8, 256, 2, 2, 1200, 128)
    db = m.prepare_batch(batch)
    kw = dict(temperature=1.3, top_k=50, top_p=0.95)
    dec = sampler(m, 4, seed=1, **kw)
    a = run(dec, db, max_len=16)
    g = dec._graph
    b = run(dec, db, max_len=16)
    assert dec._graph is g
    for k in a:
        assert torch.equal(a[k], b[k]), k
    e = run(sampler(m, 4, graph=False, seed=1, **kw), db, max_len=16)
    for k in a:
        assert torch.equal(a[k], e[k]), k
    s2 = run(dec, db, max_len=16, seed=2)                                      # pa_decode_sample_set on the captured step
    assert dec._graph is g
    f2 = run(sampler(m, 4, seed=2, **kw), db, max_len=16)
    for k in f2:
        assert torch.equal(s2[k], f2[k]), k
    # the decoder's own seed again after a per-call seed
    c = run(dec, db, max_len=16)
    assert torch.equal(c["rows_tokens"], a["rows_tokens"])
    # tau = 1, two seeds: different samples somewhere
    p1 = run(sampler(m, 4, seed=1), db, max_len=16)
    p2 = run(sampler(m, 4, seed=2), db, max_len=16)
    assert not torch.equal(p1["rows_tokens"], p2["rows_tokens"])


# ------------------------------------------------------------------------------------------ 4. / 5. bf16 properties
def check_properties(r, batch, sd_cfg, N, early_stop_run, nats_per_token, end=512, pad=513, vocab=514):
    tok, att, sc = r["rows_tokens"], r["rows_attach"], r["rows_scores"]
    R, n = tok.shape
    assert bool(((tok >= 0) & (tok < vocab)).all())
    assert bool(torch.isfinite(sc).all()) and bool((sc <= 0).all())
    lengths = []
    for row in range(R):
        e = (tok[row] == end).nonzero()
        live = int(e[0]) + 1 if len(e) else n
        lengths.append(live)
        assert bool((tok[row, live:] == pad).all()) and bool((att[row, live:] == -1).all()), row
        for t in (att[row, :live] >= 0).nonzero()[:, 0].tolist():
            j = int(att[row, t])
            assert j < t and int(tok[row, t]) == int(tok[row, j]), (row, t, j)      # (disallowed j carry the 1e-6 fill: drawable)
    assert r["sample_tokens"].shape[2] == early_stop_run["sample_tokens"].shape[2]
    for k in r:
        assert torch.equal(r[k], early_stop_run[k]), k
    # ranking: alpha = 0 orders by score
    assert bool((r["scores"][:, :-1] >= r["scores"][:, 1:]).all())
    if sd_cfg is not None:
        sd, cfg = sd_cfg
        with torch.no_grad():
            tf = BR.teacher_forced_logprob(sd, cfg, batch, tok.view(R // N, N, n), att.view(R // N, N, n))
        per_tok = ((tf.view(-1) - sc.double()).abs() / torch.tensor(lengths, dtype=torch.float64))
        assert float(per_tok.mean()) <= nats_per_token, float(per_tok.mean())
        return float(per_tok.mean())


def headline_case(B):
    c = LC.CASES["headline"]
    m = case_model("headline", "bf16")
    db = m.prepare_batch(LC.case_batch(c, decode=True, batch_size=B))
    return c, m, db


def test_properties_b16_n8_bf16():
    """B 16 x N 8, Tmax 128, bf16 (the headline model's decode shape): tokens in range, attach < t pointing at an equal token,
    rows frozen after END, the same result with and without early stop, and scores within a mean of 0.05 nats per token of the
    float64 teacher-forced log-likelihood of the same sequences (the headline case's float64 reference is too slow for the
    suite, so the bound is checked on the small fixture's bf16 samples, B 4 x N 8)."""
    _, m, db = headline_case(16)
    dec = sampler(m, 8, temperature=0.8, top_k=50, top_p=0.95, seed=3)
    r = run(dec, db, max_len=128, early_stop=False)
    r2 = run(dec, db, max_len=128, early_stop=True)
    assert r["sample_tokens"].shape[:2] == (16, 8)
    check_properties(r, db, None, 8, r2, None)


def test_bf16_scores_against_float64_small(small_fixture):
    sd, batch, _ = small_fixture
    m = make(sd, "bf16")
    dec = sampler(m, 8, seed=9)
    r = run(dec, dev(batch), early_stop=False)
    r2 = run(dec, dev(batch))
    got = check_properties(r, batch, (sd, O.OracleCfg(**SMALL)), 8, r2, 0.05)
    print(f"    bf16 score error: mean {got:.4f} nats per token")


def test_t1024_samples():
    """B 16 x N 4 at Tmax 1024 (bf16): the properties of the B 16 x N 8 test over the long decode."""
    c = LC.CASES["t1024"]
    m = case_model("t1024", "bf16")
    db = m.prepare_batch(LC.case_batch(c, decode=True, batch_size=16))
    dec = sampler(m, 4, seed=5)
    r = run(dec, db, early_stop=False)
    r2 = run(dec, db)
    assert r["sample_tokens"].shape[:2] == (16, 4)
    check_properties(r, db, None, 4, r2, None)


# ------------------------------------------------------------------------------------------ 6. surface and errors
def test_model_sample_and_eval_step(small_fixture):
    from plankassembly_amd.config import CfgNode
    from plankassembly_amd.models import build_model
    sd, batch, _ = small_fixture
    model = dict(NUM_MODEL=64, NUM_HEAD=4, NUM_FEEDFORWARD=128, DROPOUT=0.0, ACTIVATION="relu", NORMALIZE_BEFORE=True,
                 NUM_ENCODER_LAYERS=2, NUM_DECODER_LAYERS=2, COMPUTE_DTYPE="f32", NUM_SAMPLES=4, TEMPERATURE=1.5, TOP_K=20,
                 SAMPLE_SEED=7)
    data = dict(NUM_VIEW=3, NUM_TYPE=2, NUM_INPUT_DOF=4, NUM_OUTPUT_DOF=6, MAX_INPUT_LENGTH=65, MAX_OUTPUT_LENGTH=36,
                VOCAB_SIZE=514)
    m = build_model(CfgNode(dict(MODEL=model, DATA=data, TOKEN=dict(END=512, PAD=513))))
    m.load_state_dict(sd)
    m = m.cuda().eval()
    with torch.no_grad():
        out = m(dev(batch))
        out2 = m(dev(batch))
        direct = m.sample(dev(batch), 4, temperature=1.5, top_k=20, seed=7)
    assert {"samples", "attach", "predicts", "groundtruths", "scores", "sample_tokens", "sample_attach"} <= set(out)
    assert out["scores"].shape == (4, 4)
    ref = run(sampler(m, 4, temperature=1.5, top_k=20, seed=7), dev(batch))
    for o in (out, out2, direct):
        assert torch.equal(o["samples"].cpu(), ref["tokens"]) and torch.equal(o["attach"].cpu(), ref["attach"])
        assert torch.equal(o["scores"].cpu(), ref["scores"]) and torch.equal(o["sample_tokens"].cpu(), ref["sample_tokens"])
    assert torch.equal(out["samples"].cpu(), out["sample_tokens"][:, 0].cpu())
    for i, pr in enumerate(out["predicts"]):
        assert torch.equal(pr.cpu(), m.parse_sequence(ref["tokens"][i].cuda()).cpu())


def test_invalid_parameters_raise(small_fixture):
    import plankassembly_amd.decode as D
    from plankassembly_amd import _lib as L
    sd, batch, _ = small_fixture
    m = make(sd)
    for bad in (dict(num_samples=0), dict(num_samples=65), dict(num_samples=2, temperature=0.0),
                dict(num_samples=2, temperature=float("inf")), dict(num_samples=2, top_k=-1), dict(num_samples=2, top_p=0.0),
                dict(num_samples=2, top_p=1.5)):
        with pytest.raises(ValueError):
            D.SampleDecoder(m, **bad)
    dec = sampler(m, 2)
    dec.begin(dev(batch))
    lib, h, st = L.lib(), dec._lanes[0].h(), L.stream()
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    base = C.c_void_p((ws.data_ptr() + 255) // 256 * 256)
    good = dict(seed=1, n_per_drawing=2, temperature=1.0, top_k=0, top_p=1.0)
    for field, v in (("n_per_drawing", 0), ("n_per_drawing", 65), ("n_per_drawing", 3), ("temperature", 0.0),
                     ("temperature", -1.0), ("temperature", float("nan")), ("temperature", float("inf")), ("top_k", -1),
                     ("top_p", 0.0), ("top_p", 1.01)):
        p = L.SampleParams(**{**good, field: v})
        with pytest.raises(L.PlankHipError):
            L.check(lib.pa_decode_sample_begin(h, C.byref(p), base, C.c_int64(1 << 15), st), f"begin {field}={v}")
        with pytest.raises(L.PlankHipError):
            L.check(lib.pa_decode_sample_set(h, C.byref(p), st), f"set {field}={v}")
    with pytest.raises(L.PlankHipError):                                      # workspace too small
        L.check(lib.pa_decode_sample_begin(h, C.byref(L.SampleParams(**good)), base, C.c_int64(256), st), "small ws")
    fresh = m.new_bound_handle()
    try:
        with pytest.raises(L.PlankHipError):                                  # a decode that was not begun
            L.check(lib.pa_decode_sample_begin(fresh, C.byref(L.SampleParams(**good)), base, C.c_int64(1 << 15), st), "no decode")
    finally:
        lib.pa_model_destroy(fresh)
    torch.cuda.synchronize()


def test_modes_replace_each_other_and_two_lanes_refuse(small_fixture):
    import plankassembly_amd.decode as D
    from plankassembly_amd import _lib as L
    sd, batch, _ = small_fixture
    m = make(sd)
    s, a = greedy(m, dev(batch))
    dec = sampler(m, 2, seed=4)
    dec.begin(dev(batch))
    h, st = dec._lanes[0].h(), L.stream()
    assert dec.max_lanes == 1 and dec._active == 1                              # sampling runs as one lane
    # beam begin after sample begin: beam mode (sample buffers refused); sample begin after beam begin: sampling mode
    bws = torch.empty(int(L.lib().pa_decode_beam_ws_bytes(h, 8, 65, 36, 2)) + 256, dtype=torch.uint8, device="cuda")
    bbase = C.c_void_p((bws.data_ptr() + 255) // 256 * 256)
    L.check(L.lib().pa_decode_beam_begin(h, 2, bbase, C.c_int64(bws.numel() - 256), st), "beam begin")
    p = C.c_void_p()
    assert L.lib().pa_decode_sample_buffers(h, C.byref(p)) != 0
    L.check(L.lib().pa_decode_beam_buffers(h, C.byref(p), C.byref(C.c_void_p()), C.byref(C.c_void_p())), "beam buffers")
    r = run(dec, dev(batch), early_stop=False)                                  # (begin: sample mode again)
    assert L.lib().pa_decode_beam_buffers(h, C.byref(p), C.byref(C.c_void_p()), C.byref(C.c_void_p())) != 0
    ref = run(sampler(make(sd), 2, seed=4), dev(batch), early_stop=False)
    assert torch.equal(r["rows_tokens"], ref["rows_tokens"])
    # a greedy run on the same handle after sampling gives the greedy tokens
    s2, a2 = greedy(m, dev(batch))
    assert torch.equal(s2, s) and torch.equal(a2, a)
    torch.cuda.synchronize()
