"""Beam-search decode on the GPU (decode.BeamDecoder, include/plank_hip.h pa_decode_beam_*)."""
import types

import numpy as np
import pytest
import torch

import large_cases as LC
import beam_reference as BR
from conftest import load_fixture
from oracle import plank_oracle as O

pytestmark = pytest.mark.gpu

TOKEN = types.SimpleNamespace(END=512, PAD=513)
SMALL = dict(d_model=64, n_head=4, d_ff=128, n_enc=2, n_dec=2, max_input_length=65, max_output_length=36)


def make(sd, dtype="f32", d=64, h=4, ff=128, ne=2, nd=2, max_in=65, max_out=36, **kw):
    from plankassembly_amd.models import PlankModel
    m = PlankModel(d, h, ff, 0.0, "relu", True, ne, nd, 3, 2, 4, 6, max_in, max_out, 514, TOKEN, compute_dtype=dtype, **kw)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    m._ensure_handle()
    m._refresh_shadow()
    return m


def case_model(name, dtype):
    c = LC.CASES[name]
    return make(LC.case_state_dict(c), dtype, c["d"], c["h"], c["ff"], c["ne"], c["nd"], c["max_in"], c["max_out"])


def tiny_case():
    from plankassembly_amd.data import SynthSpec, synth_batch
    sd, _, g = load_fixture("fixture_tiny.npz")
    batch = synth_batch(4, SynthSpec(1200, 128, (8, 299), (2, 21), True), seed=int(g["g8::seed"]))
    batch.pop("name")
    cfg = O.OracleCfg(d_model=128, n_head=8, d_ff=256, n_enc=2, n_dec=2, max_input_length=1200, max_output_length=128)
    return sd, batch, cfg


def dev(batch):
    return {k: v.cuda() for k, v in batch.items()}


def greedy(m, batch, graph=True, max_len=None):
    import plankassembly_amd.decode as D
    with torch.no_grad():
        s, a = D.GreedyDecoder(m, use_graph=graph, strict_graph=graph).run(batch, max_len=max_len, early_stop=False)
    return s.cpu(), a.cpu()


def beam(m, batch, K, graph=True, max_len=None, early_stop=True, alpha=0.0, dec=None):
    import plankassembly_amd.decode as D
    dec = dec or D.BeamDecoder(m, K, alpha, use_graph=graph, strict_graph=graph)
    with torch.no_grad():
        r = dec.run(batch, max_len=max_len, early_stop=early_stop)
    return {k: v.cpu() for k, v in r.items()}


def assert_k1_is_greedy(s, a, r, end=512):
    bt, ba = r["beam_tokens"][:, 0], r["beam_attach"][:, 0]
    for i in range(s.shape[0]):
        e = (s[i] == end).nonzero()
        n = int(e[0]) + 1 if len(e) else s.shape[1]
        assert bt.shape[1] >= n
        assert torch.equal(bt[i, :n], s[i, :n]) and torch.equal(ba[i, :n], a[i, :n]), (i, n)


# ------------------------------------------------------------------------------------------ 1. K = 1 is greedy, bit for bit
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("graph", [False, True])
def test_k1_equals_greedy_small(small_fixture, dtype, graph):
    sd, batch, _ = small_fixture
    m = make(sd, dtype)
    s, a = greedy(m, dev(batch), graph)
    r = beam(m, dev(batch), 1, graph, early_stop=False)
    assert_k1_is_greedy(s, a, r)
    assert bool((r["beam_attach"] >= 0).any())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_k1_equals_greedy_ragged_sideface(ragged_fixture, dtype):
    sd, batch, _ = ragged_fixture
    m = make(sd, dtype)
    s, a = greedy(m, dev(batch))
    assert_k1_is_greedy(s, a, beam(m, dev(batch), 1, early_stop=False))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("graph", [False, True])
def test_k1_equals_greedy_headline_rows(dtype, graph):
    c = LC.CASES["headline"]
    m = case_model("headline", dtype)
    db = m.prepare_batch(LC.case_batch(c, decode=True, batch_size=4))
    s, a = greedy(m, db, graph)
    assert_k1_is_greedy(s, a, beam(m, db, 1, graph, early_stop=False))


# ------------------------------------------------------------------------------------------ 2. K = 4 / 8 against float64
def compare_to_reference(r, ref, K):
    B = ref["scores"].shape[0]
    allowed = 0
    for b in range(B):
        n = min(r["beam_tokens"].shape[2], ref["beam_tokens"].shape[2])
        same = (torch.equal(r["beam_tokens"][b, :, :n], ref["beam_tokens"][b, :, :n])
                and torch.equal(r["beam_attach"][b, :, :n], ref["beam_attach"][b, :, :n])
                and torch.equal(r["finished"][b], ref["finished"][b]))
        if same:
            d = (r["scores"][b].double() - ref["scores"][b]).abs()
            fin = torch.isfinite(ref["scores"][b])
            assert bool(torch.equal(torch.isfinite(r["scores"][b]), fin)) and float(d[fin].max()) <= 1e-4, (b, r["scores"][b], ref["scores"][b])
            continue
        neq = ((r["beam_tokens"][b, :, :n] != ref["beam_tokens"][b, :, :n]) | (r["beam_attach"][b, :, :n] != ref["beam_attach"][b, :, :n]))
        t0 = int(neq.any(0).nonzero()[0]) if bool(neq.any()) else n - 1
        sc = ref["scores"][b]
        rank_tie = bool(((sc[:-1] - sc[1:]).abs() <= 1e-5).any())
        print(f"    drawing {b}: beams diverge from step {t0}; reference near-tie before it: {bool(ref['near_tie'][b, :t0 + 1].any())}")
        assert bool(ref["near_tie"][b, :t0 + 1].any()) or rank_tie, f"drawing {b} diverges at step {t0} without a near-tie"
        allowed += 1
    assert allowed <= 1, allowed


@pytest.mark.parametrize("K", [4, 8])
def test_beams_f32_match_float64_reference_small(small_fixture, K):
    sd, batch, _ = small_fixture
    m = make(sd, "f32")
    r = beam(m, dev(batch), K)
    with torch.no_grad():
        ref = BR.beam_search(sd, O.OracleCfg(**SMALL), batch, K)
    assert r["beam_tokens"].shape[:2] == (4, K)
    compare_to_reference(r, ref, K)


@pytest.mark.parametrize("K", [4, 8])
def test_beams_f32_match_float64_reference_tiny(K):
    sd, batch, cfg = tiny_case()
    m = make(sd, "f32", 128, 8, 256, 2, 2, 1200, 128)
    db = m.prepare_batch(batch)
    r = beam(m, db, K, max_len=24)
    with torch.no_grad():
        ref = BR.beam_search(sd, cfg, batch, K, max_steps=24)
    compare_to_reference(r, ref, K)


# ------------------------------------------------------------------------------------------ 3. bf16 against f32
def test_bf16_k4_best_beam_mostly_agrees(small_fixture):
    sd, batch, _ = small_fixture
    r32 = beam(make(sd, "f32"), dev(batch), 4)
    r16 = beam(make(sd, "bf16"), dev(batch), 4)
    n = min(r32["tokens"].shape[1], r16["tokens"].shape[1])
    agree = (r16["tokens"][:, :n] == r32["tokens"][:, :n]).float().mean().item()
    assert agree > 0.9, agree


# ------------------------------------------------------------------------------------------ 4. properties at B 16 x K 8 x Tmax 128
def check_properties(r, K, end=512, pad=513):
    B, _, n = r["beam_tokens"].shape
    assert bool((r["scores"][:, :-1] >= r["scores"][:, 1:]).all())              # alpha = 0: final order is score order
    pm = O.pointer_mask(O.OracleCfg(), max(n, 6))
    for b in range(B):
        for k in range(K):
            tk, at = r["beam_tokens"][b, k], r["beam_attach"][b, k]
            e = (tk == end).nonzero()
            if len(e):
                e = int(e[0])
                assert bool((tk[e + 1:] == pad).all()) and bool((at[e + 1:] == -1).all())
                assert bool(r["finished"][b, k]) and int(r["lengths"][b, k]) == e + 1
                live = e + 1
            else:
                live = n
            for t in (at[:live] >= 0).nonzero()[:, 0].tolist():
                j = int(at[t])
                assert j < t and pm[t, j] == 1, (b, k, t, j)
                assert int(tk[t]) == int(tk[j]), (b, k, t, j)


def test_properties_b16_k8_bf16_graph():
    import plankassembly_amd.decode as D
    c = LC.CASES["headline"]
    m = case_model("headline", "bf16")
    db = m.prepare_batch(LC.case_batch(c, decode=True, batch_size=16))
    dec = D.BeamDecoder(m, 8, use_graph=True, strict_graph=True)
    r = beam(m, db, 8, dec=dec)
    assert r["beam_tokens"].shape[:2] == (16, 8)
    assert bool(torch.isfinite(r["scores"]).all())
    check_properties(r, 8)
    r2 = beam(m, db, 8, dec=dec)                                                   # graph reuse
    g = dec._graph
    for k in r:
        assert torch.equal(r[k], r2[k]), k
    r3 = beam(m, db, 8, dec=dec, early_stop=False)
    assert dec._graph is g
    for k in r:
        assert torch.equal(r[k], r3[k]), k


def test_t1024_beams():
    """The 1024-step decode shape: K = 1 is greedy over all 1024 steps; K = 4 (history reorder up to t = 1023) keeps every
    beam consistent."""
    c = LC.CASES["t1024"]
    m = case_model("t1024", "bf16")
    db = m.prepare_batch(LC.case_batch(c, decode=True, batch_size=2))
    s, a = greedy(m, db)
    r1 = beam(m, db, 1, early_stop=False)
    assert_k1_is_greedy(s, a, r1)
    r = beam(m, db, 4)
    assert r["beam_tokens"].shape == (2, 4, 1024)
    assert bool(torch.isfinite(r["scores"]).all())
    check_properties(r, 4)


# ------------------------------------------------------------------------------------------ 5. model surface
def test_model_eval_routes_through_beam_search(small_fixture):
    import plankassembly_amd.decode as D
    sd, batch, _ = small_fixture
    m = make(sd, "f32", beam_size=4)
    with torch.no_grad():
        out = m(dev(batch))
    assert {"samples", "attach", "predicts", "groundtruths", "scores"} <= set(out)
    r = beam(m, dev(batch), 4)
    assert torch.equal(out["samples"].cpu(), r["tokens"]) and torch.equal(out["attach"].cpu(), r["attach"])
    assert torch.equal(out["scores"].cpu(), r["scores"])
    for i, pr in enumerate(out["predicts"]):
        assert torch.equal(pr.cpu(), m.parse_sequence(r["tokens"][i].cuda()).cpu())
    g = make(sd, "f32")
    with torch.no_grad():
        og = g(dev(batch))
        s, a = D.GreedyDecoder(g).run(dev(batch))
    assert "scores" not in og
    assert torch.equal(og["samples"], s) and torch.equal(og["attach"], a)


# ------------------------------------------------------------------------------------------ 6. errors
@pytest.mark.parametrize("K", [0, 17])
def test_invalid_beam_size_raises(small_fixture, K):
    import plankassembly_amd.decode as D
    from plankassembly_amd._lib import PlankHipError
    sd, _, _ = small_fixture
    with pytest.raises(PlankHipError):
        D.BeamDecoder(make(sd), K)


def test_beams_refuse_two_lanes(small_fixture, monkeypatch):
    """Beams run as one lane whatever PLANK_DECODE_LANES says (the library call that stepped two lanes in turns, and refused a handle
    in beam mode, is gone; this is what remains to refuse)."""
    import plankassembly_amd.decode as D
    sd, batch, _ = small_fixture
    m = make(sd)
    monkeypatch.setenv("PLANK_DECODE_LANES", "2")
    dec = D.BeamDecoder(m, 2)
    dec.begin(dev(batch))
    assert dec.max_lanes == 1 and dec._active == 1
    torch.cuda.synchronize()
