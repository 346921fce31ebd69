"""Forced-prefix decoding and sequence scoring on the GPU (include/plank_hip.h pa_decode_prefix_*, decode.prefix_table,
PlankModel.score / complete)."""
import ctypes as C

import numpy as np
import pytest
import torch

import large_cases as LC
import prefix_reference as PR
import test_beam_gpu as BG
import test_sample_gpu as SG
from oracle import plank_oracle as O
from test_beam_gpu import SMALL, case_model, dev, make, tiny_case
from test_prefix_cpu import gt_prefix

pytestmark = pytest.mark.gpu

V, END, PAD = 514, 512, 513


def D():
    import plankassembly_amd.decode as d
    return d


def greedy_dec(m, graph=True):
    return D().GreedyDecoder(m, use_graph=graph, strict_graph=graph)


def grun(dec, batch, prefix=None, max_len=None, early_stop=False):
    with torch.no_grad():
        s, a = dec.run(batch, max_len=max_len, early_stop=early_stop, prefix=prefix)
    ps, pl = dec.last_prefix_scores, dec.last_prefix_logprobs
    return s.cpu(), a.cpu(), (None if ps is None else ps.clone()), (None if pl is None else pl.clone())


def first_end(s):
    e = (s == END)
    return torch.where(e.any(1), e.long().argmax(1), torch.full((s.shape[0],), -1))


def same_dict(a, b, keys=None):
    for k in keys or a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------ 1. no table / empty table
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("graph", [False, True])
def test_no_table_and_empty_table_change_nothing(small_fixture, dtype, graph):
    sd, batch, _ = small_fixture
    m = make(sd, dtype)
    db = dev(batch)
    empty = {"tokens": torch.zeros(4, 0, dtype=torch.long)}
    zero_len = {"tokens": batch["output_value"][:, :12], "lengths": [0, 0, 0, 0]}
    s, a, ps, _ = grun(greedy_dec(m, graph), db)
    assert ps is None
    for pre in (empty, zero_len):
        dec = greedy_dec(m, graph)
        s2, a2, ps2, pl2 = grun(dec, db, pre)
        assert torch.equal(s2, s) and torch.equal(a2, a)
        assert float(ps2.abs().max()) == 0.0 and float(pl2.abs().max()) == 0.0
        s3, a3, ps3, _ = grun(dec, db)                               # the same decoder without a prefix again
        assert torch.equal(s3, s) and torch.equal(a3, a) and ps3 is None
    b0 = BG.beam(m, db, 4, graph)
    assert float(b0["prefix_scores"].abs().max()) == 0.0
    r0 = SG.run(SG.sampler(m, 4, graph, seed=3, top_k=20), db)
    for pre in (empty, zero_len):
        with torch.no_grad():
            b1 = {k: v.cpu() for k, v in D().BeamDecoder(m, 4, use_graph=graph, strict_graph=graph).run(db, prefix=pre).items()}
            r1 = {k: v.cpu() for k, v in SG.sampler(m, 4, graph, seed=3, top_k=20).run(db, prefix=pre).items()}
        same_dict(b0, b1)
        same_dict(r1, r0, keys=r1)


# ------------------------------------------------------------------------------------------ 2. self-consistency, bit-exact
def check_self_consistency(m, db, s, a, Tmax, lengths_list, graph=True):
    """Forcing greedy's own output gives it back bit for bit; K = 1 beam and top_k = 1, N = 1 sampling (the same row count) give its
    tokens up to each row's first END, the forced positions' score bit for bit."""
    B = s.shape[0]
    fe = first_end(s)
    gdec, bdec, sdec = greedy_dec(m, graph), D().BeamDecoder(m, 1, use_graph=graph, strict_graph=graph), SG.sampler(m, 1, graph, top_k=1, seed=5)
    for lengths in lengths_list:
        lengths = torch.as_tensor(lengths)
        pre = {"tokens": s, "attach": a, "lengths": lengths}
        s2, a2, ps, pl = grun(gdec, db, pre, max_len=Tmax)
        assert torch.equal(s2, s) and torch.equal(a2, a), lengths
        assert bool(torch.isfinite(ps).all()) and bool((pl <= 0).all())
        for r in range(B):
            n = int(lengths[r])
            assert bool((pl[r, n:] == 0).all()) and (n == 0 or bool((pl[r, :n] < 0).any()))
        with torch.no_grad():
            rb = {k: v.cpu() for k, v in bdec.run(db, max_len=Tmax, early_stop=False, prefix=pre).items()}
            rs = {k: v.cpu() for k, v in sdec.run(db, max_len=Tmax, early_stop=False, prefix=pre).items()}
        BG.assert_k1_is_greedy(s, a, rb)
        SG.assert_greedy_prefix(s, a, rs["sample_tokens"][:, 0], rs["sample_attach"][:, 0], 1)
        for r in (rb, rs):
            assert torch.equal(r["prefix_scores"][:, 0], ps), (r["prefix_scores"][:, 0], ps)
            for i in range(B):
                if fe[i] >= 0 and int(lengths[i]) > int(fe[i]):      # forced through its END: the whole score is the prefix score
                    assert float(r["scores"][i, 0]) == float(ps[i]), (i, r["scores"][i, 0], ps[i])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("graph", [False, True])
def test_forcing_greedys_own_output_small(small_fixture, dtype, graph):
    sd, batch, _ = small_fixture
    m = make(sd, dtype)
    db = dev(batch)
    s, a, _, _ = grun(greedy_dec(m, graph), db)
    assert bool((a >= 0).any())
    fe = first_end(s)
    mix = [0, min(int(fe[1]) + 3, 36) if fe[1] >= 0 else 36, 7, 36]
    check_self_consistency(m, db, s, a, 36, [[P] * 4 for P in (1, 5, 6, 7, 36)] + [mix], graph)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_forcing_greedys_own_output_headline_rows(dtype):
    c = LC.CASES["headline"]
    m = case_model("headline", dtype)
    db = m.prepare_batch(LC.case_batch(c, decode=True, batch_size=4))
    s, a, _, _ = grun(greedy_dec(m), db)
    fe = first_end(s)
    beyond = min(int(fe[1]) + 3, 128) if fe[1] >= 0 else 128
    check_self_consistency(m, db, s, a, 128, [[P] * 4 for P in (1, 5, 6, 7, 64)] + [[0, beyond, 7, 64]])


# ------------------------------------------------------------------------------------------ 3. scores against float64
WORST = {"cum": 0.0, "tok": 0.0}


def check_score(m, db, sd, cfg, batch, tokens, attach, lengths=None):
    with torch.no_grad():
        got = m.score(db, tokens, attach, lengths)
        ref_sc, ref_lp = PR.score(sd, cfg, batch, tokens.cpu(), None if attach is None else attach.cpu(), lengths)
    n = ref_lp.shape[1]
    assert got["logprobs"].shape == ref_lp.shape and got["scores"].dtype == torch.float32
    fin = torch.isfinite(ref_lp)
    assert torch.equal(torch.isfinite(got["logprobs"]), fin)
    d_tok = (got["logprobs"].double() - ref_lp)[fin].abs().max()
    fs = torch.isfinite(ref_sc)
    assert torch.equal(torch.isfinite(got["scores"]), fs)
    d_cum = (got["scores"].double() - ref_sc)[fs].abs().max() if bool(fs.any()) else torch.tensor(0.0)
    WORST["cum"], WORST["tok"] = max(WORST["cum"], float(d_cum)), max(WORST["tok"], float(d_tok))
    print(f"    score against float64: cumulative {float(d_cum):.3e}, per token {float(d_tok):.3e} (n {n}; worst so far "
          f"{WORST['cum']:.3e} / {WORST['tok']:.3e})")
    assert float(d_cum) <= 1e-3 and float(d_tok) <= 1e-3, (float(d_cum), float(d_tok))
    return got, ref_lp


def gt_attach(batch):
    lab = batch["output_label"]
    return torch.where(lab >= V, lab - V, torch.full_like(lab, -1))


@pytest.mark.parametrize("name", ["small", "ragged", "tiny"])
def test_score_matches_float64(name, small_fixture, ragged_fixture):
    if name == "tiny":
        sd, batch, cfg = tiny_case()
        m = make(sd, "f32", 128, 8, 256, 2, 2, 1200, 128)
        db = m.prepare_batch(batch)
        cut = 24                                                     # (the float64 reference of the tiny case: 24 steps, as its other tests)
    else:
        sd, batch, _ = small_fixture if name == "small" else ragged_fixture
        cfg = O.OracleCfg(**SMALL)
        m = make(sd, "f32")
        db = dev(batch)
        cut = 36
    B = batch["output_value"].shape[0]
    # greedy's own output
    s, a, _, _ = grun(greedy_dec(m), db, max_len=cut)
    check_score(m, db, sd, cfg, batch, s, a)
    # ground truth: with the pointers of output_label (score()'s default), and as vocab entries only
    tok, att = batch["output_value"][:, :cut], gt_attach(batch)[:, :cut]
    lengths = torch.tensor([min(PR.default_length(tok[r], cfg), cut) for r in range(B)])
    got, ref_lp = check_score(m, db, sd, cfg, batch, tok, att, lengths)
    if cut == batch["output_value"].shape[1]:
        with torch.no_grad():
            dflt = m.score(db)
        assert torch.equal(dflt["scores"], got["scores"]) and torch.equal(dflt["logprobs"], got["logprobs"])
        assert torch.equal(dflt["lengths"], lengths)
    check_score(m, db, sd, cfg, batch, tok, None, lengths)


def test_score_fill_and_missing_candidates(small_fixture):
    """A pointer the eval branch disallows scores the 1e-6 fill: logf(1e-6f), whatever the model; a pointer that is no candidate at its
    step scores -inf; nothing is refused."""
    sd, batch, _ = small_fixture
    cfg = O.OracleCfg(**SMALL)
    m = make(sd, "f32")
    tok, att = batch["output_value"].clone(), gt_attach(batch)
    lengths = torch.tensor([12, 30, 12, 18])
    att[0, 7], att[1, 8], att[2, 9], att[3, 13] = 0, 7, 1, 6         # disallowed by ptr_allowed(i, j): the fill
    att[1, 3], att[3, 10] = 1, 11                                    # t < 5; attach >= t
    got, ref_lp = check_score(m, dev(batch), sd, cfg, batch, tok, att, lengths)
    # logf(1e-6f) is the device's logf, which is not correctly rounded (within one ulp): every fill position carries the same bits,
    # whatever the row and step, and that value is within one float32 ulp of ln(1e-6f)
    fill = np.float32(np.log(np.float64(np.float32(1e-6))))
    vals = {float(got["logprobs"][r, t]) for r, t in ((0, 7), (1, 8), (2, 9), (3, 13))}
    for r, t in ((0, 7), (1, 8), (2, 9), (3, 13)):
        assert abs(float(ref_lp[r, t]) - float(np.log(1e-6))) < 1e-12
    print(f"    fill lp {vals!r} (float32 nearest to ln(1e-6f): {float(fill)!r})")
    assert len(vals) == 1 and abs(vals.pop() - float(fill)) <= float(np.spacing(np.abs(fill))), vals
    assert got["logprobs"][1, 3] == float("-inf") and got["logprobs"][3, 10] == float("-inf")
    assert got["scores"][1] == float("-inf") and got["scores"][3] == float("-inf")
    assert bool(torch.isfinite(got["scores"][[0, 2]]).all())


# ------------------------------------------------------------------------------------------ 4. the scorer against the decoders
def score_hypotheses(m32, batch_or_db, tokens, attach, K):
    """score() takes one sequence per batch row: the K hypotheses of a drawing are scored on the batch repeated K times."""
    B, _, n = tokens.shape
    rep = D()._repeat_batch(batch_or_db, K)
    if m32.unpad:
        rep = m32.prepare_batch(rep, groups=False)
    with torch.no_grad():
        return m32.score(rep, tokens.reshape(B * K, n), attach.reshape(B * K, n))


def test_score_of_beam_and_sample_outputs_small(small_fixture):
    sd, batch, _ = small_fixture
    m = make(sd, "f32")
    db = dev(batch)
    rb = BG.beam(m, db, 4)
    rs = SG.run(SG.sampler(m, 4, seed=2, temperature=1.2, top_k=40), db)
    for name, r, tk, at in (("beam", rb, rb["beam_tokens"], rb["beam_attach"]), ("sample", rs, rs["sample_tokens"], rs["sample_attach"])):
        sc = score_hypotheses(m, db, tk, at, 4)
        fin = torch.isfinite(r["scores"].view(-1))
        assert bool(fin.any())
        d = (sc["scores"].double() - r["scores"].view(-1).double())[fin].abs().max()
        print(f"    {name}: score() against the decoder's own scores: {float(d):.3e}")
        assert float(d) <= 1e-3, float(d)


# ------------------------------------------------------------------------------------------ 5. completion against float64
def prefix_dict(pre, B, rows):
    plen, tok, att = (x[::rows] for x in pre)
    return {"tokens": tok, "attach": att, "lengths": plen}


@pytest.mark.parametrize("planks", [1, 2, 5])
def test_greedy_completion_matches_float64(small_fixture, planks):
    sd, batch, _ = small_fixture
    cfg = O.OracleCfg(**SMALL)
    m = make(sd, "f32")
    pre = gt_prefix(batch, planks * 6)
    with torch.no_grad():
        out = m.complete(dev(batch), planks)
        ref = PR.greedy(sd, cfg, batch, pre)
    n = out["samples"].shape[1]
    assert torch.equal(out["samples"].cpu(), ref["tokens"][:, :n]) and torch.equal(out["attach"].cpu(), ref["attach"][:, :n])
    for r in range(4):
        k = int(pre[0][r])
        assert k > 0 and torch.equal(out["samples"][r, :k].cpu(), batch["output_value"][r, :k])
    d = (out["prefix_scores"].double() - ref["prefix_score"]).abs().max()
    assert float(d) <= 1e-3, float(d)
    # the same through the decoder, graph and eager
    for graph in (False, True):
        s, a, ps, _ = grun(greedy_dec(m, graph), dev(batch), prefix_dict(pre, 4, 1), early_stop=True)
        assert torch.equal(s, out["samples"].cpu()) and torch.equal(a, out["attach"].cpu()) and torch.equal(ps, out["prefix_scores"])


@pytest.mark.parametrize("planks", [1, 2])
def test_beam_completion_matches_float64(small_fixture, planks):
    sd, batch, _ = small_fixture
    cfg = O.OracleCfg(**SMALL)
    m = make(sd, "f32")
    pre = gt_prefix(batch, planks * 6, 4)
    with torch.no_grad():
        r = {k: v.cpu() for k, v in D().BeamDecoder(m, 4, use_graph=True, strict_graph=True).run(dev(batch), prefix=prefix_dict(pre, 4, 4)).items()}
        ref = PR.beam_search(sd, cfg, batch, 4, pre)
    BG.compare_to_reference(r, ref, 4)
    d = (r["prefix_scores"].double() - ref["prefix_score"]).abs().max()
    assert float(d) <= 1e-3, float(d)
    for b in range(4):
        k = int(pre[0][b * 4])
        assert torch.equal(r["tokens"][b, :k], batch["output_value"][b, :k])


@pytest.mark.parametrize("planks", [1, 2])
def test_sample_completion_matches_float64(small_fixture, planks):
    sd, batch, _ = small_fixture
    cfg = O.OracleCfg(**SMALL)
    m = make(sd, "f32")
    pre = gt_prefix(batch, planks * 6, 4)
    kw = dict(temperature=0.7, top_k=8)
    dec = SG.sampler(m, 4, seed=1, **kw)
    with torch.no_grad():
        res = dec.run(dev(batch), early_stop=False, prefix=prefix_dict(pre, 4, 4))
        tok, att, _ = dec._lanes[0].buffers(16, 36)
        r = {"rows_tokens": tok.cpu().clone(), "rows_attach": att.cpu().clone()}
        ref = PR.sample_decode(sd, cfg, batch, 4, pre, seed=1, max_steps=36, early_stop=False, **kw)
    SG.compare_to_reference(r, ref, 4)
    for row in range(16):
        k = int(pre[0][row])
        assert torch.equal(r["rows_tokens"][row, :k], batch["output_value"][row // 4, :k])
    assert bool((res["scores"] <= res["prefix_scores"]).all())


# ------------------------------------------------------------------------------------------ 6. graph reuse
def test_one_captured_graph_serves_new_tables(small_fixture):
    from plankassembly_amd import _lib as L
    sd, batch, _ = small_fixture
    m = make(sd, "f32")
    db = dev(batch)
    dec = greedy_dec(m, True)
    g = None
    for planks in (1, 2, 5):
        pre = prefix_dict(gt_prefix(batch, planks * 6), 4, 1)
        got = grun(dec, db, pre)
        g = g or dec._graph
        assert g is not None and dec._graph is g, planks
        want = grun(greedy_dec(m, False), db, pre)
        for x, y in zip(got, want):
            assert torch.equal(x, y), planks
    # pa_decode_prefix_set: a new table after pa_decode_prefix_begin, the captured step replayed
    with torch.no_grad():
        dec.begin(db)
        t1 = D().prefix_table(prefix_dict(gt_prefix(batch, 6), 4, 1), 4, 36, V, END, PAD)
        t5 = D().prefix_table(prefix_dict(gt_prefix(batch, 30), 4, 1), 4, 36, V, END, PAD)
        ps, pl = dec._prefix_begin(t1, 1, 4, 36)
        keep = (t5[0].to(torch.int32).cuda(), t5[1].cuda(), t5[2].cuda())
        L.check(L.lib().pa_decode_prefix_set(dec._lanes[0].h(), L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(keep[2]), L.stream()), "prefix_set")
        assert dec._graph is g
        dec.steps(36)
        tok, att, _ = dec._lanes[0].buffers(4, 36)
        torch.cuda.synchronize()
    assert torch.equal(tok.cpu(), want[0]) and torch.equal(att.cpu(), want[1])
    assert torch.equal(ps.cpu(), want[2]) and torch.equal(pl.cpu(), want[3])


# ------------------------------------------------------------------------------------------ 7. the headline model, bf16
@pytest.mark.parametrize("mode", ["beam", "sample"])
def test_headline_bf16_scores_against_f32_scorer(mode):
    """B 16 x K 8 / B 16 x N 8, Tmax 128, bf16: the decoder's scores against PlankModel.score in exact f32 on the same tokens,
    mean absolute error per token below 0.05 nats (the bound DESIGN.md section 13 uses on the small fixture)."""
    c = LC.CASES["headline"]
    mb, m32 = case_model("headline", "bf16"), case_model("headline", "f32")
    batch = LC.case_batch(c, decode=True, batch_size=16)
    db = mb.prepare_batch(batch)
    if mode == "beam":
        r = BG.beam(mb, db, 8)
        tk, at = r["beam_tokens"], r["beam_attach"]
    else:
        r = SG.run(SG.sampler(mb, 8, temperature=0.8, top_k=50, top_p=0.95, seed=3), db, max_len=128)
        tk, at = r["sample_tokens"], r["sample_attach"]
    sc = score_hypotheses(m32, dev(batch), tk, at, 8)
    fin = torch.isfinite(r["scores"].view(-1))
    assert bool(fin.all()) and bool(torch.isfinite(sc["scores"]).all())
    per_tok = (sc["scores"].double() - r["scores"].view(-1).double()).abs() / sc["lengths"].double()
    print(f"    headline bf16 {mode} scores against score() in f32: mean {float(per_tok.mean()):.5f} nats per token "
          f"(max {float(per_tok.max()):.5f}; lengths {int(sc['lengths'].min())}-{int(sc['lengths'].max())})")
    assert float(per_tok.mean()) < 0.05, float(per_tok.mean())


# ------------------------------------------------------------------------------------------ 8. surface and errors
def test_model_surface(small_fixture):
    sd, batch, _ = small_fixture
    m = make(sd, "f32")
    db = dev(batch)
    pre = prefix_dict(gt_prefix(batch, 12), 4, 1)
    with torch.no_grad():
        ev = m.eval_step(db, prefix=pre)
        cp = m.complete(db, 2)
        bs = m.beam_search(db, 4, prefix=pre)
        sm = m.sample(db, 4, top_k=20, seed=7, prefix=pre)
        plain = m.eval_step(db)
        sc = m.score(db)
    assert torch.equal(ev["samples"], cp["samples"]) and torch.equal(ev["prefix_scores"], cp["prefix_scores"])
    assert "prefix_scores" not in plain and {"samples", "attach", "predicts", "groundtruths"} <= set(ev)
    assert ev["prefix_scores"].shape == (4,) and ev["prefix_logprobs"].shape == (4, ev["samples"].shape[1])
    assert bs["prefix_scores"].shape == (4, 4) and sm["prefix_scores"].shape == (4, 4) and sm["sample_tokens"].shape[:2] == (4, 4)
    for out in (ev, bs, sm):
        for r in range(4):
            k = int(pre["lengths"][r])
            assert torch.equal(out["samples"][r, :k].cpu(), batch["output_value"][r, :k])
    assert float((bs["prefix_scores"][:, 0] - ev["prefix_scores"]).abs().max()) <= 1e-3          # (another row count: not bitwise)
    assert set(sc) == {"scores", "logprobs", "lengths"} and sc["scores"].shape == (4,) and sc["scores"].dtype == torch.float32
    want = [PR.default_length(batch["output_value"][r], O.OracleCfg(**SMALL)) for r in range(4)]
    assert sc["lengths"].tolist() == want and want[0] == 13 and sc["logprobs"].shape == (4, max(want))
    # errors: through the model entry points (ValueError before anything is launched)
    tok = batch["output_value"][:, :12]
    att = torch.full_like(tok, -1)
    bad = []
    for t, j in ((6, 6), (4, 0), (7, -2)):
        x = att.clone()
        x[0, t] = j
        bad.append({"tokens": tok, "attach": x})
    x = att.clone()
    x[1, 7] = 2                                                       # tokens[7] != tokens[2]
    bad += [{"tokens": tok, "attach": x}, {"tokens": torch.zeros(4, 37, dtype=torch.long)}, {"tokens": torch.full((4, 3), V)},
            {"tokens": tok, "lengths": [13, 1, 1, 1]}]
    for p in bad:
        for call in (lambda: m.eval_step(db, prefix=p), lambda: m.beam_search(db, 2, prefix=p), lambda: m.sample(db, 2, prefix=p)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        m.score(db, torch.full((4, 3), V))
    with pytest.raises(ValueError):
        D().GreedyDecoder(m, lanes=2).run(db, prefix=pre)
    with torch.no_grad():
        again = m.eval_step(db)
    assert torch.equal(again["samples"], plain["samples"])


def test_abi_errors(small_fixture):
    from plankassembly_amd import _lib as L
    sd, batch, _ = small_fixture
    m = make(sd)
    db = dev(batch)
    lib, st = L.lib(), L.stream()
    dec = greedy_dec(m, False)
    dec.begin(db)
    h = dec._lanes[0].h()
    need = int(lib.pa_decode_prefix_ws_bytes(h, 4, 36))
    assert need > 0 and int(lib.pa_decode_prefix_ws_bytes(h, 0, 36)) < 0 and int(lib.pa_decode_prefix_ws_bytes(h, 4, 0)) < 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    base = C.c_void_p((ws.data_ptr() + 255) // 256 * 256)
    plen = torch.zeros(4, dtype=torch.int32, device="cuda")
    ptok = torch.zeros(4, 36, dtype=torch.int64, device="cuda")
    patt = torch.full((4, 36), -1, dtype=torch.int64, device="cuda")
    p = C.c_void_p()
    assert lib.pa_decode_prefix_buffers(h, C.byref(p), C.byref(C.c_void_p())) != 0          # no prefix yet
    assert lib.pa_decode_prefix_set(h, L.ptr(plen), L.ptr(ptok), L.ptr(patt), st) != 0
    for args in ((None, L.ptr(ptok), L.ptr(patt), base, C.c_int64(need)), (L.ptr(plen), None, L.ptr(patt), base, C.c_int64(need)),
                 (L.ptr(plen), L.ptr(ptok), None, base, C.c_int64(need)), (L.ptr(plen), L.ptr(ptok), L.ptr(patt), None, C.c_int64(need)),
                 (L.ptr(plen), L.ptr(ptok), L.ptr(patt), base, C.c_int64(256))):
        with pytest.raises(L.PlankHipError):
            L.check(lib.pa_decode_prefix_begin(h, *args, st), "prefix_begin")
    fresh = m.new_bound_handle()
    try:
        with pytest.raises(L.PlankHipError):                                  # a decode that was not begun
            L.check(lib.pa_decode_prefix_begin(fresh, L.ptr(plen), L.ptr(ptok), L.ptr(patt), base, C.c_int64(need), st), "no decode")
        assert int(lib.pa_decode_prefix_ws_bytes(fresh, 4, 36)) == need
    finally:
        lib.pa_model_destroy(fresh)
    L.check(lib.pa_decode_prefix_begin(h, L.ptr(plen), L.ptr(ptok), L.ptr(patt), base, C.c_int64(need), st), "prefix_begin")
    L.check(lib.pa_decode_prefix_buffers(h, C.byref(p), C.byref(C.c_void_p())), "prefix_buffers")
    L.check(lib.pa_decode_prefix_set(h, L.ptr(plen), L.ptr(ptok), L.ptr(patt), st), "prefix_set")
    with pytest.raises(L.PlankHipError):
        L.check(lib.pa_decode_prefix_set(h, None, L.ptr(ptok), L.ptr(patt), st), "prefix_set null")
    dec.begin(db)                                                             # pa_decode_begin clears the prefix
    assert lib.pa_decode_prefix_buffers(h, C.byref(p), C.byref(C.c_void_p())) != 0
    torch.cuda.synchronize()
