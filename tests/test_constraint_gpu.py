"""Grammar-constrained decoding on the GPU (include/plank_hip.h pa_decode_constraint_set, decode.plank_grammar / check_planks;
DESIGN.md section 15)."""
import ctypes as C
import functools

import pytest
import torch

import large_cases as LC
import test_beam_gpu as BG
import test_prefix_gpu as PG
import test_sample_gpu as SG
from test_beam_gpu import case_model, dev, make, tiny_case
from test_constraint_cpu import END, N_VAL, PAD, planks_ok, ref_beam, ref_greedy, ref_sample

pytestmark = pytest.mark.gpu

FILTERED = dict(temperature=0.8, top_k=50, top_p=0.95)


def D():
    import plankassembly_amd.decode as d
    return d


def grammar(*a, **k):
    return D().plank_grammar(*a, **k)


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """(model, device batch, Tmax) of the three shapes: small_fixture (B 4, d 64, S 65, Tmax 36), the tiny case at max_len 32 (END
    forced at 30) and 4 headline rows (d 512, Tmax 128, END forced at 126).  Built once per session; the decodes do not change them."""
    if name == "small":
        sd, batch, _ = BG.load_fixture("fixture_small.npz")
        return make(sd, dtype), dev(batch), 36
    if name == "tiny":
        sd, batch, _ = tiny_case()
        m = make(sd, dtype, 128, 8, 256, 2, 2, 1200, 128)
        return m, m.prepare_batch(batch), 32
    m = case_model("headline", dtype)
    return m, m.prepare_batch(LC.case_batch(LC.CASES["headline"], decode=True, batch_size=4)), 128


def greedy(m, db, Tmax, constraint=None, graph=True, prefix=None, dec=None):
    dec = dec or D().GreedyDecoder(m, use_graph=graph, strict_graph=graph)
    with torch.no_grad():
        s, a = dec.run(db, max_len=Tmax, early_stop=False, prefix=prefix, constraint=constraint)
    return s.cpu(), a.cpu()


def beam(m, db, Tmax, K, constraint=None, graph=True, dec=None, early_stop=True):
    dec = dec or D().BeamDecoder(m, K, use_graph=graph, strict_graph=graph)
    with torch.no_grad():
        return {k: v.cpu() for k, v in dec.run(db, max_len=Tmax, early_stop=early_stop, constraint=constraint).items()}


def sample(m, db, Tmax, N, constraint=None, graph=True, dec=None, early_stop=True, **kw):
    """The ranked dict plus the per-row buffers rows_tokens / rows_attach / rows_scores (row b*N + n), as test_sample_gpu.run."""
    dec = dec or SG.sampler(m, N, graph, **kw)
    with torch.no_grad():
        r = dec.run(db, max_len=Tmax, early_stop=early_stop, constraint=constraint)
        n, rows = r["sample_tokens"].shape[2], r["sample_tokens"].shape[0] * N
        tok, att, _ = dec._lanes[0].buffers(rows, Tmax)
        out = {k: v.cpu() for k, v in r.items()}
        out["rows_tokens"], out["rows_attach"], out["rows_scores"] = tok[:, :n].cpu(), att[:, :n].cpu(), dec._scores(rows).cpu().clone()
    return out


def first_end(tok):
    e = tok == END
    return torch.where(e.any(1), e.long().argmax(1), torch.full((tok.shape[0],), -1))


def check_pointers(tok, att):
    """Up to each row's first END a pointer points backwards and carries the token it points to; after it PAD / -1 (rows [R, n])."""
    fe = first_end(tok)
    for r in range(tok.shape[0]):
        n = int(fe[r]) + 1 if fe[r] >= 0 else tok.shape[1]
        assert bool((tok[r, n:] == PAD).all()) and bool((att[r, n:] == -1).all()), r
        for t in (att[r, :n] >= 0).nonzero()[:, 0].tolist():
            assert int(att[r, t]) < t and int(tok[r, t]) == int(tok[r, att[r, t]]), (r, t)


# ------------------------------------------------------------------------------------------ 1. validity
@pytest.mark.parametrize("name", ["small", "tiny", "headline"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("graph", [False, True])
def test_constrained_rows_are_valid_programs(name, dtype, graph):
    """Greedy, beam K 4 and sampling N 4 (unfiltered, and tau 0.8 / top_k 50 / top_p 0.95): every row that finished is a valid plank
    program, and every row finishes (the grammar forces END at the last plank boundary, on the headline rows at 126).  The same batch
    decoded without the constraint is not valid on small: this test fails without the feature."""
    m, db, Tmax = case(name, dtype)
    g = grammar()
    last = (Tmax - 1) // 6 * 6
    s, _ = greedy(m, db, Tmax, g, graph)
    fe = first_end(s)
    assert bool((fe >= 0).all()) and int(fe.max()) <= last and bool(planks_ok(s).all()), (fe, planks_ok(s))
    rb = beam(m, db, Tmax, 4, g, graph)
    assert bool(rb["finished"].all()) and bool(torch.isfinite(rb["scores"]).all())
    assert bool(planks_ok(rb["beam_tokens"].reshape(16, -1)).all()) and int(rb["lengths"].max()) <= last + 1
    check_pointers(rb["beam_tokens"].reshape(16, -1), rb["beam_attach"].reshape(16, -1))
    for kw in (dict(), FILTERED):
        rs = sample(m, db, Tmax, 4, g, graph, seed=3, **kw)
        assert bool(rs["finished"].all()) and bool(torch.isfinite(rs["scores"]).all())
        assert bool(planks_ok(rs["sample_tokens"].reshape(16, -1)).all()) and int(rs["lengths"].max()) <= last + 1
        check_pointers(rs["rows_tokens"], rs["rows_attach"])
    if name == "small":
        free, _ = greedy(m, db, Tmax, None, graph)
        assert not bool(planks_ok(free).all())


# ------------------------------------------------------------------------------------------ 2. token-exact against float64, f32
@pytest.mark.parametrize("name", ["small", "tiny"])
def test_greedy_f32_matches_float64_reference(name):
    """Up to each row's first END, every row: the constrained float64 reference (tests/constraint_reference.py) has no near tie at
    1e-5 among allowed candidates on either fixture before a first END (measured on the CPU: 0 on small, 0 on tiny - asserted in
    tests/test_constraint_cpu.py), so no row is left out."""
    m, db, Tmax = case(name, "f32")
    ref = ref_greedy(name)
    assert ref["first_end"].tolist() == ([12, 24, 12, 18] if name == "small" else [30] * 4)
    for graph in (False, True):
        s, a = greedy(m, db, Tmax, grammar(), graph)
        for r in range(4):
            n = int(ref["first_end"][r]) + 1
            assert not bool(ref["near_tie"][r, :n].any())
            assert torch.equal(s[r, :n], ref["tokens"][r, :n]) and torch.equal(a[r, :n], ref["attach"][r, :n]), (r, s[r], ref["tokens"][r])


@pytest.mark.parametrize("name", ["small", "tiny"])
def test_beams_f32_match_float64_reference(name):
    """test_beam_gpu.compare_to_reference's rule: at most one diverging drawing, and only behind a reference near-tie.  The
    constrained reference flags one near-tie step in one drawing on small and none on tiny (measured on the CPU)."""
    m, db, Tmax = case(name, "f32")
    ref = ref_beam(name)
    assert int(ref["near_tie"].any(1).sum()) <= (1 if name == "small" else 0)
    BG.compare_to_reference(beam(m, db, Tmax, 4, grammar()), ref, 4)


@pytest.mark.parametrize("name", ["small", "tiny"])
def test_samples_f32_match_float64_reference(name):
    """test_sample_gpu.compare_to_reference at its 1e-6 margin, N 4, seed 1, unfiltered: rows equal the reference up to their first
    near-boundary step.  The constrained reference flags 0 of 16 rows on small and 0 of 16 on tiny (measured on the CPU; the cap
    for tiny is 2 of 16, which min_full 0.85 admits)."""
    m, db, Tmax = case(name, "f32")
    ref = ref_sample(name)
    assert int(ref["near"].any(1).sum()) <= (0 if name == "small" else 2)
    r = sample(m, db, Tmax, 4, grammar(), seed=1, early_stop=False)
    SG.compare_to_reference(r, ref, 4, min_full=0.9 if name == "small" else 0.85)
    n = min(r["rows_tokens"].shape[1], ref["tokens"].shape[1])
    eq = ((r["rows_tokens"][:, :n] == ref["tokens"][:, :n]) & (r["rows_attach"][:, :n] == ref["attach"][:, :n])).all(1)
    d = (r["rows_scores"].double() - ref["scores"])[eq].abs().max()            # (rows that took the reference's path: its score)
    assert float(d) <= 1e-3, float(d)


# ------------------------------------------------------------------------------------------ 3. self-consistency, bit-exact
@pytest.mark.parametrize("name", ["small", "headline"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_k1_and_top_k1_are_constrained_greedy(name, dtype):
    m, db, Tmax = case(name, dtype)
    for g in (grammar(), grammar(3, 4)):
        s, a = greedy(m, db, Tmax, g)
        assert name != "small" or bool((a >= 0).any())
        BG.assert_k1_is_greedy(s, a, beam(m, db, Tmax, 1, g, early_stop=False))
        r = sample(m, db, Tmax, 1, g, temperature=0.7, top_k=1, top_p=0.9, seed=5, early_stop=False)
        SG.assert_greedy_prefix(s, a, r["rows_tokens"], r["rows_attach"], 1)


# ------------------------------------------------------------------------------------------ 4. scores are the model's
def test_scores_are_the_models_log_likelihood():
    """No renormalisation: PlankModel.score (every position forced, no constraint) of the returned constrained beams and samples is
    the run's own score, within the 1e-3 test_prefix_gpu.check_score allows between f32 and float64."""
    m, db, Tmax = case("small", "f32")
    rb = beam(m, db, Tmax, 4, grammar())
    rs = sample(m, db, Tmax, 4, grammar(), seed=2, temperature=1.2, top_k=40)
    for what, r, tk, at in (("beam", rb, rb["beam_tokens"], rb["beam_attach"]), ("sample", rs, rs["sample_tokens"], rs["sample_attach"])):
        sc = PG.score_hypotheses(m, db, tk, at, 4)
        assert bool(torch.isfinite(r["scores"]).all())
        d = (sc["scores"].double() - r["scores"].view(-1).double()).abs().max()
        print(f"    {what}: score() against the constrained decoder's own scores: {float(d):.3e}")
        assert float(d) <= 1e-3, float(d)


# ------------------------------------------------------------------------------------------ 5. off means off
def same(a, b):
    if isinstance(a, dict):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    else:
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_off_means_off_and_parameters_recapture(dtype):
    m, db, Tmax = case("small", dtype)
    g1, g3 = grammar(), grammar(min_planks=3)
    runs = ((lambda dec, c: greedy(m, db, Tmax, c, dec=dec), lambda: D().GreedyDecoder(m, use_graph=True, strict_graph=True)),
            (lambda dec, c: beam(m, db, Tmax, 4, c, dec=dec), lambda: D().BeamDecoder(m, 4, use_graph=True, strict_graph=True)),
            (lambda dec, c: sample(m, db, Tmax, 4, c, dec=dec), lambda: SG.sampler(m, 4, True, seed=3, **FILTERED)))
    for run, new in runs:
        plain = run(new(), None)
        dec = new()
        on1 = run(dec, g1)
        graph1 = dec._graph
        assert graph1 is not None
        same(run(dec, g1), on1)
        assert dec._graph is graph1                                  # the same parameters replay the same graph
        on3 = run(dec, g3)
        assert dec._graph is not graph1                              # new parameters are new kernel arguments: captured again
        same(run(new(), g3), on3)
        same(run(dec, None), plain)                                  # and the unconstrained bits again on the next run without
        same(run(dec, False), plain)
        same(run(dec, g1), on1)
        tok1 = on1[0] if isinstance(on1, tuple) else on1["tokens"]
        tok3 = on3[0] if isinstance(on3, tuple) else on3["tokens"]
        assert bool(planks_ok(tok1).all()) and bool(planks_ok(tok3, 3).all()) and bool((first_end(tok3) >= 18).all())
        if isinstance(plain, tuple):                                 # greedy: free rows are not valid, and min_planks 1 ends before 18
            assert not bool(planks_ok(plain[0]).all()) and int(first_end(tok1).min()) < 18


# ------------------------------------------------------------------------------------------ 6. prefix + constraint
@pytest.mark.parametrize("name", ["small", "headline"])
def test_prefix_of_the_constrained_output_gives_it_back(name):
    m, db, Tmax = case(name, "f32")
    g = grammar()
    dec = D().GreedyDecoder(m, use_graph=True, strict_graph=True)
    s, a = greedy(m, db, Tmax, g, dec=dec)
    pre = {"tokens": s[:, :9], "attach": a[:, :9], "lengths": [9] * 4}
    s2, a2 = greedy(m, db, Tmax, g, prefix=pre, dec=dec)
    assert torch.equal(s2, s) and torch.equal(a2, a)
    assert bool(torch.isfinite(dec.last_prefix_scores).all()) and bool((dec.last_prefix_logprobs[:, :9] <= 0).all())
    # forced positions are not filtered: a degenerate plank (x1 == x0) goes through as given, the free steps after it stay valid
    bad = s[:, :6].clone()
    bad[:, 3] = bad[:, 0]
    s3, _ = greedy(m, db, Tmax, g, prefix={"tokens": bad, "lengths": [6] * 4}, dec=dec)
    assert torch.equal(s3[:, :6], bad) and not bool(planks_ok(s3).any())
    fe = first_end(s3)
    assert bool((fe >= 0).all()) and bool(planks_ok(torch.cat([s[:, :6], s3[:, 6:]], 1)).all())
    rb = beam(m, db, Tmax, 4, g)
    P = min(9, rb["tokens"].shape[1])
    pre = {"tokens": rb["tokens"][:, :P], "attach": rb["attach"][:, :P], "lengths": [P] * 4}
    with torch.no_grad():
        rp = D().BeamDecoder(m, 4, use_graph=True, strict_graph=True).run(db, max_len=Tmax, prefix=pre, constraint=g)
    assert bool(torch.isfinite(rp["prefix_scores"]).all()) and bool(planks_ok(rp["beam_tokens"].cpu().reshape(16, -1)).all())


# ------------------------------------------------------------------------------------------ 7. limits
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_min_and_max_planks(dtype):
    m, db, Tmax = case("small", dtype)
    for g, ok in ((grammar(max_planks=2), lambda fe: bool(((fe >= 6) & (fe <= 12)).all())),
                  (grammar(min_planks=3), lambda fe: bool((fe >= 18).all())),
                  (grammar(min_planks=0, max_planks=1), lambda fe: bool((fe <= 6).all())),
                  (grammar(min_planks=2, max_planks=1000), lambda fe: bool(((fe >= 12) & (fe <= 30)).all()))):   # (clamped to (36 - 1) // 6 = 5)
        s, _ = greedy(m, db, Tmax, g)
        rb = beam(m, db, Tmax, 4, g)
        rs = sample(m, db, Tmax, 4, g, seed=4)
        for tok in (s, rb["beam_tokens"].reshape(16, -1), rs["sample_tokens"].reshape(16, -1)):
            fe = first_end(tok)
            assert ok(fe) and bool((fe % 6 == 0).all()) and bool(planks_ok(tok, g.min_planks).all()), (tuple(g), fe)


# ------------------------------------------------------------------------------------------ 8. routing and errors
def test_model_routing_and_errors():
    import types
    from plankassembly_amd.models import PlankModel, build_model
    from plankassembly_amd.trainer import Trainer
    from test_beam_cpu import _model_cfg
    sd, batch, _ = BG.load_fixture("fixture_small.npz")
    db = dev(batch)
    plain_m, _, _ = case("small", "f32")
    for extra in (dict(), dict(BEAM_SIZE=4), dict(NUM_SAMPLES=4, TOP_K=50)):
        m = build_model(_model_cfg(CONSTRAIN_PLANKS=True, COMPUTE_DTYPE="f32", **extra))
        m.load_state_dict(sd)
        m = m.cuda().eval()
        with torch.no_grad():
            out = m(db)
            off = m.eval_step(db, constraint=False)
        assert bool(planks_ok(out["samples"].cpu()).all())
        assert extra or not bool(planks_ok(off["samples"].cpu()).all())        # (greedy: the free rows of this fixture are not valid)
        for pred in out["predicts"]:                                  # the trainer's degenerate-plank filter drops nothing
            assert len(pred) >= 1 and torch.equal(Trainer._valid_pred(None, pred), pred)
            assert bool((pred[:, 3:] > pred[:, :3]).all())
    with torch.no_grad():
        want, _ = greedy(plain_m, db, 36, grammar())
        ev = plain_m.eval_step(db, constraint=grammar())
        cp = plain_m.complete(db, 1, constraint=grammar())
        bs = plain_m.beam_search(db, 4, constraint=grammar())
        sm = plain_m.sample(db, 4, top_k=20, seed=7, constraint=grammar())
        free = plain_m.eval_step(db)
    n = ev["samples"].shape[1]
    assert torch.equal(ev["samples"].cpu(), want[:, :n]) and not bool(planks_ok(free["samples"].cpu()).all())
    from test_prefix_cpu import gt_prefix
    for r, k in enumerate(gt_prefix(batch, 6)[0].tolist()):
        assert k > 0 and torch.equal(cp["samples"][r, :k].cpu(), batch["output_value"][r, :k])
    assert bool(torch.isfinite(cp["prefix_scores"]).all())
    for out in (ev, bs, sm):
        assert bool(planks_ok(out["samples"].cpu()).all())
    # errors, before anything is launched
    with pytest.raises(ValueError):
        D().GreedyDecoder(plain_m, lanes=2).run(db, constraint=grammar())
    for bad in ({"min_planks": 1}, (1, 2), 7):
        for call in (lambda: plain_m.eval_step(db, constraint=bad), lambda: plain_m.beam_search(db, 2, constraint=bad),
                     lambda: plain_m.sample(db, 2, constraint=bad)):
            with pytest.raises(ValueError):
                call()
    for a in ((-1, None), (2, 1), (0, 0)):
        with pytest.raises(ValueError):
            grammar(*a)
    with pytest.raises(ValueError):
        PlankModel(64, 4, 128, 0.0, "relu", True, 2, 2, 3, 2, 4, 6, 65, 36, 514, types.SimpleNamespace(END=512, PAD=513), constraint=(1, 2))
    with torch.no_grad():
        again = plain_m.eval_step(db)
    assert torch.equal(again["samples"], free["samples"])


def test_abi_errors():
    from plankassembly_amd import _lib as L
    m, db, _ = case("small", "f32")
    lib, st = L.lib(), L.stream()
    P = L.ConstraintParams
    free, _ = greedy(m, db, 36)                                               # (first: decoders of one model share its handle)
    fresh = m.new_bound_handle()
    try:
        assert lib.pa_decode_constraint_set(fresh, C.byref(P(N_VAL, 1, 5, 0))) != 0          # a decode that was not begun
    finally:
        lib.pa_model_destroy(fresh)
    dec = D().GreedyDecoder(m, use_graph=False)
    dec.begin(db)
    h = dec._lanes[0].h()
    assert lib.pa_decode_constraint_set(None, C.byref(P(N_VAL, 1, 5, 0))) != 0
    for bad in (P(N_VAL, -1, 5, 0), P(N_VAL, 1, 0, 0), P(N_VAL, 3, 2, 0), P(N_VAL, 0, 0, 0), P(1, 1, 5, 0), P(515, 1, 5, 0)):
        with pytest.raises(L.PlankHipError):
            L.check(lib.pa_decode_constraint_set(h, C.byref(bad)), "constraint_set")
    L.check(lib.pa_decode_constraint_set(h, C.byref(P(N_VAL, 0, 1, 0))), "constraint_set")
    tok, _, _ = dec._lanes[0].buffers(4, 36)
    dec.steps(36)                                                             # min_planks 0, max_planks 1: END at 0 or 6
    assert bool((first_end(tok.cpu()) <= 6).all()) and bool(planks_ok(tok.cpu(), 0).all())
    dec.begin(db)
    L.check(lib.pa_decode_constraint_set(h, C.byref(P(N_VAL, 0, 1, 0))), "constraint_set")
    L.check(lib.pa_decode_constraint_set(h, None), "clear")                   # NULL clears it
    dec.steps(36)
    assert torch.equal(tok.cpu(), free)
    L.check(lib.pa_decode_constraint_set(h, C.byref(P(N_VAL, 1, 2 ** 31 - 1, 0))), "constraint_set")
    dec.begin(db)                                                             # pa_decode_begin clears it as well
    dec.steps(36)
    assert torch.equal(tok.cpu(), free)
    torch.cuda.synchronize()
