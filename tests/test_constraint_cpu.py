"""Grammar-constrained decoding: the CPU reference (tests/constraint_reference.py), decode.plank_grammar / check_planks and the ABI
surface.  No GPU."""
import functools
import os
import re

import pytest
import torch

from conftest import REPO
from oracle import plank_oracle as O
import beam_reference as BR
import constraint_reference as CR
import prefix_reference as PR
import sample_reference as SR
from test_beam_cpu import _model_cfg, load_case

V, END, PAD, N_VAL = 514, 512, 513, 512


@functools.lru_cache(maxsize=None)
def ref_greedy(name, min_planks=None, max_planks=None, free=False):
    """The float64 greedy reference of a committed case (36 / 32 steps), computed once per session and shared (read only)."""
    sd, batch, cfg, steps = load_case(name)
    with torch.no_grad():
        return CR.greedy(sd, cfg, batch, None if free else dict(min_planks=1 if min_planks is None else min_planks, max_planks=max_planks),
                         max_steps=steps)


@functools.lru_cache(maxsize=None)
def ref_beam(name, K=4):
    sd, batch, cfg, steps = load_case(name)
    with torch.no_grad(), CR.constrained():
        return BR.beam_search(sd, cfg, batch, K, max_steps=steps)


@functools.lru_cache(maxsize=None)
def ref_sample(name, N=4, seed=1, tol=1e-6):
    sd, batch, cfg, steps = load_case(name)
    with torch.no_grad(), CR.constrained():
        return SR.sample_decode(sd, cfg, batch, N, seed=seed, max_steps=steps, early_stop=False, tol=tol)


def planks_ok(tokens, min_planks=1):
    from plankassembly_amd.decode import check_planks
    return check_planks(tokens, END, N_VAL, min_planks)


# ---------------------------------------------------------------------------------------------- the window
@pytest.mark.parametrize("min_planks,max_planks", [(1, None), (0, 1), (3, 4), (2, 2), (5, 1000)])
def test_window_is_never_empty(min_planks, max_planks):
    """Every t < 2048 and every token 0 .. 513 at t - 3: the window holds a token, every token of it is a coordinate value or END
    (never PAD), END only at a plank boundary k >= min_planks, and from max_planks on nothing but END."""
    steps = 2048
    lo_p, hi_p = CR.resolve(steps, min_planks, max_planks)
    assert hi_p == min((steps - 1) // 6, max_planks or 10 ** 9)
    for t in range(steps):
        c, k = t % 6, t // 6
        for prev in (range(V) if c >= 3 else (0,)):
            lo, hi, end_ok = CR.window(t, prev, N_VAL, lo_p, hi_p)
            assert lo <= hi or end_ok, (t, prev)
            if lo <= hi:
                assert 0 <= lo and hi <= N_VAL - 1
            if c >= 3:
                assert lo > min(prev, N_VAL - 2) and hi == N_VAL - 1 and not end_ok
            elif c > 0:
                assert (lo, hi, end_ok) == (0, N_VAL - 2, False)
            elif k >= hi_p:
                assert lo > hi and end_ok
            else:
                assert (lo, hi) == (0, N_VAL - 2) and end_ok == (k >= lo_p)


def test_allowed_mask_judges_pointers_by_their_token():
    hist = torch.tensor([[5, 7, 9, 300, 510, 511, 3, 0, 0, 0, 0, 0]])
    # t = 9: c = 3, prev = tokens[6] = 3 -> [4, 511]; pointers j < 9 by hist[j]; j >= 9 never
    m = CR.allowed_mask(9, hist, V, END, N_VAL, 1, 5, V + 10)[0]
    assert m[:V].nonzero()[:, 0].tolist() == list(range(4, 512))
    assert m[V:].tolist() == [True, True, True, True, True, True, False, False, False, False]
    # t = 6: c = 0, k = 1 >= min_planks -> [0, 510] + END; the pointer to 511 is out
    m = CR.allowed_mask(6, hist, V, END, N_VAL, 1, 5, V + 7)[0]
    assert bool(m[END]) and not bool(m[PAD]) and not bool(m[511]) and m[V:].tolist() == [True, True, True, True, True, False, False]
    # t = 6 with max_planks 1: END only, no pointer
    m = CR.allowed_mask(6, hist, V, END, N_VAL, 1, 1, V + 7)[0]
    assert m.nonzero()[:, 0].tolist() == [END]


# ---------------------------------------------------------------------------------------------- the reference
def test_reference_without_a_constraint_is_the_existing_reference():
    sd, batch, cfg, _ = load_case("small")
    steps = 12
    with torch.no_grad():
        s, at = O.greedy_decode_cached(sd, cfg, batch, max_steps=steps, early_stop=False)
        g = CR.greedy(sd, cfg, batch, None, max_steps=steps, dtype=torch.float32)
        assert torch.equal(g["tokens"], s) and torch.equal(g["attach"], at)
        b0 = BR.beam_search(sd, cfg, batch, 2, max_steps=steps)
        s0 = SR.sample_decode(sd, cfg, batch, 2, seed=3, top_k=20, max_steps=steps)
        saved = (BR._Stepper, SR._Stepper, PR._Stepper)
        with CR.constrained(min_planks=1) as cls:
            assert BR._Stepper is cls and SR._Stepper is cls and PR._Stepper is cls
            b1 = BR.beam_search(sd, cfg, batch, 2, max_steps=steps)
        assert (BR._Stepper, SR._Stepper, PR._Stepper) == saved
        with pytest.raises(RuntimeError):
            with CR.constrained():
                raise RuntimeError("restored on the way out of an exception too")
        assert (BR._Stepper, SR._Stepper, PR._Stepper) == saved
        b2 = BR.beam_search(sd, cfg, batch, 2, max_steps=steps)
        s2 = SR.sample_decode(sd, cfg, batch, 2, seed=3, top_k=20, max_steps=steps)
    assert not torch.equal(b1["beam_tokens"], b0["beam_tokens"])             # (the constraint did act inside)
    for k in b0:
        assert torch.equal(torch.as_tensor(b0[k]), torch.as_tensor(b2[k])), k
    for k in s0:
        assert torch.equal(torch.as_tensor(s0[k]), torch.as_tensor(s2[k])), k


def first_end(tok):
    e = tok == END
    return torch.where(e.any(1), e.long().argmax(1), torch.full((tok.shape[0],), -1)).tolist()


def test_fixture_facts_small():
    """fixture_small, 36 steps, float64: free greedy has no valid row (a plank with max <= min in each); constrained greedy is
    valid everywhere with first ENDs at 12 / 24 / 12 / 18, and at 18 / 24 / 18 / 18 with min_planks 3, max_planks 4.  The
    constrained reference has no near tie (1e-5, among allowed candidates) up to any row's first END."""
    free, g, g34 = ref_greedy("small", free=True), ref_greedy("small"), ref_greedy("small", 3, 4)
    assert planks_ok(free["tokens"]).tolist() == [False] * 4
    assert planks_ok(g["tokens"]).tolist() == [True] * 4 and first_end(g["tokens"]) == [12, 24, 12, 18] == g["first_end"].tolist()
    assert first_end(g34["tokens"]) == [18, 24, 18, 18] and planks_ok(g34["tokens"], 3).tolist() == [True] * 4
    for r in range(4):
        assert not bool(g["near_tie"][r, :int(g["first_end"][r]) + 1].any())
    # pointers are used, point backwards and carry their token
    tok, att = g["tokens"], g["attach"]
    assert bool((att >= 0).any())
    for r, t in (att >= 0).nonzero().tolist():
        assert att[r, t] < t and tok[r, t] == tok[r, att[r, t]]


def test_fixture_facts_tiny():
    """The tiny case, 32 steps: free greedy never emits END; constrained greedy closes every row at 30, the last plank boundary."""
    free, g = ref_greedy("tiny", free=True), ref_greedy("tiny")
    assert first_end(free["tokens"]) == [-1] * 4 and planks_ok(free["tokens"]).tolist() == [False] * 4
    assert first_end(g["tokens"]) == [30] * 4 and planks_ok(g["tokens"]).tolist() == [True] * 4
    assert not bool(g["near_tie"][:, :31].any())


def test_constrained_beam_and_sampling_references():
    """Beam K 4 and sampling N 4 through the installed stepper: every hypothesis finishes and is a valid program, the scores stay
    the teacher-forced log-likelihood of the unconstrained model (no renormalisation).  The near-tie / near-boundary counts the GPU
    test relies on: one beam step in one drawing on small, none on tiny; no sample row at the 1e-6 margin on either."""
    for name in ("small", "tiny"):
        sd, batch, cfg, steps = load_case(name)
        rb, rs = ref_beam(name), ref_sample(name)
        assert bool(rb["finished"].all()) and all(planks_ok(rb["beam_tokens"][b]).all() for b in range(4))
        assert bool((rs["first_end"] >= 0).all()) and bool(planks_ok(rs["tokens"]).all())
        ties = rb["near_tie"].sum(1).tolist()
        print(f"    {name}: beam near-tie steps per drawing {ties}, sample rows flagged {int(rs['near'].any(1).sum())} of 16")
        assert sorted(ties) == ([0, 0, 0, 1] if name == "small" else [0, 0, 0, 0])
        assert int(rs["near"].any(1).sum()) <= (0 if name == "small" else 2)
        with torch.no_grad():
            tf = BR.teacher_forced_logprob(sd, cfg, batch, rb["beam_tokens"], rb["beam_attach"])
        assert torch.allclose(tf, rb["scores"], rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------------------------- check_planks / plank_grammar
def test_check_planks_on_hand_made_rows():
    good = [1, 2, 3, 4, 5, 6, 0, 0, 0, 511, 1, 510, END, PAD, PAD]
    rows = {
        "good": (good, True),
        "end mid-plank": ([1, 2, 3, 4, 5, 6, 0, 0, 0, END, PAD, PAD, PAD, PAD, PAD], False),
        "max == min": ([1, 2, 3, 4, 2, 6, END] + [PAD] * 8, False),
        "max < min": ([9, 2, 3, 4, 5, 6, END] + [PAD] * 8, False),
        "pad inside": ([1, 2, 3, 4, 5, 6, 0, PAD, 0, 1, 1, 1, END, PAD, PAD], False),
        "no end": ([1, 2, 3, 4, 5, 6, 0, 0, 0, 1, 1, 1, 0, 0, 0], False),
        "empty program": ([END] + [PAD] * 14, False),
        "junk after end": ([1, 2, 3, 4, 5, 6, END, 7, 7, 7, 7, 7, 7, END, 3], True),
    }
    tok = torch.tensor([r for r, _ in rows.values()])
    assert planks_ok(tok).tolist() == [w for _, w in rows.values()], list(rows)
    assert planks_ok(tok, 2).tolist() == [True] + [False] * 7                 # fewer than min_planks
    assert planks_ok(tok, 0).tolist()[6] is True                              # min_planks 0 admits the empty program
    assert planks_ok(torch.tensor([[END]])).tolist() == [False] and planks_ok(torch.tensor([[END]]), 0).tolist() == [True]


def test_plank_grammar_validation():
    from plankassembly_amd.decode import GreedyDecoder, plank_grammar
    assert tuple(plank_grammar()) == (1, None) and tuple(plank_grammar(0, 1)) == (0, 1) and tuple(plank_grammar(3, 3)) == (3, 3)
    for bad in ((-1, None), (2, 1), (0, 0), (1.5, None), (1, 2.0), (True, None), ("1", None)):
        with pytest.raises(ValueError):
            plank_grammar(*bad)
    import types
    m = types.SimpleNamespace(max_output_length=16, vocab_size=V, token=types.SimpleNamespace(END=END, PAD=PAD))
    one = GreedyDecoder(m, use_graph=False, lanes=1)
    assert one._check_constraint(None) is None and one._check_constraint(False) is None
    assert tuple(one._check_constraint(True)) == (1, None) and tuple(one._check_constraint(plank_grammar(2, 5))) == (2, 5)
    for bad in ({"min_planks": 1}, (1, None), 3):
        with pytest.raises(ValueError):
            one._check_constraint(bad)
    with pytest.raises(ValueError):                                           # one lane only, like prefixes
        GreedyDecoder(m, use_graph=False, lanes=2)._check_constraint(plank_grammar())


def test_config_keys():
    from plankassembly_amd.models import build_model
    assert build_model(_model_cfg()).constraint is None
    assert build_model(_model_cfg(MIN_PLANKS=3)).constraint is None           # off unless CONSTRAIN_PLANKS
    assert tuple(build_model(_model_cfg(CONSTRAIN_PLANKS=True)).constraint) == (1, None)
    assert tuple(build_model(_model_cfg(CONSTRAIN_PLANKS=True, MIN_PLANKS=2, MAX_PLANKS=4)).constraint) == (2, 4)
    for bad in (dict(CONSTRAIN_PLANKS=True, MIN_PLANKS=-1), dict(CONSTRAIN_PLANKS=True, MIN_PLANKS=3, MAX_PLANKS=2),
                dict(CONSTRAIN_PLANKS=1)):
        with pytest.raises(ValueError):
            build_model(_model_cfg(**bad))


# ---------------------------------------------------------------------------------------------- the ABI
def test_abi_is_declared_and_bound():
    header = open(os.path.join(REPO, "include", "plank_hip.h")).read()
    binding = open(os.path.join(REPO, "plankassembly_amd", "_lib.py")).read()
    source = open(os.path.join(REPO, "plankassembly_amd", "csrc", "decode.hip")).read()
    assert re.search(r"\bpa_decode_constraint_set\(pa_model\* m, const pa_constraint_params\* p\);", header)
    assert re.search(r"\}\s*pa_constraint_params;", header)
    assert '"pa_decode_constraint_set"' in binding and "class ConstraintParams" in binding
    assert re.search(r'extern "C" int pa_decode_constraint_set\(', source)
    from plankassembly_amd import _lib as L
    assert [f[0] for f in L.ConstraintParams._fields_] == re.search(
        r"typedef struct \{([^}]*)\}\s*pa_constraint_params;", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1).replace(
        "int32_t", "").replace(";", " ").split()


def test_abi_export_exists_in_the_built_library():
    import ctypes
    lib = os.path.join(REPO, "plankassembly_amd", "libplank_hip.so")
    if not os.path.exists(lib):
        from plankassembly_amd.build import build
        build()
    import torch as _t                                             # noqa: F401  (torch's HIP runtime first, as _lib does)
    assert hasattr(ctypes.CDLL(lib), "pa_decode_constraint_set")
