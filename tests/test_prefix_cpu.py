"""Forced prefixes and scoring: the CPU reference (tests/prefix_reference.py), the validating helper and the ABI surface.  No GPU."""
import os
import re

import pytest
import torch

from conftest import REPO
from oracle import plank_oracle as O
import beam_reference as BR
import prefix_reference as PR
import sample_reference as SR
from test_beam_cpu import load_case

V, END, PAD = 514, 512, 513


def gt_prefix(batch, P, rows=1):
    """Ground-truth prefix of P positions (clipped before END) with the pointers of output_label, per row of a batch repeated
    `rows` times."""
    tok = batch["output_value"][:, :P]
    lab = batch["output_label"][:, :P]
    att = torch.where(lab >= V, lab - V, torch.full_like(lab, -1))
    stop = (tok == END) | (tok == PAD)
    plen = torch.where(stop.any(1), stop.long().argmax(1), torch.full((tok.shape[0],), P))
    return tuple(x.repeat_interleave(rows, dim=0) for x in (plen, tok, att))


def test_empty_prefix_is_the_unforced_reference():
    sd, batch, cfg, steps = load_case("small")
    with torch.no_grad():
        a = BR.beam_search(sd, cfg, batch, 3, max_steps=steps)
        b = PR.beam_search(sd, cfg, batch, 3, max_steps=steps)
        for k in a:
            assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), k
        assert float(b["prefix_score"].abs().max()) == 0.0
        a = SR.sample_decode(sd, cfg, batch, 2, seed=3, top_k=20, max_steps=steps)
        b = PR.sample_decode(sd, cfg, batch, 2, seed=3, top_k=20, max_steps=steps)
        for k in a:
            assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), k
        s, at = O.greedy_decode_cached(sd, cfg, batch, max_steps=steps, early_stop=False)
        g = PR.greedy(sd, cfg, batch, max_steps=steps, dtype=torch.float32)
    assert torch.equal(g["tokens"], s) and torch.equal(g["attach"], at)


@pytest.mark.parametrize("name", ["small", "tiny"])
def test_fully_forced_sum_is_teacher_forced_logprob(name):
    sd, batch, cfg, steps = load_case(name)
    steps = min(steps, 24)
    with torch.no_grad():
        g = PR.greedy(sd, cfg, batch, max_steps=steps)
        s, a = g["tokens"], g["attach"]
        B = s.shape[0]
        sc, lp = PR.score(sd, cfg, batch, s, a, lengths=torch.full((B,), steps))
        tf = BR.teacher_forced_logprob(sd, cfg, batch, s[:, None], a[:, None])[:, 0]
        # forcing greedy's own output gives it back
        again = PR.greedy(sd, cfg, batch, (torch.full((B,), steps), s, a), max_steps=steps)
    assert torch.allclose(sc, tf, rtol=0, atol=1e-9), (sc, tf)
    assert lp.shape == (B, steps) and bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())
    assert torch.equal(again["tokens"], s) and torch.equal(again["attach"], a)
    # the score stops after the first END, the per-token values do not
    for r in range(B):
        n = int(g["first_end"][r]) + 1 if g["first_end"][r] >= 0 else steps
        assert abs(float(lp[r, :n].sum() - sc[r])) < 1e-9


def test_ground_truth_scores_and_invalid_candidates():
    sd, batch, cfg, _ = load_case("small")
    tok, lab = batch["output_value"], batch["output_label"]
    att = torch.where(lab >= V, lab - V, torch.full_like(lab, -1))
    with torch.no_grad():
        sc, lp = PR.score(sd, cfg, batch, tok, att)
        tf = BR.teacher_forced_logprob(sd, cfg, batch, tok[:, None, :lp.shape[1]], att[:, None, :lp.shape[1]])[:, 0]
        assert torch.allclose(sc, tf, rtol=0, atol=1e-9)
        # a pointer at t < 5 and a pointer with attach >= t are no candidates: -inf, nothing read out of bounds
        bad = att.clone()
        bad[0, 3] = 1
        bad[1, 7] = 9
        sc2, lp2 = PR.score(sd, cfg, batch, tok, bad)
    assert lp2[0, 3] == float("-inf") and lp2[1, 7] == float("-inf") and sc2[0] == float("-inf")
    assert torch.equal(lp2[2:], lp[2:])


def test_beam_and_sampling_with_a_prefix_carry_it():
    sd, batch, cfg, steps = load_case("small")
    K = 3
    pre = gt_prefix(batch, 12, K)
    with torch.no_grad():
        r = PR.beam_search(sd, cfg, batch, K, pre, max_steps=steps)
        tf = BR.teacher_forced_logprob(sd, cfg, batch, r["beam_tokens"], r["beam_attach"])
        s = PR.sample_decode(sd, cfg, batch, K, pre, seed=2, max_steps=steps)
    fin = torch.isfinite(r["scores"])
    assert bool(fin[:, 0].all()) and torch.allclose(tf[fin], r["scores"][fin], rtol=0, atol=1e-9)
    B = batch["input_value"].shape[0]
    for b in range(B):
        n = int(pre[0][b * K])
        for k in range(K):
            if fin[b, k]:
                assert torch.equal(r["beam_tokens"][b, k, :n], pre[1][b * K, :n]) and torch.equal(r["beam_attach"][b, k, :n], pre[2][b * K, :n])
            assert torch.equal(s["tokens"][b * K + k, :n], pre[1][b * K, :n]) and torch.equal(s["attach"][b * K + k, :n], pre[2][b * K, :n])
        assert abs(float(r["prefix_lp"][b, 0, :n].sum() - r["prefix_score"][b, 0])) < 1e-9
    assert bool((s["prefix_score"] <= 0).all()) and bool((s["scores"] <= s["prefix_score"] + 1e-12).all())


# ---------------------------------------------------------------------------------------------- the validating helper
def table(prefix, B=2, Tmax=16, strict=True):
    from plankassembly_amd.decode import prefix_table
    return prefix_table(prefix, B, Tmax, V, END, PAD, strict=strict)


def test_prefix_table_defaults():
    tok = torch.tensor([[1, 2, 3, 4, 5, 6, 1, END, PAD, PAD], [7, 8, 9, 10, 11, 12, PAD, PAD, PAD, PAD]])
    plen, ptok, patt = table({"tokens": tok})
    assert plen.tolist() == [8, 6]                                  # through END; PAD never counts
    assert ptok.shape == (2, 16) and patt.shape == (2, 16) and bool((patt == -1).all())
    assert ptok[0, :8].tolist() == tok[0, :8].tolist() and bool((ptok[0, 8:] == 0).all()) and bool((ptok[1, 6:] == 0).all())
    att = torch.full_like(tok, -1)
    att[0, 6] = 0
    plen, ptok, patt = table({"tokens": tok, "attach": att, "lengths": [7, 0]})
    assert plen.tolist() == [7, 0] and int(patt[0, 6]) == 0 and bool((ptok[1] == 0).all())
    assert table({"tokens": torch.zeros(2, 0, dtype=torch.long)})[0].tolist() == [0, 0]


def test_prefix_table_errors():
    tok = torch.tensor([[1, 2, 3, 4, 5, 6, 1, 2], [7, 8, 9, 10, 11, 12, 7, 9]])
    ok = torch.full_like(tok, -1)
    ok[0, 6], ok[1, 7] = 0, 2
    table({"tokens": tok, "attach": ok})

    def bad_att(r, t, j):
        a = ok.clone()
        a[r, t] = j
        return {"tokens": tok, "attach": a}

    cases = [
        {"tokens": torch.zeros(2, 17, dtype=torch.long)},           # P > Tmax
        {"tokens": torch.tensor([[1, V], [1, 2]])},                 # token outside [0, V)
        {"tokens": torch.tensor([[1, -1], [1, 2]])},
        bad_att(0, 6, 6), bad_att(0, 6, 7),                         # attach[t] >= t
        bad_att(0, 4, 0),                                           # a pointer at t < 5
        bad_att(0, 7, 0),                                           # tokens[t] != tokens[attach[t]]
        bad_att(0, 7, -2),
        {"tokens": tok, "lengths": [9, 1]}, {"tokens": tok, "lengths": [-1, 1]}, {"tokens": tok, "lengths": [1]},
        {"tokens": tok, "attach": ok[:, :4]}, {"tokens": tok[0]}, {"attach": ok}, "nothing",
    ]
    for c in cases:
        with pytest.raises(ValueError):
            table(c)
    # outside a row's length anything goes; the scorer's checks leave the pointers to the kernel
    table({"tokens": torch.tensor([[1, V + 5], [1, 2]]), "lengths": [1, 2]})
    for c in (bad_att(0, 6, 7), bad_att(0, 4, 0), bad_att(0, 7, 0)):
        table(c, strict=False)
    with pytest.raises(ValueError):
        table({"tokens": torch.tensor([[1, V], [1, 2]])}, strict=False)


def test_two_lane_decoder_refuses_a_prefix():
    import types
    from plankassembly_amd.decode import GreedyDecoder
    m = types.SimpleNamespace(max_output_length=16, vocab_size=V, token=types.SimpleNamespace(END=END, PAD=PAD))
    batch = {"input_value": torch.zeros(2, 4, dtype=torch.long)}
    pre = {"tokens": torch.tensor([[1, 2], [3, 4]])}
    with pytest.raises(ValueError):
        GreedyDecoder(m, use_graph=False, lanes=2)._check_prefix(pre, batch, None)
    assert GreedyDecoder(m, use_graph=False, lanes=1)._check_prefix(pre, batch, None)[0].tolist() == [2, 2]
    assert GreedyDecoder(m, use_graph=False, lanes=1)._check_prefix(None, batch, None) is None


# ---------------------------------------------------------------------------------------------- the ABI
NAMES = ["pa_decode_prefix_ws_bytes", "pa_decode_prefix_begin", "pa_decode_prefix_set", "pa_decode_prefix_buffers"]


def test_abi_is_declared_and_bound():
    header = open(os.path.join(REPO, "include", "plank_hip.h")).read()
    binding = open(os.path.join(REPO, "plankassembly_amd", "_lib.py")).read()
    source = open(os.path.join(REPO, "plankassembly_amd", "csrc", "decode.hip")).read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\(pa_model\* m", header), n
        assert f'"{n}"' in binding, n
        assert re.search(r'extern "C" \w+ ' + n + r"\(", source), n


def test_abi_exports_exist_in_the_built_library():
    import ctypes
    lib = os.path.join(REPO, "plankassembly_amd", "libplank_hip.so")
    if not os.path.exists(lib):
        from plankassembly_amd.build import build
        build()
    import torch as _t                                             # noqa: F401  (torch's HIP runtime first, as _lib does)
    h = ctypes.CDLL(lib)
    for n in NAMES:
        assert hasattr(h, n), n
