"""The machinery of the log-probability parity tests (tests/decode_logprob_cases.py, the teacher-forced mode of
tests/bf16_decode_sim.py) checked on the small fixture, and the power of the f32 per-token bound shown on mutated oracles.  No GPU."""
import math

import pytest
import torch

import bf16_decode_sim as SIM
import decode_logprob_cases as DL
import prefix_reference as PR
from oracle import plank_oracle as O
from test_beam_cpu import load_case

V = 514


def small(n=36, seed=11):
    sd, batch, cfg, steps = load_case("small")
    rows = list(range(batch["input_value"].shape[0]))
    tokens, attach = DL.random_forced(rows, min(n, steps), seed)
    return dict(sd=sd, cfg=cfg), batch, rows, tokens, attach


def test_generator_candidates_exist_and_pointers_are_half():
    n = 128
    rows = [0, 1, 2, 3]
    tok, att = DL.random_forced(rows, n, 5)
    assert tok.dtype == att.dtype == torch.long and tok.shape == att.shape == (4, n)
    assert int(tok.min()) >= 0 and int(tok.max()) < DL.N_VOCAB_FORCED                  # never END / PAD
    share = float((att >= 0).double().mean())
    assert 0.35 <= share <= 0.65, share
    for i, r in enumerate(rows):
        fills = DL.fill_positions(r, n)
        assert fills[0] >= 12 and fills[1] >= 12 and fills[0] != fills[1]
        for t in range(n):
            j = int(att[i, t])
            if j < 0:
                assert t not in fills
                continue
            assert 0 <= j < t and t >= 5 and int(tok[i, t]) == int(tok[i, j])
            assert DL.pointer_allowed(t, j) == (t not in fills), (r, t, j)
    # a sub-batch's sequences are those of the full batch; another seed gives other sequences
    tok2, att2 = DL.random_forced([3, 0], n, 5)
    assert torch.equal(tok2, tok[[3, 0]]) and torch.equal(att2, att[[3, 0]])
    assert not torch.equal(DL.random_forced([0], n, 6)[0], tok[:1])
    # a shorter draw of a row is a prefix of a longer one up to its own second fill position (n - 1 - r % 5)
    tok3, att3 = DL.random_forced([1], 36, 5)
    assert torch.equal(tok3[0, :34], tok[1, :34]) and torch.equal(att3[0, :34], att[1, :34])


def test_rows_of_a_batch_are_independent_in_the_oracle():
    """What licenses scoring a subset of a 256-row GPU batch on the CPU."""
    case, batch, rows, tok, att = small()
    n = tok.shape[1]
    with torch.no_grad():
        _, full = PR.score(case["sd"], case["cfg"], batch, tok, att, torch.full((4,), n))
    sub = DL.reference(case, batch, [0, 2], tok[[0, 2]], att[[0, 2]])
    assert float((sub["lp"] - full[[0, 2]]).abs().max()) <= 1e-12
    assert sub["lp32"].shape == (2, n) and sub["rows32"] == [0, 1]
    one = DL.reference(case, batch, [0, 2], tok[[0, 2]], att[[0, 2]], f32_rows=1)
    assert one["rows32"] == [0] and float((one["lp32"] - sub["lp32"][:1]).abs().max()) <= 5e-5


def test_fill_positions_score_the_fill():
    case, batch, rows, tok, att = small()
    ref = DL.reference(case, batch, rows, tok, att)
    for i, r in enumerate(rows):
        for t in DL.fill_positions(r, tok.shape[1]):
            assert abs(float(ref["lp"][i, t]) - math.log(1e-6)) < 1e-12, (r, t)
    assert int((ref["lp"] == ref["lp"][0, DL.fill_positions(0, tok.shape[1])[0]]).sum()) == 2 * len(rows)


@pytest.mark.parametrize("mode", ["all_bf16", "f32_resid", "step_all_bf16", "step_f32res"])
def test_simulation_without_rounding_is_the_float32_oracle(mode, monkeypatch):
    """The forced path of the simulation with every rounding replaced by the identity: two float32 evaluations of the same
    distribution in different association (each within 7e-6 of float64 at full size)."""
    case, batch, rows, tok, att = small()
    monkeypatch.setattr(SIM, "rb", lambda x: x)
    lp = DL.simulated(case, batch, rows, tok, att, mode)
    with torch.no_grad():
        _, want = PR.score(case["sd"], case["cfg"], batch, tok, att, torch.full((len(rows),), tok.shape[1]), dtype=torch.float32)
    assert lp.dtype == torch.float64 and lp.shape == want.shape and bool(torch.isfinite(lp).all())
    d = float((lp - want).abs().max())
    print(f"    simulation ({mode}, no rounding) against the float32 oracle: {d:.3e}")
    assert d <= 5e-5, d


def test_simulation_with_rounding_differs_and_free_running_is_unchanged():
    case, batch, rows, tok, att = small()
    ref = DL.reference(case, batch, rows, tok, att)
    for mode in ("step_all_bf16", "step_f32res", "all_bf16"):
        d = (DL.simulated(case, batch, rows, tok, att, mode) - ref["lp"]).abs()
        assert 1e-5 < float(d.max()) < 1.0, (mode, float(d.max()))                # bf16 roundings are there, and are roundings
    with torch.no_grad():
        out = SIM.run(case["sd"], case["cfg"], batch, "all_bf16", 12)
    assert len(out) == 2 and out[0].shape == (4, 12)


def test_range_stats_cover_every_token():
    d = torch.arange(2 * 1024, dtype=torch.float64).view(2, 1024) - 500.0
    st = DL.range_stats(d)
    assert sum(st[k][3] for k in st if k != "all") == st["all"][3] == d.numel()
    assert set(DL.range_stats(d[:, :128])) == {"all", (0, 6), (6, 128)}
    assert st["all"][0] == float(d.abs().max()) and abs(st[(0, 6)][2] - float(d[:, :6].mean())) < 1e-12


# ------------------------------------------------------------------------------------------ the power of the f32 per-token bound
def mutated(kind, counts):
    """O.last_row_dist with one subtle error in a copy of its distribution; counts the steps whose arg-max the error changes."""
    orig = O.last_row_dist

    def dist(p, cfg, hid, eps=1e-6):
        good = orig(p, cfg, hid, eps)
        sz = hid.shape[1]
        if sz < 6:
            return good
        t = sz - 1
        h = hid[:, t]
        prob = torch.sigmoid(O.linear(h, p["switch_head.weight"], p["switch_head.bias"]))
        allowed = (O.pointer_mask(cfg, sz)[t] != 0)[None]
        bad = good.clone()
        if kind == "last_row_left_out":        # the most recent cached hidden row (t - 1) never enters the pointer softmax
            ptr = torch.einsum("bd,bjd->bj", O.linear(h, p["pointer_head.weight"], p["pointer_head.bias"]), hid) / cfg.d_model
            ptr[:, t:] = O.NEG_INF
            s_last = O.softmax_lastdim(ptr)[:, t - 1:t]
            pd = good[:, V:] / (1 - s_last)
            pd[:, t - 1] = 0.0
            bad[:, V:] = torch.where(allowed, pd, good[:, V:])
        else:                                   # the switch gate 1 % too large
            bad[:, :V] = good[:, :V] / (1 - prob) * (1 - 1.01 * prob)
            bad[:, V:] = torch.where(allowed, good[:, V:] * 1.01, good[:, V:])
        counts["steps"] += good.shape[0]
        counts["flips"] += int((bad[:, :V + t].argmax(-1) != good[:, :V + t].argmax(-1)).sum())
        return bad
    return dist


@pytest.mark.parametrize("kind", ["last_row_left_out", "gate_times_1.01"])
def test_f32_per_token_bound_catches_a_subtly_wrong_distribution(kind, monkeypatch):
    """A device that is wrong like this cannot be built, so the bound's power is shown on the float32 oracle: each mutation fails
    the per-token bound the GPU tests hold the f32 step to, while the arg-max - all the token-exact tests see - hardly moves."""
    case, batch, rows, tok, att = small()
    ref = DL.reference(case, batch, rows, tok, att)
    assert len(DL.f32_per_token_failures(ref["lp32"], ref["lp"])) == 0             # the unmutated float32 oracle passes
    own = float((ref["lp32"] - ref["lp"]).abs().max())
    counts = {"steps": 0, "flips": 0}
    monkeypatch.setattr(O, "last_row_dist", mutated(kind, counts))
    with torch.no_grad():
        _, lp = PR.score(case["sd"], case["cfg"], batch, tok, att, torch.full((len(rows),), tok.shape[1]), dtype=torch.float32)
    fails = DL.f32_per_token_failures(lp, ref["lp"])
    fin = torch.isfinite(lp)
    worst = float((lp - ref["lp"])[fin].abs().max())
    print(f"    {kind}: {len(fails)} of {lp.numel()} tokens miss the 1e-4 bound (largest finite deviation {worst:.3e}; the unmutated "
          f"float32 oracle: {own:.3e}); the arg-max differs at {counts['flips']} of {counts['steps']} row-steps")
    assert len(fails) > 0 and worst > DL.F32_TOKEN_BOUND
    assert counts["steps"] == len(rows) * (tok.shape[1] - 5)


def test_simulation_mode_follows_the_switches_of_decode_modes(monkeypatch):
    """decode_logprob_cases.sim_mode restates csrc/decode.hip decode_modes(): `f32res` at d_model 512, at most 512 rows, unless
    PLANK_DECODE_F32_RESID=0 or the LayerNorm fold is forced off."""
    G = DL
    for k in ("PLANK_DECODE_F32_RESID", "PLANK_DECODE_FOLD_LN"):
        monkeypatch.delenv(k, raising=False)
    assert [G.sim_mode(c) for c in "ABCDEF"] == ["step_f32res"] * 4 + ["step_all_bf16"] * 2
    monkeypatch.setenv("PLANK_DECODE_F32_RESID", "0")
    assert {G.sim_mode(c) for c in "ABCDEF"} == {"step_all_bf16"}
    monkeypatch.setenv("PLANK_DECODE_F32_RESID", "1")
    monkeypatch.setenv("PLANK_DECODE_FOLD_LN", "0")
    assert {G.sim_mode(c) for c in "ABCDEF"} == {"step_all_bf16"}
    assert set(G.CASES["C"]["rows"]) >= {0, 1, 127, 128, 255} and len(G.CASES["C"]["rows"]) == 16
    assert all(len(G.CASES[c]["rows"]) == 4 for c in "ABE") and {0, 15} <= set(G.CASES["A"]["rows"]) and {0, 39} <= set(G.CASES["B"]["rows"])
    assert {0, 519} <= set(G.CASES["E"]["rows"]) and len(G.CASES["D"]["rows"]) == 2
