"""Consensus choice among samples on the GPU (PlankModel.sample(select="consensus"), decode.consensus_select)
against the restatement tests/match_reference.py, on fixture_small."""
import numpy as np
import pytest
import torch

import match_reference as R
from test_beam_gpu import dev, greedy, make

pytestmark = pytest.mark.gpu

KEYS = ("scores", "sample_tokens", "sample_attach")


def both(m, batch, N, seed, **kw):
    with torch.no_grad():
        plain = m.sample(batch, N, seed=seed, **kw)
        picked = m.sample(batch, N, seed=seed, select="consensus", **kw)
    return plain, picked


def check_against_restatement(picked, threshold=0.5):
    st = picked["sample_tokens"].cpu().numpy()
    uq, index, f1 = R.consensus(st, threshold=threshold)
    assert picked["consensus_index"].cpu().tolist() == index
    assert picked["consensus_f1"].dtype == torch.float64 and picked["consensus_f1"].is_cuda
    assert np.array_equal(picked["consensus_f1"].cpu().numpy(), f1)
    at = torch.as_tensor(index)
    rows = torch.arange(len(index))
    assert torch.equal(picked["samples"].cpu(), picked["sample_tokens"].cpu()[rows, at])
    assert torch.equal(picked["attach"].cpu(), picked["sample_attach"].cpu()[rows, at])
    for b, p in enumerate(picked["predicts"]):
        assert np.array_equal(p.cpu().numpy(), R.parse_row(np.concatenate([[0] * 6, picked["samples"][b].cpu().numpy()]), 512, False))
    return uq, index


@pytest.mark.parametrize("seed,kw", [(3, dict()), (11, dict(temperature=1.5)), (5, dict(temperature=0.7, top_k=8))])
def test_consensus_keeps_the_samples_and_picks_what_the_restatement_picks(small_fixture, seed, kw):
    sd, batch, _ = small_fixture
    m = make(sd)
    plain, picked = both(m, dev(batch), 8, seed, **kw)
    for k in KEYS:
        assert torch.equal(plain[k], picked[k]), k
    assert "consensus_index" not in plain and sorted(set(picked) - set(plain)) == ["consensus_f1", "consensus_index"]
    assert torch.equal(plain["samples"], plain["sample_tokens"][:, 0])
    uq, index = check_against_restatement(picked)
    assert len(picked["groundtruths"]) == len(index)


def test_consensus_with_its_own_threshold_and_without_parse(small_fixture):
    sd, batch, _ = small_fixture
    m = make(sd)
    with torch.no_grad():
        picked = m.sample(dev(batch), 8, seed=3, temperature=1.5, select="consensus", consensus_threshold=0.25, parse=False)
    assert "predicts" not in picked and "groundtruths" not in picked
    st = picked["sample_tokens"].cpu().numpy()
    uq, index, f1 = R.consensus(st, threshold=0.25)
    assert picked["consensus_index"].cpu().tolist() == index and np.array_equal(picked["consensus_f1"].cpu().numpy(), f1)


def hand_made_samples():
    """[B, N, n] with N = 6: duplicates, a rotation of them, thirds, all-empty, and lattice programs that share planks."""
    rng = np.random.default_rng(9)
    x, y = R.random_planks(rng, 5, jitter=False), R.random_planks(rng, 4, jitter=False)
    lone = np.asarray([(200, 200, 200, 210, 210, 210)])
    a3 = np.concatenate([x[:1], lone])
    truth = R.random_planks(rng, 9, jitter=False)
    shared = [truth[rng.permutation(9)[: int(k)]] for k in (2, 7, 8, 5, 8, 3)]          # subsets of one program
    mixed = [np.concatenate([truth[:6], R.random_planks(rng, int(k))]) for k in (4, 0, 1, 3, 0, 2)]
    mixed[4] = mixed[1].copy()                                                        # a duplicate behind a lower index
    sets = [[lone, x, y, x, x, y], [x, lone, x, y, y, x], [x[:1], a3, a3, a3, lone, []], [[]] * 6, shared, mixed]
    return np.stack([R.rows_of(s, 128) for s in sets])


@pytest.mark.parametrize("threshold", [0.5, 0.25])
def test_consensus_select_on_hand_made_samples(threshold):
    """decode.consensus_select itself against the restatement, B = 6 drawings: utilities above zero, winners other than sample 0,
    ties to the lowest index.  consensus_f1 = u_q / 2^40 / (N - 1) with u_q < 2^43: two utilities that differ give doubles that
    differ, so equal f1 bits mean equal integer utilities."""
    from plankassembly_amd.decode import consensus_select
    st = hand_made_samples()
    uq, index, f1 = R.consensus(st, threshold=threshold)
    got = consensus_select(torch.from_numpy(st).cuda(), R.END, threshold)
    assert got["consensus_index"].dtype == torch.int64 and got["consensus_index"].is_cuda
    assert got["consensus_index"].cpu().tolist() == index
    assert np.array_equal(got["consensus_f1"].cpu().numpy(), f1)
    assert index[:4] == [1, 0, 1, 0] and any(i > 0 for i in index[4:]), index
    assert uq[0][1] == uq[0][3] == uq[0][4] >= 2 * 2 ** 40 and uq[2][1] == uq[2][2] == uq[2][3] and uq[3] == [0] * 6
    assert all(max(u) > 0 for k, u in enumerate(uq) if k != 3)
    assert index[5] == 1 and uq[5][1] == uq[5][4] == max(uq[5])         # equal utilities at 1 and 4: the lower index wins
    assert len({tuple(u) for u in uq}) == 6 and all(len(set(u)) >= 2 for k, u in enumerate(uq) if k != 3)
    # every drawing on its own gives what it gives in the batch: the pair list keeps the drawings apart
    for b in (1, 4):
        one = consensus_select(torch.from_numpy(st[b:b + 1]).cuda(), R.END, threshold)
        assert one["consensus_index"].cpu().tolist() == [index[b]] and np.array_equal(one["consensus_f1"].cpu().numpy(), f1[b:b + 1])


@pytest.mark.parametrize("seed,kw,moved", [(3, dict(), True), (2, dict(temperature=1.2), True), (5, dict(temperature=0.7, top_k=8), False)])
def test_consensus_on_trained_weights_moves_the_choice(seed, kw, moved):
    """fixture_f1's briefly trained weights sample real planks: the utilities are above zero and - ``moved`` - the consensus winner
    of some drawing is not its most likely sample; the returned rows are sample_tokens[b, index] / sample_attach[b, index]."""
    from conftest import load_fixture
    sd, batch, _ = load_fixture("fixture_f1.npz")
    m = make(sd)
    plain, picked = both(m, dev(batch), 8, seed, **kw)
    for k in KEYS:
        assert torch.equal(plain[k], picked[k]), k
    uq, index = check_against_restatement(picked)
    assert sum(max(u) > 0 for u in uq) >= 3, uq
    assert float(picked["consensus_f1"].max()) > 0.0 and float(picked["consensus_f1"].max()) == max(max(u) for u in uq) / 2.0 ** 40 / 7
    if moved:
        assert any(i > 0 for i in index), index
        b = next(b for b, i in enumerate(index) if i > 0)
        assert not torch.equal(picked["samples"][b], plain["samples"][b])


def test_identical_samples_select_the_first_and_equal_greedy(small_fixture):
    sd, batch, _ = small_fixture
    m = make(sd)
    s, a = greedy(m, dev(batch))
    _, picked = both(m, dev(batch), 8, 7, top_k=1)
    assert picked["consensus_index"].cpu().tolist() == [0] * s.shape[0]
    f1 = picked["consensus_f1"].cpu()
    assert bool((f1 == f1[:, :1]).all())                           # duplicates: exactly equal utilities
    n = picked["samples"].shape[1]
    for b in range(s.shape[0]):
        e = (s[b] == 512).nonzero()
        stop = int(e[0]) + 1 if len(e) else n
        assert torch.equal(picked["samples"][b, :stop].cpu(), s[b, :stop]) and torch.equal(picked["attach"][b, :stop].cpu(), a[b, :stop])
    check_against_restatement(picked)


def test_one_sample_selects_it(small_fixture):
    sd, batch, _ = small_fixture
    m = make(sd)
    plain, picked = both(m, dev(batch), 1, 2)
    assert picked["consensus_index"].cpu().tolist() == [0] * plain["samples"].shape[0]
    assert picked["consensus_f1"].shape == (plain["samples"].shape[0], 1) and not bool(picked["consensus_f1"].any())
    assert torch.equal(plain["samples"], picked["samples"]) and torch.equal(plain["attach"], picked["attach"])


def test_sample_select_is_a_model_option(small_fixture):
    from plankassembly_amd.models import PlankModel
    sd, batch, _ = small_fixture
    m = make(sd, num_samples=4, sample_seed=3, sample_select="consensus")
    with torch.no_grad():
        out = m.eval_step(dev(batch))
    assert "consensus_index" in out
    check_against_restatement(out)
    with pytest.raises(ValueError):
        make(sd, num_samples=4, sample_select="median")
    with pytest.raises(ValueError):
        m.sample(dev(batch), 4, select="best")
    assert PlankModel._check_select("none") is None
