"""Plank matching without a GPU: the restatement tests/match_reference.py against metric.HungarianMatcher
(the reference's matcher restated), the tie fallback of metric.DevicePlankScorer, the stand-alone host program of tools/match_host
(the kernel's own core, csrc/match_core.h, built by the host compiler) and the consensus utility."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import match_reference as R
from conftest import GOLDEN, REPO
from plankassembly_amd import metric as M


def host_prf(pred_boxes, gt_boxes, threshold=0.5):
    return tuple(float(x) for x in M.HungarianMatcher(threshold)(np.asarray(pred_boxes).reshape(-1, 6),
                                                                 np.asarray(gt_boxes).reshape(-1, 6)))


def counts_prf(c):
    p, r, f = M.prf_from_counts([c[0]], [c[1]], [c[2]])
    return float(p[0]), float(r[0]), float(f[0])


# ------------------------------------------------------------------------------------------------ restatement vs the matcher
def test_restatement_on_the_golden_matcher_cases():
    z = np.load(os.path.join(GOLDEN, "matcher.npz"))
    (_, case), = [c for c in R.golden_cases(GOLDEN) if c[0] == "matcher"]
    a, b, pairs, kw = R.case_args(case)
    got = R.plank_match(a, b, pairs, **kw)
    for i in range(int(z["n"])):
        assert (got[i, 1], got[i, 2]) == (len(z[f"pred{i}"]), len(z[f"gt{i}"]))
        if got[i, 3] == 0:
            assert np.allclose(counts_prf(got[i]), z[f"prf{i}"], atol=1e-7), i
            assert counts_prf(got[i]) == host_prf(z[f"pred{i}"], z[f"gt{i}"])
        else:                                              # a pair at IoU == 0.5 exactly: the stored TP is tp or more, by at most ties
            tp_ref = round(float(z[f"prf{i}"][0]) * got[i, 1])
            assert got[i, 0] <= tp_ref <= got[i, 0] + got[i, 3]
    assert int((got[:, 3] == 0).sum()) >= 4


def test_restatement_on_the_f1_fixture():
    z = np.load(os.path.join(GOLDEN, "fixture_f1.npz"))
    (_, case), = [c for c in R.golden_cases(GOLDEN) if c[0] == "fixture_f1"]
    a, b, pairs, kw = R.case_args(case)
    got = R.plank_match(a, b, pairs, **kw)
    for i in range(int(z["n"])):
        assert got[i, 1] == len(z[f"valid_pred{i}"]) - 1            # row 0 of the stored prediction is the bounding box
        assert got[i, 3] == 0
        assert np.allclose(counts_prf(got[i]), z[f"prf{i}"], atol=1e-7), i


def test_restatement_equals_the_host_matcher_where_no_pair_ties():
    """3 000 seeded cases of 0 - 20 planks a side on an 8-lattice with jitter: wherever no pair sits at IoU == threshold exactly the
    maximum matching IS the reference's TP (binary cost) - precision / recall / F1 from the integers equal HungarianMatcher's bits."""
    rng = np.random.default_rng(2024)
    compared = tied = 0
    for _ in range(3000):
        pred, gt = R.random_pair(rng)
        c = R.match_rows(R.row_of(pred, 128), R.row_of(gt, 128), filter_a=False, filter_b=False)
        assert (c[1], c[2]) == (len(pred), len(gt))
        if c[3] > 0:
            tied += 1
            continue
        assert counts_prf(c) == host_prf(pred, gt), (pred.tolist(), gt.tolist(), c)
        compared += 1
    assert compared >= 500 and tied >= 100 and compared + tied == 3000, (compared, tied)


def test_integer_iou_decisions_are_those_of_metric_py():
    """`>` and `==` against the threshold: the exact-integer quotient against metric.pairwise_iou_3d, thresholds on and off a value."""
    rng = np.random.default_rng(5)
    a, b = R.random_planks(rng, 40), R.random_planks(rng, 40, jitter=False)
    a[:4, [0, 3]] = a[:4, [3, 0]]                           # inverted planks
    iou = M.pairwise_iou_3d(a, b)
    for thr in (0.5, 0.25, 1.0 / 3.0, 0.1, float(np.unique(iou)[len(np.unique(iou)) // 2])):
        for i in range(len(a)):
            for j in range(len(b)):
                gt, tie = R.iou_decision(a[i], b[j], thr)
                assert gt == bool(iou[i, j] > thr) and tie == bool(iou[i, j] >= thr and not iou[i, j] > thr)


def test_chain_family_needs_the_augmenting_search():
    """Threshold 0.25, cubes of edge 10 shifted by 4 / 5 / 6: 0.43 is an edge, 0.25 exactly is a tie and no edge, and with shift 5
    the index-order greedy matching is one short of the maximum."""
    short = 0
    for k in (1, 2, 3, 5, 9):
        for shift, tail in ((4, True), (5, True), (5, False), (6, True)):
            pa, pb = R.chain_case(k, shift, tail)
            edges, ties = R.adjacency(pa, pb, 0.25)
            best, greedy = R.max_matching(edges, len(pb)), R.greedy_matching(edges, len(pb))
            assert greedy <= best
            short += greedy < best
            assert ties == (0 if shift == 5 else k)
            assert best == {4: k, 5: k + int(tail), 6: k + int(tail)}[shift]
            if ties == 0:
                assert counts_prf((best, len(pa), len(pb))) == host_prf(pa, pb, 0.25)
    assert short >= 5
    gt, tie = R.iou_decision((4, 0, 0, 14, 10, 10), (10, 0, 0, 20, 10, 10), 0.25)
    assert (gt, tie) == (False, True)
    assert R.iou_decision((4, 0, 0, 14, 10, 10), (0, 0, 0, 10, 10, 10), 0.25) == (True, False)


# ------------------------------------------------------------------------------------------------ DevicePlankScorer's tie fallback
def _parent_host_path(samples, truth, threshold, end):
    """The host path as the trainers run it: parse_sequence, _valid_pred, PlankScorer.add per drawing (torch, as on the parent)."""
    def parse(seq):
        valid = seq[torch.cumsum(seq == end, 0) == 0]
        return valid[: len(valid) // 6 * 6].reshape(-1, 6)

    def valid_pred(pred):
        if len(pred) <= 1:
            return pred
        ok = torch.all(torch.abs(pred[1:, 3:] - pred[1:, :3]) != 0, dim=1)
        return torch.concat((pred[:1], pred[1:][ok]))

    scorer = M.PlankScorer(threshold)
    dicts = [scorer.add(valid_pred(parse(s)), parse(t)) for s, t in zip(samples, truth)]
    return dicts, scorer.means(sync=False)


def test_device_scorer_with_tie_fallback_reproduces_the_host_means_bit_for_bit():
    rng = np.random.default_rng(77)
    pairs = [R.random_pair(rng) for _ in range(240)]
    for pred, _ in pairs[::7]:                              # zero-extent predictions: the filter of the prediction side
        if len(pred):
            pred[0, 3] = pred[0, 0]
    samples = torch.from_numpy(R.rows_of([p for p, _ in pairs], 128))
    truth = torch.from_numpy(R.rows_of([g for _, g in pairs], 130))
    launches = []

    def stub(s, t):
        launches.append(len(s))
        return torch.from_numpy(R.plank_match(s.numpy(), t.numpy(), filter_a=True, filter_b=False, threshold=0.5))

    dev = M.DevicePlankScorer(0.5, R.END, match=stub)
    got = []
    for lo in range(0, 240, 48):                            # five batches; the third is read back at once, as test_step does
        d = dev.add_batch(samples[lo:lo + 48], truth[lo:lo + 48], scores=(lo == 96))
        assert (d is None) == (lo != 96)
        if d is not None:
            got = d
    want_dicts, want = _parent_host_path(samples, truth, 0.5, R.END)
    assert got == want_dicts[96:144]
    means = dev.means(sync=False)
    assert means == want, (means, want)
    assert launches == [48] * 5 and dev.fallbacks >= 50, dev.fallbacks
    assert dev.means(sync=False) == (0.0, 0.0, 0.0)          # reset, like PlankScorer


def test_device_scorer_keep_mask_and_single_adds_keep_the_order():
    rng = np.random.default_rng(78)
    pairs = [R.random_pair(rng, 6) for _ in range(8)]
    samples = torch.from_numpy(R.rows_of([p for p, _ in pairs], 64))
    truth = torch.from_numpy(R.rows_of([g for _, g in pairs], 64))
    stub = lambda s, t: torch.from_numpy(R.plank_match(s.numpy(), t.numpy()))       # noqa: E731
    dev = M.DevicePlankScorer(0.5, R.END, match=stub)
    keep = [True, False, True, True, False, True, True, True]
    d = dev.add_batch(samples, truth, scores=True, keep=keep)
    assert [x is None for x in d] == [not k for k in keep]
    idx = [i for i, k in enumerate(keep) if k]
    want_dicts, want = _parent_host_path(samples[idx], truth[idx], 0.5, R.END)
    assert [x for x in d if x is not None] == want_dicts and dev.means(sync=False) == want


# ------------------------------------------------------------------------------------------------ the host program (csrc/match_core.h)
def _host_compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise RuntimeError("no host C++ compiler found (set CXX)")


@pytest.fixture(scope="module")
def match_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("match_host") / "match_host")
    src = os.path.join(REPO, "tools", "match_host", "main.cpp")
    r = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run_host(exe, tmp_path, case):
    a, b, pairs, kw = R.case_args(case)
    if pairs is None:
        pairs = [(i, i) for i in range(len(a))]
    lines = [f"{len(pairs)} {kw['end_token']} {int(kw['filter_a'])} {int(kw['filter_b'])} {float(kw['threshold']).hex()}"]
    for i, j in pairs:
        for row in (a[i], b[j]):
            lines.append(" ".join([str(len(row))] + [str(int(v)) for v in row]))
    path = os.path.join(str(tmp_path), "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    return np.asarray([[int(v) for v in ln.split()] for ln in r.stdout.splitlines()], dtype=np.int32).reshape(-1, 4)


def test_host_program_equals_the_restatement(match_host, tmp_path):
    cases = R.golden_cases(GOLDEN) + R.edge_cases() + [c for c in R.large_cases() if c[0] in ("170x170", "chain_170")]
    names = {n for n, _ in cases}
    assert {"matcher", "fixture_f1", "no_end_128", "end_at_0", "out_of_vocabulary", "170x170"} <= names
    for name, case in cases:
        a, b, pairs, kw = R.case_args(case)
        assert np.array_equal(_run_host(match_host, tmp_path, case), R.plank_match(a, b, pairs, **kw)), name


def test_host_program_refuses_what_the_library_refuses(match_host, tmp_path):
    for text in ("1 512 1 0 0.0\n6 0 0 0 1 1 1\n6 0 0 0 1 1 1\n", "1 512 1 0 0.5\n1027 " + "1 " * 1027 + "\n6 0 0 0 1 1 1\n"):
        path = os.path.join(str(tmp_path), "bad.txt")
        with open(path, "w") as f:
            f.write(text)
        r = subprocess.run([match_host, path], capture_output=True, text=True)
        assert r.returncode == 2 and r.stdout.strip() == "error"


# ------------------------------------------------------------------------------------------------ consensus utility
def _samples(plank_sets, length=64):
    return R.rows_of(plank_sets, length)[None]


def test_consensus_duplicates_get_equal_utilities_and_the_lowest_index_wins():
    rng = np.random.default_rng(9)
    x, y = R.random_planks(rng, 5, jitter=False), R.random_planks(rng, 4, jitter=False)
    lone = np.asarray([(200, 200, 200, 210, 210, 210)])
    uq, index, f1 = R.consensus(_samples([lone, x, y, x, x, y]))
    assert uq[0][1] == uq[0][3] == uq[0][4] and uq[0][2] == uq[0][5]
    assert index == [1]                                     # three copies of x agree best; the first of them is the most likely
    assert uq[0][1] >= 2 * 2 ** 40 and f1[0, 1] == uq[0][1] / 2.0 ** 40 / 5
    assert f1.dtype == np.float64 and f1.shape == (1, 6)
    # a rotation of the same samples: the winner is still the first copy of x
    assert R.consensus(_samples([x, lone, x, y, y, x]))[1] == [0]
    # thirds do not sum alike in floating point, the integers do: F1 = 2/3 three times either way round
    a3 = np.concatenate([x[:1], lone])
    u3 = R.consensus(_samples([x[:1], a3, a3, a3]))[0][0]
    assert u3[1] == u3[2] == u3[3] and u3[0] == 3 * round(2 / 3 * 2.0 ** 40)


def test_consensus_of_empty_samples_and_of_one_sample():
    uq, index, f1 = R.consensus(_samples([[], [], []]))
    assert uq == [[0, 0, 0]] and index == [0] and not f1.any()
    rng = np.random.default_rng(10)
    uq, index, f1 = R.consensus(_samples([R.random_planks(rng, 3)]))
    assert uq == [[0]] and index == [0] and f1.tolist() == [[0.0]]


# ------------------------------------------------------------------------------------------------ the two config keys
def test_device_metric_and_sample_select_are_read_from_the_config():
    from plankassembly_amd.config import load_cli_config
    from plankassembly_amd.trainer import Trainer

    def trainer(model=None, **hparams):
        _, _, hp = load_cli_config(os.path.join(REPO, "configs", "train_complete.yaml"))
        hp["MODEL"].update(NUM_MODEL=64, NUM_HEAD=4, NUM_FEEDFORWARD=128, NUM_ENCODER_LAYERS=1, NUM_DECODER_LAYERS=1, **(model or {}))
        hp["DATA"].update(MAX_INPUT_LENGTH=65, MAX_OUTPUT_LENGTH=36)
        hp.update(hparams)
        return Trainer(hp)

    t = trainer()
    assert type(t.scorer) is M.PlankScorer and not t.device_metric and t.model.sample_select is None
    t = trainer(dict(NUM_SAMPLES=4, SAMPLE_SELECT="consensus"), DEVICE_METRIC=True)
    assert type(t.scorer) is M.DevicePlankScorer and t.scorer.end_token == 512 and t.scorer.threshold == t.cfg.THRESHOLD
    assert t.matcher is t.scorer.matcher and t.criterion is t.scorer.criterion
    assert t.model.sample_select == "consensus" and t.model.num_samples == 4
    with pytest.raises(ValueError):
        trainer(dict(NUM_SAMPLES=4, SAMPLE_SELECT="median"))
    for model in (dict(SAMPLE_SELECT="consensus"), dict(SAMPLE_SELECT="consensus", BEAM_SIZE=4)):      # nothing to choose among
        with pytest.raises(ValueError):
            trainer(model)
