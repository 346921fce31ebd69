"""The assembly volume on the GPU: ops.plank_volume / pa_plank_volume against the restatement of
tests/volume_reference.py by integer equality, then decode.volume_select, PlankModel.volume / sample(select="volume") and the
trainer hparam VOLUME_METRIC.  A few launches, each well under a second."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import volume_reference as R
from conftest import REPO, load_fixture
from test_beam_gpu import dev, make

pytestmark = pytest.mark.gpu
END = R.END
SELECT_KEYS = ["self_overlap", "volume_index", "volume_iou"]


def gpu_volume(a, b=None, pairs=None, **kw):
    from plankassembly_amd import ops
    out = ops.plank_volume(torch.as_tensor(np.asarray(a)).cuda(), None if b is None else torch.as_tensor(np.asarray(b)).cuda(), pairs,
                           end_token=END, **kw)
    assert out.dtype == torch.int64 and out.is_cuda and out.shape[1] == 8
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def table():
    a, b = R.case_table()
    return a, b, R.volume_counts(a, b)


# ------------------------------------------------------------------------------------------------------------------ the kernel
def test_the_table_in_one_launch_and_twice_the_same(table):
    a, b, want = table
    assert a.shape[1] == 132
    first = gpu_volume(a, b)
    assert np.array_equal(first, want)
    assert np.array_equal(gpu_volume(a, b), first)                          # bitwise equal on the same input
    for name, ra, rb, answer in R.hand_cases():
        assert gpu_volume([ra], None if rb is None else [rb])[0].tolist() == answer, name


def test_pair_lists_strides_and_no_b_side(table):
    from plankassembly_amd import ops
    a, b, _ = table
    pairs = [(3, 7), (0, 0), (47, 1), (7, 3), (7, 3)]
    assert np.array_equal(gpu_volume(a, b, pairs), R.volume_counts(a, b, pairs))
    assert np.array_equal(gpu_volume(a, b, torch.tensor(pairs, dtype=torch.int64).cuda()), R.volume_counts(a, b, pairs))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    one = ta[5:6].expand(len(b), -1)                                        # stride_a = 0: one row of a against every row of b
    assert one.stride(0) == 0
    got = ops.plank_volume(one, tb, end_token=END).cpu().numpy()
    assert np.array_equal(got, R.volume_counts(a, b, [(5, j) for j in range(len(b))]))
    wide = torch.full((len(a), 200), 7, dtype=torch.int64, device="cuda")   # a slice: the row stride is not the row length
    wide[:, 10:142] = ta
    assert np.array_equal(ops.plank_volume(wide[:, 10:142], tb, end_token=END).cpu().numpy(), R.volume_counts(a, b))
    assert np.array_equal(ops.plank_volume(ta[:, :60], tb[:, :100], end_token=END).cpu().numpy(), R.volume_counts(a[:, :60], b[:, :100]))
    # no b side: the self-overlap-only call
    want = R.volume_counts(a, None)
    assert not want[:, [2, 3, 4, 7]].any() and np.array_equal(want[:, 5], want[:, 0])
    assert np.array_equal(gpu_volume(a), want)
    assert np.array_equal(gpu_volume(a, None, [4, 4, 0]), want[[4, 4, 0]])
    assert ops.plank_volume(ta, tb, [], end_token=END).shape == (0, 8)
    with pytest.raises(IndexError):
        ops.plank_volume(ta, tb, [(0, len(b))], end_token=END)
    with pytest.raises(IndexError):
        ops.plank_volume(ta, None, [len(a)], end_token=END)
    with pytest.raises(ValueError):
        ops.plank_volume(ta, tb[:5], end_token=END)
    with pytest.raises(TypeError):
        ops.plank_volume(ta.cpu(), tb, end_token=END)
    with pytest.raises(TypeError):
        ops.plank_volume(ta.int(), tb, end_token=END)


def test_plank_counts_0_1_2_21_a_side():
    rng = np.random.default_rng(5)
    rows = {k: R.row_of([R.random_box(rng, 31, 1, 14) for _ in range(k)], 132) for k in (0, 1, 2, 21)}
    ks = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 2), (2, 1), (21, 21), (21, 0), (2, 21)]
    a, b = np.stack([rows[i] for i, _ in ks]), np.stack([rows[j] for _, j in ks])
    want = R.volume_counts(a, b)
    assert want[:, 6:].tolist() == [list(k) for k in ks]
    assert np.array_equal(want, R.voxel_counts(a, b, bits=5))
    assert np.array_equal(gpu_volume(a, b), want)


@pytest.mark.parametrize("total", [63, 64, 65, 127, 128, 129])
def test_bit_row_word_edges(total):
    """Rows exactly as long as their planks: the launch's capacity, and so its bit rows, end at `total` boxes."""
    rng = np.random.default_rng(total)
    na = (total + 1) // 2
    nb = total - na
    a = R.row_of([R.random_box(rng, 31, 1, 10) for _ in range(na)], 6 * (na + 1))[None]
    b = R.row_of([R.random_box(rng, 31, 1, 10) for _ in range(nb)], 6 * (nb + 1))[None]
    want = R.volume_counts(a, b)
    assert want[0, 6:].tolist() == [na, nb]
    assert np.array_equal(want, R.voxel_counts(a, b, bits=5))
    assert np.array_equal(gpu_volume(a, b), want)


def test_170_planks_a_side():
    """One launch of four pairs at the LDS ceiling: dense random, all disjoint, all identical, a against an empty b."""
    a, b = R.ceiling_pairs()
    assert a.shape == (4, 1026) and b.shape == (4, 1026)
    want = R.volume_counts(a, b)
    assert want[:, 6].tolist() == [170] * 4 and want[:, 7].tolist() == [170, 170, 170, 0]
    assert np.array_equal(gpu_volume(a, b), want)


def test_tokens_outside_int16():
    rng = np.random.default_rng(9)
    edge = np.asarray([-2 ** 40, -32770, -32769, -32768, -32767, -1, 0, 1, 32766, 32767, 32768, 2 ** 31, 2 ** 40, 2 ** 62])
    rows_a, rows_b = [], []
    for _ in range(12):
        for rows in (rows_a, rows_b):
            planks = []
            for _ in range(int(rng.integers(1, 6))):
                lo, hi = rng.choice(edge, 3), rng.choice(edge, 3)
                planks.append(np.concatenate((np.minimum(lo, hi), np.maximum(lo, hi) if rng.random() < 0.8 else lo)))
            rows.append(R.row_of(planks, 48, plank0=(-2 ** 50, 0, 0, 2 ** 50, 1, 1)))
    a, b = np.stack(rows_a), np.stack(rows_b)
    want = R.volume_counts(a, b)
    assert want[:, 5].max() > 2 ** 40 and (want[:, 4] > 0).any()            # volumes past 2^40: the int64 sums carry them
    assert np.array_equal(gpu_volume(a, b), want)


def test_the_launch_captures_into_a_graph(table):
    from plankassembly_amd import ops
    a, b, _ = table
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.plank_volume(ta, tb, end_token=END)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.plank_volume(ta, tb, end_token=END)
    ta.copy_(torch.flip(ta, [0]))                                           # new rows, same buffers: the replays must see them
    g.replay()
    torch.cuda.synchronize()
    first = out.cpu().numpy().copy()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), first)
    assert np.array_equal(first, R.volume_counts(a[::-1], b))


def test_error_statuses_come_back_without_a_launch():
    from plankassembly_amd import _lib as L
    from plankassembly_amd import ops
    W = 1030
    rows = torch.zeros((2, W), dtype=torch.int64, device="cuda")
    out = torch.full((2, 8), -7, dtype=torch.int64, device="cuda")
    one = torch.zeros(2, dtype=torch.int32, device="cuda")

    def call(seq_a=rows, seq_b=rows, len_a=64, len_b=64, stride_a=W, stride_b=W, pa=None, pb=None, n=2, dof=6, o=out):
        return L.lib().pa_plank_volume(L.ptr(seq_a), C.c_int64(stride_a), len_a, L.ptr(seq_b), C.c_int64(stride_b), len_b, L.ptr(pa),
                                       L.ptr(pb), n, END, dof, L.ptr(o), L.stream())

    assert call(len_a=1027) == -3 and call(len_b=1027) == -3 and call(dof=4) == -3 and call(dof=0) == -3        # PA_ESHAPE
    for kw in (dict(seq_a=None), dict(o=None), dict(pa=one), dict(pb=one), dict(stride_a=-1), dict(stride_b=-1), dict(len_a=-1),
               dict(len_b=-1), dict(n=-1)):
        assert call(**kw) == -1, kw                                                                            # PA_EINVAL
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7).all())                          # nothing was launched
    assert call(len_a=1026, len_b=1026) == 0                # the limit itself runs: 170 planks of zeros a side occupy nothing
    assert call(seq_b=None, len_b=-5, stride_b=-5) == 0     # without a b side its len and stride are not read
    torch.cuda.synchronize()
    assert not out.any()
    with pytest.raises(L.PlankHipError):
        ops.plank_volume(rows, rows, end_token=END)           # 1030 tokens


# ------------------------------------------------------------------------------------------------------------------- the model
def host_select(sample_tokens):
    """volume_index, volume_iou and self_overlap of [B, N, n] samples by the restatement."""
    B, N, _ = sample_tokens.shape
    pairs = [(n, m) for n in range(N) for m in range(n + 1, N)]
    counts = np.stack([R.volume_counts(sample_tokens[b], sample_tokens[b], pairs) for b in range(B)])
    index, mean = R.select(counts, N)
    own = np.stack([R.scores(R.volume_counts(sample_tokens[b], None))["self_overlap_a"] for b in range(B)])
    return index, mean, own


def check_selected(plain, picked):
    for k in ("scores", "sample_tokens", "sample_attach"):
        assert torch.equal(plain[k], picked[k]), k
    assert sorted(set(picked) - set(plain)) == SELECT_KEYS
    index = picked["volume_index"]
    assert index.dtype == torch.int64 and index.is_cuda and picked["volume_iou"].dtype == torch.float64
    rows = torch.arange(index.shape[0], device=index.device)
    assert torch.equal(picked["samples"], picked["sample_tokens"][rows, index])
    assert torch.equal(picked["attach"], picked["sample_attach"][rows, index])
    want_index, want_mean, want_own = host_select(picked["sample_tokens"].cpu().numpy())
    assert index.cpu().tolist() == want_index.tolist()
    assert np.array_equal(picked["volume_iou"].cpu().numpy().view(np.int64), want_mean.view(np.int64))
    assert np.array_equal(picked["self_overlap"].cpu().numpy().view(np.int64), want_own.view(np.int64))
    return picked["volume_iou"].cpu().tolist()


@pytest.mark.parametrize("share", [False, True])
def test_sample_select_volume_returns_the_indexed_sample(small_fixture, share):
    sd, batch, _ = small_fixture
    m = make(sd)
    with torch.no_grad():
        plain = m.sample(dev(batch), 4, seed=3, share_encoder=share)
        picked = m.sample(dev(batch), 4, seed=3, select="volume", share_encoder=share)
    print("small volume_iou", check_selected(plain, picked))
    assert len(picked["predicts"]) == batch["input_value"].shape[0]


def test_sample_select_volume_on_trained_weights_and_as_a_model_option():
    """fixture_f1's briefly trained weights sample real planks: the solids are not empty."""
    from plankassembly_amd.decode import plank_grammar
    sd, batch, _ = load_fixture("fixture_f1.npz")
    m = make(sd, num_samples=4, sample_seed=2, temperature=1.2, sample_select="volume")
    with torch.no_grad():
        plain = m.sample(dev(batch), 4, seed=2, temperature=1.2, parse=False, constraint=plank_grammar())
        picked = m.sample(dev(batch), 4, seed=2, temperature=1.2, select="volume", parse=False, constraint=plank_grammar())
        out = m.eval_step(dev(batch), parse=False)
        same = m.sample(dev(batch), 4, seed=2, temperature=1.2, select="volume", parse=False)
    mean = check_selected(plain, picked)
    print("trained volume_iou", mean)
    assert max(max(row) for row in mean) > 0.0
    assert "volume_index" in out and all(torch.equal(out[k], same[k]) for k in SELECT_KEYS + ["samples"])
    with pytest.raises(ValueError):
        m.sample(dev(batch), 4, select="median")


def test_volume_select_on_hand_built_samples():
    from plankassembly_amd.decode import volume_scores, volume_select
    x = R.row_of([(0, 0, 0, 4, 4, 4), (2, 2, 2, 8, 8, 8)], 36)
    y = R.row_of([(1, 1, 1, 5, 5, 5)], 36)
    z = R.row_of([(20, 20, 20, 22, 22, 22)], 36)
    e = R.row_of([], 36)
    st = np.stack([np.stack(rows) for rows in ([y, x, x, z], [x, x, x, x], [e, e, z, e], [z, y, x, y], [e, e, e, e])])
    got = volume_select(torch.from_numpy(st).cuda(), END)
    assert sorted(got) == SELECT_KEYS
    index, mean, own = host_select(st)
    assert got["volume_index"].cpu().tolist() == index.tolist() == [1, 0, 0, 1, 0]
    assert np.array_equal(got["volume_iou"].cpu().numpy().view(np.int64), mean.view(np.int64))
    assert np.array_equal(got["self_overlap"].cpu().numpy().view(np.int64), own.view(np.int64))
    single = volume_select(torch.from_numpy(st[:, :1]).cuda(), END)          # nothing to compare with: index 0, the self-overlap stays
    assert single["volume_index"].cpu().tolist() == [0] * 5 and not single["volume_iou"].any()
    assert np.array_equal(single["self_overlap"].cpu().numpy(), own[:, :1])
    # volume_scores: against a reference, and the self-overlap alone
    ref, tok = st[:, 0], st[:, 1]
    r = volume_scores(torch.from_numpy(ref).cuda(), torch.from_numpy(tok).cuda(), END)
    assert sorted(r) == ["self_overlap", "volume_counts", "volume_iou", "volume_precision", "volume_recall"]
    want = R.volume_counts(ref, tok)
    s = R.scores(want)
    assert np.array_equal(r["volume_counts"].cpu().numpy(), want)
    for k, w in (("volume_iou", "volume_iou"), ("volume_precision", "volume_precision"), ("volume_recall", "volume_recall"),
                 ("self_overlap", "self_overlap_b")):
        assert r[k].dtype == torch.float64 and np.array_equal(r[k].cpu().numpy().view(np.int64), s[w].view(np.int64)), k
    alone = volume_scores(None, torch.from_numpy(tok).cuda(), END)
    assert sorted(alone) == ["self_overlap", "volume_counts"]
    assert np.array_equal(alone["volume_counts"].cpu().numpy(), R.volume_counts(tok, None))
    assert np.array_equal(alone["self_overlap"].cpu().numpy(), s["self_overlap_b"])


@pytest.mark.parametrize("fixture", ["fixture_small.npz", "fixture_f1.npz"])
def test_model_volume_equals_the_restatement_on_the_greedy_rows(fixture):
    sd, batch, _ = load_fixture(fixture)
    m = make(sd)
    with torch.no_grad():
        rows = m.eval_step(dev(batch), parse=False)["samples"]
        r = m.volume(dev(batch))
        given = m.volume(dev(batch), rows.cpu())
    want = R.volume_counts(batch["output_value"].numpy(), rows.cpu().numpy())
    print(fixture, want.tolist())
    assert np.array_equal(r["volume_counts"].cpu().numpy(), want) and torch.equal(given["volume_counts"], r["volume_counts"])
    s = R.scores(want)
    for k, w in (("volume_iou", "volume_iou"), ("volume_precision", "volume_precision"), ("volume_recall", "volume_recall"),
                 ("self_overlap", "self_overlap_b")):
        assert r[k].is_cuda and np.array_equal(r[k].cpu().numpy().view(np.int64), s[w].view(np.int64)), k


# ----------------------------------------------------------------------------------------------------------------- the trainer
def f1_trainer(**extra):
    from plankassembly_amd.config import load_cli_config
    from plankassembly_amd.trainer import Trainer
    _, _, hp = load_cli_config(os.path.join(REPO, "configs", "train_complete.yaml"))
    hp["MODEL"].update(NUM_MODEL=64, NUM_HEAD=4, NUM_FEEDFORWARD=128, NUM_ENCODER_LAYERS=2, NUM_DECODER_LAYERS=2,
                       DROPOUT=0.0, COMPUTE_DTYPE="f32")
    hp["DATA"].update(MAX_INPUT_LENGTH=65, MAX_OUTPUT_LENGTH=36)
    hp.update(extra)
    sd, batch, g = load_fixture("fixture_f1.npz")
    t = Trainer(hp)
    t.model.load_state_dict(sd)
    t.model.cuda().eval()
    return t, t.model.prepare_batch(batch), g


def test_trainer_logs_the_four_volume_means(tmp_path):
    logged = {}
    for key, extra in (("off", {}), ("host", dict(VOLUME_METRIC=True)), ("device", dict(VOLUME_METRIC=True, DEVICE_METRIC=True))):
        t, gb, g = f1_trainer(**extra)
        t.logger = types.SimpleNamespace(log_dir=str(tmp_path / key), log=lambda *a: None)
        with torch.no_grad():
            t.validation_step(gb, 0)
            t.validation_step(gb, 1)
            t.validation_epoch_end()
            t.test_step(dict(gb, name=[f"f1case{i}" for i in range(int(g["n"]))]), 0)
            t.test_epoch_end()
            rows = t.model.eval_step(gb, parse=False)["samples"].cpu().numpy()
        logged[key] = dict(t._logged)
    before = ["test/fmeasure", "test/precision", "test/recall", "val/fmeasure", "val/precision", "val/recall"]
    keys = ["volume_iou", "volume_precision", "volume_recall", "self_overlap"]
    assert sorted(logged["off"]) == before
    assert sorted(logged["host"]) == sorted(before + [f"{s}/{k}" for s in ("val", "test") for k in keys])
    assert logged["device"] == logged["host"] and all(logged["host"][k] == logged["off"][k] for k in before)
    # the means from the host: the restatement's counts and scores on the returned programs, summed as the trainer sums them
    s = R.scores(R.volume_counts(gb["output_value"].cpu().numpy(), rows))
    n = len(rows)
    for k, w in zip(keys, ("volume_iou", "volume_precision", "volume_recall", "self_overlap_b")):
        v = torch.from_numpy(s[w]).cuda()
        assert logged["host"][f"val/{k}"] == float((v.sum() + v.sum()).cpu()) / (2 * n), k
        assert logged["host"][f"test/{k}"] == float(v.sum().cpu()) / n, k
    print("logged", {k: logged["host"][f"val/{k}"] for k in keys})
    assert logged["host"]["val/volume_iou"] > 0.0
