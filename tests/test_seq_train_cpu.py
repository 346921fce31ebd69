"""Sequence-level training without a GPU: the weight rules of pa_sequence_batch as tests/seq_train_reference.py
restates them, the row construction on hand-made rows, the SEQ_TRAIN block of the trainer and the per-step sampling seed."""
import ctypes
import os
import re

import numpy as np
import pytest

import seq_train_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24                                       # unit roundoff of float32
U64 = 2.0 ** -53


def some_rewards(rng, N):
    n_a, n_b = rng.integers(0, 9, size=N), np.full(N, rng.integers(1, 9))
    tp = np.array([rng.integers(0, min(a, b) + 1) for a, b in zip(n_a, n_b)])
    return R.rewards(np.stack([tp, n_a, n_b, np.zeros(N, dtype=np.int64)], 1))


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("N", [2, 3, 5, 8, 64])
def test_mean_baseline_weights_sum_to_zero(N):
    """In exact arithmetic sum_n (r_n - mean of the others) / N = 0.  The restated w_n differ from the exact ones by, with rewards in
    [0, 1]: the sum of the others (N - 2 roundings of partial sums <= N - 1: (N - 2)(N - 1) U64, which the division by N - 1 turns
    into (N - 2) U64), that division's own rounding (U64), the subtraction (U64) - N U64 so far, U64 after the division by N - and
    that division's rounding (U64 / N): at most 2 U64 in float64; then the single rounding to float32, relative U32 on |w_n| <= 1 / N.
    Summed over n in float64 (N roundings of partial sums below 1): |sum| <= N (U32 / N + 2 U64) + N U64 = U32 + 3 N U64; one more
    N U64 covers the second-order terms."""
    rng = np.random.default_rng(N)
    bound = U32 + 4 * N * U64
    worst = 0.0
    for _ in range(200):
        r = some_rewards(rng, N)
        assert r.dtype == np.float32 and 0.0 <= r.min() and r.max() <= 1.0
        w = R.reinforce_weights(r, "mean")
        total = abs(float(np.sum(w.astype(np.float64))))
        worst = max(worst, total)
        assert total <= bound, (r, w, total, bound)
    print(f"N {N}: largest |sum of weights| {worst:.3e} (bound {bound:.3e})")


@pytest.mark.parametrize("N", [2, 3, 7, 64])
def test_equal_rewards_give_exact_positive_zeros(N):
    for value in (0.0, 1.0, 0.4, 2.0 / 3.0, 0.1):
        r = np.full(N, np.float32(value), dtype=np.float32)
        w = R.reinforce_weights(r, "mean")
        assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), np.zeros(N, dtype=np.uint32)), (value, w)


def test_none_and_greedy_baselines():
    r = np.array([0.5, 0.25, 1.0], dtype=np.float32)
    assert np.array_equal(R.reinforce_weights(r, "none"), (r.astype(np.float64) / 3.0).astype(np.float32))
    w = R.reinforce_weights(r, "greedy", np.float32(0.5))
    assert np.array_equal(w, ((r.astype(np.float64) - 0.5) / 3.0).astype(np.float32)) and w[0] == 0.0 and w[1] < 0.0 < w[2]


def expected_risk(scores64, r, alpha):
    s = alpha * scores64
    q = np.exp(s - s.max())
    q = q / q.sum()
    return float(np.sum(q * (1.0 - r.astype(np.float64))))


@pytest.mark.parametrize("N,alpha", [(2, 1.0), (5, 0.5), (8, 0.05), (16, 2.0)])
def test_risk_weights_are_minus_the_derivative_of_the_expected_risk(N, alpha):
    """w_n = -d/ds_n f, f = sum_m q_m c_m with c = 1 - r in [0, 1] and q = softmax(alpha s), against the central difference with step
    h in float64.  In x = alpha s_n: g' = q_n (c_n - f), g'' = g' (1 - 2 q_n), g''' = g'' (1 - 2 q_n) - 2 g' q_n (1 - q_n), so
    |g'| <= 1, |g''| <= 1 and |g'''| <= 1.5, and f''' = alpha^3 g'''.  Truncation of the central difference: h^2 / 6 * max|f'''| <=
    h^2 alpha^3 / 4.  Cancellation: each f is N exponentials, two sums of N terms and a few more operations on values in [0, 1] -
    at most (2 N + 8) U64 - and the difference of two of them is divided by 2 h: (2 N + 8) U64 / h.  The perturbed score itself is
    rounded (|s| <= 8: 8 U64), which moves each f by at most alpha * 8 U64: 8 alpha U64 / h.  The restated weight carries the same
    (2 N + 8) U64.  h = 1e-4 keeps the first two terms near each other for alpha around 1."""
    rng = np.random.default_rng(100 + N)
    h = 1e-4
    tol = h * h * alpha ** 3 / 4.0 + (2 * N + 8) * U64 / h + 8 * alpha * U64 / h + (2 * N + 8) * U64
    worst = 0.0
    for _ in range(20):
        r = some_rewards(rng, N)
        scores = (-rng.random(N) * 8.0).astype(np.float32)
        a32 = float(np.float32(alpha))
        w = R.risk_weights64(r, scores, alpha)
        s64 = scores.astype(np.float64)
        for n in range(N):
            up, dn = s64.copy(), s64.copy()
            up[n] += h
            dn[n] -= h
            fd = (expected_risk(up, r, a32) - expected_risk(dn, r, a32)) / (2 * h)
            worst = max(worst, abs(w[n] + fd))
            assert abs(w[n] + fd) <= tol, (n, w[n], fd, tol)
    print(f"N {N} alpha {alpha}: largest |w + dR/ds| {worst:.3e} (tolerance {tol:.3e})")


def test_reward_is_prf_from_counts():
    from plankassembly_amd.metric import prf_from_counts
    counts = np.array([[0, 0, 3, 0], [0, 2, 0, 0], [0, 0, 0, 0], [2, 3, 4, 1], [5, 5, 5, 0], [1, 7, 3, 2]], dtype=np.int32)
    r = R.rewards(counts)
    assert r.dtype == np.float32 and np.array_equal(r, prf_from_counts(counts[:, 0], counts[:, 1], counts[:, 2])[2].numpy())
    assert r[0] == 0 and r[1] == 0 and r[2] == 0 and r[4] == np.float32(np.float32(2.0) / (np.float32(2.0) + np.float32(1e-10)))


# ------------------------------------------------------------------------------------------------ rows
def test_row_construction_on_hand_made_rows():
    Tmax, T = 8, 10
    tok = np.array([[R.END, R.PAD, R.PAD, R.PAD, R.PAD, R.PAD, R.PAD, R.PAD],            # END at position 0
                    [1, 2, 3, 4, 5, 6, 2, R.END],                                         # END at Tmax - 1, a pointer right before it
                    [1, 2, 3, 4, 5, 6, 7, 3],                                             # no END, a pointer at the last position
                    [9, 8, 7, R.END, R.PAD, R.PAD, R.PAD, R.PAD]], dtype=np.int64)
    att = np.full_like(tok, -1)
    att[1, 6], att[2, 7] = 1, 2
    att[3, 5] = 0                                                                         # behind the END: never read
    fe = np.array([0, 7, -1, 3], dtype=np.int32)
    counts = np.array([[0, 0, 2, 0], [1, 1, 2, 0], [1, 1, 2, 0], [0, 0, 2, 0]], dtype=np.int32)
    gt = np.full((2, T), R.PAD, dtype=np.int64)
    gt[0, :7] = [1, 2, 3, 4, 5, 6, R.END]
    gt[1, :1] = [R.END]
    gl = gt.copy()
    gl[0, 5] = R.VOCAB + 2
    out = R.sequence_batch(tok, att, fe, np.zeros(4, dtype=np.float32), counts, gt, gl, N=2, baseline="none", nll_weight=0.25)
    v, l, m, w = out["out_value"], out["out_label"], out["out_mask"], out["out_weight"]
    assert v.shape == (6, T) and l.shape == (6, T) and m.shape == (6, T) and m.dtype == np.uint8 and w.shape == (6,)
    P = R.PAD
    assert v[0].tolist() == [R.END] + [P] * 9 and l[0].tolist() == v[0].tolist() and m[0].tolist() == [0] + [1] * 9
    assert v[1].tolist() == [1, 2, 3, 4, 5, 6, 2, R.END, P, P] and m[1].tolist() == [0] * 8 + [1, 1]
    assert l[1].tolist() == [1, 2, 3, 4, 5, 6, R.VOCAB + 1, R.END, P, P]
    assert v[2].tolist() == gt[0].tolist() and l[2].tolist() == gl[0].tolist() and m[2].tolist() == [0] * 7 + [1] * 3
    assert v[3].tolist() == [1, 2, 3, 4, 5, 6, 7, 3, P, P] and R.END not in l[3] and m[3].tolist() == [0] * 8 + [1, 1]
    assert l[3].tolist() == [1, 2, 3, 4, 5, 6, 7, R.VOCAB + 2, P, P]
    assert v[4].tolist() == [9, 8, 7, R.END] + [P] * 6 and l[4].tolist() == v[4].tolist() and m[4].tolist() == [0] * 4 + [1] * 6
    assert v[5].tolist() == gt[1].tolist() and m[5].tolist() == [0] + [1] * 9
    assert w[2] == np.float32(0.25) and w[5] == np.float32(0.25)
    f1 = R.rewards(counts)
    assert np.array_equal(out["reward"], f1.reshape(2, 2)) and np.array_equal(w[[0, 1, 3, 4]], (f1.astype(np.float64) / 2).astype(np.float32))
    # without the ground-truth row: G == N and the sample rows are the same rows
    bare = R.sequence_batch(tok, att, fe, np.zeros(4, dtype=np.float32), counts, gt, gl, N=2, baseline="none")
    assert bare["out_value"].shape == (4, T) and np.array_equal(bare["out_value"], v[[0, 1, 3, 4]])
    assert np.array_equal(bare["out_label"], l[[0, 1, 3, 4]]) and np.array_equal(bare["out_mask"], m[[0, 1, 3, 4]])


# ------------------------------------------------------------------------------------------------ trainer block
GOOD = {"NUM_SAMPLES": 4}


def test_seq_train_options_defaults_and_absence():
    from plankassembly_amd.trainer import seq_train_options
    assert seq_train_options({}) is None and seq_train_options({"SEQ_TRAIN": None}) is None
    o = seq_train_options({"SEQ_TRAIN": dict(GOOD)})
    assert o == {"step": {"num_samples": 4, "temperature": 1.0, "top_k": 0, "top_p": 1.0, "objective": "reinforce", "baseline": "mean",
                          "alpha": 1.0, "nll_weight": 0.0, "constraint": None}, "start_step": 0, "seed": 0}
    o = seq_train_options({"SEQ_TRAIN": {"NUM_SAMPLES": 1, "TEMPERATURE": 1.5, "TOP_K": 20, "TOP_P": 0.9, "OBJECTIVE": "risk",
                                         "BASELINE": "none", "ALPHA": 0.05, "NLL_WEIGHT": 0.5, "CONSTRAIN_PLANKS": True,
                                         "START_STEP": 1000, "SEED": 7}})
    assert o == {"step": {"num_samples": 1, "temperature": 1.5, "top_k": 20, "top_p": 0.9, "objective": "risk", "baseline": "none",
                          "alpha": 0.05, "nll_weight": 0.5, "constraint": True}, "start_step": 1000, "seed": 7}
    assert seq_train_options({"SEQ_TRAIN": dict(GOOD, BASELINE="greedy", NLL_WEIGHT=-0.5)})["step"]["nll_weight"] == -0.5


@pytest.mark.parametrize("key,bad", [
    ("NUM_SAMPLES", 0), ("NUM_SAMPLES", 65), ("NUM_SAMPLES", 2.0), ("NUM_SAMPLES", True), ("NUM_SAMPLES", None),
    ("TEMPERATURE", 0), ("TEMPERATURE", float("inf")), ("TEMPERATURE", "hot"), ("TOP_K", -1), ("TOP_K", 1.5),
    ("TOP_P", 0), ("TOP_P", 1.5), ("OBJECTIVE", "mle"), ("OBJECTIVE", 1), ("BASELINE", "median"), ("BASELINE", True),
    ("ALPHA", 0), ("ALPHA", -1.0), ("ALPHA", float("nan")), ("ALPHA", float("inf")), ("ALPHA", "1"),
    ("NLL_WEIGHT", float("nan")), ("NLL_WEIGHT", float("inf")), ("NLL_WEIGHT", float("-inf")), ("NLL_WEIGHT", "x"),
    ("CONSTRAIN_PLANKS", 1), ("CONSTRAIN_PLANKS", "yes"), ("START_STEP", -1), ("START_STEP", 1.5), ("START_STEP", True),
    ("SEED", -1), ("SEED", 2 ** 32), ("SEED", 0.5)])
def test_seq_train_options_refuses_bad_values_by_key(key, bad):
    from plankassembly_amd.trainer import seq_train_options
    with pytest.raises(ValueError, match=key):
        seq_train_options({"SEQ_TRAIN": dict(GOOD, **{key: bad})})


def test_seq_train_options_refuses_bad_blocks():
    from plankassembly_amd.trainer import Trainer, seq_train_options
    with pytest.raises(ValueError, match="BASELINE"):
        seq_train_options({"SEQ_TRAIN": {"NUM_SAMPLES": 1}})                    # the default baseline needs two samples
    with pytest.raises(ValueError, match="NUM_SAMPLE"):
        seq_train_options({"SEQ_TRAIN": {"NUM_SAMPLE": 4}})                     # a misspelt key is not ignored
    with pytest.raises(ValueError, match="SEQ_TRAIN"):
        seq_train_options({"SEQ_TRAIN": 4})
    from test_trainer_surface import small_hparams
    with pytest.raises(ValueError, match="OBJECTIVE"):
        Trainer(small_hparams(SEQ_TRAIN=dict(GOOD, OBJECTIVE="mle")))           # the trainer validates it when it is built
    assert Trainer(small_hparams()).seq_train is None
    assert Trainer(small_hparams(SEQ_TRAIN=dict(GOOD))).seq_train["step"]["num_samples"] == 4


def test_seq_train_seed_is_the_documented_function_and_distinct():
    from plankassembly_amd.trainer import seq_train_seed
    seen = set()
    for rank in range(8):
        for step in range(1000):
            s = seq_train_seed(7, step, rank)
            assert s == (7 + 4096 * step + rank) % 2 ** 32 and 0 <= s < 2 ** 32
            seen.add(s)
    assert len(seen) == 8000
    assert seq_train_seed(2 ** 32 - 1, 2 ** 20, 3) == (2 ** 32 - 1 + 4096 * 2 ** 20 + 3) % 2 ** 32      # wraps, stays a valid seed


def test_training_step_without_the_block_makes_todays_calls():
    """No SEQ_TRAIN block: training_step calls the model once, as before, and nothing else; with the block it calls seq_train_step
    from START_STEP on, with the documented seed and the block's arguments."""
    import torch
    from plankassembly_amd.trainer import Trainer, seq_train_seed
    from test_trainer_surface import small_hparams

    class Spy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.calls = []

        def forward(self, batch):
            self.calls.append(("forward", batch))
            return {"loss": torch.tensor(2.0), "accuracy": torch.tensor(0.5)}

        def seq_train_step(self, batch, **kw):
            self.calls.append(("seq_train_step", batch, kw))
            return {"loss": torch.tensor(1.0), "accuracy": torch.tensor(0.5), "nll": torch.tensor(3.0), "reward": torch.tensor(0.25)}

    t = Trainer(small_hparams())
    t.model = Spy()
    assert float(t.training_step("b0", 0)) == 2.0 and t.model.calls == [("forward", "b0")] and t._train_reward is None
    t = Trainer(small_hparams(SEQ_TRAIN=dict(GOOD, START_STEP=2, SEED=5, NLL_WEIGHT=0.5)))
    t.model = Spy()
    t.global_step = 1
    assert float(t.training_step("b1", 0)) == 2.0 and t.model.calls == [("forward", "b1")] and t._train_reward is None
    t.global_step = 2
    assert float(t.training_step("b2", 1)) == 1.0 and float(t._train_reward) == 0.25 and float(t._train_nll) == 3.0
    name, batch, kw = t.model.calls[1]
    assert name == "seq_train_step" and batch == "b2" and kw == dict(t.seq_train["step"], seed=seq_train_seed(5, 2, 0), threshold=0.5)


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_is_declared_bound_and_sized():
    from plankassembly_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "plank_hip.h")).read()
    assert "int pa_sequence_batch(const pa_seq_batch_args* a, void* stream);" in hdr
    body = re.search(r"typedef struct \{([^}]*)\} pa_seq_batch_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [re.sub(r"^(const\s+)?\w+\s*\*?\s*", "", d.strip()) for d in body.split(";") if d.strip()]       # the type goes
    names = [n.strip() for d in decls for n in d.split(",")]
    assert names == [f[0] for f in L.SeqBatchArgs._fields_], names
    if os.path.exists(L.LIB_PATH):                                            # the size from the compiled library itself
        lib = ctypes.CDLL(L.LIB_PATH)
        lib.pa_seq_batch_args_bytes.restype = ctypes.c_int64
        assert lib.pa_seq_batch_args_bytes() == ctypes.sizeof(L.SeqBatchArgs) and hasattr(lib, "pa_sequence_batch")
