"""Sampling: the CPU reference (tests/sample_reference.py), its random numbers and the configuration surface.  No GPU."""
import math

import numpy as np
import pytest
import torch

from oracle import plank_oracle as O
import beam_reference as BR
import sample_reference as SR
from test_beam_cpu import _model_cfg, load_case


@pytest.mark.parametrize("name", ["small", "tiny"])
def test_reference_top_k1_is_greedy(name):
    sd, batch, cfg, steps = load_case(name)
    with torch.no_grad():
        s_ref, a_ref = O.greedy_decode_cached(sd, cfg, batch, max_steps=steps, early_stop=False)
        r = SR.sample_decode(sd, cfg, batch, 2, seed=5, temperature=2.0, top_k=1, max_steps=steps, early_stop=False,
                             dtype=torch.float32)
    for row in range(r["tokens"].shape[0]):
        i = row // 2
        ends = (s_ref[i] == cfg.end).nonzero()
        n = int(ends[0]) + 1 if len(ends) else s_ref.shape[1]
        assert torch.equal(r["tokens"][row, :n], s_ref[i, :n]) and torch.equal(r["attach"][row, :n], a_ref[i, :n]), row
        assert bool((r["tokens"][row, n:] == cfg.pad).all()) and bool((r["attach"][row, n:] == -1).all())


@pytest.mark.parametrize("name,setting", [("small", dict()), ("tiny", dict(temperature=1.3, top_k=50, top_p=0.95))])
def test_reference_scores_are_teacher_forced_sums(name, setting):
    sd, batch, cfg, steps = load_case(name)
    N = 3
    with torch.no_grad():
        r = SR.sample_decode(sd, cfg, batch, N, seed=11, max_steps=min(steps, 24), **setting)
        n = r["steps"]
        B = r["tokens"].shape[0] // N
        tf = BR.teacher_forced_logprob(sd, cfg, batch, r["tokens"][:, :n].view(B, N, n), r["attach"][:, :n].view(B, N, n))
    assert bool(torch.isfinite(r["scores"]).all())
    assert torch.allclose(tf.view(-1), r["scores"], rtol=0, atol=1e-9), (tf, r["scores"])


def test_u_is_close_to_uniform():
    """Kolmogorov-Smirnov statistic of 2^16 draws against U(0, 1), below the 1e-3 critical value (1.95 / sqrt(n))."""
    g = np.arange(1 << 16, dtype=np.uint64)
    u = np.sort(SR.sample_u(7, g >> np.uint64(10), (g >> np.uint64(4)) & np.uint64(63), g & np.uint64(15)))
    n = len(u)
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
    d = max(float((np.arange(1, n + 1) / n - u).max()), float((u - np.arange(n) / n).max()))
    assert d < 1.95 / math.sqrt(n), d


@pytest.mark.parametrize("seed", [0, 0xFFFFFFFF])
def test_hash_has_no_collisions_on_a_grid(seed):
    """The 32-bit hashes of a 64 x 64 x 64 (b, n, t) grid are distinct (u itself keeps 24 of their bits, so ~2 000 of the 2^18 u
    values of such a grid coincide by the birthday bound)."""
    b, n, t = np.meshgrid(np.arange(64), np.arange(64), np.arange(64), indexing="ij")
    h = SR.sample_hash(seed, b.ravel(), n.ravel(), t.ravel())
    assert len(np.unique(h)) == h.size


def test_select_filters():
    """Rank order, top-k, top-p and the index-order draw on a hand-made row."""
    p = np.array([0.1, 0.4, 0.0, 0.2, 0.2, 0.1])
    # u = 0: the first kept candidate in index order
    assert SR.select(p, 0.0)[0] == 0
    assert SR.select(p, 0.0, top_k=1)[0] == 1
    # top_k = 3: ranks 1, 3, 4 (the tie 3 / 4 and 0 / 5 go to the smaller index); w = p / 0.4
    assert SR.select(p, 0.0, top_k=3)[0] == 1 and SR.select(p, 0.999, top_k=3)[0] == 4
    assert SR.select(p, 0.999, top_k=2)[0] == 3
    # top_p = 0.5 of the total 2.5 (w): 1.0 (index 1) + 0.5 (index 3) = 1.5 >= 1.25
    assert SR.select(p, 0.999, top_p=0.5)[0] == 3
    assert SR.select(p, 0.999)[0] == 5
    assert SR.select(p, 0.999)[1] is False
    # a draw right at a prefix-sum edge is flagged
    assert SR.select(p, 0.1, tol=1e-4) == (1, True)             # u W = 0.25 = the prefix sum before index 1


def test_config_sample_keys_accepted():
    from plankassembly_amd.models import build_model
    m = build_model(_model_cfg())
    assert m.num_samples == 0
    m = build_model(_model_cfg(NUM_SAMPLES=0, BEAM_SIZE=4))
    assert m.num_samples == 0 and m.beam_size == 4
    m = build_model(_model_cfg(NUM_SAMPLES=8, TEMPERATURE=0.8, TOP_K=50, TOP_P=0.95, SAMPLE_SEED=123, LENGTH_PENALTY=0.6))
    assert m.num_samples == 8 and m.beam_size == 1 and math.isclose(m.length_penalty, 0.6)
    assert m.sample_cfg == dict(temperature=0.8, top_k=50, top_p=0.95, seed=123)
    m = build_model(_model_cfg(NUM_SAMPLES=64, TOP_P=1.0, TEMPERATURE=1, BEAM_SIZE=1))
    assert m.num_samples == 64 and m.sample_cfg["temperature"] == 1.0


@pytest.mark.parametrize("extra", [
    dict(NUM_SAMPLES=-1), dict(NUM_SAMPLES=65), dict(NUM_SAMPLES=2.5), dict(NUM_SAMPLES=True), dict(NUM_SAMPLES="4"),
    dict(NUM_SAMPLES=4, TEMPERATURE=0.0), dict(NUM_SAMPLES=4, TEMPERATURE=-1.0), dict(NUM_SAMPLES=4, TEMPERATURE=float("inf")),
    dict(NUM_SAMPLES=4, TEMPERATURE=float("nan")), dict(NUM_SAMPLES=4, TOP_K=-1), dict(NUM_SAMPLES=4, TOP_K=2.5),
    dict(NUM_SAMPLES=4, TOP_P=0.0), dict(NUM_SAMPLES=4, TOP_P=1.5), dict(NUM_SAMPLES=4, TOP_P=float("nan")),
    dict(NUM_SAMPLES=4, SAMPLE_SEED=-1), dict(NUM_SAMPLES=4, SAMPLE_SEED=1 << 32), dict(NUM_SAMPLES=4, SAMPLE_SEED=1.5),
    dict(TEMPERATURE=0.0), dict(TOP_P=2.0),
    dict(NUM_SAMPLES=4, BEAM_SIZE=4), dict(NUM_SAMPLES=1, BEAM_SIZE=2),
])
def test_config_rejects_invalid_sample_keys(extra):
    from plankassembly_amd.models import build_model
    with pytest.raises(ValueError):
        build_model(_model_cfg(**extra))
