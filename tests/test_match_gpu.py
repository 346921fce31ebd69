"""The plank-matching kernel on the GPU (csrc/match.hip, include/plank_hip.h pa_plank_match, ops.plank_match):
all four integers of every pair equal the restatement tests/match_reference.py, exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import match_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def gpu_match(a, b, pairs=None, **kw):
    from plankassembly_amd import ops
    out = ops.plank_match(torch.as_tensor(a).cuda(), torch.as_tensor(b).cuda(), pairs, **kw)
    assert out.dtype == torch.int32 and out.is_cuda
    return out.cpu().numpy()


def check(case, name):
    a, b, pairs, kw = R.case_args(case)
    got, want = gpu_match(a, b, pairs, **kw), R.plank_match(a, b, pairs, **kw)
    assert got.shape == want.shape and np.array_equal(got, want), (name, got.tolist(), want.tolist())
    return got


@pytest.mark.parametrize("name,case", R.golden_cases(GOLDEN), ids=lambda v: v if isinstance(v, str) else "")
def test_golden_cases(name, case):
    check(case, name)


@pytest.mark.parametrize("name,case", R.edge_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_edge_cases(name, case):
    got = check(case, name)
    if name == "no_end_128":
        assert got.tolist() == [[20, 20, 20, 0]]
    if name == "chain_025":
        assert int((got[:, 3] > 0).sum()) >= 10 and int((got[:, 3] == 0).sum()) >= 10


@pytest.mark.parametrize("name,case", R.large_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_large_cases(name, case):
    got = check(case, name)
    if name == "chain_170":
        assert got.tolist() == [[170, 170, 170, 0]]        # an augmenting path through all 339 edges


def test_random_family_in_one_launch():
    rng = np.random.default_rng(31)
    pairs = [R.random_pair(rng) for _ in range(300)]
    a, b = R.rows_of([p for p, _ in pairs], 128), R.rows_of([g for _, g in pairs], 128)
    got = gpu_match(a, b, end_token=R.END, filter_a=True, filter_b=False, threshold=0.5)
    want = R.plank_match(a, b)
    assert np.array_equal(got, want)
    assert int((want[:, 3] > 0).sum()) >= 30 and int((want[:, 0] > 0).sum()) >= 100


def test_pair_lists_strides_and_shared_tensor():
    from plankassembly_amd import ops
    rng = np.random.default_rng(32)
    sets = [R.random_planks(rng, int(n), jitter=False) for n in rng.integers(0, 9, size=7)]
    sets[3] = sets[1].copy()
    rows = R.rows_of(sets, 64)
    kw = dict(end_token=R.END, filter_a=True, filter_b=True, threshold=0.5)
    dev_rows = torch.from_numpy(rows).cuda()
    # a and b the same tensor, identity: every program against itself
    got = ops.plank_match(dev_rows, dev_rows, **kw).cpu().numpy()
    assert np.array_equal(got, R.plank_match(rows, rows, **kw))
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 1], got[:, 2])
    # explicit pairs with repeated rows, as a list, a host tensor and a device tensor
    pairs = [(0, 1), (1, 3), (1, 3), (6, 0), (2, 2), (5, 4), (0, 1)]
    want = R.plank_match(rows, rows, pairs, **kw)
    for p in (pairs, torch.tensor(pairs), torch.tensor(pairs, dtype=torch.int32).cuda()):
        assert np.array_equal(ops.plank_match(dev_rows, dev_rows, p, **kw).cpu().numpy(), want)
    assert want[1].tolist() == want[2].tolist() and want[1, 0] == want[1, 1]
    # rows with stride > len: a column slice (stride 64, len 40) and every second row of it
    sl = dev_rows[:, :40]
    assert sl.stride(0) == 64 and not sl.is_contiguous()
    assert np.array_equal(ops.plank_match(sl, dev_rows, **kw).cpu().numpy(), R.plank_match(rows[:, :40], rows, **kw))
    ev = dev_rows[::2, :40]
    assert ev.stride(0) == 128
    assert np.array_equal(ops.plank_match(ev, ev, [(0, 3), (3, 1)], **kw).cpu().numpy(),
                          R.plank_match(rows[::2, :40], rows[::2, :40], [(0, 3), (3, 1)], **kw))
    # pairs outside the rows never reach the kernel
    for bad in ([(0, 7)], [(-1, 0)], torch.tensor([(7, 0)]).cuda()):
        with pytest.raises(IndexError):
            ops.plank_match(dev_rows, dev_rows, bad, **kw)
    assert ops.plank_match(dev_rows[:0], dev_rows[:0], **kw).shape == (0, 4)
    assert ops.plank_match(dev_rows, dev_rows, [], **kw).shape == (0, 4)


def test_error_statuses_come_back_without_a_launch():
    from plankassembly_amd import _lib as L
    from plankassembly_amd import ops
    rows = torch.full((2, 1027), 513, dtype=torch.int64, device="cuda")
    out = torch.full((2, 4), -7, dtype=torch.int32, device="cuda")

    def call(len_a=64, len_b=64, dof=6, threshold=0.5, pa=None, pb=None, a=rows):
        return L.lib().pa_plank_match(L.ptr(a), C.c_int64(1027), len_a, L.ptr(rows), C.c_int64(1027), len_b, L.ptr(pa), L.ptr(pb), 2,
                                      R.END, dof, 1, 0, threshold, L.ptr(out), L.stream())

    one = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert call(len_a=1027) == -3 and call(len_b=1027) == -3 and call(dof=5) == -3            # PA_ESHAPE
    assert call(threshold=0.0) == -1 and call(threshold=float("nan")) == -1 and call(pa=one) == -1 and call(a=None) == -1
    torch.cuda.synchronize()
    assert bool((out == -7).all())                          # nothing was launched
    assert call(len_a=1026, len_b=1026) == 0                # the limit itself runs: 170 PAD planks a side, all zero extent
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[0, 0, 170, 0]] * 2
    with pytest.raises(L.PlankHipError):
        ops.plank_match(rows, rows, end_token=R.END, filter_a=True, filter_b=False, threshold=0.5)       # len 1027
    with pytest.raises(L.PlankHipError):
        ops.plank_match(rows[:, :64], rows[:, :64], end_token=R.END, filter_a=True, filter_b=False, threshold=0.0)


def test_the_launch_captures_into_a_graph():
    from plankassembly_amd import ops
    rng = np.random.default_rng(33)
    pairs = [R.random_pair(rng, 8) for _ in range(16)]
    a = torch.from_numpy(R.rows_of([p for p, _ in pairs], 64)).cuda()
    b = torch.from_numpy(R.rows_of([g for _, g in pairs], 64)).cuda()
    kw = dict(end_token=R.END, filter_a=True, filter_b=False, threshold=0.5)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.plank_match(a, b, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.plank_match(a, b, **kw)
    a.copy_(torch.flip(a, [0]))                            # new tokens, same buffers: the replay must see them
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), R.plank_match(a.cpu().numpy(), b.cpu().numpy()))
