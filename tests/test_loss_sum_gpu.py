"""The training loss is summed in an order-free way (csrc/rowops.hip mixture_nll_fwd_kernel<true, false>, pa_mixture_nll_fwd_fin): the
blocks' NLL sums meet in a 64-bit fixed-point word, so the loss has the same bits whatever order the blocks arrive in - which
tests/test_device_data_gpu.py::test_train_step_equals_the_cpu_collated_batch relies on (a float atomic made it differ by 3 ulp)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
B, T, V, LDV, PAD = 6, 100, 514, 520, 513           # 600 rows: 150 blocks of 4 rows; T % 4 == 0, so a block never spans two members


def _inputs():
    g = torch.Generator().manual_seed(5)
    vocab = torch.randn(B, T, LDV, generator=g) * 3
    ptr = torch.randn(B, T, T, generator=g) * 2
    sw = torch.randn(B * T, generator=g)
    label = torch.randint(0, V + T, (B, T), generator=g)
    label[torch.rand(B, T, generator=g) < 0.3] = PAD
    label[:, 90:] = PAD                              # whole blocks that add nothing
    return vocab, ptr, sw, label


def _run(vocab, ptr, sw, label):
    from plankassembly_amd import _lib as L
    dev = [x.cuda().contiguous() for x in (vocab, ptr, sw, label)]
    stats = torch.full((8,), 7.0, device="cuda")     # the launch zeroes the block itself
    lse = torch.empty(B * T, 2, device="cuda")
    L.check(L.lib().pa_mixture_nll_fwd_fin(L.ptr(stats), L.ptr(lse), L.ptr(dev[0]), LDV, L.ptr(dev[1]), L.ptr(dev[2]), L.ptr(dev[3]),
                                           B, T, V, PAD, L.stream()), "pa_mixture_nll_fwd_fin")
    torch.cuda.synchronize()
    return stats.cpu()


def _reference(vocab, ptr, sw, label):
    """float64: (sum of -log p(label) over the non-PAD rows, their number, the largest magnitude a row's three terms have)."""
    v, p, s = vocab[..., :V].double(), ptr.double().clone(), sw.double().view(B, T)
    p[torch.triu(torch.ones(T, T, dtype=torch.bool))[None].expand(B, T, T)] = 1e-6
    lse_v, lse_p = torch.logsumexp(v, -1), torch.logsumexp(p, -1)
    prob = torch.sigmoid(s)
    lv, lp = torch.log(torch.clamp(1 - prob, min=1e-6)), torch.log(torch.clamp(prob, min=1e-6))
    both = torch.cat((v - lse_v[..., None] + lv[..., None], p - lse_p[..., None] + lp[..., None]), -1)
    valid = label != PAD
    logp = both.gather(-1, label[..., None])[..., 0][valid]
    big = max(float(v.abs().max()), float(p.abs().max()), float(lse_v.abs().max()), float(lse_p.abs().max()), -float(lv.min()), -float(lp.min()))
    return float(-logp.sum()), int(valid.sum()), big


def test_loss_bits_do_not_depend_on_the_order_of_the_blocks():
    x = _inputs()
    first = _run(*x)
    ref, n, big = _reference(*x)
    # a row's -log p is three f32 terms of magnitude <= big, each within a few ulp (expf / logf): 16 x 2^-24 big per row
    assert int(first[1]) == n and abs(float(first[0]) - ref) <= n * 2.0 ** -20 * big, (float(first[0]), ref)
    q = int(first[6:8].view(torch.int64)[0])
    assert first[0].item() == float(np.float32(q * 2.0 ** -30))
    assert abs(first[4].item() - first[0].item() / n) <= 2.0 ** -22 * first[0].item() / n       # one f32 division
    for _ in range(8):                                # run to run
        assert torch.equal(_run(*x).view(torch.int32), first.view(torch.int32))
    # the members in another order: every block keeps its four rows, and meets the others at another place in the sum
    perm = torch.tensor([3, 5, 0, 2, 4, 1])
    vocab, ptr, sw, label = x
    moved = _run(vocab[perm], ptr[perm], sw.view(B, T)[perm].reshape(-1), label[perm])
    assert torch.equal(moved.view(torch.int32), first.view(torch.int32)), (moved, first)


def test_a_loss_that_is_not_finite_stays_so():
    vocab, ptr, sw, label = _inputs()
    label[2, 7] = 11
    for bad in (float("nan"), float("-inf")):
        vocab[2, 7, 11] = bad
        assert not torch.isfinite(_run(vocab, ptr, sw, label)[4])
