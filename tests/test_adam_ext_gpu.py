"""pa_adam_step_ext at kernel level (include/plank_hip.h, through `ops`): the off switches against the two
existing Adam entries, decoupled decay against torch.optim.AdamW on the CPU, the decay bitmask at every alignment edge, the EMA
against a float64 restatement (tests/adam_ext_reference.py), the skip semantics and the argument checks.  GPU only (`-m gpu`)."""
import numpy as np
import pytest
import torch

import adam_ext_reference as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from plankassembly_amd import ops
    from plankassembly_amd import _lib as L

DEV = "cuda"
N_TAIL, N_ONE, N_TWO = 3, 100_003, 2 * 2048 * 256 * 4 + 5      # tail only / tail + one sweep / two grid-stride sweeps + tail
EPS24 = 2.0 ** -24


def rnd(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * scale


def bits(t):
    return t.detach().view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[t.dtype])


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def f64(t):
    return t.detach().cpu().double().numpy()


class State:
    """p, m, v, the bf16 shadow and (optionally) an EMA on the device, from one drawn p."""

    def __init__(self, p0, ema=False):
        n = p0.numel()
        self.p, self.m, self.v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        self.pb = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        self.ema = p0.to(DEV) if ema else None

    def all(self):
        return [t for t in (self.p, self.m, self.v, self.pb, self.ema) if t is not None]

    def snapshot(self):
        return [t.clone() for t in self.all()]

    def ext(self, g, **kw):
        ops.adam_step_ext(self.p, g, self.m, self.v, p_bf16=self.pb, ema=self.ema, **kw)


def assert_same_bits(state, before):
    for t, b in zip(state.all(), before):
        assert torch.equal(bits(t), bits(b))


# ------------------------------------------------------------------------------------------------ off switches
@pytest.mark.parametrize("n", [N_TAIL, N_ONE, N_TWO])
def test_everything_off_under_the_guard_is_the_guarded_step(n):
    """weight_decay 0, no EMA, ctl given: p, m, v and the shadow equal pa_adam_step_guarded's bit for bit, over two steps with
    an active clip coefficient (max_norm below the norm) and a value clamp."""
    a, b = State(rnd(n, 300, 0.25)), State(rnd(n, 300, 0.25))
    ws = ops.grad_guard_ws(DEV)
    for k in (1, 2):
        g = rnd(n, 300 + k, 1e-3).to(DEV)
        ops.grad_guard(g, ws, max_norm=1e-3, skip_nonfinite=True, lr=1e-4)          # both kernels only read the control block
        ops.adam_step_guarded(a.p, g, a.m, a.v, ws, clip_value=5e-4, p_bf16=a.pb)
        b.ext(g, ws=ws, clip_value=5e-4, lr=1e-4)
    ctl = ops.grad_guard_ctl(ws)
    assert ctl["applied"] == 2 and (ctl["coef"] < 1.0 or n == N_TAIL)
    assert a.m.abs().max() > 0
    assert_same_bits(b, a.all())


@pytest.mark.parametrize("n", [N_TAIL, N_ONE, N_TWO])
def test_everything_off_without_the_guard_against_the_plain_step(n):
    """ctl NULL: m and v equal pa_adam_step's bit for bit; p is within one f32 ulp of it, and the shadow is the bf16 of the
    kernel's own p, so it equals pa_adam_step's wherever p does.

    pa_adam_step and pa_adam_step_ext launch the same kernel instantiation (adam_ext_kernel<0, false>), so this now holds the
    two entries' host set-up together and observes 0 differing elements.  It was written when pa_adam_step had a kernel of its
    own in plain C++ expressions, whose fused multiply-adds the compiler chose (observed then on MI355X, three steps: 0 elements
    of p differing at n = 3, 100 003 and 4 194 309); that pa_adam_step still gives that kernel's bits is held by
    tests/test_rowops_family_bits_gpu.py."""
    a, b = State(rnd(n, 310, 0.25)), State(rnd(n, 310, 0.25))
    for step in (1, 2, 3):
        g = rnd(n, 310 + step, 1e-3).to(DEV)
        before = a.p.clone()
        ops.adam_step(a.p, g, a.m, a.v, step, lr=1e-4, p_bf16=a.pb)
        with torch.no_grad():
            b.p.copy_(before)                                   # (per-step comparison: both start the step from the same p)
        b.ext(g, step=step, lr=1e-4)
        assert torch.equal(bits(a.m), bits(b.m)) and torch.equal(bits(a.v), bits(b.v))
        pa, pe = a.p.cpu().numpy(), b.p.cpu().numpy()
        differ = pa != pe
        print(f"n {n} step {step}: {int(differ.sum())} of {n} elements of p differ from pa_adam_step, "
              f"max |dp| {float(np.abs(pa - pe).max()):.3e}")
        assert (np.abs(pa.astype(np.float64) - pe) <= np.spacing(np.maximum(np.abs(pa), np.abs(pe)))).all()
        assert torch.equal(bits(b.pb), bits(b.p.to(torch.bfloat16)))
        same = torch.from_numpy(~differ).to(DEV)
        assert torch.equal(bits(a.pb)[same], bits(b.pb)[same])


# ------------------------------------------------------------------------------------------------ AdamW parity
@pytest.mark.parametrize("guarded", [False, True])
def test_three_steps_match_torch_adamw(guarded):
    """Reference: f32 torch.optim.AdamW(lr 1e-4, weight_decay 0.1) on the CPU, every element decaying (decay_bits NULL).
    Bounds: those of test_four_steps_unclipped_clipped_skipped_clipped_match_torch (p 2e-7, m 2e-5 rel, v 1.2e-4 rel); p gets
    half an f32 ulp of max|p| per step on top for the one extra rounding (the decayed p), computed from the drawn p."""
    n, lr, wd = N_ONE, 1e-4, 0.1
    p0 = rnd(n, 320, 0.25)
    grads = [rnd(n, 321 + k, 1e-3) for k in range(3)]
    ref = torch.nn.Parameter(p0.clone())
    topt = torch.optim.AdamW([ref], lr=lr, weight_decay=wd)
    for g in grads:
        ref.grad = g.clone()
        topt.step()
    st = topt.state[ref]
    s = State(p0)
    ws = ops.grad_guard_ws(DEV) if guarded else None
    for k, g in enumerate(grads):
        gd = g.to(DEV)
        if guarded:
            ops.grad_guard(gd, ws, max_norm=1e30, skip_nonfinite=True, lr=lr)
        s.ext(gd, step=k + 1, ws=ws, lr=lr, weight_decay=wd)
    half_ulp = 0.5 * float(np.spacing(np.float32(p0.abs().max())))
    bound = 2e-7 + 3 * half_ulp
    dp = float((s.p.cpu() - ref.detach()).abs().max())
    dm, dv = rel_err(s.m, st["exp_avg"]), rel_err(s.v, st["exp_avg_sq"])
    moved = float((ref.detach() - p0).abs().max())
    print(f"AdamW guarded={guarded}: |dp| {dp:.3e} (bound {bound:.3e}, half ulp {half_ulp:.3e})  m rel {dm:.3e}  v rel {dv:.3e}")
    assert moved > 100 * bound                                   # (decay + three updates are far above what is being bounded)
    assert dp <= bound
    assert dm <= 2e-5
    assert dv <= 1.2e-4
    assert torch.equal(bits(s.pb), bits(s.p.to(torch.bfloat16)))


# ------------------------------------------------------------------------------------------------ mask edges
def test_decay_mask_edges_and_null_mask():
    """n = 100 003, lr 0.1, weight_decay 0.5 (f = 0.95), |p| >= 0.25: an element decayed or spared by mistake is off by at least
    0.05 * 0.25 = 1.25e-2.  Decayed ranges start and end off every alignment (nibble, byte, f32x4, the tail).  Every element
    against the float64 restatement; tolerance per element 2^-24 * (2 |p| + 10 lr): the decayed product and the final
    difference round once each (<= 2^-24 |p| and 2^-24 (|p| + lr)), and the update term of size <= lr carries about eight
    roundings (g scale, m, v, sqrt, denominator, step_size, product, quotient)."""
    n, lr, wd = N_ONE, 0.1, 0.5
    g0 = torch.Generator().manual_seed(330)
    p0 = (0.25 + torch.rand(n, generator=g0)) * torch.where(torch.rand(n, generator=g0) < 0.5, -1.0, 1.0)
    g = rnd(n, 331, 1e-3)
    mask = np.zeros(n, dtype=bool)
    for lo, hi in ((0, 5), (9, 10), (4093, 8191), (n - 3, n)):
        mask[lo:hi] = True
    assert n - 3 == (n >> 2) << 2                                               # the last range IS the n % 4 tail
    packed = torch.from_numpy(R.pack_bits(mask)).to(DEV)
    assert packed.numel() == (n + 7) // 8
    s = State(p0)
    s.ext(g.to(DEV), step=1, lr=lr, weight_decay=wd, decay_bits=packed)
    want, _, _ = R.adam_ext_step(f64(p0), f64(g), np.zeros(n), np.zeros(n), 1, lr=lr, weight_decay=wd, decay_mask=mask)
    wrong, _, _ = R.adam_ext_step(f64(p0), f64(g), np.zeros(n), np.zeros(n), 1, lr=lr, weight_decay=wd, decay_mask=~mask)
    assert np.abs(want - wrong).min() > 1e-2
    err = np.abs(f64(s.p) - want)
    tol = EPS24 * (2 * np.abs(want) + 10 * lr)
    print(f"mask edges: max err {err.max():.3e}, max err / tol {(err / tol).max():.3f}")
    assert (err <= tol).all(), np.nonzero(err > tol)[0][:10]
    assert torch.equal(bits(s.pb), bits(s.p.to(torch.bfloat16)))
    # ---- decay_bits NULL against the all-ones mask: the same bits
    ones = torch.full(((n + 7) // 8,), 255, dtype=torch.uint8, device=DEV)
    a, b = State(p0), State(p0)
    a.ext(g.to(DEV), step=1, lr=lr, weight_decay=wd, decay_bits=ones)
    b.ext(g.to(DEV), step=1, lr=lr, weight_decay=wd, decay_bits=None)
    assert_same_bits(b, a.all())
    all_ref, _, _ = R.adam_ext_step(f64(p0), f64(g), np.zeros(n), np.zeros(n), 1, lr=lr, weight_decay=wd)
    assert (np.abs(f64(b.p) - all_ref) <= EPS24 * (2 * np.abs(all_ref) + 10 * lr)).all()
    # ---- weight_decay 0 with a mask present does not touch p beyond Adam's own update
    c, d = State(p0), State(p0)
    c.ext(g.to(DEV), step=1, lr=lr, weight_decay=0.0, decay_bits=ones)
    d.ext(g.to(DEV), step=1, lr=lr)
    assert_same_bits(c, d.all())


# ------------------------------------------------------------------------------------------------ EMA
def ema_bound(p, e):
    return 4 * EPS24 * (np.abs(p) + np.abs(e))


def test_ema_warmup_decay_hand_values():
    assert [R.ema_d(0.9, t, True) for t in (1, 2, 3)] == [2 / 11, 3 / 12, 4 / 13]
    assert abs(2 / 11 - 0.1818) < 1e-4 and 3 / 12 == 0.25 and abs(4 / 13 - 0.3077) < 1e-4
    assert R.ema_d(0.9, 100, True) == R.ema_d(0.9, 1, False) == float(np.float32(0.9))


@pytest.mark.parametrize("n,warmup", [(N_TAIL, False), (N_ONE, False), (N_TWO, False), (N_ONE, True)])
def test_ema_follows_the_weights(n, warmup):
    """Three steps, ema_decay 0.9 (with warmup: d_t = 2/11, 1/4, 4/13).  Per element and per step against
    e + (1 - d_t) (p_new - e) in float64, fed the device's own p_new and its own e of the step before.

    Bound 4 * 2^-24 * (|p| + |e|) from the spelled form e' = fma(w, p - e, e), w = (float)(1 - d_t): the difference s = p - e
    rounds once, <= 2^-24 (|p| + |e|) / 2 and enters scaled by w <= 1; w itself is off by <= 2^-24 w relative, <= 2^-24 |s| in
    the product; the fma rounds once more, <= 2^-24 |e'| / 2 <= 2^-24 (|p| + |e|) / 2.  Sum <= 2 * 2^-24 (|p| + |e|); twice that
    is asserted.  The unguarded path (1 - d_t from the host) and the guarded one (every thread derives it from ctl->applied)
    are held to the same reference, and to each other within the same bound."""
    lr, d = 1e-2, 0.9
    p0 = rnd(n, 340, 0.25)
    host, dev = State(p0, ema=True), State(p0, ema=True)
    ws = ops.grad_guard_ws(DEV)
    for t in (1, 2, 3):
        g = rnd(n, 340 + t, 1e-3).to(DEV)
        e_host, e_dev = f64(host.ema), f64(dev.ema)
        host.ext(g, step=t, lr=lr, ema_decay=d, ema_warmup=warmup)
        ops.grad_guard(g, ws, max_norm=1e30, skip_nonfinite=True, lr=lr)
        dev.ext(g, ws=ws, lr=lr, ema_decay=d, ema_warmup=warmup)
        for name, s, e_before in (("host", host, e_host), ("guarded", dev, e_dev)):
            want = R.ema_step(e_before, f64(s.p), d, t, warmup)
            err = np.abs(f64(s.ema) - want)
            bound = ema_bound(f64(s.p), e_before)
            print(f"n {n} warmup {warmup} step {t} {name}: d_t {R.ema_d(d, t, warmup):.6f} max err / bound {(err / bound).max():.3f}")
            assert (err <= bound).all()
            assert np.abs(f64(s.ema) - e_before).max() > 100 * bound.max()         # (the EMA moved by far more than the bound)
        assert (np.abs(f64(host.ema) - f64(dev.ema)) <= ema_bound(f64(host.p), f64(host.ema))).all()
    assert ops.grad_guard_ctl(ws)["applied"] == 3
    assert torch.equal(bits(host.pb), bits(host.p.to(torch.bfloat16)))


def test_ema_with_decay_and_mask_in_one_pass():
    """Both features and the guard together (the configuration the trainer runs): p against the float64 rule, the EMA against the
    device's own p."""
    n, lr, wd, d = N_ONE, 1e-2, 0.1, 0.9
    p0 = rnd(n, 350, 0.25)
    g = rnd(n, 351, 1e-3)
    mask = np.arange(n) % 3 != 0
    s = State(p0, ema=True)
    ws = ops.grad_guard_ws(DEV)
    ops.grad_guard(g.to(DEV), ws, max_norm=1e30, lr=lr)
    s.ext(g.to(DEV), ws=ws, lr=lr, weight_decay=wd, decay_bits=torch.from_numpy(R.pack_bits(mask)).to(DEV), ema_decay=d)
    want, _, _ = R.adam_ext_step(f64(p0), f64(g), np.zeros(n), np.zeros(n), 1, lr=lr, weight_decay=wd, decay_mask=mask)
    assert (np.abs(f64(s.p) - want) <= EPS24 * (2 * np.abs(want) + 10 * lr)).all()
    e_want = R.ema_step(f64(p0), f64(s.p), d, 1)
    assert (np.abs(f64(s.ema) - e_want) <= ema_bound(f64(s.p), f64(p0))).all()


# ------------------------------------------------------------------------------------------------ skip
def test_a_skipped_step_keeps_every_bit_and_the_ema_step_count():
    """Guarded, skip_nonfinite, ema_warmup: step 1 clean, step 2 with one NaN in g, step 3 clean.  The skipped step changes no
    bit of p, m, v, the shadow or the EMA and leaves `applied` at 1; the clean step after it is Adam step 2, so its d_t is
    3/12 - not 4/13, which the same data tells apart by far more than the bound."""
    n, lr, wd, d = N_ONE, 1e-2, 0.1, 0.9
    s = State(rnd(n, 360, 0.25), ema=True)
    ws = ops.grad_guard_ws(DEV)
    kw = dict(ws=ws, lr=lr, weight_decay=wd, ema_decay=d, ema_warmup=True)

    def step(g):
        ops.grad_guard(g, ws, max_norm=1.0, skip_nonfinite=True, lr=lr)
        s.ext(g, **kw)
        return ops.grad_guard_ctl(ws)

    assert step(rnd(n, 361, 1e-3).to(DEV))["applied"] == 1
    before = s.snapshot()
    bad = rnd(n, 362, 1e-3)
    bad[n // 3] = float("nan")
    ctl = step(bad.to(DEV))
    assert ctl["apply"] == 0 and ctl["applied"] == 1 and ctl["skipped"] == 1
    assert_same_bits(s, before)
    e_before = f64(s.ema)
    ctl = step(rnd(n, 363, 1e-3).to(DEV))
    assert ctl["apply"] == 1 and ctl["applied"] == 2
    bound = ema_bound(f64(s.p), e_before)
    assert (np.abs(f64(s.ema) - R.ema_step(e_before, f64(s.p), d, 2, True)) <= bound).all()
    assert (np.abs(f64(s.ema) - R.ema_step(e_before, f64(s.p), d, 3, True)) > bound).mean() > 0.9
    assert torch.isfinite(s.p).all() and torch.isfinite(s.ema).all()


# ------------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_return_an_error_and_launch_nothing():
    n = 1024
    g = torch.ones(n, device=DEV)
    s = State(torch.zeros(n))
    ema_buf = torch.full((n + 4,), 7.0, device=DEV)
    ema = ema_buf[:n]
    call = lambda **kw: ops.adam_step_ext(s.p, g, s.m, s.v, p_bf16=s.pb, **{"step": 1, "ema": ema, "ema_decay": 0.9, **kw})
    with pytest.raises(L.PlankHipError, match="PA_EALIGN"):
        call(ema=ema_buf[1:n + 1])                                           # 4 bytes off a 16-byte boundary
    with pytest.raises(L.PlankHipError, match="PA_EINVAL"):
        call(ema_decay=1.0)
    with pytest.raises(L.PlankHipError, match="PA_EINVAL"):
        call(ema_decay=float("nan"))
    with pytest.raises(L.PlankHipError, match="PA_EINVAL"):
        call(weight_decay=-0.1)
    with pytest.raises(L.PlankHipError, match="PA_EINVAL"):
        call(weight_decay=float("nan"))
    with pytest.raises(L.PlankHipError, match="PA_EINVAL"):
        call(step=0)                                                         # no ctl: the step count must be given
    with pytest.raises(L.PlankHipError, match="PA_EINVAL"):
        ops.adam_step_ext(s.p[:0], g[:0], s.m[:0], s.v[:0], step=1)
    with pytest.raises(L.PlankHipError, match="PA_EALIGN"):
        ops.adam_step_ext(s.p, ema_buf[1:n + 1], s.m, s.v, step=1)           # misaligned g
    torch.cuda.synchronize()
    assert not s.p.any() and not s.m.any() and not s.v.any() and not s.pb.any() and bool((ema_buf == 7.0).all())
    assert int(L.lib().pa_adam_ext_args_bytes()) == 112
