"""The gradient guard at kernel level (include/plank_hip.h pa_grad_guard / pa_adam_step_guarded, through `ops`): the global
norm against float64, non-finite detection, clipping + skipping against torch's clip_grad_norm_ + torch.optim.Adam on the CPU,
value clipping, the guard-on-but-inactive path against pa_adam_step, and the argument checks.  GPU only (`-m gpu`)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from plankassembly_amd import ops
    from plankassembly_amd import _lib as L

DEV = "cuda"
N_TAIL, N_ONE, N_TWO = 3, 100_003, 2 * 2048 * 256 * 4 + 5      # tail only / tail + one sweep / two grid-stride sweeps + tail


def rnd(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * scale


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


_BIG = {}


def big_gradient():
    """One 4 194 309-element gradient (CPU and device copy) shared by the tests that need two sweeps; never modified."""
    if not _BIG:
        g = rnd(N_TWO, seed=170, scale=1e-2)
        _BIG["cpu"], _BIG["dev"] = g, g.to(DEV)
    return _BIG["cpu"], _BIG["dev"]


def guard_once(g, **kw):
    ws = ops.grad_guard_ws(g.device)
    ops.grad_guard(g, ws, **kw)
    return ops.grad_guard_ctl(ws)


@pytest.mark.parametrize("n", [N_TAIL, N_ONE, N_TWO])
def test_norm_matches_float64_and_is_reproducible(n):
    """Relative error <= 1e-5: the f32 work is a per-thread chain of k <= 12 adds at these sizes, a 6-step wave butterfly and
    a short tree over four waves, all of non-negative terms: <= (k + 16) * 2^-24 ~ 1.7e-6; the block partials are added in
    double.  No atomics, so a second call gives the same bits, and a power-of-two gscale scales the norm exactly."""
    if n == N_TWO:
        cpu, g = big_gradient()
    else:
        cpu = rnd(n, seed=160 + n % 7, scale=1e-2)
        g = cpu.to(DEV)
    ref = float(cpu.double().norm())
    a = guard_once(g)
    b = guard_once(g)
    print(f"n {n}: norm {a['norm']!r} float64 {ref!r} rel {abs(a['norm'] - ref) / ref:.3e}")
    assert abs(a["norm"] - ref) <= 1e-5 * ref
    assert a["norm"] == b["norm"]                                           # (floats read from the same 4 bytes: bit equality)
    assert a["coef"] == 1.0 and a["apply"] == 1 and a["applied"] == 1 and a["attempts"] == 1 and a["skipped"] == 0
    eighth = guard_once(g, gscale=0.125)
    assert eighth["norm"] == a["norm"] / 8


@pytest.mark.parametrize("where,value", [("tail", float("nan")), ("first", float("inf")), ("second_sweep", float("-inf"))])
def test_nonfinite_entries_are_seen_wherever_they_sit(where, value):
    _, clean = big_gradient()
    g = clean.clone()
    idx = {"tail": N_TWO - 1, "first": 0, "second_sweep": 2048 * 256 * 4 + 902_849}[where]
    assert (idx >= (N_TWO & ~3)) == (where == "tail") and (idx >= 2048 * 256 * 4) == (where != "first")
    g[idx] = value
    skip = guard_once(g, skip_nonfinite=True, max_norm=1.0)
    assert skip["apply"] == 0 and skip["applied"] == 0 and skip["skipped"] == 1 and skip["first_skipped_attempt"] == 1
    assert not math.isfinite(skip["norm"])
    keep = guard_once(g, skip_nonfinite=False, max_norm=1.0)
    assert keep["apply"] == 1 and keep["applied"] == 1 and keep["skipped"] == 0 and keep["first_skipped_attempt"] == -1
    assert not math.isfinite(keep["norm"])


def test_four_steps_unclipped_clipped_skipped_clipped_match_torch():
    """Reference: f32 torch on the CPU, clip_grad_norm_(max_norm 0.5) + torch.optim.Adam(lr 1e-4), step 3 (one NaN) not stepped.
    |g| ~ 0.316 * scale: scale 1 is below the threshold (coef exactly 1), 4 and 3 are above it.

    Bounds: those of test_adam_vs_oracle (p 2e-7 over its three steps, m 1e-5, v 1e-4) plus the norm's 1e-5, which enters m
    once and v twice through coef.  p is drawn at scale 0.25 - the size of trained weights - because the absolute 2e-7 is below
    ONE f32 ulp from |p| = 2 on (2.4e-7): there two correctly rounded implementations of the same step can differ by more than
    the bound through the last bit of p alone, and the test would measure the draw, not the kernel."""
    n, lr, max_norm = N_ONE, 1e-4, 0.5
    p0 = rnd(n, seed=180, scale=0.25)
    base = rnd(n, seed=181, scale=1e-3)
    grads = [base * 1.0, rnd(n, seed=182, scale=1e-3) * 4.0, base * 2.0, rnd(n, seed=183, scale=1e-3) * 3.0]
    grads[2][n // 3] = float("nan")
    # ---- reference
    ref = torch.nn.Parameter(p0.clone())
    topt = torch.optim.Adam([ref], lr=lr)
    coefs = []
    for k, g in enumerate(grads):
        if k == 2:
            continue
        ref.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([ref], max_norm)
        coefs.append(min(1.0, max_norm / (float(total) + 1e-6)))
        topt.step()
    assert coefs[0] == 1.0 and coefs[1] < 0.5 and coefs[2] < 0.6
    st = topt.state[ref]
    # ---- device
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pb = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    ws = ops.grad_guard_ws(DEV)
    seen = []
    for k, g in enumerate(grads):
        gd = g.to(DEV)
        before = [t.clone() for t in (p, m, v, pb)] if k == 2 else None
        ops.grad_guard(gd, ws, max_norm=max_norm, skip_nonfinite=True, lr=lr)
        ops.adam_step_guarded(p, gd, m, v, ws, p_bf16=pb)
        seen.append(ops.grad_guard_ctl(ws))
        if k == 2:
            for t, b in zip((p, m, v, pb), before):                          # the skipped step kept every bit
                assert torch.equal(t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32),
                                   b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))
    assert [c["apply"] for c in seen] == [1, 1, 0, 1]
    assert seen[0]["coef"] == 1.0
    assert abs(seen[1]["coef"] - coefs[1]) <= 1e-5 * coefs[1] and abs(seen[3]["coef"] - coefs[2]) <= 1e-5 * coefs[2]
    last = seen[-1]
    assert (last["applied"], last["skipped"], last["attempts"], last["first_skipped_attempt"]) == (3, 1, 4, 3)
    dp = float((p.cpu() - ref.detach()).abs().max())
    dm, dv = rel_err(m, st["exp_avg"]), rel_err(v, st["exp_avg_sq"])
    print(f"four steps: |dp| {dp:.3e}  m rel {dm:.3e}  v rel {dv:.3e}")
    assert dp <= 2e-7
    assert dm <= 2e-5
    assert dv <= 1.2e-4
    assert torch.equal(pb.cpu().view(torch.int16), p.cpu().to(torch.bfloat16).view(torch.int16))


def test_clip_value_clamps_the_gradient_adam_sees():
    n, c, b1 = N_ONE, 5e-4, 0.9
    g = rnd(n, seed=190, scale=1e-3)
    assert float((g.abs() > c).float().mean()) > 0.3
    p, m, v = rnd(n, seed=191, scale=0.25).to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ws = ops.grad_guard_ws(DEV)
    ops.grad_guard(g.to(DEV), ws)
    ops.adam_step_guarded(p, g.to(DEV), m, v, ws, clip_value=c)
    want = (1 - b1) * g.clamp(-c, c)
    print("clip_value: m rel", rel_err(m, want))
    assert rel_err(m, want) <= 1e-6
    ctl = ops.grad_guard_ctl(ws)
    assert ctl["coef"] == 1.0 and ctl["applied"] == 1


def test_guard_on_but_inactive_equals_the_plain_step():
    """max_norm 1e30, finite gradients: coef is exactly 1, so the two paths can differ only by one ulp of step_size and of
    inv_sqrt_bc2 (device pow against host pow) on an update of at most lr = 1e-4 per step: 2 * 6e-8 * 1e-4 per step, ~4e-11
    over three steps; bound 3e-10."""
    n, lr = N_ONE, 1e-4
    p0 = rnd(n, seed=200, scale=0.25)
    pa, ma, va = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pg, mg, vg = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ws = ops.grad_guard_ws(DEV)
    for step in (1, 2, 3):
        g = rnd(n, seed=200 + step, scale=1e-3).to(DEV)
        ops.adam_step(pa, g, ma, va, step, lr=lr)
        ops.grad_guard(g, ws, max_norm=1e30, skip_nonfinite=True, lr=lr)
        ops.adam_step_guarded(pg, g, mg, vg, ws)
    ctl = ops.grad_guard_ctl(ws)
    assert ctl["coef"] == 1.0 and ctl["applied"] == 3 and ctl["skipped"] == 0
    dp = float((pa - pg).abs().max())
    print(f"guard on, inactive: |dp| {dp:.3e}  step_size {ctl['step_size']!r} inv_sqrt_bc2 {ctl['inv_sqrt_bc2']!r}")
    assert dp <= 3e-10
    assert torch.equal(ma, mg) and torch.equal(va, vg)                       # (the moments do not see the step size at all)


def test_bad_arguments_return_an_error_and_launch_nothing():
    n = 1024
    g = torch.ones(n + 4, device=DEV)
    p, m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ws = ops.grad_guard_ws(DEV)
    with pytest.raises(L.PlankHipError, match="PA_EALIGN"):
        ops.grad_guard(g[1:n + 1], ws)                                       # 4 bytes off a 16-byte boundary
    with pytest.raises(L.PlankHipError, match="PA_EINVAL"):
        ops.grad_guard(g[:0], ws)                                            # n = 0
    with pytest.raises(L.PlankHipError, match="PA_EINVAL"):
        ops.grad_guard(g[:n], ws[:L.GRAD_GUARD_WS_BYTES - 16])               # workspace too small
    with pytest.raises(L.PlankHipError, match="PA_EINVAL"):
        ops.grad_guard(g[:n], ws, max_norm=-1.0)
    with pytest.raises(L.PlankHipError, match="PA_EALIGN"):
        ops.adam_step_guarded(p, g[1:n + 1], m, v, ws)
    with pytest.raises(L.PlankHipError, match="PA_EINVAL"):
        ops.adam_step_guarded(p[:0], g[:0], m[:0], v[:0], ws)
    with pytest.raises(L.PlankHipError, match="PA_EINVAL"):
        L.check(L.lib().pa_grad_guard_init(L.ptr(ws), ws.numel(), -1, L.stream()), "pa_grad_guard_init")
    ctl = ops.grad_guard_ctl(ws)
    assert ctl["attempts"] == 0 and ctl["applied"] == 0                      # no finish kernel ever ran
    assert not p.any() and not m.any() and not v.any()                       # nor an Adam kernel
    assert int(L.lib().pa_grad_guard_ws_bytes()) == L.GRAD_GUARD_WS_BYTES == ws.numel()
