"""Float64 numpy restatement of pa_adam_step_ext's per-element rule (include/plank_hip.h) and of optim.lr_factor, for
tests/test_adam_ext_cpu.py, tests/test_adam_ext_gpu.py and tests/test_fused_adam_ext_gpu.py.  No import from the package: what is
written here is the documented rule, not the code under test."""
import math

import numpy as np


def f32(x):
    return float(np.float32(x))


def ema_d(ema_decay, t, warmup):
    """d_t of Adam step count t: the f32 ``ema_decay`` argument as a double, or min(that, (1 + t) / (10 + t)) with warmup."""
    d = f32(ema_decay)
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def decay_factor(lr, weight_decay):
    """f = (float)(1.0 - (double)lr * weight_decay) of the f32 arguments."""
    return f32(1.0 - f32(lr) * f32(weight_decay))


def unpack_bits(bits, n):
    """uint8 bitmask (bit i & 7 of byte i >> 3) -> bool [n]."""
    return np.unpackbits(np.asarray(bits, dtype=np.uint8), bitorder="little")[:n].astype(bool)


def pack_bits(mask):
    return np.packbits(np.asarray(mask, dtype=np.uint8), bitorder="little")


def adam_ext_step(p, g, m, v, t, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0, coef=1.0, clip_value=0.0,
                  weight_decay=0.0, decay_mask=None):
    """One applied step in float64 -> (p, m, v).  ``decay_mask``: bool [n] or None (every element decays); ``t`` >= 1 is the
    Adam step count of this step.  b1 / b2 / eps / gscale / lr enter as the f32 values the C ABI receives."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2, eps, gscale = f32(b1), f32(b2), f32(eps), f32(gscale)
    gj = g * gscale * coef
    if clip_value > 0:
        gj = np.clip(gj, -f32(clip_value), f32(clip_value))
    m = b1 * m + (1.0 - b1) * gj
    v = b2 * v + (1.0 - b2) * gj * gj
    if weight_decay > 0:
        f = decay_factor(lr, weight_decay)
        p = np.where(np.ones(p.shape, bool) if decay_mask is None else decay_mask, p * f, p)
    step_size = f32(lr) / (1.0 - b1 ** t)
    inv_sqrt_bc2 = 1.0 / math.sqrt(1.0 - b2 ** t)
    p = p - step_size * m / (np.sqrt(v) * inv_sqrt_bc2 + eps)
    return p, m, v


def ema_step(e, p_new, ema_decay, t, warmup=False):
    """e + (1 - d_t) * (p_new - e) in float64."""
    e, p_new = np.asarray(e, dtype=np.float64), np.asarray(p_new, dtype=np.float64)
    return e + (1.0 - ema_d(ema_decay, t, warmup)) * (p_new - e)


def lr_factor(kind, step, warmup_steps=0, total_steps=0, min_ratio=0.0):
    if kind == "constant":
        return 1.0
    if step < warmup_steps:
        return (step + 1) / warmup_steps
    if kind == "warmup":
        return 1.0
    if kind == "inverse_sqrt":
        return math.sqrt(warmup_steps / (step + 1))
    assert kind == "cosine"
    progress = min(1.0, (step - warmup_steps) / (total_steps - warmup_steps))
    return min_ratio + (1.0 - min_ratio) * 0.5 * (1.0 + math.cos(math.pi * progress))
