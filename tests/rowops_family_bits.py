"""The Adam and mixture-NLL entries of csrc/rowops.hip run on the case tables of tests/rowops_parity.py, every input and output buffer
reduced to the sha256 of its bytes (TEST INFRASTRUCTURE; the runs need the GPU).

tools/record_rowops_bits.py writes these records, taken from a build of a chosen commit, to tests/golden/rowops_family_bits.json;
tests/test_rowops_family_bits_gpu.py runs them again and compares.  Inputs are generated on the CPU, seeded by case name; only entries
of include/plank_hip.h are called, through plankassembly_amd.ops / _lib, so the same file runs against any build that has them.

Not recorded: stats[0] of pa_mixture_nll_fwd (a float atomic sum: its last bits depend on the order the blocks arrive in)."""
import ctypes as C
import hashlib
import math

import torch

import loss_ext_reference as R
import rowops_parity as rp

HP = rp.ADAM_HP
MAX_NORM = 1e-3                                                     # below the norm of every step's gradient (n = 1 apart: its gradient is 0)
WEIGHT_DECAY, EMA_DECAY = 0.01, 0.999
ADAM_EXT = {  # configuration -> (weight decay on, bitmask, EMA with warmup)
    "off": (False, False, False), "decay_all": (True, False, False), "decay_mask": (True, True, False), "ema_warmup": (False, False, True),
    "decay_mask_ema": (True, True, True)}
_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(-1).view(_VIEW[t.element_size()]).numpy().tobytes()).hexdigest()


def _api():
    from plankassembly_amd import _lib as L, ops
    return L, ops


def clip_value(n):
    """Half the root mean square of a gradient of n elements scaled to MAX_NORM: about six elements in ten are clamped."""
    return 0.5 * MAX_NORM / math.sqrt(n)


def decay_bits(c):
    g = torch.Generator().manual_seed(rp.seed_of(c["name"], 55))
    return torch.randint(0, 256, ((c["n"] + 7) // 8,), generator=g, dtype=torch.int32).to(torch.uint8)


# ------------------------------------------------------------------------------------------------ Adam
def _adam_state(t, shadow, ema):
    d = {k: t[k].clone() for k in ("p", "m", "v")}
    d["pb"] = torch.zeros(t["p"].numel(), dtype=torch.bfloat16, device="cuda") if shadow else None
    d["ema"] = t["p"].clone() if ema else None
    return d


def _adam_out(d, ws=None):
    L, _ = _api()
    torch.cuda.synchronize()
    out = {k: sha(x) for k, x in d.items() if x is not None}
    if ws is not None:
        out["ctl"] = sha(ws[L.GRAD_GUARD_CTL_OFFSET:L.GRAD_GUARD_WS_BYTES])
    return out


def _adam_run(c, t, variant, shadow, bits):
    """One variant on fresh copies of the device tensors `t`: HP["steps"] steps (one for "skipped"), then the hashes of everything the steps may write."""
    _, ops = _api()
    kind, _, cfg = variant.partition(":")
    hp = dict(lr=HP["lr"], b1=HP["b1"], b2=HP["b2"])
    decay, mask, ema = ADAM_EXT[cfg] if cfg else (False, False, False)
    d = _adam_state(t, shadow, ema)
    ext = dict(weight_decay=WEIGHT_DECAY if decay else 0.0, decay_bits=bits if mask else None, ema=d["ema"], ema_decay=EMA_DECAY if ema else 0.0,
               ema_warmup=ema, p_bf16=d["pb"], eps=HP["eps"], gscale=HP["gscale"], **hp)
    guarded = kind in ("guarded", "ext_guarded", "skipped")
    ws = ops.grad_guard_ws("cuda") if guarded else None
    grads = t["g"]
    if kind == "skipped":
        bad = t["g"][0].clone()
        bad[bad.numel() // 2] = float("inf")
        grads = [bad]
    for k, g in enumerate(grads):
        if guarded:
            ops.grad_guard(g, ws, gscale=HP["gscale"], max_norm=MAX_NORM, skip_nonfinite=kind == "skipped", **hp)
        if kind == "plain":
            ops.adam_step(d["p"], g, d["m"], d["v"], k + 1, eps=HP["eps"], gscale=HP["gscale"], p_bf16=d["pb"], **hp)
        elif kind == "guarded" or (kind == "skipped" and not cfg):
            ops.adam_step_guarded(d["p"], g, d["m"], d["v"], ws, b1=HP["b1"], b2=HP["b2"], eps=HP["eps"], gscale=HP["gscale"],
                                  clip_value=clip_value(c["n"]), p_bf16=d["pb"])
        else:
            ops.adam_step_ext(d["p"], g, d["m"], d["v"], step=k + 1, ws=ws, clip_value=clip_value(c["n"]) if guarded else 0.0, **ext)
    return _adam_out(d, ws)


def adam_variants():
    return (["plain", "guarded"] + [f"ext:{k}" for k in ADAM_EXT] + [f"ext_guarded:{k}" for k in ADAM_EXT] + ["skipped", "skipped:decay_mask_ema"])


def adam_records():
    """[{name, inputs: {buffer: sha256}, outputs: {variant/shadow: {buffer: sha256}}}] over rowops_parity.adam_cases()."""
    recs = []
    for c in rp.adam_cases():
        t = rp.adam_inputs(c)
        bits = decay_bits(c)
        inputs = {k: sha(t[k]) for k in ("p", "m", "v")}
        inputs.update({f"g{k}": sha(g) for k, g in enumerate(t["g"])})
        inputs["decay_bits"] = sha(bits)
        dev = dict(p=t["p"].cuda(), m=t["m"].cuda(), v=t["v"].cuda(), g=[g.cuda() for g in t["g"]])
        dev_bits = bits.cuda()
        outputs = {f"{v}/{'shadow' if s else 'no_shadow'}": _adam_run(c, dev, v, s, dev_bits) for v in adam_variants() for s in (False, True)}
        recs.append(dict(name=c["name"], inputs=inputs, outputs=outputs))
    return recs


# ------------------------------------------------------------------------------------------------ mixture NLL
def nll_record(c):
    L, ops = _api()
    lib, st = L.lib(), L.stream()
    t = rp.nll_inputs(c)
    B, T, V, ldv, pad = c["B"], c["T"], c["V"], c["ldv"], t["pad"]
    n = B * T
    wt = R.ext_weight(c, "BT")
    buf = torch.zeros(n, ldv)
    buf[:, :V] = t["vocab"]
    inputs = dict(vocab=sha(buf), ptr=sha(t["ptr"]), sw=sha(t["sw"]), label=sha(t["label"]), up=sha(t["up"]), weight=sha(wt))
    vocab, ptr, sw, up, w = buf.cuda()[:, :V], t["ptr"].cuda(), t["sw"].cuda(), t["up"].cuda(), wt.cuda()
    label = t["label"].cuda().view(B, T)
    f32 = dict(dtype=torch.float32, device="cuda")
    out = {}

    def grads(dt):
        return torch.empty(n, ldv, dtype=dt, device="cuda"), torch.empty(n, T, dtype=dt, device="cuda"), torch.empty(n, **f32)

    def put(key, **tensors):
        torch.cuda.synchronize()
        out[key] = {k: sha(x) for k, x in tensors.items()}

    stats8, lse = torch.empty(8, **f32), torch.empty(n, 2, **f32)
    L.check(lib.pa_mixture_nll_fwd_fin(L.ptr(stats8), L.ptr(lse), L.ptr(vocab), ldv, L.ptr(ptr), L.ptr(sw), L.ptr(label), B, T, V, pad, st), "pa_mixture_nll_fwd_fin")
    put("fwd_fin", stats8=stats8, row_lse=lse)
    stats, lse4 = ops.mixture_nll_fwd(vocab, ptr, sw, label, V, pad)
    put("fwd", row_lse=lse4, count_hits=stats[1:3])
    for odt in ("f32", "bf16"):
        for gscale in (1.0, 0.25):
            for use_up in (False, True):
                dv, dp, dsw = grads(rp.DT[odt])
                L.check(lib.pa_mixture_nll_bwd_up(L.ptr(dv), L.ptr(dp), rp.PADT[odt], L.ptr(dsw), L.ptr(stats8), L.ptr(lse), L.ptr(vocab), ldv, L.ptr(ptr), L.ptr(sw),
                                                  L.ptr(label), B, T, V, pad, C.c_float(gscale), L.ptr(up) if use_up else None, st), "pa_mixture_nll_bwd_up")
                put(f"bwd_up/{odt}/gscale{gscale}/{'up' if use_up else 'stats3'}", dvocab=dv, dptr=dp, dsw=dsw)
    for tag, eps, weight, token in (("ext_off", 0.0, None, False), ("ext_eps0.1_wBT_token", 0.1, w, True)):
        s8, l2, ext, tok = ops.mixture_nll_ext_fwd(vocab, ptr, sw, label, V, pad, smoothing=eps, weight=weight, token_nll=token)
        put(f"{tag}/fwd", stats8=s8, row_lse=l2, ext_stats=ext, **({"token_nll": tok} if token else {}))
        for odt, gscale, use_up in rp.NLL_BWD_FORMS:
            dv, dp, dsw = grads(rp.DT[odt])
            ops.mixture_nll_ext_bwd(s8, l2, ext, vocab, ptr, sw, label, V, pad, smoothing=eps, weight=weight, gscale=gscale,
                                    upstream=up if use_up else None, out=dict(dvocab=dv, dptr=dp, dsw=dsw))
            put(f"{tag}/bwd/{odt}/gscale{gscale}/{'up' if use_up else 'stats3'}", dvocab=dv, dptr=dp, dsw=dsw)
    return dict(name=c["name"], inputs=inputs, outputs=out)


def nll_records():
    return [nll_record(c) for c in rp.nll_cases()]
