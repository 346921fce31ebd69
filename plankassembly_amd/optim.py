"""Fused Adam over the model's flat parameter buffer (one HIP kernel per step).

Same update rule and defaults as ``torch.optim.Adam(model.parameters(), lr=cfg.LR)`` used by the
reference (trainer_complete.py:127-129): betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad.
Also refreshes the model's bf16 GEMM-operand shadow in the same pass.

Optional gradient guard (``max_grad_norm`` / ``clip_value`` / ``skip_nonfinite``): the global norm of
the flat gradient buffer, the clip coefficient and the decision to apply or skip the step are computed on the device and
read by the Adam kernel, so a guarded step is three launches instead of one and never waits for the GPU.

Optional recipe extensions (``weight_decay`` / ``no_decay`` / ``ema_decay`` / ``ema_warmup``): decoupled
weight decay (torch.optim.AdamW) and an exponential moving average of the weights, both inside the same streaming pass
with or without the guard; and :func:`lr_factor`, the learning-rate schedule the trainer applies on the host.

Every step goes through pa_adam_step_ext (one Adam kernel: include/plank_hip.h); with nothing set it is pa_adam_step's rule bit for bit.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import ops


def _threshold(name, value):
    """None, or ``value`` as a float when it is a finite number above 0; anything else is a ValueError."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value <= 0:
        raise ValueError(f"{name} must be a finite number above 0 (or None for off), got {value!r}")
    return float(value)


LR_SCHEDULES = ("constant", "warmup", "cosine", "inverse_sqrt")
NO_DECAY_MODES = ("1d", "none")


def lr_factor(kind, step, warmup_steps=0, total_steps=0, min_ratio=0.0):
    """The factor on the base learning rate for optimizer step number ``step`` (0-based): a pure function.

    ``step`` counts the optimizer steps ATTEMPTED so far - the trainer's ``global_step``, which the host knows without asking
    the device.  A step the gradient guard skipped still advances the schedule, as a step torch AMP's GradScaler skipped still
    advances a Lightning scheduler.

    ``constant``: 1.  ``warmup``: min(1, (step + 1) / warmup_steps).  ``cosine``: that linear warmup, then
    min_ratio + (1 - min_ratio) * 0.5 * (1 + cos(pi * progress)) with progress running from 0 at ``warmup_steps`` to 1 at
    ``total_steps`` and staying there.  ``inverse_sqrt``: the linear warmup, then sqrt(warmup_steps / (step + 1))."""
    if kind not in LR_SCHEDULES:
        raise ValueError(f"lr schedule must be one of {LR_SCHEDULES}, got {kind!r}")
    for name, val in (("step", step), ("warmup_steps", warmup_steps), ("total_steps", total_steps)):
        if isinstance(val, bool) or not isinstance(val, int) or val < 0:
            raise ValueError(f"{name} must be an integer >= 0, got {val!r}")
    if isinstance(min_ratio, bool) or not isinstance(min_ratio, (int, float)) or not 0.0 <= min_ratio <= 1.0:
        raise ValueError(f"min_ratio must be a number in [0, 1], got {min_ratio!r}")
    if kind == "constant":
        return 1.0
    if kind in ("warmup", "inverse_sqrt") and warmup_steps < 1:
        raise ValueError(f"lr schedule {kind!r} needs warmup_steps >= 1, got {warmup_steps!r}")
    if kind == "cosine" and total_steps <= warmup_steps:
        raise ValueError(f"lr schedule 'cosine' needs total_steps > warmup_steps, got {total_steps!r} <= {warmup_steps!r}")
    if step < warmup_steps:
        return (step + 1) / warmup_steps
    if kind == "warmup":
        return 1.0
    if kind == "inverse_sqrt":
        return math.sqrt(warmup_steps / (step + 1))
    progress = min(1.0, (step - warmup_steps) / (total_steps - warmup_steps))
    return min_ratio + (1.0 - min_ratio) * 0.5 * (1.0 + math.cos(math.pi * progress))


def decay_bitmask(model, no_decay="1d"):
    """The host-side decay mask over ``model``'s flat buffer as a uint8 numpy array of ceil(numel / 8) bytes: bit (i & 7) of byte
    (i >> 3) is set when element i decays.  ``"1d"``: every element of every parameter with ndim >= 2; biases, LayerNorm gains
    and shifts and the alignment padding between parameters stay clear.  ``"none"``: None (every element decays)."""
    if no_decay not in NO_DECAY_MODES:
        raise ValueError(f"no_decay must be one of {NO_DECAY_MODES}, got {no_decay!r}")
    if no_decay == "none":
        return None
    bits = np.zeros(model.flat_params.numel(), dtype=np.uint8)
    for k, p in model.named_parameters():
        if p.ndim >= 2:
            off = model._offsets[k]
            bits[off:off + p.numel()] = 1
    return np.packbits(bits, bitorder="little")


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, max_grad_norm=None, clip_value=None,
                 skip_nonfinite=False, weight_decay=0.0, no_decay="1d", ema_decay=None, ema_warmup=False):
        """``max_grad_norm``: torch.nn.utils.clip_grad_norm_ over all gradients (after ``grad_scale``); ``clip_value``:
        clip_grad_value_; one of the two at most.  ``skip_nonfinite``: a step whose gradient norm is inf / NaN changes nothing
        (parameters, moments, bf16 shadow, Adam step count) and is counted instead - see :meth:`guard_stats`.

        ``weight_decay`` > 0: decoupled decay, p *= 1 - lr * weight_decay before the Adam update (torch.optim.AdamW), for the
        elements ``no_decay`` leaves in: ``"1d"`` exempts every parameter with ndim < 2, ``"none"`` decays everything.
        ``ema_decay`` in [0, 1): an exponential moving average of the weights, e += (1 - d_t) * (p_new - e) after every applied
        step, d_t = ema_decay, or min(ema_decay, (1 + t) / (10 + t)) at Adam step t with ``ema_warmup``; a skipped step leaves it
        alone.  See :meth:`ema_weights`.  ``lr`` is kept as ``base_lr``: the trainer's schedule sets
        ``param_groups[0]["lr"] = base_lr * lr_factor(...)`` before each step."""
        if isinstance(weight_decay, bool) or not isinstance(weight_decay, (int, float)) or not 0.0 <= weight_decay < math.inf:
            raise ValueError(f"weight_decay must be a finite number >= 0, got {weight_decay!r}")
        if no_decay not in NO_DECAY_MODES:
            raise ValueError(f"no_decay must be one of {NO_DECAY_MODES}, got {no_decay!r}")
        if ema_decay is not None and (isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float))
                                      or not 0.0 <= ema_decay < 1.0):
            raise ValueError(f"ema_decay must be a number in [0, 1) (or None for off), got {ema_decay!r}")
        max_grad_norm, clip_value = _threshold("max_grad_norm", max_grad_norm), _threshold("clip_value", clip_value)
        if max_grad_norm is not None and clip_value is not None:
            raise ValueError("max_grad_norm and clip_value are two clipping algorithms: set one of them")
        params = [p for p in model.parameters() if p.requires_grad]
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self.model = model
        self.grad_scale = grad_scale
        self.max_grad_norm, self.clip_value, self.skip_nonfinite = max_grad_norm, clip_value, bool(skip_nonfinite)
        self.guarded = max_grad_norm is not None or clip_value is not None or self.skip_nonfinite
        self._step = 0                # unguarded: the Adam step count; guarded: step0 of the workspace + attempts since
        self._m = None
        self._v = None
        self._ws = None               # the guard's device workspace (partials + control block), made on first use
        self._ws_stale = True         # True: the control block must be (re)initialised from self._step before the next step
        self.base_lr = lr
        self.weight_decay, self.no_decay = float(weight_decay), no_decay
        self.ema_decay, self.ema_warmup = None if ema_decay is None else float(ema_decay), bool(ema_warmup)
        self.extended = self.weight_decay > 0 or self.ema_decay is not None      # decay or EMA on
        self._ema = None              # f32 [numel] on the device, a copy of the weights when the first step begins
        self._ema_base = 0            # ema_updates - Adam step count (an EMA that began later than the optimizer: negative)
        self._bits = None             # the uploaded decay bitmask (no_decay "1d"), rebuilt when the flat buffer moves
        self._in_ema = False          # inside ema_weights(): the flat buffer holds the EMA

    def zero_grad(self, set_to_none: bool = True):
        for p in self.model._params.values():
            p.grad = None

    @torch.no_grad()
    def step(self, closure=None):
        if self._in_ema:
            raise RuntimeError("step() inside ema_weights(): the flat buffer holds the EMA, not the weights being trained")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        m = self.model
        flat, g = m.flat_params, m.flat_grads
        if self._m is None or self._m.device != flat.device:
            self._m = torch.zeros_like(flat)
            self._v = torch.zeros_like(flat)
        grp = self.param_groups[0]
        shadow = m._shadow if m.compute_dtype == "bf16" else None
        self._adam_step(flat, g, grp, shadow)
        # (the in-place update through the C ABI does not bump torch's version counters; a skipped guarded step rewrote
        # nothing, so a fresh shadow stays fresh either way)
        if shadow is not None:
            m.mark_shadow_fresh()
        else:
            m.invalidate_shadow()
        return loss

    def _enqueue_guard(self, flat, g, grp):
        """pa_grad_guard into the device control block (made and initialised from self._step on first use)."""
        lib = L.lib()
        if self._ws is None or self._ws.device != flat.device:
            self._ws = torch.empty(L.GRAD_GUARD_WS_BYTES, dtype=torch.uint8, device=flat.device)
            self._ws_stale = True
        nws = C.c_int64(self._ws.numel())
        if self._ws_stale:
            L.check(lib.pa_grad_guard_init(L.ptr(self._ws), nws, int(self._step), L.stream()), "pa_grad_guard_init")
            self._ws_stale = False
        self._step += 1
        b1, b2 = grp["betas"]
        L.check(lib.pa_grad_guard(L.ptr(g), C.c_int64(g.numel()), C.c_float(self.grad_scale),
                                  C.c_float(self.max_grad_norm or 0.0), int(self.skip_nonfinite), C.c_float(grp["lr"]),
                                  C.c_float(b1), C.c_float(b2), L.ptr(self._ws), nws, L.stream()), "pa_grad_guard")

    def _adam_step(self, flat, g, grp, shadow):
        """The one step path: pa_adam_step_ext, with decay and / or EMA inside the Adam pass when they are set.  With the guard on,
        pa_grad_guard first (norm, coefficient, apply-or-skip, bias corrections: all into the device control block) and the block
        handed to the kernel, which then takes the step count, and with it the EMA's d_t, from the device.  Enqueue only: whether
        a guarded step was applied is not known to the host here."""
        if self.ema_decay is not None:
            if self._ema is None:
                self._ema = flat.detach().clone()
                self._ema_base = -self._applied_steps()
            elif self._ema.device != flat.device:
                self._ema = self._ema.to(flat.device)
        masked = self.weight_decay > 0 and self.no_decay == "1d"
        if masked and (self._bits is None or self._bits.device != flat.device):
            self._bits = torch.from_numpy(decay_bitmask(self.model, "1d")).to(flat.device)
        if self.guarded:
            self._enqueue_guard(flat, g, grp)
        else:
            self._step += 1
        self.model.wait_transposed()             # (the side-stream W^T refresh of the step before reads what this kernel rewrites)
        ops.adam_step_ext(flat, g, self._m, self._v, step=self._step, ws=self._ws if self.guarded else None, lr=grp["lr"],
                          b1=grp["betas"][0], b2=grp["betas"][1], eps=grp["eps"], gscale=self.grad_scale,
                          clip_value=self.clip_value or 0.0, weight_decay=self.weight_decay,
                          decay_bits=self._bits if masked else None, ema=self._ema,
                          ema_decay=self.ema_decay or 0.0, ema_warmup=self.ema_warmup, p_bf16=shadow)

    @property
    def ema_updates(self):
        """The number of steps the EMA has followed: the applied steps since it began.  Guard on: a synchronising read."""
        return 0 if self._ema is None else self._applied_steps() + self._ema_base

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block ``model.flat_params`` (and with it every parameter, state_dict(), forward and decode) holds the EMA;
        on exit - also through an exception - the raw weights are back bit for bit, from a device-side stash.  The bf16 shadow
        and the W^T shadows are re-derived on entry and on exit.  Not re-entrant, and step() is refused inside."""
        if self._in_ema:
            raise RuntimeError("ema_weights() inside ema_weights()")
        if self.ema_decay is None:
            raise RuntimeError("ema_weights(): this FusedAdam was built without ema_decay")
        flat = self.model.flat_params
        ema = flat if self._ema is None else self._ema.to(flat.device)        # (before the first step the EMA IS the weights)
        stash = flat.detach().clone()
        self._in_ema = True
        try:
            self._swap_in(ema)
            yield self.model
        finally:
            self._swap_in(stash)
            self._in_ema = False

    @torch.no_grad()
    def _swap_in(self, src):
        m = self.model
        m.wait_transposed()                       # (a side-stream W^T refresh may still read what the copy rewrites)
        if src is not m.flat_params:
            m.flat_params.copy_(src)
        m.invalidate_shadow()
        if m._handle is not None:                 # bound to the runtime: bf16 shadow and W^T now, not at the next forward
            m._refresh_shadow()

    def _ctl(self):
        """The device control block (a synchronising 64-byte read), or None while it holds nothing newer than self._step."""
        if not self.guarded or self._ws is None or self._ws_stale:
            return None
        raw = self._ws[L.GRAD_GUARD_CTL_OFFSET:L.GRAD_GUARD_WS_BYTES].cpu().numpy().tobytes()
        return L.GradGuardCtl.from_buffer_copy(raw)

    def _applied_steps(self):
        """The Adam step count (what the bias correction of the next step builds on).  Guard on: the device's count."""
        c = self._ctl()
        return self._step if c is None else int(c.applied)

    def guard_stats(self):
        """The guard's counters and the last step's norm / clip coefficient.  The guard's ONE synchronising call (the trainer
        makes it once per epoch).  ``attempts`` / ``skipped_steps`` / ``first_skipped_attempt`` (1-based, -1: none) count from
        the construction of this optimizer or its last load_state_dict; ``applied_steps`` is the Adam step count."""
        if not self.guarded:
            raise RuntimeError("guard_stats(): this FusedAdam was built without max_grad_norm / clip_value / skip_nonfinite")
        c = self._ctl()
        if c is None:
            return {"norm": 0.0, "coef": 1.0, "applied_steps": self._step, "skipped_steps": 0, "attempts": 0,
                    "first_skipped_attempt": -1}
        return {"norm": float(c.norm), "coef": float(c.coef), "applied_steps": int(c.applied), "skipped_steps": int(c.skipped),
                "attempts": int(c.attempts), "first_skipped_attempt": int(c.first_skipped_attempt)}

    def state_dict(self):
        """Flat moments + step (CPU tensors: checkpoint payload)."""
        cpu = lambda t: None if t is None else t.detach().cpu()
        return {"step": self._applied_steps(), "m": cpu(self._m), "v": cpu(self._v),
                "ema": cpu(self._ema), "ema_updates": self.ema_updates, "weight_decay": self.weight_decay,
                "no_decay": self.no_decay,
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    # ---- torch.optim.Adam <-> flat layout (Lightning checkpoints store `optimizer_states` in torch's format)
    def _trainable(self):
        """(name, parameter) in ``model.parameters()`` order = the index order of torch.optim.Adam's state."""
        return [(k, p) for k, p in self.model.named_parameters() if p.requires_grad]

    def torch_state_dict(self):
        """The state as ``torch.optim.Adam(model.parameters()).state_dict()`` would hold it (CPU tensors); ``weight_decay`` is
        this optimizer's (one group: with ``no_decay="1d"`` torch would need two, which the flat layout does not record)."""
        state = {}
        step = self._applied_steps()
        if self._m is not None and step > 0:
            m, v = self._m.detach().cpu(), self._v.detach().cpu()
            for i, (k, p) in enumerate(self._trainable()):
                off, n = self.model._offsets[k], p.numel()
                state[i] = {"step": torch.tensor(float(step)), "exp_avg": m[off:off + n].view(p.shape).clone(),
                            "exp_avg_sq": v[off:off + n].view(p.shape).clone()}
        g = self.param_groups[0]
        group = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": self.weight_decay or 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "params": list(range(len(self._trainable())))}
        return {"state": state, "param_groups": [group]}

    def load_torch_state_dict(self, sd):
        """Inverse of :meth:`torch_state_dict`: accepts the ``optimizer_states[0]`` entry of a Lightning checkpoint written
        with the reference's torch.optim.Adam (trainer_complete.py:127-129)."""
        flat = self.model.flat_params
        self._m = torch.zeros_like(flat)
        self._v = torch.zeros_like(flat)
        steps = set()
        names = self._trainable()
        for i, st in sd.get("state", {}).items():
            k, p = names[int(i)]
            off, n = self.model._offsets[k], p.numel()
            self._m[off:off + n].copy_(st["exp_avg"].reshape(-1).to(flat.device, torch.float32))
            self._v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1).to(flat.device, torch.float32))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"per-parameter step counts differ ({sorted(steps)}): not a plain Adam state")
        self._step = steps.pop() if steps else 0
        self._ws_stale = True
        self._ema, self._ema_base = None, 0             # (torch's layout has no EMA: load_ema() restores one)
        for g, sg in zip(self.param_groups, sd.get("param_groups", [])):
            g["lr"], g["betas"], g["eps"] = sg.get("lr", g["lr"]), tuple(sg.get("betas", g["betas"])), sg.get("eps", g["eps"])

    def load_state_dict(self, sd):
        if "state" in sd:                                   # torch.optim.Adam layout
            return self.load_torch_state_dict(sd)
        dev = self.model.flat_params.device
        self._step = int(sd["step"])
        self._ws_stale = True
        self._m = None if sd.get("m") is None else sd["m"].to(dev, torch.float32).clone()
        self._v = None if sd.get("v") is None else sd["v"].to(dev, torch.float32).clone()
        self._ema, self._ema_base = None, 0
        if sd.get("ema") is not None and self.ema_decay is not None:
            self.load_ema(sd["ema"], sd.get("ema_updates", self._step))
        if "weight_decay" in sd:
            self.weight_decay = float(sd["weight_decay"])
            self.extended = self.weight_decay > 0 or self.ema_decay is not None
        if sd.get("no_decay") in NO_DECAY_MODES and sd["no_decay"] != self.no_decay:
            self.no_decay, self._bits = sd["no_decay"], None
        for g, sg in zip(self.param_groups, sd.get("param_groups", [])):
            for k in ("lr", "betas", "eps"):
                if k in sg:
                    g[k] = tuple(sg[k]) if k == "betas" else sg[k]

    def load_ema(self, flat_ema, ema_updates):
        """Restore the EMA (a flat f32 tensor in the layout of ``model.flat_params``) and the number of steps it has followed;
        call after the moments / step count are loaded."""
        if self.ema_decay is None:
            raise RuntimeError("load_ema(): this FusedAdam was built without ema_decay")
        flat = self.model.flat_params
        if flat_ema.numel() != flat.numel():
            raise ValueError(f"EMA of {flat_ema.numel()} elements for a flat buffer of {flat.numel()}")
        self._ema = flat_ema.detach().reshape(-1).to(flat.device, torch.float32).clone()
        self._ema_base = int(ema_updates) - self._step

    def ema_state_dict(self):
        """The EMA under the names and shapes of ``model.state_dict()`` (CPU tensors), or None while there is none."""
        if self._ema is None:
            return None
        e = self._ema.detach().cpu()
        out = {}
        for k, p in self.model.state_dict().items():
            off = self.model._offsets[k]
            out[k] = e[off:off + p.numel()].view(p.shape).clone()
        return out

    def load_ema_state_dict(self, sd, ema_updates):
        """Inverse of :meth:`ema_state_dict`; parameters ``sd`` does not name start from the current weights."""
        flat = self.model.flat_params.detach().cpu().clone()
        for k, t in sd.items():
            off = self.model._offsets[k]
            flat[off:off + t.numel()] = t.reshape(-1).to(torch.float32)
        self.load_ema(flat, ema_updates)
