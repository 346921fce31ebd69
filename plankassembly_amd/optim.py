"""Fused Adam over the model's flat parameter buffer (one HIP kernel per step).

Same update rule and defaults as ``torch.optim.Adam(model.parameters(), lr=cfg.LR)`` used by the
reference (trainer_complete.py:127-129): betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad.
Also refreshes the model's bf16 GEMM-operand shadow in the same pass.

Optional gradient guard (``max_grad_norm`` / ``clip_value`` / ``skip_nonfinite``): the global norm of
the flat gradient buffer, the clip coefficient and the decision to apply or skip the step are computed on the device and
read by a second Adam kernel, so a guarded step is three launches instead of one and never waits for the GPU.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L


def _threshold(name, value):
    """None, or ``value`` as a float when it is a finite number above 0; anything else is a ValueError."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value <= 0:
        raise ValueError(f"{name} must be a finite number above 0 (or None for off), got {value!r}")
    return float(value)


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, max_grad_norm=None, clip_value=None,
                 skip_nonfinite=False):
        """``max_grad_norm``: torch.nn.utils.clip_grad_norm_ over all gradients (after ``grad_scale``); ``clip_value``:
        clip_grad_value_; one of the two at most.  ``skip_nonfinite``: a step whose gradient norm is inf / NaN changes nothing
        (parameters, moments, bf16 shadow, Adam step count) and is counted instead - see :meth:`guard_stats`."""
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

    def zero_grad(self, set_to_none: bool = True):
        for p in self.model._params.values():
            p.grad = None

    @torch.no_grad()
    def step(self, closure=None):
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
        if self.guarded:
            self._guarded_step(flat, g, grp, shadow)
        else:
            self._plain_step(flat, g, grp, shadow)
        # (the in-place update through the C ABI does not bump torch's version counters; a skipped guarded step rewrote
        # nothing, so a fresh shadow stays fresh either way)
        if shadow is not None:
            m.mark_shadow_fresh()
        else:
            m.invalidate_shadow()
        return loss

    def _plain_step(self, flat, g, grp, shadow):
        self._step += 1
        self.model.wait_transposed()             # (the side-stream W^T refresh of the step before reads what this kernel rewrites)
        L.check(L.lib().pa_adam_step(L.ptr(flat), L.ptr(g), L.ptr(self._m), L.ptr(self._v), L.ptr(shadow),
                                     C.c_int64(flat.numel()), C.c_float(grp["lr"]), C.c_float(grp["betas"][0]),
                                     C.c_float(grp["betas"][1]), C.c_float(grp["eps"]), self._step,
                                     C.c_float(self.grad_scale), L.stream()), "pa_adam_step")

    def _guarded_step(self, flat, g, grp, shadow):
        """pa_grad_guard (norm, coefficient, apply-or-skip, bias corrections: all into the device control block), then the
        Adam kernel that reads them.  Enqueue only: whether the step was applied is not known to the host here."""
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
        self.model.wait_transposed()
        L.check(lib.pa_adam_step_guarded(L.ptr(flat), L.ptr(g), L.ptr(self._m), L.ptr(self._v), L.ptr(shadow),
                                         C.c_int64(flat.numel()), C.c_float(b1), C.c_float(b2), C.c_float(grp["eps"]),
                                         C.c_float(self.grad_scale), C.c_float(self.clip_value or 0.0),
                                         C.c_void_p(self._ws.data_ptr() + L.GRAD_GUARD_CTL_OFFSET), L.stream()),
                "pa_adam_step_guarded")

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
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    # ---- torch.optim.Adam <-> flat layout (Lightning checkpoints store `optimizer_states` in torch's format)
    def _trainable(self):
        """(name, parameter) in ``model.parameters()`` order = the index order of torch.optim.Adam's state."""
        return [(k, p) for k, p in self.model.named_parameters() if p.requires_grad]

    def torch_state_dict(self):
        """The state as ``torch.optim.Adam(model.parameters()).state_dict()`` would hold it (CPU tensors)."""
        state = {}
        step = self._applied_steps()
        if self._m is not None and step > 0:
            m, v = self._m.detach().cpu(), self._v.detach().cpu()
            for i, (k, p) in enumerate(self._trainable()):
                off, n = self.model._offsets[k], p.numel()
                state[i] = {"step": torch.tensor(float(step)), "exp_avg": m[off:off + n].view(p.shape).clone(),
                            "exp_avg_sq": v[off:off + n].view(p.shape).clone()}
        g = self.param_groups[0]
        group = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": 0, "amsgrad": False,
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
        for g, sg in zip(self.param_groups, sd.get("param_groups", [])):
            for k in ("lr", "betas", "eps"):
                if k in sg:
                    g[k] = tuple(sg[k]) if k == "betas" else sg[k]
