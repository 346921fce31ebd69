"""Float64 / float32 restatements of the extended mixture NLL (include/plank_hip.h pa_loss_ext) and their checker
(TEST INFRASTRUCTURE; plain numpy / torch, no GPU).  Case table, inputs, per-row quantities, `Checked`, the guard pattern and the
tiers are those of tests/rowops_parity.py; tests/test_loss_ext_cpu.py tests this file (against autograd and on seeded defects),
tests/test_loss_ext_gpu.py holds the kernels to it.

Definition, row (b, i) with label y and the training distribution log p of rowops_parity.nll_rows (pointer logits j >= i hold the
VALUE 1e-6 and stay in lse_p):
    plain = -log p_y;   smooth = -(1 / C) sum_{c allowed} log p_c,  allowed = {k < V} + {V + j : j < i},  C = V + i;
    ell = (1 - eps) plain + eps smooth  (eps == 0: plain; smooth is not formed);   loss = sum_valid w ell / N,  N = #non-PAD labels.

Bounds per element (u = 2^-24), rowops_parity's mixture-NLL bounds extended by first-order propagation.  Derived, not measured:
    log p_c = x_c - lse + l:   e(log p_c) = e_lse + e_l + 2 u (|x_c| + |lse| + |l|)                      (that file's own)
    smooth:   e = (1 / C) [sum_c e(log p_c) + (C + 2) u sum_c |log p_c|] + u |smooth|
    ell:      e = (1 - eps) e(plain) + eps e(smooth) + 2 u (|plain| + |smooth|)                        (eps == 0: e(plain))
    w ell:    e = |w| e(ell) + u |w ell|;   sum over `count` rows: sum e + (count + 2) u sum |w ell| (+ 2^-31 per block: the fixed-point word)
    loss, plain mean = sum / count:  e / count + u |.|;     token_nll: e(plain)
    gradients (row_lse, count, upstream as stored), G = gscale upstream / count w (3 roundings), E = exp(x - lse): e_E = u E (|x - lse| + 3),
      A = [label in this part] (E - hot): e_A = e_E + u |A|;   S = n E - 1 (n = V, or i for the pointers): e_S = n e_E + 2 u (n E + 1);
      t = (1 - eps) A + (eps / C) S:  e_t = (1 - eps) e_A + (eps / C) e_S + 3 u ((1 - eps) |A| + (eps / C) |S|);   d = G t:  |G| e_t + 3 u |d|
      dsw: dlv = -prob (0 when clamped): e_prob;  dlp = 1 - prob (0 when clamped): e_prob + u;  sel = dlv or dlp by the label's part, m = V dlv + i dlp:
      e_m = V e_prob + i (e_prob + u) + 2 u (V |dlv| + i |dlp|);  t = -(1 - eps) sel - (eps / C) m:  e_t = (1 - eps) e_sel + (eps / C) e_m
      + 3 u ((1 - eps) |sel| + (eps / C) |m|);  dsw = G t: |G| e_t + 3 u |dsw|.
Tier 1: |got - ref| <= 2 e.  Tier 2: r(got) <= FACTOR * r(cpu32), cpu32 the float32 restatement below - never the kernel's output.
"""
import numpy as np
import torch

import rowops_parity as rp
from rowops_parity import C6, U24, Checked, f64, nll_cases, nll_inputs, nll_rows, store          # noqa: F401  (re-exported to the tests)

# rowops_parity's rule: 16 unless a kernel that passes tier 1 was MEASURED above it on the hardware; then twice its worst measured
# value, never above 256 (profiles/loss_ext_time.txt holds the measurements).
FACTOR = {"loss_ext_fwd": 16.0, "loss_ext_bwd": 16.0}
EPS = (0.0, 0.1, 0.5)
WEIGHT_KINDS = (None, "B", "BT")
DEFECTS = ("smooth_over_fills", "weight_in_denominator", "dsw_without_eps", "weight_indexed_by_row", "inv_C_as_inv_V", "other_part_zero")


class ExtChecked(Checked):
    """rowops_parity.Checked with this file's FACTOR for tier 2 (tier 1 and the exact zeros are rowops_parity.check's)."""

    def __call__(self, what, got, ref, e, out_dt="f32", cpu=None, zero=None, kernel=None):
        k = kernel or self.kernel
        r, rc = rp.check(self.c["name"], what, "nll_bwd", got, ref, e, out_dt, None, zero)           # (no cpu: tier 2 is done below)
        if cpu is not None:
            ee = np.asarray(e, dtype=np.float64) + 0.5 * rp.TINY
            fin = np.isfinite(np.asarray(ref, dtype=np.float64))
            rc = rp.ratio(np.asarray(cpu, dtype=np.float64)[fin], np.asarray(ref, dtype=np.float64)[fin], ee[fin])
            if out_dt == "f32" and not r <= FACTOR[k] * rc:
                raise AssertionError(f"{self.c['name']}: {what} [{k}]: tier 2: r(got) = {r:.4g} > {FACTOR[k]:g} x r_cpu = {FACTOR[k]:g} x {rc:.4g}")
        if out_dt == "f32":
            self.r, self.r_cpu = max(self.r or 0.0, r), max(self.r_cpu or 0.0, rc or 0.0)


def ext_weight(c, kind):
    """Seeded float32 weights of a case: None, [B] or [B, T]; a zero and a negative one wherever the shape has room for both."""
    B, T = c["B"], c["T"]
    if kind is None:
        return None
    s = rp.seed_of(c["name"], 77)
    if kind == "B":
        w = rp.randn((B,), s, scale=0.5, shift=1.0)
        if B >= 2:
            w[0], w[1] = -0.5, 0.0
        return w
    w = rp.randn((B, T), s + 1, scale=0.5, shift=1.0)
    w[:, 1], w[:, 2] = 0.0, -0.75
    return w


def _row_weight(c, w, wrong_index=False):
    """Weight per row [B * T] (float64), 1 without weights."""
    B, T = c["B"], c["T"]
    if w is None:
        return np.ones(B * T)
    w = f64(w)
    if w.ndim == 2:
        return w.reshape(-1)
    return w[np.arange(B * T) % B] if wrong_index else np.repeat(w, T)


def _switch_logs(R):
    """lv, lp and their bounds as rowops_parity.nll_rows forms them (it does not return them)."""
    prob, q = R["prob"], 1 - R["prob"]
    lv, lp = np.log(np.maximum(q, C6)), np.log(np.maximum(prob, C6))
    e_lv = np.where(q < C6, 0.0, (R["e_prob"] + U24 * q) / np.maximum(q, C6)) + U24 * np.abs(lv)
    e_lp = np.where(prob < C6, 0.0, R["e_prob"] / np.maximum(prob, C6)) + U24 * np.abs(lp)
    return lv, lp, e_lv, e_lp


def ext_fwd_ref(c, t, eps, w):
    """Float64 forward: objective sum, loss, plain sum / mean, token_nll, each with its bound; count, hits and row_lse from rowops_parity."""
    base = rp.nll_fwd_ref(c, t, fixed=True)
    R = base["R"]
    V, T = c["V"], c["T"]
    i = R["i"]
    Cn = (V + i).astype(np.float64)
    plain, e_plain = -R["logp"], R["e_logp"]
    if eps > 0:
        lv, lp, e_lv, e_lp = _switch_logs(R)
        lpv = R["x"] - R["lse_v"][:, None] + lv[:, None]
        e_lpv = (R["e_lse_v"] + e_lv)[:, None] + 2 * U24 * (np.abs(R["x"]) + np.abs(R["lse_v"] + 0.0)[:, None] + np.abs(lv)[:, None])
        ok = ~R["masked"]
        lpp = np.where(ok, R["p"] - R["lse_p"][:, None] + lp[:, None], 0.0)
        e_lpp = np.where(ok, (R["e_lse_p"] + e_lp)[:, None] + 2 * U24 * (np.abs(R["p"]) + np.abs(R["lse_p"])[:, None] + np.abs(lp)[:, None]), 0.0)
        smooth = -(lpv.sum(1) + lpp.sum(1)) / Cn
        e_smooth = (e_lpv.sum(1) + e_lpp.sum(1) + (Cn + 2) * U24 * (np.abs(lpv).sum(1) + np.abs(lpp).sum(1))) / Cn + U24 * np.abs(smooth)
        ell = (1 - eps) * plain + eps * smooth
        e_ell = (1 - eps) * e_plain + eps * e_smooth + 2 * U24 * (np.abs(plain) + np.abs(smooth))
    else:
        ell, e_ell = plain, e_plain
    wr = _row_weight(c, w)
    valid = R["valid"]
    term = np.where(valid & (wr != 0), wr * np.where(valid, ell, 0.0), 0.0)
    e_term = np.where(valid, np.abs(wr) * e_ell + U24 * np.abs(term), 0.0)
    cnt = base["count"]
    blocks = -(-(c["B"] * T) // 4)
    obj = term.sum()
    e_obj = e_term.sum() + (cnt + 2) * U24 * np.abs(term).sum() + blocks * 2.0 ** -31
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float64(obj) / np.float64(cnt)
        e_loss = (e_obj / cnt + U24 * abs(loss)) if cnt else 0.0
    return dict(R=R, base=base, obj=(obj, e_obj), loss=(loss, e_loss), nll=base["nll"], mean=base["loss"], count=cnt, hits=base["hits"], lse=base["lse"],
                token=(np.where(valid, plain, 0.0), np.where(valid, e_plain, 0.0)), ell=np.where(valid, ell, 0.0))


def ext_fwd_cpu32(c, t, eps, w, defect=None):
    """The forward restated in float32 on the CPU, in the kernel's arithmetic: smooth from sum x - V lse + V lv, not from a matrix of log p."""
    B, T, V = c["B"], c["T"], c["V"]
    f32 = np.float32
    x, z, s, lab = t["vocab"], t["ptr"].clone(), t["sw"], t["label"]
    n = B * T
    i = torch.arange(n) % T
    masked = torch.arange(T)[None, :] >= i[:, None]
    z[masked] = C6

    def lse(a):
        m = a.max(1).values
        return m + torch.log(torch.exp(a - m[:, None]).sum(1))
    lse_v, lse_p = lse(x), lse(z)
    prob = 1.0 / (1.0 + torch.exp(-s))
    lv, lp = torch.log(torch.clamp(1 - prob, min=C6)), torch.log(torch.clamp(prob, min=C6))
    valid = lab != t["pad"]
    is_v = valid & (lab < V)
    r = torch.arange(n)
    logp = torch.where(is_v, x[r, lab.clamp(0, V - 1)] - lse_v + lv, z[r, (lab - V).clamp(0, T - 1)] - lse_p + lp)
    plain = torch.where(valid, -logp, torch.zeros_like(logp))
    ell = plain
    if eps > 0:
        Vf, If = f32(V), i.to(torch.float32)
        sum_x = x.sum(1)
        if defect == "smooth_over_fills":
            sum_z, If_z, Cn = z.sum(1), torch.full_like(If, T), torch.full_like(If, V + T)
        else:
            sum_z, If_z, Cn = torch.where(masked, torch.zeros(1), z).sum(1), If, Vf + If
        if defect == "inv_C_as_inv_V":
            Cn = torch.full_like(If, V)
        av = (sum_x - Vf * lse_v) + Vf * lv
        ap = (sum_z - If_z * lse_p) + If_z * lp
        smooth = -(av + ap) / Cn
        ell = f32(1 - f32(eps)) * plain + f32(eps) * smooth
    wr = torch.from_numpy(_row_weight(c, w, defect == "weight_indexed_by_row")).to(torch.float32)
    term = torch.where(valid & (wr != 0), wr * ell, torch.zeros_like(ell))
    cnt = int(valid.sum())
    obj = term.sum()
    den = float((wr * valid).sum()) if defect == "weight_in_denominator" else cnt
    nll = plain.sum()
    av_, ap_ = x.argmax(1), z.argmax(1)
    pred = torch.where(z[r, ap_] - lse_p + lp > x[r, av_] - lse_v + lv, V + ap_, av_)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = float(f32(obj) / f32(den)) if den else float("nan")
        mean = float(f32(nll) / f32(cnt)) if cnt else float("nan")
    return dict(obj=float(obj), loss=loss, nll=float(nll), mean=mean, count=cnt, hits=int((valid & (pred == lab)).sum()), token=plain.numpy(),
                lse=torch.stack([lse_v, lse_p], 1).numpy(), den=den)


def _bwd_parts(R, c, t, lse_v, lse_p):
    V, T = c["V"], c["T"]
    n = c["B"] * T
    r = np.arange(n)
    hot_v = np.zeros((n, V)); hot_v[r[R["is_v"]], R["lab"][R["is_v"]]] = 1.0
    hot_p = np.zeros((n, T)); hot_p[r[R["is_p"]], R["lab"][R["is_p"]] - V] = 1.0
    hot_p[R["masked"]] = 0.0
    zz = np.where(R["masked"], 0.0, f64(t["ptr"]))
    with np.errstate(over="ignore"):
        Ev = np.exp(R["x"] - lse_v[:, None])
        Ep = np.where(R["masked"], 0.0, np.exp(zz - lse_p[:, None]))
    return hot_v, hot_p, zz, Ev, Ep


def ext_bwd_ref(c, t, eps, w, row_lse32, count32, up32, gscale):
    """Float64 gradients from the STORED row_lse [n][2], count and upstream value (float32 as the kernel reads them), with bounds and the
    masks of the elements that must be exactly zero."""
    R = nll_rows(c, t)
    V, T = c["V"], c["T"]
    n = c["B"] * T
    lse_v, lse_p = f64(row_lse32)[:, 0], f64(row_lse32)[:, 1]
    wr = _row_weight(c, w)
    live = R["valid"] & (wr != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        g0 = float(np.float64(np.float32(gscale)) * np.float64(up32) / np.float64(count32)) if R["valid"].any() else 0.0
    G = np.where(live, g0 * wr, 0.0)[:, None]
    hot_v, hot_p, zz, Ev, Ep = _bwd_parts(R, c, t, lse_v, lse_p)
    i = R["i"].astype(np.float64)[:, None]
    Cn = V + i
    om, ec = 1.0 - eps, eps / Cn
    in_v, in_p = R["is_v"][:, None], R["is_p"][:, None]
    ok = ~R["masked"]
    e_Ev = U24 * Ev * (np.abs(R["x"] - lse_v[:, None]) + 3)
    e_Ep = U24 * Ep * (np.abs(zz - lse_p[:, None]) + 3)
    Av, Ap = np.where(in_v, Ev - hot_v, 0.0), np.where(in_p & ok, Ep - hot_p, 0.0)
    e_Av, e_Ap = np.where(in_v, e_Ev + U24 * np.abs(Av), 0.0), np.where(in_p & ok, e_Ep + U24 * np.abs(Ap), 0.0)
    if eps > 0:
        Sv, Sp = V * Ev - 1.0, np.where(ok, i * Ep - 1.0, 0.0)
        e_Sv, e_Sp = V * e_Ev + 2 * U24 * (V * Ev + 1), np.where(ok, i * e_Ep + 2 * U24 * (i * Ep + 1), 0.0)
    else:
        Sv = Sp = e_Sv = e_Sp = 0.0
    tv, tp = om * Av + ec * Sv, om * Ap + ec * Sp
    e_tv = om * e_Av + ec * e_Sv + 3 * U24 * (om * np.abs(Av) + ec * np.abs(Sv))
    e_tp = om * e_Ap + ec * e_Sp + 3 * U24 * (om * np.abs(Ap) + ec * np.abs(Sp))
    dv, dp = G * tv, G * tp
    e_dv, e_dp = np.abs(G) * e_tv + 3 * U24 * np.abs(dv), np.abs(G) * e_tp + 3 * U24 * np.abs(dp)
    prob, q = R["prob"], 1 - R["prob"]
    dlv, dlp = np.where(q >= C6, -prob, 0.0), np.where(prob >= C6, q, 0.0)
    e_dlv, e_dlp = R["e_prob"], R["e_prob"] + U24
    sel, e_sel = np.where(R["is_v"], dlv, dlp), np.where(R["is_v"], e_dlv, e_dlp)
    i1, C1, ec1 = i[:, 0], Cn[:, 0], (eps / Cn)[:, 0]
    m = V * dlv + i1 * dlp
    e_m = V * e_dlv + i1 * e_dlp + 2 * U24 * (V * np.abs(dlv) + i1 * np.abs(dlp))
    ts = -om * sel - ec1 * m
    e_ts = om * e_sel + ec1 * e_m + 3 * U24 * (om * np.abs(sel) + ec1 * np.abs(m))
    dsw = G[:, 0] * ts
    e_dsw = np.abs(G[:, 0]) * e_ts + 3 * U24 * np.abs(dsw)
    dead = ~live[:, None]
    zero_v = dead | ((~in_v) & (eps == 0)) | np.zeros((1, V), bool)
    zero_p = dead | R["masked"] | ((~in_p) & (eps == 0))
    return dict(dv=(dv, e_dv), dp=(dp, e_dp), dsw=(dsw, e_dsw), zero_v=zero_v, zero_p=zero_p, zero_s=~live)


def ext_bwd_cpu32(c, t, eps, w, row_lse32, count32, up32, gscale, defect=None, den=None):
    """The backward restated in float32 on the CPU.  `den`: the denominator a defective forward divided by (weight_in_denominator)."""
    V, T = c["V"], c["T"]
    n = c["B"] * T
    f32 = np.float32
    x, z, s, lab = t["vocab"], t["ptr"], t["sw"], t["label"]
    i = torch.arange(n) % T
    masked = torch.arange(T)[None, :] >= i[:, None]
    valid = lab != t["pad"]
    is_v, is_p = valid & (lab < V), valid & (lab >= V)
    wr = torch.from_numpy(_row_weight(c, w, defect == "weight_indexed_by_row")).to(torch.float32)
    live = valid & (wr != 0)
    count = f32(den) if (defect == "weight_in_denominator" and den is not None) else f32(count32)
    g0 = f32(gscale) * f32(up32) / count if float(count) else f32(0)
    G = torch.where(live, g0 * wr, torch.zeros(1))[:, None]
    r = torch.arange(n)
    hot_v = torch.zeros(n, V); hot_v[r[is_v], lab[is_v]] = 1.0
    hot_p = torch.zeros(n, T); hot_p[r[is_p], lab[is_p] - V] = 1.0
    hot_p[masked] = 0.0
    Ev, Ep = torch.exp(x - row_lse32[:, :1]), torch.exp(z - row_lse32[:, 1:])
    zero = torch.zeros(1)
    Av, Ap = torch.where(is_v[:, None], Ev - hot_v, zero), torch.where(is_p[:, None], Ep - hot_p, zero)
    prob = 1.0 / (1.0 + torch.exp(-s))
    dlv, dlp = torch.where(1 - prob >= C6, -prob, zero), torch.where(prob >= C6, 1 - prob, zero)
    sel = torch.where(is_v, dlv, dlp)
    If = i.to(torch.float32)
    if eps > 0:
        om = f32(1 - f32(eps))
        Vf = f32(V)
        n_p = torch.full_like(If, T) if defect == "smooth_over_fills" else If
        Cn = Vf + n_p
        if defect == "inv_C_as_inv_V":
            Cn = torch.full_like(If, V)
        ec = f32(eps) / Cn
        tv = om * Av + ec[:, None] * (Vf * Ev - 1)
        tp = om * Ap + ec[:, None] * (n_p[:, None] * Ep - 1)
        if defect == "other_part_zero":
            tv, tp = torch.where(is_v[:, None], tv, zero), torch.where(is_p[:, None], tp, zero)
        ts = -om * sel - (0 if defect == "dsw_without_eps" else ec * (Vf * dlv + n_p * dlp))
    else:
        tv, tp, ts = Av, Ap, -sel
    dv = G * tv
    dp = torch.where(masked & torch.tensor(defect != "smooth_over_fills" or eps == 0), zero, G * tp)
    dsw = G[:, 0] * ts
    return dict(dv=dv.numpy(), dp=dp.numpy(), dsw=dsw.numpy())


def loss_from_dists(dists, label, pad, eps, weight=None):
    """The definition as torch operations on a matrix of log-probabilities [B, T, V + T] (create_dist_train of oracle/plank_oracle.py), so that
    autograd can differentiate it: (loss, plain mean, token_nll [B, T]).  `weight`: None, [B] or [B, T]."""
    B, T, W = dists.shape
    V = W - T
    valid = label != pad
    plain = -dists.gather(-1, label.clamp(0, W - 1)[..., None])[..., 0]
    ell = plain
    if eps > 0:
        allowed = torch.cat((torch.ones(T, V), torch.tril(torch.ones(T, T), -1)), 1) == 1            # row i: every k < V, pointers j < i
        Cn = (V + torch.arange(T)).to(dists.dtype)
        smooth = -torch.where(allowed[None], dists, torch.zeros((), dtype=dists.dtype)).sum(-1) / Cn[None]
        ell = (1 - eps) * plain + eps * smooth
    w = torch.ones(B, T, dtype=dists.dtype) if weight is None else (weight.to(dists.dtype) if weight.dim() == 2 else weight.to(dists.dtype)[:, None].expand(B, T))
    zero = torch.zeros((), dtype=dists.dtype)
    N = valid.sum()
    token = torch.where(valid, plain, zero)
    return torch.where(valid, w * ell, zero).sum() / N, token.sum() / N, token


def simulate(c, t, eps, w, defect=None):
    """What the entries would return if they computed the float32 restatement (with a seeded defect): the shape verify() takes."""
    f = ext_fwd_cpu32(c, t, eps, w, defect)
    got = dict(fwd=f, bwd=[])
    lse32, cnt = torch.from_numpy(f["lse"]), np.float32(f["count"])
    for odt, gscale, use_up in rp.NLL_BWD_FORMS:
        up = np.float32(t["up"][0]) if use_up else np.float32(1.0)
        b = ext_bwd_cpu32(c, t, eps, w, lse32, cnt, up, gscale, defect, den=f["den"])
        got["bwd"].append(dict(lse32=lse32, count32=cnt, up32=up, dv=store(b["dv"], odt), dp=store(b["dp"], odt), dsw=b["dsw"]))
    return got


def verify(c, t, eps, w, got):
    """Every output of one (case, eps, weight) against the float64 reference under tiers 1 / 2.  got: {'fwd': {obj, loss, nll, mean, count,
    hits, token [n], lse [n][2]}, 'bwd': [{lse32, count32, up32, dv [n][V], dp [n][T], dsw [n]} per rowops_parity.NLL_BWD_FORMS]}."""
    ck, ckb = ExtChecked(c, "loss_ext_fwd"), ExtChecked(c, "loss_ext_bwd")
    ref, cpu = ext_fwd_ref(c, t, eps, w), ext_fwd_cpu32(c, t, eps, w)
    f = got["fwd"]
    one = lambda v: np.array([v], dtype=np.float64)
    ck("row_lse", f["lse"], *ref["lse"], cpu=cpu["lse"])
    ck("objective sum", one(f["obj"]), one(ref["obj"][0]), one(ref["obj"][1]), cpu=one(cpu["obj"]))
    ck("loss", one(f["loss"]), one(ref["loss"][0]), one(ref["loss"][1]), cpu=one(cpu["loss"]))
    ck("plain sum", one(f["nll"]), one(ref["nll"][0]), one(ref["nll"][1]), cpu=one(cpu["nll"]))
    ck("plain mean", one(f["mean"]), one(ref["mean"][0]), one(ref["mean"][1]), cpu=one(cpu["mean"]))
    ck("token_nll", np.asarray(f["token"]).reshape(-1), *ref["token"], cpu=cpu["token"], zero=~ref["R"]["valid"])
    assert f["count"] == ref["count"], f"{c['name']}: count {f['count']!r}, want {ref['count']}"
    assert f["hits"] == int(f["hits"]) and ref["hits"][0] <= f["hits"] <= ref["hits"][1], f"{c['name']}: hits {f['hits']!r}, want {ref['hits']}"
    for (odt, gscale, use_up), b in zip(rp.NLL_BWD_FORMS, got["bwd"]):
        rb = ext_bwd_ref(c, t, eps, w, b["lse32"], b["count32"], b["up32"], gscale)
        cb = ext_bwd_cpu32(c, t, eps, w, b["lse32"], b["count32"], b["up32"], gscale)
        what = f"{odt} gscale {gscale} {'upstream' if use_up else 'stats[3]'}"
        ckb(f"dvocab {what}", b["dv"], *rb["dv"], out_dt=odt, cpu=cb["dv"], zero=rb["zero_v"])
        ckb(f"dptr {what}", b["dp"], *rb["dp"], out_dt=odt, cpu=cb["dp"], zero=rb["zero_p"])
        ckb(f"dsw {what}", b["dsw"], *rb["dsw"], cpu=cb["dsw"], zero=rb["zero_s"])
    return [("loss_ext_fwd", ck.r, ck.r_cpu), ("loss_ext_bwd", ckb.r, ckb.r_cpu)]
