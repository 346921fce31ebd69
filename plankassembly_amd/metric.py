"""Box matching metric of the evaluation callers.

``HungarianMatcher`` follows reference third_party/matcher.py:15-78 (3-D axis-aligned IoU between
predicted and ground-truth planks, Hungarian assignment with cost -1 where IoU > threshold, TP
counted where the matched IoU >= threshold) and ``Criterion`` follows reference
plankassembly/metric.py:6-30 (running sums of precision / recall / F1 and a count, summed over
ranks).  Written from scratch on numpy/scipy: <= 21 boxes per sample, CPU work by nature.

``DevicePlankScorer`` (opt-in, trainer hparam ``DEVICE_METRIC``) does the matching of a whole batch in one
launch of ``ops.plank_match`` and keeps only the tie cases for the host matcher; its means are ``PlankScorer``'s bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from .distributed import allreduce_metric_sums

LARGE_COST = 100000


def pairwise_iou_3d(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a [N,6], b [M,6] as (x1,y1,z1,x2,y2,z2) -> IoU [N,M] (0 where the union is empty)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 6)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 6)
    va = np.prod(a[:, 3:] - a[:, :3], axis=1)
    vb = np.prod(b[:, 3:] - b[:, :3], axis=1)
    lo = np.maximum(a[:, None, :3], b[None, :, :3])
    hi = np.minimum(a[:, None, 3:], b[None, :, 3:])
    inter = np.prod(np.clip(hi - lo, 0, None), axis=2)
    union = va[:, None] + vb[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(inter > 0, inter / union, 0.0)
    return iou


class HungarianMatcher:
    def __init__(self, threshold: float = 0.5):
        assert threshold != 0, "threshold cant be 0"
        self.threshold = threshold

    def __call__(self, pred_boxes, boxes):
        pb = pred_boxes.detach().cpu().numpy() if torch.is_tensor(pred_boxes) else np.asarray(pred_boxes)
        gb = boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else np.asarray(boxes)
        n_pred, n_gt = len(pb), len(gb)
        iou = pairwise_iou_3d(pb, gb)
        cost = np.full((n_pred, n_gt), LARGE_COST)
        cost[iou > self.threshold] = -1
        r, c = linear_sum_assignment(cost)
        tp = float(np.sum(iou[r, c] >= self.threshold))
        prec = torch.tensor(tp / n_pred if n_pred else 0.0)
        rec = torch.tensor(tp / n_gt if n_gt else 0.0)
        f1 = prec * rec * 2 / (prec + rec + 1e-10)
        return prec, rec, f1


def build_matcher(threshold):
    return HungarianMatcher(threshold)


class Criterion:
    """Stand-in for the reference's torchmetrics Metric (torchmetrics is not installed here)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.sums = torch.zeros(4, dtype=torch.float64)      # precision, recall, fmeasure, total

    def update(self, prec, rec, f1):
        self.sums += torch.tensor([float(prec), float(rec), float(f1), 1.0], dtype=torch.float64)

    def compute(self, sync=True):
        s = self.sums.clone()
        if sync:
            s = allreduce_metric_sums(s)
        total = s[3].clamp(min=1.0) if s[3] == 0 else s[3]
        return s[0] / total, s[1] / total, s[2] / total


def build_criterion():
    return Criterion()


class PlankScorer:
    """One sample at a time: match predicted planks against ground-truth planks (row 0 of both is the overall bounding
    box and takes no part - reference trainer_complete.py:80, evaluate.py:54), feed the running means, hand the three
    numbers back.  The validation / test hooks of the trainers and the offline re-scoring of evaluate.py all go
    through here, so a sample is scored the same way wherever it is scored."""

    def __init__(self, threshold: float):
        self.matcher = build_matcher(threshold)
        self.criterion = build_criterion()

    def add(self, planks, truth):
        scores = self.matcher(planks[1:], truth[1:])
        self.criterion.update(*scores)
        return {"precision": float(scores[0]), "recall": float(scores[1]), "fmeasure": float(scores[2])}

    def means(self, sync=True):
        """(precision, recall, fmeasure) averaged over every sample added since the last call; resets."""
        out = tuple(float(x) for x in self.criterion.compute(sync=sync))
        self.criterion.reset()
        return out


def prf_from_counts(tp, n_pred, n_gt):
    """``HungarianMatcher.__call__``'s last four lines for many drawings at once: float64 quotients rounded to float32, then the
    same float32 torch CPU expressions - elementwise, so every drawing gets the bits the one-at-a-time call gives it."""
    tp = np.asarray(tp, dtype=np.float64).reshape(-1)
    n_pred = np.asarray(n_pred, dtype=np.int64).reshape(-1)
    n_gt = np.asarray(n_gt, dtype=np.int64).reshape(-1)
    prec = torch.from_numpy(np.where(n_pred > 0, tp / np.maximum(n_pred, 1), 0.0)).to(torch.float32)
    rec = torch.from_numpy(np.where(n_gt > 0, tp / np.maximum(n_gt, 1), 0.0)).to(torch.float32)
    f1 = prec * rec * 2 / (prec + rec + 1e-10)
    return prec, rec, f1


def planks_of_row(row, end_token, dof=6):
    """``PlankModel.parse_sequence`` on a host row: the whole planks before the first END, [n, dof]."""
    row = np.asarray(row).reshape(-1)
    hits = np.nonzero(row == end_token)[0]
    n = (int(hits[0]) if len(hits) else len(row)) // dof
    return row[: n * dof].reshape(-1, dof)


def valid_planks(pred):
    """The trainers' ``_valid_pred`` on a host array: planks with a zero extent dropped, row 0 (the bounding box) kept."""
    if len(pred) <= 1:
        return pred
    ok = np.all(np.abs(pred[1:, 3:] - pred[1:, :3]) != 0, axis=1)
    return np.concatenate((pred[:1], pred[1:][ok]))


class DevicePlankScorer:
    """``PlankScorer`` with the matching on the GPU: ``add_batch`` launches ``ops.plank_match`` once for a
    whole batch of decoded rows against their ground-truth rows and reads nothing back; ``means`` copies the integers of every
    batch to the host in one transfer, forms precision / recall / F1 per drawing with HungarianMatcher's own float32 expressions
    and feeds the same ``Criterion`` in drawing order - the means are bit-identical to ``PlankScorer``'s.

    A pair of planks at IoU == threshold exactly is no edge of the matching but counts as a true positive when scipy happens to
    assign it among the equal-cost leftovers; the kernel reports the number of such pairs per drawing (``ties``) and those
    drawings - only those - are scored by ``HungarianMatcher`` on their tokens, like the host path.

    ``match``: the launch, ``(samples, truth) -> int [B, 4]`` (tp, n_pred, n_gt, ties); the tests put a restatement here."""

    def __init__(self, threshold: float, end_token: int, match=None):
        self.threshold, self.end_token = float(threshold), int(end_token)
        self.matcher = build_matcher(threshold)
        self.criterion = build_criterion()
        self._match = match or self._launch
        self._pending = []                     # (counts [B, 4], samples, truth, keep) of the batches not yet read back
        self.fallbacks = 0                     # drawings that went to the host matcher because of a tie

    def _launch(self, samples, truth):
        from . import ops
        return ops.plank_match(samples, truth.to(samples.device), end_token=self.end_token, filter_a=True, filter_b=False,
                               threshold=self.threshold)

    def add(self, planks, truth):
        """One drawing on the host, as ``PlankScorer.add`` (after everything ``add_batch`` has queued: the sums keep their order)."""
        self._resolve()
        scores = self.matcher(planks[1:], truth[1:])
        self.criterion.update(*scores)
        return {"precision": float(scores[0]), "recall": float(scores[1]), "fmeasure": float(scores[2])}

    def add_batch(self, samples, truth_tokens, scores=False, keep=None):
        """Decoded rows ``samples`` int64 [B, n] against the ground-truth rows ``truth_tokens`` int64 [B, T]: one launch, nothing
        read back.  ``keep``: host booleans [B], False for a drawing that takes no part (SidefaceTrainer's empty inputs).
        ``scores=True`` reads this batch (and everything queued before it) back now and returns the per-drawing dicts of
        ``PlankScorer.add`` (None where ``keep`` is False)."""
        if samples.shape[0] != truth_tokens.shape[0]:
            raise ValueError(f"{samples.shape[0]} decoded rows against {truth_tokens.shape[0]} ground-truth rows")
        keep = None if keep is None else [bool(k) for k in keep]
        self._pending.append((self._match(samples, truth_tokens), samples, truth_tokens, keep))
        return self._resolve()[-1] if scores else None

    def _resolve(self):
        """Everything queued -> the criterion, in drawing order.  One device-to-host copy of the integers; tokens only for ties."""
        pending, self._pending = self._pending, []
        if not pending:
            return []
        counts = torch.cat([p[0].reshape(-1, 4) for p in pending]).cpu().numpy().astype(np.int64)
        prec, rec, f1 = prf_from_counts(counts[:, 0], counts[:, 1], counts[:, 2])
        out, at = [], 0
        for c, samples, truth, keep in pending:
            B = c.shape[0]
            mine = counts[at:at + B]
            p, r, f = prec[at:at + B].clone(), rec[at:at + B].clone(), f1[at:at + B].clone()
            tied = [i for i in np.nonzero(mine[:, 3] > 0)[0].tolist() if keep is None or keep[i]]
            if tied:                                                    # the host path for these drawings, on their tokens
                idx = torch.as_tensor(tied)
                s_rows = samples.index_select(0, idx.to(samples.device)).cpu().numpy()
                t_rows = truth.index_select(0, idx.to(truth.device)).cpu().numpy()
                for k, i in enumerate(tied):
                    pred = valid_planks(planks_of_row(s_rows[k], self.end_token))
                    gt = planks_of_row(t_rows[k], self.end_token)
                    p[i], r[i], f[i] = self.matcher(pred[1:], gt[1:])
                self.fallbacks += len(tied)
            dicts = []
            for i in range(B):
                if keep is not None and not keep[i]:
                    dicts.append(None)
                    continue
                self.criterion.update(p[i], r[i], f[i])
                dicts.append({"precision": float(p[i]), "recall": float(r[i]), "fmeasure": float(f[i])})
            out.append(dicts)
            at += B
        return out

    def means(self, sync=True):
        """(precision, recall, fmeasure) averaged over every drawing added since the last call; resets."""
        self._resolve()
        out = tuple(float(x) for x in self.criterion.compute(sync=sync))
        self.criterion.reset()
        return out


OVERLAP_MODES = ("ignore", "match", "visible")


def _overlap_lines(side, end_token, num_bits, read_type, drop_hidden):
    """One encoder row -> (kept lines int64 [k, 6] = group, c, lo, hi, type, length; number skipped).  group = view * 2 + vertical."""
    value = np.asarray(side[0], dtype=np.int64).reshape(-1)
    view = np.asarray(side[1], dtype=np.int64).reshape(-1)
    hits = np.nonzero(value == end_token)[0]
    n = (int(hits[0]) if len(hits) else len(value)) // 4
    t = value[:4 * n].reshape(n, 4)
    vw = view[:4 * n:4]
    ty = np.zeros(n, dtype=np.int64)
    if read_type and len(side) > 2 and side[2] is not None:
        ty = np.clip(np.asarray(side[2], dtype=np.int64).reshape(-1)[:4 * n:4], -2 ** 31, 2 ** 31 - 1)
    part = ty == 0 if drop_hidden else np.ones(n, dtype=bool)
    x0, x1 = np.minimum(t[:, 0], t[:, 2]), np.maximum(t[:, 0], t[:, 2])
    y0, y1 = np.minimum(t[:, 1], t[:, 3]), np.maximum(t[:, 1], t[:, 3])
    ok = part & np.all((t >= 0) & (t < 2 ** int(num_bits)), axis=1) & (vw >= 0) & (vw <= 2)
    hor, ver = ok & (y0 == y1) & (x0 < x1), ok & (x0 == x1) & (y0 < y1)
    rows = np.concatenate((np.stack((vw * 2, y0, x0, x1, ty, x1 - x0), 1)[hor], np.stack((vw * 2 + 1, x0, y0, y1, ty, y1 - y0), 1)[ver]))
    return rows.reshape(-1, 6), int(part.sum() - hor.sum() - ver.sum())


def _overlap_cov(A, B, tol, match_type):
    """cov(A | B) by interval algebra: per line a, the dilated intervals of its matching lines sorted, merged, clipped to a."""
    total = 0
    for g, c, lo, hi, ty, _ in A.tolist():
        m = (B[:, 0] == g) & (np.abs(B[:, 1] - c) <= tol)
        if match_type:
            m &= B[:, 4] == ty
        spans = sorted(zip((B[m, 2] - tol).tolist(), (B[m, 3] + tol).tolist()))
        merged = []
        for s, e in spans:
            if merged and s <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], e)
            else:
                merged.append([s, e])
        total += sum(max(0, min(e, hi) - max(s, lo)) for s, e in merged)
    return total


def line_overlap_counts(a, b, *, end_token, num_bits, tol=1, types="ignore"):
    """The reprojection counts of ONE pair of line drawings on the host (``ops.line_overlap`` is the device
    entry and computes the same integers).  ``a`` (the given drawing) and ``b`` (the rendering) are ``(value, view[, type])``
    rows of the batch contract (``input_value`` / ``input_view`` / ``input_type`` of one drawing; line drawings only - the
    tokens of a sideface input are faces, not lines).  A row holds (index of its first END, or its width) // 4 lines; a line
    is kept if its four tokens are coordinates of ``num_bits`` bits, its view is 0, 1 or 2 and it is horizontal or vertical
    with a positive length, and skipped otherwise.  A kept line b matches a kept line a of the other side at equal view and
    orientation, ``|c_b - c_a| <= tol`` and - ``types='match'`` - equal type; covered(a) is the length of a inside the union of
    its matching lines, each dilated by ``tol`` at both ends.  ``types='visible'``: only the type-0 lines of ``b`` take part.
    Returns int32 [8]: cov(A|B), len(A), cov(B|A), len(B), kept_A, kept_B, skipped_A, skipped_B."""
    if types not in OVERLAP_MODES:
        raise ValueError(f"types must be one of {OVERLAP_MODES}, not {types!r}")
    tol = int(tol)
    if not 0 <= tol <= 255:
        raise ValueError(f"tol must be in 0 .. 255, not {tol}")
    if types == "match" and (len(a) < 3 or a[2] is None or len(b) < 3 or b[2] is None):
        raise ValueError("types='match' needs a type row on both sides")
    A, skip_a = _overlap_lines(a, end_token, num_bits, types == "match", False)
    B, skip_b = _overlap_lines(b, end_token, num_bits, types != "ignore", types == "visible")
    m = types == "match"
    return np.asarray([_overlap_cov(A, B, tol, m), A[:, 5].sum(), _overlap_cov(B, A, tol, m), B[:, 5].sum(), len(A), len(B),
                       skip_a, skip_b], dtype=np.int32)


def overlap_scores(counts):
    """recall, precision, F1 of integer [..., 8] reprojection counts (a tensor on any device) in float64, each operation rounded
    on its own: recall = cov(A|B) / len(A), precision = cov(B|A) / len(B), f1 = 2 p r / (p + r), each 0 where its denominator
    is 0.  The divisors are tensors: torch divides by a host scalar as a multiplication by its reciprocal."""
    c = counts.to(torch.float64)
    one = torch.ones((), dtype=torch.float64, device=c.device)
    zero = torch.zeros((), dtype=torch.float64, device=c.device)
    rec = torch.where(c[..., 1] > 0, c[..., 0] / torch.where(c[..., 1] > 0, c[..., 1], one), zero)
    prec = torch.where(c[..., 3] > 0, c[..., 2] / torch.where(c[..., 3] > 0, c[..., 3], one), zero)
    den = prec + rec
    f1 = torch.where(den > 0, ((2.0 * prec) * rec) / torch.where(den > 0, den, one), zero)
    return rec, prec, f1


def _solid_boxes(row, end_token):
    """One token row -> its solid planks int64 [k, 6]: cut at the first END, plank 0 dropped, tokens clamped to the int16 range,
    planks with a zero or negative extent on any axis dropped."""
    if row is None:
        return np.zeros((0, 6), dtype=np.int64)
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    hits = np.nonzero(row == end_token)[0]
    planks = (int(hits[0]) if len(hits) else len(row)) // 6
    boxes = np.clip(row[:6 * planks].reshape(planks, 6)[1:], -32768, 32767)
    return boxes[np.all(boxes[:, 3:] - boxes[:, :3] > 0, axis=1)]


def _union_volume(boxes):
    """The volume of a union of half-open integer boxes [k, 6], by coordinate compression: per slab of x between consecutive
    bounds, the boxes that span it are painted into a grid over the compressed y and z bounds."""
    if len(boxes) == 0:
        return 0
    total = 0
    xs = np.unique(boxes[:, [0, 3]])
    for x0, x1 in zip(xs[:-1].tolist(), xs[1:].tolist()):
        live = boxes[(boxes[:, 0] <= x0) & (boxes[:, 3] >= x1)]
        if len(live) == 0:
            continue
        ys, zs = np.unique(live[:, [1, 4]]), np.unique(live[:, [2, 5]])
        grid = np.zeros((len(ys) - 1, len(zs) - 1), dtype=bool)
        for j0, j1, k0, k1 in zip(np.searchsorted(ys, live[:, 1]).tolist(), np.searchsorted(ys, live[:, 4]).tolist(),
                                  np.searchsorted(zs, live[:, 2]).tolist(), np.searchsorted(zs, live[:, 5]).tolist()):
            grid[j0:j1, k0:k1] = True
        total += (x1 - x0) * int(np.diff(ys) @ grid.astype(np.int64) @ np.diff(zs))
    return total


def plank_volume_counts(a, b, end_token):
    """The assembly-volume counts of ONE pair of token rows on the host (``ops.plank_volume`` is the device
    entry and computes the same integers).  A row is read as ``plank_match`` reads it - cut at its first ``end_token``, L // 6
    planks, plank 0 dropped, tokens clamped to [-32768, 32767]; a plank is solid if hi - lo > 0 on all three axes and occupies
    [lo, hi) on each, any other plank occupies nothing and is not counted.  ``b`` may be None (an empty side).  Returns int64
    [8]: union_a, sum_a, union_b, sum_b, inter, union_ab, n_a, n_b - the volumes of the unions of each side's solid planks, the
    sums of the planks' own volumes, the volume both unions share, the volume of both together, the solid planks."""
    A, B = _solid_boxes(a, end_token), _solid_boxes(b, end_token)
    ua, ub, uab = _union_volume(A), _union_volume(B), _union_volume(np.concatenate((A, B)))
    own = lambda X: int(np.prod(X[:, 3:] - X[:, :3], axis=1).sum())
    return np.asarray([ua, own(A), ub, own(B), ua + ub - uab, uab, len(A), len(B)], dtype=np.int64)


def volume_scores(counts):
    """The scores of integer [..., 8] assembly-volume counts (a tensor on any device, or numpy -> numpy) in float64, each ONE
    division of two exactly converted integers and 0 where its denominator is 0: ``volume_iou`` = inter / union_ab,
    ``volume_recall`` = inter / union_a (side a is the ground truth), ``volume_precision`` = inter / union_b, ``self_overlap_a`` =
    (sum_a - union_a) / sum_a and ``self_overlap_b`` alike.  The divisors are tensors: torch divides by a host scalar as a
    multiplication by its reciprocal."""
    if not torch.is_tensor(counts):
        return {k: v.numpy() for k, v in volume_scores(torch.from_numpy(np.asarray(counts, dtype=np.int64))).items()}
    c = counts.to(torch.int64)
    one = torch.ones((), dtype=torch.float64, device=c.device)
    zero = torch.zeros((), dtype=torch.float64, device=c.device)

    def ratio(num, den):
        return torch.where(den > 0, num.to(torch.float64) / torch.where(den > 0, den.to(torch.float64), one), zero)

    return {"volume_iou": ratio(c[..., 4], c[..., 5]), "volume_recall": ratio(c[..., 4], c[..., 0]),
            "volume_precision": ratio(c[..., 4], c[..., 2]), "self_overlap_a": ratio(c[..., 1] - c[..., 0], c[..., 1]),
            "self_overlap_b": ratio(c[..., 3] - c[..., 2], c[..., 3])}
