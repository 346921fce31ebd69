"""Numpy restatement of pa_sequence_batch (include/plank_hip.h; csrc/seqtrain.hip): arrays in, expected arrays
out, the kernel's operation order in float64 with float32 roundings where the header states them.  The reward is
metric.prf_from_counts itself."""
import numpy as np

from plankassembly_amd.metric import prf_from_counts

VOCAB, END, PAD = 514, 512, 513
OBJECTIVES = ("reinforce", "risk")
BASELINES = ("none", "mean", "greedy")


def rewards(counts):
    """F1 f32 [rows] of count rows [rows, 4] (tp, n_a = predicted planks, n_b = ground-truth planks, ties: not used)."""
    c = np.asarray(counts).reshape(-1, 4)
    return prf_from_counts(c[:, 0], c[:, 1], c[:, 2])[2].numpy()


def reinforce_weights(r, baseline, base=None):
    """r f32 [N] -> f32 [N]: w_n = (r_n - b_n) / N in float64, rounded once.  ``base``: the greedy F1 (f32) of the drawing."""
    r = np.asarray(r, dtype=np.float32)
    N = len(r)
    out = np.empty(N, dtype=np.float32)
    for n in range(N):
        b = np.float64(0.0)
        if baseline == "mean":
            s = np.float64(0.0)
            for m in range(N):                                   # m ascending, n skipped
                if m != n:
                    s = s + np.float64(r[m])
            b = s / np.float64(N - 1)
        elif baseline == "greedy":
            b = np.float64(np.float32(base))
        out[n] = np.float32((np.float64(r[n]) - b) / np.float64(N))
    return out


def risk_weights64(r, scores, alpha):
    """w_n = (alpha q_n) A_n, A_n = sum_m q_m (r_n - r_m), in float64 in the header's order, before the single rounding."""
    r = np.asarray(r, dtype=np.float32).astype(np.float64)
    a = np.float64(np.float32(alpha))
    s = a * np.asarray(scores, dtype=np.float32).astype(np.float64)
    N = len(s)
    mx = s[0]
    for m in range(1, N):
        mx = s[m] if s[m] > mx else mx
    e = np.exp(s - mx)
    z = np.float64(0.0)
    for m in range(N):
        z = z + e[m]
    q = e / z
    w = np.empty(N, dtype=np.float64)
    for n in range(N):
        adv = np.float64(0.0)
        for m in range(N):
            adv = adv + q[m] * (r[n] - r[m])
        w[n] = (a * q[n]) * adv
    return w


def risk_weights(r, scores, alpha):
    return risk_weights64(r, scores, alpha).astype(np.float32)


def sample_row(tokens, attach, first_end, Tmax, T, vocab=VOCAB, pad=PAD):
    """One sample -> (value int64 [T], label int64 [T], mask uint8 [T])."""
    tokens, attach = np.asarray(tokens, dtype=np.int64), np.asarray(attach, dtype=np.int64)
    L = min(int(first_end) + 1 if first_end >= 0 else Tmax, Tmax)
    value = np.full(T, pad, dtype=np.int64)
    label = np.full(T, pad, dtype=np.int64)
    mask = np.ones(T, dtype=np.uint8)
    value[:L] = tokens[:L]
    label[:L] = np.where(attach[:L] >= 0, vocab + attach[:L], tokens[:L])
    mask[:L] = 0
    return value, label, mask


def sequence_batch(tokens, attach, first_end, scores, counts, gt_value, gt_label, N, objective="reinforce", baseline="mean", alpha=1.0,
                   nll_weight=0.0, base_counts=None, vocab=VOCAB, pad=PAD):
    """tokens / attach int64 [B*N, Tmax], first_end int32 [B*N], scores f32 [B*N], counts int32 [B*N, 4], base_counts int32 [B, 4] or
    None, gt_value / gt_label int64 [B, T] -> dict of out_value / out_label int64 [B*G, T], out_mask uint8 [B*G, T], out_weight f32
    [B*G], reward f32 [B, N]."""
    tokens, attach = np.asarray(tokens), np.asarray(attach)
    gt_value, gt_label = np.asarray(gt_value, dtype=np.int64), np.asarray(gt_label, dtype=np.int64)
    B, T = gt_value.shape
    Tmax = tokens.shape[1]
    assert tokens.shape[0] == B * N and Tmax <= T and objective in OBJECTIVES and baseline in BASELINES
    G = N + (1 if np.float32(nll_weight) != 0 else 0)
    reward = rewards(counts).reshape(B, N)
    base = rewards(base_counts) if base_counts is not None else None
    value = np.empty((B * G, T), dtype=np.int64)
    label = np.empty((B * G, T), dtype=np.int64)
    mask = np.empty((B * G, T), dtype=np.uint8)
    weight = np.empty(B * G, dtype=np.float32)
    for b in range(B):
        if objective == "reinforce":
            w = reinforce_weights(reward[b], baseline, None if base is None else base[b])
        else:
            w = risk_weights(reward[b], np.asarray(scores)[b * N:(b + 1) * N], alpha)
        for n in range(N):
            value[b * G + n], label[b * G + n], mask[b * G + n] = sample_row(tokens[b * N + n], attach[b * N + n],
                                                                             int(np.asarray(first_end)[b * N + n]), Tmax, T, vocab, pad)
        weight[b * G:b * G + N] = w
        if G > N:
            value[b * G + N], label[b * G + N] = gt_value[b], gt_label[b]
            mask[b * G + N] = gt_value[b] == pad
            weight[b * G + N] = np.float32(nll_weight)
    return {"out_value": value, "out_label": label, "out_mask": mask, "out_weight": weight, "reward": reward}


# ------------------------------------------------------------------------------------------------ synthetic inputs
def synthetic(B, N, Tmax, T, seed, equal_drawing=None):
    """Decoder-shaped inputs for the kernel tests: rows with first_end -1, END at 0, END at Tmax - 1 and pointers; counts with
    n_a == 0, n_b == 0, ties > 0; ``equal_drawing``: a drawing whose samples all carry the same counts."""
    rng = np.random.default_rng(seed)
    rows = B * N
    tokens = rng.integers(0, 512, size=(rows, Tmax)).astype(np.int64)
    attach = np.where(rng.random((rows, Tmax)) < 0.3, rng.integers(0, max(Tmax - 1, 1), size=(rows, Tmax)), -1).astype(np.int64)
    first_end = rng.integers(-1, Tmax, size=rows).astype(np.int32)
    first_end[0] = -1
    if rows > 1:
        first_end[1] = 0
    if rows > 2:
        first_end[2] = Tmax - 1
    for r in range(rows):
        if first_end[r] >= 0:
            tokens[r, first_end[r]], attach[r, first_end[r]] = END, -1
            tokens[r, first_end[r] + 1:], attach[r, first_end[r] + 1:] = PAD, -1
            if first_end[r] >= 1:
                attach[r, first_end[r] - 1] = max(first_end[r] - 2, 0)           # a pointer at the last live position before END
    n_a = rng.integers(0, 9, size=rows)
    n_b = np.repeat(rng.integers(0, 9, size=B), N)
    tp = np.array([rng.integers(0, min(a, b) + 1) for a, b in zip(n_a, n_b)])
    ties = rng.integers(0, 3, size=rows)
    counts = np.stack([tp, n_a, n_b, ties], 1).astype(np.int32)
    counts[0] = (0, 0, counts[0, 2], 1)                                          # n_a == 0, ties > 0
    if B > 1:
        counts[N:2 * N, 2] = 0                                                   # a drawing without ground-truth planks: n_b == 0
        counts[N:2 * N, 0] = 0
    if equal_drawing is not None:
        counts[equal_drawing * N:(equal_drawing + 1) * N] = (2, 3, 4, 0)
    scores = (-rng.random(rows) * 40.0).astype(np.float32)
    nb = rng.integers(1, 9, size=B)
    base_counts = np.stack([rng.integers(0, nb + 1), nb, np.maximum(n_b[::N], 1), np.zeros(B, dtype=np.int64)], 1).astype(np.int32)
    base_counts[:, 0] = np.minimum(base_counts[:, 0], base_counts[:, 2])
    gt_value = rng.integers(0, 512, size=(B, T)).astype(np.int64)
    gt_label = gt_value.copy()
    for b in range(B):
        e = int(rng.integers(1, T))
        gt_value[b, e], gt_label[b, e] = END, END
        gt_value[b, e + 1:], gt_label[b, e + 1:] = PAD, PAD
        if e > 7:
            gt_label[b, 7] = VOCAB + 1
    return dict(tokens=tokens, attach=attach, first_end=first_end, scores=scores, counts=counts, base_counts=base_counts,
                gt_value=gt_value, gt_label=gt_label)
