"""Restatement of the plank-matching kernel (csrc/match.hip, csrc/match_core.h) in plain numpy and Python
integers: parse, filter, integer IoU, the double comparison, tp by a simple augmenting-path matcher, ties, and the consensus
utility.  The oracle of the GPU tests; tests/test_match_cpu.py pins it to metric.HungarianMatcher."""
import numpy as np

DOF = 6
COORD_MIN, COORD_MAX = -32768, 32767
END = 512


def parse_row(row, end_token, filter_zero):
    """Token row -> the kept planks [n, 6] (Python ints in an int64 array): up to the first END, whole planks only, plank 0
    dropped, zero-extent planks dropped when ``filter_zero``; coordinates clamped as the kernel holds them."""
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    hits = np.nonzero(row == end_token)[0]
    L = int(hits[0]) if len(hits) else len(row)
    planks = np.clip(row[: L // DOF * DOF], COORD_MIN, COORD_MAX).reshape(-1, DOF)[1:]
    if filter_zero and len(planks):
        planks = planks[np.all(planks[:, 3:] - planks[:, :3] != 0, axis=1)]
    return planks


def iou_decision(a, b, threshold):
    """(iou > threshold, iou >= threshold and not iou > threshold) for two planks, the integers exact, one double division."""
    inter = 1
    for d in range(3):
        inter *= max(0, min(int(a[d + 3]), int(b[d + 3])) - max(int(a[d]), int(b[d])))
    iou = 0.0
    if inter > 0:
        va = (int(a[3]) - int(a[0])) * (int(a[4]) - int(a[1])) * (int(a[5]) - int(a[2]))
        vb = (int(b[3]) - int(b[0])) * (int(b[4]) - int(b[1])) * (int(b[5]) - int(b[2]))
        iou = float(inter) / float(va + vb - inter)
    gt = iou > threshold
    return gt, (iou >= threshold) and not gt


def adjacency(pa, pb, threshold):
    edges = [[False] * len(pb) for _ in pa]
    ties = 0
    for i, a in enumerate(pa):
        for j, b in enumerate(pb):
            gt, tie = iou_decision(a, b, threshold)
            edges[i][j] = gt
            ties += int(tie)
    return edges, ties


def max_matching(edges, nb):
    """Kuhn's algorithm, the textbook form (one augmenting search per plank of a) without recursion."""
    match_b = [-1] * nb
    size = 0
    for u in range(len(edges)):
        seen = [False] * nb
        parent = {}                                    # plank of b -> the plank of a that reached for it
        queue, found = [u], -1
        while queue and found < 0:                     # breadth first: the matching size does not depend on the search order
            a = queue.pop(0)
            for j in range(nb):
                if edges[a][j] and not seen[j]:
                    seen[j] = True
                    parent[j] = a
                    if match_b[j] < 0:
                        found = j
                        break
                    queue.append(match_b[j])
        if found < 0:
            continue
        j = found
        while True:                                    # flip the path back to u
            a = parent[j]
            prev = next((k for k in range(nb) if match_b[k] == a), -1)
            match_b[j] = a
            if a == u:
                break
            j = prev
        size += 1
    return size


def greedy_matching(edges, nb):
    """Index-order greedy (no augmenting): what a matcher without the search would give."""
    used, size = [False] * nb, 0
    for row in edges:
        for j in range(nb):
            if row[j] and not used[j]:
                used[j] = True
                size += 1
                break
    return size


def match_rows(row_a, row_b, end_token=END, filter_a=True, filter_b=False, threshold=0.5):
    """The kernel's four integers for one pair of rows: (tp, n_a, n_b, ties)."""
    pa, pb = parse_row(row_a, end_token, filter_a), parse_row(row_b, end_token, filter_b)
    edges, ties = adjacency(pa, pb, threshold)
    return max_matching(edges, len(pb)), len(pa), len(pb), ties


def plank_match(seq_a, seq_b, pairs=None, end_token=END, filter_a=True, filter_b=False, threshold=0.5):
    """ops.plank_match restated: int32 [n, 4]."""
    seq_a, seq_b = np.asarray(seq_a), np.asarray(seq_b)
    if pairs is None:
        assert len(seq_a) == len(seq_b)
        pairs = [(i, i) for i in range(len(seq_a))]
    out = [match_rows(seq_a[i], seq_b[j], end_token, filter_a, filter_b, threshold) for i, j in pairs]
    return np.asarray(out, dtype=np.int32).reshape(-1, 4)


def consensus(sample_tokens, end_token=END, threshold=0.5):
    """Minimum-Bayes-risk choice among the N samples of every drawing: u_q [B][N] Python ints (sum over m != n of
    round_half_even(F1(n, m) * 2^40), F1 = 2 tp / (n_a + n_b) in float64, 0 where tp == 0, ties no edges, both sides
    filtered), index [B] (the largest utility, the lowest n among equals) and consensus_f1 [B][N] float64."""
    st = np.asarray(sample_tokens)
    B, N = st.shape[:2]
    uq, index, f1 = [], [], []
    for b in range(B):
        u = [0] * N
        for n in range(N):
            for m in range(n + 1, N):
                tp, na, nb, _ = match_rows(st[b, n], st[b, m], end_token, True, True, threshold)
                q = round((2 * tp) / (na + nb) * 2.0 ** 40) if tp > 0 else 0      # Python's round: half to even, like llrint
                u[n] += q
                u[m] += q
        uq.append(u)
        index.append(max(range(N), key=lambda n: (u[n], -n)))
        f1.append([float(x) / 2.0 ** 40 / max(N - 1, 1) for x in u])
    return uq, index, np.asarray(f1, dtype=np.float64).reshape(B, N)


# ---------------------------------------------------------------------------------------------------- case builders
def row_of(planks, length, end_token=END, pad_token=513, bbox=(0, 0, 0, 1, 1, 1), end=True):
    """A token row: the bounding-box plank, the planks, END (when it fits and ``end``), PAD."""
    toks = list(bbox) + [int(v) for p in planks for v in p]
    if end and len(toks) < length:
        toks.append(end_token)
    assert len(toks) <= length, (len(toks), length)
    return np.asarray(toks + [pad_token] * (length - len(toks)), dtype=np.int64)


def random_planks(rng, n, grid=8, jitter=True, size=64):
    """Integer boxes on a ``grid`` lattice (so that exact overlaps and exact halves occur), some jittered by one."""
    lo = rng.integers(0, size // grid, size=(n, 3)) * grid
    ext = rng.integers(1, 4, size=(n, 3)) * grid
    box = np.concatenate([lo, lo + ext], axis=1).astype(np.int64)
    if jitter and n:
        box += (rng.random((n, 6)) < 0.15) * rng.integers(-1, 2, size=(n, 6))
    return box


def random_pair(rng, max_planks=20, share=0.6):
    """A prediction / truth pair: the truth's planks, some of them copied or shifted into the prediction."""
    nb = int(rng.integers(0, max_planks + 1))
    gt = random_planks(rng, nb, jitter=False)
    na = int(rng.integers(0, max_planks + 1))
    pred = random_planks(rng, na)
    for i in range(na):
        if nb and rng.random() < share:
            src = gt[rng.integers(0, nb)].copy()
            if rng.random() < 0.5:
                src[rng.integers(0, 3)] += 8 * int(rng.integers(-1, 2))      # one face moved by a lattice step: exact fractions
            pred[i] = src
    return pred, gt


def chain_case(k, shift, tail=True):
    """The chain family at threshold 0.25, from the one-dimensional example a = [4, 14] against b = [0, 10], [10, 20] (overlap 6
    of union 14 = 0.43, overlap 4 of union 16 = 0.25 exactly) extended to three dimensions with equal extents.  Side b: k + 1 cubes
    of edge 10 in a row along x, b_j = [10 j, 10 j + 10].  Side a: a_i = b_i moved by ``shift`` along x for i < k, then - ``tail`` -
    one more cube equal to b_0.
      shift 4: a_i has an edge to b_i (0.43) and a TIE with b_{i+1} (0.25, no edge); the tail cube competes with a_0 for b_0 and
               loses: maximum = greedy = k.
      shift 5: a_i has edges to b_i and b_{i+1} (5 / 15 = 0.33 each).  Index-order greedy gives a_i -> b_i and leaves the tail
               cube out (k); the maximum moves the whole chain up by one (k + 1): an augmenting path through all 2 k + 1 edges.
      shift 6: the mirror of 4: a tie with b_i, an edge to b_{i+1}; greedy = maximum = k + 1."""
    b = [(10 * j, 0, 0, 10 * j + 10, 10, 10) for j in range(k + 1)]
    a = [(10 * i + shift, 0, 0, 10 * i + shift + 10, 10, 10) for i in range(k)]
    if tail:
        a.append(b[0])
    return np.asarray(a, dtype=np.int64).reshape(-1, 6), np.asarray(b, dtype=np.int64).reshape(-1, 6)


def rows_of(plank_sets, length, **kw):
    return np.stack([row_of(p, length, **kw) for p in plank_sets])


def golden_cases(golden_dir):
    """The five matcher.npz cases as token rows (neither side filtered: the stored boxes went to the matcher as they are) and the
    six fixture_f1 drawings (decoded rows against ground-truth rows, the prediction side filtered).  -> [(name, case dict)]."""
    import os
    z = np.load(os.path.join(golden_dir, "matcher.npz"))
    n = int(z["n"])
    out = [("matcher", dict(seq_a=rows_of([z[f"pred{i}"] for i in range(n)], 64), seq_b=rows_of([z[f"gt{i}"] for i in range(n)], 64),
                            filter_a=False, filter_b=False, threshold=0.5))]
    f = np.load(os.path.join(golden_dir, "fixture_f1.npz"))
    out.append(("fixture_f1", dict(seq_a=f["samples"], seq_b=f["batch::output_value"], filter_a=True, filter_b=False, threshold=0.5)))
    return out


def edge_cases():
    """The rows at which the kernel can go wrong, as [(name, case dict)]; a case dict holds seq_a, seq_b and optionally pairs,
    filter_a, filter_b, threshold (defaults: identity pairs, True, False, 0.5)."""
    rng = np.random.default_rng(20)
    cases = []
    some = random_planks(rng, 5, jitter=False)
    cases.append(("empty_sides", dict(seq_a=rows_of([[], some, []], 64), seq_b=rows_of([some, [], []], 64))))
    # no END in a 128-token row: 21 planks with row 0, 20 kept, 2 trailing tokens ignored
    full = random_planks(rng, 20)
    a = np.concatenate([row_of(full, 126, end=False), [7, 9]]).astype(np.int64)
    b = np.concatenate([row_of(full[::-1], 126, end=False), [3, 4]]).astype(np.int64)
    cases.append(("no_end_128", dict(seq_a=a[None], seq_b=b[None])))
    e0 = np.full(64, 513, dtype=np.int64); e0[0] = END
    cases.append(("end_at_0", dict(seq_a=np.stack([e0, row_of(some, 64)]), seq_b=np.stack([row_of(some, 64), e0]))))
    mid = row_of(some, 64); mid[6 * 4 + 3] = END                                   # L = 6 k + 3: the cut plank is ignored
    cases.append(("end_mid_plank", dict(seq_a=np.stack([mid, row_of(some, 64)]), seq_b=np.stack([row_of(some, 64), mid]))))
    zero = some.copy(); zero[1, 3] = zero[1, 0]; zero[3, 5] = zero[3, 2]           # two planks with a zero extent
    cases.append(("zero_extent", dict(seq_a=rows_of([zero, zero], 64), seq_b=rows_of([zero, some], 64))))
    cases.append(("zero_extent_both", dict(seq_a=rows_of([zero], 64), seq_b=rows_of([zero], 64), filter_b=True)))
    inv = some.copy(); inv[0, [0, 3]] = inv[0, [3, 0]]; inv[2, [1, 4]] = inv[2, [4, 1]]      # hi < lo
    cases.append(("inverted", dict(seq_a=rows_of([inv, some, inv], 64), seq_b=rows_of([some, inv, inv], 64))))
    big = np.asarray([(500, 500, 500, 513, 513, 512), (0, 0, 0, 513, 512, 513), (256, 0, 0, 513, 513, 513)], dtype=np.int64)
    big_b = np.asarray([(500, 500, 500, 513, 513, 513), (0, 0, 0, 513, 513, 513)], dtype=np.int64)
    # 512 / 513 as coordinates: END is another token here, so the rows have none and their PAD tail parses as zero-extent planks
    cases.append(("tokens_512_513", dict(seq_a=rows_of([big, big_b], 64, end_token=-1, end=False),
                                         seq_b=rows_of([big_b, big], 64, end_token=-1, end=False), end_token=600)))
    cases.append(("tokens_512_is_end", dict(seq_a=rows_of([big], 64), seq_b=rows_of([big_b], 64))))
    wild = np.asarray([(-5, -(2 ** 40), 0, 2 ** 40, 7, 2 ** 62), (0, 0, 0, 40000, 40000, 40000), (1, 1, 1, 9, 9, 9)], dtype=np.int64)
    cases.append(("out_of_vocabulary", dict(seq_a=rows_of([wild, some], 64), seq_b=rows_of([wild[::-1], wild], 64))))
    sa, sb = [], []
    for k in (1, 2, 3, 5, 9):
        for shift in (4, 5, 6):
            for tail in (False, True):
                pa, pb = chain_case(k, shift, tail)
                sa.append(pa); sb.append(pb)
                sa.append(pa[::-1]); sb.append(pb)                                 # the tail cube first: another search order
    cases.append(("chain_025", dict(seq_a=rows_of(sa, 128), seq_b=rows_of(sb, 128), threshold=0.25)))
    base = random_planks(rng, 6, jitter=False)
    nested = np.concatenate([base, base, base + np.asarray([0, 0, 0, 8, 0, 0]), base[:3] + np.asarray([2, 2, 2, -2, -2, -2])])
    cases.append(("duplicated_nested_b", dict(seq_a=rows_of([base, np.concatenate([base, base[:2]])], 160),
                                              seq_b=rows_of([nested, nested], 160))))
    return cases


def large_cases():
    """65 x 65 (crosses the 64-bit word of an adjacency row) and 170 x 170 (the limit: len 1026, no END)."""
    rng = np.random.default_rng(65)
    out = []
    for n in (65, 170):
        a = random_planks(rng, n, size=96)
        b = a[rng.permutation(n)].copy()
        move = rng.random(n) < 0.5
        b[move] = random_planks(rng, int(move.sum()), size=96)
        length = 6 * (n + 1)
        out.append((f"{n}x{n}", dict(seq_a=rows_of([a, a], length, end=False), seq_b=rows_of([b, a[::-1]], length, end=False),
                                     filter_b=True)))
    # a long chain at the limit: 169 shifted cubes and the tail cube against 170 cubes - one augmenting path through every plank
    pa, pb = chain_case(169, 5, True)
    out.append(("chain_170", dict(seq_a=rows_of([pa], 1026, end=False), seq_b=rows_of([pb], 1026, end=False), threshold=0.25)))
    return out


def case_args(case):
    """A case dict -> (seq_a, seq_b, pairs, keyword arguments of plank_match)."""
    kw = dict(end_token=case.get("end_token", END), filter_a=case.get("filter_a", True), filter_b=case.get("filter_b", False),
              threshold=case.get("threshold", 0.5))
    return case["seq_a"], case["seq_b"], case.get("pairs"), kw
