"""The assembly volume restated twice, independently of plankassembly_amd, and the cases the tests share.

`volume_counts` is the numpy restatement for any int64 tokens: clamp, coordinate compression, one boolean cell per compressed
cell.  `voxel_counts` is the oracle it is pinned to: a boolean [2^bits]^3 grid of unit cells filled box by box, for tokens
inside [0, 2^bits) only - no compression, no sorting, nothing shared with the restatement but the way a row is cut into planks.
Both return int64 [P, 8] = union_a, sum_a, union_b, sum_b, inter, union_ab, n_a, n_b."""
import numpy as np

END, PAD = 512, 513
LO, HI = -32768, 32767


def planks_of(row, end_token):
    """A token row -> int64 [k, 6]: cut at the first END (the whole row without one), L // 6 planks, plank 0 dropped."""
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    cut = len(row)
    for i, t in enumerate(row.tolist()):
        if t == end_token:
            cut = i
            break
    k = cut // 6
    return row[:6 * k].reshape(k, 6)[1:]


def solid(planks):
    p = np.clip(planks, LO, HI)
    keep = (p[:, 3] > p[:, 0]) & (p[:, 4] > p[:, 1]) & (p[:, 5] > p[:, 2])
    return p[keep]


def _compressed_union(boxes_list):
    """Volumes of the unions of several box sets over ONE compressed grid: [len(boxes_list)] python ints."""
    every = np.concatenate(boxes_list) if boxes_list else np.zeros((0, 6), dtype=np.int64)
    if len(every) == 0:
        return [0] * len(boxes_list)
    axes = [np.unique(every[:, [d, d + 3]]) for d in range(3)]
    widths = [np.diff(ax) for ax in axes]
    cell = widths[0][:, None, None] * widths[1][None, :, None] * widths[2][None, None, :]
    out = []
    for boxes in boxes_list:
        grid = np.zeros(cell.shape, dtype=bool)
        for b in boxes:
            i0, i1 = np.searchsorted(axes[0], b[0]), np.searchsorted(axes[0], b[3])
            j0, j1 = np.searchsorted(axes[1], b[1]), np.searchsorted(axes[1], b[4])
            k0, k1 = np.searchsorted(axes[2], b[2]), np.searchsorted(axes[2], b[5])
            grid[i0:i1, j0:j1, k0:k1] = True
        out.append(int(cell[grid].sum()))
    return out


def _own(boxes):
    return int(sum(int(b[3] - b[0]) * int(b[4] - b[1]) * int(b[5] - b[2]) for b in boxes))


def _pairs(a, b, pairs):
    if pairs is None:
        assert b is None or len(a) == len(b)
        return [(i, i) for i in range(len(a))]
    return [(int(i), int(j)) for i, j in pairs]


def volume_counts(a, b, pairs=None, end_token=END):
    """The restatement.  `a`, `b`: sequences of token rows (b None: every b side is empty); `pairs` None (rows i and i) or (i, j)."""
    out = []
    for i, j in _pairs(a, b, pairs):
        A = solid(planks_of(a[i], end_token))
        B = solid(planks_of(b[j], end_token)) if b is not None else np.zeros((0, 6), dtype=np.int64)
        ua, ub, uab = _compressed_union([A, B, np.concatenate((A, B))])
        out.append([ua, _own(A), ub, _own(B), ua + ub - uab, uab, len(A), len(B)])
    return np.asarray(out, dtype=np.int64).reshape(-1, 8)


def voxel_counts(a, b, pairs=None, end_token=END, bits=5):
    """The oracle: unit cells.  Every token of a plank that is read must lie in [0, 2^bits)."""
    n = 1 << bits
    out = []
    for i, j in _pairs(a, b, pairs):
        grids, sums, counts = [], [], []
        for row in (a[i], b[j] if b is not None else None):
            g = np.zeros((n, n, n), dtype=bool)
            total = k = 0
            for p in (planks_of(row, end_token).tolist() if row is not None else []):
                assert all(0 <= t < n for t in p), "the voxel oracle reads coordinates of the grid only"
                x0, y0, z0, x1, y1, z1 = p
                if x1 > x0 and y1 > y0 and z1 > z0:
                    g[x0:x1, y0:y1, z0:z1] = True
                    total += (x1 - x0) * (y1 - y0) * (z1 - z0)
                    k += 1
            grids.append(g); sums.append(total); counts.append(k)
        out.append([int(grids[0].sum()), sums[0], int(grids[1].sum()), sums[1], int((grids[0] & grids[1]).sum()),
                    int((grids[0] | grids[1]).sum()), counts[0], counts[1]])
    return np.asarray(out, dtype=np.int64).reshape(-1, 8)


def scores(counts):
    """The five float64 scores of int64 [..., 8] counts in numpy: one division each, 0 at a zero denominator."""
    c = np.asarray(counts, dtype=np.int64)

    def ratio(num, den):
        out = np.zeros(den.shape, dtype=np.float64)
        np.divide(num.astype(np.float64), den.astype(np.float64), out=out, where=den > 0)
        return out

    return {"volume_iou": ratio(c[..., 4], c[..., 5]), "volume_recall": ratio(c[..., 4], c[..., 0]),
            "volume_precision": ratio(c[..., 4], c[..., 2]), "self_overlap_a": ratio(c[..., 1] - c[..., 0], c[..., 1]),
            "self_overlap_b": ratio(c[..., 3] - c[..., 2], c[..., 3])}


def select(counts, N):
    """volume_index [B], utility / 2^40 / max(N - 1, 1) [B, N] from int64 [B, N (N - 1) / 2, 8] counts of the pairs n < m in
    row-major order - in python integers."""
    counts = np.asarray(counts, dtype=np.int64)
    iou = scores(counts)["volume_iou"]
    index, mean = [], []
    for b in range(counts.shape[0]):
        util = [0] * N
        k = 0
        for n in range(N):
            for m in range(n + 1, N):
                q = int(np.rint(iou[b, k] * 2.0 ** 40))
                util[n] += q; util[m] += q
                k += 1
        index.append(util.index(max(util)))
        mean.append([u / 2.0 ** 40 / max(N - 1, 1) for u in util])
    return np.asarray(index, dtype=np.int64), np.asarray(mean, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------- the cases
def row_of(planks, length, end=True, plank0=(0, 0, 0, 31, 31, 31)):
    """plank 0, the planks, then END and PAD - or, without END, zeros: planks that occupy nothing, up to the row's end."""
    toks = list(plank0) + [int(t) for p in planks for t in p]
    assert len(toks) <= length
    if end and len(toks) < length:
        toks.append(END)
    return np.asarray(toks + [PAD if end else 0] * (length - len(toks)), dtype=np.int64)


def random_box(rng, size, lo_size, hi_size):
    ext = rng.integers(lo_size, hi_size + 1, 3)
    lo = np.asarray([rng.integers(0, size - e + 1) for e in ext])
    return np.concatenate((lo, lo + ext))


def random_planks(rng, k, size=31, lo_size=1, hi_size=12, odd=0.15):
    """k planks with every coordinate in [0, size]; a share `odd` of them inverted on one axis or with a zero extent (they occupy nothing)."""
    out = []
    for _ in range(k):
        b = random_box(rng, size, lo_size, hi_size)
        u = rng.random()
        if u < odd / 2:
            d = int(rng.integers(0, 3)); b[d], b[d + 3] = b[d + 3], b[d]
        elif u < odd:
            d = int(rng.integers(0, 3)); b[d + 3] = b[d]
        out.append(b)
    return out


def case_table(seed=20, n=48, length=132):
    """n random pairs of rows of `length` tokens, at most 8 planks a side, every coordinate in [0, 32): rows a [n, length],
    rows b [n, length].  A quarter of the pairs are sparse (few small planks), so some sides do not meet."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for i in range(n):
        sparse = i % 4 == 3
        for rows in (a, b):
            k = int(rng.integers(1, 4)) if sparse else int(rng.integers(0, 9))
            planks = random_planks(rng, k, hi_size=5 if sparse else 16)
            rows.append(row_of(planks, length, end=bool(rng.random() < 0.8)))
    return np.stack(a), np.stack(b)


def cube(x, y, z, e=1):
    return (x, y, z, x + e, y + e, z + e)


def hand_cases():
    """(name, row a, row b or None, the eight integers) - answers worked out by hand."""
    L = 36
    r = lambda *p, **kw: row_of(p, kw.pop("length", L), **kw)
    out = [
        ("face_sharing_unit_cubes", r(cube(3, 3, 3)), r(cube(4, 3, 3)), [1, 1, 1, 1, 0, 2, 1, 1]),
        ("nested", r((0, 0, 0, 10, 10, 10)), r((2, 2, 2, 4, 5, 6)), [1000, 1000, 24, 24, 24, 1000, 1, 1]),
        ("identical_sides", r((1, 2, 3, 5, 7, 9), cube(20, 20, 20, 2)), r((1, 2, 3, 5, 7, 9), cube(20, 20, 20, 2)),
         [128, 128, 128, 128, 128, 128, 2, 2]),
        ("same_plank_twice", r((1, 1, 1, 4, 5, 6), (1, 1, 1, 4, 5, 6)), None, [60, 120, 0, 0, 0, 60, 2, 0]),
        ("inverted_and_zero_extent", r((5, 5, 5, 2, 9, 9), (1, 1, 1, 1, 4, 4), cube(0, 0, 0, 2)), r((3, 3, 3, 3, 3, 3)),
         [8, 8, 0, 0, 0, 8, 1, 0]),
        ("empty_side_a", r(), r(cube(1, 1, 1, 3)), [0, 0, 27, 27, 0, 27, 0, 1]),
        ("both_empty", r(), r(), [0, 0, 0, 0, 0, 0, 0, 0]),
        ("partial_overlap", r((0, 0, 0, 4, 4, 4)), r((2, 2, 2, 6, 6, 6)), [64, 64, 64, 64, 8, 120, 1, 1]),
        ("clamped_at_2_40", r((-2 ** 40, 0, 0, 2 ** 40, 1, 1)), r((-2 ** 40, 0, 0, 0, 1, 2 ** 40)),
         [65535, 65535, 32768 * 32767, 32768 * 32767, 32768, 65535 + 32768 * 32767 - 32768, 1, 1]),
    ]
    # END at 0, 5, 6, 11, 12 and absent: two planks behind plank 0 in a row of 18 tokens, END written over token `at`
    base = np.asarray([0] * 6 + list(cube(1, 1, 1, 2)) + list(cube(10, 10, 10, 3)), dtype=np.int64)
    for at, planks in ((0, 0), (5, 0), (6, 0), (11, 0), (12, 1), (None, 2)):
        row = base.copy()
        if at is not None:
            row[at] = END
        vol = [0, 8, 35][planks]
        out.append((f"end_at_{at}", row, row.copy(), [vol, vol, vol, vol, vol, vol, planks, planks]))
    return out


def dense_rows(seed, k, size, length, lo_size=1, hi_size=24):
    """One row of k solid random planks in [0, size) and `length` tokens, no END where the planks fill it."""
    rng = np.random.default_rng(seed)
    return row_of([random_box(rng, size, lo_size, hi_size) for _ in range(k)], length)


def disjoint_row(k, length, step=4, per=6, shift=0):
    """k planks of 3 x 3 x 2 on a lattice of `step`: no two of them meet."""
    planks = []
    for i in range(k):
        x, y, z = (i % per) * step + shift, (i // per % per) * step, (i // (per * per)) * step
        planks.append((x, y, z, x + 3, y + 3, z + 2))
    return row_of(planks, length)


def ceiling_pairs(length=1026, k=170):
    """The four pairs at the LDS ceiling: dense random, all disjoint, all identical, a against an empty b."""
    a = [dense_rows(1, k, 64, length), disjoint_row(k, length), row_of([(3, 4, 5, 40, 41, 42)] * k, length), dense_rows(2, k, 160, length)]
    b = [dense_rows(3, k, 64, length), disjoint_row(k, length, shift=1), row_of([(3, 4, 5, 40, 41, 42)] * k, length), row_of([], length)]
    return np.stack(a), np.stack(b)
