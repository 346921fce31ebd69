// Assembly volume core: what one pair of token rows means as two solids - the unions of their planks - and
// the volumes of those unions, of their union and of the planks on their own, as exact integers on the token grid.  Every
// function here is plain integer C++ and compiles for the device (csrc/volume.hip, one block per pair) and for the host alone
// (tools/volume_host, the stand-alone program the sanitizer build runs).  tests/volume_reference.py holds the numpy restatement
// and the voxel oracle both are pinned to.
//
// A row is read as pa_plank_match reads it: cut at its first END, L / 6 planks, plank 0 dropped, every token clamped by
// pm_coord.  A plank is SOLID if hi - lo > 0 on all three axes and then occupies [lo, hi) on each; every other plank occupies
// nothing and is not counted.  Clamped coordinates fit int16, an extent is below 2^16, a plank volume below 2^48 and a sum over
// at most 170 planks below 2^56.
//
// The method: the solid planks of both sides form one box list in z_lo order (side b marked); the x bounds and the y bounds of
// all boxes are sorted (duplicates stay: a slab between equal bounds has no width and is skipped); every y slab has a bit row
// over the boxes that span it, an x slab's bit row is built when the slab is taken up (by every thread that shares the slab).
// A column (x slab i, y slab j) holds the boxes `rowx & rowy[j]`; visiting the set bits in ascending order is visiting them in
// z_lo order, so three running interval ends (side a, side b, either) give the covered z length of the column with one
// comparison each per box.
//
// No recursion, no local arrays: every array is handed in by the caller (LDS on the device).
#ifndef PLANK_VOLUME_CORE_H
#define PLANK_VOLUME_CORE_H

#include "match_core.h"

#define PV_THREADS 256                                     /* the kernel's block; the x-slab rows are laid out for it */
#define PV_BOX 8                                           /* int16 per box: x0 y0 z0 x1 y1 z1 side pad */
#define PV_MAX_BOXES (2 * PM_MAX_PLANKS)
#define PV_MAX_WORDS ((PV_MAX_BOXES + 63) / 64)
#define PV_OUT 8                                           /* union_a sum_a union_b sum_b inter union_ab n_a n_b */
#define PV_BELOW (-40000)                                  /* below every clamped coordinate */

PM_HD bool pv_solid(const int32_t* box) { return box[3] - box[0] > 0 && box[4] - box[1] > 0 && box[5] - box[2] > 0; }

PM_HD int64_t pv_volume(const int32_t* box) { return (int64_t)(box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2]); }

// Where everything of one pair lives, in bytes from a 16-byte aligned base: LDS on the device, one heap block on the host.
struct PvLayout {
    int cap;                   // boxes both sides can hold together after row 0 is dropped
    int words;                 // 64-bit words of one bit row over the boxes
    int bounds;                // 2 * cap: the bounds of one axis
    int rowy;                  // uint64 [max(bounds - 1, 1)][words]: the y slabs' bit rows
    int rowx;                  // uint64 [words][PV_THREADS]: one x slab's bit row per thread, word w of thread t at w * PV_THREADS + t
    int red;                   // int64 [PV_THREADS / 64][5]: the block reduction
    int cnt;                   // int32 [PV_THREADS / 64]: the compaction's wave counts
    int box;                   // int16 [cap][PV_BOX]: the boxes in z_lo order
    int tok;                   // int16 [len_a + len_b]: the clamped tokens of both rows
    int zkey;                  // int16 [cap]: z_lo of the compacted planks, before they are ordered
    int xs, ys;                // int16 [bounds] each: the sorted bounds
    int bytes;
};

PM_HD PvLayout pv_layout(int len_a, int len_b) {
    PvLayout l;
    l.cap = pm_cap(len_a) + pm_cap(len_b);
    l.words = (l.cap + 63) / 64; if (l.words < 1) l.words = 1;
    l.bounds = 2 * l.cap;
    const int cap1 = l.cap > 0 ? l.cap : 1;
    const int len = len_a + len_b > 0 ? len_a + len_b : 1;
    int at = 0;
    l.rowy = at; at += 8 * (l.bounds > 1 ? l.bounds - 1 : 1) * l.words;
    l.rowx = at; at += 8 * l.words * PV_THREADS;
    l.red = at; at += 8 * (PV_THREADS / 64) * 5;
    l.cnt = at; at += 4 * (PV_THREADS / 64);
    l.box = at; at += 2 * PV_BOX * cap1;
    l.tok = at; at += 2 * len; at = (at + 3) & ~3;
    l.zkey = at; at += 2 * cap1; at = (at + 3) & ~3;
    l.xs = at; at += 2 * 2 * cap1;
    l.ys = at; at += 2 * 2 * cap1;
    l.bytes = (at + 15) & ~15;
    return l;
}

// Position of entry i among n keys read at key[i * stride]: the number of entries before it in (key, index) order.
PM_HD int pv_rank(const int16_t* key, int stride, int n, int i) {
    const int16_t v = key[i * stride];
    int below = 0;
    for (int j = 0; j < n; ++j) {
        const int16_t u = key[j * stride];
        below += (u < v) || (u == v && j < i);
    }
    return below;
}

// Bound e of axis `d` (0 x, 1 y) of n boxes: the lower bounds of all boxes, then the upper bounds.
PM_HD int16_t pv_bound(const int16_t* box, int n, int d, int e) { return e < n ? box[PV_BOX * e + d] : box[PV_BOX * (e - n) + 3 + d]; }

// Position of bound e among the 2 n bounds of axis d in (value, e) order.
PM_HD int pv_bound_rank(const int16_t* box, int n, int d, int e) {
    const int16_t v = pv_bound(box, n, d, e);
    int below = 0;
    for (int j = 0; j < n; ++j) {
        const int16_t lo = box[PV_BOX * j + d], hi = box[PV_BOX * j + 3 + d];
        below += (lo < v) || (lo == v && j < e);
        below += (hi < v) || (hi == v && j + n < e);
    }
    return below;
}

// The bit row of the slab [lo, hi), lo < hi, of axis d over n boxes: bit k if box k spans it.  `row` is written at row[w * stride].
// Returns whether any bit is set.
PM_HD bool pv_slab_row(const int16_t* box, int n, int words, int d, int lo, int hi, uint64_t* row, int stride) {
    uint64_t any = 0;
    for (int w = 0; w < words; ++w) {
        uint64_t bits = 0;
        const int end = n < w * 64 + 64 ? n : w * 64 + 64;
        for (int k = w * 64; k < end; ++k)
            bits |= (uint64_t)(box[PV_BOX * k + d] <= lo && box[PV_BOX * k + 3 + d] >= hi) << (k - w * 64);
        row[w * stride] = bits;
        any |= bits;
    }
    return any != 0;
}

// One column: the z length covered by the boxes of side a, of side b and of either, among the boxes `rowx & rowy`.
PM_HD void pv_column(const uint64_t* rowx, int stride, const uint64_t* rowy, int words, const int16_t* box, int32_t* len3) {
    int32_t end_a = PV_BELOW, end_b = PV_BELOW, end_e = PV_BELOW, la = 0, lb = 0, le = 0;
    for (int w = 0; w < words; ++w) {
        uint64_t m = rowx[w * stride] & rowy[w];
        while (m) {
            const int16_t* b = box + PV_BOX * (w * 64 + __builtin_ctzll(m));
            m &= m - 1;
            const int32_t z0 = b[2], z1 = b[5];
            const int32_t from_e = z0 > end_e ? z0 : end_e;                  // z0 only grows: what lies below end_e is counted
            if (z1 > from_e) { le += z1 - from_e; end_e = z1; }
            if (b[6]) {
                const int32_t from = z0 > end_b ? z0 : end_b;
                if (z1 > from) { lb += z1 - from; end_b = z1; }
            } else {
                const int32_t from = z0 > end_a ? z0 : end_a;
                if (z1 > from) { la += z1 - from; end_a = z1; }
            }
        }
    }
    len3[0] = la; len3[1] = lb; len3[2] = le;
}

// The x slab i of n boxes: its bit row goes to `rowx`, then the y slabs j0, j0 + jstep, ... are swept (0 and 1: all of them).
// Adds the three volumes to vol3.
PM_HD void pv_x_slab(const int16_t* box, int n, int words, const int16_t* xs, const int16_t* ys, const uint64_t* rowy, int i,
                     int j0, int jstep, uint64_t* rowx, int stride, int64_t* vol3) {
    const int x0 = xs[i], x1 = xs[i + 1];
    if (x1 == x0 || !pv_slab_row(box, n, words, 0, x0, x1, rowx, stride)) return;
    int64_t a = 0, b = 0, e = 0;
    for (int j = j0; j + 1 < 2 * n; j += jstep) {
        const int dy = ys[j + 1] - ys[j];
        if (dy == 0) continue;
        int32_t len3[3];
        pv_column(rowx, stride, rowy + j * words, words, box, len3);
        a += (int64_t)len3[0] * dy; b += (int64_t)len3[1] * dy; e += (int64_t)len3[2] * dy;
    }
    vol3[0] += a * (x1 - x0); vol3[1] += b * (x1 - x0); vol3[2] += e * (x1 - x0);
}

PM_HD void pv_results(int64_t union_a, int64_t sum_a, int64_t union_b, int64_t sum_b, int64_t union_ab, int n_a, int n_b, int64_t* out8) {
    out8[0] = union_a; out8[1] = sum_a; out8[2] = union_b; out8[3] = sum_b;
    out8[4] = union_a + union_b - union_ab; out8[5] = union_ab; out8[6] = n_a; out8[7] = n_b;
}

// ---- one pair, serially: what the kernel computes, in the kernel's own order of steps.  `mem`: pv_layout(len_a, len_b).bytes.
// One row -> its clamped tokens in tok[0 .. len) and its solid planks appended to the unordered list (zkey, ubox) from `n` on.
PM_HD int pv_load_side_serial(const int64_t* row, int len, int end_token, int side, int16_t* tok, int16_t* zkey, int16_t* ubox,
                              int n, int64_t* sum) {
    int first = len;
    for (int i = 0; i < len; ++i) {
        const int64_t t = row[i];
        tok[i] = (int16_t)pm_coord(t);
        if (t == (int64_t)end_token && first == len) first = i;
    }
    const int planks = first / PM_DOF;
    for (int p = 1; p < planks; ++p) {
        int32_t b[PM_DOF];
        for (int d = 0; d < PM_DOF; ++d) b[d] = tok[PM_DOF * p + d];
        if (!pv_solid(b)) continue;
        for (int d = 0; d < PM_DOF; ++d) ubox[PV_BOX * n + d] = (int16_t)b[d];
        ubox[PV_BOX * n + 6] = (int16_t)side; ubox[PV_BOX * n + 7] = 0;
        zkey[n] = (int16_t)b[2];
        *sum += pv_volume(b);
        ++n;
    }
    return n;
}

// `ubox`: int16 [cap][PV_BOX] of the caller's, beside `mem` (the kernel keeps the unordered boxes in registers).
PM_HD void pv_pair_serial(const int64_t* row_a, int len_a, const int64_t* row_b, int len_b, int end_token, unsigned char* mem,
                          int16_t* ubox, int64_t* out8) {
    const PvLayout l = pv_layout(len_a, len_b);
    int16_t* tok = (int16_t*)(mem + l.tok);
    int16_t* zkey = (int16_t*)(mem + l.zkey);
    int16_t* box = (int16_t*)(mem + l.box);
    int16_t* xs = (int16_t*)(mem + l.xs);
    int16_t* ys = (int16_t*)(mem + l.ys);
    uint64_t* rowy = (uint64_t*)(mem + l.rowy);
    uint64_t* rowx = (uint64_t*)(mem + l.rowx);
    int64_t sum_a = 0, sum_b = 0;
    const int na = pv_load_side_serial(row_a, len_a, end_token, 0, tok, zkey, ubox, 0, &sum_a);
    const int n = row_b ? pv_load_side_serial(row_b, len_b, end_token, 1, tok + len_a, zkey, ubox, na, &sum_b) : na;
    for (int i = 0; i < n; ++i) {
        const int at = pv_rank(zkey, 1, n, i);
        for (int d = 0; d < PV_BOX; ++d) box[PV_BOX * at + d] = ubox[PV_BOX * i + d];
    }
    for (int e = 0; e < 2 * n; ++e) {
        xs[pv_bound_rank(box, n, 0, e)] = pv_bound(box, n, 0, e);
        ys[pv_bound_rank(box, n, 1, e)] = pv_bound(box, n, 1, e);
    }
    for (int j = 0; j + 1 < 2 * n; ++j) {
        if (ys[j + 1] > ys[j]) pv_slab_row(box, n, l.words, 1, ys[j], ys[j + 1], rowy + j * l.words, 1);
        else for (int w = 0; w < l.words; ++w) rowy[j * l.words + w] = 0;
    }
    int64_t vol3[3] = {0, 0, 0};
    for (int i = 0; i + 1 < 2 * n; ++i)                                    // thread i % PV_THREADS's row, as in the kernel
        pv_x_slab(box, n, l.words, xs, ys, rowy, i, 0, 1, rowx + i % PV_THREADS, PV_THREADS, vol3);
    pv_results(vol3[0], sum_a, vol3[1], sum_b, vol3[2], na, n - na, out8);
}

#endif
