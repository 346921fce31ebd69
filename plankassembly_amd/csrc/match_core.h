// Plank matching core: what one pair of token rows means as two sets of planks, and how many of them
// match.  Every function here is plain integer / double C++ and compiles for the device (csrc/match.hip, one wave per pair) and
// for the host alone (tools/match_host, the stand-alone program the sanitizer build runs).  tests/match_reference.py is the
// numpy restatement both are pinned to.
//
// What it restates: plankassembly_amd/metric.py `pairwise_iou_3d` + `HungarianMatcher` (reference third_party/matcher.py:29-61)
// with the box pipeline of the trainers (row 0 dropped on both sides, zero-extent planks dropped where `filter` is set).  The
// Hungarian cost is binary (-1 where IoU > threshold, else 100000), so the assignment is a maximum-cardinality bipartite
// matching on the edges IoU > threshold; pairs with IoU == threshold are no edges and are counted apart (`ties`).
//
// No recursion, no local arrays: every array is handed in by the caller (LDS on the device), so the device build needs no
// scratch memory and no device stack.
#ifndef PLANK_MATCH_CORE_H
#define PLANK_MATCH_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PM_HD __host__ __device__ __forceinline__
#else
#define PM_HD static inline
#endif

#define PM_DOF 6
#define PM_MAX_PLANKS 170                                  /* per side, after row 0 is dropped */
#define PM_MAX_LEN (PM_DOF * (PM_MAX_PLANKS + 1))          /* 1026 tokens: the 1024-step decode */
#define PM_MAX_WORDS ((PM_MAX_PLANKS + 63) / 64)           /* 64-bit words of one adjacency row */
// Coordinates are held as int32 clamped to the int16 range: an extent is below 2^16, a volume below 2^48 and a union below
// 2^50, so the integer arithmetic cannot overflow for ANY int64 token value and every integer is exact as a double.  Tokens of
// the vocabulary (0 .. 513) are far inside.
#define PM_COORD_MIN (-32768)
#define PM_COORD_MAX 32767

PM_HD int32_t pm_coord(int64_t t) {
    return (int32_t)(t < PM_COORD_MIN ? PM_COORD_MIN : (t > PM_COORD_MAX ? PM_COORD_MAX : t));
}

// The trainers' `_valid_pred`: with `filter`, a plank with any zero extent is dropped.  Inverted planks (hi < lo) stay.
PM_HD bool pm_keep(const int32_t* box, int filter) {
    if (!filter) return true;
    return box[3] - box[0] != 0 && box[4] - box[1] != 0 && box[5] - box[2] != 0;
}

// bit 0: iou > threshold (an edge); bit 1: iou >= threshold && !(iou > threshold) (a tie).  metric.pairwise_iou_3d's float64
// values are exact integers here, and the quotient is the same single correctly rounded double division.
PM_HD int pm_edge(const int32_t* a, const int32_t* b, double threshold) {
    int64_t inter = 1;
    for (int d = 0; d < 3; ++d) {
        const int32_t lo = a[d] > b[d] ? a[d] : b[d];
        const int32_t hi = a[d + 3] < b[d + 3] ? a[d + 3] : b[d + 3];
        const int32_t e = hi - lo;
        inter *= e > 0 ? e : 0;
    }
    double iou = 0.0;
    if (inter > 0) {                                       // both planks then have positive extents: union >= each volume > 0
        const int64_t va = (int64_t)(a[3] - a[0]) * (a[4] - a[1]) * (a[5] - a[2]);
        const int64_t vb = (int64_t)(b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]);
        iou = (double)inter / (double)(va + vb - inter);
    }
    const int gt = iou > threshold, ge = iou >= threshold;
    return gt | ((ge && !gt) << 1);
}

// Where everything of one pair lives, in bytes from a 16-byte aligned base: LDS on the device, one heap block on the host.
struct PmLayout {
    int cap_a, cap_b;          // planks a side can hold after row 0 is dropped
    int words;                 // 64-bit words per adjacency row
    int adj, visited, taken;   // uint64 [cap_a][words], [words], [words]
    int tok_a, tok_b;          // int32 [len_a], [len_b]: the clamped tokens, then - in place - the kept boxes
    int match_b, stk_a, stk_j; // int16 [cap_b], [cap_a], [cap_a]
    int bytes;
};

PM_HD int pm_cap(int len) { const int p = len / PM_DOF - 1; return p > 0 ? p : 0; }

PM_HD PmLayout pm_layout(int len_a, int len_b) {
    PmLayout l;
    l.cap_a = pm_cap(len_a); l.cap_b = pm_cap(len_b);
    l.words = (l.cap_b + 63) / 64; if (l.words < 1) l.words = 1;
    int at = 0;
    l.adj = at; at += 8 * (l.cap_a > 0 ? l.cap_a : 1) * l.words;
    l.visited = at; at += 8 * l.words;
    l.taken = at; at += 8 * l.words;
    l.tok_a = at; at += 4 * (len_a > 0 ? len_a : 1);
    l.tok_b = at; at += 4 * (len_b > 0 ? len_b : 1);
    l.match_b = at; at += 2 * (l.cap_b > 0 ? l.cap_b : 1);
    l.stk_a = at; at += 2 * (l.cap_a > 0 ? l.cap_a : 1);
    l.stk_j = at; at += 2 * (l.cap_a > 0 ? l.cap_a : 1);
    l.bytes = (at + 15) & ~15;
    return l;
}

// Maximum-cardinality matching of na x nb over the bit rows `adj` (bit j of row i: an edge; no bit at or above nb is set).
// Augmenting paths, depth first, iterative: level k of the explicit stack holds a plank of side a (stk_a[k]) and the plank of
// side b it reached for (stk_j[k]).  A plank of b is looked at once per search (`visited`), a free one is preferred (`taken`:
// the matched planks of b), so a search ends after at most nb pushes and the stack never holds more than min(na, nb + 1) levels.
PM_HD int pm_match(const uint64_t* adj, int na, int nb, int words, int16_t* match_b, int16_t* stk_a, int16_t* stk_j,
                   uint64_t* visited, uint64_t* taken) {
    for (int j = 0; j < nb; ++j) match_b[j] = -1;
    for (int w = 0; w < words; ++w) taken[w] = 0;
    int tp = 0;
    for (int u = 0; u < na; ++u) {
        for (int w = 0; w < words; ++w) visited[w] = 0;
        int sp = 0;
        stk_a[0] = (int16_t)u;
        while (sp >= 0) {
            const uint64_t* row = adj + (int)stk_a[sp] * words;
            int j = -1;
            bool is_free = false;
            for (int w = 0; w < words && j < 0; ++w) {
                const uint64_t c = row[w] & ~visited[w] & ~taken[w];
                if (c) { j = w * 64 + __builtin_ctzll(c); is_free = true; }
            }
            for (int w = 0; w < words && j < 0; ++w) {
                const uint64_t c = row[w] & ~visited[w];
                if (c) j = w * 64 + __builtin_ctzll(c);
            }
            if (j < 0) { --sp; continue; }                 // dead end: back to the plank below, which tries its next edge
            visited[j >> 6] |= 1ull << (j & 63);
            stk_j[sp] = (int16_t)j;
            if (is_free) {                                 // flip the path: every level takes the plank it reached for
                taken[j >> 6] |= 1ull << (j & 63);
                for (int k = sp; k >= 0; --k) match_b[stk_j[k]] = stk_a[k];
                ++tp;
                break;
            }
            stk_a[++sp] = match_b[j];                      // j is matched: its partner has to move
        }
    }
    return tp;
}

// ---- one pair, serially: what the kernel computes, in the kernel's own order of steps.  `mem`: pm_layout(len_a, len_b).bytes.
// L = index of the first `end_token` (len without one); L / 6 planks, plank 0 dropped, the kept ones compacted in place.
PM_HD int pm_load_side_serial(const int64_t* row, int len, int end_token, int filter, int32_t* tok) {
    int first = len;
    for (int i = 0; i < len; ++i) {
        const int64_t t = row[i];
        tok[i] = pm_coord(t);
        if (t == (int64_t)end_token && first == len) first = i;
    }
    const int planks = first / PM_DOF;
    int n = 0;
    for (int p = 1; p < planks; ++p) {
        int32_t box[PM_DOF];
        for (int d = 0; d < PM_DOF; ++d) box[d] = tok[PM_DOF * p + d];
        if (!pm_keep(box, filter)) continue;
        for (int d = 0; d < PM_DOF; ++d) tok[PM_DOF * n + d] = box[d];        // n <= p - 1: behind every plank still to read
        ++n;
    }
    return n;
}

PM_HD void pm_pair_serial(const int64_t* row_a, int len_a, const int64_t* row_b, int len_b, int end_token, int filter_a,
                          int filter_b, double threshold, unsigned char* mem, int32_t* out4) {
    const PmLayout l = pm_layout(len_a, len_b);
    uint64_t* adj = (uint64_t*)(mem + l.adj);
    int32_t* tok_a = (int32_t*)(mem + l.tok_a);
    int32_t* tok_b = (int32_t*)(mem + l.tok_b);
    const int na = pm_load_side_serial(row_a, len_a, end_token, filter_a, tok_a);
    const int nb = pm_load_side_serial(row_b, len_b, end_token, filter_b, tok_b);
    int ties = 0;
    for (int i = 0; i < na; ++i)
        for (int w = 0; w < l.words; ++w) {
            uint64_t bits = 0;
            const int hi = nb < w * 64 + 64 ? nb : w * 64 + 64;
            for (int j = w * 64; j < hi; ++j) {
                const int e = pm_edge(tok_a + PM_DOF * i, tok_b + PM_DOF * j, threshold);
                bits |= (uint64_t)(e & 1) << (j - w * 64);
                ties += e >> 1;
            }
            adj[i * l.words + w] = bits;
        }
    out4[0] = pm_match(adj, na, nb, l.words, (int16_t*)(mem + l.match_b), (int16_t*)(mem + l.stk_a), (int16_t*)(mem + l.stk_j),
                       (uint64_t*)(mem + l.visited), (uint64_t*)(mem + l.taken));
    out4[1] = na; out4[2] = nb; out4[3] = ties;
}

#endif
