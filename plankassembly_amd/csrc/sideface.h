// Side-face extraction from the line drawing, on the device: included by tokenise.hip, inside its
// namespace, after the stages it shares with tokenise_kernel.  One block of 256 threads per drawing, one launch per batch:
// noise (the line kind's draws), faces of the three views, centre lines, the sequential merge, boxes, tokens.  What it
// restates: plankassembly_amd/datasets.py `extract_sideface_flags` (reference sideface_data.py:22-135 polygonize / parse /
// merge / buffer, :233-245 augmentation and fallback) - float64, every operation rounded on its own, comparisons only.
//
// The graph of a drawing: half-edge 2i / 2i + 1 is line i forward / backward; a node is named by the smallest half-edge that
// starts at its point (same view, same coordinates by value); table[node][E N W S] holds the half-edge leaving in that
// direction + 1.  Every loop is bounded by a count known on entry, so a malformed drawing sets flags and never spins.
//
// LDS at PA_TOKENISE_MAX_LINES = 1024 lines (2048 half-edges, <= 512 bounded faces, <= 1024 centre lines):
//   seg 32 KB + node 4 KB + hdir 2 KB + est 1 KB                                     39 KB   the graph
//   scratch 36 KB: table 16 + next 4 + label 2 x 4 + jump 2 x 4 while tracing,
//                  then centre / width / lo / hi of the centre lines, 4 x 8 KB        36 KB
//   fbox 16 KB + frep 1 KB + forder 1 KB + fview 0.5 KB + cmeta 1 KB                 19.5 KB the faces and the list's flags
//   key 8 + skey 8 + selh 4 + spos 2 KB (tokenise_kernel's own)                      22 KB
//   total 117.8 KB (120 584 B with the counters and alignment) of the 160 KB a gfx950 workgroup may take; one block per CU, and a batch is 64 blocks on 256 CUs.

constexpr int SF_MAX_HALF = 2 * TK_MAX_LINES;
constexpr int SF_MAX_FACES = SF_MAX_HALF / 4;          // a bounded ring has at least 4 half-edges, and rings share none
constexpr int SF_MAX_CANDS = 2 * SF_MAX_FACES;         // horizontal + vertical centre line per face
static_assert(SF_MAX_CANDS <= TK_MAX_LINES, "a centre line's number must fit the sort key's line field");
enum { SF_OUT_OF_DOMAIN = 1, SF_TRUNCATED = 2, SF_FELL_BACK = 4, SF_DEGENERATE = 8 };
enum { SF_ALIVE = 1, SF_MARK = 2, SF_DEAD_VIEW = 0xff };
constexpr double SF_DEGENERATE_AREA2 = 1e-12;

struct SfArgs {
    TkArgs t;
    double max_thickness, min_thickness, merge_tolerance;
    double* faces_out; uint8_t* faceviews_out; int32_t* n_faces_out; int32_t* flags_out;
};

struct SfLds {
    double* seg; uint16_t* node; uint8_t* hdir; uint8_t* est; uint8_t* eview;
    uint16_t* table; uint16_t* next; uint16_t* lab; uint16_t* jmp;      // lab / jmp: two buffers of SF_MAX_HALF
    double* ccen; double* cwid; unsigned long long* clo; unsigned long long* chi;
    double* fbox; uint16_t* frep; uint16_t* forder; uint8_t* fview; uint8_t* cmeta;
    uint64_t* key; uint64_t* skey; uint32_t* selh; uint16_t* spos;
    int* counter;                                      // [0] faces found, [1] flags of the pass
};

// doubles <-> unsigned keys of the same order, for the LDS min / max of the merge
__device__ __forceinline__ unsigned long long sf_ordered(double v) {
    const unsigned long long u = (unsigned long long)__builtin_bit_cast(uint64_t, v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double sf_unordered(unsigned long long k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __builtin_bit_cast(double, u);
}

__device__ __forceinline__ int sf_degree(const uint16_t* table, int node) {
    const uint16_t* t = table + 4 * node;
    return (t[0] != 0) + (t[1] != 0) + (t[2] != 0) + (t[3] != 0);
}

// next(u -> v): at v, from the direction v -> u clockwise to the first direction with an outgoing half-edge; then the ring
// label of every surviving half-edge (the smallest half-edge of its ring) by pointer doubling over `rounds` rounds.
__device__ __forceinline__ int sf_rings(const SfLds& m, int n, int rounds) {
    const int tid = threadIdx.x;
    for (int h = tid; h < 2 * n; h += TK_THREADS) {
        int nx = h;
        if (m.est[h >> 1] & SF_ALIVE) {
            const int v = m.node[h ^ 1], back = m.hdir[h ^ 1];
            for (int k = 1; k <= 4; ++k) {
                const int t = m.table[4 * v + ((back - k) & 3)];
                if (t) { nx = t - 1; break; }
            }
        }
        m.next[h] = (uint16_t)nx;
        m.lab[h] = (uint16_t)h;
        m.jmp[h] = (uint16_t)nx;
    }
    __syncthreads();
    int cur = 0;                                                               // offset of the buffer that holds the state
    for (int r = 0; r < rounds; ++r) {
        const int nxt = cur ^ SF_MAX_HALF;
        for (int h = tid; h < 2 * n; h += TK_THREADS) {
            const int j = m.jmp[cur + h];
            const uint16_t a = m.lab[cur + h], b = m.lab[cur + j];
            m.lab[nxt + h] = a < b ? a : b;
            m.jmp[nxt + h] = m.jmp[cur + j];
        }
        __syncthreads();
        cur = nxt;
    }
    return cur;
}

// One extraction pass over the drawing's n lines (noisy: as the draws leave them).  Fills key[0 .. 2 * faces) with the sort
// keys of the merged boxes (TK_DELETED where a centre line is gone) and returns that count; the pass's flags go to counter[1].
__device__ __forceinline__ int sf_extract(const SfArgs& s, const SfLds& m, int lo, int n, bool noisy, int num_select, uint32_t base,
                                          double rq) {
    const TkArgs& a = s.t;
    const int tid = threadIdx.x;
    if (tid == 0) { m.counter[0] = 0; m.counter[1] = 0; }
    // ---- lines -> half-edges; the domain
    bool bad = false;
    for (int i = tid; i < n; i += TK_THREADS) {
        double x0, y0, x1, y1;
        bool kept = true;
        if (noisy) kept = tk_noisy_segment(a, lo, i, n, m.selh, num_select, base, x0, y0, x1, y1);
        else { const double* g = a.seg + (size_t)(lo + i) * 4; x0 = g[0]; y0 = g[1]; x1 = g[2]; y1 = g[3]; }
        x0 = x0 + 0.0; y0 = y0 + 0.0; x1 = x1 + 0.0; y1 = y1 + 0.0;            // -0.0 -> 0.0: nodes compare by value
        const int view = a.view[lo + i];
        kept = kept && view <= 2 && (x0 != x1 || y0 != y1);                    // views 0, 1, 2 only; no zero-length segment
        int fwd = 0;
        if (kept) {
            const bool inside = x0 >= -1.0 && x0 <= 1.0 && y0 >= -1.0 && y0 <= 1.0 && x1 >= -1.0 && x1 <= 1.0 && y1 >= -1.0 && y1 <= 1.0;
            if (!inside || (x0 != x1 && y0 != y1)) { bad = true; kept = false; }
            fwd = y0 == y1 ? (x1 > x0 ? 0 : 2) : (y1 > y0 ? 1 : 3);           // E N W S
        }
        m.seg[4 * i] = x0; m.seg[4 * i + 1] = y0; m.seg[4 * i + 2] = x1; m.seg[4 * i + 3] = y1;
        m.est[i] = kept ? SF_ALIVE : 0;
        m.eview[i] = kept ? (uint8_t)view : (uint8_t)SF_DEAD_VIEW;
        m.hdir[2 * i] = (uint8_t)fwd; m.hdir[2 * i + 1] = (uint8_t)((fwd + 2) & 3);
    }
    for (int j = tid; j < 8 * n; j += TK_THREADS) m.table[j] = 0;
    int n_bad = __syncthreads_count(bad);
    // ---- nodes: the smallest half-edge that starts at the same point of the same view
    for (int h = tid; h < 2 * n; h += TK_THREADS) {
        int nd = h;
        const int view = m.eview[h >> 1];
        if (view != SF_DEAD_VIEW && !n_bad) {
            const double x = m.seg[2 * h], y = m.seg[2 * h + 1];               // half-edge h starts at point h of the segment array
            for (int g = 0; g < h; ++g)
                if (m.seg[2 * g] == x && m.seg[2 * g + 1] == y && m.eview[g >> 1] == view) { nd = g; break; }
        }
        m.node[h] = (uint16_t)nd;
    }
    __syncthreads();
    for (int h = tid; h < 2 * n; h += TK_THREADS)
        if (m.est[h >> 1] & SF_ALIVE) m.table[4 * m.node[h] + m.hdir[h]] = (uint16_t)(h + 1);
    __syncthreads();
    bad = false;                                                               // two half-edges leaving a node in one direction
    for (int h = tid; h < 2 * n; h += TK_THREADS)
        if ((m.est[h >> 1] & SF_ALIVE) && m.table[4 * m.node[h] + m.hdir[h]] != (uint16_t)(h + 1)) bad = true;
    n_bad += __syncthreads_count(bad);
    if (n_bad) {                                                               // outside the domain: no face at all
        if (tid == 0) m.counter[1] = SF_OUT_OF_DOMAIN;
        __syncthreads();
        return 0;
    }
    // ---- dangles: every edge with an end node of degree 1, until none is left (at most one round per edge)
    for (int round = 0; round < n; ++round) {
        bool any = false;
        for (int i = tid; i < n; i += TK_THREADS)
            if ((m.est[i] & SF_ALIVE) && (sf_degree(m.table, m.node[2 * i]) == 1 || sf_degree(m.table, m.node[2 * i + 1]) == 1)) {
                m.est[i] |= SF_MARK;
                any = true;
            }
        if (!__syncthreads_count(any)) break;
        for (int i = tid; i < n; i += TK_THREADS)
            if (m.est[i] & SF_MARK) {
                m.est[i] = 0;
                m.table[4 * m.node[2 * i] + m.hdir[2 * i]] = 0;
                m.table[4 * m.node[2 * i + 1] + m.hdir[2 * i + 1]] = 0;
            }
        __syncthreads();
    }
    // ---- rings; cut edges (both half-edges on one ring) out; rings once more
    int rounds = 0;
    while ((1 << rounds) < 2 * n) ++rounds;
    int cur = sf_rings(m, n, rounds);
    bool any = false;
    for (int i = tid; i < n; i += TK_THREADS)
        if ((m.est[i] & SF_ALIVE) && m.lab[cur + 2 * i] == m.lab[cur + 2 * i + 1]) { m.est[i] |= SF_MARK; any = true; }
    if (__syncthreads_count(any)) {
        for (int i = tid; i < n; i += TK_THREADS)
            if (m.est[i] & SF_MARK) {
                m.est[i] = 0;
                m.table[4 * m.node[2 * i] + m.hdir[2 * i]] = 0;
                m.table[4 * m.node[2 * i + 1] + m.hdir[2 * i + 1]] = 0;
            }
        __syncthreads();
        cur = sf_rings(m, n, rounds);
    }
    // ---- the ring's smallest half-edge walks it: float64 shoelace from there, bounds; positive = a bounded face
    for (int h = tid; h < 2 * n; h += TK_THREADS) {
        if (!(m.est[h >> 1] & SF_ALIVE) || m.lab[cur + h] != h) continue;
        double area2 = 0.0, xmin = m.seg[2 * h], ymin = m.seg[2 * h + 1], xmax = xmin, ymax = ymin;
        int g = h;
        for (int step = 0; step < 2 * n; ++step) {
            const double xu = m.seg[2 * g], yu = m.seg[2 * g + 1], xv = m.seg[2 * (g ^ 1)], yv = m.seg[2 * (g ^ 1) + 1];
            const double p = xu * yv, q = xv * yu;
            area2 = area2 + (p - q);
            xmin = xu < xmin ? xu : xmin; xmax = xu > xmax ? xu : xmax;
            ymin = yu < ymin ? yu : ymin; ymax = yu > ymax ? yu : ymax;
            g = m.next[g];
            if (g == h) break;
        }
        if (__builtin_fabs(area2) < SF_DEGENERATE_AREA2) atomicOr(&m.counter[1], (int)SF_DEGENERATE);
        else if (area2 > 0.0) {
            const int slot = atomicAdd(&m.counter[0], 1);
            if (slot < SF_MAX_FACES) {
                m.fbox[4 * slot] = xmin; m.fbox[4 * slot + 1] = ymin; m.fbox[4 * slot + 2] = xmax; m.fbox[4 * slot + 3] = ymax;
                m.frep[slot] = (uint16_t)h;
                m.fview[slot] = m.eview[h >> 1];
            }
        }
    }
    __syncthreads();
    const int nf = m.counter[0] < SF_MAX_FACES ? m.counter[0] : SF_MAX_FACES;
    // ---- the defined order: (view, xmin, ymin, xmax, ymax, smallest half-edge); from here on table / next / labels are dead
    for (int f = tid; f < nf; f += TK_THREADS) {
        const double b0 = m.fbox[4 * f], b1 = m.fbox[4 * f + 1], b2 = m.fbox[4 * f + 2], b3 = m.fbox[4 * f + 3];
        const int view = m.fview[f], rep = m.frep[f];
        int below = 0;
        for (int g = 0; g < nf; ++g) {
            const double c0 = m.fbox[4 * g], c1 = m.fbox[4 * g + 1], c2 = m.fbox[4 * g + 2], c3 = m.fbox[4 * g + 3];
            const int cv = m.fview[g], cr = m.frep[g];
            bool less = cr < rep;
            less = c3 != b3 ? c3 < b3 : less;
            less = c2 != b2 ? c2 < b2 : less;
            less = c1 != b1 ? c1 < b1 : less;
            less = c0 != b0 ? c0 < b0 : less;
            less = cv != view ? cv < view : less;
            below += less;
        }
        m.forder[below] = (uint16_t)f;
    }
    __syncthreads();
    // ---- centre lines (parse_sideface_from_polygons): horizontal at 2r, vertical at 2r + 1 for the face of rank r
    for (int c = tid; c < 2 * nf; c += TK_THREADS) {
        const int f = m.forder[c >> 1], horizontal = !(c & 1);
        const double xmin = m.fbox[4 * f], ymin = m.fbox[4 * f + 1], xmax = m.fbox[4 * f + 2], ymax = m.fbox[4 * f + 3];
        const double width = horizontal ? ymax - ymin : xmax - xmin;
        const double sum = horizontal ? ymin + ymax : xmin + xmax;
        m.ccen[c] = sum / 2.0;
        m.cwid[c] = width;
        m.clo[c] = sf_ordered(horizontal ? xmin : ymin);
        m.chi[c] = sf_ordered(horizontal ? xmax : ymax);
        m.cmeta[c] = width < s.max_thickness ? (uint8_t)(SF_ALIVE | (horizontal << 1) | (m.fview[f] << 2)) : (uint8_t)0;
    }
    __syncthreads();
    // ---- merge_colinaer_sidefaces, one centre line at a time, the block's threads spread over the list so far.  Line c of the
    // list is centre line c once it has been appended; a merged line leaves the list by losing SF_ALIVE.  q's own range is read
    // from its face (immutable), the union goes to clo / chi [c], which no thread reads before the barrier.
    for (int c = 1; c < 2 * nf; ++c) {
        const int meta = m.cmeta[c];
        if (!(meta & SF_ALIVE)) continue;                                      // the same for every thread
        const int f = m.forder[c >> 1], horizontal = !(c & 1);
        const double qlo = horizontal ? m.fbox[4 * f] : m.fbox[4 * f + 1], qhi = horizontal ? m.fbox[4 * f + 2] : m.fbox[4 * f + 3];
        const double qcen = m.ccen[c], qwid = m.cwid[c];
        for (int j = tid; j < c; j += TK_THREADS) {
            if (m.cmeta[j] != meta) continue;                                  // alive, same type, same view
            const double d = qwid - m.cwid[j];
            if (!(__builtin_fabs(d) < s.merge_tolerance) || m.ccen[j] != qcen) continue;
            const double jlo = sf_unordered(m.clo[j]), jhi = sf_unordered(m.chi[j]);
            if (!(qlo <= jhi && jlo <= qhi)) continue;                         // the closed ranges overlap or touch
            m.cmeta[j] = 0;
            atomicMin(&m.clo[c], m.clo[j]);
            atomicMax(&m.chi[c], m.chi[j]);
        }
        __syncthreads();
    }
    // ---- boxes (the flat-capped buffer's bounds) of the lines that stay and are wide enough -> sort keys
    for (int c = tid; c < 2 * nf; c += TK_THREADS) {
        uint64_t k = TK_DELETED;
        const int meta = m.cmeta[c];
        if ((meta & SF_ALIVE) && m.cwid[c] >= s.min_thickness) {
            const double half = m.cwid[c] / 2.0, cen = m.ccen[c], l = sf_unordered(m.clo[c]), h = sf_unordered(m.chi[c]);
            const double a0 = cen - half, a1 = cen + half;
            k = (meta & 2) ? tk_key((uint32_t)(meta >> 2), l, a0, h, a1, rq, c) : tk_key((uint32_t)(meta >> 2), a0, l, a1, h, rq, c);
        }
        m.key[c] = k;
    }
    __syncthreads();
    return 2 * nf;
}

__global__ __launch_bounds__(TK_THREADS) void sideface_kernel(SfArgs s) {
    __shared__ double seg[TK_MAX_LINES * 4];
    __shared__ uint16_t node[SF_MAX_HALF];
    __shared__ uint8_t hdir[SF_MAX_HALF];
    __shared__ uint8_t est[TK_MAX_LINES], eview[TK_MAX_LINES];
    __shared__ double scratch[SF_MAX_HALF * 18 / 8];                           // 36 KB, see the budget above
    __shared__ double fbox[SF_MAX_FACES * 4];
    __shared__ uint16_t frep[SF_MAX_FACES], forder[SF_MAX_FACES];
    __shared__ uint8_t fview[SF_MAX_FACES], cmeta[SF_MAX_CANDS];
    __shared__ uint64_t key[TK_MAX_LINES], skey[TK_MAX_LINES];
    __shared__ uint32_t selh[TK_MAX_LINES];
    __shared__ uint16_t spos[TK_MAX_LINES];
    __shared__ int counter[2];
    static_assert(4 * SF_MAX_CANDS * 8 <= SF_MAX_HALF * 18, "the centre lines reuse the tracing arrays");

    SfLds m;
    m.seg = seg; m.node = node; m.hdir = hdir; m.est = est; m.eview = eview;
    m.table = reinterpret_cast<uint16_t*>(scratch);
    m.next = m.table + 4 * SF_MAX_HALF;
    m.lab = m.next + SF_MAX_HALF;
    m.jmp = m.lab + 2 * SF_MAX_HALF;
    m.ccen = scratch; m.cwid = m.ccen + SF_MAX_CANDS;
    m.clo = reinterpret_cast<unsigned long long*>(m.cwid + SF_MAX_CANDS); m.chi = m.clo + SF_MAX_CANDS;
    m.fbox = fbox; m.frep = frep; m.forder = forder; m.fview = fview; m.cmeta = cmeta;
    m.key = key; m.skey = skey; m.selh = selh; m.spos = spos; m.counter = counter;

    const TkArgs& a = s.t;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int d = a.index[b];
    const bool have = d >= 0 && d < a.N;
    const int lo = have ? a.line_off[d] : 0;
    int n = have ? a.line_off[d + 1] - lo : 0;
    n = n < 0 ? 0 : (n > TK_MAX_LINES ? TK_MAX_LINES : n);
    int max_faces = (a.S - 1) >> 2;                    // what fits the row
    max_faces = max_faces < 0 ? 0 : max_faces;
    const double rq = (double)((1 << a.n_bits) - 1);

    uint32_t base;
    int num_select;
    const bool augmented = tk_draws(a, d, n, selh, base, num_select);
    int flags = 0;
    int nc = sf_extract(s, m, lo, n, augmented, num_select, base, rq);
    int nk = tk_rank(key, skey, spos, nc);
    flags |= counter[1];
    if (augmented && nk == 0) {                        // the noise left no face: the clean drawing (sideface_data.py:240-245)
        __syncthreads();
        flags |= SF_FELL_BACK;
        nc = sf_extract(s, m, lo, n, false, 0, 0, rq);
        nk = tk_rank(key, skey, spos, nc);
        flags |= counter[1];
    }
    if (nk > max_faces) { nk = max_faces; flags |= SF_TRUNCATED; }     // the faces that sort first stay
    tk_store_inputs(a, b, lo, skey, spos, nk);
    tk_store_outputs(a, b, d, have, rq);

    // ---- the merged boxes before quantisation, in the row's order
    if (s.faces_out)
        for (int j = tid; j < 4 * max_faces; j += TK_THREADS) {
            double v = 0.0;
            if (j < 4 * nk) {
                const int c = (int)(skey[j >> 2] & (TK_MAX_LINES - 1)), col = j & 3;
                const double half = m.cwid[c] / 2.0, cen = m.ccen[c];
                const double l = sf_unordered(m.clo[c]), h = sf_unordered(m.chi[c]);
                const bool horizontal = m.cmeta[c] & 2;
                const double across = (col & 2) ? cen + half : cen - half, along = (col & 2) ? h : l;
                v = ((col & 1) != 0) == horizontal ? across : along;           // horizontal: x along, y across; vertical: x across
            }
            s.faces_out[(size_t)b * 4 * max_faces + j] = v;
        }
    if (s.faceviews_out)
        for (int j = tid; j < max_faces; j += TK_THREADS)
            s.faceviews_out[(size_t)b * max_faces + j] = j < nk ? (uint8_t)((skey[j] >> TK_VIEW_SHIFT) & 0xff) : (uint8_t)0;
    if (tid == 0) {
        if (s.n_faces_out) s.n_faces_out[b] = nk;
        s.flags_out[b] = flags;
    }
}
