// The three-view line drawing from the planks, on the device: included by tokenise.hip, inside its
// namespace, after the stages it shares with tokenise_kernel.  One block of 256 threads per batch row, one launch per batch:
// hidden-line rendering of the row's planks, the line noise (the line kind's draws, keyed by the canonical line number), tokens.
// What it restates: plankassembly_amd/datasets.py `render_drawing` (reference dataset/data_utils.py:49-205: HLR of a compound of
// boxes, then noding) for axis-aligned boxes seen along the axes - float64 compares only, no arithmetic on a coordinate but the
// exact negation of the view table.
//
// One view at a time, on its compressed grid: the distinct rectangle coordinates of each 2D axis are ranked by counting (at most
// 2 * RD_MAX_PLANKS per axis), every box becomes a rank rectangle with the rank of its near-face depth.  cell[i][j]: the nearest
// depth rank of the boxes covering the cell.  A unit piece of a grid line is present where a rectangle's boundary covers it; its
// depth d* is the nearest such rectangle's, and it is hidden iff the cells on both of its sides are strictly nearer than d* (the
// per-segment rule of section 27; a box's far-face edges lie under its near-face edges, so they never decide).  A grid point on a
// line is a node where a perpendicular piece is incident.  One thread per grid line counts, then writes, its runs between nodes.
// Every loop is bounded by a count known on entry.
//
// LDS at RD_MAX_PLANKS = 32, PA_TOKENISE_MAX_LINES = 1024:
//   raw 32 KB + can 32 KB + their view / type bytes 4 KB                              68 KB   the lines, as emitted and in canonical order
//   cell 4 KB + hp 4 KB + vp 4 KB                                                     12 KB   the compressed grid of one view
//   box3 1.5 KB + 5 x 256 B rectangles + us / vs 1 KB + ranks, counts, offsets ~1.5 KB  5 KB
//   key 8 + skey 8 + selh 4 + spos 2 KB (tokenise_kernel's own)                       22 KB
//   total 107 KB of the 160 KB a gfx950 workgroup may take; one block per CU, as sideface_kernel.

constexpr int RD_MAX_PLANKS = PA_RENDER_MAX_PLANKS;
constexpr int RD_GRID = 2 * RD_MAX_PLANKS;            // distinct coordinates per 2D axis, at most
static_assert(RD_GRID == 64, "the grid arrays are indexed with shifts by 6");
static_assert(6 * RD_MAX_PLANKS <= TK_THREADS && 5 * RD_MAX_PLANKS <= TK_THREADS, "one thread per coordinate of the row");
enum { RD_OUT_OF_DOMAIN = 1, RD_TRUNCATED = 2, RD_DEGENERATE = 8, RD_OVERFLOW = 16 };

struct RdArgs {
    TkArgs t;
    const int32_t* plank_cnt;
    int32_t skip_first;
    double* lines_out; uint8_t* views_out; uint8_t* types_out; int32_t* n_lines_out; int32_t* flags_out;
};

// (view, xmin, ymin, xmax, ymax) of line j before that of line i
__device__ __forceinline__ bool rd_less(const double* ln, const uint8_t* lv, int j, int i) {
    const double* p = ln + 4 * j;
    const double* q = ln + 4 * i;
    bool less = false;
    less = p[3] != q[3] ? p[3] < q[3] : less;
    less = p[2] != q[2] ? p[2] < q[2] : less;
    less = p[1] != q[1] ? p[1] < q[1] : less;
    less = p[0] != q[0] ? p[0] < q[0] : less;
    less = lv[j] != lv[i] ? lv[j] < lv[i] : less;
    return less;
}

__global__ __launch_bounds__(TK_THREADS) void render_kernel(RdArgs r) {
    __shared__ double raw[TK_MAX_LINES * 4], can[TK_MAX_LINES * 4];
    __shared__ uint8_t rawv[TK_MAX_LINES], rawt[TK_MAX_LINES], canv[TK_MAX_LINES], cant[TK_MAX_LINES];
    __shared__ uint8_t cell[RD_GRID * RD_GRID], hp[RD_GRID * RD_GRID], vp[RD_GRID * RD_GRID];
    __shared__ double box3[RD_MAX_PLANKS * 6];
    __shared__ double bu0[RD_MAX_PLANKS], bv0[RD_MAX_PLANKS], bu1[RD_MAX_PLANKS], bv1[RD_MAX_PLANKS], bnear[RD_MAX_PLANKS];
    __shared__ double us[RD_GRID], vs[RD_GRID];
    __shared__ uint8_t bvalid[RD_MAX_PLANKS], bdep[RD_MAX_PLANKS];
    __shared__ uint8_t ru[RD_GRID], rv[RD_GRID];       // rank of u0 / u1 (v0 / v1) of box k at 2k / 2k + 1
    __shared__ uint8_t firstu[RD_GRID], firstv[RD_GRID];
    __shared__ int cnt[2 * RD_GRID];
    __shared__ int poff[2];
    __shared__ uint64_t key[TK_MAX_LINES], skey[TK_MAX_LINES];
    __shared__ uint32_t selh[TK_MAX_LINES];
    __shared__ uint16_t spos[TK_MAX_LINES];

    TkArgs a = r.t;                                    // seg / type / plank_off are pointed at the block's own arrays below
    const int b = blockIdx.x, tid = threadIdx.x;
    const int d = a.index[b];
    const bool have = d >= 0 && d < a.N;
    const int plo = have ? a.plank_off[d] : 0;
    int np = have ? (r.plank_cnt ? r.plank_cnt[d] : a.plank_off[d + 1] - plo) : 0;
    np = np < 0 ? 0 : np;
    const int skip = r.skip_first ? 1 : 0;
    int flags = 0;
    int nb = np - skip;                                // the boxes to render
    nb = nb < 0 ? 0 : nb;
    if (nb > RD_MAX_PLANKS - skip) { nb = RD_MAX_PLANKS - skip; flags |= RD_TRUNCATED; }      // (the entry refuses such a set)
    const double rq = (double)((1 << a.n_bits) - 1);
    int max_lines = (a.S - 1) >> 2;                    // what fits the row
    max_lines = max_lines < 0 ? 0 : max_lines;

    // ---- the row's boxes, -0.0 -> 0.0; the domain
    bool bad = false;
    if (tid < 6 * nb) {
        const double v = a.coords[(size_t)(plo + skip) * 6 + tid] + 0.0;
        bad = !(v >= -1.0 && v <= 1.0);                // NaN and the infinities too
        box3[tid] = v;
    }
    if (__syncthreads_count(bad)) { flags |= RD_OUT_OF_DOMAIN; nb = 0; }
    bool degenerate = false;
    if (tid < nb) {
        const double* c = box3 + 6 * tid;
        const bool ok = c[0] < c[3] && c[1] < c[4] && c[2] < c[5];
        bvalid[tid] = ok;
        degenerate = !ok;
    }
    if (__syncthreads_count(degenerate)) flags |= RD_DEGENERATE;

    int total = 0;                                     // lines emitted so far (may pass TK_MAX_LINES: only the first are stored)
    for (int view = 0; view < 3; ++view) {
        // ---- THE view table (section 27): view 0 (x, -z) smaller y nearer; 1 (x, -y) larger z nearer; 2 (y, -z) larger x nearer
        const int ua = view == 2 ? 1 : 0, va = view == 1 ? 1 : 2, da = view == 0 ? 1 : (view == 1 ? 2 : 0);
        if (tid < nb) {
            const double* c = box3 + 6 * tid;
            bu0[tid] = c[ua]; bu1[tid] = c[ua + 3];
            bv0[tid] = -c[va + 3] + 0.0; bv1[tid] = -c[va] + 0.0;
            bnear[tid] = view == 0 ? -c[da] : c[da + 3];                       // nearness of the near face: larger = nearer
        }
        __syncthreads();
        // ---- ranks by counting: threads 0 .. 63 the u coordinates, 64 .. 127 the v coordinates, 128 .. the near depths
        const int e = tid & (RD_GRID - 1), ek = e >> 1;
        const bool isu = tid < RD_GRID, isv = tid >= RD_GRID && tid < 2 * RD_GRID;
        const bool live = (isu || isv) && ek < nb && bvalid[ek];
        double mine = 0.0;
        bool first = false;
        if (live) {
            mine = isu ? ((e & 1) ? bu1[ek] : bu0[ek]) : ((e & 1) ? bv1[ek] : bv0[ek]);
            first = true;
            for (int g = 0; g < e; ++g) {
                const int gk = g >> 1;
                if (!bvalid[gk]) continue;
                const double other = isu ? ((g & 1) ? bu1[gk] : bu0[gk]) : ((g & 1) ? bv1[gk] : bv0[gk]);
                if (other == mine) first = false;
            }
            (isu ? firstu : firstv)[e] = first;
        }
        const int nu = __syncthreads_count(isu && first);
        const int nv = __syncthreads_count(isv && first);
        if (live) {
            int rank = 0;                                                       // distinct values below mine
            for (int g = 0; g < 2 * nb; ++g) {
                const int gk = g >> 1;
                if (!bvalid[gk] || !(isu ? firstu : firstv)[g]) continue;
                const double other = isu ? ((g & 1) ? bu1[gk] : bu0[gk]) : ((g & 1) ? bv1[gk] : bv0[gk]);
                rank += other < mine;
            }
            (isu ? ru : rv)[e] = (uint8_t)rank;
            if (first) (isu ? us : vs)[rank] = mine;
        }
        if (tid >= 2 * RD_GRID && tid - 2 * RD_GRID < nb) {
            const int k = tid - 2 * RD_GRID;
            int below = 0;
            for (int g = 0; g < nb; ++g) below += bvalid[g] && bnear[g] < bnear[k];
            bdep[k] = (uint8_t)(below + 1);                                     // 0 is "no box"; equal depths get equal ranks
        }
        __syncthreads();
        // ---- the nearest depth rank over every cell (i, j): us[i] .. us[i + 1] x vs[j] .. vs[j + 1]
        for (int c = tid; c < RD_GRID * RD_GRID; c += TK_THREADS) {
            const int i = c >> 6, j = c & (RD_GRID - 1);
            int m = 0;
            if (i < nu - 1 && j < nv - 1)
                for (int k = 0; k < nb; ++k)
                    if (bvalid[k] && ru[2 * k] <= i && i < ru[2 * k + 1] && rv[2 * k] <= j && j < rv[2 * k + 1]) m = bdep[k] > m ? bdep[k] : m;
            cell[c] = (uint8_t)m;
        }
        __syncthreads();
        // ---- unit pieces: 0 absent, 1 visible, 2 hidden.  hp[j][i]: us[i] .. us[i + 1] at vs[j]; vp[i][j]: vs[j] .. vs[j + 1] at us[i]
        for (int c = tid; c < RD_GRID * RD_GRID; c += TK_THREADS) {
            const int hi = c >> 6, lo = c & (RD_GRID - 1);
            int hd = 0, vd = 0;                                                 // d* of the horizontal piece (line hi, piece lo), the vertical
            if (lo < nu - 1 && hi < nv)
                for (int k = 0; k < nb; ++k)
                    if (bvalid[k] && (rv[2 * k] == hi || rv[2 * k + 1] == hi) && ru[2 * k] <= lo && lo < ru[2 * k + 1])
                        hd = bdep[k] > hd ? bdep[k] : hd;
            if (lo < nv - 1 && hi < nu)
                for (int k = 0; k < nb; ++k)
                    if (bvalid[k] && (ru[2 * k] == hi || ru[2 * k + 1] == hi) && rv[2 * k] <= lo && lo < rv[2 * k + 1])
                        vd = bdep[k] > vd ? bdep[k] : vd;
            int hs = 0, vst = 0;
            if (hd) {                                                           // cells above (lo, hi) and below (lo, hi - 1)
                const int above = hi < nv - 1 ? cell[(lo << 6) + hi] : 0, below = hi > 0 ? cell[(lo << 6) + hi - 1] : 0;
                hs = above > hd && below > hd ? 2 : 1;
            }
            if (vd) {                                                           // cells right (hi, lo) and left (hi - 1, lo)
                const int right = hi < nu - 1 ? cell[(hi << 6) + lo] : 0, left = hi > 0 ? cell[((hi - 1) << 6) + lo] : 0;
                vst = right > vd && left > vd ? 2 : 1;
            }
            hp[c] = (uint8_t)hs;
            vp[c] = (uint8_t)vst;
        }
        __syncthreads();
        // ---- one thread per grid line: threads 0 .. nv - 1 the horizontal lines, 64 .. 64 + nu - 1 the vertical ones
        const bool hline = tid < nv, vline = tid >= RD_GRID && tid < RD_GRID + nu;
        const int line = tid & (RD_GRID - 1);
        const uint8_t* mine_p = (hline ? hp : vp) + (line << 6);               // this line's pieces
        const uint8_t* cross_p = hline ? vp : hp;                               // cross_p[p][line - 1], [p][line]: the pieces meeting point p
        const int pieces = (hline ? nu : nv) - 1, cross_lines = hline ? nv : nu;
        for (int pass = 0; pass < 2; ++pass) {                                  // count, then write
            int runs = 0, start = 0, at = 0;
            if (pass == 1 && (hline || vline))
                for (int g = 0; g < tid; ++g) at += cnt[g];
            if (hline || vline)
                for (int p = 0; p <= pieces; ++p) {
                    const bool present = p < pieces && mine_p[p] != 0;
                    const bool before = p > 0 && mine_p[p - 1] != 0;
                    const bool node = (line > 0 && cross_p[(p << 6) + line - 1] != 0) || (line < cross_lines - 1 && cross_p[(p << 6) + line] != 0);
                    if (before && (!present || node)) {                         // the run start .. p ends at point p
                        const int slot = total + at + runs;
                        if (pass == 1 && slot < TK_MAX_LINES) {
                            const double along0 = (hline ? us : vs)[start], along1 = (hline ? us : vs)[p], across = (hline ? vs : us)[line];
                            double* o = raw + 4 * slot;
                            o[0] = hline ? along0 : across; o[1] = hline ? across : along0;
                            o[2] = hline ? along1 : across; o[3] = hline ? across : along1;
                            rawv[slot] = (uint8_t)view;
                            rawt[slot] = (uint8_t)(mine_p[start] == 2);
                        }
                        ++runs;
                    }
                    if (present && (!before || node)) start = p;
                }
            if (pass == 0) {
                if (tid < 2 * RD_GRID) cnt[tid] = runs;
                __syncthreads();
            }
        }
        int emitted = 0;
        for (int g = 0; g < 2 * RD_GRID; ++g) emitted += cnt[g];
        total += emitted;
        __syncthreads();                                                        // the next view reuses the grid and cnt
    }

    // ---- the canonical order (view, xmin, ymin, xmax, ymax): distinct atomic segments are distinct tuples
    int n = total;
    if (n > TK_MAX_LINES) { n = TK_MAX_LINES; flags |= RD_TRUNCATED | RD_OVERFLOW; }     // beyond the sort keys: the first emitted stay
    for (int i = tid; i < n; i += TK_THREADS) {
        int below = 0;
        for (int j = 0; j < n; ++j) below += rd_less(raw, rawv, j, i);
        can[4 * below] = raw[4 * i]; can[4 * below + 1] = raw[4 * i + 1]; can[4 * below + 2] = raw[4 * i + 2]; can[4 * below + 3] = raw[4 * i + 3];
        canv[below] = rawv[i];
        cant[below] = rawt[i];
    }
    __syncthreads();
    double* ln = can;
    uint8_t* lv = canv;
    uint8_t* lt = cant;
    // ---- the capacity: the lines that sort first in the order of the row's tokens stay, renumbered in canonical order
    if (n > max_lines) {
        flags |= RD_TRUNCATED;
        for (int i = tid; i < n; i += TK_THREADS) {
            key[i] = tk_key(lv[i], ln[4 * i], ln[4 * i + 1], ln[4 * i + 2], ln[4 * i + 3], rq, i);
            selh[i] = 0;
        }
        __syncthreads();
        tk_rank(key, skey, spos, n);
        for (int j = tid; j < max_lines; j += TK_THREADS) selh[skey[j] & (TK_MAX_LINES - 1)] = 1;
        __syncthreads();
        for (int i = tid; i < n; i += TK_THREADS)
            if (selh[i]) {
                int dst = 0;
                for (int j = 0; j < i; ++j) dst += selh[j] != 0;
                raw[4 * dst] = ln[4 * i]; raw[4 * dst + 1] = ln[4 * i + 1]; raw[4 * dst + 2] = ln[4 * i + 2]; raw[4 * dst + 3] = ln[4 * i + 3];
                rawv[dst] = lv[i];
                rawt[dst] = lt[i];
            }
        __syncthreads();
        ln = raw; lv = rawv; lt = rawt;
        n = max_lines;
    }

    // ---- noise and tokens, as tokenise_kernel: the block's lines are the drawing's segments (xmin, ymin) -> (xmax, ymax)
    a.seg = ln;
    a.type = lt;
    uint32_t base;
    int num_select;
    const bool augmented = tk_draws(a, d, n, selh, base, num_select);
    for (int i = tid; i < n; i += TK_THREADS) {
        double x0 = ln[4 * i], y0 = ln[4 * i + 1], x1 = ln[4 * i + 2], y1 = ln[4 * i + 3];
        bool kept = true;
        if (augmented) {
            double sx0, sy0, sx1, sy1;
            kept = tk_noisy_segment(a, 0, i, n, selh, num_select, base, sx0, sy0, sx1, sy1);
            x0 = sx0 < sx1 ? sx0 : sx1; x1 = sx0 < sx1 ? sx1 : sx0;
            y0 = sy0 < sy1 ? sy0 : sy1; y1 = sy0 < sy1 ? sy1 : sy0;
        }
        key[i] = kept ? tk_key(lv[i], x0, y0, x1, y1, rq, i) : TK_DELETED;
    }
    if (tid == 0) { poff[0] = plo; poff[1] = plo + np; }
    __syncthreads();
    const int nk = tk_rank(key, skey, spos, n);
    tk_store_inputs(a, b, 0, skey, spos, nk);
    if (a.out_value) {
        a.plank_off = poff;                                                     // the row's planks, whichever way they were counted
        tk_store_outputs(a, b, 0, have, rq);
    }

    // ---- the rendered lines before the noise, in canonical order
    if (r.lines_out)
        for (int j = tid; j < 4 * max_lines; j += TK_THREADS) r.lines_out[(size_t)b * 4 * max_lines + j] = j < 4 * n ? ln[j] : 0.0;
    if (r.views_out)
        for (int j = tid; j < max_lines; j += TK_THREADS) r.views_out[(size_t)b * max_lines + j] = j < n ? lv[j] : (uint8_t)0;
    if (r.types_out)
        for (int j = tid; j < max_lines; j += TK_THREADS) r.types_out[(size_t)b * max_lines + j] = j < n ? lt[j] : (uint8_t)0;
    if (tid == 0) {
        if (r.n_lines_out) r.n_lines_out[b] = n;
        r.flags_out[b] = flags;
    }
}
