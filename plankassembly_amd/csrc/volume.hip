// Assembly volume for gfx950: one launch reads a list of pairs of token rows as pairs of solids - the
// unions of their planks - and writes, per pair, the volume of each union, of the two together and of the planks on their own,
// with the counts of solid planks: eight exact int64.  The core is csrc/volume_core.h, shared with the host program of
// tools/volume_host; tests/volume_reference.py holds the restatement and the voxel oracle it is pinned to.
//
// One block of 256 threads per pair.  Both rows go once into LDS as clamped int16 tokens (coalesced, the END search rides on
// the same pass); thread t takes plank t + 1 of each side into registers, the solid ones are numbered by ballot and ranked by
// z_lo into one box list of at most 340 boxes with a side mark.  The x and the y bounds of the boxes are ranked into sorted
// order (at most 680 each); thread j builds the bit row of y slab j over the boxes that span it.  Then the x slabs are dealt
// over the threads, 256 / slabs threads to a slab (one from 129 slabs on): a thread builds the slab's bit row in its own LDS
// words and sweeps its share of the slab's columns - per column one AND per word, the set bits in ascending (= z_lo) order,
// three running interval ends - into three int64 sums.  The block reduces and thread 0 writes the eight results.  Plain stores
// only, no atomics, no global scratch, no allocation, no synchronisation with the host: the launch captures into a graph like
// every other entry point.
//
// LDS: requested per launch from pv_layout.  Of the two bit-row tables the design could hold (x slabs and y slabs, 32.6 KB each
// at 170 planks a side, 65 KB together) only the y table is kept; an x slab's row is rebuilt by each thread that takes the slab
// (12 KB for the block at the cap).  So the largest launch needs 58 000 bytes, under the 64 KB a block gets without opting in,
// and a Tmax-128 launch (21 planks a side) 4 512 bytes.
#include "pa_device.h"
#include "volume_core.h"
#include "../../include/plank_hip.h"

namespace {

#define ST(s) reinterpret_cast<hipStream_t>(s)

constexpr int PV_WAVES = PV_THREADS / 64;
static_assert(PM_MAX_LEN == PA_MATCH_MAX_LEN, "the header's limit is the core's");
static_assert(PM_MAX_PLANKS <= PV_THREADS, "one thread per plank of a side");
static_assert(PV_OUT == 8, "out is [n_pairs][8]");

struct VolumeArgs {
    const int64_t* seq[2];
    int64_t stride[2];
    const int32_t* pair[2];
    int32_t len[2];
    int32_t end_token;
    int64_t* out;
};

__device__ __forceinline__ int pv_wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ long long pv_wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// What a thread keeps of the plank it took from one side.
struct PvHeld { int32_t b0, b1, b2, b3, b4, b5; int pos; bool solid; };

// One row -> its clamped tokens in tok[0 .. len), plank tid + 1 in `h` with its number h.pos among the solid planks so far, its
// z_lo in zkey[h.pos].  Returns the number of solid planks so far (uniform).  Called by the whole block; cnt is free on return.
__device__ __forceinline__ int pv_load_side(const int64_t* __restrict__ row, int len, int end_token, int16_t* tok, int16_t* zkey,
                                            int32_t* cnt, int n0, PvHeld* h) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int first = len;
    for (int i = tid; i < len; i += PV_THREADS) {
        const int64_t t = row[i];
        tok[i] = (int16_t)pm_coord(t);
        if (t == (int64_t)end_token && first == len) first = i;          // i only grows: the thread's first END
    }
    first = pv_wave_min(first);
    if (lane == 0) cnt[wave] = first;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < PV_WAVES; ++w) first = cnt[w] < first ? cnt[w] : first;
    __syncthreads();                                                      // cnt is read: it is written again below
    const int planks = first / PM_DOF;                                    // plank 0 included; <= PM_MAX_PLANKS + 1
    const int p = tid + 1;
    h->b0 = h->b1 = h->b2 = h->b3 = h->b4 = h->b5 = 0;
    if (p < planks) {
        const int16_t* s = tok + PM_DOF * p;                              // 6 p + 5 < 6 planks <= first <= len
        h->b0 = s[0]; h->b1 = s[1]; h->b2 = s[2]; h->b3 = s[3]; h->b4 = s[4]; h->b5 = s[5];
    }
    const int32_t box[PM_DOF] = {h->b0, h->b1, h->b2, h->b3, h->b4, h->b5};
    h->solid = p < planks && pv_solid(box);
    const unsigned long long m = __ballot(h->solid);
    if (lane == 0) cnt[wave] = __popcll(m);
    __syncthreads();
    int before = n0, total = n0;
#pragma unroll
    for (int w = 0; w < PV_WAVES; ++w) { before += w < wave ? cnt[w] : 0; total += cnt[w]; }
    h->pos = before + __popcll(m & ((1ull << lane) - 1ull));              // < total <= n0 + planks - 1: inside the side's share of cap
    if (h->solid) zkey[h->pos] = (int16_t)h->b2;
    __syncthreads();
    return total;
}

__device__ __forceinline__ void pv_place(const PvHeld& h, int side, const int16_t* zkey, int n, int16_t* box) {
    if (!h.solid) return;
    int16_t* d = box + PV_BOX * pv_rank(zkey, 1, n, h.pos);               // a permutation of 0 .. n - 1
    d[0] = (int16_t)h.b0; d[1] = (int16_t)h.b1; d[2] = (int16_t)h.b2; d[3] = (int16_t)h.b3; d[4] = (int16_t)h.b4; d[5] = (int16_t)h.b5;
    d[6] = (int16_t)side; d[7] = 0;
}

__global__ __launch_bounds__(PV_THREADS) void plank_volume_kernel(VolumeArgs g) {
    extern __shared__ __align__(16) unsigned char mem[];
    const PvLayout l = pv_layout(g.len[0], g.len[1]);
    int16_t* tok = reinterpret_cast<int16_t*>(mem + l.tok);
    int16_t* zkey = reinterpret_cast<int16_t*>(mem + l.zkey);
    int16_t* box = reinterpret_cast<int16_t*>(mem + l.box);
    int16_t* xs = reinterpret_cast<int16_t*>(mem + l.xs);
    int16_t* ys = reinterpret_cast<int16_t*>(mem + l.ys);
    uint64_t* rowy = reinterpret_cast<uint64_t*>(mem + l.rowy);
    uint64_t* rowx = reinterpret_cast<uint64_t*>(mem + l.rowx);
    int64_t* red = reinterpret_cast<int64_t*>(mem + l.red);
    int32_t* cnt = reinterpret_cast<int32_t*>(mem + l.cnt);

    const int pair = blockIdx.x, tid = threadIdx.x;
    PvHeld ha, hb;
    const int64_t ra = g.pair[0] ? (int64_t)g.pair[0][pair] : (int64_t)pair;
    const int na = pv_load_side(g.seq[0] + ra * g.stride[0], g.len[0], g.end_token, tok, zkey, cnt, 0, &ha);
    int n = na;
    hb.solid = false;
    if (g.seq[1]) {                                                        // uniform
        const int64_t rb = g.pair[1] ? (int64_t)g.pair[1][pair] : (int64_t)pair;
        n = pv_load_side(g.seq[1] + rb * g.stride[1], g.len[1], g.end_token, tok + g.len[0], zkey, cnt, na, &hb);
    }

    // ---- the box list in z_lo order; the planks' own volumes
    pv_place(ha, 0, zkey, n, box);
    pv_place(hb, 1, zkey, n, box);
    long long sums[5] = {0, 0, 0, 0, 0};                                   // union_a, union_b, union_ab, sum_a, sum_b
    if (ha.solid) sums[3] = (long long)(ha.b3 - ha.b0) * (ha.b4 - ha.b1) * (ha.b5 - ha.b2);
    if (hb.solid) sums[4] = (long long)(hb.b3 - hb.b0) * (hb.b4 - hb.b1) * (hb.b5 - hb.b2);
    __syncthreads();

    // ---- the sorted bounds of x and y (2 n <= l.bounds each)
    for (int e = tid; e < 2 * n; e += PV_THREADS) {
        xs[pv_bound_rank(box, n, 0, e)] = pv_bound(box, n, 0, e);
        ys[pv_bound_rank(box, n, 1, e)] = pv_bound(box, n, 1, e);
    }
    __syncthreads();

    // ---- the y slabs' bit rows (slab j < 2 n - 1 <= l.bounds - 1)
    for (int j = tid; j + 1 < 2 * n; j += PV_THREADS) {
        if (ys[j + 1] > ys[j]) pv_slab_row(box, n, l.words, 1, ys[j], ys[j + 1], rowy + j * l.words, 1);
        else for (int w = 0; w < l.words; ++w) rowy[j * l.words + w] = 0;
    }
    __syncthreads();

    // ---- the x slabs: `share` threads to a slab, each with the slab's row in its own words (word w of this thread's row is
    // rowx[w * PV_THREADS + tid]) and every share-th y slab; one thread to a slab once there are 129 slabs or more
    int64_t vol3[3] = {0, 0, 0};
    const int slabs = 2 * n - 1;                                           // uniform; < 1 without two bounds
    const int share = slabs > 0 && slabs < PV_THREADS ? PV_THREADS / slabs : 1;
    const int teams = PV_THREADS / share;                                  // teams * share <= PV_THREADS: the threads beyond idle
    if (tid < teams * share)
        for (int i = tid / share; i < slabs; i += teams)
            pv_x_slab(box, n, l.words, xs, ys, rowy, i, tid % share, share, rowx + tid, PV_THREADS, vol3);
    sums[0] = vol3[0]; sums[1] = vol3[1]; sums[2] = vol3[2];

#pragma unroll
    for (int q = 0; q < 5; ++q) sums[q] = pv_wave_sum(sums[q]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 5; ++q) red[(tid >> 6) * 5 + q] = sums[q];
    }
    __syncthreads();
    if (tid == 0) {
        int64_t t[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) t[q] = red[q] + red[5 + q] + red[10 + q] + red[15 + q];
        pv_results(t[0], t[3], t[1], t[4], t[2], na, n - na, g.out + (int64_t)pair * PV_OUT);
    }
}

}  // namespace

extern "C" int pa_plank_volume(const int64_t* seq_a, int64_t stride_a, int32_t len_a, const int64_t* seq_b, int64_t stride_b,
                               int32_t len_b, const int32_t* pair_a, const int32_t* pair_b, int32_t n_pairs, int32_t end_token,
                               int32_t dof, int64_t* out, void* stream) {
    if (!seq_b) { stride_b = 0; len_b = 0; }                               // every b side is empty: its len and stride are not read
    if (!seq_a || !out || n_pairs < 0 || stride_a < 0 || stride_b < 0 || len_a < 0 || len_b < 0) return PA_EINVAL;
    if ((pair_a == nullptr) != (pair_b == nullptr)) return PA_EINVAL;
    if (dof != PM_DOF) return PA_ESHAPE;
    if (len_a > PM_MAX_LEN || len_b > PM_MAX_LEN) return PA_ESHAPE;
    if (n_pairs == 0) return 0;
    VolumeArgs g;
    g.seq[0] = seq_a; g.seq[1] = seq_b; g.stride[0] = stride_a; g.stride[1] = stride_b; g.pair[0] = pair_a; g.pair[1] = pair_b;
    g.len[0] = len_a; g.len[1] = len_b; g.end_token = end_token; g.out = out;
    const PvLayout l = pv_layout(len_a, len_b);
    PA_LAUNCH(plank_volume_kernel, dim3((unsigned)n_pairs), dim3(PV_THREADS), (size_t)l.bytes, ST(stream), g);
    return 0;
}
