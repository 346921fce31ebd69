// On-device plank matching for gfx950: one launch scores a list of pairs of token rows as sets of planks -
// tp = the maximum matching over IoU > threshold, the two plank counts, and the number of pairs at IoU == threshold exactly.
// What it restates: plankassembly_amd/metric.py `pairwise_iou_3d` + `HungarianMatcher` behind the trainers' box pipeline
// (`parse_sequence`, row 0 dropped, `_valid_pred`; reference third_party/matcher.py:29-61, trainer_complete.py:78-80); the core is
// csrc/match_core.h, shared with the host program of tools/match_host; tests/match_reference.py is the restatement it is pinned to.
//
// One wave (a 64-thread block) per pair.  Both rows go once into LDS as clamped int32 tokens (coalesced, the END search rides
// on the same pass); the kept planks are compacted in place, 64 at a time, by ballot; lane i builds the adjacency bit rows of
// planks i, i + 64, ... of side a; lane 0 runs the iterative augmenting-path search over them.  Plain stores only, no atomics,
// no allocation, no synchronisation with the host: the launch captures into a graph like every other entry point.
#include "pa_device.h"
#include "match_core.h"
#include "../../include/plank_hip.h"

#pragma clang fp contract(off)          // this whole file: the IoU quotient is one division of two exactly converted integers

namespace {

#define ST(s) reinterpret_cast<hipStream_t>(s)

constexpr int PM_THREADS = 64;
static_assert(PM_MAX_LEN == PA_MATCH_MAX_LEN, "the header's limit is the core's");

struct MatchArgs {
    const int64_t* seq_a; const int64_t* seq_b;
    int64_t stride_a, stride_b;
    const int32_t* pair_a; const int32_t* pair_b;
    int32_t len_a, len_b, end_token, filter_a, filter_b;
    double threshold;
    int32_t* out;
};

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// One row -> the kept planks as int32 boxes tok[6 s .. 6 s + 5], s < n (returned; uniform across the wave).
__device__ __forceinline__ int load_side(const int64_t* __restrict__ row, int len, int end_token, int filter, int32_t* tok,
                                         int lane) {
    int first = len;
    for (int i = lane; i < len; i += PM_THREADS) {
        const int64_t t = row[i];
        tok[i] = pm_coord(t);
        if (t == (int64_t)end_token && first == len) first = i;          // i only grows: the lane's first END
    }
    first = wave_min(first);
    __syncthreads();
    const int planks = first / PM_DOF;                                    // plank 0 included; trailing tokens ignored
    int n = 0;
    for (int base = 1; base < planks; base += PM_THREADS) {               // uniform trip count
        const int p = base + lane;
        const bool have = p < planks;
        int32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0, b5 = 0;
        if (have) {
            const int32_t* s = tok + PM_DOF * p;                          // 6 p + 5 < 6 planks <= first <= len
            b0 = s[0]; b1 = s[1]; b2 = s[2]; b3 = s[3]; b4 = s[4]; b5 = s[5];
        }
        const int32_t box[PM_DOF] = {b0, b1, b2, b3, b4, b5};
        const bool keep = have && pm_keep(box, filter);
        const unsigned long long m = __ballot(keep);
        const int pos = n + __popcll(m & ((1ull << lane) - 1ull));        // pos <= p - 1
        __syncthreads();                                                  // every read of this chunk is done
        if (keep) {
            int32_t* d = tok + PM_DOF * pos;                              // below token 6 (base + 63): the next chunk starts above
            d[0] = b0; d[1] = b1; d[2] = b2; d[3] = b3; d[4] = b4; d[5] = b5;
        }
        n += __popcll(m);
        __syncthreads();
    }
    return n;
}

__global__ __launch_bounds__(PM_THREADS) void plank_match_kernel(MatchArgs g) {
    extern __shared__ __align__(16) unsigned char mem[];
    const PmLayout l = pm_layout(g.len_a, g.len_b);
    uint64_t* adj = reinterpret_cast<uint64_t*>(mem + l.adj);
    int32_t* tok_a = reinterpret_cast<int32_t*>(mem + l.tok_a);
    int32_t* tok_b = reinterpret_cast<int32_t*>(mem + l.tok_b);

    const int pair = blockIdx.x, lane = threadIdx.x;
    const int64_t ra = g.pair_a ? (int64_t)g.pair_a[pair] : (int64_t)pair;
    const int64_t rb = g.pair_b ? (int64_t)g.pair_b[pair] : (int64_t)pair;
    const int na = load_side(g.seq_a + ra * g.stride_a, g.len_a, g.end_token, g.filter_a, tok_a, lane);
    const int nb = load_side(g.seq_b + rb * g.stride_b, g.len_b, g.end_token, g.filter_b, tok_b, lane);

    // ---- adjacency: lane i owns planks i, i + 64, ... of side a; the planks of b are LDS broadcasts
    int ties = 0;
    for (int i = lane; i < na; i += PM_THREADS) {                          // na <= cap_a
        const int32_t* s = tok_a + PM_DOF * i;
        const int32_t a[PM_DOF] = {s[0], s[1], s[2], s[3], s[4], s[5]};
        for (int w = 0; w < l.words; ++w) {
            uint64_t bits = 0;
            const int hi = nb < w * 64 + 64 ? nb : w * 64 + 64;            // nb <= cap_b <= 64 * words
            for (int j = w * 64; j < hi; ++j) {
                const int32_t* t = tok_b + PM_DOF * j;
                const int32_t b[PM_DOF] = {t[0], t[1], t[2], t[3], t[4], t[5]};
                const int e = pm_edge(a, b, g.threshold);
                bits |= (uint64_t)(e & 1) << (j - w * 64);
                ties += e >> 1;
            }
            adj[i * l.words + w] = bits;
        }
    }
    ties = wave_sum(ties);
    __syncthreads();

    // ---- the matching: one lane, iterative, every array in LDS
    if (lane == 0) {
        const int tp = pm_match(adj, na, nb, l.words, reinterpret_cast<int16_t*>(mem + l.match_b),
                                reinterpret_cast<int16_t*>(mem + l.stk_a), reinterpret_cast<int16_t*>(mem + l.stk_j),
                                reinterpret_cast<uint64_t*>(mem + l.visited), reinterpret_cast<uint64_t*>(mem + l.taken));
        int32_t* o = g.out + (int64_t)pair * 4;
        o[0] = tp; o[1] = na; o[2] = nb; o[3] = ties;
    }
}

}  // namespace

extern "C" int pa_plank_match(const int64_t* seq_a, int64_t stride_a, int32_t len_a, const int64_t* seq_b, int64_t stride_b,
                              int32_t len_b, const int32_t* pair_a, const int32_t* pair_b, int32_t n_pairs, int32_t end_token,
                              int32_t dof, int32_t filter_a, int32_t filter_b, double threshold, int32_t* out, void* stream) {
    if (!seq_a || !seq_b || !out || n_pairs < 0 || stride_a < 0 || stride_b < 0) return PA_EINVAL;
    if ((pair_a == nullptr) != (pair_b == nullptr)) return PA_EINVAL;
    if (!(threshold == threshold) || threshold == 0.0) return PA_EINVAL;       // the reference's "threshold cant be 0"; NaN
    if (dof != PM_DOF) return PA_ESHAPE;
    if (len_a < 0 || len_b < 0 || len_a > PM_MAX_LEN || len_b > PM_MAX_LEN) return PA_ESHAPE;
    if (n_pairs == 0) return 0;
    MatchArgs g;
    g.seq_a = seq_a; g.seq_b = seq_b; g.stride_a = stride_a; g.stride_b = stride_b; g.pair_a = pair_a; g.pair_b = pair_b;
    g.len_a = len_a; g.len_b = len_b; g.end_token = end_token; g.filter_a = filter_a != 0; g.filter_b = filter_b != 0;
    g.threshold = threshold; g.out = out;
    const PmLayout l = pm_layout(len_a, len_b);
    PA_LAUNCH(plank_match_kernel, dim3((unsigned)n_pairs), dim3(PM_THREADS), (size_t)l.bytes, ST(stream), g);
    return 0;
}
