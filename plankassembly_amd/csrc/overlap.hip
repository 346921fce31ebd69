// Line-set overlap for gfx950: one launch compares a list of pairs of encoder rows as sets of axis-aligned
// lines - how much of the length of each side's lines the other side's lines cover within `tol` quantisation levels, both ways,
// with the lengths and the counts of kept and skipped lines.  What it reads: the encoder rows of the batch contract
// (plankassembly_amd/datasets.py `prepare_input_sequence`; reference line_data.py:34-83), as the dataset or pa_render_drawings
// wrote them.  The core is csrc/overlap_core.h, shared with the host program of tools/overlap_host;
// tests/reprojection_reference.py is the raster it is pinned to.
//
// One block of 256 threads per pair.  A side is loaded by the whole block: its tokens go once into LDS as int16 (coalesced,
// the END search rides on the same pass), thread t builds the records of lines t, t + 256, ... in registers, the keys are
// ranked by counting (the technique of tk_rank, csrc/tokenise.hip) and the records scattered into sorted order; eight threads
// find the group starts by binary search.  Then thread t sweeps the other side's group for the sorted lines t, t + 256, ...
// of each side.  Plain stores only, no atomics, no global scratch, no allocation, no synchronisation with the host: the launch
// captures into a graph like every other entry point.
#include "pa_device.h"
#include "overlap_core.h"
#include "../../include/plank_hip.h"

namespace {

#define ST(s) reinterpret_cast<hipStream_t>(s)

constexpr int OV_THREADS = 256;
constexpr int OV_WAVES = OV_THREADS / 64;
constexpr int OV_PER = OV_MAX_LINES / OV_THREADS;          // lines a thread owns at most
static_assert(OV_MAX_LINES == PA_TOKENISE_MAX_LINES, "the core's limit is the tokeniser's");
static_assert((1 << OV_LINE_BITS) == OV_MAX_LINES, "line field must hold every line number");
static_assert(OV_MAX_TOL == PA_OVERLAP_MAX_TOL, "the header's limit is the core's");

struct OvArgs {
    const int64_t* value[2]; const int64_t* view[2]; const int64_t* type[2];
    int64_t stride[2];
    const int32_t* pair[2];
    int32_t len[2];
    int32_t end_token, num_bits, tol, mode;
    int32_t* out;
};

__device__ __forceinline__ int ov_wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int ov_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// One side of one pair -> its sorted keys / records / types and its group starts.  Called by the whole block; tok / key / red
// are free to reuse on return.
__device__ __forceinline__ void ov_load_side(const int64_t* __restrict__ value, const int64_t* __restrict__ view,
                                             const int64_t* __restrict__ type, int len, int end_token, int num_bits, int drop_hidden,
                                             int16_t* tok, uint32_t* key, uint32_t* skey, uint32_t* srec, int32_t* stype, int32_t* start,
                                             int32_t* red) {
    const int tid = threadIdx.x;
    const int ntok = 4 * ov_lines(len);                                   // <= 4 * OV_MAX_LINES: the entry refuses wider rows
    int first = ntok;
    for (int j = tid; j < ntok; j += OV_THREADS) {
        const int64_t t = value[j];
        tok[j] = ov_tok(t, num_bits);
        if (t == (int64_t)end_token && j < first) first = j;
    }
    first = ov_wave_min(first);
    if ((tid & 63) == 0) red[tid >> 6] = first;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < OV_WAVES; ++w) first = red[w] < first ? red[w] : first;
    const int n = first / 4;                                              // uniform; 4 n <= ntok

    uint32_t rk[OV_PER], rr[OV_PER];
    int32_t rt[OV_PER];
#pragma unroll
    for (int k = 0; k < OV_PER; ++k) {
        const int i = k * OV_THREADS + tid;
        rk[k] = 0; rr[k] = 0; rt[k] = 0;
        if (i < n) {                                                      // 4 i + 3 < 4 n <= ntok <= len
            rt[k] = type ? ov_type(type[4 * i]) : 0;
            ov_record(tok + 4 * i, view[4 * i], drop_hidden && rt[k] != 0, (uint32_t)i, &rk[k], &rr[k]);
            key[i] = rk[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < OV_PER; ++k) {
        const int i = k * OV_THREADS + tid;
        if (i < n) {
            int below = 0;                                                // every key is distinct: below is a permutation of 0 .. n - 1
            for (int j = 0; j < n; ++j) below += key[j] < rk[k];
            skey[below] = rk[k]; srec[below] = rr[k]; stype[below] = rt[k];
        }
    }
    __syncthreads();
    if (tid < OV_STARTS) start[tid] = ov_group_start(skey, n, tid);
    __syncthreads();
}

__global__ __launch_bounds__(OV_THREADS) void line_overlap_kernel(OvArgs g) {
    extern __shared__ __align__(16) unsigned char mem[];
    const OvLayout l = ov_layout(g.len[0], g.len[1]);
    int16_t* tok = reinterpret_cast<int16_t*>(mem + l.tok);
    uint32_t* key = reinterpret_cast<uint32_t*>(mem + l.key);
    int32_t* start = reinterpret_cast<int32_t*>(mem + l.start);
    int32_t* red = reinterpret_cast<int32_t*>(mem + l.red);

    const int pair = blockIdx.x, tid = threadIdx.x;
    const int match_type = g.mode == OV_MODE_MATCH;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int64_t r = g.pair[s] ? (int64_t)g.pair[s][pair] : (int64_t)pair;
        const int64_t at = r * g.stride[s];
        const bool read_type = g.type[s] && (s == 0 ? match_type : g.mode != OV_MODE_IGNORE);
        ov_load_side(g.value[s] + at, g.view[s] + at, read_type ? g.type[s] + at : nullptr, g.len[s], g.end_token, g.num_bits,
                     s == 1 && g.mode == OV_MODE_VISIBLE, tok, key, reinterpret_cast<uint32_t*>(mem + l.skey[s]),
                     reinterpret_cast<uint32_t*>(mem + l.srec[s]), reinterpret_cast<int32_t*>(mem + l.stype[s]),
                     start + s * OV_STARTS, red);
    }

    int sums[4];                                                          // cov(A|B), len(A), cov(B|A), len(B)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int o = 1 - s;
        const uint32_t* skey = reinterpret_cast<const uint32_t*>(mem + l.skey[s]);
        const uint32_t* srec = reinterpret_cast<const uint32_t*>(mem + l.srec[s]);
        const int32_t* stype = reinterpret_cast<const int32_t*>(mem + l.stype[s]);
        const int kept = start[s * OV_STARTS + OV_GROUP_SKIPPED];         // the kept lines sort first; kept <= lines of the side
        int cov = 0, len = 0;
#pragma unroll
        for (int k = 0; k < OV_PER; ++k) {
            const int i = k * OV_THREADS + tid;
            if (i < kept) {
                const uint32_t ka = skey[i], ra = srec[i];
                cov += ov_covered(ka, ra, stype[i], reinterpret_cast<const uint32_t*>(mem + l.skey[o]),
                                  reinterpret_cast<const uint32_t*>(mem + l.srec[o]), reinterpret_cast<const int32_t*>(mem + l.stype[o]),
                                  start + o * OV_STARTS, g.tol, match_type);
                len += ov_hi(ra) - ov_lo(ka);
            }
        }
        sums[2 * s] = ov_wave_sum(cov); sums[2 * s + 1] = ov_wave_sum(len);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[(tid >> 6) * 4 + q] = sums[q];
    }
    __syncthreads();
    if (tid == 0) {
        int32_t* o = g.out + (int64_t)pair * 8;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = red[q] + red[4 + q] + red[8 + q] + red[12 + q];
        o[4] = start[OV_GROUP_SKIPPED]; o[5] = start[OV_STARTS + OV_GROUP_SKIPPED];
        o[6] = start[OV_GROUP_DROPPED] - start[OV_GROUP_SKIPPED];
        o[7] = start[OV_STARTS + OV_GROUP_DROPPED] - start[OV_STARTS + OV_GROUP_SKIPPED];
    }
}

}  // namespace

extern "C" int pa_line_overlap(const int64_t* value_a, const int64_t* view_a, const int64_t* type_a, int64_t stride_a, int32_t len_a,
                               const int64_t* value_b, const int64_t* view_b, const int64_t* type_b, int64_t stride_b, int32_t len_b,
                               const int32_t* pair_a, const int32_t* pair_b, int32_t n_pairs, int32_t end_token, int32_t num_bits,
                               int32_t tol, int32_t type_mode, int32_t* out, void* stream) {
    if (!value_a || !view_a || !value_b || !view_b || !out) return PA_EINVAL;
    if (n_pairs < 0 || stride_a < 0 || stride_b < 0 || len_a < 0 || len_b < 0 || tol < 0 || tol > OV_MAX_TOL) return PA_EINVAL;
    if ((pair_a == nullptr) != (pair_b == nullptr)) return PA_EINVAL;
    if (type_mode != PA_OVERLAP_IGNORE && type_mode != PA_OVERLAP_MATCH && type_mode != PA_OVERLAP_VISIBLE) return PA_EINVAL;
    if (type_mode == PA_OVERLAP_MATCH && (!type_a || !type_b)) return PA_EINVAL;
    if (num_bits < 1 || num_bits > OV_MAX_BITS) return PA_ESHAPE;
    if (ov_lines(len_a) > OV_MAX_LINES || ov_lines(len_b) > OV_MAX_LINES) return PA_ESHAPE;
    if (n_pairs == 0) return 0;
    OvArgs g;
    g.value[0] = value_a; g.view[0] = view_a; g.type[0] = type_a; g.stride[0] = stride_a; g.pair[0] = pair_a; g.len[0] = len_a;
    g.value[1] = value_b; g.view[1] = view_b; g.type[1] = type_b; g.stride[1] = stride_b; g.pair[1] = pair_b; g.len[1] = len_b;
    g.end_token = end_token; g.num_bits = num_bits; g.tol = tol; g.mode = type_mode; g.out = out;
    const OvLayout l = ov_layout(len_a, len_b);
    PA_LAUNCH(line_overlap_kernel, dim3((unsigned)n_pairs), dim3(OV_THREADS), (size_t)l.bytes, ST(stream), g);
    return 0;
}
