// Greedy autoregressive decode for gfx950: reference plankassembly/models.py:267-307 (eval_step) with a
// K/V cache instead of the reference's O(T^2) prefix recompute (mathematically identical for a causal
// decoder in eval mode).  One decode step = a fixed sequence of kernels that
// read the step index from DEVICE memory, so the host can capture the step once in a hipGraph and
// replay it max_output_length times.
//   * single-query attention (HBM-bound batched GEMV): 16-byte K/V row chunks per lane, score
//     reduction across the lanes of a row with wave shuffles, online softmax per lane group,
//     partial (m, l, acc) merge through LDS.
//   * sampling kernel fuses: pointer logits against the hidden-state cache, switch head, vocab /
//     pointer softmax, gating, the 1e-6 pointer-mask fill, first-max argmax, pointer copy, END tracking
//     (reference models.py:168-186 eval branch of _create_dist and 235-256 _sample).
#include <cmath>
#include <math.h>
#include <new>
#include <string.h>
#include "pa_device.h"
#include "model.h"

struct BeamSeg {
    char* ptr;
    int64_t row_stride, outer_stride, scr_off, scr_outer;
    int32_t outer, unit, by_pos, pos_add, vec16, pad_;
};
constexpr int BEAM_MAX_SEG = 40;
struct BeamCopy {
    char* scratch;
    int64_t scr_row;
    int32_t nseg, pad_;
    BeamSeg seg[BEAM_MAX_SEG];
};

// What plan_decode() decides for a decode of B rows over S memory positions and Tmax steps: the fields pa_decode_plan reports
// (include/plank_hip.h; the rule and the measurements: plan_decode) and the status pa_decode_begin / pa_decode_ws_bytes answer with.
// `group`: the decode group (pa_decode_group_plan) - rows = B drawings x G, rows_per_block / units of the absorbed cross launch.
struct DecodePlan : pa_decode_plan_info { int status = 0; pa_decode_group_info group{}; };

struct DecodeLayout {
    int B = 0, S = 0, Tmax = 0;                // B: the decode's ROWS (drawings x G); S: memory positions per drawing
    int G = 1, Bd = 0;                         // decode group (pa_decode_group_begin): G rows per drawing, Bd = B / G drawings - mem, kpm, cu, cross_k / cross_v are per drawing
    DecodePlan plan{};                         // of this (B, S, Tmax): the layout, pa_decode_begin, the beam reorder and the step read it
    std::vector<void*> cross_k, cross_v, self_k, self_v;   // per decoder layer, per-head contiguous: [B][H][S|Tmax][dh]
    void* kv_tmp;                              // [B*S][2d] projection output before the per-head re-layout
    void *hid_cache, *x, *qkv, *ao, *z, *y, *q, *ff, *pfeat, *h;
    float *vlog, *mean, *rstd;
    int64_t *tokens, *attach; int32_t *first_end, *t_dev;
    uint8_t* kpm;                              // copy of input_mask: the captured step must not depend on batch tensors
    int32_t* cu;                               // copy of the packed-row offsets (NULL: dense memory + kpm)
    int32_t* cu_store;
    // LayerNorm folded into the Linear that consumes it (bf16; pa_gemm_norm_a): per decoder layer, for the three Linears whose
    // input is a sublayer's LayerNorm output - [0] self-attention in_proj (norm3 of the layer before), [1] the cross-attention
    // query projection (norm1), [2] linear1 (norm2): gamma-scaled weight, u, v (include/plank_hip.h)
    void* z2 = nullptr;                        // second pre-norm buffer (z of the cross-attention block)
    std::vector<void*> fw[3]; std::vector<float*> fu[3], fv[3];
    // f32 residual stream of the bf16 step (PLANK_DECODE_F32_RESID, default on with `fold`): x / y / z / z2 hold f32 rows, zb / z2b /
    // xb / hb their bf16 copies = the matrix operands of the Linears that read them, hf = decoder.norm's output in f32 (vocabulary head).
    // Everything else of the step - weights, Q / K / V, the caches, attention outputs, FFN hidden rows - stays bf16.
    void *zb = nullptr, *z2b = nullptr, *xb = nullptr;
    float* hf = nullptr;
    // Absorbed ("multi-query") cross-attention (csrc/decode_mq.h; bf16, d_model 512, <= 8 heads, with `fold`): the step attends over a
    // copy of the encoder output rows (`mem`) instead of per-layer K / V caches.  qt / ctx: [B][H][d] query / context rows of a step;
    // wo_t / bo_t per layer: W_o,h W_v,h as one [d][H d] bf16 matrix and b_o + W_o b_v; with `mq_contract` (exact f32, dh 64) W_v is its
    // own launch in front of the ordinary out-projection instead (decode_mq.h).
    // `mq_self` (exact f32): the SELF-attention absorbed too - self_k[i] caches the layer-input rows [B][Tmax][d]
    std::vector<void*> wvt_self;               // per layer: head-transposed W_v of the self-attention (mq_contract_v_kernel)
    void *mem = nullptr, *qt = nullptr, *ctx = nullptr;
    std::vector<void*> wo_t; std::vector<float*> bo_t;
    // `mq_self_bf` (bf16 step, f32 residual stream), round 6: the SELF-attention absorbed as well - self_k[i] caches the layer-input rows
    // (bf16), the out-projection runs on the context rows with W~o,self = W_o,h W_v,h (wo_ts / bo_ts); self_v is not read
    std::vector<void*> wo_ts; std::vector<float*> bo_ts;
    void* mq_sp = nullptr;                     // range blocks of the absorbed launches (decode_mq.h; plan.mq_sp_bytes): tickets (zero between launches) + partials
    // beam search (pa_decode_beam_begin; 0 = greedy): K beams per drawing over the B rows, state in the caller's beam workspace
    int beamK = 0;
    float *bm_score = nullptr, *bm_clp = nullptr;
    int32_t *bm_fin = nullptr, *bm_parent = nullptr, *bm_ctok = nullptr, *bm_catt = nullptr;
    BeamCopy bm_copy{};                        // segment table of the history reorder (passed to the copy kernel by value)
    // sampling (pa_decode_sample_begin; 0 = not sampling): N samples per drawing over the B rows, state in the caller's sample workspace
    int sampleN = 0;
    void* sm_prm = nullptr;                    // the device parameter block (SampleParamsDev)
    float* sm_score = nullptr;
    // forced prefixes (pa_decode_prefix_begin; any mode): the table and its scores in the caller's prefix workspace
    bool px_on = false;
    int32_t *px_len = nullptr, *px_tok = nullptr, *px_att = nullptr;   // [rows], [rows][Tmax], [rows][Tmax]
    float *px_score = nullptr, *px_lp = nullptr;                      // [rows], [rows][Tmax]
    // plank grammar (pa_decode_constraint_set; any mode): the caller's parameters, handed to the end-of-step kernels by value
    bool cs_on = false;
    pa_constraint_params cs{};
};

namespace {

#define RC(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)
#define HIP_RC(x) do { hipError_t he_ = (x); if (he_ != hipSuccess) return (int)he_; } while (0)
constexpr float LOG2E_F = 1.4426950408889634f;
#include "split_merge.h"
}  // namespace
#include "decode_mq.h"
namespace {

// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void dec_embed_kernel(T* x, const float* value, const float* coord, const float* pos,
                                                        const int64_t* tokens, int Tmax, const int32_t* t_dev, int B, int d, int dof,
                                                        bf16* x_lp = nullptr) {
    const int t = *t_dev;
    const int vec = d >> 2;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < B * vec; e += gridDim.x * 256) {
        const int b = e / vec, c = (e % vec) << 2;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (t > 0) {
            const int64_t v = tokens[(int64_t)b * Tmax + (t - 1)];
            acc = *reinterpret_cast<const f32x4*>(value + v * d + c);
            acc += *reinterpret_cast<const f32x4*>(coord + (int64_t)((t - 1) % dof) * d + c);
            acc += *reinterpret_cast<const f32x4*>(pos + (int64_t)((t - 1) / dof) * d + c);
        }
        st4<T>(x + (int64_t)b * d + c, acc);
        if (x_lp) st4<bf16>(x_lp + (int64_t)b * d + c, acc);
    }
}

// bf16 copy of f32 rows (the f32-residual step: decoder.norm's output as the pointer head's operand and for the hidden cache)
__global__ __launch_bounds__(256) void dec_cast_kernel(bf16* out, const float* in, int64_t n4) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256)
        st4<bf16>(out + 4 * e, *reinterpret_cast<const f32x4*>(in + 4 * e));
}

// K/V caches are kept per head ([B][H][L][dh], each (b, h) a contiguous stream): reading 128-byte head slices out of
// [B*L][2d] rows is a 2 KiB-strided access that camps on two L2 channels per XCD.  The self-attention caches are appended
// to by dec_attn_kernel itself (`newkv`).
// [B*S][2d] (k | v) -> K [B][H][S][dh], V [B][H][S][dh]
template <typename T>
__global__ __launch_bounds__(256) void dec_split_heads_kernel(T* kc, T* vc, const T* kv, int64_t rows, int S, int d, int H,
                                                              const int32_t* cu, const int32_t* rowmap) {
    const int dh = d / H, vec = d >> 2;
    const int64_t total = rows * vec;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / vec;
        const int c = (int)(e % vec) << 2;
        int b = (int)(row / S), s = (int)(row % S);
        if (cu) { b = rowmap[row] / S; s = (int)row - cu[b]; }          // packed memory: s-th valid position of element b
        const int h = c / dh, cc = c % dh;
        const int64_t dst = (((int64_t)b * H + h) * S + s) * dh + cc;
        st4<T>(kc + dst, ld4<T>(kv + row * 2 * d + c));
        st4<T>(vc + dst, ld4<T>(kv + row * 2 * d + d + c));
    }
}

// single-query attention; grid (H, B), 4 waves.  Lk = fixed_lk or *t_dev + 1.
// `newkv` (self-attention): the step's in_proj output [B][3d]; key t = Lk - 1 is not in the cache yet - its K / V head
// slices are taken from there (per-lane source select, no read-after-write through memory) and appended to the caches by
// this block for the later steps.  That is the whole of what a separate append launch did (6 launches per step).
// `G` (cross-attention of a decode group; 1 elsewhere): row b attends over the caches, mask and offsets of drawing b / G.
template <typename T, int DH>
__global__ __launch_bounds__(256) void dec_attn_kernel(T* out, const T* q, int ldq, T* kc, T* vc, int Lmax,
                                                       const uint8_t* kpm, int fixed_lk, const int32_t* t_dev,
                                                       int d, float scale, const int32_t* cu, const T* newkv, int G) {
    constexpr int EB = ET<T>::EB;
    constexpr int LPR = DH / EB;             // lanes per key row
    constexpr int KPW = 64 / LPR;            // keys per wave step
    constexpr int NG = 4 * KPW;              // partial groups per block
    __shared__ float part[NG * (DH + 2)];
    const int h = blockIdx.x, b = blockIdx.y, bk = b / G;         // bk: whose keys (the self-attention caches are per row: G 1)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane % LPR, slot = lane / LPR;
    const int Lk = cu ? (cu[bk + 1] - cu[bk]) : (fixed_lk > 0 ? fixed_lk : (*t_dev + 1));
    constexpr int ldkv = DH;                                     // per-head contiguous cache
    const int64_t bh = ((int64_t)bk * gridDim.x + h) * Lmax * DH + c * EB;
    const T* kb = kc + bh;
    const T* vb = vc + bh;
    const T* nk = newkv ? newkv + (int64_t)b * 3 * d + d + h * DH + c * EB : nullptr;        // this lane's chunk of the new K row
    const T* nv = newkv ? nk + d : nullptr;
    if (newkv && tid < LPR) {                                                                // append for the steps to come
        const int64_t dst = ((int64_t)b * gridDim.x + h) * Lmax * DH + (int64_t)(Lk - 1) * DH + c * EB;
        *reinterpret_cast<u32x4*>(kc + dst) = *reinterpret_cast<const u32x4*>(nk);
        *reinterpret_cast<u32x4*>(vc + dst) = *reinterpret_cast<const u32x4*>(nv);
    }
    const uint8_t* mk = kpm ? kpm + (int64_t)bk * Lmax : nullptr;
    float qv[EB];
    {
        const T* qp = q + (int64_t)b * ldq + h * DH + c * EB;
#pragma unroll
        for (int e = 0; e < EB; e += 4) { const f32x4 t4 = ld4<T>(qp + e); qv[e] = t4[0]; qv[e + 1] = t4[1]; qv[e + 2] = t4[2]; qv[e + 3] = t4[3]; }
    }
    const float sl = scale * LOG2E_F;
    float m = -INFINITY, l = 0.f, acc[EB];
#pragma unroll
    for (int e = 0; e < EB; ++e) acc[e] = 0.f;
    // UN key groups per iteration; K and V rows travel as raw 16-byte vectors (one load each per lane and key) and are
    // widened only when used, so 2*UN loads are in flight per lane at 2*UN*4 VGPRs
    constexpr int UN = 8;
    auto widen = [](const u32x4& raw, float* f) {
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int w = 0; w < 4; ++w) { f[2 * w] = bf16_lo(raw[w]); f[2 * w + 1] = bf16_hi(raw[w]); }
        } else {
#pragma unroll
            for (int w = 0; w < 4; ++w) f[w] = __uint_as_float(raw[w]);
        }
    };
    for (int base0 = wave * KPW; base0 < Lk; base0 += 4 * KPW * UN) {
        u32x4 kraw[UN], vraw[UN];
        bool okk[UN];
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            const int key = base0 + j * 4 * KPW + slot;
            const bool in = key < Lk;
            okk[j] = in && !(mk && mk[in ? key : 0]);
            // unconditional loads (clamped row; out-of-range keys are discarded through okk): a branch around the loads
            // would put a wait between them
            const int64_t kc_ = (int64_t)min(key, Lk - 1) * ldkv;
            const bool fresh = newkv && key >= Lk - 1;                 // the row this step produced (clamped keys land here too)
            // (streamed once per step, never re-read by this CU: non-temporal, so the lines do not displace the weights in L2)
            kraw[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(fresh ? nk : kb + kc_));
            vraw[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(fresh ? nv : vb + kc_));
        }
        float s[UN];
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            float kf[EB];
            widen(kraw[j], kf);
            float a = 0.f;
#pragma unroll
            for (int e = 0; e < EB; ++e) a += qv[e] * kf[e];
#pragma unroll
            for (int o = 1; o < LPR; o <<= 1) a += __shfl_xor(a, o);
            s[j] = okk[j] ? a * sl : -INFINITY;
        }
        float mn = m;
#pragma unroll
        for (int j = 0; j < UN; ++j) mn = fmaxf(mn, s[j]);
        if (mn > -INFINITY) {
            const float alpha = exp2f(m - mn);
            l *= alpha;
#pragma unroll
            for (int e = 0; e < EB; ++e) acc[e] *= alpha;
#pragma unroll
            for (int j = 0; j < UN; ++j) {
                const float pj = exp2f(s[j] - mn);           // exp2(-inf) = 0 for masked / out-of-range keys
                l += pj;
                float vf[EB];
                widen(vraw[j], vf);
#pragma unroll
                for (int e = 0; e < EB; ++e) acc[e] += pj * vf[e];
            }
            m = mn;
        }
    }
    const int g = wave * KPW + slot;
    if (c == 0) { part[g * (DH + 2)] = m; part[g * (DH + 2) + 1] = l; }
#pragma unroll
    for (int e = 0; e < EB; ++e) part[g * (DH + 2) + 2 + c * EB + e] = acc[e];
    __syncthreads();
    if (tid < DH) {
        float M = -INFINITY;
        for (int i = 0; i < NG; ++i) M = fmaxf(M, part[i * (DH + 2)]);
        float num = 0.f, den = 0.f;
        for (int i = 0; i < NG; ++i) {
            const float mi = part[i * (DH + 2)];
            if (mi == -INFINITY) continue;
            const float w = exp2f(mi - M);
            den += part[i * (DH + 2) + 1] * w;
            num += part[i * (DH + 2) + 2 + tid] * w;
        }
        st1<T>(out + (int64_t)b * d + h * DH + tid, den > 0.f ? num / den : 0.f);
    }
}

// ------------------------------------------------------------------------------------------------
struct ArgMax { float v; int i; };
__device__ __forceinline__ ArgMax better(ArgMax a, ArgMax b) {   // first-max: larger value, then smaller index
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
// 256-thread block arg-max in better()'s first-max order, valid in every thread on return.  A caller that reduces again puts a barrier
// of its own before the next call (sha is rewritten).
__device__ __forceinline__ ArgMax block_argmax(ArgMax best, ArgMax* sha) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ArgMax other{__shfl_xor(best.v, o), __shfl_xor(best.i, o)};
        best = better(best, other);
    }
    if ((threadIdx.x & 63) == 0) sha[threadIdx.x >> 6] = best;
    __syncthreads();
    return better(better(sha[0], sha[1]), better(sha[2], sha[3]));
}
// Candidate index -> the token and attach to write: vocab entry k < V is itself; pointer j (index V + j) takes the row's own token at j
// (reference models.py:248-251).  `row` = the row's token history.
struct TokAtt { int64_t tok, att; };
__device__ __forceinline__ TokAtt candidate_token(int idx, int V, const int64_t* row) {
    TokAtt c{idx, -1};
    if (idx >= V) { c.att = idx - V; c.tok = row[c.att]; }
    return c;
}
__device__ __forceinline__ float block_max(float v, float* sh) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    __syncthreads();
    return v;
}
__device__ __forceinline__ float block_sum(float v, float* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return v;
}
__device__ __forceinline__ bool ptr_allowed(int i, int j) {      // reference models.py:91-101, closed form
    if (i < 6) return false;
    return j < 6 ? (j == i % 6) : ((j % 6) == ((i % 6) + 3) % 6);
}

constexpr int MAX_T = 2048;

// The distribution of row b at step t (reference models.py:168-186, eval branch), shared by the greedy kernel and the beam
// candidate kernel so that the two cannot drift apart.  row_dist_prepare computes the softmax statistics (vocabulary, and for
// sz = t + 1 >= 6 the pointer logits over the hidden prefix into `plog` plus the switch gate); row_dist_visit then hands every
// candidate of this thread to f(p, index) - vocab entries k < V as index k, pointers j < jend as index V + j - with the same f32
// arithmetic each time it is called, so a caller may walk the candidates more than once.  Every thread of the block must call both.
struct RowDist { float vmax, vsum, pmax, psum, prob; };
template <typename T>
__device__ __forceinline__ RowDist row_dist_prepare(const float* vr, int V, const T* pfeat, const T* hb, const T* cache, int64_t nb,
                                                    int t, int d, const float* sw_w, const float* sw_b, float* plog, float* sh, float* s_sw) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sz = t + 1;
    RowDist r{-INFINITY, 0.f, -INFINITY, 0.f, 0.f};
    // vocab softmax statistics
    float vmax = -INFINITY;
    for (int k = tid; k < V; k += 256) vmax = fmaxf(vmax, vr[k]);
    vmax = block_max(vmax, sh);
    float vsum = 0.f;
    for (int k = tid; k < V; k += 256) vsum += expf(vr[k] - vmax);
    vsum = block_sum(vsum, sh);
    r.vmax = vmax; r.vsum = vsum;
    if (sz < 6) return r;                                             // models.py:172-173: un-gated vocab softmax
    // pointer logits over the hidden prefix (row j = t is written by the caller but masked: j >= i)
    // each wave takes 8 cached rows at a time, all their loads issued (unconditionally: rows clamped, tail discarded)
    // before the first reduction; the pointer-feature row stays in registers.  Per row the arithmetic order is the
    // one-row-at-a-time order (chunk by chunk per lane, then the wave sum): logits and greedy tokens are unchanged.
    const T* pf = pfeat;
    auto ptr_logits = [&](auto NCH_) {
        constexpr int NCH = decltype(NCH_)::value, PUN = 8;           // NCH = d / 256 chunks of 4 columns per lane
        f32x4 pa[NCH];
#pragma unroll
        for (int q = 0; q < NCH; ++q) pa[q] = ld4<T>(pf + (lane << 2) + q * 256);
        for (int j0 = wave * PUN; j0 < t; j0 += 4 * PUN) {
            f32x4 hh[PUN][NCH];
#pragma unroll
            for (int u = 0; u < PUN; ++u) {
                const T* row = cache + (int64_t)min(j0 + u, t - 1) * nb * d + (lane << 2);
#pragma unroll
                for (int q = 0; q < NCH; ++q) hh[u][q] = ld4<T>(row + q * 256);
            }
#pragma unroll
            for (int u = 0; u < PUN; ++u) {
                float sacc = 0.f;
#pragma unroll
                for (int q = 0; q < NCH; ++q)
                    sacc += pa[q][0] * hh[u][q][0] + pa[q][1] * hh[u][q][1] + pa[q][2] * hh[u][q][2] + pa[q][3] * hh[u][q][3];
                sacc = wave_sum(sacc);
                if (lane == 0 && j0 + u < t) plog[j0 + u] = sacc / (float)d;
            }
        }
    };
    if (d == 512) ptr_logits(std::integral_constant<int, 2>{});
    else if (d == 256) ptr_logits(std::integral_constant<int, 1>{});
    else if (d == 768) ptr_logits(std::integral_constant<int, 3>{});
    else if (d == 1024) ptr_logits(std::integral_constant<int, 4>{});
    else {
        for (int j = wave; j < t; j += 4) {
            float s = 0.f;
            for (int c = lane << 2; c < d; c += 256) {
                const f32x4 a = ld4<T>(pf + c), hh = ld4<T>(cache + (int64_t)j * nb * d + c);
                s += a[0] * hh[0] + a[1] * hh[1] + a[2] * hh[2] + a[3] * hh[3];
            }
            s = wave_sum(s);
            if (lane == 0) plog[j] = s / (float)d;
        }
    }
    if (wave == 0) {
        float s = 0.f;
        for (int c = lane << 2; c < d; c += 256) {
            const f32x4 hh = ld4<T>(hb + c); const f32x4 w = *reinterpret_cast<const f32x4*>(sw_w + c);
            s += hh[0] * w[0] + hh[1] * w[1] + hh[2] * w[2] + hh[3] * w[3];
        }
        s = wave_sum(s);
        if (lane == 0) *s_sw = s + sw_b[0];
    }
    __syncthreads();
    r.prob = 1.0f / (1.0f + expf(-*s_sw));
    float pmax = -INFINITY;
    for (int j = tid; j < t; j += 256) pmax = fmaxf(pmax, plog[j]);
    pmax = block_max(pmax, sh);
    float psum = 0.f;
    for (int j = tid; j < t; j += 256) psum += expf(plog[j] - pmax);
    psum = block_sum(psum, sh);
    r.pmax = pmax; r.psum = psum;
    return r;
}

// p of one candidate, the expressions row_dist_visit hands out and the forced path (section 14) evaluates for its one index: the vocab
// softmax term (un-gated; sz >= 6 multiplies it by 1 - prob) and the pointer j of step i = t.
__device__ __forceinline__ float dist_p_vocab(const RowDist& r, const float* vr, int k) { return expf(vr[k] - r.vmax) / r.vsum; }
__device__ __forceinline__ float dist_p_ptr(const RowDist& r, const float* plog, int i, int j) {
    float val = 1e-6f;                                                // models.py:183-184 fill after gating
    if (ptr_allowed(i, j)) val = (j < i) ? (expf(plog[j] - r.pmax) / r.psum) * r.prob : 0.f;
    return val;
}

// Plank grammar: a plank is six coordinate tokens x0 y0 z0 x1 y1 z1 with max > min per axis, END stands at a
// plank boundary only.  At step t = 6 k + c the written token of a free row must lie in a window that depends on t and on the row's own
// token at t - 3 alone: tokens [lo, hi] (lo > hi: none), plus END when `end`.  The clamp of the c >= 3 window keeps it non-empty whatever
// stands at t - 3 (a greedy row steps on after its END, a forced prefix may put anything there).  Passed by value: a captured step
// depends on the parameters (max_planks arrives clamped to the last boundary that leaves room for END, (Tmax - 1) / 6).
struct ConstraintDev { int32_t on, n_val, end_tok, min_planks, max_planks; };
struct Window { int lo, hi, end; };
__device__ __forceinline__ Window plank_window(const ConstraintDev& cs, const int64_t* row, int t) {
    const int c = t % 6, k = t / 6;
    if (c == 0) return k >= cs.max_planks ? Window{1, 0, 1} : Window{0, cs.n_val - 2, k >= cs.min_planks ? 1 : 0};
    if (c < 3) return Window{0, cs.n_val - 2, 0};
    const int64_t prev = row[t - 3];
    return Window{(int)max(min(prev, (int64_t)(cs.n_val - 2)), (int64_t)-1) + 1, cs.n_val - 1, 0};
}
// The allowed-predicate of row `row` at step t, by candidate index: vocab entry k writes token k; pointer j < t writes the row's own
// token at j and is judged by it; a pointer j >= t is never allowed.  Off: everything is allowed and nothing is read.  Every thread of
// the block builds its own copy (one broadcast load of row[t - 3]).
struct Allow {
    Window w; int end_tok, V, t; const int64_t* row; bool on;
    __device__ __forceinline__ bool token(int64_t k) const { return (k >= w.lo && k <= w.hi) || (w.end && k == end_tok); }
    __device__ __forceinline__ bool operator()(int idx) const {
        if (!on) return true;
        if (idx < V) return token(idx);
        const int j = idx - V;
        return j < t && token(row[j]);
    }
    // an allowed vocab entry, for the step at which every allowed candidate has p = 0 in f32: the lowest of the window, else END
    __device__ __forceinline__ int fallback() const { return w.lo <= w.hi ? w.lo : end_tok; }
};
__device__ __forceinline__ Allow make_allow(const ConstraintDev& cs, const int64_t* row, int V, int t) {
    if (!cs.on) return Allow{Window{0, -1, 0}, 0, V, t, row, false};
    return Allow{plank_window(cs, row, t), cs.end_tok, V, t, row, true};
}

// f(p, index, ok): ok = the candidate is allowed under the row's constraint (always true without one); p is the same either way - the
// constraint only removes candidates from a caller's SELECTION.
template <typename F>
__device__ __forceinline__ void row_dist_visit(const RowDist& r, const float* vr, int V, const float* plog, int t, int jend,
                                               const Allow& al, F&& f) {
    const int tid = threadIdx.x, sz = t + 1, i = t;
    if (sz < 6) {                                                     // models.py:172-173: un-gated vocab softmax
        for (int k = tid; k < V; k += 256) f(dist_p_vocab(r, vr, k), k, al(k));
        return;
    }
    const float gate_v = 1.0f - r.prob;
    for (int k = tid; k < V; k += 256) f(dist_p_vocab(r, vr, k) * gate_v, k, al(k));
    for (int j = tid; j < jend; j += 256) f(dist_p_ptr(r, plog, i, j), V + j, al(V + j));
}

// The p row_dist_visit hands out for the single index idx (vocab k as k, pointer j as V + j).  An index that is no candidate at step
// t - outside the table, a pointer while sz < 6, a pointer j >= t - has p = 0 and reads nothing.
__device__ __forceinline__ float row_dist_at(const RowDist& r, const float* vr, int V, const float* plog, int t, int idx) {
    if (idx < 0) return 0.f;
    if (t + 1 < 6) return idx < V ? dist_p_vocab(r, vr, idx) : 0.f;
    if (idx < V) return dist_p_vocab(r, vr, idx) * (1.0f - r.prob);
    const int j = idx - V;
    return j < t ? dist_p_ptr(r, plog, t, j) : 0.f;
}

// The whole distribution of a row, stand-alone (pa_dec_row_dist): what the four tails do before they choose - the
// hidden row stored into cache row t, row_dist_prepare, then every p row_dist_visit hands out (jend = t + 1, no constraint) written to
// p_out [rows][V + Tmax] by its candidate index, and the RowDist fields to stats [rows][5].  No arithmetic of its own.
template <typename T>
__global__ __launch_bounds__(256) void dec_row_dist_kernel(float* p_out, float* stats, const float* vlog, int ldv, const T* pfeat, const T* h,
                                                           T* hid_cache, const float* sw_w, const float* sw_b, const int32_t* t_dev,
                                                           int Tmax, int d, int V) {
    __shared__ float plog[MAX_T];
    __shared__ float sh[4];
    __shared__ float s_sw;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int t = *t_dev;
    const T* hb = h + (int64_t)b * d;
    const int64_t nb = gridDim.x;
    T* cache = hid_cache + (int64_t)b * d;                          // [Tmax][rows][d], as in dec_sample_kernel
    for (int c = tid; c < d; c += 256) cache[(int64_t)t * nb * d + c] = hb[c];
    const float* vr = vlog + (int64_t)b * ldv;
    const RowDist rd = row_dist_prepare<T>(vr, V, pfeat + (int64_t)b * d, hb, cache, nb, t, d, sw_w, sw_b, plog, sh, &s_sw);
    const Allow al = make_allow(ConstraintDev{0, 0, 0, 0, 0}, nullptr, V, t);
    float* po = p_out + (int64_t)b * (V + Tmax);
    row_dist_visit(rd, vr, V, plog, t, t + 1, al, [&](float p, int k, bool) { po[k] = p; });
    if (tid == 0) {
        float* so = stats + (int64_t)b * 5;
        so[0] = rd.vmax; so[1] = rd.vsum; so[2] = rd.pmax; so[3] = rd.psum; so[4] = rd.prob;
    }
}

// ------------------------------------------------------------------------------------------------
// Forced prefixes.  The prefix arena of pa_decode_prefix_begin: per row r a length plen[r] and the forced
// candidate of every position t < plen[r] - ptok, and patt = -1 for the vocab entry ptok or j >= 0 for the pointer candidate j -
// plus what the forced positions scored: lp [rows][Tmax] per token and score [rows], their sum in step order.  plen = NULL: no table;
// the end-of-step kernels then do exactly what they did without this argument.  A row is forced or free per step (t < plen[r]) - one
// row per block, so the branch is uniform - and a forced row takes its candidate without arg-max, ranking or draw.
struct PrefixDev { const int32_t* plen; const int32_t* ptok; const int32_t* patt; float* score; float* lp; int32_t pad_tok; int32_t pad_; };

// The forced candidate of row r at step t: lp = logf(p) of its index with row_dist_visit's own arithmetic, the token and attach to
// write (a pointer takes the row's own token at patt, models.py:248-251).  A candidate that does not exist at this step scores -inf
// and reads nothing out of bounds; a token outside the vocabulary is written as PAD, so that the next step's embedding stays inside
// its table.  One thread calls it, after row_dist_prepare; it also stores lp in the per-token buffer.
struct Forced { float lp; int64_t tok, att; };
__device__ __forceinline__ Forced forced_candidate(const PrefixDev& px, int r, int t, int Tmax, const RowDist& rd, const float* vr, int V,
                                                   const float* plog, const int64_t* tokens) {
    const int ft = px.ptok[(int64_t)r * Tmax + t], fa = px.patt[(int64_t)r * Tmax + t];
    const bool tok_ok = ft >= 0 && ft < V;
    Forced f{-INFINITY, tok_ok ? ft : px.pad_tok, -1};
    if (fa < 0) {
        if (tok_ok) f.lp = logf(row_dist_at(rd, vr, V, plog, t, ft));
    } else if (fa < t && t + 1 >= 6) {
        f.att = fa; f.tok = tokens[(int64_t)r * Tmax + fa];
        f.lp = logf(row_dist_at(rd, vr, V, plog, t, V + fa));
    }
    px.lp[(int64_t)r * Tmax + t] = f.lp;
    return f;
}

template <typename T>
__global__ __launch_bounds__(256) void dec_sample_kernel(const float* vlog, int ldv, const T* pfeat, const T* h, T* hid_cache,
                                                         const float* sw_w, const float* sw_b, int64_t* tokens,
                                                         int64_t* attach, int32_t* first_end, int32_t* t_dev,
                                                         int Tmax, int d, int V, int end_tok, const PrefixDev px,
                                                         const ConstraintDev cs) {
    __shared__ float plog[MAX_T];
    __shared__ float sh[4];
    __shared__ ArgMax sha[4];
    __shared__ float s_sw;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int t = *t_dev, sz = t + 1;
    const T* hb = h + (int64_t)b * d;
    // hidden-state cache laid out [Tmax][B][d]: the 256 blocks walk the rows j in step, and with a per-sequence
    // [B][Tmax][d] layout (1 MB apart) they would all hit the same HBM channel at the same time
    const int64_t nb = gridDim.x;
    T* cache = hid_cache + (int64_t)b * d;                          // row j of this sequence: cache + j * nb * d
    for (int c = tid; c < d; c += 256) cache[(int64_t)t * nb * d + c] = hb[c];
    const float* vr = vlog + (int64_t)b * ldv;
    const RowDist rd = row_dist_prepare<T>(vr, V, pfeat + (int64_t)b * d, hb, cache, nb, t, d, sw_w, sw_b, plog, sh, &s_sw);
    if (px.plen && t < px.plen[b]) {                                // forced row (section 14)
        if (tid == 0) {
            const Forced f = forced_candidate(px, b, t, Tmax, rd, vr, V, plog, tokens);
            tokens[(int64_t)b * Tmax + t] = f.tok;
            attach[(int64_t)b * Tmax + t] = f.att;
            if (first_end[b] < 0) {                                 // greedy freezes nothing: forced and scored up to plen, summed up to END
                px.score[b] += f.lp;
                if (f.tok == end_tok) first_end[b] = t;
            }
        }
        return;
    }
    // (constrained, section 15: the arg-max runs over the allowed candidates only - one with p = 0 still beats every disallowed one,
    // and the window always holds a vocab entry, so best.i is a candidate)
    const Allow al = make_allow(cs, tokens + (int64_t)b * Tmax, V, t);
    ArgMax best{-INFINITY, 0x7fffffff};
    row_dist_visit(rd, vr, V, plog, t, sz, al, [&](float p, int k, bool ok) { if (ok) best = better(best, ArgMax{p, k}); });
    best = block_argmax(best, sha);
    if (tid == 0) {
        if (al.on && best.i == 0x7fffffff) best.i = al.fallback();  // (every allowed p is NaN: still an allowed token)
        const TokAtt c = candidate_token(best.i, V, tokens + (int64_t)b * Tmax);
        tokens[(int64_t)b * Tmax + t] = c.tok;
        attach[(int64_t)b * Tmax + t] = c.att;
        if (c.tok == end_tok && first_end[b] < 0) first_end[b] = t;
    }
}

// ------------------------------------------------------------------------------------------------
// Beam search.  Rows are hypotheses: row b * K + k is beam k of drawing b.  The step up to the heads is the
// greedy step on B * K rows; its end is these three kernels instead of dec_sample_kernel.

// Per-row top-K of the distribution (row_dist_prepare / row_dist_visit, the greedy kernel's own p values), ranked by the greedy
// kernel's first-max order (larger p, then the smaller index), candidates with p = 0 and the self pointer j = t left out.  K rounds of
// the block arg-max, round k taking the best candidate ordered strictly after the one of round k - 1 (the order is total, so no
// candidate is marked).  Writes cand_lp = logf(p), cand_tok (a pointer resolves its token from this row's own history,
// models.py:248-251), cand_att for ranks 0 .. K-1; ranks without a candidate get (-inf, PAD, -1).  A finished row has the one
// candidate (0, PAD, -1).  Also writes this row's hidden state into hid_cache, as the greedy kernel does.
template <typename T>
__global__ __launch_bounds__(256) void dec_beam_cand_kernel(const float* vlog, int ldv, const T* pfeat, const T* h, T* hid_cache,
                                                            const float* sw_w, const float* sw_b, const int64_t* tokens,
                                                            const int32_t* finished, const int32_t* t_dev, int Tmax, int d, int V,
                                                            int K, int pad_tok, float* cand_lp, int32_t* cand_tok, int32_t* cand_att,
                                                            const PrefixDev px, const ConstraintDev cs) {
    __shared__ float plog[MAX_T];
    __shared__ float sh[4];
    __shared__ ArgMax sha[4];
    __shared__ float s_sw;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int t = *t_dev;
    const T* hb = h + (int64_t)b * d;
    const int64_t nb = gridDim.x;
    T* cache = hid_cache + (int64_t)b * d;                          // [Tmax][rows][d], as in dec_sample_kernel
    for (int c = tid; c < d; c += 256) cache[(int64_t)t * nb * d + c] = hb[c];
    float* lp = cand_lp + (int64_t)b * K;
    int32_t* ct = cand_tok + (int64_t)b * K;
    int32_t* ca = cand_att + (int64_t)b * K;
    if (finished[b]) {                                              // frozen beam (uniform branch: one row per block)
        if (tid < K) { lp[tid] = tid == 0 ? 0.f : -INFINITY; ct[tid] = pad_tok; ca[tid] = -1; }
        return;
    }
    const float* vr = vlog + (int64_t)b * ldv;
    const RowDist rd = row_dist_prepare<T>(vr, V, pfeat + (int64_t)b * d, hb, cache, nb, t, d, sw_w, sw_b, plog, sh, &s_sw);
    if (px.plen && t < px.plen[b]) {                                // forced live row (section 14): the one candidate at rank 0
        if (tid == 0) {
            const Forced f = forced_candidate(px, b, t, Tmax, rd, vr, V, plog, tokens);
            lp[0] = f.lp; ct[0] = (int32_t)f.tok; ca[0] = (int32_t)f.att;
            px.score[b] += f.lp;
        } else if (tid < K) { lp[tid] = -INFINITY; ct[tid] = pad_tok; ca[tid] = -1; }
        return;
    }
    const Allow al = make_allow(cs, tokens + (int64_t)b * Tmax, V, t);   // (section 15: the ranking runs over the allowed candidates only)
    ArgMax prev{INFINITY, -1};
    for (int k = 0; k < K; ++k) {
        ArgMax best{-INFINITY, 0x7fffffff};
        row_dist_visit(rd, vr, V, plog, t, t, al, [&](float p, int idx, bool ok) {      // (jend = t: the self pointer is no candidate)
            if (ok && p > 0.f && (p < prev.v || (p == prev.v && idx > prev.i))) best = better(best, ArgMax{p, idx});
        });
        best = block_argmax(best, sha);
        __syncthreads();                                            // (sha is rewritten by the next round)
        if (tid == 0) {
            // no candidate left: (-inf, PAD, -1) - constrained, rank 0 of a row without any candidate of p > 0 carries an allowed token
            if (best.i == 0x7fffffff) { lp[k] = -INFINITY; ct[k] = (al.on && k == 0) ? al.fallback() : pad_tok; ca[k] = -1; }
            else {
                const TokAtt c = candidate_token(best.i, V, tokens + (int64_t)b * Tmax);
                lp[k] = logf(best.v); ct[k] = (int32_t)c.tok; ca[k] = (int32_t)c.att;
            }
        }
        prev = best;
    }
}

// Merge per drawing (one block, K * K <= 256 candidates, thread c = parent beam c / K, per-row rank c % K): ranked by
// score[parent] + cand_lp (f32) descending, ties to the smaller parent beam, then the better rank - i.e. to the smaller c.  The best K
// become the new beams: score, finished, first_end, parent row, and the token / attach at position t.  Everything of the drawing is
// read before anything is written (the new beams replace their parents' rows).
__global__ __launch_bounds__(256) void dec_beam_merge_kernel(const float* cand_lp, const int32_t* cand_tok, const int32_t* cand_att,
                                                             float* scores, int32_t* finished, int32_t* first_end, int32_t* parent,
                                                             int64_t* tokens, int64_t* attach, const int32_t* t_dev, int Tmax, int K,
                                                             int end_tok) {
    __shared__ float sc[256];
    __shared__ int32_t n_par[16], n_tok[16], n_att[16], n_fin[16], n_fe[16];
    __shared__ float n_sc[16];
    const int tid = threadIdx.x, KK = K * K, r0 = blockIdx.x * K;
    const int t = *t_dev;
    float mine = -INFINITY;
    int kp = 0, tok = 0, att = -1, fin = 0, fe = -1;
    if (tid < KK) {
        kp = tid / K;
        mine = scores[r0 + kp] + cand_lp[(int64_t)r0 * K + tid];
        tok = cand_tok[(int64_t)r0 * K + tid]; att = cand_att[(int64_t)r0 * K + tid];
        fin = finished[r0 + kp]; fe = first_end[r0 + kp];
        sc[tid] = mine;
    }
    __syncthreads();
    if (tid < KK) {
        int pos = 0;
        for (int j = 0; j < KK; ++j) pos += (sc[j] > mine || (sc[j] == mine && j < tid)) ? 1 : 0;
        if (pos < K) {
            const bool ended = fin || tok == end_tok;
            n_par[pos] = r0 + kp; n_tok[pos] = tok; n_att[pos] = att; n_sc[pos] = mine;
            n_fin[pos] = ended ? 1 : 0;
            n_fe[pos] = fin ? fe : (tok == end_tok ? t : -1);
        }
    }
    __syncthreads();
    if (tid < K) {
        const int r = r0 + tid;
        scores[r] = n_sc[tid]; finished[r] = n_fin[tid]; first_end[r] = n_fe[tid]; parent[r] = n_par[tid];
        tokens[(int64_t)r * Tmax + t] = n_tok[tid];
        attach[(int64_t)r * Tmax + t] = n_att[tid];
    }
}

// History reorder: every row r whose parent p = parent[r] is another row takes p's history.  Two launches: dir 0 copies the parent's
// history into r's slot of the scratch, dir 1 copies the slot back into row r - so every row reads its parent's OLD history.  A segment
// is one per-row cache: `outer` pieces `outer_stride` bytes apart, each (t + pos_add) * unit contiguous bytes (per-head self-attention
// caches, the row caches of the absorbed self-attention, tokens / attach), or - `by_pos` - t + pos_add pieces of `unit` bytes
// (hid_cache, [Tmax][rows][d]).
__global__ __launch_bounds__(256) void dec_beam_copy_kernel(const BeamCopy cp, const int32_t* parent, const int32_t* t_dev, int dir) {
    const int r = blockIdx.y, p = parent[r];
    if (p == r) return;
    const int t = *t_dev;
    char* slot = cp.scratch + (int64_t)r * cp.scr_row;
    for (int s = 0; s < cp.nseg; ++s) {
        const BeamSeg g = cp.seg[s];
        const int npos = t + g.pos_add;
        const int64_t outer = g.by_pos ? npos : g.outer;
        const int64_t inner = g.by_pos ? (int64_t)g.unit : (int64_t)npos * g.unit;     // bytes
        char* row = g.ptr + (int64_t)(dir == 0 ? p : r) * g.row_stride;
        char* scr = slot + g.scr_off;
        if (g.vec16) {
            const int64_t nv = inner >> 4, total = outer * nv;
            for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
                const int64_t o = e / nv, i = (e - o * nv) << 4;
                u32x4* a = reinterpret_cast<u32x4*>(row + o * g.outer_stride + i);
                u32x4* c = reinterpret_cast<u32x4*>(scr + o * g.scr_outer + i);
                if (dir == 0) *c = *a; else *a = *c;
            }
        } else {                                                    // (8-byte units: tokens / attach)
            const int64_t nv = inner >> 3, total = outer * nv;
            for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
                const int64_t o = e / nv, i = (e - o * nv) << 3;
                int64_t* a = reinterpret_cast<int64_t*>(row + o * g.outer_stride + i);
                int64_t* c = reinterpret_cast<int64_t*>(scr + o * g.scr_outer + i);
                if (dir == 0) *c = *a; else *a = *c;
            }
        }
    }
}

__global__ __launch_bounds__(256) void dec_beam_init_kernel(float* scores, int32_t* finished, int32_t* parent, int rows, int K) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < rows; r += gridDim.x * 256) {
        scores[r] = (r % K) == 0 ? 0.f : -INFINITY;                 // only beam 0 of a drawing is live at t = 0
        finished[r] = 0; parent[r] = r;
    }
}

// ------------------------------------------------------------------------------------------------
// Sampling.  Rows are samples: row b * N + n is sample n of drawing b.  The step up to the heads is the greedy
// step on B * N rows; its end is dec_sample_draw_kernel instead of dec_sample_kernel.  The parameters live in device memory
// (pa_decode_sample_begin / _set write them with dec_sample_init_kernel), so new parameters need no new graph capture.
struct SampleParamsDev { uint32_t seed; int32_t n; float temperature; int32_t top_k; float top_p; };
constexpr int SAMPLE_MAX_V = 2048;                                  // vocabulary bound of the staged candidate arrays
constexpr int SAMPLE_MAX_C = SAMPLE_MAX_V + MAX_T;

__device__ __forceinline__ int block_sum_i(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return v;
}
__device__ __forceinline__ int block_min_i(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = min(min(sh[0], sh[1]), min(sh[2], sh[3]));
    __syncthreads();
    return v;
}

// u in [0, 1) of sample n of drawing b at step t: a pure function of (seed, b, n, t) (tests/sample_reference.py restates it)
__device__ __forceinline__ float sample_u(uint32_t seed, uint32_t b, uint32_t n, uint32_t t) {
    const uint32_t h = mix32(t ^ mix32(n ^ mix32(b ^ mix32(seed + 0x9e3779b9u))));
    return (float)(h >> 8) * 0x1p-24f;
}

// One block per row.  Writes the row's hidden state into hid_cache (as the greedy kernel does), stages the candidates' p of
// row_dist_visit (vocab k at k, pointer j < t at V + j; the self pointer is no candidate) and their weights w in LDS, then:
//   top-k  (k > 0): bisection on the p bit pattern (p >= 0: the bits order as the values) for the k-th largest p, then - if the
//                   boundary p value is shared - on the index, for the smaller indices of that tie group (rank order: p
//                   descending, ties to the smaller index);
//   top-p  (< 1):   the same two bisections for the shortest rank-order prefix whose sum of w reaches top_p * (sum of kept w);
//                   every probe is the same fixed-order block sum with the excluded terms zeroed - f32 addition of
//                   non-negative terms is monotone, so the probes are monotone in the threshold;
//   draw:           per-thread contiguous index ranges, an exclusive scan of the 256 partial sums, and the first kept candidate
//                   whose inclusive prefix sum exceeds u * W (W = the prefix sum at the last candidate); none: the last kept one.
// Integer block reductions and fixed-order float ones only: the same seed gives the same tokens and scores on every run.
template <typename T>
__global__ __launch_bounds__(256) void dec_sample_draw_kernel(const float* vlog, int ldv, const T* pfeat, const T* h, T* hid_cache,
                                                              const float* sw_w, const float* sw_b, int64_t* tokens, int64_t* attach,
                                                              int32_t* first_end, const int32_t* t_dev, int Tmax, int d, int V,
                                                              int end_tok, int pad_tok, const SampleParamsDev* prm, float* scores,
                                                              const PrefixDev px, const ConstraintDev cs) {
    __shared__ float plog[MAX_T];
    __shared__ float sp[SAMPLE_MAX_C], sw[SAMPLE_MAX_C];           // p and w of candidate i
    __shared__ float sh[4], scan[4];
    __shared__ int shi[4];
    __shared__ float s_sw, s_W;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = *t_dev;
    const T* hb = h + (int64_t)r * d;
    const int64_t nb = gridDim.x;
    T* cache = hid_cache + (int64_t)r * d;                          // [Tmax][rows][d], as in dec_sample_kernel
    for (int c = tid; c < d; c += 256) cache[(int64_t)t * nb * d + c] = hb[c];
    if (first_end[r] >= 0) {                                        // finished: frozen (uniform branch: one row per block)
        if (tid == 0) { tokens[(int64_t)r * Tmax + t] = pad_tok; attach[(int64_t)r * Tmax + t] = -1; }
        return;
    }
    const SampleParamsDev P = *prm;
    const float* vr = vlog + (int64_t)r * ldv;
    const RowDist rd = row_dist_prepare<T>(vr, V, pfeat + (int64_t)r * d, hb, cache, nb, t, d, sw_w, sw_b, plog, sh, &s_sw);
    if (px.plen && t < px.plen[r]) {                                // forced live row (section 14): no draw, u is not consumed
        if (tid == 0) {
            const Forced f = forced_candidate(px, r, t, Tmax, rd, vr, V, plog, tokens);
            tokens[(int64_t)r * Tmax + t] = f.tok;
            attach[(int64_t)r * Tmax + t] = f.att;
            scores[r] += f.lp;
            px.score[r] += f.lp;
            if (f.tok == end_tok) first_end[r] = t;
        }
        return;
    }
    const int nc = t + 1 < 6 ? V : V + t;                           // candidates: vocab, then the pointers j < t
    // (section 15: a disallowed candidate is staged with p = 0, i.e. as no candidate - the allowed ones with p > 0 are the candidate set
    // of everything below, and the chosen one's sp is its own unfiltered p)
    const Allow al = make_allow(cs, tokens + (int64_t)r * Tmax, V, t);
    float pmax = -INFINITY;
    row_dist_visit(rd, vr, V, plog, t, t, al, [&](float p, int i, bool ok) { p = ok ? p : 0.f; sp[i] = p; pmax = fmaxf(pmax, p); });
    pmax = block_max(pmax, sh);                                     // (its barriers also publish sp)
    const float tau = P.temperature, lpmax = logf(pmax);
    for (int i = tid; i < nc; i += 256) {
        const float p = sp[i];
        sw[i] = !(p > 0.f) ? 0.f : (tau == 1.0f ? p / pmax : expf((logf(p) - lpmax) / tau));
    }
    __syncthreads();
    const uint32_t hi0 = __float_as_uint(pmax) + 1;                 // no candidate's p bits reach this
    auto pbits = [&](int i) { return __float_as_uint(sp[i]); };
    // keep the rank-order prefix {p bits > th} + {p bits == th, index <= ith}: zero the others' w
    auto cut = [&](uint32_t th, int ith) {
        for (int i = tid; i < nc; i += 256) {
            const uint32_t pb = pbits(i);
            if (!(pb > th || (pb == th && i <= ith))) sw[i] = 0.f;
        }
        __syncthreads();
    };
    if (P.top_k > 0) {
        auto count_ge = [&](uint32_t th) {                          // candidates with p > 0 and p bits >= th
            int c = 0;
            for (int i = tid; i < nc; i += 256) c += (sp[i] > 0.f && pbits(i) >= th) ? 1 : 0;
            return block_sum_i(c, shi);
        };
        const int n_pos = count_ge(1u);
        if (n_pos > P.top_k) {                                      // (otherwise top-k keeps every candidate)
            uint32_t lo = 1u, hi = hi0;                             // count_ge(lo) >= k > count_ge(hi)
            int c_hi = 0, c_lo = n_pos;
            while (hi - lo > 1u) {
                const uint32_t mid = lo + (hi - lo) / 2;
                const int c = count_ge(mid);
                if (c >= P.top_k) { lo = mid; c_lo = c; } else { hi = mid; c_hi = c; }
            }
            const int need = P.top_k - c_hi;                        // taken from the tie group p bits == lo, smaller indices first
            int ith = nc - 1;
            if (c_lo - c_hi > need) {
                int ilo = -1, ihi = nc - 1;                         // count(group, index <= ilo) < need <= count(group, index <= ihi)
                while (ihi - ilo > 1) {
                    const int mid = ilo + (ihi - ilo) / 2;
                    int c = 0;
                    for (int i = tid; i <= mid; i += 256) c += (sp[i] > 0.f && pbits(i) == lo) ? 1 : 0;
                    if (block_sum_i(c, shi) >= need) ihi = mid; else ilo = mid;
                }
                ith = ihi;
            }
            cut(lo, ith);
        }
    }
    if (P.top_p < 1.0f) {
        auto wsum = [&](uint32_t th, int ith) {                     // fixed-order sum of the kept w inside the prefix (th, ith)
            float s = 0.f;
            for (int i = tid; i < nc; i += 256) {
                const uint32_t pb = pbits(i);
                s += (pb > th || (pb == th && i <= ith)) ? sw[i] : 0.f;
            }
            return block_sum(s, sh);
        };
        const float target = P.top_p * wsum(0u, nc - 1);            // (> 0: the top candidate is kept with w = 1)
        uint32_t lo = 0u, hi = hi0;                                 // wsum over p bits >= lo reaches target, over >= hi not
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (wsum(mid, nc - 1) >= target) lo = mid; else hi = mid;
        }
        int c = 0;
        for (int i = tid; i < nc; i += 256) c += (pbits(i) == lo && sw[i] > 0.f) ? 1 : 0;
        int ith = nc - 1;
        if (block_sum_i(c, shi) > 1) {
            int ilo = -1, ihi = nc - 1;                             // wsum(lo, ilo) < target <= wsum(lo, ihi)
            while (ihi - ilo > 1) {
                const int mid = ilo + (ihi - ilo) / 2;
                if (wsum(lo, mid) >= target) ihi = mid; else ilo = mid;
            }
            ith = ihi;
        }
        cut(lo, ith);
    }
    // the draw: thread tid owns candidates [i0, i1) in index order
    const int per = (nc + 255) / 256;
    const int i0 = min(tid * per, nc), i1 = min(i0 + per, nc);
    float part = 0.f;
    for (int i = i0; i < i1; ++i) part += sw[i];
    float inc = part;                                               // inclusive scan of the partial sums within the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
    }
    if (lane == 63) scan[wave] = inc;
    __syncthreads();
    float off = 0.f;
    for (int w = 0; w < wave; ++w) off += scan[w];
    float excl = __shfl_up(inc, 1);
    excl = lane == 0 ? off : off + excl;
    if (i0 < nc && i1 == nc) s_W = excl + part;                     // W: the prefix sum at the last candidate
    __syncthreads();
    const float uW = sample_u(P.seed, (uint32_t)(r / P.n), (uint32_t)(r % P.n), (uint32_t)t) * s_W;
    int pick = 0x7fffffff, last = -1;
    {
        float loc = 0.f;
        for (int i = i0; i < i1; ++i) {
            const float w = sw[i];
            loc += w;
            if (w > 0.f) {
                last = i;
                if (pick == 0x7fffffff && excl + loc > uW) pick = i;
            }
        }
    }
    pick = block_min_i(pick, shi);
    if (pick == 0x7fffffff) pick = -block_min_i(-last, shi);       // rounding left no crossing: the last kept candidate
    if (tid == 0) {
        // (the top candidate always has w = 1: pick >= 0 - unless no candidate has p > 0; constrained, that step writes an allowed token)
        const int idx = pick < 0 ? (al.on ? al.fallback() : 0) : pick;
        const TokAtt c = candidate_token(idx, V, tokens + (int64_t)r * Tmax);
        tokens[(int64_t)r * Tmax + t] = c.tok;
        attach[(int64_t)r * Tmax + t] = c.att;
        scores[r] += logf(sp[idx]);                                 // the untempered, unfiltered p
        if (c.tok == end_tok) first_end[r] = t;
    }
}

// The parameter block (by kernel argument: no host-to-device copy) and, at pa_decode_sample_begin, zero scores.
__global__ __launch_bounds__(256) void dec_sample_init_kernel(SampleParamsDev* prm, SampleParamsDev p, float* scores, int rows) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *prm = p;
    if (scores)
        for (int r = blockIdx.x * 256 + threadIdx.x; r < rows; r += gridDim.x * 256) scores[r] = 0.f;
}

// The prefix arena from the caller's table (device memory; section 14): lengths clamped to [0, Tmax], tokens and pointers narrowed to
// int32 (a value that does not fit becomes one that is no candidate), prefix_score and prefix_lp zero.
__global__ __launch_bounds__(256) void dec_prefix_init_kernel(int32_t* len, int32_t* tok, int32_t* att, float* score, float* lp,
                                                              const int32_t* plen, const int64_t* ptok, const int64_t* patt, int rows,
                                                              int Tmax) {
    const int64_t n = (int64_t)rows * Tmax;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t tk = ptok[i], at = patt[i];
        tok[i] = (tk < 0 || tk > 0x7fffffff) ? -1 : (int32_t)tk;
        att[i] = at < 0 ? -1 : (at > 0x7fffffff ? 0x7fffffff : (int32_t)at);
        lp[i] = 0.f;
        if (i < rows) { len[i] = min(max(plen[i], 0), Tmax); score[i] = 0.f; }
    }
}

__global__ void dec_advance_kernel(int32_t* t_dev) { if (threadIdx.x == 0) *t_dev += 1; }

// ------------------------------------------------------------------------------------------------
int linear(pa_model* m, const void* A, const void* W, const float* bias, void* Cout, int ldc, int M, int N, int K,
           int relu, const void* R, int out_dtype, void* st) {
    pa_gemm_args g; memset(&g, 0, sizeof(g));
    g.A = A; g.B = W; g.C = Cout; g.bias = bias; g.R = R;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = ldc; g.ldr = ldc;
    g.batch = 1; g.a_kcontig = 1; g.b_kcontig = 1;
    g.in_dtype = m->cfg.dtype; g.out_dtype = out_dtype < 0 ? m->cfg.dtype : out_dtype;
    g.alpha = 1.f; g.relu = relu; g.aux_scale = 1.f; g.splitk = 1;
    return pa_gemm(&g, st);
}

// y = LayerNorm(R + A W^T + bias): pa_gemm into `z` followed by pa_layernorm_fwd
int linear_ln(pa_model* m, const void* A, const void* W, const float* bias, const void* R, void* z, void* y, const float* gamma,
              const float* beta, float eps, int M, int K, void* st) {
    const pa_model_cfg& c = m->cfg;
    RC(linear(m, A, W, bias, z, c.d_model, M, c.d_model, K, 0, R, -1, st));
    return pa_layernorm_fwd(y, z, gamma, beta, m->dec->mean, m->dec->rstd, M, c.d_model, eps, c.dtype, st);
}

// C = epi(LayerNorm(Z) W^T + b) with the LayerNorm folded into the product (pa_gemm_norm_a); Y (optional) receives LayerNorm(Z)
int linear_norm_a(pa_model* m, const void* Z, const void* Wf, const float* u, const float* v, const float* gamma, const float* beta,
                  float eps, void* Y, void* Cout, int ldc, int M, int N, int K, int relu, void* st) {
    pa_gemm_args g; memset(&g, 0, sizeof(g));
    g.A = Z; g.B = Wf; g.C = Cout; g.bias = v;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = ldc;
    g.batch = 1; g.a_kcontig = 1; g.b_kcontig = 1; g.in_dtype = m->cfg.dtype; g.out_dtype = m->cfg.dtype;
    g.alpha = 1.f; g.relu = relu; g.aux_scale = 1.f; g.splitk = 1;
    pa_gemm_norm_ext x; memset(&x, 0, sizeof(x));
    x.u = u; x.gamma = gamma; x.beta = beta; x.y = Y; x.ldy = K; x.eps = eps;
    if (m->cfg.dtype == PA_F32) { x.zf = (const float*)Z; x.ldzf = K; x.y_f32 = 1; }     // exact-f32 fold: statistics from the rows themselves
    return pa_gemm_norm_a(&g, &x, st);
}

// f32-residual forms (bf16 step): Z (f32) = A W^T + bias + R (f32), with its bf16 copy for the next matrix product
int linear_res32(pa_model* m, const void* A, const void* W, const float* bias, const float* R, float* Z, void* Zb, int M, int N, int K, void* st) {
    pa_gemm_args g; memset(&g, 0, sizeof(g));
    g.A = A; g.B = W; g.C = Z; g.bias = bias; g.R = R; g.C_lp = Zb; g.ldc_lp = N;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N; g.ldr = N;
    g.batch = 1; g.a_kcontig = 1; g.b_kcontig = 1; g.in_dtype = PA_BF16; g.out_dtype = PA_F32;
    g.alpha = 1.f; g.aux_scale = 1.f; g.splitk = 1;
    return pa_gemm(&g, st);
}
// C (bf16) = epi(LayerNorm(Zf) W^T + b) with the product on the bf16 copy Zb and the statistics / Y (f32) from the f32 rows
int linear_norm_a32(pa_model* m, const void* Zb, const float* Zf, const void* Wf, const float* u, const float* v, const float* gamma,
                    const float* beta, float eps, float* Y, void* Cout, int ldc, int M, int N, int K, int relu, void* st) {
    (void)m;
    pa_gemm_args g; memset(&g, 0, sizeof(g));
    g.A = Zb; g.B = Wf; g.C = Cout; g.bias = v;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = ldc;
    g.batch = 1; g.a_kcontig = 1; g.b_kcontig = 1; g.in_dtype = PA_BF16; g.out_dtype = PA_BF16;
    g.alpha = 1.f; g.relu = relu; g.aux_scale = 1.f; g.splitk = 1;
    pa_gemm_norm_ext x; memset(&x, 0, sizeof(x));
    x.u = u; x.gamma = gamma; x.beta = beta; x.y = Y; x.ldy = K; x.eps = eps; x.zf = Zf; x.ldzf = K; x.y_f32 = 1;
    return pa_gemm_norm_a(&g, &x, st);
}

// =====================================================================================================
// Host side of the step: decode_switches() reads every switch once, plan_decode() - a pure function - turns (cfg, B, S, Tmax) into the
// forms the step takes and the bytes it needs; the layout, pa_decode_begin, the beam reorder and the step read that one value
// (DecodeLayout::plan).  pa_decode_plan reports it without a handle or a launch (tests/test_decode_plan_cpu.py pins it without a GPU).
struct DecodeSwitches {
    // step form
    int fold_ln;           // PLANK_DECODE_FOLD_LN (unset = -1: on at d_model 512 and at most 512 rows): 0 / 1 force the LayerNorm fold off / on
    int f32_resid;         // PLANK_DECODE_F32_RESID (1): 0 = the all-bf16 residual stream in the bf16 step
    int mq;                // PLANK_DECODE_MQ (1): 0 = per-layer cross-attention K / V caches in the bf16 step
    int mq_f32;            // PLANK_DECODE_MQ_F32 (1): the same for the exact-f32 step
    int mq_contract;       // PLANK_DECODE_MQ_CONTRACT (unset = -1: exact f32 only): 0 / 1 force W_v as its own launch off / on (dh 64)
    int mq_self;           // PLANK_DECODE_MQ_SELF (1): 0 = per-head self-attention K / V caches in the exact-f32 step
    int mq_self_bf16;      // PLANK_DECODE_MQ_SELF_BF16 (unset = -1: B >= mq_self_minb): 0 never, 1 always absorb the bf16 self-attention
    int mq_self_minb;      // PLANK_DECODE_MQ_SELF_MINB (200): fewest rows from which the bf16 self-attention is absorbed
    // range blocks of the absorbed launches (decode_mq.h mq_parts)
    int mq_parts;          // PLANK_DECODE_MQ_PARTS (0 = by rule): n > 0 forces n range blocks per row (at most 64), 1 = never
    int mq_mint;           // PLANK_DECODE_MQ_MINT (8): fewest key tiles of a range block
    int mq_pair;           // PLANK_DECODE_MQ_PAIR (1): 0 = one row per block in the absorbed cross launch of a decode group (even G, 2 H <= 16 slots)
    // kernel variants of the absorbed launches
    int mq_nt;             // PLANK_DECODE_MQ_NT (1): 0 = default-policy DMA instead of non-temporal (aux 2; measured in the step,
                           //   B 256 x 1024: 0.958 vs 0.989 ms)
    int mq_swap;           // PLANK_DECODE_MQ_SWAP (1): 0 = ds_bpermute row reductions instead of v_permlane*_swap
    int mq32_w8;           // PLANK_DECODE_MQ32_W8 (1): 0 = the four-wave f32 kernel (one wave per SIMD) instead of eight waves with skewed halves
};
const DecodeSwitches& decode_switches() {
    static const DecodeSwitches sw = [] {
        auto env = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        DecodeSwitches s;
        s.fold_ln = env("PLANK_DECODE_FOLD_LN", -1);
        s.f32_resid = env("PLANK_DECODE_F32_RESID", 1);
        s.mq = env("PLANK_DECODE_MQ", 1);
        s.mq_f32 = env("PLANK_DECODE_MQ_F32", 1);
        s.mq_contract = env("PLANK_DECODE_MQ_CONTRACT", -1);
        s.mq_self = env("PLANK_DECODE_MQ_SELF", 1);
        s.mq_self_bf16 = env("PLANK_DECODE_MQ_SELF_BF16", -1);
        s.mq_self_minb = env("PLANK_DECODE_MQ_SELF_MINB", 200);
        s.mq_parts = env("PLANK_DECODE_MQ_PARTS", 0);
        s.mq_mint = env("PLANK_DECODE_MQ_MINT", 8);
        s.mq_pair = env("PLANK_DECODE_MQ_PAIR", 1);
        s.mq_nt = env("PLANK_DECODE_MQ_NT", 1);
        s.mq_swap = env("PLANK_DECODE_MQ_SWAP", 1);
        s.mq32_w8 = env("PLANK_DECODE_MQ32_W8", 1);
        return s;
    }();
    return sw;
}

// The decode workspace for plan `pl`; base NULL is the size query (L then holds no pointers).
// B rows over Bd drawings (B = Bd x G): what the cross-attention reads - mem, kpm, cu_store, cross_k / cross_v, kv_tmp - is per drawing.
size_t dec_layout(const pa_model_cfg& c, const DecodePlan& pl, DecodeLayout* L, char* base, int Bd, int B, int S, int Tmax) {
    const size_t e = c.dtype == PA_BF16 ? 2 : 4, d = c.d_model, ff = c.d_ff;
    Arena a{base, 0};
    L->B = B; L->S = S; L->Tmax = Tmax; L->Bd = Bd; L->G = B / Bd;
    L->cross_k.assign(c.n_dec, nullptr); L->cross_v.assign(c.n_dec, nullptr); L->self_k.resize(c.n_dec); L->self_v.resize(c.n_dec);
    L->wo_t.assign(c.n_dec, nullptr); L->bo_t.assign(c.n_dec, nullptr);
    for (int i = 0; i < c.n_dec; ++i) {
        if (!pl.mq) { L->cross_k[i] = a.take((size_t)Bd * S * d * e); L->cross_v[i] = a.take((size_t)Bd * S * d * e); }
        L->self_k[i] = a.take((size_t)B * Tmax * d * e); L->self_v[i] = a.take((size_t)B * Tmax * d * e);
    }
    L->mem = L->qt = L->ctx = L->mq_sp = nullptr;
    if (pl.mq) {
        const size_t H = c.n_head;
        L->mem = a.take((size_t)Bd * S * d * e);
        L->qt = a.take((size_t)B * H * d * e); L->ctx = a.take((size_t)B * H * d * e);
        if (pl.mq_sp_bytes > 0) L->mq_sp = a.take((size_t)pl.mq_sp_bytes);
        for (int i = 0; i < c.n_dec; ++i) { L->wo_t[i] = a.take(d * H * d * e); L->bo_t[i] = (float*)a.take(d * 4); }
        L->wvt_self.assign(c.n_dec, nullptr);
        if (c.dtype == PA_F32) for (int i = 0; i < c.n_dec; ++i) L->wvt_self[i] = a.take(d * d * e);
        L->wo_ts.assign(c.n_dec, nullptr); L->bo_ts.assign(c.n_dec, nullptr);
        if (c.dtype == PA_BF16) for (int i = 0; i < c.n_dec; ++i) { L->wo_ts[i] = a.take(d * H * d * e); L->bo_ts[i] = (float*)a.take(d * 4); }
    }
    L->kv_tmp = pl.mq ? nullptr : a.take((size_t)Bd * S * 2 * d * e);
    L->hid_cache = a.take((size_t)B * Tmax * d * e);
    // (x / y / z / z2 are sized for f32 rows: the bf16 step keeps its residual stream in f32, `f32res`)
    L->x = a.take(B * d * 4); L->qkv = a.take(B * 3 * d * e); L->ao = a.take(B * d * e); L->z = a.take(B * d * 4);
    L->y = a.take(B * d * 4); L->q = a.take(B * d * e); L->ff = a.take(B * ff * e); L->pfeat = a.take(B * d * e);
    L->h = a.take(B * d * e);
    L->zb = a.take(B * d * 2); L->z2b = a.take(B * d * 2); L->xb = a.take(B * d * 2); L->hf = (float*)a.take(B * d * 4);
    L->vlog = (float*)a.take((size_t)B * ((c.vocab + 7) / 8 * 8) * 4);
    L->mean = (float*)a.take(B * 4); L->rstd = (float*)a.take(B * 4);
    L->tokens = (int64_t*)a.take((size_t)B * Tmax * 8); L->attach = (int64_t*)a.take((size_t)B * Tmax * 8);
    L->first_end = (int32_t*)a.take(B * 4); L->t_dev = (int32_t*)a.take(256);
    L->kpm = (uint8_t*)a.take((size_t)Bd * S);
    L->cu_store = (int32_t*)a.take((size_t)(Bd + 1) * 4);
    L->z2 = a.take(B * d * 4);
    for (int k = 0; k < 3; ++k) { L->fw[k].resize(c.n_dec); L->fu[k].resize(c.n_dec); L->fv[k].resize(c.n_dec); }
    for (int i = 0; i < c.n_dec; ++i) {
        const size_t rows[3] = {3 * d, d, ff};
        for (int k = 0; k < 3; ++k) {
            L->fw[k][i] = a.take(rows[k] * d * e);          // folded weight in the step's dtype (bf16, or f32 for the exact-f32 step)
            L->fu[k][i] = (float*)a.take(rows[k] * 4); L->fv[k][i] = (float*)a.take(rows[k] * 4);
        }
    }
    return a.off;
}

template <typename T>
int launch_attn(int d, int H, T* out, const T* q, int ldq, T* kc, T* vc, int Lmax, const uint8_t* kpm,
                int fixed_lk, const int32_t* t_dev, int B, void* st, const int32_t* cu = nullptr, const T* newkv = nullptr, int G = 1) {
    const int dh = d / H;
    const float scale = 1.0f / sqrtf((float)dh);
    dim3 grid(H, B);
    hipStream_t s = (hipStream_t)st;
    switch (dh) {
        case 16: PA_LAUNCH((dec_attn_kernel<T, 16>), grid, dim3(256), 0, s, out, q, ldq, kc, vc, Lmax, kpm, fixed_lk, t_dev, d, scale, cu, newkv, G); break;
        case 32: PA_LAUNCH((dec_attn_kernel<T, 32>), grid, dim3(256), 0, s, out, q, ldq, kc, vc, Lmax, kpm, fixed_lk, t_dev, d, scale, cu, newkv, G); break;
        case 64: PA_LAUNCH((dec_attn_kernel<T, 64>), grid, dim3(256), 0, s, out, q, ldq, kc, vc, Lmax, kpm, fixed_lk, t_dev, d, scale, cu, newkv, G); break;
        default: return PA_ESHAPE;
    }
    return 0;
}

// Segment table of the beam history reorder (dec_beam_copy_kernel) for `rows` hypothesis rows of a step planned as `pl`; L may be NULL
// (the workspace query).  Returns the scratch bytes of one row, or a negative PA_E* code.
int64_t beam_segments(const pa_model_cfg& c, const DecodePlan& pl, const DecodeLayout* L, int rows, int Tmax, BeamCopy* cp) {
    const int64_t e = c.dtype == PA_BF16 ? 2 : 4, d = c.d_model, H = c.n_head, dh = d / H;
    int n = 0;
    int64_t off = 0;
    auto add = [&](void* ptr, int64_t row_stride, int outer, int64_t outer_stride, int unit, int by_pos, int pos_add) {
        if (n >= BEAM_MAX_SEG) { n = BEAM_MAX_SEG + 1; return; }
        BeamSeg& g = cp->seg[n++];
        g.ptr = (char*)ptr; g.row_stride = row_stride; g.outer = outer; g.outer_stride = outer_stride; g.unit = unit;
        g.by_pos = by_pos; g.pos_add = pos_add; g.pad_ = 0;
        g.vec16 = (unit % 16 == 0 && row_stride % 16 == 0 && outer_stride % 16 == 0) ? 1 : 0;
        g.scr_off = off; g.scr_outer = by_pos ? unit : (int64_t)Tmax * unit;
        off += ((by_pos ? (int64_t)Tmax * unit : (int64_t)outer * Tmax * unit) + 15) / 16 * 16;
    };
    for (int i = 0; i < c.n_dec; ++i) {
        if (pl.mq_self || pl.mq_self_bf) {      // row cache of the layer inputs [rows][Tmax][d] (self_v is not read in these forms)
            add(L ? L->self_k[i] : nullptr, Tmax * d * e, 1, 0, (int)(d * e), 0, 1);
        } else {                                // per-head K / V caches [rows][H][Tmax][dh]
            add(L ? L->self_k[i] : nullptr, H * Tmax * dh * e, (int)H, Tmax * dh * e, (int)(dh * e), 0, 1);
            add(L ? L->self_v[i] : nullptr, H * Tmax * dh * e, (int)H, Tmax * dh * e, (int)(dh * e), 0, 1);
        }
    }
    add(L ? L->hid_cache : nullptr, d * e, 0, (int64_t)rows * d * e, (int)(d * e), 1, 1);     // [Tmax][rows][d]
    add(L ? (void*)L->tokens : nullptr, (int64_t)Tmax * 8, 1, 0, 8, 0, 0);                    // positions 0 .. t-1
    add(L ? (void*)L->attach : nullptr, (int64_t)Tmax * 8, 1, 0, 8, 0, 0);
    if (n > BEAM_MAX_SEG) return PA_ESHAPE;
    cp->nseg = n; cp->pad_ = 0;
    cp->scr_row = (off + 255) / 256 * 256;
    return cp->scr_row;
}

// Which forms the step takes and what it needs, from the configuration, the shape and the switches alone.
// fold: LayerNorm folded into its consumer Linear (bf16 decode): 17 LayerNorm launches fewer per step.
// On the ring kernel (gemm3s_kernel's prologue statistics pass) this was MEASURED NULL on MI355X (B 256, 1024 steps, one lane:
// 1.228 ms / step folded against 1.210 - the statistics pass pays the memory round trips the LayerNorm launch paid).  On
// gemm_skinny_kernel the Z tile is resident in LDS and the statistics cost no round trip: 1.072 against 1.089 ms / step.  So: on by
// default exactly where pa_gemm_norm_a takes the skinny kernel (d_model 512, at most 512 rows); PLANK_DECODE_FOLD_LN=0 / 1 forces.
// The exact-f32 step folds too since round 4 (pa_ln_fold_weights_f32 + the f32 skinny kernel with the statistics taken from
// the rows themselves): 17 LayerNorm launches fewer per step - measured +0.5 % only (B 256: 1.995 vs 2.005 ms / step; the folded
// Linears re-read their rows for the statistics), token-exact against the reference in every decode test.  d_model 512, <= 512 rows.
// f32res: f32 residual stream inside the bf16 step (see DecodeLayout): on wherever every Linear of the step takes the skinny
// kernel (d_model 512, at most 512 rows).  tests/bf16_decode_sim.py / profiles/r04_bf16_decode_rounding_sim.txt: exact-prefix
// agreement with the f32 tokens 0.40 -> 0.63-0.70 on 32 rows x 128 steps.  PLANK_DECODE_F32_RESID=0 restores the all-bf16 step.
// mq: absorbed cross-attention (csrc/decode_mq.h) wherever the fold is on, with at most 8 heads; PLANK_DECODE_MQ=0 (bf16) /
// PLANK_DECODE_MQ_F32=0 (exact f32) restore the per-layer K / V caches.
// Decode groups (G > 1): Bd drawings x G rows.  Everything that depends on the row count - fold, f32res, mq_self_bf,
// the 512-row limits, the self launches' range blocks - is decided for B = Bd G rows; the memory side of the layout is Bd drawings'.  The
// absorbed cross launch puts two rows of a drawing into one block (group.rows_per_block 2: the 16 head slots of the score tile hold
// 2 x 8 heads, decode_mq.h) when G is even and 2 n_head <= 16; PLANK_DECODE_MQ_PAIR=0 keeps one row per block.  Its range blocks are
// per unit (block of rows).  With G 1 the plan is the ungrouped one, field for field.
DecodePlan plan_decode(const pa_model_cfg& c, int Bd, int G, int S, int Tmax, const DecodeSwitches& sw) {
    DecodePlan r{};
    const int d = c.d_model;
    // (the configuration checks are pa_model_create's: no handle exists for a cfg that fails them)
    if (d <= 0 || c.n_head <= 0 || d % c.n_head || (c.dtype != PA_F32 && c.dtype != PA_BF16)) { r.status = PA_EINVAL; return r; }
    const int dh = d / c.n_head;
    if ((dh != 16 && dh != 32 && dh != 64) || d % 8 || c.d_ff % 8) { r.status = PA_ESHAPE; return r; }
    if (Bd <= 0 || S <= 0 || Tmax <= 0 || Tmax > MAX_T || c.n_dec < 0 || G < 1 || G > PA_SAMPLE_MAX) { r.status = PA_EINVAL; return r; }
    if (Bd > INT32_MAX / G) { r.status = PA_EINVAL; return r; }
    const int B = Bd * G;                      // rows
    const bool f32 = c.dtype == PA_F32;
    const bool fold_env = sw.fold_ln >= 0 ? sw.fold_ln != 0 : (d == 512 && B <= 512);
    r.fold = fold_env && !f32 && d % 64 == 0 && c.d_ff % 32 == 0 && c.d_ff >= d && (size_t)((B + 63) / 64) * ((3 * d + 63) / 64) <= 512;
    if (f32) r.fold = fold_env && d == 512 && B <= 512 && c.d_ff % 32 == 0 && c.d_ff >= d;   // (N < K: pa_gemm_norm_a's f32 form cannot materialise y - ADVICE r4)
    r.f32res = r.fold && !f32 && sw.f32_resid != 0 && d == 512 && B <= 512 && c.d_ff % 512 == 0;
    r.mq = r.fold && (f32 ? sw.mq_f32 != 0 : sw.mq != 0) && d == MQ_D && B <= 512 && c.n_head <= MQ_MAXH &&
           S <= (f32 ? 16000 : MQ_MAXS);     // (f32: launch_cross_mq32 keeps 16 KB of partial-score slots beside the ring)
    r.mq_contract = r.mq && dh == 64 && (sw.mq_contract >= 0 ? sw.mq_contract != 0 : f32);
    // exact f32: the self-attention in the same form - the step caches the layer-input rows x_t instead of K and V (half the bytes of what is
    // then the largest stream of the f32 step), q~ = W_k^T q, W_v behind the softmax (q . b_k cancels, b_v is added once).  PLANK_DECODE_MQ_SELF=0.
    r.mq_self = r.mq && r.mq_contract && f32 && sw.mq_self != 0 && Tmax <= 16000;
    // bf16 (round 6; needs the f32 residual stream's step form): pays from ~200 batch elements on - measured in one session, B 256 x 1024 steps:
    // 0.969 -> 0.929 ms / step (264 k -> 276 k tokens/s; half the bytes of the self-attention stream against one more launch and a K = H d
    // out-projection per layer); B 64: 0.557 -> 0.662, B 16: 0.476 -> 0.609 (profiles/r06_decode_self_absorbed.txt).
    // PLANK_DECODE_MQ_SELF_BF16: 0 never, 1 always, unset = B >= PLANK_DECODE_MQ_SELF_MINB (200).
    r.mq_self_bf = r.mq && !r.mq_contract && !f32 && r.f32res && dh == 64 && Tmax <= MQ_MAXS &&
                   (sw.mq_self_bf16 >= 0 ? sw.mq_self_bf16 != 0 : B >= sw.mq_self_minb);
    r.mq_nt = sw.mq_nt; r.mq_swap = sw.mq_swap; r.mq32_w8 = sw.mq32_w8;
    if (r.mq) {
        r.group.rows_per_block = (sw.mq_pair != 0 && G % 2 == 0 && 2 * c.n_head <= MQ_SLOTS) ? 2 : 1;
        r.group.units = B / r.group.rows_per_block;
        const int ps = mq_parts(r.group.units, S, sw.mq_parts, sw.mq_mint), pt = mq_parts(B, Tmax, sw.mq_parts, sw.mq_mint);
        r.parts_cross = ps;
        if (r.mq_self || r.mq_self_bf) r.parts_self = pt;
        // (sized for either launch, whichever self-attention form the step takes; one ticket area, of the B rows - mq_split_bytes)
        r.mq_sp_bytes = std::max(mq_split_bytes(r.group.units, ps, B), mq_split_bytes(B, pt, B));
    }
    if (!r.mq) { r.group.rows_per_block = 1; r.group.units = B; }
    r.group.rows = B; r.group.mem_rows = (int64_t)Bd * S;
    DecodeLayout sizes;
    BeamCopy cp;
    r.ws_bytes = (int64_t)dec_layout(c, r, &sizes, nullptr, Bd, B, S, Tmax) + 256;
    r.scr_row = beam_segments(c, r, nullptr, B, Tmax, &cp);    // (negative: the PA_E* code pa_decode_beam_ws_bytes answers with)
    return r;
}


// Beam workspace: scores f32 [rows], finished / parent int32 [rows], candidates (f32 log p, int32 token, int32 attach) [rows][K], then
// the reorder scratch [rows][scr_row].  The mode layouts (this one, sample_layout, prefix_layout): base NULL is the size query and
// leaves L alone (L may be NULL).
size_t beam_layout(DecodeLayout* L, char* base, int rows, int K, int64_t scr_row) {
    Arena a{base, 0};
    const size_t row = (size_t)rows * 4, cand = row * K;
    void *score = a.take(row), *fin = a.take(row), *parent = a.take(row);
    void *clp = a.take(cand), *ctok = a.take(cand), *catt = a.take(cand);
    void* scratch = a.take((size_t)rows * scr_row);
    if (base) {
        L->bm_score = (float*)score; L->bm_fin = (int32_t*)fin; L->bm_parent = (int32_t*)parent;
        L->bm_clp = (float*)clp; L->bm_ctok = (int32_t*)ctok; L->bm_catt = (int32_t*)catt;
        L->bm_copy.scratch = (char*)scratch;
    }
    return a.off;
}

// The prefix table as the end-of-step kernels take it (no table: all NULL, and the kernels do what they did without it).
PrefixDev prefix_arg(const pa_model* m) {
    const DecodeLayout* L = m->dec;
    if (!L->px_on) return PrefixDev{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    return PrefixDev{L->px_len, L->px_tok, L->px_att, L->px_score, L->px_lp, m->cfg.pad, 0};
}

// The constraint as the end-of-step kernels take it (none: off, and the kernels select among every candidate as without this argument).
ConstraintDev constraint_arg(const pa_model* m) {
    const DecodeLayout* L = m->dec;
    if (!L->cs_on) return ConstraintDev{0, 0, 0, 0, 0};
    return ConstraintDev{1, L->cs.n_val, m->cfg.end, L->cs.min_planks, std::min(L->cs.max_planks, (L->Tmax - 1) / 6)};
}

// The end of a greedy step: arg-max (or the forced candidate) per row.
template <typename T>
int greedy_tail(pa_model* m, int ldv, hipStream_t s) {
    const pa_model_cfg& c = m->cfg;
    DecodeLayout* L = m->dec;
    const int tl = m->tail();
    PA_LAUNCH(dec_sample_kernel<T>, dim3(L->B), dim3(256), 0, s, L->vlog, ldv, (const T*)L->pfeat, (const T*)L->h, (T*)L->hid_cache,
              (const float*)m->pf[tl + T_SW_W], (const float*)m->pf[tl + T_SW_B], L->tokens, L->attach, L->first_end, L->t_dev, L->Tmax,
              c.d_model, c.vocab, c.end, prefix_arg(m), constraint_arg(m));
    return 0;
}

// The end of a beam step (in place of dec_sample_kernel): candidates, merge, history reorder.  The next step's input embedding is
// dec_embed_kernel at the start of the next step (it reads the token at t - 1 of each row, i.e. of the new beam).
template <typename T>
int beam_tail(pa_model* m, int ldv, hipStream_t s) {
    const pa_model_cfg& c = m->cfg;
    DecodeLayout* L = m->dec;
    const int rows = L->B, K = L->beamK, tl = m->tail();
    PA_LAUNCH(dec_beam_cand_kernel<T>, dim3(rows), dim3(256), 0, s, L->vlog, ldv, (const T*)L->pfeat, (const T*)L->h, (T*)L->hid_cache,
              (const float*)m->pf[tl + T_SW_W], (const float*)m->pf[tl + T_SW_B], L->tokens, L->bm_fin, L->t_dev, L->Tmax, c.d_model, c.vocab,
              K, c.pad, L->bm_clp, L->bm_ctok, L->bm_catt, prefix_arg(m), constraint_arg(m));
    PA_LAUNCH(dec_beam_merge_kernel, dim3(rows / K), dim3(256), 0, s, L->bm_clp, L->bm_ctok, L->bm_catt, L->bm_score, L->bm_fin,
              L->first_end, L->bm_parent, L->tokens, L->attach, L->t_dev, L->Tmax, K, c.end);
    if (K > 1) {
        const dim3 g(std::max(4, std::min(64, 4096 / rows)), rows);
        PA_LAUNCH(dec_beam_copy_kernel, g, dim3(256), 0, s, L->bm_copy, L->bm_parent, L->t_dev, 0);
        PA_LAUNCH(dec_beam_copy_kernel, g, dim3(256), 0, s, L->bm_copy, L->bm_parent, L->t_dev, 1);
    }
    return 0;
}

// The end of a sampling step (in place of dec_sample_kernel): one draw per row.  The next step's input embedding is dec_embed_kernel at
// the start of the next step, as for beam search - the same launch count as the greedy step.
template <typename T>
int sample_tail(pa_model* m, int ldv, hipStream_t s) {
    const pa_model_cfg& c = m->cfg;
    DecodeLayout* L = m->dec;
    const int tl = m->tail();
    PA_LAUNCH(dec_sample_draw_kernel<T>, dim3(L->B), dim3(256), 0, s, L->vlog, ldv, (const T*)L->pfeat, (const T*)L->h, (T*)L->hid_cache,
              (const float*)m->pf[tl + T_SW_W], (const float*)m->pf[tl + T_SW_B], L->tokens, L->attach, L->first_end, L->t_dev, L->Tmax,
              c.d_model, c.vocab, c.end, c.pad, (const SampleParamsDev*)L->sm_prm, L->sm_score, prefix_arg(m),
              constraint_arg(m));
    return 0;
}

// The end of every step, whatever the mode and the residual-stream form: the mode's choice of a token per row, then the step counter.
// (The next step's embedding is dec_embed_kernel at its start.  A fused tail - embedding and counter inside dec_sample_kernel, norm3 +
// decoder.norm in one launch, PLANK_DECODE_FUSE_TAIL - was built, MEASURED NULL on MI355X in round 5 (B 256 x 1024 steps under graph
// replay: bf16 1.0905 ms / step fused against 1.0794, f32 1.9954 against 1.9813) and removed.)
template <typename T>
int end_of_step(pa_model* m, int ldv, hipStream_t s) {
    DecodeLayout* L = m->dec;
    if (L->beamK > 0) RC(beam_tail<T>(m, ldv, s));
    else if (L->sampleN > 0) RC(sample_tail<T>(m, ldv, s));
    else RC(greedy_tail<T>(m, ldv, s));
    PA_LAUNCH(dec_advance_kernel, dim3(1), dim3(64), 0, s, L->t_dev);
    return 0;
}

// ---- one decode step: the embedding, then per layer the self-attention, cross-attention and feed-forward blocks, then the tail -------
// The attention launches are the HBM-bound third of the step (they stream the caches); everything between them is a chain of
// latency-bound launches on B rows.

// self-attention of layer i over the per-head K / V caches (the kernel appends this step's K / V rows itself)
template <typename T>
int self_attn(pa_model* m, int i, void* st) {
    DecodeLayout* L = m->dec;
    const int d = m->cfg.d_model;
    return launch_attn<T>(d, m->cfg.n_head, (T*)L->ao, (const T*)L->qkv, 3 * d, (T*)L->self_k[i], (T*)L->self_v[i], L->Tmax, nullptr, 0, L->t_dev, L->B, st,
                          nullptr, (const T*)L->qkv);
}
// cross-attention of layer i over the per-head K / V caches of the memory (one set per drawing: the G rows of a group share it)
template <typename T>
int cross_attn(pa_model* m, int i, void* st) {
    DecodeLayout* L = m->dec;
    return launch_attn<T>(m->cfg.d_model, m->cfg.n_head, (T*)L->ao, (const T*)L->q, m->cfg.d_model, (T*)L->cross_k[i], (T*)L->cross_v[i], L->S, L->cu ? nullptr : L->kpm,
                          L->S, L->t_dev, L->B, st, L->cu, (const T*)nullptr, L->G);
}

// Absorbed attention (csrc/decode_mq.h) of the query rows in L->q over `nk` rows per element of `cache`: q~_h = scale log2e W_k,h^T q_h
// for all heads (-> L->qt), then attention over the cached rows themselves (-> L->ctx); the caller applies W_v / W_o behind it.
//   cross-attention: cache = the memory rows, nk = S, with the key-padding mask or the packed offsets, no t_dev, no xrow;
//   self-attention:  cache = the layer-input rows so far, nk = Tmax of which t_dev + 1 count; the expand launch appends this step's
//                    row from `xrow` (the residual stream's x) to the cache.
//   G / rpb (cross-attention of a decode group): G rows share a drawing's `cache` rows, rpb of them a block (decode_mq.h mq_units).
template <typename T, typename XT>
int absorbed_attn(pa_model* m, const T* Wk, T* cache, int nk, int nparts, const int32_t* t_dev, const uint8_t* kpm, const int32_t* cu,
                  const XT* xrow, hipStream_t s, int G = 1, int rpb = 1) {
    DecodeLayout* L = m->dec;
    const DecodePlan& pl = L->plan;
    const int d = m->cfg.d_model, H = m->cfg.n_head, B = L->B;
    const float sl = LOG2E_F / sqrtf((float)(d / H));
    const dim3 xg((B + MQ_XR - 1) / MQ_XR, H);
    T* const xcache = xrow ? cache : nullptr;
    const int xT = xrow ? L->Tmax : 0;
    if (d / H == 64) PA_LAUNCH((mq_expand_q_kernel<64, T, XT>), xg, dim3(512), 0, s, (T*)L->qt, (const T*)L->q, d, Wk, B, d, H, sl, xrow, xcache, t_dev, xT);
    else if constexpr (std::is_same<T, XT>::value) PA_LAUNCH((mq_expand_q_kernel<0, T, XT>), xg, dim3(512), 0, s, (T*)L->qt, (const T*)L->q, d, Wk, B, d, H, sl, xrow, xcache, t_dev, xT);
    else return PA_ESHAPE;
    if constexpr (sizeof(T) == 2)
        return launch_cross_mq((bf16*)L->ctx, (const bf16*)L->qt, (const bf16*)cache, kpm, cu, B, nk, H, d, s, nparts, pl.mq_nt, pl.mq_swap,
                               L->mq_sp, pl.mq_sp_bytes, t_dev, G, rpb, B);
    else
        return launch_cross_mq32((float*)L->ctx, (const float*)L->qt, (const float*)cache, kpm, cu, B, nk, H, d, s, nparts, pl.mq32_w8, t_dev,
                                 L->mq_sp, pl.mq_sp_bytes, G, rpb, B);
}

// The residual stream of the folded step in its two number formats.  Pre-norm rows live in z (k = 0) / z2 (k = 1), normed rows in x / y.
//   add:         pre-norm buffer k = A W^T + bias + R                                   (Linear + residual)
//   norm_linear: Cout = epi(LayerNorm(pre-norm buffer k) Wf^T + v), Y = the normed rows   (pa_gemm_norm_a with the folded weights of
//                `site` - DecodeLayout::fw - of layer i)
template <typename T>
struct StreamSame {        // rows in the step's dtype
    typedef T row_t;
    pa_model* m; void* st;
    int row_dtype() const { return m->cfg.dtype; }
    const void* x_operand() const { return m->dec->x; }
    int add(const void* A, const void* W, const float* bias, const void* R, int k, int K) const {
        DecodeLayout* L = m->dec;
        return linear(m, A, W, bias, k ? L->z2 : L->z, m->cfg.d_model, L->B, m->cfg.d_model, K, 0, R, -1, st);
    }
    int norm_linear(int k, int site, int i, const float* gamma, const float* beta, void* Y, void* Cout, int N, int relu) const {
        DecodeLayout* L = m->dec;
        return linear_norm_a(m, k ? L->z2 : L->z, L->fw[site][i], L->fu[site][i], L->fv[site][i], gamma, beta, m->cfg.eps_layer, Y, Cout, N,
                             L->B, N, m->cfg.d_model, relu, st);
    }
};
struct StreamF32 {         // bf16 step, f32 rows: x / y / z / z2 hold f32, zb / z2b / xb their bf16 copies = the matrix operands (plan.f32res)
    typedef float row_t;
    pa_model* m; void* st;
    int row_dtype() const { return PA_F32; }
    const void* x_operand() const { return m->dec->xb; }
    int add(const void* A, const void* W, const float* bias, const void* R, int k, int K) const {
        DecodeLayout* L = m->dec;
        return linear_res32(m, A, W, bias, (const float*)R, (float*)(k ? L->z2 : L->z), k ? L->z2b : L->zb, L->B, m->cfg.d_model, K, st);
    }
    int norm_linear(int k, int site, int i, const float* gamma, const float* beta, void* Y, void* Cout, int N, int relu) const {
        DecodeLayout* L = m->dec;
        return linear_norm_a32(m, k ? L->z2b : L->zb, (const float*)(k ? L->z2 : L->z), L->fw[site][i], L->fu[site][i], L->fv[site][i], gamma,
                               beta, m->cfg.eps_layer, (float*)Y, Cout, N, L->B, N, m->cfg.d_model, relu, st);
    }
};

// The layers of the folded step (plan.fold) over residual stream `rs`.  Every LayerNorm but the last rides in the Linear behind it:
//   self:  q (k, v) = norm3(z of the layer before) W_in^T, x = the normed rows;  z2 = attention W_o^T + b + x
//   cross: q = norm1(z2) W_q^T, y = the normed rows;                             z2 = attention W_o^T + b + y
//   ffn:   ff = act(norm2(z2) W_1^T + b_1), x = the normed rows;                 z = ff W_2^T + b_2 + x
template <typename T, typename Stream>
int folded_layers(pa_model* m, const Stream& rs, void* st) {
    const pa_model_cfg& c = m->cfg;
    DecodeLayout* L = m->dec;
    const DecodePlan& pl = L->plan;
    const int d = c.d_model, ff = c.d_ff, H = c.n_head, B = L->B;
    hipStream_t s = (hipStream_t)st;
    auto PF = [&](int i) { return (const float*)m->pf[i]; };
    auto PL = [&](int i) { return (const void*)m->pl[i]; };
    typedef typename Stream::row_t XT;
    // FFN activation: ReLU rides in the first Linear's epilogue (relu flag); ACTIVATION gelu is a launch of its own behind it
    const bool gelu = c.activation == 2;
    const bool self_abs = pl.mq_self || pl.mq_self_bf;       // only the query rows are projected; K / V never exist
    void* const qout = self_abs ? L->q : L->qkv;
    const int nq = self_abs ? d : 3 * d;
    const dim3 vg((B + MQ_XR - 1) / MQ_XR, H);
    for (int i = 0; i < c.n_dec; ++i) {
        const int pb = m->dec_base(i);
        if (i > 0) {
            const int pp = m->dec_base(i - 1);
            RC(rs.norm_linear(0, 0, i, PF(pp + D_N3_W), PF(pp + D_N3_B), L->x, qout, nq, 0));
        } else {                                // the first layer's input is the embedding: nothing to fold
            RC(linear(m, rs.x_operand(), PL(pb + D_SA_IN_W), PF(pb + D_SA_IN_B), qout, nq, B, nq, d, 0, nullptr, -1, st));
        }
        if (self_abs) {
            RC((absorbed_attn<T, XT>(m, (const T*)PL(pb + D_SA_IN_W) + (size_t)d * d, (T*)L->self_k[i], L->Tmax, pl.parts_self, L->t_dev, nullptr,
                                     nullptr, (const XT*)L->x, s)));
            if (pl.mq_self)
                PA_LAUNCH(mq_contract_v_kernel<float>, vg, dim3(512), 0, s, (float*)L->ao, d, (const float*)L->ctx, (const float*)L->wvt_self[i],
                          PF(pb + D_SA_IN_B) + 2 * d, B, d, H);
        } else {
            RC(self_attn<T>(m, i, st));
        }
        if (pl.mq_self_bf) RC(rs.add(L->ctx, L->wo_ts[i], L->bo_ts[i], L->x, 1, H * d));   // W_o,h W_v,h on the context rows
        else RC(rs.add(L->ao, PL(pb + D_SA_OUT_W), PF(pb + D_SA_OUT_B), L->x, 1, d));
        RC(rs.norm_linear(1, 1, i, PF(pb + D_N1_W), PF(pb + D_N1_B), L->y, L->q, d, 0));
        if (pl.mq) {
            RC((absorbed_attn<T, T>(m, (const T*)PL(pb + D_CA_IN_W) + (size_t)d * d, (T*)L->mem, L->S, pl.parts_cross, nullptr,
                                    L->cu ? nullptr : L->kpm, L->cu, (const T*)nullptr, s, L->G, pl.group.rows_per_block)));
        } else {
            RC(cross_attn<T>(m, i, st));
        }
        if (pl.mq && pl.mq_contract) {
            PA_LAUNCH(mq_contract_v_kernel<T>, vg, dim3(512), 0, s, (T*)L->ao, d, (const T*)L->ctx, (const T*)L->wo_t[i], PF(pb + D_CA_IN_B) + 2 * d,
                      B, d, H);
            RC(rs.add(L->ao, PL(pb + D_CA_OUT_W), PF(pb + D_CA_OUT_B), L->y, 1, d));
        } else if (pl.mq) RC(rs.add(L->ctx, L->wo_t[i], L->bo_t[i], L->y, 1, H * d));      // W_o,h W_v,h on the context rows
        else RC(rs.add(L->ao, PL(pb + D_CA_OUT_W), PF(pb + D_CA_OUT_B), L->y, 1, d));
        RC(rs.norm_linear(1, 2, i, PF(pb + D_N2_W), PF(pb + D_N2_B), L->x, L->ff, ff, gelu ? 0 : 1));
        if (gelu) RC(pa_gelu_fwd(L->ff, L->ff, B, ff, ff, c.dtype, 0.f, 0, st));
        RC(rs.add(L->ff, PL(pb + D_L2_W), PF(pb + D_L2_B), L->x, 0, ff));
    }
    if (c.n_dec < 1) return 0;
    const int pb = m->dec_base(c.n_dec - 1);   // the last layer's norm3 has no Linear behind it: explicit
    return pa_layernorm_fwd(L->x, L->z, PF(pb + D_N3_W), PF(pb + D_N3_B), L->mean, L->rstd, B, d, c.eps_layer, rs.row_dtype(), st);
}

// The layers of the un-folded step: every LayerNorm a launch of its own (linear_ln), per-head K / V caches
template <typename T>
int plain_layers(pa_model* m, void* st) {
    const pa_model_cfg& c = m->cfg;
    DecodeLayout* L = m->dec;
    const int d = c.d_model, ff = c.d_ff, B = L->B;
    auto PF = [&](int i) { return (const float*)m->pf[i]; };
    auto PL = [&](int i) { return (const void*)m->pl[i]; };
    const bool gelu = c.activation == 2;
    for (int i = 0; i < c.n_dec; ++i) {
        const int pb = m->dec_base(i);
        RC(linear(m, L->x, PL(pb + D_SA_IN_W), PF(pb + D_SA_IN_B), L->qkv, 3 * d, B, 3 * d, d, 0, nullptr, -1, st));
        RC(self_attn<T>(m, i, st));
        RC(linear_ln(m, L->ao, PL(pb + D_SA_OUT_W), PF(pb + D_SA_OUT_B), L->x, L->z, L->y, PF(pb + D_N1_W), PF(pb + D_N1_B), c.eps_layer, B, d, st));
        RC(linear(m, L->y, PL(pb + D_CA_IN_W), PF(pb + D_CA_IN_B), L->q, d, B, d, d, 0, nullptr, -1, st));
        RC(cross_attn<T>(m, i, st));
        RC(linear_ln(m, L->ao, PL(pb + D_CA_OUT_W), PF(pb + D_CA_OUT_B), L->y, L->z, L->x, PF(pb + D_N2_W), PF(pb + D_N2_B), c.eps_layer, B, d, st));
        RC(linear(m, L->x, PL(pb + D_L1_W), PF(pb + D_L1_B), L->ff, ff, B, ff, d, gelu ? 0 : 1, nullptr, -1, st));
        if (gelu) RC(pa_gelu_fwd(L->ff, L->ff, B, ff, ff, c.dtype, 0.f, 0, st));
        RC(linear_ln(m, L->ff, PL(pb + D_L2_W), PF(pb + D_L2_B), L->x, L->z, L->x, PF(pb + D_N3_W), PF(pb + D_N3_B), c.eps_layer, B, ff, st));
    }
    return 0;
}

template <typename T>
int decode_step(pa_model* m, void* st) {
    const pa_model_cfg& c = m->cfg;
    DecodeLayout* L = m->dec;
    const DecodePlan& pl = L->plan;
    const int d = c.d_model, B = L->B;
    hipStream_t s = (hipStream_t)st;
    auto PF = [&](int i) { return (const float*)m->pf[i]; };
    auto PL = [&](int i) { return (const void*)m->pl[i]; };
    // the step's input embedding from the token of step t - 1 (all zeros at t = 0, reference models.py:114-123 with no token yet)
    const int g1 = (B * (d / 4) + 255) / 256;
    if (pl.f32res)
        PA_LAUNCH(dec_embed_kernel<float>, dim3(g1), dim3(256), 0, s, (float*)L->x, PF(P_IN_VALUE), PF(P_Q_COORD), PF(P_Q_POS),
                           L->tokens, L->Tmax, L->t_dev, B, d, c.out_dof, (bf16*)L->xb);
    else
        PA_LAUNCH(dec_embed_kernel<T>, dim3(g1), dim3(256), 0, s, (T*)L->x, PF(P_IN_VALUE), PF(P_Q_COORD), PF(P_Q_POS),
                           L->tokens, L->Tmax, L->t_dev, B, d, c.out_dof, (bf16*)nullptr);
    if (pl.f32res) {
        if constexpr (sizeof(T) == 2) RC((folded_layers<T, StreamF32>(m, StreamF32{m, st}, st)));
        else return PA_EINVAL;
    } else if (pl.fold) {
        RC((folded_layers<T, StreamSame<T>>(m, StreamSame<T>{m, st}, st)));
    } else {
        RC(plain_layers<T>(m, st));
    }
    // the tail: decoder.norm, the vocabulary and pointer heads, the mode's choice of a token
    const int tl = m->tail(), ldv = (c.vocab + 7) / 8 * 8;
    if (pl.f32res) {
        RC(pa_layernorm_fwd(L->hf, L->x, PF(m->dec_norm()), PF(m->dec_norm() + 1), L->mean, L->rstd, B, d, c.eps_final, PA_F32, st));
        {   // vocabulary head in f32 on the f32 hidden rows (f32 master weight; the f32 skinny kernel)
            pa_gemm_args g; memset(&g, 0, sizeof(g));
            g.A = L->hf; g.B = PF(tl + T_VOCAB_W); g.C = L->vlog; g.bias = PF(tl + T_VOCAB_B);
            g.M = B; g.N = c.vocab; g.K = d; g.lda = d; g.ldb = d; g.ldc = ldv;
            g.batch = 1; g.a_kcontig = 1; g.b_kcontig = 1; g.in_dtype = PA_F32; g.out_dtype = PA_F32;
            g.alpha = 1.f; g.aux_scale = 1.f; g.splitk = 1;
            RC(pa_gemm(&g, st));
        }
        PA_LAUNCH(dec_cast_kernel, dim3((B * d / 4 + 255) / 256), dim3(256), 0, s, (bf16*)L->h, (const float*)L->hf, (int64_t)B * d / 4);
    } else {
        RC(pa_layernorm_fwd(L->h, L->x, PF(m->dec_norm()), PF(m->dec_norm() + 1), L->mean, L->rstd, B, d, c.eps_final, c.dtype, st));
        RC(linear(m, L->h, PL(tl + T_VOCAB_W), PF(tl + T_VOCAB_B), L->vlog, ldv, B, c.vocab, d, 0, nullptr, PA_F32, st));
    }
    RC(linear(m, L->h, PL(tl + T_PTR_W), PF(tl + T_PTR_B), L->pfeat, d, B, d, d, 0, nullptr, -1, st));
    return end_of_step<T>(m, ldv, s);
}

}  // namespace

void pa_decode_free_layout(pa_model* m) {
    if (m && m->dec) { delete m->dec; m->dec = nullptr; }
}

extern "C" int64_t pa_decode_group_ws_bytes(pa_model* m, int32_t B, int32_t G, int32_t S, int32_t Tmax) {
    if (!m) return PA_EINVAL;
    const DecodePlan pl = plan_decode(m->cfg, B, G, S, Tmax, decode_switches());
    return pl.status ? pl.status : pl.ws_bytes;
}
extern "C" int64_t pa_decode_ws_bytes(pa_model* m, int32_t B, int32_t S, int32_t Tmax) { return pa_decode_group_ws_bytes(m, B, 1, S, Tmax); }

static_assert(sizeof(pa_decode_plan_info) == 72, "pa_decode_plan_info is 72 bytes (plankassembly_amd/_lib.py mirrors it)");
// The dry run of pa_decode_begin / pa_decode_ws_bytes / pa_decode_beam_ws_bytes (include/plank_hip.h): no handle, no device, no launch.
static_assert(sizeof(pa_decode_group_info) == 24, "pa_decode_group_info is 24 bytes (plankassembly_amd/_lib.py mirrors it)");
extern "C" int pa_decode_group_plan(const pa_model_cfg* cfg, int32_t B, int32_t G, int32_t S, int32_t Tmax, pa_decode_plan_info* out,
                                    pa_decode_group_info* g) {
    if (!cfg || !out || !g) return PA_EINVAL;
    *out = pa_decode_plan_info();
    *g = pa_decode_group_info();
    const DecodePlan pl = plan_decode(*cfg, B, G, S, Tmax, decode_switches());
    if (!pl.status) { *out = pl; *g = pl.group; }
    return pl.status;
}
extern "C" int pa_decode_plan(const pa_model_cfg* cfg, int32_t B, int32_t S, int32_t Tmax, pa_decode_plan_info* out) {
    pa_decode_group_info g;
    return pa_decode_group_plan(cfg, B, 1, S, Tmax, out, &g);
}

// Requires a preceding encoder-only pa_model_train_fwd (batch.output_value == NULL) on the same stream:
// uses its memory, batch size, sequence length and input_mask.
// Decode group: the encoder ran on m->B DRAWINGS; the decode is laid out for m->B * G rows (row r belongs to drawing r / G) over one
// copy of the memory, mask and offsets - or one set of cross-attention K / V caches - per drawing.  G 1 is the plain decode.
extern "C" int pa_decode_group_begin(pa_model* m, int32_t G, void* ws, int64_t ws_bytes, int32_t Tmax, void* stream) {
    if (!m || !m->bound || !ws || m->B <= 0 || Tmax <= 0 || Tmax > MAX_T || G < 1 || G > PA_SAMPLE_MAX) return PA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(ws) & 255) != 0) return PA_EALIGN;
    const pa_model_cfg& c = m->cfg;
    const DecodePlan pl = plan_decode(c, m->B, G, m->S, Tmax, decode_switches());
    if (pl.status) return pl.status;
    if (pl.ws_bytes > ws_bytes) return PA_EINVAL;          // (the documented size; the layout itself ends 256 bytes before it)
    if (!m->dec) m->dec = new (std::nothrow) DecodeLayout();
    if (!m->dec) return PA_EINVAL;
    DecodeLayout* L = m->dec;
    L->plan = pl;
    dec_layout(c, pl, L, (char*)ws, m->B, m->B * G, m->S, Tmax);
    const int d = c.d_model, Bd = m->B, B = Bd * G, S = m->S;            // B: rows
    const size_t e = c.dtype == PA_BF16 ? 2 : 4;
    const void* memory = c.has_enc_norm ? m->memory : m->X[c.n_enc];
    hipStream_t s = (hipStream_t)stream;
    L->beamK = 0; L->sampleN = 0;                               // greedy until pa_decode_beam_begin / pa_decode_sample_begin
    L->px_on = false;                                           // and no forced prefix until pa_decode_prefix_begin
    L->cs_on = false;                                           // and no constraint until pa_decode_constraint_set
    if (pl.mq) {
        // absorbed cross-attention: the step reads the encoder output rows themselves - no K / V projection of the memory at all
        HIP_RC(hipMemcpyAsync(L->mem, memory, (size_t)m->NE * d * e, hipMemcpyDeviceToDevice, s));
    }
    for (int i = 0; i < c.n_dec && !pl.mq; ++i) {       // cross-attention K/V of the memory: once per sequence, not per step
        const int pb = m->dec_base(i);
        RC(linear(m, memory, (const char*)m->pl[pb + D_CA_IN_W] + (size_t)d * d * e, (const float*)m->pf[pb + D_CA_IN_B] + d,
                  L->kv_tmp, 2 * d, m->NE, 2 * d, d, 0, nullptr, -1, stream));
        if (c.dtype == PA_BF16)
            PA_LAUNCH(dec_split_heads_kernel<bf16>, dim3(2048), dim3(256), 0, s, (bf16*)L->cross_k[i], (bf16*)L->cross_v[i],
                      (const bf16*)L->kv_tmp, (int64_t)m->NE, S, d, c.n_head, m->batch.cu_in, m->batch.rowmap);
        else
            PA_LAUNCH(dec_split_heads_kernel<float>, dim3(2048), dim3(256), 0, s, (float*)L->cross_k[i], (float*)L->cross_v[i],
                      (const float*)L->kv_tmp, (int64_t)m->NE, S, d, c.n_head, m->batch.cu_in, m->batch.rowmap);
    }
    const bool fold32 = pl.fold && c.dtype == PA_F32;
    if (pl.fold) {
        for (int i = 0; i < c.n_dec; ++i) {
            const int pb = m->dec_base(i);
            auto F = [&](int idx) { return (const float*)m->pf[idx]; };
            auto foldw = [&](void* wf, float* u, float* v, const float* W, const float* bias, const float* g_, const float* b_, int N) -> int {
                return fold32 ? pa_ln_fold_weights_f32((float*)wf, u, v, W, bias, g_, b_, N, d, stream)
                              : pa_ln_fold_weights(wf, u, v, W, bias, g_, b_, N, d, stream);
            };
            if (i > 0) {
                const int pp = m->dec_base(i - 1);
                RC(foldw(L->fw[0][i], L->fu[0][i], L->fv[0][i], F(pb + D_SA_IN_W), F(pb + D_SA_IN_B), F(pp + D_N3_W), F(pp + D_N3_B), 3 * d));
            }
            RC(foldw(L->fw[1][i], L->fu[1][i], L->fv[1][i], F(pb + D_CA_IN_W), F(pb + D_CA_IN_B), F(pb + D_N1_W), F(pb + D_N1_B), d));
            if (pl.mq && pl.mq_contract) {     // the head-transposed copy of W_v for mq_contract_v_kernel (in the wo_t buffer, unused in this form)
                if (c.dtype == PA_BF16)
                    PA_LAUNCH(mq_transpose_v_kernel<bf16>, dim3(1024), dim3(256), 0, s, (bf16*)L->wo_t[i], (const bf16*)m->pl[pb + D_CA_IN_W] + (size_t)2 * d * d, d, c.n_head);
                else
                    PA_LAUNCH(mq_transpose_v_kernel<float>, dim3(1024), dim3(256), 0, s, (float*)L->wo_t[i], (const float*)m->pl[pb + D_CA_IN_W] + (size_t)2 * d * d, d, c.n_head);
            }
            if (pl.mq_self)
                PA_LAUNCH(mq_transpose_v_kernel<float>, dim3(1024), dim3(256), 0, s, (float*)L->wvt_self[i], (const float*)m->pl[pb + D_SA_IN_W] + (size_t)2 * d * d, d, c.n_head);
            if (pl.mq_self_bf)
                PA_LAUNCH(mq_absorb_o_kernel<bf16>, dim3(d), dim3(256), 0, s, (bf16*)L->wo_ts[i], L->bo_ts[i], F(pb + D_SA_OUT_W), F(pb + D_SA_OUT_B),
                          F(pb + D_SA_IN_W), F(pb + D_SA_IN_B), d, c.n_head);
            if (pl.mq && !pl.mq_contract) {    // W~o = W_o,h W_v,h, b~o = b_o + W_o b_v for the Linear behind the absorbed attention (csrc/decode_mq.h)
                if (c.dtype == PA_BF16)
                    PA_LAUNCH(mq_absorb_o_kernel<bf16>, dim3(d), dim3(256), 0, s, (bf16*)L->wo_t[i], L->bo_t[i], F(pb + D_CA_OUT_W), F(pb + D_CA_OUT_B),
                              F(pb + D_CA_IN_W), F(pb + D_CA_IN_B), d, c.n_head);
                else
                    PA_LAUNCH(mq_absorb_o_kernel<float>, dim3(d), dim3(256), 0, s, (float*)L->wo_t[i], L->bo_t[i], F(pb + D_CA_OUT_W), F(pb + D_CA_OUT_B),
                              F(pb + D_CA_IN_W), F(pb + D_CA_IN_B), d, c.n_head);
            }
            RC(foldw(L->fw[2][i], L->fu[2][i], L->fv[2][i], F(pb + D_L1_W), F(pb + D_L1_B), F(pb + D_N2_W), F(pb + D_N2_B), c.d_ff));
        }
    }
    L->cu = nullptr;
    if (m->batch.cu_in) {
        HIP_RC(hipMemcpyAsync(L->cu_store, m->batch.cu_in, (size_t)(Bd + 1) * 4, hipMemcpyDeviceToDevice, s));
        L->cu = L->cu_store;
    }
    HIP_RC(hipMemcpyAsync(L->kpm, m->batch.input_mask, (size_t)Bd * S, hipMemcpyDeviceToDevice, s));
    HIP_RC(hipMemsetAsync(L->first_end, 0xFF, (size_t)B * 4, s));
    HIP_RC(hipMemsetAsync(L->t_dev, 0, 8, s));                  // step counter (and the word beside it, once the removed fused tail's ticket)
    if (L->mq_sp)                                               // the range blocks' tickets (every launch leaves them zero again)
        HIP_RC(hipMemsetAsync(L->mq_sp, 0, ((size_t)B * 4 + 255) / 256 * 256, s));
    HIP_RC(hipMemsetAsync(L->x, 0, (size_t)B * c.d_model * 4, s));
    HIP_RC(hipMemsetAsync(L->xb, 0, (size_t)B * c.d_model * 2, s));
    HIP_RC(hipMemsetAsync(L->tokens, 0, (size_t)B * Tmax * 8, s));
    HIP_RC(hipMemsetAsync(L->attach, 0xFF, (size_t)B * Tmax * 8, s));
    return 0;
}

extern "C" int pa_decode_begin(pa_model* m, void* ws, int64_t ws_bytes, int32_t Tmax, void* stream) {
    return pa_decode_group_begin(m, 1, ws, ws_bytes, Tmax, stream);
}

extern "C" int pa_decode_step(pa_model* m, void* stream) {
    if (!m || !m->dec || m->dec->B <= 0) return PA_EINVAL;
    return m->cfg.dtype == PA_BF16 ? decode_step<bf16>(m, stream) : decode_step<float>(m, stream);
}

// range blocks of a stand-alone absorbed launch: what the step would take for (B, S)
static int standalone_parts(int B, int S) { return mq_parts(B, S, decode_switches().mq_parts, decode_switches().mq_mint); }

// The absorbed cross-attention launch on its own (csrc/decode_mq.h; kernel tests / tools): ctx [B][H][512] (bf16) = per head the
// softmax(qt_h . m_s)-weighted sum of the memory rows m_s; qt [B][H][512] carries scale * log2 e; mem [rows][512] bf16 - dense
// [B][S] rows with the optional key-padding mask kpm [B][S] (1 = PAD), or packed rows with cu [B + 1].
extern "C" int pa_dec_cross_mq(void* ctx, const void* qt, const void* mem, const uint8_t* kpm, const int32_t* cu, int32_t B,
                               int32_t S, int32_t H, int32_t d, void* stream) {
    if (!ctx || !qt || !mem) return PA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(qt) | reinterpret_cast<uintptr_t>(mem)) & 15) return PA_EALIGN;
    return launch_cross_mq((bf16*)ctx, (const bf16*)qt, (const bf16*)mem, kpm, cu, B, S, H, d, (hipStream_t)stream, 1, decode_switches().mq_nt,
                           decode_switches().mq_swap);
}

// The same launch with scratch for range blocks (decode_mq.h: at small batches a batch element's keys are walked by several blocks so
// that the launch uses the whole chip).  ws: pa_dec_cross_mq_ws_bytes(B, S) bytes, 256-byte aligned, its first ceil(4 B / 256) * 256
// bytes zero before the first launch (launches leave them zero); with ws = NULL or too small it is pa_dec_cross_mq.
extern "C" int64_t pa_dec_cross_mq_ws_bytes(int32_t B, int32_t S) { return (B > 0 && S > 0) ? mq_split_bytes(B, standalone_parts(B, S)) : 0; }
extern "C" int pa_dec_cross_mq_ws(void* ctx, const void* qt, const void* mem, const uint8_t* kpm, const int32_t* cu, int32_t B,
                                  int32_t S, int32_t H, int32_t d, void* ws, int64_t ws_bytes, void* stream) {
    if (!ctx || !qt || !mem) return PA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(qt) | reinterpret_cast<uintptr_t>(mem)) & 15) return PA_EALIGN;
    return launch_cross_mq((bf16*)ctx, (const bf16*)qt, (const bf16*)mem, kpm, cu, B, S, H, d, (hipStream_t)stream, standalone_parts(B, S),
                           decode_switches().mq_nt, decode_switches().mq_swap, ws, ws_bytes);
}

extern "C" int pa_dec_cross_mq32(float* ctx, const float* qt, const float* mem, const uint8_t* kpm, const int32_t* cu, int32_t B,
                                 int32_t S, int32_t H, int32_t d, void* stream) {
    if (!ctx || !qt || !mem) return PA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(qt) | reinterpret_cast<uintptr_t>(mem) | reinterpret_cast<uintptr_t>(ctx)) & 15) return PA_EALIGN;
    return launch_cross_mq32(ctx, qt, mem, kpm, cu, B, S, H, d, (hipStream_t)stream, 1, decode_switches().mq32_w8);
}

extern "C" int pa_dec_cross_mq32_ws(float* ctx, const float* qt, const float* mem, const uint8_t* kpm, const int32_t* cu, int32_t B,
                                    int32_t S, int32_t H, int32_t d, void* ws, int64_t ws_bytes, void* stream) {
    if (!ctx || !qt || !mem) return PA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(qt) | reinterpret_cast<uintptr_t>(mem) | reinterpret_cast<uintptr_t>(ctx)) & 15) return PA_EALIGN;
    return launch_cross_mq32(ctx, qt, mem, kpm, cu, B, S, H, d, (hipStream_t)stream, standalone_parts(B, S), decode_switches().mq32_w8, nullptr, ws,
                             ws_bytes);
}

// The launches of a decode group on their own (include/plank_hip.h; tests / tools/group_time.py): B drawings' memory rows (mem, kpm, cu
// as above), qt / ctx [B * G][H][512] - row r attends over drawing r / G; rows_per_block 1 or 2 rows of a drawing per block
// (PA_EINVAL for 2 with an odd G or 2 H > 16); nparts 0 = range blocks by the rule for the launch's units, n > 0 = n per unit (1 where
// ws - 256-byte aligned, its ticket words zero - cannot hold them: ceil(4 units / 256) * 256 + units * nparts * 40 KB).
template <typename T>
static int dec_cross_group(T* ctx, const T* qt, const T* mem, const uint8_t* kpm, const int32_t* cu, int B, int G, int S, int H, int d,
                           int rpb, int nparts, void* ws, int64_t ws_bytes, void* stream) {
    if (!ctx || !qt || !mem || B <= 0 || G < 1 || G > PA_SAMPLE_MAX || B > INT32_MAX / G || nparts < 0 || H < 1) return PA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(qt) | reinterpret_cast<uintptr_t>(mem) | reinterpret_cast<uintptr_t>(ctx)) & 15) return PA_EALIGN;
    MqUnits un;
    if (int rc = mq_units(B * G, H, G, rpb, &un)) return rc;
    const int parts = nparts > 0 ? std::min(nparts, 64) : standalone_parts(un.units, S);
    const DecodeSwitches& sw = decode_switches();
    if constexpr (sizeof(T) == 2)
        return launch_cross_mq(ctx, qt, mem, kpm, cu, B * G, S, H, d, (hipStream_t)stream, parts, sw.mq_nt, sw.mq_swap, ws, ws_bytes, nullptr, G, rpb);
    else
        return launch_cross_mq32(ctx, qt, mem, kpm, cu, B * G, S, H, d, (hipStream_t)stream, parts, sw.mq32_w8, nullptr, ws, ws_bytes, G, rpb);
}
extern "C" int pa_dec_cross_mq_group(void* ctx, const void* qt, const void* mem, const uint8_t* kpm, const int32_t* cu, int32_t B, int32_t G,
                                     int32_t S, int32_t H, int32_t d, int32_t rows_per_block, int32_t nparts, void* ws, int64_t ws_bytes,
                                     void* stream) {
    return dec_cross_group<bf16>((bf16*)ctx, (const bf16*)qt, (const bf16*)mem, kpm, cu, B, G, S, H, d, rows_per_block, nparts, ws, ws_bytes, stream);
}
extern "C" int pa_dec_cross_mq32_group(float* ctx, const float* qt, const float* mem, const uint8_t* kpm, const int32_t* cu, int32_t B,
                                       int32_t G, int32_t S, int32_t H, int32_t d, int32_t rows_per_block, int32_t nparts, void* ws,
                                       int64_t ws_bytes, void* stream) {
    return dec_cross_group<float>(ctx, qt, mem, kpm, cu, B, G, S, H, d, rows_per_block, nparts, ws, ws_bytes, stream);
}

extern "C" int pa_dec_self_mq32(float* ctx, const float* qt, const float* xcache, const int32_t* t_dev, int32_t B, int32_t Tmax,
                                int32_t H, int32_t d, void* stream) {
    if (!ctx || !qt || !xcache || !t_dev) return PA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(qt) | reinterpret_cast<uintptr_t>(xcache) | reinterpret_cast<uintptr_t>(ctx)) & 15) return PA_EALIGN;
    return launch_cross_mq32(ctx, qt, xcache, nullptr, nullptr, B, Tmax, H, d, (hipStream_t)stream, 1, decode_switches().mq32_w8, t_dev);
}

// The self-attention form in both types, with range blocks (include/plank_hip.h): what the step launches on its row cache - the bf16
// form from PLANK_DECODE_MQ_SELF_MINB rows on - reachable on its own (tests/test_dec_mq_float64_gpu.py).
extern "C" int pa_dec_self_mq_ws(void* ctx, const void* qt, const void* xcache, const int32_t* t_dev, int32_t B, int32_t Tmax, int32_t H,
                                 int32_t d, int32_t dtype, int32_t nparts, void* ws, int64_t ws_bytes, void* stream) {
    if (!ctx || !qt || !xcache || !t_dev || nparts < 0 || (dtype != PA_BF16 && dtype != PA_F32)) return PA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(qt) | reinterpret_cast<uintptr_t>(xcache) | reinterpret_cast<uintptr_t>(ctx)) & 15) return PA_EALIGN;
    const DecodeSwitches& sw = decode_switches();
    const int parts = nparts > 0 ? std::min(nparts, 64) : 1;
    if (dtype == PA_BF16)
        return launch_cross_mq((bf16*)ctx, (const bf16*)qt, (const bf16*)xcache, nullptr, nullptr, B, Tmax, H, d, (hipStream_t)stream, parts, sw.mq_nt,
                               sw.mq_swap, ws, ws_bytes, t_dev);
    return launch_cross_mq32((float*)ctx, (const float*)qt, (const float*)xcache, nullptr, nullptr, B, Tmax, H, d, (hipStream_t)stream, parts, sw.mq32_w8,
                             t_dev, ws, ws_bytes);
}

// ---- the step's own kernels on their own (include/plank_hip.h; tests/test_dec_step_float64_gpu.py) -------------
static bool off16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

extern "C" int pa_dec_attn(void* out, const void* q, int32_t ldq, void* kc, void* vc, int32_t Lmax, const uint8_t* kpm, int32_t fixed_lk,
                           const int32_t* t_dev, int32_t B, int32_t H, int32_t d, int32_t dtype, const int32_t* cu, const void* newkv, int32_t G,
                           void* stream) {
    if (!out || !q || !kc || !vc || (dtype != PA_BF16 && dtype != PA_F32)) return PA_EINVAL;
    if (!cu && fixed_lk <= 0 && !t_dev) return PA_EINVAL;           // (the key count has to come from somewhere)
    if (B <= 0 || H <= 0 || d <= 0 || d % H || Lmax <= 0 || fixed_lk > Lmax || G < 1 || B % G) return PA_EINVAL;
    if (newkv && (cu || kpm || G > 1)) return PA_EINVAL;            // (the self form: per-row caches, no mask, no packing)
    const int dh = d / H, vecw = dtype == PA_BF16 ? 8 : 4;
    if (dh != 16 && dh != 32 && dh != 64) return PA_ESHAPE;
    if (off16(out) || off16(q) || off16(kc) || off16(vc) || off16(newkv) || ldq < d || ldq % vecw) return PA_EALIGN;
    if (dtype == PA_BF16)
        return launch_attn<bf16>(d, H, (bf16*)out, (const bf16*)q, ldq, (bf16*)kc, (bf16*)vc, Lmax, kpm, fixed_lk, t_dev, B, stream, cu, (const bf16*)newkv, G);
    return launch_attn<float>(d, H, (float*)out, (const float*)q, ldq, (float*)kc, (float*)vc, Lmax, kpm, fixed_lk, t_dev, B, stream, cu, (const float*)newkv, G);
}

extern "C" int pa_dec_split_heads(void* kc, void* vc, const void* kv, int64_t rows, int32_t S, int32_t d, int32_t H, int32_t dtype,
                                  const int32_t* cu, const int32_t* rowmap, void* stream) {
    if (!kc || !vc || !kv || (dtype != PA_BF16 && dtype != PA_F32) || (cu == nullptr) != (rowmap == nullptr)) return PA_EINVAL;
    if (rows < 0 || S <= 0 || H <= 0 || d <= 0 || d % H) return PA_EINVAL;
    if ((d / H) % 4) return PA_ESHAPE;                              // (a 4-element vector stays inside one head)
    if (off16(kc) || off16(vc) || off16(kv)) return PA_EALIGN;
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PA_BF16)
        PA_LAUNCH(dec_split_heads_kernel<bf16>, dim3(2048), dim3(256), 0, s, (bf16*)kc, (bf16*)vc, (const bf16*)kv, rows, S, d, H, cu, rowmap);
    else
        PA_LAUNCH(dec_split_heads_kernel<float>, dim3(2048), dim3(256), 0, s, (float*)kc, (float*)vc, (const float*)kv, rows, S, d, H, cu, rowmap);
    return 0;
}

extern "C" int pa_dec_embed(void* x, void* x_lp, const float* value, const float* coord, const float* pos, const int64_t* tokens, int32_t Tmax,
                            const int32_t* t_dev, int32_t B, int32_t d, int32_t dof, int32_t dtype, void* stream) {
    if (!x || !value || !coord || !pos || !tokens || !t_dev || (dtype != PA_BF16 && dtype != PA_F32)) return PA_EINVAL;
    if (B <= 0 || d <= 0 || dof <= 0 || Tmax <= 0) return PA_EINVAL;
    if (d % 4) return PA_ESHAPE;
    if (off16(x) || off16(x_lp) || off16(value) || off16(coord) || off16(pos)) return PA_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int g1 = (B * (d / 4) + 255) / 256;
    if (dtype == PA_BF16)
        PA_LAUNCH(dec_embed_kernel<bf16>, dim3(g1), dim3(256), 0, s, (bf16*)x, value, coord, pos, tokens, Tmax, t_dev, B, d, dof, (bf16*)x_lp);
    else
        PA_LAUNCH(dec_embed_kernel<float>, dim3(g1), dim3(256), 0, s, (float*)x, value, coord, pos, tokens, Tmax, t_dev, B, d, dof, (bf16*)x_lp);
    return 0;
}

extern "C" int pa_dec_row_dist(float* p_out, float* stats, const float* vlog, int32_t ldv, const void* pfeat, const void* h, void* hid_cache,
                               const float* sw_w, const float* sw_b, const int32_t* t_dev, int32_t rows, int32_t Tmax, int32_t d, int32_t V,
                               int32_t dtype, void* stream) {
    if (!p_out || !stats || !vlog || !pfeat || !h || !hid_cache || !sw_w || !sw_b || !t_dev || (dtype != PA_BF16 && dtype != PA_F32)) return PA_EINVAL;
    if (rows <= 0 || Tmax <= 0 || Tmax > MAX_T || d <= 0 || V <= 0 || ldv < V) return PA_EINVAL;
    if (d % 8) return PA_ESHAPE;
    if (off16(pfeat) || off16(h) || off16(hid_cache) || off16(sw_w)) return PA_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PA_BF16)
        PA_LAUNCH(dec_row_dist_kernel<bf16>, dim3(rows), dim3(256), 0, s, p_out, stats, vlog, ldv, (const bf16*)pfeat, (const bf16*)h, (bf16*)hid_cache,
                  sw_w, sw_b, t_dev, Tmax, d, V);
    else
        PA_LAUNCH(dec_row_dist_kernel<float>, dim3(rows), dim3(256), 0, s, p_out, stats, vlog, ldv, (const float*)pfeat, (const float*)h,
                  (float*)hid_cache, sw_w, sw_b, t_dev, Tmax, d, V);
    return 0;
}

extern "C" int pa_decode_buffers(pa_model* m, void** tokens, void** attach, void** first_end, void** t_dev) {
    if (!m || !m->dec || !tokens || !attach || !first_end || !t_dev) return PA_EINVAL;
    *tokens = m->dec->tokens; *attach = m->dec->attach; *first_end = m->dec->first_end; *t_dev = m->dec->t_dev;
    return 0;
}

// Beam search over a begun decode (include/plank_hip.h).
extern "C" int64_t pa_decode_beam_ws_bytes(pa_model* m, int32_t rows, int32_t S, int32_t Tmax, int32_t K) {
    if (!m || K < 1 || K > PA_BEAM_MAX || rows <= 0 || rows % K != 0) return PA_EINVAL;
    const DecodePlan pl = plan_decode(m->cfg, rows, 1, S, Tmax, decode_switches());   // (scr_row depends on the rows, not on their grouping)
    if (pl.status || pl.scr_row < 0) return pl.status ? pl.status : pl.scr_row;
    return (int64_t)beam_layout(nullptr, nullptr, rows, K, pl.scr_row) + 256;
}

extern "C" int pa_decode_beam_begin(pa_model* m, int32_t K, void* ws, int64_t ws_bytes, void* stream) {
    if (!m || !m->dec || m->dec->B <= 0 || !ws || K < 1 || K > PA_BEAM_MAX || m->dec->B % K != 0) return PA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(ws) & 255) != 0) return PA_EALIGN;
    DecodeLayout* L = m->dec;
    const int rows = L->B;
    const int64_t scr = beam_segments(m->cfg, L->plan, L, rows, L->Tmax, &L->bm_copy);
    if (scr < 0) return (int)scr;
    if ((int64_t)beam_layout(nullptr, nullptr, rows, K, scr) > ws_bytes) { L->beamK = 0; return PA_EINVAL; }
    beam_layout(L, (char*)ws, rows, K, scr);
    PA_LAUNCH(dec_beam_init_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, L->bm_score, L->bm_fin, L->bm_parent, rows, K);
    L->beamK = K; L->sampleN = 0;                               // (beam mode replaces sampling mode)
    return 0;
}

extern "C" int pa_decode_beam_buffers(pa_model* m, void** scores, void** parents, void** finished) {
    if (!m || !m->dec || m->dec->beamK <= 0 || !scores || !parents || !finished) return PA_EINVAL;
    *scores = m->dec->bm_score; *parents = m->dec->bm_parent; *finished = m->dec->bm_fin;
    return 0;
}

// Sampling over a begun decode (include/plank_hip.h).
namespace {
// the parameter checks shared by pa_decode_sample_begin and pa_decode_sample_set
bool sample_params_ok(const pa_sample_params* p, int rows) {
    return p && p->n_per_drawing >= 1 && p->n_per_drawing <= PA_SAMPLE_MAX && rows % p->n_per_drawing == 0 &&
           std::isfinite(p->temperature) && p->temperature > 0.f && p->top_k >= 0 && p->top_p > 0.f && p->top_p <= 1.f;
}
// sampling workspace: the parameter block, then scores f32 [rows]
size_t sample_layout(DecodeLayout* L, char* base, int rows) {
    Arena a{base, 0};
    void* prm = a.take(sizeof(SampleParamsDev));
    void* score = a.take((size_t)rows * 4);
    if (base) { L->sm_prm = prm; L->sm_score = (float*)score; }
    return a.off;
}
int sample_write_params(DecodeLayout* L, const pa_sample_params* p, float* zero_scores, void* stream) {
    const SampleParamsDev v{p->seed, p->n_per_drawing, p->temperature, p->top_k, p->top_p};
    const int rows = L->B;
    PA_LAUNCH(dec_sample_init_kernel, dim3(zero_scores ? (rows + 255) / 256 : 1), dim3(256), 0, (hipStream_t)stream,
              (SampleParamsDev*)L->sm_prm, v, zero_scores, rows);
    return 0;
}
}  // namespace

extern "C" int64_t pa_decode_sample_ws_bytes(pa_model* m, int32_t rows) {
    if (!m || rows <= 0) return PA_EINVAL;
    return (int64_t)sample_layout(nullptr, nullptr, rows) + 256;
}

extern "C" int pa_decode_sample_begin(pa_model* m, const pa_sample_params* p, void* ws, int64_t ws_bytes, void* stream) {
    if (!m || !m->dec || m->dec->B <= 0 || !ws || !sample_params_ok(p, m->dec->B)) return PA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(ws) & 255) != 0) return PA_EALIGN;
    if (m->cfg.vocab > SAMPLE_MAX_V) return PA_ESHAPE;
    DecodeLayout* L = m->dec;
    if ((int64_t)sample_layout(nullptr, nullptr, L->B) > ws_bytes) return PA_EINVAL;
    sample_layout(L, (char*)ws, L->B);
    RC(sample_write_params(L, p, L->sm_score, stream));
    L->sampleN = p->n_per_drawing; L->beamK = 0;                // (sampling mode replaces beam mode)
    return 0;
}

extern "C" int pa_decode_sample_set(pa_model* m, const pa_sample_params* p, void* stream) {
    if (!m || !m->dec || m->dec->sampleN <= 0 || !sample_params_ok(p, m->dec->B) || p->n_per_drawing != m->dec->sampleN) return PA_EINVAL;
    return sample_write_params(m->dec, p, nullptr, stream);
}

extern "C" int pa_decode_sample_buffers(pa_model* m, void** scores) {
    if (!m || !m->dec || m->dec->sampleN <= 0 || !scores) return PA_EINVAL;
    *scores = m->dec->sm_score;
    return 0;
}

// Forced prefixes over a begun decode, in any mode (include/plank_hip.h).
namespace {
// prefix workspace: plen int32 [rows], ptok / patt int32 [rows][Tmax], prefix_score f32 [rows], prefix_lp f32 [rows][Tmax]
size_t prefix_layout(DecodeLayout* L, char* base, int rows, int Tmax) {
    Arena a{base, 0};
    const size_t row = (size_t)rows * 4, table = row * Tmax;
    void *len = a.take(row), *tok = a.take(table), *att = a.take(table), *score = a.take(row), *lp = a.take(table);
    if (base) {
        L->px_len = (int32_t*)len; L->px_tok = (int32_t*)tok; L->px_att = (int32_t*)att;
        L->px_score = (float*)score; L->px_lp = (float*)lp;
    }
    return a.off;
}
int prefix_write(DecodeLayout* L, const int32_t* plen, const int64_t* ptok, const int64_t* patt, void* stream) {
    const int64_t n = (int64_t)L->B * L->Tmax;
    PA_LAUNCH(dec_prefix_init_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0, (hipStream_t)stream,
              L->px_len, L->px_tok, L->px_att, L->px_score, L->px_lp, plen, ptok, patt, L->B, L->Tmax);
    return 0;
}
}  // namespace

extern "C" int64_t pa_decode_prefix_ws_bytes(pa_model* m, int32_t rows, int32_t Tmax) {
    if (!m || rows <= 0 || Tmax <= 0 || Tmax > MAX_T) return PA_EINVAL;
    return (int64_t)prefix_layout(nullptr, nullptr, rows, Tmax) + 256;
}

extern "C" int pa_decode_prefix_begin(pa_model* m, const int32_t* plen, const int64_t* ptok, const int64_t* patt, void* ws,
                                      int64_t ws_bytes, void* stream) {
    if (!m || !m->dec || m->dec->B <= 0 || !plen || !ptok || !patt || !ws) return PA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(ws) & 255) != 0) return PA_EALIGN;
    DecodeLayout* L = m->dec;
    if ((int64_t)prefix_layout(nullptr, nullptr, L->B, L->Tmax) > ws_bytes) return PA_EINVAL;
    prefix_layout(L, (char*)ws, L->B, L->Tmax);
    RC(prefix_write(L, plen, ptok, patt, stream));
    L->px_on = true;
    return 0;
}

extern "C" int pa_decode_prefix_set(pa_model* m, const int32_t* plen, const int64_t* ptok, const int64_t* patt, void* stream) {
    if (!m || !m->dec || !m->dec->px_on || !plen || !ptok || !patt) return PA_EINVAL;
    return prefix_write(m->dec, plen, ptok, patt, stream);
}

extern "C" int pa_decode_prefix_buffers(pa_model* m, void** prefix_score, void** prefix_lp) {
    if (!m || !m->dec || !m->dec->px_on || !prefix_score || !prefix_lp) return PA_EINVAL;
    *prefix_score = m->dec->px_score; *prefix_lp = m->dec->px_lp;
    return 0;
}

// Plank grammar over a begun decode, in any mode (include/plank_hip.h).  Host state only: the parameters reach the
// end-of-step kernels as arguments of the next pa_decode_step.
extern "C" int pa_decode_constraint_set(pa_model* m, const pa_constraint_params* p) {
    if (!m || !m->dec || m->dec->B <= 0) return PA_EINVAL;
    DecodeLayout* L = m->dec;
    if (!p) { L->cs_on = false; return 0; }
    if (p->min_planks < 0 || p->max_planks < std::max(p->min_planks, 1) || p->n_val < 2) return PA_EINVAL;
    if (p->n_val > m->cfg.vocab || m->cfg.out_dof != 6) return PA_EINVAL;      // (the window's tokens are vocab entries; planks of six)
    L->cs = *p; L->cs_on = true;
    return 0;
}
