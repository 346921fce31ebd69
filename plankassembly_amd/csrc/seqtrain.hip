// Sequence-level training batches for gfx950: one launch turns the sample decoder's buffers and the match
// counts of its rows into the teacher-forced, weighted batch `PlankModel.train_step` consumes - rows cut at END and padded, pointer
// labels, the ground-truth row, one policy-gradient weight per row and the rewards - with nothing returned to the host.
// What it restates: plankassembly_amd/metric.py `prf_from_counts` (HungarianMatcher's last four lines; reference
// third_party/matcher.py:57-61) for the reward, and the batch contract of plankassembly_amd/data.py / datasets.py
// (`prepare_output_sequence`: label = vocab_size + attach at a pointer, PAD and mask 1 behind the END) that `PlankModel.score`
// reads back.  tests/seq_train_reference.py is the numpy restatement the kernel is pinned to.
//
// Grid (row g, drawing b), one block of 256 threads per output row.  Every block recomputes its drawing's N <= 64 rewards from the
// drawing's count rows (lane n owns sample n) and thread 0 forms the block's own weight from them in a fixed order: no block waits
// for another, no atomics, no tickets.  The row itself is a strided loop over T, one int64 per lane per pass (coalesced 2 KiB
// per pass and array).  Plain loads and stores only; the launch captures into a graph like every other entry point.
#include "pa_device.h"
#include "../../include/plank_hip.h"

#pragma clang fp contract(off)          // this whole file: every product and sum of the weights is rounded on its own, as in numpy

namespace {

#define ST(s) reinterpret_cast<hipStream_t>(s)

constexpr int SQ_THREADS = 256;
constexpr int SQ_MAX_N = PA_SEQ_MAX_SAMPLES;
static_assert(SQ_MAX_N <= SQ_THREADS, "one lane per sample");

// metric.prf_from_counts on one count row: double quotients rounded to f32, then f32 expressions.  An f32 quotient taken in double
// and rounded once more is the correctly rounded f32 quotient (53 >= 2 * 24 + 2), whatever the compiler makes of an f32 division.
__device__ __forceinline__ float sq_f1(const int32_t* c) {
    const int32_t tp = c[0], n_pred = c[1], n_gt = c[2];
    const float prec = n_pred > 0 ? (float)((double)tp / (double)n_pred) : 0.0f;
    const float rec = n_gt > 0 ? (float)((double)tp / (double)n_gt) : 0.0f;
    const float num = (prec * rec) * 2.0f;
    const float den = (prec + rec) + 1e-10f;
    return (float)((double)num / (double)den);
}

__global__ __launch_bounds__(SQ_THREADS) void sequence_batch_kernel(pa_seq_batch_args a) {
    __shared__ float r_s[SQ_MAX_N];
    __shared__ double e_s[SQ_MAX_N];
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int N = a.N, T = a.T;
    const int G = N + (a.nll_weight != 0.0f ? 1 : 0);
    const int64_t out_row = (int64_t)b * G + g;

    // ---- the drawing's rewards (and, under risk, the softmax numerators), lane n = sample n
    if (tid < N) {
        const int64_t row = (int64_t)b * N + tid;
        const float r = sq_f1(a.counts + row * 4);
        r_s[tid] = r;
        if (g == tid) a.reward[row] = r;                                  // block g < N writes reward[b][g]: every element once
        if (a.objective == 1) e_s[tid] = (double)a.alpha * (double)a.scores[row];
    }
    __syncthreads();

    // ---- this row's weight: thread 0, double, the order of the header
    if (tid == 0) {
        float w;
        if (g == N) {
            w = a.nll_weight;
        } else if (a.objective == 0) {
            double base = 0.0;
            if (a.baseline == 1) {
                double s = 0.0;
                for (int m = 0; m < N; ++m)
                    if (m != g) s += (double)r_s[m];
                base = s / (double)(N - 1);
            } else if (a.baseline == 2) {
                base = (double)sq_f1(a.base_counts + (int64_t)b * 4);
            }
            w = (float)(((double)r_s[g] - base) / (double)N);
        } else {
            double mx = e_s[0];
            for (int m = 1; m < N; ++m) mx = e_s[m] > mx ? e_s[m] : mx;
            double z = 0.0, mine = 0.0;
            for (int m = 0; m < N; ++m) {
                const double e = exp(e_s[m] - mx);
                e_s[m] = e;                                               // (thread 0 alone reads and writes e_s from here on)
                z += e;
                if (m == g) mine = e;
            }
            // r_g - sum_m q_m r_m as sum_m q_m (r_g - r_m): no large terms cancel, and equal rewards give an exact +0.0
            double adv = 0.0;
            for (int m = 0; m < N; ++m) adv += (e_s[m] / z) * ((double)r_s[g] - (double)r_s[m]);
            w = (float)(((double)a.alpha * (mine / z)) * adv);
        }
        a.out_weight[out_row] = w;
    }

    // ---- the row
    int64_t* ov = a.out_value + out_row * T;
    int64_t* ol = a.out_label + out_row * T;
    uint8_t* om = a.out_mask + out_row * T;
    const int64_t pad = (int64_t)a.pad_token;
    if (g == N) {                                                         // the ground-truth row, as it is
        const int64_t* gv = a.gt_value + (int64_t)b * a.gt_stride;
        const int64_t* gl = a.gt_label + (int64_t)b * a.gt_stride;
        for (int t = tid; t < T; t += SQ_THREADS) {
            const int64_t v = gv[t];
            ov[t] = v; ol[t] = gl[t]; om[t] = v == pad ? 1 : 0;
        }
        return;
    }
    const int64_t row = (int64_t)b * N + g;
    const int32_t fe = a.first_end[row];
    int L = fe >= 0 ? fe + 1 : a.Tmax;
    L = L < a.Tmax ? L : a.Tmax;                                          // never past the decoder's row, whatever first_end holds
    const int64_t* tk = a.tokens + row * a.sample_stride;
    const int64_t* at = a.attach + row * a.sample_stride;
    for (int t = tid; t < T; t += SQ_THREADS) {
        int64_t v = pad, l = pad;
        if (t < L) {                                                      // t < L <= Tmax: inside the decoder's row
            v = tk[t];
            const int64_t j = at[t];
            l = j >= 0 ? (int64_t)a.vocab_size + j : v;
        }
        ov[t] = v; ol[t] = l; om[t] = t < L ? 0 : 1;
    }
}

}  // namespace

extern "C" int64_t pa_seq_batch_args_bytes(void) { return (int64_t)sizeof(pa_seq_batch_args); }

extern "C" int pa_sequence_batch(const pa_seq_batch_args* a, void* stream) {
    if (!a) return PA_EINVAL;
    if (!a->tokens || !a->attach || !a->first_end || !a->scores || !a->counts || !a->gt_value || !a->gt_label) return PA_EINVAL;
    if (!a->out_value || !a->out_label || !a->out_mask || !a->out_weight || !a->reward) return PA_EINVAL;
    if (a->B < 0 || a->N < 1 || a->N > SQ_MAX_N || a->Tmax < 0 || a->T < 0 || a->Tmax > a->T) return PA_EINVAL;
    if (a->sample_stride < 0 || a->gt_stride < 0) return PA_EINVAL;
    if (a->objective < 0 || a->objective > 1 || a->baseline < 0 || a->baseline > 2) return PA_EINVAL;
    if (!(a->nll_weight - a->nll_weight == 0.0f)) return PA_EINVAL;                           // NaN / inf
    if (a->baseline == 1 && a->N < 2) return PA_EINVAL;
    if (a->baseline == 2 && !a->base_counts) return PA_EINVAL;
    if (a->objective == 1 && !(a->alpha > 0.0f && a->alpha - a->alpha == 0.0f)) return PA_EINVAL;
    if (a->B > 65535) return PA_ESHAPE;                                                       // grid.y
    if (a->B == 0) return 0;
    const int G = a->N + (a->nll_weight != 0.0f ? 1 : 0);
    PA_LAUNCH(sequence_batch_kernel, dim3((unsigned)G, (unsigned)a->B), dim3(SQ_THREADS), 0, ST(stream), *a);
    return 0;
}
