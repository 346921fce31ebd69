// Device-resident dataset for gfx950: one launch turns B prepared drawings (CSR arrays in HBM) into the batch the model
// consumes - quantise, sort, position ids, END / PAD, the plank sequence with its pointer labels and, for training, the
// line noise of the reference's augmentation.  What it restates: plankassembly_amd/datasets.py `_sorted_tokens`,
// `_pad_inputs`, `prepare_output_sequence`, `add_noise` (reference line_data.py:34-142, sideface_data.py:137-213,
// data_utils.py:6-68).  DESIGN.md section 17; tests/device_data_reference.py is the numpy restatement the kernel is
// pinned to bit for bit.
//
// One block of 256 threads (4 waves) per drawing.  Thread t owns the lines t, t + 256, ... (at most TK_MAX_LINES / 256).
// All coordinate arithmetic is float64 with fused multiply-add contraction OFF (numpy rounds every product and sum).
#include "pa_device.h"
#include "../../include/plank_hip.h"

#pragma clang fp contract(off)          // this whole file: a * b + c stays two roundings, as in numpy

namespace {

#define ST(s) reinterpret_cast<hipStream_t>(s)

constexpr int TK_THREADS = 256;
constexpr int TK_MAX_LINES = PA_TOKENISE_MAX_LINES;
constexpr int TK_LINE_BITS = 10;                       // line number: the stable-sort tie break
constexpr int TK_Q_BITS = 11;                          // per quantised coordinate (n_bits <= 11)
constexpr int TK_VIEW_SHIFT = TK_LINE_BITS + 4 * TK_Q_BITS;     // 54: view in bits 54..61
constexpr uint64_t TK_DELETED = ~0ull;                 // a line the noise removed: sorts behind every kept one
static_assert((1 << TK_LINE_BITS) == TK_MAX_LINES, "line field must hold every line number");

struct TkArgs {
    const int32_t* line_off; const double* box; const double* seg; const uint8_t* view; const uint8_t* type;
    const int32_t* plank_off; const double* coords; const int32_t* attach;
    const int32_t* index;
    int32_t N, S, T, n_bits, tok_end, tok_pad, vocab, with_type, augment;
    double aug_ratio, noise_ratio, noise_length;
    uint32_t seed, epoch;
    int64_t* in_value; int64_t* in_pos; int64_t* in_coord; int64_t* in_view; int64_t* in_type; uint8_t* in_mask;
    int64_t* out_value; int64_t* out_label; uint8_t* out_mask;
    int32_t* n_tokens;
};

// ---- the draws (tests/device_data_reference.py draw_hash): a pure function of (seed, epoch, drawing, line, slot)
__device__ __forceinline__ uint32_t tk_base(uint32_t seed, uint32_t epoch, uint32_t drawing) {
    return mix32(drawing ^ mix32(epoch ^ mix32(seed + 0x9e3779b9u)));
}
__device__ __forceinline__ uint32_t tk_draw(uint32_t base, uint32_t line, uint32_t slot) {
    return mix32(slot ^ mix32(line ^ base));
}
__device__ __forceinline__ double tk_unit(uint32_t h) { return (double)(h >> 8) * 0x1p-24; }    // [0, 1), exact
constexpr uint32_t TK_DRAWING = 0xffffffffu;           // the "line number" of the two per-drawing draws
enum { TK_SLOT_SELECT = 0, TK_SLOT_DELETE = 1, TK_SLOT_NOISE = 2, TK_SLOT_END = 3 };
enum { TK_SLOT_AUGMENT = 0, TK_SLOT_COUNT = 1 };

// numpy's ((v - (-1)) * rq / 2).astype(long): each operation rounded on its own, truncation toward zero
__device__ __forceinline__ int64_t tk_quantise(double v, double rq) {
    const double a = v + 1.0;
    const double b = a * rq;
    return (int64_t)(b / 2.0);
}

// datasets.add_noise on one selected two-point segment (x0, y0) -> (x1, y1).  false: the line is deleted.
__device__ __forceinline__ bool tk_noise(double& x0, double& y0, double& x1, double& y1, uint32_t base, uint32_t line,
                                         double noise_length) {
    if (tk_unit(tk_draw(base, line, TK_SLOT_DELETE)) > 0.5) return false;
    const double dx = x1 - x0, dy = y1 - y0;
    const double xx = dx * dx, yy = dy * dy;
    const double length = __builtin_sqrt(xx + yy);                            // np.linalg.norm of the one difference row
    const double scaled = tk_unit(tk_draw(base, line, TK_SLOT_NOISE)) * noise_length;
    const double noise = __builtin_rint(scaled * 1000.0) / 1000.0;            // np.round(x, 3)
    if (length <= noise) return false;
    double d0, d1;                                                            // arc lengths of the two new end points
    if (tk_unit(tk_draw(base, line, TK_SLOT_END)) > 0.5) { d0 = 0.0; d1 = length - noise; }       // shortened at the tail
    else { d0 = noise; d1 = length; }                                                             // shortened at the head
    const double t0 = d0 / length, t1 = d1 / length;                          // datasets._interpolate, two-point segment
    const double ax = t0 * dx, ay = t0 * dy, bx = t1 * dx, by = t1 * dy;
    const double nx0 = x0 + ax, ny0 = y0 + ay, nx1 = x0 + bx, ny1 = y0 + by;
    x0 = nx0; y0 = ny0; x1 = nx1; y1 = ny1;
    return true;
}

// ---- the stages tokenise_kernel and sideface_kernel (sideface.h) share; every one is called by the whole block
// The two per-drawing draws over the drawing's ``n`` lines, and the selection hash of every line.  true: the drawing is augmented.
__device__ __forceinline__ bool tk_draws(const TkArgs& a, int d, int n, uint32_t* selh, uint32_t& base, int& num_select) {
    const int tid = threadIdx.x;
    bool augmented = false;
    num_select = 0;
    base = 0;
    if (a.augment && a.seg && n > 0) {
        base = tk_base(a.seed, a.epoch, (uint32_t)d);
        if (tk_unit(tk_draw(base, TK_DRAWING, TK_SLOT_AUGMENT)) < a.aug_ratio) {
            const double scaled = (double)n * a.noise_ratio;
            const int max_sel = (int)__builtin_ceil(scaled) < n ? (int)__builtin_ceil(scaled) : n;
            if (max_sel >= 1) {
                augmented = true;
                num_select = 1 + (int)(((uint64_t)tk_draw(base, TK_DRAWING, TK_SLOT_COUNT) * (uint64_t)max_sel) >> 32);
            }
        }
    }
    if (augmented) {
        for (int i = tid; i < n; i += TK_THREADS) selh[i] = tk_draw(base, (uint32_t)i, TK_SLOT_SELECT);
        __syncthreads();
    }
    return augmented;
}

// Line i of an augmented drawing: the segment as the noise leaves it.  false: the line is deleted.
__device__ __forceinline__ bool tk_noisy_segment(const TkArgs& a, int lo, int i, int n, const uint32_t* selh, int num_select,
                                                 uint32_t base, double& sx0, double& sy0, double& sx1, double& sy1) {
    const double* s = a.seg + (size_t)(lo + i) * 4;
    sx0 = s[0]; sy0 = s[1]; sx1 = s[2]; sy1 = s[3];
    const uint64_t mine = ((uint64_t)selh[i] << 32) | (uint32_t)i;
    int below = 0;                                                   // the num_select smallest (hash, line) pairs
    for (int j = 0; j < n; ++j) below += (((uint64_t)selh[j] << 32) | (uint32_t)j) < mine;
    if (below < num_select) return tk_noise(sx0, sy0, sx1, sy1, base, (uint32_t)i, a.noise_length);
    return true;
}

// np.lexsort(with_view.T[[3, 1, 2, 0, 4]]): view, column 0, column 2, column 1, column 3; stable -> primitive number i
__device__ __forceinline__ uint64_t tk_key(uint32_t view, double x0, double y0, double x1, double y1, double rq, int i) {
    const uint64_t qmask = (1ull << TK_Q_BITS) - 1;
    const uint64_t q0 = (uint64_t)tk_quantise(x0, rq) & qmask, q1 = (uint64_t)tk_quantise(y0, rq) & qmask;
    const uint64_t q2 = (uint64_t)tk_quantise(x1, rq) & qmask, q3 = (uint64_t)tk_quantise(y1, rq) & qmask;
    return ((uint64_t)view << TK_VIEW_SHIFT) | (q0 << (TK_LINE_BITS + 3 * TK_Q_BITS)) |
           (q2 << (TK_LINE_BITS + 2 * TK_Q_BITS)) | (q1 << (TK_LINE_BITS + TK_Q_BITS)) | (q3 << TK_LINE_BITS) | (uint64_t)i;
}

// Rank by counting: every key is distinct (the primitive number is part of it).  Returns the number of kept primitives.
__device__ __forceinline__ int tk_rank(const uint64_t* key, uint64_t* skey, uint16_t* spos, int n) {
    const int tid = threadIdx.x;
    int nk = 0;
    for (int i0 = 0; i0 < n; i0 += TK_THREADS) {
        const int i = i0 + tid;
        const uint64_t mine = i < n ? key[i] : TK_DELETED;
        const bool kept = mine != TK_DELETED;
        if (kept) {
            const uint64_t view_floor = mine >> TK_VIEW_SHIFT << TK_VIEW_SHIFT;      // the smallest key of the primitive's view
            int below = 0, below_view = 0;
            for (int j = 0; j < n; ++j) {
                const uint64_t k = key[j];
                below += k < mine;
                below_view += k < view_floor;
            }
            skey[below] = mine;
            spos[below] = (uint16_t)(below - below_view);
        }
        nk += __syncthreads_count(kept);
    }
    __syncthreads();
    return nk;
}

// Encoder rows: 4 tokens per kept primitive, END, PAD; consecutive threads store consecutive elements
__device__ __forceinline__ void tk_store_inputs(const TkArgs& a, int b, int lo, const uint64_t* skey, const uint16_t* spos, int nk) {
    const int tid = threadIdx.x;
    const size_t row = (size_t)b * a.S;
    const int n_tok = 4 * nk;
    for (int j = tid; j < a.S; j += TK_THREADS) {
        int64_t value = j == n_tok ? a.tok_end : a.tok_pad, pos = 0, coord = 0, view = 0, type = 0;
        if (j < n_tok) {
            const uint64_t k = skey[j >> 2];
            const int c = j & 3;
            const int field = c == 0 ? 3 : (c == 1 ? 1 : (c == 2 ? 2 : 0));      // key order is column 0, 2, 1, 3
            value = (int64_t)((k >> (TK_LINE_BITS + field * TK_Q_BITS)) & ((1ull << TK_Q_BITS) - 1));
            pos = spos[j >> 2];
            coord = c;
            view = (int64_t)((k >> TK_VIEW_SHIFT) & 0xff);
            if (a.with_type) type = a.type[lo + (int)(k & (TK_MAX_LINES - 1))];
        }
        a.in_value[row + j] = value;
        a.in_pos[row + j] = pos;
        a.in_coord[row + j] = coord;
        a.in_view[row + j] = view;
        if (a.with_type) a.in_type[row + j] = type;
        a.in_mask[row + j] = j > n_tok;
    }
    if (tid == 0) a.n_tokens[b] = n_tok + 1;
}

// Decoder rows: 6 tokens per plank, END, PAD; a pointer label where the plank attaches
__device__ __forceinline__ void tk_store_outputs(const TkArgs& a, int b, int d, bool have, double rq) {
    const int tid = threadIdx.x;
    const int plo = have ? a.plank_off[d] : 0;
    int np = have ? a.plank_off[d + 1] - plo : 0;
    const int max_planks = (a.T - 1) / 6;
    np = np < 0 ? 0 : (np > max_planks ? max_planks : np);
    const size_t orow = (size_t)b * a.T;
    for (int j = tid; j < a.T; j += TK_THREADS) {
        int64_t value = j == 6 * np ? a.tok_end : a.tok_pad, label;
        label = value;
        if (j < 6 * np) {
            value = tk_quantise(a.coords[(size_t)plo * 6 + j], rq);
            const int at = a.attach[(size_t)plo * 6 + j];
            label = at != -1 ? (int64_t)at + a.vocab : value;
        }
        a.out_value[orow + j] = value;
        a.out_label[orow + j] = label;
        a.out_mask[orow + j] = j > 6 * np;
    }
}

__global__ __launch_bounds__(TK_THREADS) void tokenise_kernel(TkArgs a) {
    __shared__ uint64_t key[TK_MAX_LINES];             // sort key per line (line order)
    __shared__ uint64_t skey[TK_MAX_LINES];            // the keys in sorted order
    __shared__ uint32_t selh[TK_MAX_LINES];            // selection hash per line
    __shared__ uint16_t spos[TK_MAX_LINES];            // rank within the view, sorted order

    const int b = blockIdx.x, tid = threadIdx.x;
    const int d = a.index[b];
    const bool have = d >= 0 && d < a.N;
    const int lo = have ? a.line_off[d] : 0;
    int n = have ? a.line_off[d + 1] - lo : 0;
    n = n < 0 ? 0 : (n > TK_MAX_LINES ? TK_MAX_LINES : n);
    const int max_lines = (a.S - 1) >> 2;              // what fits the row (the host rejects longer drawings)
    if (n > max_lines) n = max_lines < 0 ? 0 : max_lines;
    const double rq = (double)((1 << a.n_bits) - 1);

    uint32_t base;
    int num_select;
    const bool augmented = tk_draws(a, d, n, selh, base, num_select);

    // ---- boxes -> keys
    for (int i = tid; i < n; i += TK_THREADS) {
        double x0, y0, x1, y1;
        bool kept = true;
        if (augmented) {
            double sx0, sy0, sx1, sy1;
            kept = tk_noisy_segment(a, lo, i, n, selh, num_select, base, sx0, sy0, sx1, sy1);
            x0 = sx0 < sx1 ? sx0 : sx1; x1 = sx0 < sx1 ? sx1 : sx0;          // the bounds of the segment
            y0 = sy0 < sy1 ? sy0 : sy1; y1 = sy0 < sy1 ? sy1 : sy0;
        } else {
            const double* bx = a.box + (size_t)(lo + i) * 4;
            x0 = bx[0]; y0 = bx[1]; x1 = bx[2]; y1 = bx[3];
        }
        key[i] = kept ? tk_key(a.view[lo + i], x0, y0, x1, y1, rq, i) : TK_DELETED;
    }
    __syncthreads();

    const int nk = tk_rank(key, skey, spos, n);
    tk_store_inputs(a, b, lo, skey, spos, nk);
    tk_store_outputs(a, b, d, have, rq);
}

#include "sideface.h"                                  // sideface_kernel and its launch arguments, on the stages above
#include "render.h"                                    // render_kernel: the drawing from the planks, on the same stages

}  // namespace

extern "C" int pa_tokenise_drawings(const int32_t* line_off, const double* box, const double* seg, const uint8_t* view,
                                    const uint8_t* type, const int32_t* plank_off, const double* coords, const int32_t* attach,
                                    int32_t N, const int32_t* index, int32_t B, int32_t S, int32_t T, int32_t n_bits,
                                    int32_t tok_end, int32_t tok_pad, int32_t vocab, int32_t with_type, int32_t augmentation,
                                    double aug_ratio, double noise_ratio, double noise_length, uint32_t seed, uint32_t epoch,
                                    int64_t* in_value, int64_t* in_pos, int64_t* in_coord, int64_t* in_view, int64_t* in_type,
                                    uint8_t* in_mask, int64_t* out_value, int64_t* out_label, uint8_t* out_mask,
                                    int32_t* n_tokens, void* stream) {
    if (!line_off || !box || !view || !coords || !attach || !plank_off || !index || !in_value || !in_pos || !in_coord || !in_view || !in_mask ||
        !out_value || !out_label || !out_mask || !n_tokens)
        return PA_EINVAL;
    if (N <= 0 || B <= 0 || S <= 0 || T <= 0) return PA_EINVAL;
    if (with_type && (!type || !in_type)) return PA_EINVAL;
    if (augmentation && !seg) return PA_EINVAL;
    if (n_bits < 1 || n_bits > TK_Q_BITS) return PA_ESHAPE;
    if (!(aug_ratio >= 0.0) || !(noise_ratio >= 0.0) || !(noise_length >= 0.0)) return PA_EINVAL;
    TkArgs a;
    a.line_off = line_off; a.box = box; a.seg = seg; a.view = view; a.type = type;
    a.plank_off = plank_off; a.coords = coords; a.attach = attach; a.index = index;
    a.N = N; a.S = S; a.T = T; a.n_bits = n_bits; a.tok_end = tok_end; a.tok_pad = tok_pad; a.vocab = vocab;
    a.with_type = with_type; a.augment = augmentation;
    a.aug_ratio = aug_ratio; a.noise_ratio = noise_ratio; a.noise_length = noise_length; a.seed = seed; a.epoch = epoch;
    a.in_value = in_value; a.in_pos = in_pos; a.in_coord = in_coord; a.in_view = in_view; a.in_type = in_type;
    a.in_mask = in_mask; a.out_value = out_value; a.out_label = out_label; a.out_mask = out_mask; a.n_tokens = n_tokens;
    PA_LAUNCH(tokenise_kernel, dim3(B), dim3(TK_THREADS), 0, ST(stream), a);
    return 0;
}

extern "C" int pa_tokenise_sideface_drawings(const int32_t* line_off, const double* box, const double* seg, const uint8_t* view,
                                             const uint8_t* type, const int32_t* plank_off, const double* coords,
                                             const int32_t* attach, int32_t N, const int32_t* index, int32_t B, int32_t S, int32_t T,
                                             int32_t n_bits, int32_t tok_end, int32_t tok_pad, int32_t vocab, int32_t with_type,
                                             int32_t augmentation, double aug_ratio, double noise_ratio, double noise_length,
                                             uint32_t seed, uint32_t epoch, int64_t* in_value, int64_t* in_pos, int64_t* in_coord,
                                             int64_t* in_view, int64_t* in_type, uint8_t* in_mask, int64_t* out_value,
                                             int64_t* out_label, uint8_t* out_mask, int32_t* n_tokens, double max_thickness,
                                             double min_thickness, double merge_tolerance, double* faces_out,
                                             uint8_t* faceviews_out, int32_t* n_faces_out, int32_t* flags_out, void* stream) {
    (void)box; (void)type; (void)in_type;                                    // side faces carry no stored boxes and no type row
    if (with_type) return PA_EINVAL;
    if (!line_off || !seg || !view || !coords || !attach || !plank_off || !index || !in_value || !in_pos || !in_coord || !in_view ||
        !in_mask || !out_value || !out_label || !out_mask || !n_tokens || !flags_out)
        return PA_EINVAL;
    if (N <= 0 || B <= 0 || S <= 0 || T <= 0) return PA_EINVAL;
    if (n_bits < 1 || n_bits > TK_Q_BITS) return PA_ESHAPE;
    if ((S - 1) / 4 > TK_MAX_LINES) return PA_ESHAPE;                        // the row cannot hold more faces than the sort keys
    if (!(aug_ratio >= 0.0) || !(noise_ratio >= 0.0) || !(noise_length >= 0.0)) return PA_EINVAL;
    if (max_thickness != max_thickness || min_thickness != min_thickness || merge_tolerance != merge_tolerance) return PA_EINVAL;
    SfArgs s;
    TkArgs& a = s.t;
    a.line_off = line_off; a.box = nullptr; a.seg = seg; a.view = view; a.type = nullptr;
    a.plank_off = plank_off; a.coords = coords; a.attach = attach; a.index = index;
    a.N = N; a.S = S; a.T = T; a.n_bits = n_bits; a.tok_end = tok_end; a.tok_pad = tok_pad; a.vocab = vocab;
    a.with_type = 0; a.augment = augmentation;
    a.aug_ratio = aug_ratio; a.noise_ratio = noise_ratio; a.noise_length = noise_length; a.seed = seed; a.epoch = epoch;
    a.in_value = in_value; a.in_pos = in_pos; a.in_coord = in_coord; a.in_view = in_view; a.in_type = nullptr;
    a.in_mask = in_mask; a.out_value = out_value; a.out_label = out_label; a.out_mask = out_mask; a.n_tokens = n_tokens;
    s.max_thickness = max_thickness; s.min_thickness = min_thickness; s.merge_tolerance = merge_tolerance;
    s.faces_out = faces_out; s.faceviews_out = faceviews_out; s.n_faces_out = n_faces_out; s.flags_out = flags_out;
    PA_LAUNCH(sideface_kernel, dim3(B), dim3(TK_THREADS), 0, ST(stream), s);
    return 0;
}

extern "C" int pa_render_drawings(const int32_t* plank_off, const int32_t* plank_cnt, const double* coords, const int32_t* attach,
                                  int32_t N, const int32_t* index, int32_t B, int32_t max_planks, int32_t skip_first, int32_t S,
                                  int32_t T, int32_t n_bits, int32_t tok_end, int32_t tok_pad, int32_t vocab, int32_t with_type,
                                  int32_t augmentation, double aug_ratio, double noise_ratio, double noise_length, uint32_t seed,
                                  uint32_t epoch, int64_t* in_value, int64_t* in_pos, int64_t* in_coord, int64_t* in_view,
                                  int64_t* in_type, uint8_t* in_mask, int64_t* out_value, int64_t* out_label, uint8_t* out_mask,
                                  int32_t* n_tokens, double* lines_out, uint8_t* views_out, uint8_t* types_out,
                                  int32_t* n_lines_out, int32_t* flags_out, void* stream) {
    if (!plank_off || !coords || !index || !in_value || !in_pos || !in_coord || !in_view || !in_mask || !n_tokens || !flags_out)
        return PA_EINVAL;
    if (N <= 0 || B <= 0 || S <= 0 || max_planks < 0) return PA_EINVAL;
    if (with_type && !in_type) return PA_EINVAL;
    const bool outputs = out_value || out_label || out_mask;
    if (outputs && (!out_value || !out_label || !out_mask || !attach || T <= 0)) return PA_EINVAL;
    if (n_bits < 1 || n_bits > TK_Q_BITS) return PA_ESHAPE;
    if ((S - 1) / 4 > TK_MAX_LINES) return PA_ESHAPE;                        // the row cannot hold more lines than the sort keys
    if (max_planks > PA_RENDER_MAX_PLANKS) return PA_ESHAPE;                 // nothing is launched, nothing written
    if (!(aug_ratio >= 0.0) || !(noise_ratio >= 0.0) || !(noise_length >= 0.0)) return PA_EINVAL;
    RdArgs r;
    TkArgs& a = r.t;
    a.line_off = nullptr; a.box = nullptr; a.seg = nullptr; a.view = nullptr; a.type = nullptr;
    a.plank_off = plank_off; a.coords = coords; a.attach = attach; a.index = index;
    a.N = N; a.S = S; a.T = T; a.n_bits = n_bits; a.tok_end = tok_end; a.tok_pad = tok_pad; a.vocab = vocab;
    a.with_type = with_type; a.augment = augmentation;
    a.aug_ratio = aug_ratio; a.noise_ratio = noise_ratio; a.noise_length = noise_length; a.seed = seed; a.epoch = epoch;
    a.in_value = in_value; a.in_pos = in_pos; a.in_coord = in_coord; a.in_view = in_view; a.in_type = in_type;
    a.in_mask = in_mask; a.out_value = outputs ? out_value : nullptr; a.out_label = out_label; a.out_mask = out_mask; a.n_tokens = n_tokens;
    r.plank_cnt = plank_cnt; r.skip_first = skip_first;
    r.lines_out = lines_out; r.views_out = views_out; r.types_out = types_out; r.n_lines_out = n_lines_out; r.flags_out = flags_out;
    PA_LAUNCH(render_kernel, dim3(B), dim3(TK_THREADS), 0, ST(stream), r);
    return 0;
}
