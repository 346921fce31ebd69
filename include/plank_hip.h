/*
 * plank_hip.h -- C ABI of libplank_hip.so, the MI355X (gfx950) implementation of the
 * PlankAssembly encoder-decoder hot path.
 *
 * The reference has no FFI: its hot path (reference plankassembly/models.py) is Python glue
 * over torch.nn modules.  The drop-in boundary towards the reference's callers is therefore
 * the Python surface in plankassembly_amd/models.py (build_model / forward / state_dict,
 * SURVEY.md section 8b); THIS header is the boundary between that host code and the device
 * code.  Each entry point names the reference lines (and the torch op behind them) it
 * replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every pointer is a device pointer owned by the caller (PyTorch's caching allocator);
 *     the library never allocates, frees or synchronises; scratch is passed in explicitly;
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work on it (capturable
 *     in a hipGraph);
 *   - return value: 0 on success, a hipError_t (>0) from the launch, or a negative
 *     PA_E* code for a bad argument.  No exceptions cross the ABI;
 *   - dtypes: PA_F32 (parity path, exact-f32 MFMA) and PA_BF16 (throughput path, bf16 MFMA,
 *     f32 accumulate).  Parameters, LayerNorm statistics, losses and gradients of
 *     parameters are always f32.
 *   - one process per GPU; calls are made from that process' host thread.
 */
#ifndef PLANK_HIP_H
#define PLANK_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PA_F32 0
#define PA_BF16 1

#define PA_EINVAL (-1)   /* bad argument (null pointer, unsupported size/dtype) */
#define PA_EALIGN (-2)   /* pointer / leading dimension not 16-byte aligned where required */
#define PA_ESHAPE (-3)   /* unsupported shape (e.g. head dim) */

int pa_version(void);

/* ------------------------------------------------------------------------------------------
 * GEMM with fused epilogue:  C[b] = epi( alpha * A[b] x B[b] ),  A: M x K, B: K x N.
 * Replaces every nn.Linear / torch.bmm on the path: MHA in_proj / out_proj
 * (torch F.multi_head_attention_forward), FFN linear1/linear2 (torch transformer.py
 * _ff_block), vocab_head / pointer_head (reference models.py:145-149) and their backward
 * GEMMs (dX = dY W, dW = dY^T X).
 *   a_kcontig: 1 -> A stored [M][K] (lda = row stride); 0 -> stored [K][M]
 *   b_kcontig: 1 -> B stored [N][K] (torch Linear weight layout); 0 -> stored [K][N]
 * epilogue order: *alpha, +bias[n], relu, relu-backward gate (aux[m][n] > 0 ? v*aux_scale : 0),
 * dropout(drop_p, drop_seed), +R[m][n].  Dropout decisions are counter-based and separable: element (row = b*M+m, col = n) is
 * kept iff the low 32 bits of A[row] * C[col] are >= drop_p * 2^32, A / C = 24-bit odd hashes of (drop_seed, row) / (drop_seed,
 * col) (csrc/pa_device.h drop_keep_rc; restated in tests/dropout_masks.py linear_keep); survivors are scaled by 1/(1-p).
 * splitk > 1: contraction split into `splitk` slices, partial products go through `ws`
 * (f32, splitk*batch*M*N elements) and a reduce pass applies the epilogue.
 */
typedef struct {
    const void* A; const void* B; void* C;
    const float* bias;          /* [N] f32 or NULL */
    const void* R;              /* residual [M][ldr], dtype = out_dtype, or NULL (may alias C) */
    const void* aux;            /* relu-backward gate [M][ldaux], dtype = in_dtype, or NULL */
    void* ws;                   /* split-K workspace or NULL */
    int32_t M, N, K;
    int32_t lda, ldb, ldc, ldr, ldaux;
    int64_t sA, sB, sC, sR, sAux;   /* batch strides in elements */
    int32_t batch;
    int32_t a_kcontig, b_kcontig;
    int32_t in_dtype, out_dtype;
    float alpha;
    int32_t relu;
    float aux_scale;
    float drop_p; uint32_t drop_seed;
    int32_t splitk;
    int32_t splitk_defer;   /* 1: only write the f32 slabs to `ws`; the caller reduces them later (pa_splitk_reduce_many) */
    int64_t sBias;          /* batch stride of `bias` in elements (0: one bias for every batch member) */
    void* C_lp;             /* optional bf16 copy [M][ldc_lp] of an f32 output (out_dtype PA_F32): the next Linear's matrix operand when
                             * the residual stream is kept in f32 (bf16 greedy decode).  Launches of at most 512 rows that take the
                             * skinny kernel only (PA_EINVAL otherwise) */
    int32_t ldc_lp; int32_t pad_lp_;
} pa_gemm_args;
int pa_gemm(const pa_gemm_args* a, void* stream);
/* Leave `n` of the 256 CUs free in every persistent GEMM launch from now on (0 <= n <= 192; 0 restores the full grid): room for
 * the RCCL kernels that all-reduce finished gradient slices while the backward continues (the data-parallel exchange the
 * reference gets from Lightning's `strategy: ddp`, configs/train_complete.yaml:18).  plankassembly_amd.distributed.GradSync
 * sets it (PA_RESERVE_CUS, default 0) when the first slice of a backward is sent and clears it once the last has been waited for. */
int pa_set_reserved_cus(int32_t n);
int pa_get_reserved_cus(void);
/* Slices pa_gemm really uses for a requested `splitk` (= number of slabs it writes; <= splitk). */
int pa_gemm_effective_splitk(int32_t K, int32_t in_dtype, int32_t splitk);
/* bf16x3 ("split") mode: while `on`, every pa_gemm call with in_dtype PA_F32 - the Linears of torch's Transformer layers and of
 * the heads, reference plankassembly/models.py:60-69,85-88 (nn.TransformerEncoder/DecoderLayer's linear1/2, in_proj, out_proj;
 * vocab / pointer / switch heads) and every gradient product of their backward - runs on the bf16 matrix pipe as
 * hi*hi + hi*lo + lo*hi of the operands' bf16 hi / lo parts with f32 accumulation (~2^-17 relative per product; operands, outputs,
 * epilogues and the split-K slabs stay f32).  `ws` / `bytes`: caller-owned, 256-byte aligned scratch for the split operands of ONE
 * GEMM at a time (launches are stream-ordered): 6 bytes per operand element, e.g. 256 MB for the 16 x 1024-row headline step.
 * A GEMM whose shape the bf16 fast paths do not take (contraction length not a multiple of 64 between two k-contiguous
 * operands, rows / leading dimensions not multiples of 8 / 4, scratch too small) silently runs exact f32 instead; pa_gemm_split_stats
 * counts both.  on = 2 ("retain", the backward segments): the cut image of every k-contiguous A operand - the dY of a dX GEMM -
 * stays in the scratch buffer until the next pa_gemm_split_config call, and pa_gemm_group reuses it for the weight gradients of the
 * same segment instead of cutting dY a second time.  on = 3 (the forward of a train step): the cut image of every k-contiguous A
 * operand - the input X of a Linear - stays at the front of the buffer through the following on = 0 / on = 2 calls, until the next
 * on = 3 or on = 1 call (or until the buffer is needed: at most 3/4 of it is used this way), and the weight gradients find X already
 * cut as well; images are keyed by (address, rows, cols, leading dimension), so the caller must not rewrite a Linear input
 * between its forward GEMM and its weight gradient - which a backward pass cannot do anyway.  on = 0 switches the mode off and
 * leaves the images alone.
 * WHOSE mode: every pa_gemm_split_* / pa_attn_split_* call (and every pa_gemm / pa_attn_* / pa_layernorm_* launch) made by a host
 * thread acts on the bf16x3 CONTEXT that thread has entered - one per model: mode flags, scratch, retained images, weight cache,
 * counters (round 6; rounds 4-5 kept one process-global state).  plankassembly_amd.models.PlankModel(compute_dtype="x3") creates
 * its own context and scratch and enters it around its library calls, so models of different compute modes can step from different
 * threads / on different streams, or alternate on one.  Outside any context the calls act on a process-default context (the
 * behaviour of rounds 4-5: kernel tests and tools that never create a context). */
int pa_split_ctx_create(void** out);
void pa_split_ctx_destroy(void* ctx);
int pa_split_ctx_enter(void* ctx);                            /* this host thread: ctx until the next enter; NULL = leave */
void* pa_split_ctx_current(void);
int pa_gemm_split_config(int32_t on, void* ws, int64_t bytes);
int pa_gemm_split_active(void);                               /* 1 while the mode is on */
int64_t pa_gemm_split_reused(void);                           /* weight-gradient operands found already cut (on = 2 / 3) since the last stats reset */
int pa_gemm_split_stats(int64_t* out2, int32_t reset);        /* out2[0] GEMMs run as bf16x3, out2[1] asked but run exact */
/* Images written by the PRODUCER of an operand (bf16x3 mode, retain modes 2 / 3).  pa_gemm_split_reserve: the kernel about to write
 * the f32 matrix `src` ([rows][cols], leading dimension ld, cols % 8 == 0) also writes its cut image - [rows][3 cols] bf16, parts
 * pattern *pat: 0 = (hi, hi, lo), 1 = (hi, lo, hi), hi = bf16(x), lo = bf16(x - hi) - to the returned address, and the pa_gemm call
 * that consumes `src` as its k-contiguous A operand (and, in a backward segment, the grouped weight-gradient launch) skips its own
 * cut.  NULL: no image wanted (mode off, no retain mode, no room); the consumer then cuts as before.  Used by
 * pa_layernorm_fwd_img (csrc/runtime.hip Ctx::ln_fwd). */
void* pa_gemm_split_reserve(const void* src, int32_t rows, int32_t cols, int32_t ld, int32_t* pat);
int64_t pa_gemm_split_made_hits(void);                        /* A operands found written by their producer since the last stats reset */
/* Images of the constant operands (the weights), owned by one model: a cache over a caller-owned device buffer (256-byte aligned;
 * 12 bytes per parameter + 32 KiB holds W and W^T of every Linear).  While a cache is in use (pa_gemm_split_cache_use, inside the
 * model's own pa_gemm_split_config bracket) every unbatched k-contiguous B operand of a bf16x3 GEMM is looked up in it; a miss is
 * cut INTO the cache (the first step learns the list).  pa_gemm_split_cache_refresh cuts every image again from its source in one
 * launch: call it whenever the parameters (or their transposed copies) changed.  The sources must stay alive and in place for as
 * long as the cache exists; destroy it before freeing them. */
int pa_gemm_split_cache_create(void* buf, int64_t bytes, void** out);
void pa_gemm_split_cache_destroy(void* cache);
int pa_gemm_split_cache_use(void* cache);                     /* NULL: none */
int32_t pa_gemm_split_cache_entries(void* cache);
int pa_gemm_split_cache_refresh(void* cache, void* stream);
int64_t pa_gemm_split_cache_hits(void);
/* Dry run of the mode's cut plan: what pa_gemm(args) (n == 1) or pa_gemm_group(args, n) (n > 1) would plan in the calling thread's
 * context, made by the same plan functions the real calls run.  It launches nothing, needs no GPU and never dereferences an operand,
 * scratch or cache pointer: only their values count.  commit != 0 advances the context (offsets, image lists, the cache's list, the
 * process counters) exactly as the real call does, so a whole sequence of calls can be replayed.  `out`: one entry per member.
 * Outside the mode, or for a product that is not f32, nothing is planned: taken = 0 and the caller's own arguments come back. */
#define PA_SPLIT_SRC_CALLER 0     /* not cut: the caller's own buffer (declined, or no such operand) */
#define PA_SPLIT_SRC_SEGMENT 1    /* found: retained by this backward segment (on = 2) */
#define PA_SPLIT_SRC_FORWARD 2    /* found: retained by the forward (on = 3) */
#define PA_SPLIT_SRC_MADE 3       /* found: written by the operand's producer (pa_gemm_split_reserve) */
#define PA_SPLIT_SRC_CACHE 4      /* found in the weight-image cache */
#define PA_SPLIT_SRC_CACHE_CUT 5  /* a cache miss: cut into the cache */
#define PA_SPLIT_SRC_SCRATCH 6    /* cut into the scratch */
typedef struct {
    int32_t taken;                        /* 1: runs as bf16x3; 0: declined (pa_gemm runs it exact, pa_gemm_group returns PA_EINVAL) */
    int32_t pat;                          /* parts pattern of A: 0 (hi, hi, lo), 1 (hi, lo, hi); B has the other one */
    int32_t drop_seg, drop_fwd;           /* image lists the call empties to make room */
    int32_t source[3], mode[3], blocks[3];/* A, B, aux: PA_SPLIT_SRC_*; split mode 0 .. 4 and blocks of the cut job (blocks 0: no cut) */
    int32_t M, N, K, lda, ldb, splitk;    /* the inner call: the bf16 product over 3 K, or the exact call of a declined product */
    int32_t nkeep, nkeepL, long_closed;   /* the context after the call: images of the segment / the forward, forward list closed */
    int64_t off[3], bytes[3];             /* A, B, aux: image offset from the scratch base (PA_SPLIT_SRC_CACHE*: the cache base); bytes cut */
    int64_t sA, sB;
    int64_t keep_off, long_off;           /* the context after the call: end of the retained images / of the forward's */
} pa_split_plan_info;
int pa_gemm_split_plan(const pa_gemm_args* args, int32_t n, int32_t commit, pa_split_plan_info* out);
/* Measurement hook (bench.py's roofline census; no reference counterpart): pa_gemm_record(1) starts appending every
 * pa_gemm() argument block to a host-side list; pa_gemm_record(0) returns the count so far; pa_gemm_recorded() copies
 * up to `cap` recorded blocks out and stops recording.  Replaying the blocks re-launches the same GEMMs. */
int pa_gemm_record(int32_t enable);
int pa_gemm_recorded(pa_gemm_args* out, int32_t cap);
/* Kernel each recorded launch was dispatched to (valid until the next pa_gemm_record(1)):
 * PA_GEMM_KIND_RING = gemm3_kernel (one block per CU, 4-stage LDS ring; single-round bf16 launches),
 * PA_GEMM_KIND_PAIR = gemm_kernel (two blocks per CU; everything else). */
#define PA_GEMM_KIND_PAIR 0
#define PA_GEMM_KIND_RING 1
#define PA_GEMM_KIND_WIDE 2   /* gemm3w_kernel: 128 x 256 tiles for the large multi-round Linears (opt-in); 192 x 128 ("tall") tiles for N <= 512 Linears a few 128 x 128 tiles past one round of the CUs */
#define PA_GEMM_KIND_SMALL 3  /* gemm3s_kernel: 64 x 64 tiles for launches that cover at most half of the CUs */
#define PA_GEMM_KIND_SKINNY 4 /* gemm_skinny_kernel: <= 512 rows against a whole weight (greedy decode), 32 x 32 tiles, K resident */
#define PA_GEMM_KIND_BIG 5    /* gemm8_kernel: eight waves on 256 x 256 / 256 x 128 tiles (plain k-contiguous Linears of many rows) */
int pa_gemm_recorded_kinds(int32_t* out, int32_t cap);
/* -1 for launches made by pa_gemm; members of one pa_gemm_group launch share an id >= 0 (consecutive entries). */
int pa_gemm_recorded_groups(int32_t* out, int32_t cap);
/* Dry run of the dispatch: the status pa_gemm(args) - or, with `ext`, pa_gemm_norm_a(args, ext) - would return before its launch
 * (0 where the real call launches; a launch error or the check of a deferred split-K epilogue, which follow the launch, are not
 * predicted) and, when that is 0, the kernel family (PA_GEMM_KIND_*), tile, grid, block size and effective split-K it would use.
 * Made by the same selection function the real calls run, under the same PA_GEMM_* switches and reserved CUs.  It launches nothing,
 * needs no GPU and never dereferences the operand pointers: only their values count, for the alignment rules.  It plans the plain
 * path and ignores the bf16x3 mode (where an f32 product is re-planned as a bf16 one over 3 K: pa_gemm_split_plan reports that
 * re-planned block).  pa_gemm_group has no dry run of its kernel choice. */
typedef struct {
    int32_t kind;               /* PA_GEMM_KIND_* ("tall" tiles report PA_GEMM_KIND_WIDE, as the recorder does) */
    int32_t tile_h, tile_w;
    int32_t grid, block;
    int32_t splitk;             /* non-empty contraction slices */
    int32_t units;              /* slots of the unit enumeration the grid strides over (padding of the XCD interleave included) */
    int32_t pad_;
} pa_gemm_plan_info;

/* Linear + bias (+ dropout) + residual + LayerNorm in one launch, for the post-norm sublayer tails of the reference's
 * encoder / decoder layers (torch nn/modules/transformer.py `x = norm(x + dropout(sublayer(x)))`, used by
 * plankassembly/models.py:76-112 through nn.TransformerEncoderLayer / nn.TransformerDecoderLayer):
 *     Z[M][512] = R + drop(A[M][K] W[512][K]^T + bias),   Y = LayerNorm(Z; gamma, beta, eps),   mean / rstd per row.
 * bf16 operands and outputs, f32 bias / gamma / beta / statistics; N must be 512, K a multiple of 64, rows 16-byte aligned.
 * Z, R, bias, mean, rstd may be NULL (Z is what pa_layernorm_bwd needs; the greedy-decode step does not keep it).
 * Bit-identical to pa_gemm (same arguments) followed by pa_layernorm_fwd.  One block per 32 rows: meant for
 * M <= pa_gemm_ln_max_rows() (one round of blocks); beyond that the two separate launches are faster. */
typedef struct {
    const void* A; const void* W; const float* bias; const void* R;
    void* Z; void* Y; const float* gamma; const float* beta; float* mean; float* rstd;
    int32_t M, N, K, lda, ldw, ldr, ldz, ldy;
    float eps, drop_p; uint32_t drop_seed; int32_t pad_;
} pa_gemm_ln_args;
int pa_gemm_ln(const pa_gemm_ln_args* a, void* stream);
int pa_gemm_ln_max_rows(void);

/* Linear on LayerNorm(Z) without a LayerNorm launch - for the post-norm chains of the greedy-decode step, where a sublayer's
 * output `x = norm(z)` (torch nn/modules/transformer.py, used by plankassembly/models.py:293-294 once per generated token) feeds the
 * next Linear and the next residual add and a LayerNorm on B rows is pure launch latency.  With y = (z - mean) rstd gamma + beta:
 *     y W^T + b  =  rstd (z (W gamma)^T - mean u) + v,     u[n] = sum_k W[n][k] gamma[k],   v[n] = b[n] + sum_k W[n][k] beta[k].
 * pa_ln_fold_weights prepares Wf = bf16(W gamma) (from the f32 master weight), u (summed over the ROUNDED Wf) and v once per
 * decode; pa_gemm_norm_a runs C = epi(rstd (A Wf^T - mean u) + v) on the raw rows A = Z (bf16, k-contiguous, K % 64 == 0,
 * N % 32 == 0; `args->B` = Wf, `args->bias` = v; no residual / gate / dropout / split-K), every block computing the row
 * statistics of its own 64 rows, and - when `y` is given - writes LayerNorm(Z) [M][K] for the later residual add.
 * 64 x 64 tiles, at most two per CU (PA_ESHAPE beyond). */
typedef struct {
    const float* u; const float* gamma; const float* beta;
    void* y; int32_t ldy; float eps;
    /* f32 residual stream (optional; <= 512 rows, K = 512 only - PA_ESHAPE otherwise): `zf` = the f32 rows Z [M][ldzf] of which
     * `args->A` is the bf16 copy.  The row statistics and the materialised LayerNorm(Z) are then computed from zf, and `y` is
     * written as f32 when y_f32 != 0. */
    const float* zf; int32_t ldzf; int32_t y_f32;
} pa_gemm_norm_ext;
int pa_ln_fold_weights(void* Wf, float* u, float* v, const float* W, const float* bias, const float* gamma, const float* beta,
                       int32_t N, int32_t K, void* stream);
int pa_gemm_norm_a(const pa_gemm_args* args, const pa_gemm_norm_ext* ext, void* stream);
/* the dry run of pa_gemm (ext NULL) / pa_gemm_norm_a: see pa_gemm_plan_info above */
int pa_gemm_plan(const pa_gemm_args* args, const pa_gemm_norm_ext* ext, pa_gemm_plan_info* out);
/* The same fold in exact f32 (the f32 greedy-decode step, round 4): pa_ln_fold_weights_f32 writes Wf = W gamma as f32; pa_gemm_norm_a
 * with in_dtype = out_dtype = PA_F32 takes f32 rows A (ext->zf = the same rows: the statistics source), Wf, u, v and writes f32.
 * At most 512 rows, K = 512 (PA_ESHAPE otherwise). */
int pa_ln_fold_weights_f32(float* Wf, float* u, float* v, const float* W, const float* bias, const float* gamma, const float* beta,
                           int32_t N, int32_t K, void* stream);

/* Several weight-gradient GEMMs (dW = dY^T X: bf16 operands, contraction index strided in both, f32 output, no
 * epilogue, batch 1; splitk > 1 only with splitk_defer) in one launch of the ring kernel: its unit stream runs through
 * all members.  PA_EINVAL when a member does not qualify - the caller then launches them one by one with pa_gemm. */
#define PA_MAX_GROUP 8
int pa_gemm_group(const pa_gemm_args* args, int32_t n, void* stream);

/* Column sums of several matrices in one launch: out[n] += sum_m X[m][n] (f32 atomics; outputs are accumulated
 * into).  The backward pass queues the bias gradients of a segment (dY buffers stay live until its end) and sums
 * them together.  Rows must be 16-byte aligned vectors (PA_EALIGN otherwise - use pa_colsum). */
#define PA_MAX_COLSUM 8
typedef struct {
    const void* X; float* out;
    int32_t M, N, ldx, pad_;
} pa_colsum_desc;
int pa_colsum_many(const pa_colsum_desc* descs, int32_t n_desc, int32_t dtype, void* stream);

/* Deferred split-K reduction for plain f32 outputs (weight gradients): out[m][n] = sum_s ws[s][m][n], one launch for
 * up to PA_MAX_REDUCE launches of pa_gemm(splitk_defer = 1).  The backward pass queues every dW of a segment and
 * reduces them together (13 launches per step instead of 69).  No reference counterpart (torch accumulates dW
 * inside its GEMM). */
#define PA_MAX_REDUCE 16
typedef struct {
    const float* ws; float* out;
    int32_t rows, cols, ld_out, splitk;
} pa_reduce_desc;
int pa_splitk_reduce_many(const pa_reduce_desc* descs, int32_t n_desc, void* stream);

/* Batched 2-D transposes dst[c][r] = src[r][c] (one launch for a table of matrices; descriptors live in device
 * memory, tile_begin = prefix sum of ceil(rows/64)*ceil(cols/64)).  Keeps the transposed shadow of the Linear
 * weights current so the backward GEMM dX = dY W runs with both operands k-contiguous. */
typedef struct {
    const void* src; void* dst;
    int32_t rows, cols, ld_src, ld_dst;
    int32_t tile_begin, pad_;
} pa_tr_desc;
int pa_transpose_many(const pa_tr_desc* descs_dev, int32_t n_desc, int32_t total_tiles, int32_t dtype, void* stream);

/* column sums: out[n] (+)= sum_m X[m][n]  (bias gradients).  f32 out. `partial` is scratch of
 * pa_colsum_ws_floats(M,N) floats. */
int64_t pa_colsum_ws_floats(int32_t M, int32_t N);
int pa_colsum(const void* X, int32_t dtype, int32_t M, int32_t N, int32_t ldx, float* out,
              int32_t accumulate, float* partial, void* stream);

/* ------------------------------------------------------------------------------------------
 * Embeddings.
 * pa_embed_input_fwd: reference models.py:103-112 (_embed_input): out[t] = sum_k table_k[idx_k[t]].
 *   tables: up to 5 f32 tables [rows_k][d]; idx: int64 [n_tok] each; a NULL idx skips the table
 *   (sideface batches have no input_type).
 * pa_embed_output_fwd: reference models.py:114-138 (_embed_output): out[b][0] = 0,
 *   out[b][t] = value[tok[b][t-1]] + coord[(t-1) % dof] + pos[(t-1) / dof], t in [1, T).
 *   tok has row stride tok_ld (the reference passes output_value[:, :-1]).
 * pa_embed_*_bwd: scatter-add of d_out into the f32 table gradients (atomic; tables with <= 8 rows, whose
 *   row count the caller passes in table_rows (host array), are pre-reduced per block in LDS).
 */
int pa_embed_input_fwd(void* out, int32_t out_dtype, const float* const* tables, const int64_t* const* idx,
                       const int32_t* rowmap, int32_t n_tables, int64_t n_tok, int32_t d, void* stream);
int pa_embed_input_bwd(const void* dout, int32_t dtype, float* const* dtables, const int64_t* const* idx,
                       const int32_t* rowmap, const int32_t* table_rows, int32_t n_tables, int64_t n_tok, int32_t d,
                       void* stream);
/* Embedding-table gradients by sorted segments: the token rows are grouped by table row once per batch - order[k] =
 * row indices (into dout) sorted by id, seg[k][r] .. seg[k][r+1] = the rows that use table row r (int32, seg has
 * table_rows[k] + 1 entries) - and each table row sums its segment: dtable[r] += sum (tables with few rows split
 * their long segments over several blocks and combine with one atomic per column; in larger tables a row used by more
 * than 64 tokens is split over 8 blocks the same way).  n_rows = rows of dout (sizes the
 * splitting).  The grouping depends only on the batch, so it is built when the batch is prepared
 * (PlankModel.prepare_batch); without it the atomic scatter-add kernels (pa_embed_input_bwd / _output_bwd) run. */
#define PA_MAX_SEG_TABLES 5
int pa_embed_segment_bwd(const void* dout, int32_t dtype, float* const* dtables, const int32_t* const* order,
                         const int32_t* const* seg, const int32_t* table_rows, int32_t n_tables, int64_t n_rows,
                         int32_t d, void* stream);
/* Row packing ("unpadding"): mask uint8 [B][S] (1 = PAD) -> cu int32 [2B+1] (cu[b] = #valid rows before batch element
 * b, cu[B] = total; entries B+1..2B = the batch elements by descending row count, the dispatch order of the
 * variable-length attention launches, pa_attn_args.order) and rowmap int32 [B*S] (rowmap[packed row] = b*S + s).  Padded
 * encoder positions never reach the loss (they are masked as keys everywhere), so the encoder stack can run on the
 * packed rows only; rowmap (optional, NULL = identity) lets the embedding kernels gather / scatter packed rows. */
int pa_pack_rows(const uint8_t* mask, int32_t B, int32_t S, int32_t* cu, int32_t* rowmap, void* stream);

/* Token rows grouped by embedding-table row (the `order` / `seg` inputs of pa_embed_segment_bwd) for up to
 * PA_MAX_GROUP_TABLES tables in ONE launch (one block per table; stable counting sort, so segment sums add in token order).
 * Batch-only information like pa_pack_rows: belongs where the batch is built (the reference builds its batches in the
 * dataloader, plankassembly/datasets/line_data.py:34-109; the gradients these groupings serve are those of
 * models.py:103-138).  kind 0: an input table - entry i (0 <= i < n) uses table row idx[rowmap ? rowmap[i] : i] and
 * reads gradient row i (the packed encoder rows).  kinds 1 / 2 / 3: the decoder's value / coordinate / position tables -
 * entry i = b * (T-1) + t1 reads gradient row b*T + t1 + 1 (decoder row t embeds token t-1) and uses table row
 * idx[b * tok_ld + t1] / t1 % dof / t1 / dof; n must be B * (T-1).
 * Outputs: order int32 [n] (gradient rows sorted by table row, ties in entry order), seg int32 [rows + 1]. */
#define PA_MAX_GROUP_TABLES 8
typedef struct {
    const int64_t* idx; const int32_t* rowmap;
    int32_t n, rows, kind, T, dof, tok_ld;
    int32_t* order; int32_t* seg;
} pa_group_desc;
int pa_group_rows(const pa_group_desc* descs, int32_t n_tables, void* stream);
int pa_embed_output_fwd(void* out, int32_t out_dtype, const float* value, const float* coord, const float* pos,
                        const int64_t* tok, int32_t tok_ld, int32_t B, int32_t T, int32_t d, int32_t dof,
                        void* stream);
int pa_embed_output_bwd(const void* dout, int32_t dtype, float* dvalue, float* dcoord, float* dpos,
                        const int64_t* tok, int32_t tok_ld, int32_t B, int32_t T, int32_t d, int32_t dof,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (biased variance), torch nn.LayerNorm as used by
 * TransformerEncoderLayer/DecoderLayer post-norm branch (torch nn/modules/transformer.py) with
 * eps = 1.0 per layer (reference models.py:60-61,66-67: normalize_before lands in the eps slot)
 * and 1e-5 for encoder.norm / decoder.norm (models.py:62,68).
 * fwd: y = (z - mean) * rstd * gamma + beta; saves mean/rstd (f32 [rows]).
 * bwd: dz from dy; dgamma/dbeta are ACCUMULATED into f32 outputs through `partial` scratch
 *      (pa_layernorm_ws_floats(rows, d) floats).  If drop_p > 0, also writes
 *      ddrop = dz * dropout_mask(seed, row*d+col) / (1-p)  (gradient of the sub-layer output
 *      that went through dropout before the residual add).  dzsum (optional) accumulates the
 *      column sums of that sub-layer-output gradient (ddrop if drop_p > 0, else dz) = the bias
 *      gradient of the Linear that produced it.
 */
int64_t pa_layernorm_ws_floats(int64_t rows, int32_t d);
int pa_layernorm_fwd(void* y, const void* z, const float* gamma, const float* beta, float* mean, float* rstd,
                     int64_t rows, int32_t d, float eps, int32_t dtype, void* stream);
int pa_layernorm_bwd(void* dz, void* ddrop, const void* dy, const void* z, const float* gamma,
                     const float* mean, const float* rstd, float* dgamma, float* dbeta, float* dzsum,
                     float* partial, int64_t rows, int32_t d, int32_t dtype,
                     float drop_p, uint32_t drop_seed, void* stream);
/* The same in two steps, so that several LayerNorm backward passes share ONE finishing launch: _partial writes only the
 * per-block partial sums (pa_layernorm_bwd_nparts(rows) blocks x 3 x d floats, a distinct `partial` buffer per pass until
 * finished); pa_layernorm_finish_many adds them to dgamma / dbeta / dzsum (dzsum may be NULL). */
int pa_layernorm_bwd_partial(void* dz, void* ddrop, const void* dy, const void* z, const float* gamma,
                             const float* mean, const float* rstd, int32_t want_dzsum, float* partial,
                             int64_t rows, int32_t d, int32_t dtype, float drop_p, uint32_t drop_seed, void* stream);
/* pa_layernorm_fwd that also writes the bf16x3 image of y (f32 only; img from pa_gemm_split_reserve, NULL = none) */
int pa_layernorm_fwd_img(void* y, const void* z, const float* gamma, const float* beta, float* mean, float* rstd,
                         int64_t rows, int32_t d, float eps, int32_t dtype, void* img, int32_t img_pat, void* stream);
/* pa_layernorm_bwd_partial that also writes the bf16x3 image of its output (ddrop, or dz when drop_p == 0) for the dX GEMM that
 * consumes it; only where pa_layernorm_bwd_can_img(d, dtype) says so (f32, d = 512). */
int pa_layernorm_bwd_can_img(int32_t d, int32_t dtype);
int pa_layernorm_bwd_partial_img(void* dz, void* ddrop, const void* dy, const void* z, const float* gamma,
                                 const float* mean, const float* rstd, int32_t want_dzsum, float* partial,
                                 int64_t rows, int32_t d, int32_t dtype, float drop_p, uint32_t drop_seed,
                                 void* img, int32_t img_pat, void* stream);
int32_t pa_layernorm_bwd_nparts(int64_t rows);
#define PA_MAX_LN_FINISH 4
typedef struct {
    const float* partial; float* dgamma; float* dbeta; float* dzsum;
    int32_t nparts, pad_;
} pa_ln_finish_desc;
int pa_layernorm_finish_many(const pa_ln_finish_desc* descs, int32_t n, int32_t d, void* stream);
/* The three batched end-of-segment reductions (pa_layernorm_finish_many, pa_colsum_many, pa_splitk_reduce_many) in
 * ONE launch: they are independent of each other, their blocks are concatenated.  Any of the three lists may be empty. */
int pa_segment_tail(const pa_ln_finish_desc* ln, int32_t n_ln, int32_t d_model, const pa_colsum_desc* cs, int32_t n_cs,
                    int32_t dtype, const pa_reduce_desc* rd, int32_t n_rd, void* stream);


/* ------------------------------------------------------------------------------------------
 * Multi-head attention core: softmax(Q K^T * scale + mask) V per (batch, head), flash-style
 * (scores never reach HBM).  Replaces torch F.multi_head_attention_forward's
 * bmm/softmax/dropout/bmm (torch 1.10) resp. scaled_dot_product_attention (torch 2.x) for the
 * encoder self-attention (key padding mask), decoder self-attention (causal + key padding,
 * reference models.py:85-89,209-214) and decoder cross-attention (memory key padding).
 *   Q/K/V/O: element (b, l, h, c) at ptr[(b*L + l)*ld + h*dh + c]  (head = contiguous dh slice,
 *   so Q/K/V may be views into the packed in_proj output);
 *   kpm: uint8 [B][Lk], 1 = masked key (PAD), or NULL;  causal: key j allowed iff j <= i;
 *   lse: f32 [B][H][Lq] log-sum-exp of the scaled, masked scores (saved for backward);
 *   dropout on the attention probabilities (torch MHA `dropout`): counter-based and separable - probability (row, key) with
 *   row = (b*H+h)*Lq + i is kept iff the low 32 bits of A[row] * C[key] are >= drop_p * 2^32 (csrc/pa_device.h drop_keep2, the
 *   same function the Linear epilogues use; tests/dropout_masks.py attn_keep); survivors are scaled by 1/(1-p); the backward
 *   kernels regenerate the same decisions.
 * bwd: dq/dk/dv have the layouts of q/k/v; delta is f32 scratch [B][H][Lq].
 *   Rows without an allowed key (a packed batch element with no keys; every key of the row masked by kpm, alone or together with the
 *   causal j <= i - row 0 when key 0 is masked): the softmax is over an empty set and the row is defined as O = 0 and lse = 0; in the
 *   backward it contributes nothing to dK / dV and its dQ row is 0.  dK / dV rows of masked keys are exactly 0, and a dropped
 *   probability contributes exactly 0.  Every kernel family keeps this contract (the first-generation f32 kernels are the standard:
 *   `l_tot > 0 ? ... : 0`); tests/attn_parity.py holds all of them to it.
 *   A launch writes only its windows: the H*dh columns of the rows of o / dq / dk / dv it owns (never the gap up to ld), and of lse
 *   only the rows of each batch element that exist (rows past a packed element's length keep what they held).
 */
typedef struct {
    const void* q; const void* k; const void* v; void* o;
    float* lse;
    const uint8_t* kpm;
    int32_t B, H, Lq, Lk, dh;
    int32_t ldq, ldk, ldv, ldo;
    int32_t causal;
    float scale;
    float drop_p; uint32_t drop_seed;
    int32_t dtype;
    /* backward only */
    const void* dout; void* dq; void* dk; void* dv; float* delta;
    int32_t lddo, lddq, lddk, lddv;
    /* variable-length ("unpadded") batches: int32 [B+1] row offsets of the packed Q resp. K/V rows of each batch
     * element, or NULL for the dense [B][L] layout.  With offsets, Lq/Lk are the per-batch maxima (grid size and
     * layout of lse/delta [B][H][Lq]); no padding mask is needed because padded tokens are simply not there. */
    const int32_t* cu_q; const int32_t* cu_k;
    /* optional dispatch order: int32 [B], a permutation of the batch elements by descending length (pa_pack_rows
     * leaves it in cu[B+1 .. 2B]).  All blocks of a launch start together, a few per CU, so a variable-length launch
     * lasts as long as the CU that drew the longest elements; in this order every CU gets a long, a medium and a short
     * block.  Results do not depend on it.  NULL = batch order. */
    const int32_t* order;
    /* optional scratch (device, 256-byte aligned; NULL = none) for packed bf16 self-attention launches (cu_q == cu_k, order given,
     * H = 8, dh = 64): the key range of a long batch element - resp. its query range in the dK / dV launch - is then cut across
     * several blocks whose partial results meet in this buffer (csrc/attention.hip decode_unit_split), so that the launch lasts
     * as long as its work instead of as long as its longest element's serial chain.  OPT-IN (PA_ATTN_SPLIT=1): on MI355X every
     * extra block costs ~6 us of slot time (lookup, first tile, publish + merge) and the split launches measured 15-20 % SLOWER
     * than one block per tile (profiles/r06_attention_launch_shape.txt).  Size: pa_attn_ws_bytes() (0 while the split is off).  Contract: its
     * first pa_attn_ws_ticket_bytes(ws_bytes) bytes are ZERO before the first launch that uses the buffer; every launch leaves them
     * zero.  Launches that share a buffer must be ordered on one stream.  Results do not depend on it beyond f32 summation order. */
    void* ws; int64_t ws_bytes;
} pa_attn_args;
int pa_attn_fwd(const pa_attn_args* a, void* stream);
int pa_attn_bwd(const pa_attn_args* a, void* stream);
/* scratch for pa_attn_args.ws: rows_total packed rows of B batch elements, the longest L_max rows (0 bytes when no launch of that
 * shape would use it: split not enabled - PA_ATTN_SPLIT=1 -, H != 8, or L_max short enough for one block per tile) */
int64_t pa_attn_ws_bytes(int32_t rows_total, int32_t B, int32_t H, int32_t L_max);
int64_t pa_attn_ws_ticket_bytes(int64_t ws_bytes);
/* Dry run of the dispatch: the status pa_attn_fwd(a) (bwd = 0) / pa_attn_bwd(a) (bwd != 0) would return before its first launch and,
 * when that is 0, the launches it would make, in order, and the fields of the kernel argument block the dispatch decides.  Made by the
 * same selection function the real calls run, under the same PA_ATTN_* / PA_X3_* switches and the caller's bf16x3 mode
 * (pa_attn_split_config).  It launches nothing, needs no GPU, counts nothing in pa_attn_split_taken and never dereferences the
 * operand pointers: only their values count (NULL tests, alignment, cu_q == cu_k). */
typedef struct {
    int32_t n_launches;         /* 1 (forward) .. 3 */
    int32_t balanced;           /* 0, 1 = packed self-attention in length-balanced block order, 2 = the same cut into range blocks */
    int32_t ks_min;             /* in-block key split: elements with fewer 64-key tiles run unsplit */
    int32_t parts_q, parts_kv;  /* bf16x3 backward: blocks per owned tile of the dQ resp. dK/dV launch */
    int32_t sp_slots;           /* range blocks: (owned tile, head) slots the scratch buffer `ws` holds */
    struct {
        char kernel[56];        /* the kernel's template-id as a demangler prints it, e.g. "attn4_fwd_kernel<true, 2>" */
        uint32_t grid[3];
        int32_t block, lds_bytes;
        int32_t extra;          /* second kernel argument of attn4_bwd_merged_kernel (its dQ blocks); 0 elsewhere */
    } launch[3];
} pa_attn_plan_info;
int pa_attn_plan(const pa_attn_args* a, int32_t bwd, pa_attn_plan_info* out);
/* bf16x3 ("split") attention, the companion of pa_gemm_split_config: while `on`, f32 launches with dh = 64 compute every matrix
 * product of torch's F.multi_head_attention_forward (reference plankassembly/models.py:60-69: S = Q K^T, O = P V) and of its
 * backward as hi*hi + hi*lo + lo*hi of the operands' bf16 hi / lo parts with f32 accumulation (csrc/attention_x3.h); inputs,
 * outputs, softmax statistics, masks, lse / delta and dropout decisions are the exact-f32 kernels'.  Other head sizes run exact.
 * pa_attn_split_taken: launches (forward or backward) that ran split since the last reset. */
int pa_attn_split_config(int32_t on);
int64_t pa_attn_split_taken(int32_t reset);

/* ------------------------------------------------------------------------------------------
 * Output heads + mixture NLL (training): reference models.py:140-166,186 (_create_dist training
 * branch) and 219-227 (nll_loss(ignore_index=PAD), argmax accuracy).
 * Inputs: vocab logits [rows][ldv] f32 (rows = B*T), pointer logits [B][T][T] f32 (already
 * scaled by 1/d_model), switch logit [rows] f32, labels int64 [rows] in [0, V+T).
 * fwd accumulates stats[0] += sum of -logp(label) over non-PAD rows, stats[1] += #non-PAD rows,
 * stats[2] += #correct argmax; saves per-row (lse_vocab, lse_ptr) for backward.
 * The training mask quirk is reproduced: pointer logits j >= i are REPLACED by the value 1e-6
 * and stay in the softmax.
 * bwd writes d(vocab logits), d(pointer logits) (zero where j >= i) in `out_dtype` (they feed the
 * backward GEMMs) and d(switch logit) in f32, for loss = stats[0] / stats[1]; the upstream
 * gradient is gscale * stats[3] (stats[3] is device resident so autograd's grad_output never
 * needs a host sync).
 * pa_switch_fwd: s[row] = h[row] . w + b (reference models.py:153), pa_switch_bwd its gradient
 * (dh += ds * w fused into the caller's GEMM epilogue is not possible, so dh_out is written
 * and dw/db accumulated).  `partial`: scratch of pa_layernorm_bwd_nparts(rows) x 2 x d floats.
 */
/* ACTIVATION: gelu (reference models.py:60-61,66-67 -> torch F.gelu, exact erf form).  The GEMM epilogues are ReLU-only; in GELU
 * mode the FFN's first Linear writes its pre-activation and these two element-wise launches do the rest:
 *   pa_gelu_fwd: out[r][c] = keep(seed, r, c) ? gelu(pre[r][c]) / (1 - p) : 0        (may run in place)
 *   pa_gelu_bwd: dpre[r][c] = dh[r][c] * gelu'(pre[r][c]) * (keep(seed, r, c) ? 1 / (1 - p) : 0)   (dpre may alias dh)
 * keep = pa_gemm's Linear-output dropout decision for (row r, column c) (csrc/pa_device.h drop_keep_rc), so a step under dropout takes
 * the same decisions as the fused ReLU epilogue would.  rows x cols elements, row stride ld, cols % 4 == 0, 8 / 16-byte aligned rows. */
int pa_gelu_fwd(void* out, const void* pre, int64_t rows, int32_t cols, int32_t ld, int32_t dtype, float drop_p, uint32_t drop_seed,
                void* stream);
int pa_gelu_bwd(void* dpre, const void* dh, const void* pre, int64_t rows, int32_t cols, int32_t ld, int32_t dtype, float drop_p,
                uint32_t drop_seed, void* stream);
int pa_switch_fwd(float* s, const void* h, int32_t dtype, const float* w, const float* b, int64_t rows,
                  int32_t d, void* stream);
int pa_switch_bwd(void* dh, int32_t accumulate, float* dw, float* db, const float* ds, const void* h,
                  int32_t dtype, const float* w, float* partial, int64_t rows, int32_t d, void* stream);
int pa_mixture_nll_fwd(float* stats, float* row_lse, const float* vocab, int32_t ldv, const float* ptr,
                       const float* sw, const int64_t* label, int32_t B, int32_t T, int32_t V, int32_t pad,
                       void* stream);
int pa_mixture_nll_bwd(void* dvocab, void* dptr, int32_t out_dtype, float* dsw, const float* stats,
                       const float* row_lse, const float* vocab, int32_t ldv, const float* ptr, const float* sw,
                       const int64_t* label, int32_t B, int32_t T, int32_t V, int32_t pad, float gscale,
                       void* stream);
/* The same forward on an EIGHT-float statistics block that the launch zeroes itself: [0] summed NLL, [1] unmasked rows, [2] correct
 * rows, [3] upstream d(loss) (armed with 1.0), [4] loss = [0] / [1], [5] accuracy = [2] / ([1] + 1e-10) - reference
 * plankassembly/models.py:226-231 - written by a one-wave finishing launch behind the forward kernel; [6], [7]: one int64, the NLL sum in units of 2^-30 (the blocks add
 * their sums there with an integer atomic, so the loss does not depend on the order they arrive in; stats8 must be 8-byte aligned).  The training step returns
 * views of [4] / [5]: no element-wise launches behind the forward.  pa_mixture_nll_bwd_up: `upstream` (device f32 scalar, or NULL =
 * stats[3]) is d(loss) from the caller's autograd - read in place instead of being copied into stats[3]. */
int pa_mixture_nll_fwd_fin(float* stats8, float* row_lse, const float* vocab, int32_t ldv, const float* ptr,
                           const float* sw, const int64_t* label, int32_t B, int32_t T, int32_t V, int32_t pad,
                           void* stream);
int pa_mixture_nll_bwd_up(void* dvocab, void* dptr, int32_t out_dtype, float* dsw, const float* stats,
                       const float* row_lse, const float* vocab, int32_t ldv, const float* ptr, const float* sw,
                       const int64_t* label, int32_t B, int32_t T, int32_t V, int32_t pad, float gscale,
                       const float* upstream, void* stream);
/* The EXTENDED objective: label smoothing, a weight per drawing or per token, and the plain -log p(label) per token (reference
 * plankassembly/models.py:219-227 is the case smoothing 0, no weight).  Row (b, i), label y, log p the training distribution of the
 * entries above (pointer logits j >= i hold the VALUE 1e-6 and stay in lse_p):
 *   plain  = -log p_y
 *   smooth = -(1 / C_i) sum over the ALLOWED classes {k < V} and {V + j : j < i} of log p_c,  C_i = V + i  (the filled pointers get no mass)
 *   ell    = (1 - eps) plain + eps smooth              (eps == 0: smooth is never formed)
 *   loss   = sum over non-PAD rows of w ell / N,       N = #non-PAD labels, w = weight[b] or weight[b][i] (1 without weights; any finite f32;
 *            a row of weight 0 adds exactly 0 and gets exactly zero gradients)
 * stats8 as pa_mixture_nll_fwd_fin, with [0] / [4] / [6..7] the objective sum w ell, the loss and its fixed-point word; count, hits and the
 * accuracy are unweighted and unsmoothed.  ext_stats receives the plain sum of -log p_y and its mean over N; token_nll the per-row plain value.
 * With smoothing 0 and weight NULL every stats8 / row_lse / gradient bit is that of pa_mixture_nll_fwd_fin / pa_mixture_nll_bwd_up.
 * The backward needs row_lse and stats8 only: G = gscale upstream / N w, and with eps > 0 BOTH parts of a row get a gradient
 * (d x_k = G [(1 - eps) ([y < V] softmax_v(k) - [k == y]) + eps / C_i (V softmax_v(k) - 1)], likewise the pointers j < i with i in place of V).
 * PA_EINVAL, nothing launched: smoothing outside [0, 1) or NaN, ext_stats NULL or not 8-byte aligned, weight_per_token not 0 / 1. */
typedef struct {
    float smoothing;            /* eps in [0, 1) */
    int32_t weight_per_token;   /* 0: weight is f32 [B];  1: f32 [B][T] */
    const float* weight;        /* NULL: every weight 1 */
    float* token_nll;           /* NULL, or f32 [B][T]: -log p(label), 0 at PAD rows */
    float* ext_stats;           /* f32[4], 8-byte aligned, zeroed by the launch: [0..1] int64 plain NLL sum in 2^-30 units, [2] plain mean, [3] 0 */
} pa_loss_ext;
int64_t pa_loss_ext_bytes(void);
int pa_mixture_nll_fwd_ext(float* stats8, float* row_lse, const float* vocab, int32_t ldv, const float* ptr,
                           const float* sw, const int64_t* label, int32_t B, int32_t T, int32_t V, int32_t pad,
                           const pa_loss_ext* e, void* stream);
int pa_mixture_nll_bwd_ext(void* dvocab, void* dptr, int32_t out_dtype, float* dsw, const float* stats,
                           const float* row_lse, const float* vocab, int32_t ldv, const float* ptr, const float* sw,
                           const int64_t* label, int32_t B, int32_t T, int32_t V, int32_t pad, float gscale,
                           const float* upstream, const pa_loss_ext* e, void* stream);

/* ------------------------------------------------------------------------------------------
 * Adam (torch.optim.Adam defaults; reference trainer_complete.py:127-129), fused over one flat
 * parameter buffer.  Optionally refreshes the bf16 shadow copy of the parameters.
 * `gscale` multiplies the gradient first (1/world_size for a summed all-reduce).
 */
int pa_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float b1,
                 float b2, float eps, int32_t step, float gscale, void* stream);
int pa_cast(void* dst, int32_t dst_dtype, const void* src, int32_t src_dtype, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradient guard: global-norm clipping (torch.nn.utils.clip_grad_norm_), value clipping (clip_grad_value_) and the skip
 * of a step whose gradient is not finite, decided ON THE DEVICE - no entry point below synchronises, allocates or reads
 * anything back.  The caller owns one workspace of pa_grad_guard_ws_bytes() bytes, 16-byte aligned:
 *   [0, 4 * PA_GRAD_GUARD_PARTIALS)   f32 per-block partial sums of squares
 *   [4 * PA_GRAD_GUARD_PARTIALS, ..)  one pa_grad_guard_ctl (the control block; pass its address to pa_adam_step_guarded)
 * pa_grad_guard_init zeroes the counters and sets `applied` = step0 >= 0 (the Adam step count a resumed optimizer hands over);
 * `first_skipped_attempt` = -1.
 *
 * pa_grad_guard (two launches): sum of squares of g[0, n) - per-thread f32 accumulation, wave shuffle, LDS, ONE plain store per
 * block, no atomics: block b sums the same elements in the same order every call, so the norm is bit-reproducible - then a
 * one-block finish that adds the partials in double in a fixed order and writes the control block:
 *   norm  = sqrt(sum) * |gscale|                       (the norm of the gradient Adam will see, g * gscale)
 *   coef  = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1
 *   apply = isfinite(norm) || !skip_nonfinite
 *   attempts += 1;  apply ? (applied += 1, step_size = lr / (1 - b1^applied), inv_sqrt_bc2 = 1 / sqrt(1 - b2^applied), in
 *   double as pa_adam_step computes them on the host) : (skipped += 1, first_skipped_attempt = attempts if it was -1).
 * The squares are taken in f32: an entry with |g| above ~1.8e19 overflows its square and the step counts as NON-FINITE,
 * although the entry itself is finite.
 *
 * pa_adam_step_guarded: pa_adam_step's loop, tail and bf16 shadow store, with step_size / inv_sqrt_bc2 / coef / apply read from
 * the control block: apply == 0 returns before any store (p, m, v and the shadow keep every bit); else the gradient it applies
 * is g * gscale * coef, clamped to +-clip_value when clip_value > 0.
 * g and ws must be 16-byte aligned (PA_EALIGN), n > 0, max_norm / clip_value >= 0 and not NaN, ws_bytes >= the size above
 * (PA_EINVAL); a failed check launches nothing. */
#define PA_GRAD_GUARD_PARTIALS 2048
typedef struct {
    float norm, coef, step_size, inv_sqrt_bc2;
    int32_t apply, applied, skipped, attempts, first_skipped_attempt;
    int32_t pad_[7];
} pa_grad_guard_ctl;
int64_t pa_grad_guard_ws_bytes(void);
int pa_grad_guard_init(void* ws, int64_t ws_bytes, int32_t step0, void* stream);
int pa_grad_guard(const float* g, int64_t n, float gscale, float max_norm, int32_t skip_nonfinite, float lr, float b1,
                  float b2, void* ws, int64_t ws_bytes, void* stream);
int pa_adam_step_guarded(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float b1, float b2,
                         float eps, float gscale, float clip_value, const pa_grad_guard_ctl* ctl, void* stream);

/* ------------------------------------------------------------------------------------------
 * Extended Adam: pa_adam_step / pa_adam_step_guarded with decoupled weight decay (torch.optim.AdamW) and an exponential moving
 * average (EMA) of the weights inside the same streaming pass.  One launch; no atomics, no LDS, nothing depends on block order.
 * Per element of an applied step, in this order:
 *   gj = g * gscale * coef, clamped to +-clip_value when clip_value > 0        (coef = 1 without ctl)
 *   m, v                    as pa_adam_step_guarded forms them (same fused multiply-adds, main loop and tail)
 *   p  = p * f              f = (float)(1.0 - (double)lr * weight_decay), computed once on the host; only when weight_decay > 0
 *                           and (decay_bits == NULL or the element's bit is set); rounded to f32 before the next line
 *   p -= step_size * m / fma(sqrt(v), inv_sqrt_bc2, eps)
 *   p_bf16 = (bf16)p        when p_bf16 != NULL
 *   e  = fma(1 - d_t, p - e, e)                                                 when ema != NULL
 * with d_t = ema_decay, or min(ema_decay, (1 + t) / (10 + t)) when ema_warmup, t = the Adam step count of THIS step.
 * ctl == NULL: t = step, and step_size, inv_sqrt_bc2 and 1 - d_t are computed on the host in double and rounded once.
 * ctl != NULL (the control block pa_grad_guard has just written): step_size / inv_sqrt_bc2 / coef / apply are read from it, t is
 * ctl->applied and every thread forms 1 - d_t by the host's expression; `step` is ignored, `lr` only enters f.  apply == 0 returns
 * before any store: p, m, v, the shadow AND the EMA keep every bit.
 * decay_bits: bit (i & 7) of byte (i >> 3) set = element i decays; ceil(n / 8) bytes, any alignment.
 * p, g, m, v, ema 16-byte aligned, ctl 4-byte aligned (PA_EALIGN); n > 0, clip_value >= 0, weight_decay >= 0 and finite,
 * 0 <= ema_decay < 1, none NaN, step >= 1 when ctl == NULL (PA_EINVAL); a failed check launches nothing. */
typedef struct {
    float* p; const float* g; float* m; float* v; void* p_bf16;
    float* ema;
    const uint8_t* decay_bits;
    int64_t n;
    float lr, b1, b2, eps, gscale, clip_value, weight_decay, ema_decay;
    int32_t step;
    int32_t ema_warmup;
    const pa_grad_guard_ctl* ctl;
} pa_adam_ext_args;
int64_t pa_adam_ext_args_bytes(void);
int pa_adam_step_ext(const pa_adam_ext_args* a, void* stream);
/* One-GPU rehearsal of the data-parallel gradient exchange (the reference's `strategy: ddp`, configs/train_complete.yaml:18-21):
 * a stand-in for one ring all-reduce.  `blocks` workgroups (<= 256) stay resident for at least `min_us` microseconds and stream
 * `buf` (16-byte aligned, `bytes` long; contents unchanged) through HBM at least `passes` times.  Launched on a side stream by
 * plankassembly_amd.distributed.GradSync when PLANK_FAKE_COLLECTIVE is set and the process group has one rank, so that the CU
 * reservation of the persistent GEMM grids (pa_set_reserved_cus) can be tuned without an 8-GPU node. */
int pa_fake_collective(void* buf, int64_t bytes, int32_t blocks, int32_t passes, float min_us, void* stream);

/* ------------------------------------------------------------------------------------------
 * Model-level runtime: one call enqueues the whole training forward of reference
 * plankassembly/models.py:190-233 (train_step: _embed_input, encoder, _embed_output, decoder,
 * _create_dist, nll_loss, accuracy) resp. its backward, on the caller's stream, using only the
 * caller's workspace.  `pa_model` is a small HOST-side object (configuration, parameter pointer
 * tables, workspace layout); it owns no device memory.
 *
 * Parameters are bound as three pointer tables in the canonical order of the reference
 * state_dict (plankassembly_amd/models.py PARAM_ORDER):
 *   params_f32 : f32 master parameters (embedding tables, biases, LayerNorm affine are read here)
 *   params_lp  : the same tensors in the compute dtype (GEMM B operands); = params_f32 for PA_F32
 *   params_lpT : (pa_model_bind_transposed, optional) transposed copies W^T [in][out] of the 2-D Linear weights
 *                at the same table positions (NULL entries = not available): dX = dY W then runs as a
 *                k-contiguous GEMM against W^T.  The caller refreshes them after each optimizer step
 *                (pa_transpose_many).
 *   grads      : f32 gradients (may be NULL for inference).  Gradients that are produced by
 *                accumulation (embedding tables, LayerNorm affine, out_proj/linear2 biases, switch
 *                head) are ADDED to: the caller zeroes the gradient buffer before backward.
 * The torch argument-order slip of the reference is explicit here: eps_layer = float(NORMALIZE_BEFORE)
 * (1.0), eps_final = 1e-5, has_enc_norm = bool(NORMALIZE_BEFORE), layers are post-norm.
 */
typedef struct pa_model pa_model;
typedef struct {
    int32_t d_model, n_head, d_ff, n_enc, n_dec, vocab;
    int32_t out_dof;
    int32_t in_table_rows[5];      /* rows of input_value / input_pos / input_coord / input_view / input_type */
    float eps_layer, eps_final;
    int32_t has_enc_norm;
    float dropout;
    int32_t pad, end;
    int32_t dtype;
    int32_t activation;            /* FFN activation: 1 ReLU (every shipped config), 2 GELU (torch's exact erf form); the reference hands
                                    * cfg.MODEL.ACTIVATION to nn.TransformerEncoderLayer / DecoderLayer (models.py:60-61,66-67).  0 = 1. */
} pa_model_cfg;
typedef struct {
    const int64_t* input_idx[5];   /* input_value, input_pos, input_coord, input_view, input_type (NULL ok) : [B][S] */
    const uint8_t* input_mask;     /* [B][S], 1 = PAD */
    const int64_t* output_value;   /* [B][T]  (NULL: run the encoder only) */
    const int64_t* output_label;   /* [B][T] */
    const uint8_t* output_mask;    /* [B][T] */
    int32_t B, S, T;
    /* optional packed-encoder mode: cu_in (int32 [2B+1]) and rowmap exactly as pa_pack_rows wrote them (the runtime also
     * reads the dispatch order it leaves in cu_in[B+1 .. 2B]), or cu_in == NULL for the dense path.  n_valid is the
     * host copy of cu_in[B] (the one device->host read of a training step). */
    const int32_t* cu_in; const int32_t* rowmap; int32_t n_valid;
    /* optional grouping of the token rows by table row (pa_embed_segment_bwd; NULL = atomic scatter-add kernels):
     * in_* for the five input tables over the (packed) encoder rows; out_* for the output embedding's value / coord /
     * pos tables over the B*T decoder rows (row (b,t) uses token t-1; rows with t = 0 are left out) */
    const int32_t* in_order[5]; const int32_t* in_seg[5];
    const int32_t* out_order[3]; const int32_t* out_seg[3];
} pa_batch;

#define PA_T_MEMORY 0
#define PA_T_HIDDENS 1
#define PA_T_VOCAB_LOGITS 2
#define PA_T_PTR_LOGITS 3
/* FFN hidden activation relu(linear1(x)) (after its dropout, when training with dropout) of encoder layer l / decoder layer l:
 * [encoder rows processed (packed: valid rows)][d_ff] resp. [B*T][d_ff], compute dtype.  Its sign pattern (> 0) is the ReLU
 * branch the backward pass differentiates (torch transformer.py _ff_block, reference models.py:60-61,66-67 activation=relu);
 * the parity tests evaluate the float64 oracle on exactly these branches. */
#define PA_T_ENC_FFN(l) (16 + (l))
#define PA_T_DEC_FFN(l) (80 + (l))

int pa_model_create(const pa_model_cfg* cfg, pa_model** out);
void pa_model_destroy(pa_model* m);
int pa_model_num_params(const pa_model* m);
int pa_model_bind(pa_model* m, void* const* params_f32, void* const* params_lp, void* const* grads);
int pa_model_bind_transposed(pa_model* m, void* const* params_lpT);
/* Optional (bf16): the cross-attention K/V rows of every decoder layer's in_proj_weight, transposed and packed side by
 * side: kvT_all[k][l * 2d + n] = in_proj_weight_l[d + n][k]  ([d][n_dec * 2d], low-precision dtype).  With it bound the
 * backward pass forms d(memory) with ONE GEMM over all layers instead of n_dec accumulating ones.  NULL unbinds. */
int pa_model_bind_cross_kv_t(pa_model* m, const void* kvT_all);
int64_t pa_model_train_ws_bytes(pa_model* m, int32_t B, int32_t S, int32_t T);
/* stats (device, f32[PA_MODEL_STATS_FLOATS] = f32[8]; the forward zeroes all eight itself - pa_mixture_nll_fwd_fin):
 * [0] sum of -log p(label) over non-PAD labels, [1] #non-PAD, [2] #correct.
 * loss = stats[0]/stats[1] (reference models.py:221), accuracy = stats[2]/(stats[1]+1e-10) (:227);
 * [3] upstream gradient d(objective)/d(loss), initialised to 1 by the forward and read (on the
 * device, no host sync) by the backward; [4] loss, [5] accuracy (written by the forward's last launch), [6], [7] the NLL sum as one
 * int64 in units of 2^-30 (order-free; the block must be 8-byte aligned).
 * A caller that sized the block for the four-float layout of rounds 1-4 gets a 16-byte out-of-bounds write: size it with
 * pa_model_stats_floats().
 * `seed` keys this step's dropout masks (training != 0 and cfg.dropout > 0). */
#define PA_MODEL_STATS_FLOATS 8
int32_t pa_model_stats_floats(void);                           /* = PA_MODEL_STATS_FLOATS of the loaded library */
int pa_model_train_fwd(pa_model* m, const pa_batch* batch, void* ws, int64_t ws_bytes, uint32_t seed,
                       int32_t training, float* stats, void* stream);
/* Backward in execution-ordered segments [seg_lo, seg_hi): 0 = heads + decoder.norm,
 * 1..n_dec = decoder layers (last layer first), then output embedding, encoder.norm, encoder
 * layers (last first), input embedding.  After segment s returns, the gradients of that
 * segment's parameters are final on `stream` (the shared value-embedding table only after the
 * last segment) - the host can launch their all-reduce on a side stream. */
/* d(loss) of the next pa_model_train_bwd calls is read from `upstream` (device f32 scalar; NULL = the stats block's own slot). */
int pa_model_set_upstream(pa_model* m, const float* upstream);
/* The objective of the next pa_model_train_fwd / pa_model_train_bwd calls: the block is COPIED (its pointers must stay valid until the
 * backward has been enqueued) and holds until set again; NULL = off, the calls of pa_mixture_nll_fwd_fin / pa_mixture_nll_bwd_up.  stats[4]
 * is then the extended loss.  PA_EINVAL for a block the _ext entries would reject. */
int pa_model_set_loss(pa_model* m, const pa_loss_ext* e);
int pa_model_train_num_segments(const pa_model* m);
int pa_model_train_bwd(pa_model* m, int32_t seg_lo, int32_t seg_hi, float gscale, void* stream);
/* Dry run of the training step's host side: the status pa_model_create / pa_model_train_ws_bytes would answer for `cfg` and a batch
 * of B drawings, S input positions, T output positions and n_valid packed encoder rows (0: unpacked, B * S rows; outside 0..B*S:
 * PA_EINVAL) and, when that is 0, the workspace and what pa_model_train_bwd plans before each segment: the weight gradients the
 * segment queues for its one grouped launch, in queue order, each with its split-K and its slab inside the split-K area of the
 * workspace.  Three kinds of segment queue any: 0 heads, 1 a decoder layer, 2 an encoder layer (reported whether or not cfg has such
 * layers).  Made by the layout function and the plan function the real calls run, under the caller's bf16x3 mode
 * (pa_gemm_split_config / pa_split_ctx_enter).  It needs no handle and no GPU and launches nothing. */
typedef struct {
    int32_t rows, cols;         /* dW[rows][cols] */
    int32_t k;                  /* contraction length: the activation rows */
    int32_t splitk;             /* effective split-K (pa_gemm_effective_splitk) */
    int64_t slab;               /* offset of its splitk x rows x cols slabs in the split-K area, in floats; -1: not split */
} pa_train_plan_member;
typedef struct {
    int64_t ws_bytes;           /* = pa_model_train_ws_bytes(handle of cfg, B, S, T) */
    int64_t splitws_floats;     /* the split-K area of the workspace */
    int32_t n_segments;         /* = pa_model_train_num_segments */
    int32_t n_members[3];
    pa_train_plan_member member[3][PA_MAX_GROUP];
} pa_train_plan_info;
int pa_train_plan(const pa_model_cfg* cfg, int32_t B, int32_t S, int32_t T, int32_t n_valid, pa_train_plan_info* out);
/* introspection for parity tests: device pointer + element count of an activation of the last forward */
int pa_model_tensor(pa_model* m, int32_t which, void** ptr, int64_t* numel);

/* ------------------------------------------------------------------------------------------
 * Greedy decode: reference plankassembly/models.py:267-307 (eval_step loop), 168-186 (_create_dist
 * eval branch, last row only), 235-256 (_sample).  K/V-cached (the reference recomputes the whole
 * prefix and the cross-attention K/V projection of `memory` every step); token-exact w.r.t. the
 * reference in PA_F32.
 *   1. run the encoder: pa_model_train_fwd with batch.output_value == NULL (T = 1);
 *   2. pa_decode_begin: lays out `ws` (pa_decode_ws_bytes), projects the cross-attention K/V of
 *      `memory` for every decoder layer once, resets the device-side step counter / outputs;
 *   3. pa_decode_step x Tmax: one token for every sequence.  All step kernels read the step index
 *      from device memory, so ONE captured hipGraph of a step can be replayed Tmax times;
 *   4. pa_decode_buffers: device pointers of tokens int64 [B][Tmax], attach int64 [B][Tmax]
 *      (-1 = no pointer), first_end int32 [B] (step at which END was first emitted, -1 = never),
 *      t_dev int32 (steps done).  The reference's early stop (all rows contain END) is the
 *      host checking first_end between replays and truncating to max(first_end)+1 columns.
 */
int64_t pa_decode_ws_bytes(pa_model* m, int32_t B, int32_t S, int32_t Tmax);
int pa_decode_begin(pa_model* m, void* ws, int64_t ws_bytes, int32_t Tmax, void* stream);
int pa_decode_step(pa_model* m, void* stream);
/* Dry run of the decode dispatch: the status pa_decode_begin / pa_decode_ws_bytes would answer for a handle of `cfg` with a batch of B
 * rows, memory length S and Tmax steps and, when that is 0, the forms the step takes and the bytes it needs.  Made by the same pure
 * function the real calls run, under the same PLANK_DECODE_* switches (read once per process).  It needs no handle and no GPU and
 * launches nothing.  Two half-batch lanes are two handles, each planned for its own rows. */
typedef struct {
    int32_t fold;               /* LayerNorm folded into the Linear that consumes it */
    int32_t f32res;             /* bf16 step with an f32 residual stream */
    int32_t mq;                 /* absorbed cross-attention: the step attends over the memory rows, no per-layer K / V caches */
    int32_t mq_contract;        /* W_v as its own launch + the ordinary out-projection behind the absorbed cross-attention */
    int32_t mq_self;            /* exact f32: the self-attention absorbed too (row cache of the layer inputs) */
    int32_t mq_self_bf;         /* bf16: the same */
    int32_t parts_cross, parts_self;    /* range blocks per row of the absorbed cross- / self-attention launch; 0 = no such launch */
    int32_t mq_nt, mq_swap, mq32_w8;    /* kernel variants of the absorbed launches: PLANK_DECODE_MQ_NT / _MQ_SWAP / _MQ32_W8 */
    int32_t pad_;
    int64_t mq_sp_bytes;        /* scratch of the range blocks inside the workspace */
    int64_t ws_bytes;           /* = pa_decode_ws_bytes(handle of cfg, B, S, Tmax) */
    int64_t scr_row;            /* beam reorder scratch per hypothesis row (B = rows; independent of K and of the row count), or a
                                 * negative PA_E* code where pa_decode_beam_ws_bytes answers with one */
} pa_decode_plan_info;
int pa_decode_plan(const pa_model_cfg* cfg, int32_t B, int32_t S, int32_t Tmax, pa_decode_plan_info* out);
int pa_decode_buffers(pa_model* m, void** tokens, void** attach, void** first_end, void** t_dev);
/* Decode groups: a decode of B * G rows over an encoder batch of B drawings - row r belongs to drawing r / G
 * (the layout of the beam and sampling modes below: row b*G + g).  The encoder runs ONCE on the B drawings (step 1 above, not on a
 * batch with every drawing repeated); pa_decode_group_begin keeps one copy of the memory rows, the key-padding mask and the packed
 * offsets - or, in the K / V-cache form, one set of cross-attention caches per layer - per DRAWING and sizes everything else for the
 * B * G rows.  From there on the decode is one of B * G rows: pa_decode_step, pa_decode_buffers and the beam, sampling, prefix and
 * constraint entries work on `rows` = B * G unchanged.  1 <= G <= PA_SAMPLE_MAX (PA_EINVAL otherwise).  pa_decode_begin /
 * pa_decode_ws_bytes are the G = 1 calls.
 * In the absorbed form two rows of a drawing share a block of the cross-attention launch where G is even and 2 * n_head <= 16 (the
 * block's 16 head slots; PLANK_DECODE_MQ_PAIR=0: never), which streams the drawing's memory once for both.
 *   pa_decode_group_plan: the dry run (pa_decode_plan for G = 1, field for field): `out` for B * G rows - the decisions that depend
 *     on the row count use B * G, parts_cross counts range blocks per UNIT (block of rows_per_block rows), ws_bytes is
 *     pa_decode_group_ws_bytes - and the group itself in `g`. */
typedef struct {
    int32_t rows;               /* B * G */
    int32_t rows_per_block;     /* rows of a drawing per block of the absorbed cross-attention launch: 1 or 2 (1 without that launch) */
    int32_t units;              /* rows / rows_per_block: the blocks of that launch before range blocks */
    int32_t pad_;
    int64_t mem_rows;           /* B * S: the memory rows (and mask bytes) the workspace keeps - one set per drawing */
} pa_decode_group_info;
int64_t pa_decode_group_ws_bytes(pa_model* m, int32_t B, int32_t G, int32_t S, int32_t Tmax);
int pa_decode_group_begin(pa_model* m, int32_t G, void* ws, int64_t ws_bytes, int32_t Tmax, void* stream);
int pa_decode_group_plan(const pa_model_cfg* cfg, int32_t B, int32_t G, int32_t S, int32_t Tmax, pa_decode_plan_info* out,
                         pa_decode_group_info* g);
/* Beam search over the same step.  K beams per drawing, 1 <= K <= PA_BEAM_MAX: the caller runs the encoder and
 * pa_decode_begin on the batch with every drawing repeated K times (row b*K + k is beam k of drawing b), then switches the decode to
 * beam mode.  pa_decode_step then ends each step with the beam selection instead of the greedy arg-max:
 *   - per row, the K most probable candidates of the greedy step's own distribution (vocab entries and pointers j < t, first-max order,
 *     p = 0 never taken); a finished row has the one candidate (PAD, attach -1, log p 0);
 *   - per drawing, the K best of the K*K candidates by score + logf(p) (f32; ties to the smaller parent beam, then the better rank)
 *     become the new beams; a beam that emits END is finished and frozen;
 *   - rows whose parent is another row take the parent's history (self-attention caches, hidden-state cache, tokens, attach).
 * Everything is read from device memory: the step still captures into one hipGraph.  K = 1 gives the greedy tokens, with PAD / -1
 * after a row's first END.  The next pa_decode_begin returns the handle to greedy mode.
 *   pa_decode_beam_ws_bytes: bytes of the beam workspace for `rows` = B*K rows (the batch pa_decode_begin was given), memory length S
 *     and Tmax (the same values as pa_decode_ws_bytes); PA_EINVAL for K outside [1, PA_BEAM_MAX] or rows not a multiple of K.
 *   pa_decode_beam_begin: after pa_decode_begin, lays out `ws` (256-byte aligned, pa_decode_beam_ws_bytes bytes) and resets the beam
 *     state on `stream`: score 0 for beam 0 of every drawing and -inf for the others, nothing finished, every row its own parent.
 *     PA_EINVAL for a decode that was not begun, a bad K, rows % K != 0 or a workspace too small.
 *   pa_decode_beam_buffers: device pointers of scores f32 [rows] (cumulative log-probability), parents int32 [rows] (the row each beam
 *     came from in the last step) and finished int32 [rows] (1 = has emitted END).  Tokens / attach / first_end of every beam are the
 *     pa_decode_buffers arrays. */
#define PA_BEAM_MAX 16
int64_t pa_decode_beam_ws_bytes(pa_model* m, int32_t rows, int32_t S, int32_t Tmax, int32_t K);
int pa_decode_beam_begin(pa_model* m, int32_t K, void* ws, int64_t ws_bytes, void* stream);
int pa_decode_beam_buffers(pa_model* m, void** scores, void** parents, void** finished);
/* Sampling over the same step.  N samples per drawing, 1 <= N <= PA_SAMPLE_MAX: the caller runs the encoder and
 * pa_decode_begin on the batch with every drawing repeated N times (row b*N + n is sample n of drawing b), then switches the decode to
 * sampling mode.  pa_decode_step then ends each step with one random draw per row instead of the greedy arg-max:
 *   - the candidates are the greedy step's own distribution: vocab entries and pointers j < t with p > 0, ranked by p descending, ties
 *     to the smaller index;
 *   - weights w = expf((logf(p) - logf(p_max)) / temperature) (p / p_max at temperature 1); top_k > 0 keeps the first top_k in rank
 *     order, top_p < 1 then the shortest rank-order prefix whose sum of w reaches top_p times the sum of the kept w;
 *   - u = (h >> 8) 2^-24 with h = mix32(t ^ mix32(n ^ mix32(b ^ mix32(seed + 0x9e3779b9)))) (b = drawing, n = sample, t = step);
 *     the first kept candidate in index order (vocab, then pointers) whose inclusive prefix sum of w exceeds u times the total;
 *   - a pointer j writes the row's own token at j and attach j; the row's score gains logf(p) of the chosen candidate (untempered,
 *     unfiltered: the model's log-likelihood of the sample); a row that has emitted END is frozen (PAD, attach -1, score + 0).
 * Everything is read from device memory, the parameters included: the step captures into one hipGraph, and pa_decode_sample_set
 * changes seed / temperature / top_k / top_p for the next steps without a new capture.  The same parameters give bitwise the same
 * samples on every run.  top_k = 1 gives the greedy tokens up to each row's first END.
 * pa_decode_begin returns the handle to greedy mode; pa_decode_beam_begin and pa_decode_sample_begin replace
 * each other's mode (the last one called wins).  Vocabularies above 2048 entries: PA_ESHAPE.
 *   pa_sample_params: seed; n_per_drawing = N; temperature > 0 and finite; top_k >= 0 (0 = off); 0 < top_p <= 1 (1 = off).
 *   pa_decode_sample_ws_bytes: bytes of the sampling workspace for `rows` = B*N rows (the batch pa_decode_begin was given).
 *   pa_decode_sample_begin: after pa_decode_begin, lays out `ws` (256-byte aligned, pa_decode_sample_ws_bytes bytes), writes the
 *     parameters and zeroes the scores on `stream` (a kernel: no host-to-device copy).  PA_EINVAL for a decode that was not begun, N
 *     outside [1, PA_SAMPLE_MAX], rows not a multiple of N, a bad temperature / top_k / top_p or a workspace too small.
 *   pa_decode_sample_set: new parameters for a decode in sampling mode, on `stream`, same workspace, scores kept; N must be the N of
 *     pa_decode_sample_begin.  PA_EINVAL otherwise, or for bad parameters.
 *   pa_decode_sample_buffers: device pointer of scores f32 [rows] (cumulative log-probability of every sample).  Tokens / attach /
 *     first_end of every sample are the pa_decode_buffers arrays. */
typedef struct {
    uint32_t seed;
    int32_t n_per_drawing;
    float temperature;
    int32_t top_k;
    float top_p;
} pa_sample_params;
#define PA_SAMPLE_MAX 64
int64_t pa_decode_sample_ws_bytes(pa_model* m, int32_t rows);
int pa_decode_sample_begin(pa_model* m, const pa_sample_params* p, void* ws, int64_t ws_bytes, void* stream);
int pa_decode_sample_set(pa_model* m, const pa_sample_params* p, void* stream);
int pa_decode_sample_buffers(pa_model* m, void** scores);
/* Forced prefixes over the same step, in any mode: completion of a partly known sequence, and - with every
 * position forced - the log-likelihood of a sequence the caller brings.  The prefix table gives per row r (a row of the batch
 * pa_decode_begin was given: a sample, a beam, a batch element) a length plen[r], 0 <= plen <= Tmax, and for t < plen[r] the forced
 * candidate: ptok[r][t] with patt[r][t] = -1 for the vocab entry ptok, or patt = j >= 0 for the pointer candidate j.  At step t a row
 * with t < plen[r] ("forced row"):
 *   - writes its hidden state and computes the distribution exactly as a free row does;
 *   - takes the forced candidate without arg-max, ranking or draw (the random number of sampling stays a function of (seed, b, n, t));
 *     token ptok and attach patt are written, a pointer writing the row's own token at patt as a free step does (the caller makes sure
 *     that ptok agrees with it);
 *   - stores lp = logf(p of the forced candidate) in prefix_lp[r][t] and adds it, in step order, to prefix_score[r] - and in beam and
 *     sampling mode to the mode's own score, which stays the log-likelihood of the whole sequence;
 *   - a forced END sets first_end (beam mode: finished) as a free END does.  In beam and sampling mode a row frozen by END ignores the
 *     rest of its prefix.  Greedy mode freezes nothing: positions after END are still forced and stored in prefix_lp up to plen, but
 *     prefix_score stops after the row's first END (END's own lp included);
 *   - a forced candidate that does not exist at its step (a pointer with patt >= t or at t < 5, a token outside the vocabulary) scores
 *     -inf and reads nothing out of bounds; such a token is written as PAD.
 * Beam mode: the K rows of a drawing must carry the same prefix.  A forced live row has the single candidate at rank 0, so during the
 * prefix beam 0 carries the hypothesis and beams 1 .. K-1 stay at -inf, as at t = 0 without a prefix; the first free step fans out
 * from beam 0, and prefix_score / prefix_lp of the drawing are those of its row b*K.  Rows with t >= plen[r] behave exactly as without
 * a table, in the same step.  Without pa_decode_prefix_begin every mode launches the kernels it launched before and gives the same
 * bits, and a step with a table has the same launches.  Everything is read from device memory: the step captures into one hipGraph and
 * a new table needs no new capture.  pa_decode_begin clears the prefix.
 *   pa_decode_prefix_ws_bytes: bytes of the prefix workspace for `rows` rows and Tmax positions.
 *   pa_decode_prefix_begin: after pa_decode_begin and after any pa_decode_beam_begin / pa_decode_sample_begin.  plen int32 [rows],
 *     ptok / patt int64 [rows][Tmax] are DEVICE pointers (positions t >= plen[r] are not read by the step); a kernel on `stream` copies
 *     them into `ws` (256-byte aligned, pa_decode_prefix_ws_bytes bytes; plen clamped to [0, Tmax]) and zeroes prefix_score /
 *     prefix_lp - no host-to-device copy.  PA_EINVAL for a decode that was not begun, a null table or a workspace too small.
 *   pa_decode_prefix_set: a new table for a decode with a prefix, on `stream`, same workspace (prefix_score / prefix_lp zeroed again).
 *   pa_decode_prefix_buffers: device pointers of prefix_score f32 [rows] and prefix_lp f32 [rows][Tmax] (0 where nothing was forced). */
int64_t pa_decode_prefix_ws_bytes(pa_model* m, int32_t rows, int32_t Tmax);
int pa_decode_prefix_begin(pa_model* m, const int32_t* plen, const int64_t* ptok, const int64_t* patt, void* ws, int64_t ws_bytes,
                           void* stream);
int pa_decode_prefix_set(pa_model* m, const int32_t* plen, const int64_t* ptok, const int64_t* patt, void* stream);
int pa_decode_prefix_buffers(pa_model* m, void** prefix_score, void** prefix_lp);
/* Plank grammar over the same step, in any mode: programs that are valid by construction.  A plank is six
 * coordinate tokens x0 y0 z0 x1 y1 z1 (out_dof must be 6; PA_EINVAL otherwise) with n_val coordinate values 0 .. n_val - 1, and END
 * closes the program at a plank boundary.  At step t = 6 k + c the written token of a FREE row must lie in a window that depends on t
 * and on the row's own token at t - 3 alone:
 *   c == 0 and k >= max_planks:  END only (max_planks is clamped to (Tmax - 1) / 6, the last boundary that leaves room for END);
 *   c == 0 otherwise:            [0, n_val - 2], plus END when k >= min_planks;
 *   c in 1 .. 2:                 [0, n_val - 2];
 *   c in 3 .. 5:                 [min(tokens[t - 3], n_val - 2) + 1, n_val - 1] (the clamp keeps the window non-empty whatever the
 *                                history: a greedy row steps on after its END, a forced prefix may put anything at t - 3).
 * PAD is never allowed.  A vocab candidate k writes token k; a pointer candidate j < t writes the row's own token at j and is judged by
 * it; a pointer j >= t is never allowed.  The p of every candidate stays what the unconstrained step computes (the 1e-6 pointer fill
 * included) - the constraint only removes candidates from the selection: the greedy arg-max runs over the allowed candidates (first-max
 * order; one with p = 0 still beats every disallowed one), the beam ranking and the sampler's candidate set are the allowed candidates
 * with p > 0.  Scores are not renormalised: beam scores, sample scores and prefix scores stay the model's own log-likelihood.  Forced
 * positions (pa_decode_prefix_*) are not filtered.  Should every allowed candidate have p == 0 in f32, beam rank 0 and the sampler write
 * the window's lowest token (END for the END-only window) with log p = -inf; nothing is read out of bounds and no loop depends on it.
 * The parameters travel as kernel arguments: a captured step depends on them (capture again after a change).  Host state only, no
 * launch.  pa_decode_begin clears the constraint.
 *   pa_decode_constraint_set: after pa_decode_begin; p == NULL clears.  PA_EINVAL for a decode that was not begun, min_planks < 0,
 *     max_planks < max(min_planks, 1), n_val < 2 or n_val above the vocabulary. */
typedef struct {
    int32_t n_val;        /* coordinate values: min(END, PAD) */
    int32_t min_planks;   /* END allowed from this plank boundary on */
    int32_t max_planks;   /* END forced at this plank boundary */
    int32_t pad_;
} pa_constraint_params;
int pa_decode_constraint_set(pa_model* m, const pa_constraint_params* p);
/* Cross-attention of one decode step in absorbed ("multi-query") form (reference plankassembly/models.py:284-307, the
 * cross-attention of nn.TransformerDecoderLayer with K = W_k memory + b_k, V = W_v memory + b_v): per batch element and head
 * ctx[b][h][:] = sum_s softmax_s(qt[b][h] . mem[s]) mem[s] over the element's memory rows, where the caller has put
 * qt_h = scale log2(e) W_k,h^T q_h into `qt` and applies W_v,h (+ b_v,h) to ctx afterwards.  bf16, d == 512, H <= 8
 * (PA_ESHAPE otherwise).  qt, ctx: [B][H][512]; mem: dense [B][S][512] with optional kpm [B][S] (1 = PAD) or packed rows
 * with cu [B + 1]. */
int pa_dec_cross_mq(void* ctx, const void* qt, const void* mem, const uint8_t* kpm, const int32_t* cu, int32_t B, int32_t S,
                    int32_t H, int32_t d, void* stream);
/* The same in exact f32 (f32 ctx / qt / mem; v_mfma_f32_16x16x4_f32): the cross-attention of the parity (token-exact) decode. */
/* pa_dec_cross_mq with scratch for RANGE BLOCKS: below ~256 batch elements one block per element leaves most CUs idle (one CU streams
 * an element's S x 512 memory rows at ~22 GB/s); with scratch an element's keys are walked by up to 256 / B blocks whose partial
 * (O, m, l) are merged by the last one to arrive (csrc/decode_mq.h, csrc/split_merge.h).  ws: pa_dec_cross_mq_ws_bytes(B, S) bytes,
 * 256-byte aligned, its first ceil(4 B / 256) * 256 bytes ZERO before the first launch (launches leave them zero). */
int64_t pa_dec_cross_mq_ws_bytes(int32_t B, int32_t S);
int pa_dec_cross_mq_ws(void* ctx, const void* qt, const void* mem, const uint8_t* kpm, const int32_t* cu, int32_t B,
                       int32_t S, int32_t H, int32_t d, void* ws, int64_t ws_bytes, void* stream);
int pa_dec_cross_mq32_ws(float* ctx, const float* qt, const float* mem, const uint8_t* kpm, const int32_t* cu, int32_t B,
                         int32_t S, int32_t H, int32_t d, void* ws, int64_t ws_bytes, void* stream);    /* the exact-f32 form (same scratch size) */
int pa_dec_cross_mq32(float* ctx, const float* qt, const float* mem, const uint8_t* kpm, const int32_t* cu, int32_t B, int32_t S,
                      int32_t H, int32_t d, void* stream);
/* The same launches for a decode group: mem / kpm / cu of B drawings, qt / ctx [B * G][H][512], row r attends over drawing r / G.
 * rows_per_block 1 or 2 rows of a drawing per block (2: G even and 2 H <= 16, PA_EINVAL otherwise).  nparts 0: range blocks by the
 * rule, for the launch's units = B * G / rows_per_block; n > 0: n per unit, or 1 where ws cannot hold them.  ws: 256-byte aligned,
 * ceil(4 units / 256) * 256 zero ticket bytes + units * nparts * 40 KB.  G 1, rows_per_block 1, nparts 0 is pa_dec_cross_mq_ws. */
int pa_dec_cross_mq_group(void* ctx, const void* qt, const void* mem, const uint8_t* kpm, const int32_t* cu, int32_t B, int32_t G,
                          int32_t S, int32_t H, int32_t d, int32_t rows_per_block, int32_t nparts, void* ws, int64_t ws_bytes,
                          void* stream);
int pa_dec_cross_mq32_group(float* ctx, const float* qt, const float* mem, const uint8_t* kpm, const int32_t* cu, int32_t B, int32_t G,
                            int32_t S, int32_t H, int32_t d, int32_t rows_per_block, int32_t nparts, void* ws, int64_t ws_bytes,
                            void* stream);
/* The self-attention form of the same launch (exact f32; what the token-exact decode step runs on its cache of layer-input rows):
 * rows [B][Tmax][512], of which element b attends over rows 0 .. *t_dev (the key count t + 1 is read on the device, so the launch can
 * sit in a captured graph). */
int pa_dec_self_mq32(float* ctx, const float* qt, const float* xcache, const int32_t* t_dev, int32_t B, int32_t Tmax, int32_t H,
                     int32_t d, void* stream);
/* The self-attention form in both types (dtype PA_F32 / PA_BF16: the type of ctx, qt and xcache; the bf16 form is what the bf16 step
 * runs from PLANK_DECODE_MQ_SELF_MINB rows on).  nparts 0: one block per row - with PA_F32 that is pa_dec_self_mq32, bit for bit;
 * n > 0: n range blocks per row, or 1 where ws cannot hold them (ws as for pa_dec_cross_mq_group with units = B). */
int pa_dec_self_mq_ws(void* ctx, const void* qt, const void* xcache, const int32_t* t_dev, int32_t B, int32_t Tmax, int32_t H, int32_t d,
                      int32_t dtype, int32_t nparts, void* ws, int64_t ws_bytes, void* stream);
/* The kernels csrc/decode.hip itself defines, each on its own with the grid the step gives it (tests).  dtype
 * PA_F32 / PA_BF16 is the type of the rows.
 *   pa_dec_attn: the single-query attention over per-head caches kc / vc [B / G][H][Lmax][dh] -> out [B][d]; q rows ldq apart.  The key
 *     count is cu[b / G + 1] - cu[b / G], else fixed_lk > 0, else *t_dev + 1 read on the device.  newkv [B][3d] (the self form): key
 *     Lk - 1 is taken from its K / V slices and appended to row Lk - 1 of both caches.  kpm [B / G][Lmax], 1 = PAD.  Refused before any
 *     launch: PA_EINVAL for a NULL out / q / kc / vc, no source of the key count, fixed_lk > Lmax, G < 1, B % G != 0, newkv together
 *     with cu, kpm or G > 1; PA_ESHAPE for d / H outside {16, 32, 64}; PA_EALIGN for out / q / kc / vc / newkv off 16 bytes or ldq not a
 *     multiple of the 16-byte vector (4 f32, 8 bf16).
 *   pa_dec_split_heads: kv [rows][2d] (k | v) -> kc, vc [B][H][S][dh]; dense rows b S + s, or packed with cu [B + 1] and rowmap [rows]
 *     (the dense row of a packed one; both or neither).
 *   pa_dec_embed: x [B][d] (dtype) = value[tokens[b][t - 1]] + coord[(t - 1) % dof] + pos[(t - 1) / dof], zeros at t = *t_dev = 0; x_lp
 *     (optional) the bf16 copy of the same f32 sums.
 *   pa_dec_row_dist: per row, what the greedy / beam / sampling / forced tails compute before they choose: h stored into row t of
 *     hid_cache [Tmax][rows][d], then p of every candidate index - vocab k at p_out[row][k], pointer j <= t at p_out[row][V + j]
 *     (p_out [rows][V + Tmax]; nothing else is written, and no pointer while t + 1 < 6) - and (vmax, vsum, pmax, psum, prob) in
 *     stats [rows][5].  0 <= *t_dev < Tmax <= 2048 is the caller's to keep. */
int pa_dec_attn(void* out, const void* q, int32_t ldq, void* kc, void* vc, int32_t Lmax, const uint8_t* kpm, int32_t fixed_lk,
                const int32_t* t_dev, int32_t B, int32_t H, int32_t d, int32_t dtype, const int32_t* cu, const void* newkv, int32_t G,
                void* stream);
int pa_dec_split_heads(void* kc, void* vc, const void* kv, int64_t rows, int32_t S, int32_t d, int32_t H, int32_t dtype, const int32_t* cu,
                       const int32_t* rowmap, void* stream);
int pa_dec_embed(void* x, void* x_lp, const float* value, const float* coord, const float* pos, const int64_t* tokens, int32_t Tmax,
                 const int32_t* t_dev, int32_t B, int32_t d, int32_t dof, int32_t dtype, void* stream);
int pa_dec_row_dist(float* p_out, float* stats, const float* vlog, int32_t ldv, const void* pfeat, const void* h, void* hid_cache,
                    const float* sw_w, const float* sw_b, const int32_t* t_dev, int32_t rows, int32_t Tmax, int32_t d, int32_t V,
                    int32_t dtype, void* stream);

/* ---- device-resident dataset (csrc/tokenise.hip; plankassembly_amd/device_data.py) ----
 * One launch, one block of 256 threads per batch element: the prepared drawings stay in HBM as CSR arrays and a batch is
 * tokenised where the model reads it.  Restates plankassembly_amd/datasets.py `_sorted_tokens`, `_pad_inputs`,
 * `prepare_output_sequence` and `add_noise` (reference plankassembly/datasets/line_data.py:34-83 input sequence, :85-109
 * output sequence, :128-133 augmentation; sideface_data.py:137-213; data_utils.py:6-12 quantisation, :24-68 noise), bit for
 * bit: float64, every product and sum rounded on its own, truncation toward zero.
 *   line_off int32 [N+1], box f64 [L][4] (xmin ymin xmax ymax, used as stored when a drawing is not augmented), seg f64
 *   [L][4] (x0 y0 x1 y1 of the straight segment; NULL: side faces, no augmentation), view / type uint8 [L] (type NULL
 *   with with_type = 0), plank_off int32 [N+1], coords f64 [P][6], attach int32 [P][6] (-1: no pointer);
 *   index int32 [B]: the drawing of each batch row (outside [0, N): the empty drawing);
 *   S = MAX_INPUT_LENGTH - 1, T = MAX_OUTPUT_LENGTH, n_bits <= 11 (PA_ESHAPE beyond); END / PAD tokens, vocab size;
 *   outputs int64 [B][S] value / pos / coord / view / type (type NULL with with_type = 0), uint8 [B][S] mask, int64
 *   [B][T] value / label, uint8 [B][T] mask, n_tokens int32 [B] = the unmasked encoder rows of each drawing (4 per kept
 *   line + END).
 * A drawing with more than PA_TOKENISE_MAX_LINES lines, more than (S - 1) / 4 lines or more than (T - 1) / 6 planks is cut
 * there (the host rejects such data when it is loaded); coordinates must lie in [-1, 1].
 * augmentation != 0 (needs seg): the draws are counter-based - mix32 (csrc/pa_device.h) of (seed, epoch, drawing number,
 * line number, draw slot), so a drawing's tokens in an epoch do not depend on the batch it is in.  A drawing is augmented
 * when its draw is < aug_ratio; num_select is uniform in [1, min(n, ceil(n * noise_ratio))]; the selected lines are those
 * with the num_select smallest (hash, line) pairs; each is deleted (draw > 0.5), or loses noise = rint(u * noise_length *
 * 1000) / 1000 of its length at the tail (draw > 0.5) or the head, or is deleted when it is not longer than the noise.  A
 * drawing that loses every line tokenises as [END, PAD, ...]. */
#define PA_TOKENISE_MAX_LINES 1024
int pa_tokenise_drawings(const int32_t* line_off, const double* box, const double* seg, const uint8_t* view,
                         const uint8_t* type, const int32_t* plank_off, const double* coords, const int32_t* attach,
                         int32_t N, const int32_t* index, int32_t B, int32_t S, int32_t T, int32_t n_bits,
                         int32_t tok_end, int32_t tok_pad, int32_t vocab, int32_t with_type, int32_t augmentation,
                         double aug_ratio, double noise_ratio, double noise_length, uint32_t seed, uint32_t epoch,
                         int64_t* in_value, int64_t* in_pos, int64_t* in_coord, int64_t* in_view, int64_t* in_type,
                         uint8_t* in_mask, int64_t* out_value, int64_t* out_label, uint8_t* out_mask,
                         int32_t* n_tokens, void* stream);

/* ---- side-face extraction from the line drawing (csrc/sideface.h, compiled into csrc/tokenise.hip) ----
 * pa_tokenise_drawings for the sideface kind when the info files store no faces: one launch, one block of 256 threads per batch
 * element, extracts the side faces of each drawing from its two-point, axis-aligned segments and tokenises them.  Restates
 * plankassembly_amd/datasets.py `extract_sideface_flags` (reference plankassembly/datasets/sideface_data.py:22-38 centre lines of
 * the thin polygons, :41-80 sequential merge of collinear ones and flat-capped buffer, :109-135 per view 0 .. 2, :233-245
 * augmentation with the fallback to the clean drawing) for the domain of section 26, float64, every operation rounded on its own.
 * The arguments of pa_tokenise_drawings, of which box, type and in_type are not read (NULL) and with_type must be 0, seg is
 * required, and line_off / view describe the LINES of each drawing (at most PA_TOKENISE_MAX_LINES are read); then
 *   max_thickness, min_thickness, merge_tolerance: the thresholds already divided by SCALE (NaN: PA_EINVAL);
 *   faces_out f64 [B][F][4], faceviews_out uint8 [B][F], n_faces_out int32 [B] (each may be NULL), F = (S - 1) / 4: the merged
 *     boxes before quantisation in the order of the row's tokens (zero behind the drawing's count);
 *   flags_out int32 [B] (required): PA_EXTRACT_* bits.
 * Faces: per view, nodes are the distinct end points (by value), dangles are pruned, next(u -> v) turns clockwise at v from v -> u
 * (face on the left), edges with one ring on both sides are removed and the rings traced once more; a ring of positive float64
 * shoelace area (summed from its smallest half-edge; half-edge 2i / 2i + 1 = line i forward / backward) gives its bounds.
 * Candidates in the order (xmin, ymin, xmax, ymax, smallest half-edge) per view, horizontal before vertical; the reference's
 * merge, literally; boxes of width >= min_thickness.  With augmentation the lines first get the noise of pa_tokenise_drawings
 * (same draws); a drawing whose noisy lines give no box is extracted again from the clean lines (PA_EXTRACT_FELL_BACK).
 * A drawing outside the domain (a segment not axis-aligned, a coordinate not in [-1, 1], two segments of a view leaving an end
 * point in one direction) gives no box and PA_EXTRACT_OUT_OF_DOMAIN, never a fault; more than F boxes: those that sort first in
 * the row's order stay, PA_EXTRACT_TRUNCATED; a ring with |2A| < 1e-12 is dropped, PA_EXTRACT_DEGENERATE.
 * (S - 1) / 4 above PA_TOKENISE_MAX_LINES: PA_ESHAPE. */
#define PA_EXTRACT_OUT_OF_DOMAIN 1
#define PA_EXTRACT_TRUNCATED 2
#define PA_EXTRACT_FELL_BACK 4
#define PA_EXTRACT_DEGENERATE 8
int pa_tokenise_sideface_drawings(const int32_t* line_off, const double* box, const double* seg, const uint8_t* view,
                                  const uint8_t* type, const int32_t* plank_off, const double* coords, const int32_t* attach,
                                  int32_t N, const int32_t* index, int32_t B, int32_t S, int32_t T, int32_t n_bits,
                                  int32_t tok_end, int32_t tok_pad, int32_t vocab, int32_t with_type, int32_t augmentation,
                                  double aug_ratio, double noise_ratio, double noise_length, uint32_t seed, uint32_t epoch,
                                  int64_t* in_value, int64_t* in_pos, int64_t* in_coord, int64_t* in_view, int64_t* in_type,
                                  uint8_t* in_mask, int64_t* out_value, int64_t* out_label, uint8_t* out_mask,
                                  int32_t* n_tokens, double max_thickness, double min_thickness, double merge_tolerance,
                                  double* faces_out, uint8_t* faceviews_out, int32_t* n_faces_out, int32_t* flags_out,
                                  void* stream);

/* ---- the three-view line drawing from the planks (csrc/render.h, compiled into csrc/tokenise.hip) ----
 * pa_tokenise_drawings for drawings that are not stored: one launch, one block of 256 threads per batch row, renders the row's
 * planks as the reference's dataset/data_utils.py:49-205 does (build :49-60 - plank 0 skipped; project :63-101 - visible and
 * hidden edges of the three views on the projectors of :15-25, the 2D point [X, -Y] of :104-110; split_lines_on_crossing_points
 * :113-150, split_lines_on_endpoints and remove_overlapping_lines :153-205) for axis-aligned boxes seen along the axes, by the
 * definition of DESIGN.md section 27 - float64 compares only - then applies the line noise of pa_tokenise_drawings (same draws,
 * keyed by the canonical line number) and tokenises.  NOT pinned to OpenCASCADE / GEOS: the on-boundary and equal-depth
 * conventions and the orientation of the views are section 27's reading of the reference and unverified against it.
 *   plank_off int32 [N+1], coords f64 [P][6], attach int32 [P][6], index int32 [B], S, T, n_bits, tokens, vocab, with_type,
 *   augmentation .. epoch and the ten outputs in_value .. n_tokens: as pa_tokenise_drawings.  out_value / out_label / out_mask
 *   may be NULL together (no decoder rows; attach is then not read);
 *   plank_cnt int32 [N] or NULL: the planks of drawing d are plank_cnt[d] rows from plank_off[d] (NULL: up to plank_off[d + 1]);
 *   max_planks: the largest plank count of any drawing, as the host knows it; above PA_RENDER_MAX_PLANKS: PA_ESHAPE and nothing
 *     is launched.  (A row that holds more all the same is cut at the cap and flagged PA_RENDER_TRUNCATED, never a fault.)
 *   skip_first != 0: plank 0 of each drawing (the overall bounding box) is not drawn;
 *   lines_out f64 [B][F][4] (xmin ymin xmax ymax), views_out / types_out uint8 [B][F], n_lines_out int32 [B] (each may be NULL),
 *     F = (S - 1) / 4: the rendered lines before the noise, in the canonical order (view, xmin, ymin, xmax, ymax) as doubles, zero
 *     behind the row's count; type 0 visible, 1 hidden;
 *   flags_out int32 [B] (required): PA_RENDER_* bits.
 * Views: 0 (x, -z) smaller y nearer; 1 (x, -y) larger z nearer; 2 (y, -z) larger x nearer; -0.0 becomes 0.0.  Lines: the noded
 * arrangement of the near- and far-face rectangle edges of every box; a segment is hidden iff the cells on both of its sides are
 * covered by boxes whose near face is strictly nearer than the nearest edge covering it.  A coordinate that is not finite or not
 * in [-1, 1]: the row renders nothing, PA_RENDER_OUT_OF_DOMAIN; a box with lo >= hi on an axis is dropped, PA_RENDER_DEGENERATE;
 * more than F lines: those that sort first in the order of the row's tokens stay (renumbered in canonical order),
 * PA_RENDER_TRUNCATED.  A rendering with more lines than the sort keys hold (PA_TOKENISE_MAX_LINES) gets PA_RENDER_TRUNCATED |
 * PA_RENDER_OVERFLOW: the first PA_TOKENISE_MAX_LINES lines in the kernel's emission order (view, horizontal before vertical,
 * grid line, position) are taken before that cut, so the kept lines are NOT those of the defined order - the one flag that marks
 * a row whose lines the definition does not give.
 * (S - 1) / 4 above PA_TOKENISE_MAX_LINES: PA_ESHAPE. */
#define PA_RENDER_MAX_PLANKS 32
#define PA_RENDER_OUT_OF_DOMAIN 1
#define PA_RENDER_TRUNCATED 2
#define PA_RENDER_DEGENERATE 8
#define PA_RENDER_OVERFLOW 16
int pa_render_drawings(const int32_t* plank_off, const int32_t* plank_cnt, const double* coords, const int32_t* attach,
                       int32_t N, const int32_t* index, int32_t B, int32_t max_planks, int32_t skip_first, int32_t S, int32_t T,
                       int32_t n_bits, int32_t tok_end, int32_t tok_pad, int32_t vocab, int32_t with_type, int32_t augmentation,
                       double aug_ratio, double noise_ratio, double noise_length, uint32_t seed, uint32_t epoch,
                       int64_t* in_value, int64_t* in_pos, int64_t* in_coord, int64_t* in_view, int64_t* in_type,
                       uint8_t* in_mask, int64_t* out_value, int64_t* out_label, uint8_t* out_mask, int32_t* n_tokens,
                       double* lines_out, uint8_t* views_out, uint8_t* types_out, int32_t* n_lines_out, int32_t* flags_out,
                       void* stream);

/* ---- plank matching (csrc/match.hip, core csrc/match_core.h; plankassembly_amd/metric.py DevicePlankScorer) ----
 * One launch, one wave per pair: two token rows compared as sets of planks.  Restates plankassembly_amd/metric.py
 * `pairwise_iou_3d` and `HungarianMatcher` (reference third_party/matcher.py:15-27 IoU, :29-61 cost -1 where IoU > threshold
 * else 100000, assignment, TP) behind `PlankModel.parse_sequence` (reference models.py:258-265) and the trainers' box pipeline
 * (trainer_complete.py:78-80: zero-extent predictions dropped, row 0 of both sides dropped).
 *   seq_a int64 rows of len_a tokens, row r at seq_a + r * stride_a (stride in elements, >= 0); seq_b alike;
 *   pair_a / pair_b int32 [n_pairs]: pair i compares row pair_a[i] of a with row pair_b[i] of b (both NULL: rows i and i).  The
 *     rows named must exist: the kernel does not know how many there are;
 *   a row holds L / dof planks, L = the index of its first end_token (len without one); plank 0 is dropped; with filter_x != 0
 *     planks with any hi - lo == 0 are dropped (inverted planks stay); coordinates are clamped to [-32768, 32767];
 *   out int32 [n_pairs][4] = tp (the maximum matching over iou > threshold), n_a, n_b (planks left), ties (pairs with
 *     iou >= threshold && !(iou > threshold)); iou = inter / (vol_a + vol_b - inter) as one double division of exact
 *     integers, 0 where inter == 0 - the `>` and `==` decisions of metric.py bit for bit.
 * The cost being binary, tp equals the reference's TP whenever ties == 0; with ties > 0 the reference's TP depends on how scipy
 * breaks equal costs, and the caller re-scores that pair on the host (DevicePlankScorer).
 * len above PA_MATCH_MAX_LEN (170 planks a side after row 0) or dof != 6: PA_ESHAPE; threshold == 0 (the reference asserts it) or
 * NaN, a null row / out pointer, one pair list without the other, a negative stride: PA_EINVAL; a failed check launches nothing.
 * n_pairs == 0 launches nothing and returns 0. */
#define PA_MATCH_MAX_LEN 1026
int pa_plank_match(const int64_t* seq_a, int64_t stride_a, int32_t len_a, const int64_t* seq_b, int64_t stride_b, int32_t len_b,
                   const int32_t* pair_a, const int32_t* pair_b, int32_t n_pairs, int32_t end_token, int32_t dof,
                   int32_t filter_a, int32_t filter_b, double threshold, int32_t* out, void* stream);

/* ---- assembly volume (csrc/volume.hip, core csrc/volume_core.h; plankassembly_amd/metric.py plank_volume_counts) ----
 * One launch, one block of 256 threads per pair: two token rows compared as solids, the unions of their planks.  Defines the
 * counts behind shape IoU, self-overlap and the volume consensus.
 *   seq_a int64 rows of len_a tokens, row r at seq_a + r * stride_a (stride in elements, >= 0); seq_b alike, or NULL: every b
 *     side is empty and len_b / stride_b are not read (the self-overlap-only call);
 *   pair_a / pair_b int32 [n_pairs]: as for pa_plank_match (both NULL: rows i and i); the rows named must exist;
 *   a row holds L / 6 planks, L = the index of its first end_token (len without one), trailing tokens ignored; plank 0, the
 *     bounding box, is dropped; every token is clamped to [-32768, 32767]; a plank is SOLID if hi - lo > 0 on all three axes
 *     and then occupies the half-open box [lo, hi) on each; a plank with a zero or negative extent on any axis occupies
 *     nothing and is not counted (there is no filter argument);
 *   U(x) = the union of the solid planks of side x; out int64 [n_pairs][8] = union_a (the volume of U(a)), sum_a (the sum of
 *     the solid planks' own volumes), union_b, sum_b, inter (union_a + union_b - union_ab = the volume of U(a) ^ U(b)),
 *     union_ab (the volume of U(a) v U(b)), n_a, n_b (the solid planks).  Exact integers: an extent is below 2^16, a plank
 *     volume below 2^48, a sum over at most 170 planks below 2^56; for tokens of the vocabulary every value is below 2^33.
 *     With seq_b == NULL: union_b = sum_b = n_b = inter = 0 and union_ab = union_a.
 * The scores (metric.volume_scores) are one float64 division each, 0 where the denominator is 0: volume_iou = inter / union_ab,
 * volume_recall = inter / union_a (a is the ground truth), volume_precision = inter / union_b, self_overlap_x = (sum_x -
 * union_x) / sum_x.
 * dof != 6 or a len above PA_MATCH_MAX_LEN: PA_ESHAPE; a null seq_a / out, one pair list without the other, a negative stride /
 * len / n_pairs: PA_EINVAL; a failed check launches nothing.  n_pairs == 0 launches nothing and returns 0. */
int pa_plank_volume(const int64_t* seq_a, int64_t stride_a, int32_t len_a, const int64_t* seq_b, int64_t stride_b, int32_t len_b,
                    const int32_t* pair_a, const int32_t* pair_b, int32_t n_pairs, int32_t end_token, int32_t dof, int64_t* out,
                    void* stream);

/* ---- line-set overlap (csrc/overlap.hip, core csrc/overlap_core.h; plankassembly_amd/metric.py line_overlap_counts) ----
 * One launch, one block of 256 threads per pair: two encoder rows compared as sets of axis-aligned lines.  Defines the
 * reprojection score's counts; reads the encoder rows of the batch contract (plankassembly_amd/datasets.py
 * `prepare_input_sequence`; reference line_data.py:34-83 - four tokens x0 y0 x1 y1 per line, END, PAD, view and type per token),
 * as the dataset, pa_tokenise_drawings or pa_render_drawings wrote them.  Side a is the given drawing, side b the rendering.
 *   value_x / view_x / type_x int64 rows of len_x elements, row r of each at + r * stride_x (one stride per side, in elements,
 *     >= 0); type_x may be NULL (every type is 0 then); pair_a / pair_b int32 [n_pairs] as for pa_plank_match (both NULL: rows
 *     i and i); the rows named must exist;
 *   a row holds n = L / 4 lines, L = the index of its first end_token (len without one); line i has tokens value[4i .. 4i+3], the
 *     view view[4i] and the type type[4i]; x0 = min(t0, t2), x1 = max(t0, t2), y0 = min(t1, t3), y1 = max(t1, t3).  It is KEPT
 *     if the four tokens are in [0, 2^num_bits), the view is 0, 1 or 2 and it is horizontal (y0 == y1, x0 < x1: c = y0, lo = x0,
 *     hi = x1) or vertical (x0 == x1, y0 < y1: c = x0, lo = y0, hi = y1); every other line is SKIPPED and only counted;
 *   a kept line b MATCHES a kept line a of the other side if view and orientation are equal, |c_b - c_a| <= tol and, under
 *     PA_OVERLAP_MATCH, type_b == type_a (types saturate to int32 first); covered(a) = the length of [lo_a, hi_a] inside the
 *     union of [lo_b - tol, hi_b + tol] over the matching b; cov(A|B) = the sum of covered(a), len(A) = the sum of hi_a - lo_a;
 *     duplicate lines count once each.  Under PA_OVERLAP_VISIBLE only the lines of side b with type 0 take part, in both
 *     directions (the others are neither kept nor skipped) and the types of side a are not read; under PA_OVERLAP_IGNORE no type
 *     is read;
 *   out int32 [n_pairs][8] = cov(A|B), len(A), cov(B|A), len(B), kept_A, kept_B, skipped_A, skipped_B.  Integers only.
 * len / 4 above PA_TOKENISE_MAX_LINES on either side, or num_bits outside 1 .. 11: PA_ESHAPE; a null value / view / out pointer,
 * one pair list without the other, a negative stride / len / tol / n_pairs, tol above PA_OVERLAP_MAX_TOL, a mode that is none of
 * the three, PA_OVERLAP_MATCH with a null type row: PA_EINVAL; a failed check launches nothing.  n_pairs == 0 launches nothing
 * and returns 0. */
#define PA_OVERLAP_IGNORE 0
#define PA_OVERLAP_MATCH 1
#define PA_OVERLAP_VISIBLE 2
#define PA_OVERLAP_MAX_TOL 255
int pa_line_overlap(const int64_t* value_a, const int64_t* view_a, const int64_t* type_a, int64_t stride_a, int32_t len_a,
                    const int64_t* value_b, const int64_t* view_b, const int64_t* type_b, int64_t stride_b, int32_t len_b,
                    const int32_t* pair_a, const int32_t* pair_b, int32_t n_pairs, int32_t end_token, int32_t num_bits,
                    int32_t tol, int32_t type_mode, int32_t* out, void* stream);

/* ---- sequence-level training batches (csrc/seqtrain.hip; PlankModel.sequence_batch / seq_train_step) ----
 * One launch, one block per output row, grid (G, B): the N samples of each of B drawings, as the sample decoder left them in HBM
 * (pa_decode_buffers / pa_decode_sample_buffers, rows b*N + n, read in place), and the match counts of those rows against the
 * drawing's ground truth (pa_plank_match) become the teacher-forced batch of pa_model_train_fwd with one loss weight per row
 * (pa_loss_ext.weight, weight_per_token 0).  Restates plankassembly_amd/metric.py `prf_from_counts` (HungarianMatcher's
 * precision / recall / F1; reference third_party/matcher.py:57-61) and the output-sequence contract of plankassembly_amd/datasets.py
 * `prepare_output_sequence` (reference line_data.py:85-109: label = vocab_size + attach at a pointer, PAD behind END, mask = PAD).
 *   tokens / attach int64 [B*N] rows of Tmax, row r at + r * sample_stride (elements, >= 0); first_end int32 [B*N] (-1: the row never
 *     ended); scores f32 [B*N] (log-likelihood of each sample; read under objective 1 only);
 *   counts int32 [B*N][4] = tp, n_a (sample planks), n_b (ground-truth planks), ties of row b*N + n against drawing b;
 *   base_counts int32 [B][4] or NULL: the same for a greedy decode of drawing b (baseline 2);
 *   gt_value / gt_label int64 [B] rows of T, row b at + b * gt_stride; T >= Tmax;
 *   objective 0 = reinforce, 1 = risk; baseline 0 = none, 1 = mean of the others, 2 = greedy (the baseline enters objective 0 only,
 *     its argument rules hold under both); alpha (objective 1), nll_weight; vocab_size, pad_token; end_token is not read - a row is
 *     cut by first_end, never searched.
 * G = N + (nll_weight != 0) rows per drawing, row b*G + g:
 *   out_value / out_label int64 [B*G][T], out_mask uint8 [B*G][T], out_weight f32 [B*G], reward f32 [B][N].
 *   g < N, with L = first_end + 1 (Tmax for -1; clamped to Tmax): t < L: value = tokens[t], label = attach[t] >= 0 ? vocab_size +
 *     attach[t] : tokens[t], mask 0; t >= L: value = label = pad_token, mask 1.  A row that never ended trains on all Tmax tokens and
 *     has no END label.
 *   g == N (only with nll_weight != 0): value / label = the drawing's gt_value / gt_label, mask = (value == pad_token), weight =
 *     nll_weight.
 * reward[b][n] = F1 of counts[b*N + n], bit for bit prf_from_counts: prec = (f32)((f64)tp / n_a), rec = (f32)((f64)tp / n_b), 0
 *   where the denominator is 0; f1 = ((prec * rec) * 2) / ((prec + rec) + 1e-10f) in f32, every operation rounded on its own (no
 *   contraction).  tp is used as pa_plank_match reports it: pairs at IoU == threshold exactly (ties) are no edges and count for
 *   nothing, and no row is re-scored on the host - unlike DevicePlankScorer, a training reward does not chase scipy's tie-breaking.
 * out_weight[b*G + n], formed in double from the f32 rewards r_m in this order and rounded to f32 once:
 *   objective 0: w_n = (r_n - b_n) / N with b_n = 0 (baseline 0); b_n = (sum over m != n, m ascending, of r_m) / (N - 1)
 *     (baseline 1; a drawing whose rewards are all equal gets exact +0.0 weights: the sum of N - 1 <= 63 equal f32 values is exact
 *     in double); b_n = the F1 of base_counts[b] (baseline 2);
 *   objective 1: s_m = (f64)alpha * (f64)scores[m]; mx = max s_m; e_m = exp(s_m - mx); z = sum e_m (m ascending); q_m = e_m / z;
 *     A_n = sum of (q_m * (r_n - r_m)) (m ascending, each difference and product rounded) = r_n - sum_m q_m r_m without the
 *     cancellation of two nearly equal numbers - equal rewards give an exact +0.0 here too; w_n = (alpha * q_n) * A_n - minus the
 *     derivative of the expected risk sum_m q_m (1 - r_m) with respect to log p_n, as a weight on -log p_n.  Scores must be finite.
 * PA_EINVAL, nothing launched: a null pointer (base_counts may be NULL unless baseline == 2), N outside [1, PA_SEQ_MAX_SAMPLES],
 * baseline 1 with N < 2, baseline 2 without base_counts, Tmax > T, a negative B / Tmax / T / stride, objective or baseline out of range,
 * nll_weight not finite, alpha not finite or <= 0 under objective 1.  B above 65535: PA_ESHAPE.  B == 0 launches nothing and returns 0.
 * pa_seq_batch_args_bytes: sizeof(pa_seq_batch_args), for bindings to check their layout against. */
#define PA_SEQ_MAX_SAMPLES 64
typedef struct {
    const int64_t* tokens;
    const int64_t* attach;
    const int32_t* first_end;
    const float* scores;
    const int32_t* counts;
    const int32_t* base_counts;
    const int64_t* gt_value;
    const int64_t* gt_label;
    int64_t* out_value;
    int64_t* out_label;
    uint8_t* out_mask;
    float* out_weight;
    float* reward;
    int64_t sample_stride;
    int64_t gt_stride;
    int32_t B, N, Tmax, T;
    int32_t objective, baseline;
    float alpha, nll_weight;
    int32_t vocab_size, end_token, pad_token, pad_;
} pa_seq_batch_args;
int64_t pa_seq_batch_args_bytes(void);
int pa_sequence_batch(const pa_seq_batch_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
