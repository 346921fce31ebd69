// MFMA GEMM with fused epilogue for gfx950.  See include/plank_hip.h (pa_gemm).
//
// Structure (v2)
//  * 128 x 128 output tile per work unit, 256 threads = 4 waves (2 x 2), each wave 64 x 64 = 2 x 2 MFMA 32x32
//    tiles.  K tile = 128 bytes of contraction per row for bf16 (BK = 64), 64 bytes for f32 (BK = 16).
//  * PERSISTENT blocks: grid = min(#units, 2 x 256 CUs); a block walks units u = blockIdx.x, += gridDim.x and the
//    K-tile pipeline runs ACROSS unit boundaries (the first K tile of the next unit is fetched while the last one
//    of the current unit is multiplied and its epilogue runs) - the model's GEMMs have K = 512..1536, i.e. only
//    8..24 K tiles per unit, so fill/drain would otherwise dominate.
//  * XCD-aware unit order: blocks b = x (mod 8) run on XCD x; unit -> (tile_m = 8*(i / tiles_n) + x, tile_n = i %
//    tiles_n), so one XCD sweeps all column tiles of its row tiles and the activation panel stays in its L2.
//  * Operand tiles live in LDS as [row][k] images (k contiguous), 16-byte chunks XOR-swizzled by row.
//    k-contiguous operands are fetched with global_load_lds (direct-to-LDS DMA, no VGPR round trip; the LDS image
//    is lane-linear, so the swizzle is applied to the per-lane SOURCE address).  Operands whose contraction index is
//    strided in memory (dX = dY W, dW = dY^T X) go global -> registers -> EB x EB in-register transpose -> LDS.
//  * MFMA operands are SWAPPED (A := weight-side rows, B := activation-side rows), so a lane owns 4 consecutive
//    output columns of one output row; the epilogue stages each wave's 64 x 64 sub-tile through its own LDS slice
//    and writes whole 128/256-byte row segments with 8/16-byte vector stores (bias / ReLU / ReLU-backward gate /
//    dropout / residual applied on the way).
#include <stdlib.h>
#include <climits>
#include <atomic>
#include <new>
#include <mutex>
#include <vector>
#include <type_traits>
#include <utility>
#include "pa_device.h"
#include <mutex>
#include <vector>
#include "../../include/plank_hip.h"
#include "gemm_common.h"

namespace {

constexpr int BM = 128, BN = 128, NT = 256;
__device__ __attribute__((aligned(16))) const uint32_t pa_zero16[4] = {0u, 0u, 0u, 0u};   // source of out-of-range DMA lanes
typedef short s16x4 __attribute__((ext_vector_type(4)));

#ifdef PA_GEMM_TRACE
// cycle trace of block 0 / thread 0: timestamps go to LDS (cheap, no memory round trip) and are flushed at kernel end
__device__ unsigned long long pa_trace[8192];
__device__ int pa_trace_n;
#define TR_DECL __shared__ unsigned long long tr_lds[1024]; int tr_n = 0
#define TR(tag) do { if (blockIdx.x == 0 && threadIdx.x == 0 && tr_n < 1022) { tr_lds[tr_n++] = (unsigned long long)(tag); tr_lds[tr_n++] = __builtin_amdgcn_s_memtime(); } } while (0)
#define TR_FLUSH do { if (blockIdx.x == 0 && threadIdx.x == 0) { for (int i_ = 0; i_ < tr_n; ++i_) pa_trace[i_] = tr_lds[i_]; pa_trace_n = tr_n; } } while (0)
#else
#define TR_DECL do {} while (0)
#define TR(tag) do {} while (0)
#define TR_FLUSH do {} while (0)
#endif

// BK_ = contraction elements per K tile.  bf16: 64 (128-byte rows) or 32 (64-byte rows, half the LDS -> more blocks/CU)
template <typename T, int BK_> struct Tile {
    static constexpr int EB = ET<T>::EB;
    static constexpr int BK = BK_;
    static constexpr int RB = BK * sizeof(T);        // bytes per LDS row (128 / 64)
    static constexpr int NCH = RB / 16;              // 16-byte chunks per row (8 / 4)
    static constexpr int RPB = 256 / RB;             // rows per 256-byte bank row (2 / 4)
    static constexpr int STEPS = BK / ET<T>::KC;     // mma16B steps per K tile
    static constexpr int NLD = BM * NCH / NT;        // 16-byte chunks per thread, k-contiguous
    static constexpr int TILE_BYTES = BM * RB;       // per operand
    static constexpr int STAGE_BYTES = TILE_BYTES / 2;   // per-wave epilogue staging slice
    static constexpr int RPP = STAGE_BYTES / 256;    // output rows per staging pass
    static constexpr int KB = BK / EB;               // EB-wide k blocks per tile (transposed staging)
    static constexpr int NTB = (BM / EB) * KB;       // EB x EB blocks per transposed tile
    static constexpr int NTR = (NTB + 127) / 128;    // blocks per thread of the 128-thread half
};

template <typename TL> __device__ __forceinline__ int lds_off(int row, int chunk) {
    return row * TL::RB + (((chunk ^ (row / TL::RPB)) & (TL::NCH - 1)) << 4);
}


template <typename TL>
__device__ __forceinline__ bool decode_unit(const GemmP& p, int u, Unit& un) {
    if (u >= p.units) return false;
    const int per_z = p.tiles_m_pad * p.tiles_n;
    un.z = u / per_z;
    const int r = u - un.z * per_z;
    if (p.plain_order) {                                           // small / grouped problem: plain order, every unit valid
        un.tile_m = r / p.tiles_n;
        un.tile_n = r - un.tile_m * p.tiles_n;
    } else {
        const int xcd = r & 7, i = r >> 3;
        const int q = i / p.tiles_n;
        un.tile_n = i - q * p.tiles_n;
        un.tile_m = q * 8 + xcd;
    }
    un.b = un.z / p.splitk;
    const int slice = un.z - un.b * p.splitk;
    const int nt_total = (p.K + TL::BK - 1) / TL::BK;
    un.t_begin = slice * p.tiles_per_slice;
    un.t_end = min(nt_total, un.t_begin + p.tiles_per_slice);
    return (un.tile_m < p.tiles_m) && (un.t_begin < un.t_end);
}
__device__ __forceinline__ int next_valid_unit(int u, int stride) { return u + stride; }

// GLDS: direct-to-LDS loads for the k-contiguous operands (requires ALIGNED and K % BK == 0).
// TRG (bf16): operands whose contraction index is strided in memory are DMA'd into LDS in their NATURAL layout
//   ([k][row], 256-byte rows, 64-byte units XOR-swizzled by k&3) and the MFMA fragments are formed by
//   ds_read_b64_tr_b16 (in each 16-lane group lane L supplies row L>>2 / column 4*(L&3) of a 4 x 16 patch and
//   lane i receives column i) - no register transposes, no staging VGPRs.  Lanes whose k is past K read zeros.
// NST: LDS pipeline stages.  3 is only available when both operands are DMA'd: tile i+2 is in flight while tile i
//   is multiplied, synchronised with counted s_waitcnt vmcnt + raw s_barrier (a __syncthreads() would drain the DMA
//   queue).  Used for small problems (one block per CU anyway), where every K tile would otherwise pay a full
//   memory round trip.
// EPRE: the launch has bf16 residual or gate rows and a bf16 output - fetch them under the last K tile (prefetch_epi below).  Its own
//   instantiation because the 16 extra registers spill a few dwords (the kernel sits at 244 of 256): launches without such rows
//   keep the unspilled code.
template <typename T, int BK_, int OCC, bool A_KC, bool B_KC, bool ALIGNED, bool GLDS, bool TRG, int NST, bool EPRE = false>
__global__ __launch_bounds__(NT, OCC) void gemm_kernel(GemmP p) {
    using TL = Tile<T, BK_>;
    constexpr int EB = TL::EB;
    constexpr int SMEM = NST * 2 * TL::TILE_BYTES;      // NST == 1: 32 KiB -> four blocks per CU hide each other's latencies
    __shared__ __attribute__((aligned(256))) char smem[SMEM];   // [buf][A|B]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5;
    constexpr int esz = (int)sizeof(T);
    TR_DECL;
    TR(0);

    f32x16 acc[2][2];            // [tn][tm]  (operands swapped: rows of D = weight-side index n)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    constexpr bool A_GL = A_KC && GLDS, B_GL = B_KC && GLDS;
    constexpr bool A_TG = !A_KC && TRG, B_TG = !B_KC && TRG;
    constexpr bool ALL_DMA = (A_GL || A_TG) && (B_GL || B_TG);
    static_assert(NST == 2 || ((NST == 3 || NST == 1) && ALL_DMA), "1- and 3-stage variants need both operands DMA'd");
    static_assert(!TRG || (sizeof(T) == 2 && BK_ == 64), "transposing LDS reads: bf16, 64-deep K tile");
    constexpr int NRA = (A_GL || A_TG) ? 1 : (A_KC ? TL::NLD : TL::NTR * EB);
    constexpr int NRB = (B_GL || B_TG) ? 1 : (B_KC ? TL::NLD : TL::NTR * EB);
    u32x4 ra[NRA], rb[NRB];
    // both operands register-transposed (exact f32, contraction index strided in both - the weight gradients): ONE staging array, the
    // thread's role selects addresses instead of guarding the loads (a load inside `if (role)` is a masked definition hipcc merges
    // with v_mov copies of the freshly loaded registers - a wait right behind every load; round 6)
    constexpr bool BOTH_TR = !A_KC && !B_KC && !TRG;
    const bool a_role = A_KC || (tid < 128);
    const bool b_role = B_KC || (tid >= 128);
    const int t128 = tid & 127;

    // ---- per-unit addressing state (hoisted out of the K loop) ------------------------------------------
    // k-contiguous operand: chunk p = tid + i*NT -> (row, source chunk); byte offset of its row start (clamped)
    uint32_t offA[TL::NLD], offB[TL::NLD];
    bool okA[TL::NLD], okB[TL::NLD];                 // register path: row inside the matrix
    const char* baseA = nullptr; const char* baseB = nullptr;
    auto setup = [&](const Unit& un) {
        baseA = reinterpret_cast<const char*>(p.A) + (size_t)un.b * p.sA * esz;
        baseB = reinterpret_cast<const char*>(p.B) + (size_t)un.b * p.sB * esz;
        const int m0 = un.tile_m * BM, n0 = un.tile_n * BN;
        if constexpr (A_KC) {
#pragma unroll
            for (int i = 0; i < TL::NLD; ++i) {
                const int pidx = tid + i * NT, row = pidx / TL::NCH;
                const int ch = A_GL ? (((pidx % TL::NCH) ^ (row / TL::RPB)) & (TL::NCH - 1)) : (pidx % TL::NCH);
                okA[i] = (m0 + row) < p.M;
                offA[i] = (uint32_t)min(m0 + row, p.M - 1) * (uint32_t)(p.lda * esz) + ch * 16;
            }
        }
        if constexpr (B_KC) {
#pragma unroll
            for (int i = 0; i < TL::NLD; ++i) {
                const int pidx = tid + i * NT, row = pidx / TL::NCH;
                const int ch = B_GL ? (((pidx % TL::NCH) ^ (row / TL::RPB)) & (TL::NCH - 1)) : (pidx % TL::NCH);
                okB[i] = (n0 + row) < p.N;
                offB[i] = (uint32_t)min(n0 + row, p.N - 1) * (uint32_t)(p.ldb * esz) + ch * 16;
            }
        }
        // natural image: LDS chunk pidx = (k row = pidx >> 4, position = pidx & 15) holds source chunk pos ^ ((row & 3) << 2)
        if constexpr (A_TG) {
#pragma unroll
            for (int i = 0; i < TL::NLD; ++i) {
                const int pidx = tid + i * NT, row = pidx >> 4;
                const int col = m0 + (((pidx & 15) ^ ((row & 3) << 2)) << 3);
                okA[i] = col < p.M;
                offA[i] = (uint32_t)row * (uint32_t)(p.lda * esz) + (uint32_t)col * esz;
            }
        }
        if constexpr (B_TG) {
#pragma unroll
            for (int i = 0; i < TL::NLD; ++i) {
                const int pidx = tid + i * NT, row = pidx >> 4;
                const int col = n0 + (((pidx & 15) ^ ((row & 3) << 2)) << 3);
                okB[i] = col < p.N;
                offB[i] = (uint32_t)row * (uint32_t)(p.ldb * esz) + (uint32_t)col * esz;
            }
        }
    };

    // transposed operand: element (r, k) at base[k * ld + r]; EB x EB blocks, 128 threads per operand
    auto load_tr = [&](u32x4* regs, const char* base, int ld, int r0, int nrows, int k0) {
        constexpr int RBLK = BM / EB;
#pragma unroll
        for (int j = 0; j < TL::NTR; ++j) {
            const int blk = t128 + j * 128;
            const int rbk = blk % RBLK, kb = blk / RBLK;
            const int r = r0 + rbk * EB;
#pragma unroll
            for (int i = 0; i < EB; ++i) {
                const int k = k0 + kb * EB + i;
                u32x4 v = {0u, 0u, 0u, 0u};
                if constexpr (ALIGNED) {
                    // unconditional load on a clamped (k, r) - zeroed in store_tr, at the END of the overlapped tile: a load inside
                    // `if (in range)` (or a select right behind it) makes hipcc wait for it on the spot, and this "prefetch" of the
                    // next K tile was a synchronous load in front of the tile's MFMAs (round 6, read in the ISA; the exact-f32
                    // weight-gradient GEMMs run here)
                    const T* src = reinterpret_cast<const T*>(base) + (size_t)min(k, p.K - 1) * ld + min(r, (nrows - 1) / EB * EB);   // (the last vector may straddle nrows: the stride covers it, is_aligned)
                    v = *reinterpret_cast<const u32x4*>(src);
                } else if (blk < TL::NTB && k < p.K) {
                    const T* src = reinterpret_cast<const T*>(base) + (size_t)k * ld + r;
                    {
                        T tmp[EB];
#pragma unroll
                        for (int e = 0; e < EB; ++e) tmp[e] = (r + e < nrows) ? src[e] : (T)0.0f;
                        v = *reinterpret_cast<u32x4*>(tmp);
                    }
                }
                regs[j * EB + i] = v;
            }
        }
    };
    int tr_k0 = 0, tr_rA0 = 0, tr_rB0 = 0;      // (k, row) origin of the tile held in ra / rb (set by fetch, used by store_tr's zeroing)
    auto store_tr = [&](const u32x4* regs_in, char* lds, int r0, int nrows) {
        constexpr int RBLK = BM / EB;
#pragma unroll
        for (int j = 0; j < TL::NTR; ++j) {
            const int blk = t128 + j * 128;
            if (blk < TL::NTB) {
                const int rbk = blk % RBLK, kb = blk / RBLK;
                u32x4 regs_m[EB];
                const u32x4* regs = regs_in + j * EB;
                if constexpr (ALIGNED) {
                    const bool rin = r0 + rbk * EB < nrows;
#pragma unroll
                    for (int i = 0; i < EB; ++i) regs_m[i] = (rin && tr_k0 + kb * EB + i < p.K) ? regs[i] : u32x4{0u, 0u, 0u, 0u};
                    regs = regs_m;
                }
                u32x4 tr[EB];
                transpose_block<T>(regs, tr);
#pragma unroll
                for (int e = 0; e < EB; ++e)
                    *reinterpret_cast<u32x4*>(lds + lds_off<TL>(rbk * EB + e, kb)) = tr[e];
            }
        }
    };

    // phase 1 of a tile fetch: issue global loads (DMA straight into `buf`, or into registers)
    auto fetch = [&](const Unit& un, int t, int buf) {
        const int k0 = t * TL::BK;
        tr_k0 = k0; tr_rA0 = un.tile_m * BM; tr_rB0 = un.tile_n * BN;
        char* la = smem + buf * 2 * TL::TILE_BYTES;
        char* lb = la + TL::TILE_BYTES;
        const char* ka = baseA + (size_t)k0 * esz;          // wave-uniform
        const char* kb = baseB + (size_t)k0 * esz;
        if constexpr (A_GL) {
#pragma unroll
            for (int i = 0; i < TL::NLD; ++i)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ka + offA[i]),
                    (__attribute__((address_space(3))) void*)(la + (i * NT + wave * 64) * 16), 16, 0, 0);
        } else if constexpr (A_KC) {
#pragma unroll
            for (int i = 0; i < TL::NLD; ++i) {
                const int kk = k0 + ((tid + i * NT) % TL::NCH) * EB;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (okA[i]) {
                    const T* src = reinterpret_cast<const T*>(ka + offA[i]);
                    if (ALIGNED) { if (kk < p.K) v = *reinterpret_cast<const u32x4*>(src); }
                    else {
                        T tmp[EB];
#pragma unroll
                        for (int e = 0; e < EB; ++e) tmp[e] = (kk + e < p.K) ? src[e] : (T)0.0f;
                        v = *reinterpret_cast<u32x4*>(tmp);
                    }
                }
                ra[i] = v;
            }
        } else if constexpr (A_TG) {
            const char* kra = baseA + (size_t)k0 * p.lda * esz;            // wave-uniform: first k row of the tile
#pragma unroll
            for (int i = 0; i < TL::NLD; ++i) {
                const bool in = okA[i] && (k0 + ((tid + i * NT) >> 4)) < p.K;
                const char* src = in ? kra + offA[i] : reinterpret_cast<const char*>(pa_zero16);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                    (__attribute__((address_space(3))) void*)(la + (i * NT + wave * 64) * 16), 16, 0, 0);
            }
        } else if constexpr (BOTH_TR) { load_tr(ra, tid < 128 ? baseA : baseB, tid < 128 ? p.lda : p.ldb, tid < 128 ? un.tile_m * BM : un.tile_n * BN, tid < 128 ? p.M : p.N, k0); }
        else { if (a_role) load_tr(ra, baseA, p.lda, un.tile_m * BM, p.M, k0); }
        if constexpr (B_GL) {
#pragma unroll
            for (int i = 0; i < TL::NLD; ++i)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kb + offB[i]),
                    (__attribute__((address_space(3))) void*)(lb + (i * NT + wave * 64) * 16), 16, 0, 0);
        } else if constexpr (B_KC) {
#pragma unroll
            for (int i = 0; i < TL::NLD; ++i) {
                const int kk = k0 + ((tid + i * NT) % TL::NCH) * EB;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (okB[i]) {
                    const T* src = reinterpret_cast<const T*>(kb + offB[i]);
                    if (ALIGNED) { if (kk < p.K) v = *reinterpret_cast<const u32x4*>(src); }
                    else {
                        T tmp[EB];
#pragma unroll
                        for (int e = 0; e < EB; ++e) tmp[e] = (kk + e < p.K) ? src[e] : (T)0.0f;
                        v = *reinterpret_cast<u32x4*>(tmp);
                    }
                }
                rb[i] = v;
            }
        } else if constexpr (B_TG) {
            const char* krb = baseB + (size_t)k0 * p.ldb * esz;
#pragma unroll
            for (int i = 0; i < TL::NLD; ++i) {
                const bool in = okB[i] && (k0 + ((tid + i * NT) >> 4)) < p.K;
                const char* src = in ? krb + offB[i] : reinterpret_cast<const char*>(pa_zero16);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                    (__attribute__((address_space(3))) void*)(lb + (i * NT + wave * 64) * 16), 16, 0, 0);
            }
        } else if constexpr (BOTH_TR) { /* loaded with A above */ }
        else { if (b_role) load_tr(rb, baseB, p.ldb, un.tile_n * BN, p.N, k0); }
    };
    // phase 2: registers -> LDS (nothing to do for DMA'd operands)
    auto commit = [&](int buf) {
        char* la = smem + buf * 2 * TL::TILE_BYTES;
        char* lb = la + TL::TILE_BYTES;
        if constexpr (!A_GL && !A_TG) {
            if constexpr (A_KC) {
#pragma unroll
                for (int i = 0; i < TL::NLD; ++i) {
                    const int c = tid + i * NT;
                    *reinterpret_cast<u32x4*>(la + lds_off<TL>(c / TL::NCH, c % TL::NCH)) = ra[i];
                }
            } else if constexpr (BOTH_TR) { store_tr(ra, tid < 128 ? la : lb, tid < 128 ? tr_rA0 : tr_rB0, tid < 128 ? p.M : p.N); }
            else { if (a_role) store_tr(ra, la, tr_rA0, p.M); }
        }
        if constexpr (!B_GL && !B_TG) {
            if constexpr (B_KC) {
#pragma unroll
                for (int i = 0; i < TL::NLD; ++i) {
                    const int c = tid + i * NT;
                    *reinterpret_cast<u32x4*>(lb + lds_off<TL>(c / TL::NCH, c % TL::NCH)) = rb[i];
                }
            } else if constexpr (BOTH_TR) { /* stored with A above */ }
            else { if (b_role) store_tr(rb, lb, tr_rB0, p.N); }
        }
    };

    // bias of this lane's 4 output columns, fetched at unit start so the epilogue does not open with a dependent load
    f32x4 ubias = {0.f, 0.f, 0.f, 0.f};
    auto load_bias = [&](const Unit& un) {
        ubias = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.bias && p.splitk == 1) {
            const int n = un.tile_n * BN + wn * 64 + (lane & 15) * 4;
            const float* bp = p.bias + (size_t)un.b * p.sBias;
            if (p.vec_ok && n + 3 < p.N) ubias = *reinterpret_cast<const f32x4*>(bp + n);
            else { for (int e = 0; e < 4; ++e) if (n + e < p.N) ubias[e] = bp[n + e]; }
        }
    };

    // ---- residual / gate rows of a unit's epilogue, fetched while its LAST K tile is multiplied (two-stage variant, bf16 in and
    // out, interior column block).  The epilogue's two staging passes each used to wait one memory round trip for eight
    // 8-byte loads per lane.  The kernel already holds 244 of its 256 registers: only the first pass's rows (16 registers,
    // bf16 pairs) are fetched under the K tile, the second pass's when the epilogue starts (the fragments are dead by then).  Figures at the launch site (launch_t).
    u32x2 pepi[8];
    int pre_kind = 0;                     // 0 nothing prefetched, 1 residual rows, 2 gate rows (residual wins when a launch has both)
    const char* pre_base = nullptr;
    uint32_t pre_ld2 = 0;
    // rows [i0 * 4, i0 * 4 + 32) of this wave's 64 x 64 block: eight 8-byte loads per lane
    auto load_epi_rows = [&](u32x2 (&dst)[8], const Unit& un, int i0) {
        const int mw = un.tile_m * BM + wm * 64, n = un.tile_n * BN + wn * 64 + (lane & 15) * 4, rsub = lane >> 4;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            dst[i] = *reinterpret_cast<const u32x2*>(pre_base + ((uint32_t)min(mw + (i0 + i) * 4 + rsub, p.M - 1) * pre_ld2 + (uint32_t)n * 2u));
    };
    auto prefetch_epi = [&](const Unit& un) {
        pre_kind = 0;
        if constexpr (EPRE && sizeof(T) == 2 && TL::RPP * 2 == 64 && ALL_DMA && NST == 2) {
            if (p.splitk > 1 || p.out_dtype == PA_F32 || (p.R == nullptr && p.aux == nullptr)) return;
            if (!(p.vec_ok && un.tile_n * BN + wn * 64 + 64 <= p.N)) return;     // (wave-uniform)
            const bool use_r = p.R != nullptr;
            pre_kind = use_r ? 1 : 2;
            pre_base = use_r ? reinterpret_cast<const char*>(p.R) + (size_t)un.b * p.sR * 2
                             : reinterpret_cast<const char*>(p.aux) + (size_t)un.b * p.sAux * 2;
            pre_ld2 = (uint32_t)(use_r ? p.ldr : p.ldaux) * 2u;
            load_epi_rows(pepi, un, 0);           // the first staging pass's rows now; the second pass's at the start of the epilogue
        }
    };
    auto widen2 = [](const u32x2& u) { f32x4 r; r[0] = bf16_lo(u[0]); r[1] = bf16_hi(u[0]); r[2] = bf16_lo(u[1]); r[3] = bf16_hi(u[1]); return r; };

    // ---- epilogue of one unit: per-wave LDS staging, batched loads, vector row stores -------------------------
    auto epilogue = [&](const Unit& un, int buf) {
        char* stage = smem + buf * 2 * TL::TILE_BYTES + wave * TL::STAGE_BYTES;
        const bool slab = p.splitk > 1;
        const size_t cbase = slab ? (size_t)un.z * p.M * p.ldc : (size_t)un.b * p.sC;
        const int mw = un.tile_m * BM + wm * 64, nw = un.tile_n * BN + wn * 64;
        const int chunk = lane & 15, rsub = lane >> 4;
        const int n = nw + chunk * 4;                                     // this lane's 4 output columns (all rows)
        const bool colv = n < p.N;
        const bool full = p.vec_ok && (n + 3 < p.N);                      // vector path for this lane
        const bool fast = p.vec_ok && (nw + 64 <= p.N);                   // wave-uniform: whole column block interior
        const bool out_f32 = slab || p.out_dtype == PA_F32;
        const bool has_bias = !slab && p.bias != nullptr, has_aux = !slab && p.aux != nullptr;
        const bool has_res = !slab && p.R != nullptr, has_drop = !slab && p.drop_thr != 0;
        const f32x4 bias = has_bias ? ubias : f32x4{0.f, 0.f, 0.f, 0.f};   // fetched when the unit started (load_bias)
        const float alpha = slab ? 1.f : p.alpha;
        constexpr int NPASS = 64 / TL::RPP, NIT = TL::RPP / 4;
        u32x2 pepi1[8];
        if (pre_kind) load_epi_rows(pepi1, un, 8);                        // in flight behind the first pass
        // (static_for: the prefetched residual / gate registers are indexed by the pass - a rolled loop would put them in scratch)
        static_for<0, NPASS>([&](auto P_) {
            constexpr int pass = decltype(P_)::value;
            const int tm = (pass * TL::RPP) / 32;
            const int rsel = (pass * TL::RPP) % 32;
            const int lrow = (lane & 31) - rsel;
            if (lrow >= 0 && lrow < TL::RPP) {
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = acc[tn][tm][4 * g4 + e];
                        const int ch = (tn * 32 + 8 * g4 + 4 * half) >> 2;
                        *reinterpret_cast<f32x4*>(stage + lrow * 256 + ((ch ^ (lrow & 15)) << 4)) = v;
                    }
            }
            TR(20);
            if (fast) {
                // Interior column block, vector-aligned: straight-line code.  Row validity only predicates the final
                // stores (loads use a clamped row), so the single wait for the batched residual / gate loads is the
                // only s_waitcnt vmcnt of the pass and the stores go out back to back.
                f32x4 x[NIT];
                const int mp = mw + pass * TL::RPP + rsub;
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int lr = it * 4 + rsub;
                    x[it] = *reinterpret_cast<const f32x4*>(stage + lr * 256 + ((chunk ^ (lr & 15)) << 4));
                }
                f32x4 res[NIT], gate[NIT];
                if (has_res) {
                    if (pre_kind == 1) {                                  // fetched during the last K tile (prefetch_epi)
#pragma unroll
                        for (int it = 0; it < NIT; ++it) res[it] = widen2(pass == 0 ? pepi[it & 7] : pepi1[it & 7]);
                    } else {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) {
                            const size_t ro = (size_t)un.b * p.sR + (size_t)min(mp + it * 4, p.M - 1) * p.ldr + n;
                            res[it] = out_f32 ? ld4<float>(reinterpret_cast<const float*>(p.R) + ro)
                                              : ld4<bf16>(reinterpret_cast<const bf16*>(p.R) + ro);
                        }
                    }
                }
                if (has_aux) {
                    if (pre_kind == 2) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) gate[it] = widen2(pass == 0 ? pepi[it & 7] : pepi1[it & 7]);
                    } else {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) {
                            const size_t ao = (size_t)un.b * p.sAux + (size_t)min(mp + it * 4, p.M - 1) * p.ldaux + n;
                            gate[it] = ld4<T>(reinterpret_cast<const T*>(p.aux) + ao);
                        }
                    }
                }
                if (!slab) {
                    // one straight-line loop per optional stage behind its own uniform branch (see gemm3_kernel)
#pragma unroll
                    for (int it = 0; it < NIT; ++it)
#pragma unroll
                        for (int e = 0; e < 4; ++e) x[it][e] = x[it][e] * alpha + bias[e];
                    if (p.relu) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it)
#pragma unroll
                            for (int e = 0; e < 4; ++e) x[it][e] = fmaxf(x[it][e], 0.f);
                    }
                    if (has_aux) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it)
#pragma unroll
                            for (int e = 0; e < 4; ++e) x[it][e] = gate[it][e] > 0.f ? x[it][e] * p.aux_scale : 0.f;
                    }
                    if (has_drop) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                x[it][e] = drop_keep_rc(p.drop_seed, (uint32_t)(un.b * p.M + mp + it * 4), (uint32_t)(n + e), p.drop_thr) ? x[it][e] * p.drop_scale : 0.f;
                            }
                    }
                    if (has_res) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it)
#pragma unroll
                            for (int e = 0; e < 4; ++e) x[it][e] += res[it][e];
                    }
                }
                TR(23);
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int m = mp + it * 4;
                    if (m < p.M) {
                        const size_t co = cbase + (size_t)m * p.ldc + n;
                        if (out_f32) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + co) = x[it];
                        else st4<bf16>(reinterpret_cast<bf16*>(p.C) + co, x[it]);
                    }
                }
                return;
            }
            f32x4 v[NIT], res[NIT], gate[NIT];
            bool rowv[NIT];
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int lr = it * 4 + rsub;
                v[it] = *reinterpret_cast<const f32x4*>(stage + lr * 256 + ((chunk ^ (lr & 15)) << 4));
                rowv[it] = colv && (mw + pass * TL::RPP + lr) < p.M;
            }
            if (has_res) {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    res[it] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (rowv[it]) {
                        const int m = mw + pass * TL::RPP + it * 4 + rsub;
                        const size_t ro = (size_t)un.b * p.sR + (size_t)m * p.ldr + n;
                        if (full) res[it] = out_f32 ? ld4<float>(reinterpret_cast<const float*>(p.R) + ro)
                                                    : ld4<bf16>(reinterpret_cast<const bf16*>(p.R) + ro);
                        else { for (int e = 0; e < 4; ++e) if (n + e < p.N)
                                   res[it][e] = out_f32 ? reinterpret_cast<const float*>(p.R)[ro + e]
                                                        : (float)reinterpret_cast<const bf16*>(p.R)[ro + e]; }
                    }
                }
            }
            if (has_aux) {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    gate[it] = f32x4{1.f, 1.f, 1.f, 1.f};
                    if (rowv[it]) {
                        const int m = mw + pass * TL::RPP + it * 4 + rsub;
                        const size_t ao = (size_t)un.b * p.sAux + (size_t)m * p.ldaux + n;
                        if (full) gate[it] = ld4<T>(reinterpret_cast<const T*>(p.aux) + ao);
                        else { for (int e = 0; e < 4; ++e) if (n + e < p.N) gate[it][e] = ld1(reinterpret_cast<const T*>(p.aux) + ao + e); }
                    }
                }
            }
            // phase A: finish the arithmetic of the whole pass (this is the single point where the batched residual /
            // gate loads are waited for) ...
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!slab) {
                    const int m = mw + pass * TL::RPP + it * 4 + rsub;
                    f32x4 x = v[it];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float y = x[e] * alpha + bias[e];
                        if (p.relu) y = fmaxf(y, 0.f);
                        if (has_aux) y = gate[it][e] > 0.f ? y * p.aux_scale : 0.f;
                        if (has_drop) {
                            y = drop_keep_rc(p.drop_seed, (uint32_t)(un.b * p.M + m), (uint32_t)(n + e), p.drop_thr) ? y * p.drop_scale : 0.f;
                        }
                        if (has_res) y += res[it][e];
                        x[e] = y;
                    }
                    v[it] = x;
                }
            }
            // ... phase B: nothing but stores, so no s_waitcnt lands between them (a wait here would also drain the
            // stores already issued: one full write round trip per row group)
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!rowv[it]) continue;
                const int m = mw + pass * TL::RPP + it * 4 + rsub;
                const f32x4 x = v[it];
                const size_t co = cbase + (size_t)m * p.ldc + n;
                if (out_f32) {
                    float* cp = reinterpret_cast<float*>(p.C) + co;
                    if (full) *reinterpret_cast<f32x4*>(cp) = x;
                    else { for (int e = 0; e < 4; ++e) if (n + e < p.N) cp[e] = x[e]; }
                } else {
                    bf16* cp = reinterpret_cast<bf16*>(p.C) + co;
                    if (full) st4<bf16>(cp, x);
                    else { for (int e = 0; e < 4; ++e) if (n + e < p.N) cp[e] = (bf16)x[e]; }
                }
            }
        });
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    };

    // ---- persistent, cross-unit software pipeline ----------------------------------------------------------
    const int ustride = gridDim.x;
    const int arow = wm * 64 + (lane & 31), brow = wn * 64 + (lane & 31);
    // transposing reads: lane-constant byte offset of fragment group i inside the natural image (k row 8*half + (L>>2),
    // column window + 16*(G&1) + 4*(L&3); 64-byte units XOR-swizzled by the k row & 3 = (L>>2)&3)
    int trA[2] = {0, 0}, trB[2] = {0, 0};
    {
        const int L = lane & 15, G = lane >> 4, kr = 8 * half + (L >> 2);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ca = (wm * 64 + i * 32 + 16 * (G & 1) + 4 * (L & 3)) * 2, cb = (wn * 64 + i * 32 + 16 * (G & 1) + 4 * (L & 3)) * 2;
            trA[i] = kr * 256 + ((((ca >> 6) ^ ((L >> 2) & 3)) << 6) | (ca & 63));
            trB[i] = kr * 256 + ((((cb >> 6) ^ ((L >> 2) & 3)) << 6) | (cb & 63));
        }
    }
    // multiply the K tile held in LDS stage `buf` into the accumulators
    auto compute = [&](int buf) {
        const char* la = smem + buf * 2 * TL::TILE_BYTES;
        const char* lb = la + TL::TILE_BYTES;
        auto ldA = [&](int s, int i) -> u32x4 {
            if constexpr (A_TG) {
                const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(la + trA[i] + s * 4096));
                const s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(la + trA[i] + s * 4096 + 1024));
                u32x4 f; const u32x2 a0 = *reinterpret_cast<const u32x2*>(&x0), a1 = *reinterpret_cast<const u32x2*>(&x1);
                f[0] = a0[0]; f[1] = a0[1]; f[2] = a1[0]; f[3] = a1[1];
                return f;
            } else {
                return *reinterpret_cast<const u32x4*>(la + lds_off<TL>(arow + i * 32, 2 * s + half));
            }
        };
        auto ldB = [&](int s, int i) -> u32x4 {
            if constexpr (B_TG) {
                const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lb + trB[i] + s * 4096));
                const s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lb + trB[i] + s * 4096 + 1024));
                u32x4 f; const u32x2 b0 = *reinterpret_cast<const u32x2*>(&x0), b1 = *reinterpret_cast<const u32x2*>(&x1);
                f[0] = b0[0]; f[1] = b0[1]; f[2] = b1[0]; f[3] = b1[1];
                return f;
            } else {
                return *reinterpret_cast<const u32x4*>(lb + lds_off<TL>(brow + i * 32, 2 * s + half));
            }
        };
        if constexpr (ALL_DMA && NST != 1) {
            // all fragment reads of the tile are issued up front; LDS returns in order, so the MFMAs of step s start
            // as soon as their vectors have landed while the later ones are still in flight
            u32x4 fa[TL::STEPS][2], fb[TL::STEPS][2];
#pragma unroll
            for (int s = 0; s < TL::STEPS; ++s)
#pragma unroll
                for (int i = 0; i < 2; ++i) { fa[s][i] = ldA(s, i); fb[s][i] = ldB(s, i); }
            __builtin_amdgcn_sched_barrier(0);   // keep all reads ahead of the MFMAs (the scheduler would otherwise re-serialise them)
#pragma unroll
            for (int s = 0; s < TL::STEPS; ++s)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm) mma16B<T>(acc[tn][tm], fb[s][tn], fa[s][tm]);
        } else {
            // staging registers are live in these variants: keep the fragment footprint to one step
#pragma unroll
            for (int s = 0; s < TL::STEPS; ++s) {
                u32x4 fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) { fa[i] = ldA(s, i); fb[i] = ldB(s, i); }
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm) mma16B<T>(acc[tn][tm], fb[tn], fa[tm]);
            }
        }
    };
    // first valid unit at or after u
    auto seek = [&](int u, Unit& un) -> int {
        bool ok = decode_unit<TL>(p, u, un);
        while (u < p.units && !ok) { u += ustride; ok = decode_unit<TL>(p, u, un); }
        return u;
    };

    if constexpr (NST == 2) {
        Unit cur, nxt;
        int u = seek(blockIdx.x, cur);
        if (u >= p.units) return;
        int nu = seek(u + ustride, nxt);                    // the unit after `cur` (decoded once per unit)
        int t = cur.t_begin, buf = 0;
        setup(cur);
        load_bias(cur);
        fetch(cur, t, 0);
        commit(0);
        __syncthreads();
        while (true) {
            const bool last_k = (t + 1 >= cur.t_end);
            const bool has_next = !last_k || (nu < p.units);
            TR(1);
            if (has_next) {
                if (last_k) { setup(nxt); fetch(nxt, nxt.t_begin, buf ^ 1); }
                else fetch(cur, t + 1, buf ^ 1);
            }
            TR(2);
            if (last_k) prefetch_epi(cur);
            compute(buf);
            TR(3);
            if (last_k) {
                __syncthreads();                 // every wave is done reading `buf`: its LDS becomes the staging area
                TR(4);
                epilogue(cur, buf);
                TR(5);
            }
            // (register-staged operands: hipcc hoisted these LDS stores - and with them the waits for the next tile's global loads -
            //  above the tile's MFMAs; the fence keeps the loads in flight under the products.  DMA'd operands have nothing to commit.)
            if constexpr (!ALL_DMA) __builtin_amdgcn_sched_barrier(0);
            if (has_next) commit(buf ^ 1);
            __syncthreads();
            TR(6);
            if (!has_next) break;
            if (last_k) { u = nu; cur = nxt; t = cur.t_begin; load_bias(cur); nu = seek(u + ustride, nxt); }
            else ++t;
            buf ^= 1;
        }
        TR_FLUSH;
    } else if constexpr (NST == 1) {
        // ---- single LDS stage, no intra-block overlap: 4 blocks per CU overlap each other instead ----------------
        Unit cur;
        int u = seek(blockIdx.x, cur);
        while (u < p.units) {
            setup(cur);
            load_bias(cur);
            for (int t = cur.t_begin; t < cur.t_end; ++t) {
                fetch(cur, t, 0);
                __syncthreads();                 // (drains the DMA queue) tile landed
                compute(0);
                __syncthreads();                 // everyone is done reading the stage
            }
            epilogue(cur, 0);
            __syncthreads();                     // staging slices free before the next unit's DMA overwrites them
            u = seek(u + ustride, cur);
        }
    } else {
        // ---- 3-stage DMA ring: item i is multiplied while items i+1 and i+2 are in flight ------------------------
        constexpr int LPT = 2 * TL::NLD;                   // DMA instructions per thread per item
        struct Cur { int u, t; Unit un; };
        auto advance = [&](Cur& c) {                      // c := item after c  (c.u >= p.units: none)
            if (c.t + 1 < c.un.t_end) { ++c.t; return; }
            c.u = seek(c.u + ustride, c.un);
            c.t = c.un.t_begin;
        };
        Cur c0;
        c0.u = seek(blockIdx.x, c0.un);
        if (c0.u >= p.units) return;
        c0.t = c0.un.t_begin;
        Cur c1 = c0; advance(c1);
        Cur c2 = c1; if (c1.u < p.units) advance(c2);
        int fetched_u = c0.u;
        setup(c0.un);
        load_bias(c0.un);
        fetch(c0.un, c0.t, 0);
        if (c1.u < p.units) {
            if (c1.u != fetched_u) { setup(c1.un); fetched_u = c1.u; }
            fetch(c1.un, c1.t, 1);
        }
        int st = 0;
        while (true) {
            const bool has1 = c1.u < p.units, has2 = has1 && (c2.u < p.units);
            // item c0 has landed when at most the DMAs of the one younger item are still outstanding
            if (has1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LPT) : "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                  // ... for every wave; and stage (st+2)%3 is free again
            TR(7);
            if (has2) {
                if (c2.u != fetched_u) { setup(c2.un); fetched_u = c2.u; }
                fetch(c2.un, c2.t, (st + 2) % 3);
            }
            TR(8);
            compute(st);
            TR(9);
            if (c0.t + 1 >= c0.un.t_end) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();              // all waves done reading stage st: it becomes the staging area
                TR(10);
                epilogue(c0.un, st);
                TR(11);
            }
            if (!has1) break;
            if (c1.u != c0.u) load_bias(c1.un);
            c0 = c1; c1 = c2;
            if (has2) advance(c2);
            st = (st + 1) % 3;
        }
        TR_FLUSH;
    }
}

constexpr int PA_MAX_GROUP_ = 8;
// xcd_chunk > 0: XCD-contiguous unit order.  Blocks are dealt to the 8 XCDs round-robin (block b -> XCD b % 8), so with the
// plain order the 4 - 8 units that share a dY / X panel (same K slice, same row or column of tiles) land on 4 - 8 different
// L2s and each of them fetches the panel from HBM.  With xcd_chunk = ceil(units / 8) the launch enumerates 8 * xcd_chunk
// slots and slot u is unit (u % 8) * xcd_chunk + u / 8 of the table: every XCD walks ONE contiguous eighth of the unit list
// (whole K slices of a member: each panel is fetched by one L2).  Needs gridDim.x % 8 == 0 (slots of a block stay on its XCD
// and in ascending unit order).
struct GemmGroup { GemmP p[PA_MAX_GROUP_]; int begin[PA_MAX_GROUP_ + 1]; int n; int xcd_chunk; };
__device__ __forceinline__ const GemmP& first_problem(const GemmP& p) { return p; }
__device__ __forceinline__ const GemmP& first_problem(const GemmGroup& g) { return g.p[0]; }
__device__ __forceinline__ int total_units_of(const GemmP& p) { return p.units; }
__device__ __forceinline__ int total_units_of(const GemmGroup& g) { return g.xcd_chunk > 0 ? 8 * g.xcd_chunk : g.begin[g.n]; }

// -------------------------------------------------------------------------------------------------
// v3 (bf16, both operands DMA'd): ONE block per CU (4 waves, one per SIMD, up to 512 VGPRs each), a 4-stage LDS
// ring of K tiles and a K loop that is software-pipelined at k-step granularity, so the three per-CU engines run
// concurrently instead of in turns:
//    * TA / direct-to-LDS DMA: the K tile three items ahead is in flight (issued right after the barrier that
//      frees its stage),
//    * LDS: the MFMA fragments of k-step s+1 are being read
//    * MFMA: while the four 32x32x16 MFMAs of k-step s execute.
// Items (unit, K tile) form one stream across unit boundaries, so the ring never drains inside a launch.
// Synchronisation per item: barrier A (stage of the previous item is free -> its DMA may be overwritten) and
// barrier B (counted s_waitcnt vmcnt: the next item has landed for every wave).  The epilogue uses a per-wave
// staging slice outside the ring (no block barrier) and straight-line code (no waits between stores).
// PT = GemmP (one problem) or GemmGroup (several problems in one launch: the unit stream runs through all of them; used
// for the weight gradients of a backward segment).  pd / pc = problem the DMA cursor / the compute cursor is in.
#ifdef PA_GEMM_TRACE3
// debug build only (tools/gemm_trace.py): per-block cycle stamps of the ring kernel
__device__ unsigned long long pa_gemm3_trace[512 * 8];
__device__ unsigned long long pa_gemm3_items[64];     // block 0: cycle stamp at the start of every K-tile item (bit 63: HOT)
__device__ int pa_gemm3_nitems;
#define PA_TR3(i) do { if (threadIdx.x == 0 && blockIdx.x < 512) pa_gemm3_trace[blockIdx.x * 8 + (i)] = __builtin_readcyclecounter(); } while (0)
#else
#define PA_TR3(i) do { } while (0)
#endif
template <bool A_KC, bool B_KC, typename PT>
__global__ __launch_bounds__(NT, 1) void gemm3_kernel(PT prm) {
    constexpr bool GROUP = std::is_same<PT, GemmGroup>::value;
    GemmP pd = first_problem(prm), pc = first_problem(prm);
    int pd_i = 0, pc_i = 0;                                   // GROUP: index of pd / pc in the table
    const int total_units = total_units_of(prm);
    using T = bf16;
    using TL = Tile<bf16, 64>;
    constexpr int NSTG = 4, STAGE = 2 * TL::TILE_BYTES, EPI = 8192;   // EPI: 32 rows x 64 f32 per wave
    constexpr bool A_TG = !A_KC, B_TG = !B_KC;
    __shared__ __attribute__((aligned(256))) char smem[NSTG * STAGE + 4 * EPI];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    PA_TR3(0);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5;
    constexpr int esz = 2;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // ---- DMA addressing of the unit the DMA cursor is in ------------------------------------------------------
    uint32_t offA[TL::NLD], offB[TL::NLD];
    bool okA[TL::NLD], okB[TL::NLD];
    const char* baseA = nullptr; const char* baseB = nullptr;
    auto setup = [&](const Unit& un) {
        baseA = reinterpret_cast<const char*>(pd.A) + (size_t)un.b * pd.sA * esz;
        baseB = reinterpret_cast<const char*>(pd.B) + (size_t)un.b * pd.sB * esz;
        const int m0 = un.tile_m * BM, n0 = un.tile_n * BN;
#pragma unroll
        for (int i = 0; i < TL::NLD; ++i) {
            const int pidx = tid + i * NT;
            if constexpr (A_KC) {
                const int row = pidx / TL::NCH, ch = ((pidx % TL::NCH) ^ (row / TL::RPB)) & (TL::NCH - 1);
                okA[i] = true;
                offA[i] = (uint32_t)min(m0 + row, pd.M - 1) * (uint32_t)(pd.lda * esz) + ch * 16;
            } else {
                const int row = pidx >> 4, col = m0 + (((pidx & 15) ^ ((row & 3) << 2)) << 3);
                okA[i] = col < pd.M;
                offA[i] = (uint32_t)row * (uint32_t)(pd.lda * esz) + (uint32_t)col * esz;
            }
            if constexpr (B_KC) {
                const int row = pidx / TL::NCH, ch = ((pidx % TL::NCH) ^ (row / TL::RPB)) & (TL::NCH - 1);
                okB[i] = true;
                offB[i] = (uint32_t)min(n0 + row, pd.N - 1) * (uint32_t)(pd.ldb * esz) + ch * 16;
            } else {
                const int row = pidx >> 4, col = n0 + (((pidx & 15) ^ ((row & 3) << 2)) << 3);
                okB[i] = col < pd.N;
                offB[i] = (uint32_t)row * (uint32_t)(pd.ldb * esz) + (uint32_t)col * esz;
            }
        }
    };
    // kA / kB: wave-uniform start of the DMA cursor's current K tile (advanced by one tile per item); k_dma: its first k
    const char* kA = nullptr; const char* kB = nullptr; int k_dma = 0;
    size_t stepA = 0, stepB = 0;               // bytes per K tile along the DMA source (set per unit in dma_enter)
    // one quarter of an item's DMA: Q = 0, 1 -> A chunks {0,1}, {2,3}; Q = 2, 3 -> B chunks {0,1}, {2,3}
    auto fetch_q = [&](int stage, auto Q_) {
        constexpr int Q = decltype(Q_)::value;
        char* lx = smem + stage * STAGE + (Q >= 2 ? TL::TILE_BYTES : 0);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = (Q & 1) * 2 + j;
            const char* src;
            if constexpr (Q < 2) {
                if constexpr (A_KC) src = kA + offA[i];
                else {
                    const bool in = okA[i] && (k_dma + ((tid + i * NT) >> 4)) < pd.K;
                    src = in ? kA + offA[i] : reinterpret_cast<const char*>(pa_zero16);
                }
            } else {
                if constexpr (B_KC) src = kB + offB[i];
                else {
                    const bool in = okB[i] && (k_dma + ((tid + i * NT) >> 4)) < pd.K;
                    src = in ? kB + offB[i] : reinterpret_cast<const char*>(pa_zero16);
                }
            }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                (__attribute__((address_space(3))) void*)(lx + (i * NT + wave * 64) * 16), 16, 0, 0);
        }
    };
    auto fetch_done = [&]() { kA += stepA; kB += stepB; k_dma += TL::BK; };
    using Q0 = std::integral_constant<int, 0>; using Q1 = std::integral_constant<int, 1>;
    using Q2 = std::integral_constant<int, 2>; using Q3 = std::integral_constant<int, 3>;
    auto fetch = [&](int stage) {
        fetch_q(stage, Q0{}); fetch_q(stage, Q1{}); fetch_q(stage, Q2{}); fetch_q(stage, Q3{});
        fetch_done();
    };

    // ---- fragment reads (lane-constant offsets inside a stage) ------------------------------------------------
    // The LDS reads are issued through inline asm so that their completion can be awaited with exact lgkmcnt counts
    // (the compiler's own bookkeeping degrades to lgkmcnt(0) around the loop back edge, which would serialise the
    // reads of k-step s+1 with the MFMAs of k-step s).  LDS returns in order; NRD = read instructions per k-step.
    constexpr int NRD = (A_TG ? 4 : 2) + (B_TG ? 4 : 2);
    const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)smem);
    const int sw = ((lane & 31) >> 1) & 7;
    uint32_t xs[4];                                   // k-contiguous image: swizzled chunk offset of k-step s
#pragma unroll
    for (int s_ = 0; s_ < 4; ++s_) xs[s_] = (uint32_t)((((2 * s_ + half) ^ sw) & 7) << 4);
    uint32_t fa_off[2], fb_off[2];                    // lane-constant part of the fragment address (A / B, row group i)
    {
        const int L = lane & 15, G = lane >> 4, kr = 8 * half + (L >> 2);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if constexpr (A_TG) {
                const int ca = (wm * 64 + i * 32 + 16 * (G & 1) + 4 * (L & 3)) * 2;
                fa_off[i] = kr * 256 + ((((ca >> 6) ^ ((L >> 2) & 3)) << 6) | (ca & 63));
            } else fa_off[i] = (wm * 64 + (lane & 31) + i * 32) * TL::RB;
            if constexpr (B_TG) {
                const int cb = (wn * 64 + i * 32 + 16 * (G & 1) + 4 * (L & 3)) * 2;
                fb_off[i] = kr * 256 + ((((cb >> 6) ^ ((L >> 2) & 3)) << 6) | (cb & 63));
            } else fb_off[i] = (wn * 64 + (lane & 31) + i * 32) * TL::RB;
        }
    }
#define PA_RD128(dst, addr, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF))
#define PA_RDTR(dst, addr, OFF) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF))
    // f[0..1] = A fragments (row groups 0, 1), f[2..3] = B fragments of k-step S of the tile at LDS address `st`;
    // rd1 issues the read(s) of ONE fragment W (0, 1: A; 2, 3: B)
    auto rd1 = [&](u32x4 (&f)[4], uint32_t st, auto S_, auto W_) {
        constexpr int S = decltype(S_)::value, W = decltype(W_)::value, i = W & 1;
        if constexpr (W < 2) {
            if constexpr (A_TG) {
                u32x2 lo, hi; const uint32_t ad = st + fa_off[i];
                PA_RDTR(lo, ad, S * 4096); PA_RDTR(hi, ad, S * 4096 + 1024);
                f[W][0] = lo[0]; f[W][1] = lo[1]; f[W][2] = hi[0]; f[W][3] = hi[1];
            } else { const uint32_t ad = st + fa_off[i] + xs[S]; PA_RD128(f[W], ad, 0); }
        } else {
            if constexpr (B_TG) {
                u32x2 lo, hi; const uint32_t ad = st + fb_off[i];
                PA_RDTR(lo, ad, TL::TILE_BYTES + S * 4096); PA_RDTR(hi, ad, TL::TILE_BYTES + S * 4096 + 1024);
                f[W][0] = lo[0]; f[W][1] = lo[1]; f[W][2] = hi[0]; f[W][3] = hi[1];
            } else { const uint32_t ad = st + fb_off[i] + xs[S]; PA_RD128(f[W], ad, TL::TILE_BYTES); }
        }
    };
    using W0 = std::integral_constant<int, 0>; using W1 = std::integral_constant<int, 1>;
    using W2 = std::integral_constant<int, 2>; using W3 = std::integral_constant<int, 3>;
    auto frag = [&](u32x4 (&f)[4], uint32_t st, auto S_) { rd1(f, st, S_, W0{}); rd1(f, st, S_, W1{}); rd1(f, st, S_, W2{}); rd1(f, st, S_, W3{}); };
    // every LDS read issued so far has returned (and `f` is complete)
    auto wait_frag = [&](u32x4 (&f)[4]) {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
    };
    // The MFMAs stay compiler builtins (an asm MFMA is opaque to the hazard recogniser: accumulator copies at control-
    // flow joins would read stale registers); the scheduler keeps them interleaved with the asm-volatile reads:
    // "MFMA, LDS read, MFMA, LDS read, ..." - each read is issued while the previous MFMA executes.
#define PA_MFMA(ACC, X, Y) mma16B<T>(ACC, X, Y)

#ifdef PA_GEMM_ABLATE      // timing ablations (wrong results): PA_GEMM_DBG bits 1 no MFMA, 2 no LDS reads, 4 no DMA, 8 no barriers
    const bool dbg_nomma = pc.dbg & 1, dbg_nord = pc.dbg & 2, dbg_nodma = pc.dbg & 4, dbg_nobar = pc.dbg & 8;
#define MMA1(ACC, X, Y) do { if (!dbg_nomma) PA_MFMA(ACC, X, Y); } while (0)
#define RD1(F, st, S, W) do { if (!dbg_nord) rd1(F, st, S, W); } while (0)
#define FRAG(F, st, S) do { if (!dbg_nord) frag(F, st, S); } while (0)
#define BAR() do { if (!dbg_nobar) __builtin_amdgcn_s_barrier(); } while (0)
#define DMA(x) do { if (!dbg_nodma) { x; } } while (0)
#else
#define MMA1(ACC, X, Y) PA_MFMA(ACC, X, Y)
#define RD1(F, st, S, W) rd1(F, st, S, W)
#define FRAG(F, st, S) frag(F, st, S)
#define BAR() __builtin_amdgcn_s_barrier()
#define DMA(x) do { x; } while (0)
#endif
    int sd = 0;                                 // LDS stage the next DMA item goes to
    // one k-step: the four MFMAs on `fc`, interleaved with the reads of the next k-step's fragments into `fn`
    // (RD = false: no next k-step) and, in the hot loop, with one quarter of the DMA three items ahead
    auto step = [&](u32x4 (&fc)[4], u32x4 (&fn)[4], uint32_t stn, auto SN_, auto RD_, auto DQ_) {
        constexpr bool RD = decltype(RD_)::value;
        constexpr int DQ = decltype(DQ_)::value;       // -1: no DMA in this step
        wait_frag(fc);
        MMA1(acc[0][0], fc[2], fc[0]); if constexpr (RD) RD1(fn, stn, SN_, W0{});
        MMA1(acc[0][1], fc[2], fc[1]); if constexpr (RD) RD1(fn, stn, SN_, W1{});
        if constexpr (DQ >= 0) DMA(fetch_q(sd, std::integral_constant<int, (DQ >= 0 ? DQ : 0)>{}));
        MMA1(acc[1][0], fc[3], fc[0]); if constexpr (RD) RD1(fn, stn, SN_, W2{});
        MMA1(acc[1][1], fc[3], fc[1]); if constexpr (RD) RD1(fn, stn, SN_, W3{});
    };
    using NoQ = std::integral_constant<int, -1>;

    // (No prefetch of the first unit's residual / gate tiles before the K loop here: it was measured and removed in round 4 - the 64
    //  registers held across the K loop pushed the kernel to 256 VGPRs + 203 AGPRs used as spill space; without it 208 VGPRs + 128
    //  AGPRs and 12.15 / 15.66 / 19.12 us against 12.51 / 16.10 / 19.95 us per launch with a residual, 7 940 x 512, K 512 / 1 024 / 1 536.)
    // ---- epilogue ------------------------------------------------------------------------------------------------
    auto epilogue = [&](const Unit& un) {
        char* stage = smem + NSTG * STAGE + wave * EPI;
        const bool slab = pc.splitk > 1;
        const size_t cbase = slab ? (size_t)un.z * pc.M * pc.ldc : (size_t)un.b * pc.sC;
        const int mw = un.tile_m * BM + wm * 64, nw = un.tile_n * BN + wn * 64;
        const int chunk = lane & 15, rsub = lane >> 4;
        const int n = nw + chunk * 4;
        const bool out_f32 = slab || pc.out_dtype == PA_F32;
        const bool has_bias = !slab && pc.bias != nullptr, has_aux = !slab && pc.aux != nullptr;
        const bool has_res = !slab && pc.R != nullptr, has_drop = !slab && pc.drop_thr != 0;
        const bool fast = pc.vec_ok && (nw + 64 <= pc.N);                   // wave-uniform
        const float alpha = slab ? 1.f : pc.alpha;
        constexpr int NIT = 8;
        f32x4 bias = {0.f, 0.f, 0.f, 0.f};
        if (has_bias) {
            const float* bp = pc.bias + (size_t)un.b * pc.sBias;
            if (fast) bias = *reinterpret_cast<const f32x4*>(bp + n);
            else { for (int e = 0; e < 4; ++e) if (n + e < pc.N) bias[e] = bp[n + e]; }
        }
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {          // pass = tm: output rows mw + 32*pass .. +31
            const int lrow = lane & 31;
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[tn][pass][4 * g4 + e];
                    const int ch = tn * 8 + 2 * g4 + half;
                    *reinterpret_cast<f32x4*>(stage + lrow * 256 + ((ch ^ (lrow & 15)) << 4)) = v;
                }
            f32x4 x[NIT];
            const int mp = mw + pass * 32 + rsub;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int lr = it * 4 + rsub;
                x[it] = *reinterpret_cast<const f32x4*>(stage + lr * 256 + ((chunk ^ (lr & 15)) << 4));
            }
            if (fast) {
                f32x4 res[NIT], gate[NIT];
                if (has_res) {
                    if (out_f32) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) {
                            const size_t ro = (size_t)un.b * pc.sR + (size_t)min(mp + it * 4, pc.M - 1) * pc.ldr + n;
                            res[it] = ld4<float>(reinterpret_cast<const float*>(pc.R) + ro);
                        }
                    } else {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) {
                            const size_t ro = (size_t)un.b * pc.sR + (size_t)min(mp + it * 4, pc.M - 1) * pc.ldr + n;
                            res[it] = ld4<bf16>(reinterpret_cast<const bf16*>(pc.R) + ro);
                        }
                    }
                }
                if (has_aux) {
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        const size_t ao = (size_t)un.b * pc.sAux + (size_t)min(mp + it * 4, pc.M - 1) * pc.ldaux + n;
                        gate[it] = ld4<T>(reinterpret_cast<const T*>(pc.aux) + ao);
                    }
                }
                if (!slab) {
                    // one straight-line loop per optional stage, each behind its own (uniform) branch: as conditions inside one
                    // per-element loop every stage cost its compare / select on every element whether it was enabled or not
                    // (the epilogue of a plain Linear ran ~1 200 instructions per wave; a lone wave issues one per ~6.5 cycles)
#pragma unroll
                    for (int it = 0; it < NIT; ++it)
#pragma unroll
                        for (int e = 0; e < 4; ++e) x[it][e] = x[it][e] * alpha + bias[e];
                    if (pc.relu) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it)
#pragma unroll
                            for (int e = 0; e < 4; ++e) x[it][e] = fmaxf(x[it][e], 0.f);
                    }
                    if (has_aux) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it)
#pragma unroll
                            for (int e = 0; e < 4; ++e) x[it][e] = gate[it][e] > 0.f ? x[it][e] * pc.aux_scale : 0.f;
                    }
                    if (has_drop) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                x[it][e] = drop_keep_rc(pc.drop_seed, (uint32_t)(un.b * pc.M + mp + it * 4), (uint32_t)(n + e), pc.drop_thr) ? x[it][e] * pc.drop_scale : 0.f;
                            }
                    }
                    if (has_res) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it)
#pragma unroll
                            for (int e = 0; e < 4; ++e) x[it][e] += res[it][e];
                    }
                }
                // Stores: one running pointer, the output type and the "all 32 rows valid" test decided once per pass (as
                // run-time conditions inside the loop they were a branch pair + 64-bit index arithmetic per store, ~20
                // instructions each for a lone wave that issues one instruction per ~6.5 cycles).
                const bool interior = mw + pass * 32 + 32 <= pc.M;                   // wave-uniform
                const size_t co0 = cbase + (size_t)mp * pc.ldc + n, rstep = (size_t)4 * pc.ldc;
                if (out_f32) {
                    float* cp = reinterpret_cast<float*>(pc.C) + co0;
                    if (interior) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) *reinterpret_cast<f32x4*>(cp + it * rstep) = x[it];
                    } else {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) if (mp + it * 4 < pc.M) *reinterpret_cast<f32x4*>(cp + it * rstep) = x[it];
                    }
                } else {
                    bf16* cp = reinterpret_cast<bf16*>(pc.C) + co0;
                    if (interior) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) st4<bf16>(cp + it * rstep, x[it]);
                    } else {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) if (mp + it * 4 < pc.M) st4<bf16>(cp + it * rstep, x[it]);
                    }
                }
            } else {
                // edge / unaligned column block: element-wise (rare)
#pragma unroll 1
                for (int it = 0; it < NIT; ++it) {
                    const int m = mp + it * 4;
                    if (m >= pc.M) continue;
                    for (int e = 0; e < 4; ++e) {
                        if (n + e >= pc.N) continue;
                        float y = x[it][e];
                        if (!slab) {
                            y = y * alpha + bias[e];
                            if (pc.relu) y = fmaxf(y, 0.f);
                            if (has_aux) {
                                const float g = ld1(reinterpret_cast<const T*>(pc.aux) + (size_t)un.b * pc.sAux + (size_t)m * pc.ldaux + n + e);
                                y = g > 0.f ? y * pc.aux_scale : 0.f;
                            }
                            if (has_drop) {
                                y = drop_keep_rc(pc.drop_seed, (uint32_t)(un.b * pc.M + m), (uint32_t)(n + e), pc.drop_thr) ? y * pc.drop_scale : 0.f;
                            }
                            if (has_res) {
                                const size_t ro = (size_t)un.b * pc.sR + (size_t)m * pc.ldr + n + e;
                                y += out_f32 ? reinterpret_cast<const float*>(pc.R)[ro] : (float)reinterpret_cast<const bf16*>(pc.R)[ro];
                            }
                        }
                        const size_t co = cbase + (size_t)m * pc.ldc + n + e;
                        if (out_f32) reinterpret_cast<float*>(pc.C)[co] = y;
                        else reinterpret_cast<bf16*>(pc.C)[co] = (bf16)y;
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    };

    // ---- item stream ---------------------------------------------------------------------------------------------
    // Two cursors walk the same sequence of (unit, K tile) items: the DMA cursor three items ahead of the compute
    // cursor.  Per item each only bumps a tile counter; units are decoded (integer divisions, address set-up) once
    // per unit and cursor, off the common path.
    const int ustride = gridDim.x;
    // first valid unit >= u; GROUP: px / pi follow the unit into its problem (units only ever move forward)
    auto seek = [&](int u, Unit& un, GemmP& px, int& pi) -> int {
        while (u < total_units) {
            int local = u;
            if constexpr (GROUP) {
                int g = u;
                if (prm.xcd_chunk > 0) {
                    g = (u & 7) * prm.xcd_chunk + (u >> 3);
                    if (g >= prm.begin[prm.n]) { u += ustride; continue; }     // padding slot of the last XCD
                }
                bool moved = false;
                while (g >= prm.begin[pi + 1]) { ++pi; moved = true; }
                if (moved) px = prm.p[pi];
                local = g - prm.begin[pi];
            }
            if (decode_unit<TL>(px, local, un)) break;
            u += ustride;
        }
        return u;
    };
    int cd_u, cd_t = 0, cd_end = 0;             // DMA cursor: unit, next tile, end tile
    int cc_u, cc_t = 0, cc_end = 0;             // compute cursor
    // `known`: the unit at `u` was already decoded (the compute cursor's first unit): its integer-division chain is ~1 000
    // cycles for the lone wave of a SIMD, on the path to the block's first DMA
    auto dma_enter = [&](int u, const Unit* known = nullptr) {   // position the DMA cursor at the first valid unit >= u
        Unit un;
        if (known) { un = *known; cd_u = u; pd = pc; pd_i = pc_i; }
        else cd_u = seek(u, un, pd, pd_i);
        if (cd_u < total_units) {
            setup(un);
            cd_t = un.t_begin; cd_end = un.t_end;
            k_dma = un.t_begin * TL::BK;
            stepA = A_KC ? (size_t)TL::BK * esz : (size_t)TL::BK * pd.lda * esz;
            stepB = B_KC ? (size_t)TL::BK * esz : (size_t)TL::BK * pd.ldb * esz;
            kA = baseA + (A_KC ? (size_t)k_dma * esz : (size_t)k_dma * pd.lda * esz);
            kB = baseB + (B_KC ? (size_t)k_dma * esz : (size_t)k_dma * pd.ldb * esz);
        }
    };
    Unit cun;                                   // unit of the compute cursor (for its epilogue)
    auto cmp_enter = [&](int u) {
        cc_u = seek(u, cun, pc, pc_i);
        cc_t = cun.t_begin; cc_end = cun.t_end;
    };
    cmp_enter(blockIdx.x);
    if (cc_u >= total_units) return;
    dma_enter(cc_u, &cun);
    int pending = 0;                            // items issued and not yet finished by the MFMAs
    auto issue = [&]() {
        DMA(fetch(sd));
        sd = (sd + 1) & (NSTG - 1);
        ++pending;
        if (++cd_t >= cd_end) dma_enter(cd_u + ustride);
    };
    // wait until at most `younger` whole items (8 DMA instructions each) are still outstanding
    auto wait_items = [&](int younger) {
        if (younger >= 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    PA_TR3(1);
#pragma unroll 1
    for (int k = 0; k < 3; ++k) if (cd_u < total_units) issue();
    wait_items(pending - 1);
    __builtin_amdgcn_s_barrier();
    PA_TR3(2);
    int sc = 0;
#ifdef PA_GEMM_TRACE3
    int tr_items = 0;
#endif
    u32x4 F0[4], F1[4];
    using S0 = std::integral_constant<int, 0>; using S1 = std::integral_constant<int, 1>;
    using S2 = std::integral_constant<int, 2>; using S3 = std::integral_constant<int, 3>;
    FRAG(F0, lds0, S0{});
    // One item = one K tile.  HOT: steady state inside a unit - the DMA cursor stays in the same unit, three items are
    // in flight and a next item exists, so the body is branch-free; the general body handles the ends of the stream.
    auto item = [&](auto HOT_) -> bool {
        constexpr bool HOT = decltype(HOT_)::value;
        using QA = std::integral_constant<int, HOT ? 0 : -1>; using QB = std::integral_constant<int, HOT ? 1 : -1>;
        using QC = std::integral_constant<int, HOT ? 2 : -1>; using QD = std::integral_constant<int, HOT ? 3 : -1>;
        const uint32_t st = lds0 + sc * STAGE;
        // barrier A: every wave has finished the previous item, so its stage may be refilled (HOT: the DMA of the item
        // three ahead is spread over the four k-steps; otherwise it is issued here in one go)
#ifdef PA_GEMM_TRACE3
        if (threadIdx.x == 0 && blockIdx.x == 0 && tr_items < 63) pa_gemm3_items[tr_items++] = __builtin_readcyclecounter() | (HOT ? (1ull << 63) : 0ull);
#endif
        BAR();
        if constexpr (!HOT) { if (cd_u < total_units) issue(); }
        step(F0, F1, st, S1{}, std::true_type{}, QA{});
        step(F1, F0, st, S2{}, std::true_type{}, QB{});
        step(F0, F1, st, S3{}, std::true_type{}, QC{});
        // last k-step; barrier B: the next item has landed for every wave -> its first fragments are read meanwhile
        const bool has_next = HOT || pending >= 2;
        if (has_next) {
            if constexpr (HOT) { DMA(fetch_q(sd, Q3{}); fetch_done()); sd = (sd + 1) & (NSTG - 1); ++cd_t; wait_items(2); }
            else wait_items(pending - 2);
            BAR();
        }
        // (the next stage's first fragments are requested even when no next item exists - from a stage nobody fills any more, never
        //  used: with the reads on one path only, hipcc resolved the two paths' fragment registers with v_mov copies of registers
        //  whose reads were still in flight, in FRONT of the hand-written lgkmcnt wait - found by reading the ISA in round 6)
        step(F1, F0, lds0 + ((sc + 1) & (NSTG - 1)) * STAGE, S0{}, std::true_type{}, NoQ{});
        sc = (sc + 1) & (NSTG - 1);
        if constexpr (HOT) { ++cc_t; return true; }
        else {
            if (++cc_t >= cc_end) {
                PA_TR3(3);
#ifdef PA_GEMM_TRACE3
                if (threadIdx.x == 0 && blockIdx.x == 0) { pa_gemm3_items[tr_items] = __builtin_readcyclecounter(); pa_gemm3_nitems = tr_items; }
#endif
                epilogue(cun);
#ifdef PA_GEMM_TRACE3
                PA_TR3(5);                                     // every store of the tile issued
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
                PA_TR3(4);                                     // ... and retired
                if (has_next) cmp_enter(cc_u + ustride);
            }
            --pending;
            return has_next;
        }
    };
#pragma unroll 1
    while (true) {
        // hot stretch: while both cursors stay inside the current unit (pending == 3 on entry of every hot item)
        // (the DMA cursor's last tile of the unit is issued by the general body, which then moves it to the next unit)
        int hot = (pending == 3 && cd_u == cc_u) ? (cd_end - cd_t - 1) : 0;
#pragma unroll 1
        for (; hot > 0; --hot) item(std::true_type{});
        if (!item(std::false_type{})) break;
    }
#undef PA_RD128
#undef PA_RDTR
#undef MMA1
#undef RD1
#undef FRAG
#undef BAR
#undef DMA
#undef PA_MFMA
}

// -------------------------------------------------------------------------------------------------
// Small-tile ring kernel: 64 x 64 x 64 tiles for launches whose 128 x 128 tiling would occupy a quarter of the CUs or
// less (decoder-side Linears M = B*T = 2 048, every Linear of the greedy-decode step M = B).  Same structure as
// gemm3_kernel - one block per CU, 4-stage ring of K tiles filled by direct-to-LDS DMA, k-steps that interleave the MFMA
// with the next k-step's fragment reads - with one 32 x 32 MFMA tile per wave (2 x 2 waves), so a K tile costs a
// quarter of the LDS / MFMA time and four times as many CUs share the problem.  bf16, both operands k-contiguous,
// K % 64 == 0, one problem, no split-K.
__global__ __launch_bounds__(NT, 2) void gemm3s_kernel(GemmP p) {
    using T = bf16;
    constexpr int TB = 64;                              // tile edge
    constexpr int RB = 128, NCH = 8;                    // bytes / 16-byte chunks per LDS row (64 bf16)
    constexpr int TILE_BYTES = TB * RB;                 // 8 KiB per operand
    constexpr int NLD = TB * NCH / NT;                  // 2 chunks per thread per operand
    constexpr int NSTG = 4, STAGE = 2 * TILE_BYTES, EPI = 32 * 32 * 4;    // EPI: 32 rows x 32 f32 per wave
    __shared__ __attribute__((aligned(256))) char smem[NSTG * STAGE + 4 * EPI];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    PA_TR3(0);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5;
    constexpr int esz = 2;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    // ---- DMA addressing ---------------------------------------------------------------------------------------
    uint32_t offA[NLD], offB[NLD];
    const char* kA = nullptr; const char* kB = nullptr;
    auto setup = [&](const Unit& un, int t_begin) {
        const char* baseA = reinterpret_cast<const char*>(p.A) + (size_t)un.b * p.sA * esz + (size_t)t_begin * 64 * esz;
        const char* baseB = reinterpret_cast<const char*>(p.B) + (size_t)un.b * p.sB * esz + (size_t)t_begin * 64 * esz;
        const int m0 = un.tile_m * TB, n0 = un.tile_n * TB;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int pidx = tid + i * NT, row = pidx / NCH, ch = ((pidx % NCH) ^ (row / 2)) & (NCH - 1);
            offA[i] = (uint32_t)min(m0 + row, p.M - 1) * (uint32_t)(p.lda * esz) + ch * 16;
            offB[i] = (uint32_t)min(n0 + row, p.N - 1) * (uint32_t)(p.ldb * esz) + ch * 16;
        }
        kA = baseA; kB = baseB;
    };
    // one quarter of an item's DMA: Q = 0, 1 -> A chunk 0, 1; Q = 2, 3 -> B chunk 0, 1
    auto fetch_q = [&](int stage, auto Q_) {
        constexpr int Q = decltype(Q_)::value, i = Q & 1;
        char* lx = smem + stage * STAGE + (Q >= 2 ? TILE_BYTES : 0);
        const char* src = (Q < 2) ? kA + offA[i] : kB + offB[i];
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
            (__attribute__((address_space(3))) void*)(lx + (i * NT + wave * 64) * 16), 16, 0, 0);
    };
    auto fetch_done = [&]() { kA += 64 * esz; kB += 64 * esz; };
    using Q0 = std::integral_constant<int, 0>; using Q1 = std::integral_constant<int, 1>;
    using Q2 = std::integral_constant<int, 2>; using Q3 = std::integral_constant<int, 3>;
    auto fetch = [&](int stage) {
        fetch_q(stage, Q0{}); fetch_q(stage, Q1{}); fetch_q(stage, Q2{}); fetch_q(stage, Q3{});
        fetch_done();
    };

    // ---- fragment reads ------------------------------------------------------------------------------------------
    const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)smem);
    const int sw = ((lane & 31) >> 1) & 7;
    uint32_t xs[4];
#pragma unroll
    for (int s_ = 0; s_ < 4; ++s_) xs[s_] = (uint32_t)((((2 * s_ + half) ^ sw) & 7) << 4);
    const uint32_t fa_off = (wm * 32 + (lane & 31)) * RB, fb_off = (wn * 32 + (lane & 31)) * RB + TILE_BYTES;
#define PA_RD128(dst, addr) asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(addr))

    // residual / gate tile of the block's first unit, requested before its first K tile (as in gemm3_kernel)
    u32x2 pre_res[4], pre_aux[4];
    bool pre_live = false;
    float ln_mean[4] = {0.f, 0.f, 0.f, 0.f}, ln_rstd[4] = {1.f, 1.f, 1.f, 1.f};     // (p.ln_u: statistics of this lane's rows)
    // ---- epilogue: per-wave staging (32 x 32 f32), straight-line fast path ------------------------------------------
    auto epilogue = [&](const Unit& un) {
        char* stage = smem + NSTG * STAGE + wave * EPI;
        const bool pre = pre_live;
        pre_live = false;
        const size_t cbase = (size_t)un.b * p.sC;
        const int mw = un.tile_m * TB + wm * 32, nw = un.tile_n * TB + wn * 32;
        const int chunk = lane & 7, rsub = lane >> 3;                     // 8 chunks of 4 columns, 8 rows per instruction
        const int n = nw + chunk * 4;
        const bool out_f32 = p.out_dtype == PA_F32;
        const bool has_bias = p.bias != nullptr, has_aux = p.aux != nullptr, has_res = p.R != nullptr, has_drop = p.drop_thr != 0;
        const bool fast = p.vec_ok && (nw + 32 <= p.N);                   // wave-uniform
        constexpr int NIT = 4;
        f32x4 bias = {0.f, 0.f, 0.f, 0.f};
        if (has_bias) {
            const float* bp = p.bias + (size_t)un.b * p.sBias;
            if (fast) bias = *reinterpret_cast<const f32x4*>(bp + n);
            else { for (int e = 0; e < 4; ++e) if (n + e < p.N) bias[e] = bp[n + e]; }
        }
        {
            const int lrow = lane & 31;                                   // accumulator: row (m) = lane & 31, value r <-> n
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[4 * g4 + e];
                const int ch = 2 * g4 + half;
                *reinterpret_cast<f32x4*>(stage + lrow * 128 + ((ch ^ (lrow & 7)) << 4)) = v;
            }
        }
        f32x4 x[NIT];
        const int mp = mw + rsub;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int lr = it * 8 + rsub;
            x[it] = *reinterpret_cast<const f32x4*>(stage + lr * 128 + ((chunk ^ (lr & 7)) << 4));
        }
        if (fast) {
            f32x4 res[NIT], gate[NIT];
            auto widen = [](const u32x2& u) { f32x4 r; r[0] = bf16_lo(u[0]); r[1] = bf16_hi(u[0]); r[2] = bf16_lo(u[1]); r[3] = bf16_hi(u[1]); return r; };
            if (has_res) {
                if (pre) {
#pragma unroll
                    for (int it = 0; it < NIT; ++it) res[it] = widen(pre_res[it]);
                } else {
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        const size_t ro = (size_t)un.b * p.sR + (size_t)min(mp + it * 8, p.M - 1) * p.ldr + n;
                        if (out_f32) res[it] = ld4<float>(reinterpret_cast<const float*>(p.R) + ro);
                        else res[it] = ld4<bf16>(reinterpret_cast<const bf16*>(p.R) + ro);
                    }
                }
            }
            if (has_aux) {
                if (pre) {
#pragma unroll
                    for (int it = 0; it < NIT; ++it) gate[it] = widen(pre_aux[it]);
                } else {
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        const size_t ao = (size_t)un.b * p.sAux + (size_t)min(mp + it * 8, p.M - 1) * p.ldaux + n;
                        gate[it] = ld4<T>(reinterpret_cast<const T*>(p.aux) + ao);
                    }
                }
            }
            // one straight-line loop per optional stage behind its own uniform branch, stores with the output type and the
            // row-validity test decided once (see gemm3_kernel)
            if (p.ln_u) {                                   // A = LayerNorm(Z) folded in: rstd (acc - mean u) + (b + W beta)
                const f32x4 u4 = *reinterpret_cast<const f32x4*>(p.ln_u + n);
#pragma unroll
                for (int it = 0; it < NIT; ++it)
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[it][e] = ln_rstd[it] * (x[it][e] * p.alpha - ln_mean[it] * u4[e]) + bias[e];
            } else {
#pragma unroll
                for (int it = 0; it < NIT; ++it)
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[it][e] = x[it][e] * p.alpha + bias[e];
            }
            if (p.relu) {
#pragma unroll
                for (int it = 0; it < NIT; ++it)
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[it][e] = fmaxf(x[it][e], 0.f);
            }
            if (has_aux) {
#pragma unroll
                for (int it = 0; it < NIT; ++it)
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[it][e] = gate[it][e] > 0.f ? x[it][e] * p.aux_scale : 0.f;
            }
            if (has_drop) {
#pragma unroll
                for (int it = 0; it < NIT; ++it)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        x[it][e] = drop_keep_rc(p.drop_seed, (uint32_t)(un.b * p.M + mp + it * 8), (uint32_t)(n + e), p.drop_thr) ? x[it][e] * p.drop_scale : 0.f;
                    }
            }
            if (has_res) {
#pragma unroll
                for (int it = 0; it < NIT; ++it)
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[it][e] += res[it][e];
            }
            const bool interior = mw + 32 <= p.M;                                  // wave-uniform
            const size_t co0 = cbase + (size_t)mp * p.ldc + n, rstep = (size_t)8 * p.ldc;
            if (out_f32) {
                float* cp = reinterpret_cast<float*>(p.C) + co0;
                if (interior) {
#pragma unroll
                    for (int it = 0; it < NIT; ++it) *reinterpret_cast<f32x4*>(cp + it * rstep) = x[it];
                } else {
#pragma unroll
                    for (int it = 0; it < NIT; ++it) if (mp + it * 8 < p.M) *reinterpret_cast<f32x4*>(cp + it * rstep) = x[it];
                }
            } else {
                bf16* cp = reinterpret_cast<bf16*>(p.C) + co0;
                if (interior) {
#pragma unroll
                    for (int it = 0; it < NIT; ++it) st4<bf16>(cp + it * rstep, x[it]);
                } else {
#pragma unroll
                    for (int it = 0; it < NIT; ++it) if (mp + it * 8 < p.M) st4<bf16>(cp + it * rstep, x[it]);
                }
            }
        } else {
#pragma unroll 1
            for (int it = 0; it < NIT; ++it) {
                const int m = mp + it * 8;
                if (m >= p.M) continue;
                for (int e = 0; e < 4; ++e) {
                    if (n + e >= p.N) continue;
                    float y = x[it][e] * p.alpha + bias[e];
                    if (p.relu) y = fmaxf(y, 0.f);
                    if (has_aux) {
                        const float g = ld1(reinterpret_cast<const T*>(p.aux) + (size_t)un.b * p.sAux + (size_t)m * p.ldaux + n + e);
                        y = g > 0.f ? y * p.aux_scale : 0.f;
                    }
                    if (has_drop) {
                        y = drop_keep_rc(p.drop_seed, (uint32_t)(un.b * p.M + m), (uint32_t)(n + e), p.drop_thr) ? y * p.drop_scale : 0.f;
                    }
                    if (has_res) {
                        const size_t ro = (size_t)un.b * p.sR + (size_t)m * p.ldr + n + e;
                        y += out_f32 ? reinterpret_cast<const float*>(p.R)[ro] : (float)reinterpret_cast<const bf16*>(p.R)[ro];
                    }
                    const size_t co = cbase + (size_t)m * p.ldc + n + e;
                    if (out_f32) reinterpret_cast<float*>(p.C)[co] = y;
                    else reinterpret_cast<bf16*>(p.C)[co] = (bf16)y;
                }
            }
        }
        // every path "uses" the bias: a path that loaded it and stored nothing (a wave past the last row) would leave the load
        // pending in the COMPILER's scoreboard, and it would guard the K loop's first temporary with `s_waitcnt vmcnt(0)` - the
        // whole ring - on every item
        asm volatile("" :: "v"(bias[0]), "v"(bias[1]), "v"(bias[2]), "v"(bias[3]));
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    };

    // ---- item stream (as in gemm3_kernel; plain unit order, every unit valid, no split-K) ---------------------------------
    const int ustride = gridDim.x, nt = p.K / 64;
    auto unit_of = [&](int u, Unit& un) {
        const int per_b = p.tiles_m * p.tiles_n;
        un.b = u / per_b; un.z = un.b;
        const int r = u - un.b * per_b;
        un.tile_m = r / p.tiles_n; un.tile_n = r - un.tile_m * p.tiles_n;
        un.t_begin = 0; un.t_end = nt;
    };
    int cd_u = blockIdx.x, cd_t = 0;            // DMA cursor
    int cc_u = blockIdx.x, cc_t = 0;            // compute cursor
    // (no `cc_u >= p.units` exit: both launch sites size the grid to at most p.units, and the test put a lone dependent kernel-argument
    //  load in front of every other one - a scalar-memory round trip at the head of each of the step's 71 launches)
    Unit cun, dun;
    unit_of(cc_u, cun);
    {   // prefetch (bf16, vector path), before the first DMA instruction so that the in-order `vmcnt` counts stay exact
        const int nw0 = cun.tile_n * TB + wn * 32;
        if (p.vec_ok && nw0 + 32 <= p.N && p.out_dtype != PA_F32 && (p.R != nullptr || p.aux != nullptr)) {
            pre_live = true;
            const int mp0 = cun.tile_m * TB + wm * 32 + (lane >> 3), n0 = nw0 + (lane & 7) * 4;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int m = min(mp0 + it * 8, p.M - 1);
                if (p.R) pre_res[it] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16*>(p.R) + (size_t)cun.b * p.sR + (size_t)m * p.ldr + n0);
                if (p.aux) pre_aux[it] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16*>(p.aux) + (size_t)cun.b * p.sAux + (size_t)m * p.ldaux + n0);
            }
        }
    }
    unit_of(cd_u, dun); setup(dun, 0);
    int sd = 0, pending = 0;
    auto issue = [&]() {
        fetch(sd);
        sd = (sd + 1) & (NSTG - 1);
        ++pending;
        if (++cd_t >= nt) { cd_u += ustride; cd_t = 0; if (cd_u < p.units) { unit_of(cd_u, dun); setup(dun, 0); } }
    };
    auto wait_items = [&](int younger) {        // items are 4 DMA instructions each here
        if (younger >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    PA_TR3(1);
#pragma unroll 1
    for (int k = 0; k < 3; ++k) if (cd_u < p.units) issue();
    if (p.ln_u) {
        // LayerNorm statistics of this lane's four output rows (the epilogue's rows mp + 8 it): the eight lanes that share a
        // row (chunk = lane & 7) each sum an eighth of it, three exchanges combine them.  Ordinary loads, issued BEHIND the first
        // three K tiles' DMA (their round trips overlap); the compiler's wait for them also covers those older DMAs, and the
        // few y stores that may still be in flight at the first hand-counted vmcnt wait only make it conservative.
        const int mp0 = cun.tile_m * TB + wm * 32 + (lane >> 3), ch = lane & 7;
        const bf16* zb = reinterpret_cast<const bf16*>(p.A) + (size_t)cun.b * p.sA;
        const float inv_k = 1.0f / (float)p.K;
        // all loads of a 512-column slab are issued before the first is used (unconditional, clamped addresses; surplus
        // chunks are discarded in the arithmetic): one memory round trip per slab instead of one per chunk
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < p.K; kb += 512) {
            u32x4 v[4][8];
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const bf16* zr = zb + (size_t)min(mp0 + it * 8, p.M - 1) * p.lda;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[it][j] = *reinterpret_cast<const u32x4*>(zr + min(kb + ch * 8 + 64 * j, p.K - 8));
            }
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float keep = (kb + ch * 8 + 64 * j < p.K) ? 1.f : 0.f;
                    float t1 = 0.f, t2 = 0.f;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const float a0 = bf16_lo(v[it][j][w]), a1 = bf16_hi(v[it][j][w]);
                        t1 += a0 + a1; t2 += a0 * a0 + a1 * a1;
                    }
                    s1[it] += keep * t1; s2[it] += keep * t2;
                }
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            float a1 = s1[it], a2 = s2[it];
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) { a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o); }
            const float mean = a1 * inv_k;
            ln_mean[it] = mean;
            ln_rstd[it] = rsqrtf(fmaxf(a2 * inv_k - mean * mean, 0.f) + p.ln_eps);
        }
        // y = LayerNorm(z) for the later residual add: the column tiles 0 .. K/64 - 1 each write their 64 columns
        if (p.ln_y && cun.tile_n * TB < p.K) {
            const int n0 = cun.tile_n * TB + wn * 32 + ch * 4;
            if (n0 + 4 <= p.K) {
                const f32x4 gm = *reinterpret_cast<const f32x4*>(p.ln_gamma + n0), bt = *reinterpret_cast<const f32x4*>(p.ln_beta + n0);
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int m = mp0 + it * 8;
                    if (m < p.M) {
                        f32x4 z = ld4<bf16>(zb + (size_t)m * p.lda + n0);
#pragma unroll
                        for (int e = 0; e < 4; ++e) z[e] = (z[e] - ln_mean[it]) * ln_rstd[it] * gm[e] + bt[e];
                        st4<bf16>(reinterpret_cast<bf16*>(p.ln_y) + (size_t)m * p.ldy + n0, z);
                    }
                }
            }
        }
        // a wait the COMPILER sees (vmcnt 0, other counters untouched): without it its scoreboard carries this block's loads into
        // the K loop (the hand-counted waits there are inline assembly) and it puts its own `s_waitcnt vmcnt(0)` in front of every
        // item's DMA - every item then waited for the whole ring, one memory round trip per item
        __builtin_amdgcn_s_waitcnt(0x0F70);
    }
    wait_items(pending - 1);
    __builtin_amdgcn_s_barrier();
    PA_TR3(2);
    int sc = 0;
    // One item = one 64-deep K tile = four MFMAs per wave.  With ONE wave per SIMD nothing else hides an LDS round trip, so the
    // fragments are requested a WHOLE item ahead: behind the item's barrier (the next item has landed) the pair of reads of the
    // next item's k-step s goes out right after the MFMA of this item's k-step s, into the registers that MFMA has just read -
    // eight reads in flight, each with three MFMAs of lead (round 6; reading one k-step ahead made every k-step wait out most of
    // an LDS latency: tools/gemm_small_k.py, profiles/r06_gemm_small_tile.txt).  ONE barrier per item: behind it every wave's
    // reads of the item before have returned (its stage is the one this item's DMA refills) and every wave's share of the next
    // item has arrived.
    u32x4 F[8];
#pragma unroll
    for (int s_ = 0; s_ < 4; ++s_) { PA_RD128(F[2 * s_], lds0 + fa_off + xs[s_]); PA_RD128(F[2 * s_ + 1], lds0 + fb_off + xs[s_]); }
    // (one loop body for every item: a second, specialised body made the compiler COPY the fragment registers between the two
    //  while their reads were still in flight - the reads are inline assembly, their latency is invisible to it)
#pragma unroll 1
    while (true) {
        const bool has_next = pending >= 2;
        if (has_next) wait_items(pending - 2);
        __builtin_amdgcn_s_barrier();
        if (cd_u < p.units) issue();
        {   // (the reads go out even behind the last item - into a stage nobody fills any more, never used: the fragment
            //  registers then have ONE definition per iteration and the compiler keeps them where they are)
            const uint32_t nst = lds0 + ((sc + 1) & (NSTG - 1)) * STAGE;
#pragma unroll
            for (int s_ = 0; s_ < 4; ++s_) {
                asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(F[2 * s_]), "+v"(F[2 * s_ + 1]));       // (the six younger reads: the three k-steps behind)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&F[2 * s_ + 1]), *reinterpret_cast<const bf16x8*>(&F[2 * s_]), acc, 0, 0, 0);
                PA_RD128(F[2 * s_], nst + fa_off + xs[s_]); PA_RD128(F[2 * s_ + 1], nst + fb_off + xs[s_]);
            }
        }
        sc = (sc + 1) & (NSTG - 1);
        if (++cc_t >= nt) {
            PA_TR3(3);
            epilogue(cun);
#ifdef PA_GEMM_TRACE3
            PA_TR3(5);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
            PA_TR3(4);
            cc_u += ustride; cc_t = 0;
            if (cc_u < p.units) unit_of(cc_u, cun);
        }
        --pending;
        if (!has_next) break;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(F[0]), "+v"(F[1]), "+v"(F[2]), "+v"(F[3]), "+v"(F[4]), "+v"(F[5]), "+v"(F[6]), "+v"(F[7]));
#undef PA_RD128
}

// -------------------------------------------------------------------------------------------------
// Wide-tile ring kernel: (64*FM) x (64*FN) x 64 tiles, 2 x 2 waves with FM x FN 32x32 MFMA tiles each, for the large
// multi-round Linears (N >= 1024).  With FM = 2, FN = 4 (128 x 256) a k-step is 8 MFMAs against 6 fragment reads, so the
// LDS traffic per flop drops by a third against the 128 x 128 kernels and the MFMA pipe, not LDS, bounds the K loop.
// 3-stage ring (3 x 48 KB) + 4 KB staging per wave.  bf16, both operands k-contiguous, K % 64 == 0, no split-K.
template <int FM, int FN>
__global__ __launch_bounds__(NT, 1) void gemm3w_kernel(GemmP p) {
    using T = bf16;
    constexpr int TBM = 64 * FM, TBN = 64 * FN;
    constexpr int RB = 128, NCH = 8;
    constexpr int A_BYTES = TBM * RB, B_BYTES = TBN * RB;
    constexpr int NLA = TBM * NCH / NT, NLB = TBN * NCH / NT, NLD = NLA + NLB;      // 16-byte DMA chunks per thread per item
    constexpr int NSTG = 3, STAGE = A_BYTES + B_BYTES, EPI = 32 * 32 * 4;
    static_assert(NSTG * STAGE + 4 * EPI <= 160 * 1024, "LDS budget");
    __shared__ __attribute__((aligned(256))) char smem[NSTG * STAGE + 4 * EPI];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5;
    constexpr int esz = 2;
    f32x16 acc[FN][FM];
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    uint32_t offA[NLA], offB[NLB];
    const char* kA = nullptr; const char* kB = nullptr;
    auto setup = [&](const Unit& un) {
        kA = reinterpret_cast<const char*>(p.A) + (size_t)un.b * p.sA * esz;
        kB = reinterpret_cast<const char*>(p.B) + (size_t)un.b * p.sB * esz;
        const int m0 = un.tile_m * TBM, n0 = un.tile_n * TBN;
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            const int pidx = tid + i * NT, row = pidx / NCH, ch = ((pidx % NCH) ^ (row / 2)) & (NCH - 1);
            offA[i] = (uint32_t)min(m0 + row, p.M - 1) * (uint32_t)(p.lda * esz) + ch * 16;
        }
#pragma unroll
        for (int i = 0; i < NLB; ++i) {
            const int pidx = tid + i * NT, row = pidx / NCH, ch = ((pidx % NCH) ^ (row / 2)) & (NCH - 1);
            offB[i] = (uint32_t)min(n0 + row, p.N - 1) * (uint32_t)(p.ldb * esz) + ch * 16;
        }
    };
    // chunk c of an item's DMA: c < NLA -> A chunk c, else B chunk c - NLA
    auto fetch_c = [&](int stage, auto C_) {
        constexpr int c = decltype(C_)::value;
        char* lx = smem + stage * STAGE + (c < NLA ? 0 : A_BYTES);
        constexpr int i = c < NLA ? c : c - NLA;
        const char* src = (c < NLA) ? kA + offA[i] : kB + offB[i];
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
            (__attribute__((address_space(3))) void*)(lx + (i * NT + wave * 64) * 16), 16, 0, 0);
    };
    auto fetch_done = [&]() { kA += 64 * esz; kB += 64 * esz; };
    auto fetch_range = [&](int stage, auto LO_, auto HI_) {
        constexpr int LO = decltype(LO_)::value, HI = decltype(HI_)::value;
        static_for<LO, HI>([&](auto I_) { fetch_c(stage, I_); });
    };
    auto fetch = [&](int stage) {
        fetch_range(stage, std::integral_constant<int, 0>{}, std::integral_constant<int, NLD>{});
        fetch_done();
    };

    const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)smem);
    const int sw = ((lane & 31) >> 1) & 7;
    uint32_t xs[4];
#pragma unroll
    for (int s_ = 0; s_ < 4; ++s_) xs[s_] = (uint32_t)((((2 * s_ + half) ^ sw) & 7) << 4);
    const uint32_t fa_off = (wm * 32 * FM + (lane & 31)) * RB, fb_off = (wn * 32 * FN + (lane & 31)) * RB + A_BYTES;
#define PA_RD128O(dst, addr, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF))
    // fragment W of k-step s: W < FM -> A row group W, else B row group W - FM
    auto rd1 = [&](u32x4 (&f)[FM + FN], uint32_t st, int s_, auto W_) {
        constexpr int W = decltype(W_)::value;
        if constexpr (W < FM) { const uint32_t ad = st + fa_off + xs[s_]; PA_RD128O(f[W], ad, W * 32 * RB); }
        else { const uint32_t ad = st + fb_off + xs[s_]; PA_RD128O(f[W], ad, (W - FM) * 32 * RB); }
    };
    auto frag = [&](u32x4 (&f)[FM + FN], uint32_t st, int s_) {
        static_for<0, FM + FN>([&](auto I_) { rd1(f, st, s_, I_); });
    };
    auto wait_frag = [&](u32x4 (&f)[FM + FN]) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < FM + FN; ++i) asm volatile("" : "+v"(f[i]));
    };

    // ---- epilogue: one 32 x 32 accumulator tile at a time through a 4 KB per-wave staging slice ------------------------
    auto epilogue = [&](const Unit& un) {
        char* stage = smem + NSTG * STAGE + wave * EPI;
        const size_t cbase = (size_t)un.b * p.sC;
        const int chunk = lane & 7, rsub = lane >> 3;
        const bool out_f32 = p.out_dtype == PA_F32;
        const bool has_bias = p.bias != nullptr, has_aux = p.aux != nullptr, has_res = p.R != nullptr, has_drop = p.drop_thr != 0;
        constexpr int NIT = 4;
        // bf16 residual / gate rows of ALL of the wave's 32 x 32 tiles are requested before the first tile is staged (round 6: each
        // of the FM x FN passes used to start with its own loads - one memory round trip per pass, most of this kernel's fixed cost)
        const bool pre_ok = p.vec_ok && !out_f32 && (has_res || has_aux) && (un.tile_n * TBN + (wn * FN + FN) * 32 <= p.N);
        u32x2 pres[FN * FM][NIT], paux[FN * FM][NIT];
        if (pre_ok) {
#pragma unroll
            for (int fn = 0; fn < FN; ++fn)
#pragma unroll
                for (int fm = 0; fm < FM; ++fm)
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        const int m = min(un.tile_m * TBM + (wm * FM + fm) * 32 + rsub + it * 8, p.M - 1);
                        const int n = un.tile_n * TBN + (wn * FN + fn) * 32 + chunk * 4;
                        if (has_res) pres[fn * FM + fm][it] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16*>(p.R) + (size_t)un.b * p.sR + (size_t)m * p.ldr + n);
                        if (has_aux) paux[fn * FM + fm][it] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16*>(p.aux) + (size_t)un.b * p.sAux + (size_t)m * p.ldaux + n);
                    }
        }
        auto widen2 = [](const u32x2& u) { f32x4 r; r[0] = bf16_lo(u[0]); r[1] = bf16_hi(u[0]); r[2] = bf16_lo(u[1]); r[3] = bf16_hi(u[1]); return r; };
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) {
            const int nw = un.tile_n * TBN + (wn * FN + fn) * 32;
            const int n = nw + chunk * 4;
            const bool fast = p.vec_ok && (nw + 32 <= p.N);
            f32x4 bias = {0.f, 0.f, 0.f, 0.f};
            if (has_bias) {
                const float* bp = p.bias + (size_t)un.b * p.sBias;
                if (fast) bias = *reinterpret_cast<const f32x4*>(bp + n);
                else { for (int e = 0; e < 4; ++e) if (n + e < p.N) bias[e] = bp[n + e]; }
            }
#pragma unroll
            for (int fm = 0; fm < FM; ++fm) {
                const int mw = un.tile_m * TBM + (wm * FM + fm) * 32;
                {
                    const int lrow = lane & 31;
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = acc[fn][fm][4 * g4 + e];
                        const int ch = 2 * g4 + half;
                        *reinterpret_cast<f32x4*>(stage + lrow * 128 + ((ch ^ (lrow & 7)) << 4)) = v;
                    }
                }
                f32x4 x[NIT];
                const int mp = mw + rsub;
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int lr = it * 8 + rsub;
                    x[it] = *reinterpret_cast<const f32x4*>(stage + lr * 128 + ((chunk ^ (lr & 7)) << 4));
                }
                if (fast) {
                    f32x4 res[NIT], gate[NIT];
                    if (pre_ok) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) {
                            if (has_res) res[it] = widen2(pres[fn * FM + fm][it]);
                            if (has_aux) gate[it] = widen2(paux[fn * FM + fm][it]);
                        }
                    } else {
                        if (has_res) {
#pragma unroll
                            for (int it = 0; it < NIT; ++it) {
                                const size_t ro = (size_t)un.b * p.sR + (size_t)min(mp + it * 8, p.M - 1) * p.ldr + n;
                                res[it] = out_f32 ? ld4<float>(reinterpret_cast<const float*>(p.R) + ro)
                                                  : ld4<bf16>(reinterpret_cast<const bf16*>(p.R) + ro);
                            }
                        }
                        if (has_aux) {
#pragma unroll
                            for (int it = 0; it < NIT; ++it) {
                                const size_t ao = (size_t)un.b * p.sAux + (size_t)min(mp + it * 8, p.M - 1) * p.ldaux + n;
                                gate[it] = ld4<T>(reinterpret_cast<const T*>(p.aux) + ao);
                            }
                        }
                    }
                    // one straight-line loop per optional stage behind its own uniform branch; stores with the output type and the
                    // row test decided once (see gemm3_kernel)
#pragma unroll
                    for (int it = 0; it < NIT; ++it)
#pragma unroll
                        for (int e = 0; e < 4; ++e) x[it][e] = x[it][e] * p.alpha + bias[e];
                    if (p.relu) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it)
#pragma unroll
                            for (int e = 0; e < 4; ++e) x[it][e] = fmaxf(x[it][e], 0.f);
                    }
                    if (has_aux) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it)
#pragma unroll
                            for (int e = 0; e < 4; ++e) x[it][e] = gate[it][e] > 0.f ? x[it][e] * p.aux_scale : 0.f;
                    }
                    if (has_drop) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                x[it][e] = drop_keep_rc(p.drop_seed, (uint32_t)(un.b * p.M + mp + it * 8), (uint32_t)(n + e), p.drop_thr) ? x[it][e] * p.drop_scale : 0.f;
                            }
                    }
                    if (has_res) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it)
#pragma unroll
                            for (int e = 0; e < 4; ++e) x[it][e] += res[it][e];
                    }
                    {
                        const bool interior = mw + 32 <= p.M;                          // wave-uniform
                        const size_t co0 = cbase + (size_t)mp * p.ldc + n, rstep = (size_t)8 * p.ldc;
                        if (out_f32) {
                            float* cp = reinterpret_cast<float*>(p.C) + co0;
                            if (interior) {
#pragma unroll
                                for (int it = 0; it < NIT; ++it) *reinterpret_cast<f32x4*>(cp + it * rstep) = x[it];
                            } else {
#pragma unroll
                                for (int it = 0; it < NIT; ++it) if (mp + it * 8 < p.M) *reinterpret_cast<f32x4*>(cp + it * rstep) = x[it];
                            }
                        } else {
                            bf16* cp = reinterpret_cast<bf16*>(p.C) + co0;
                            if (interior) {
#pragma unroll
                                for (int it = 0; it < NIT; ++it) st4<bf16>(cp + it * rstep, x[it]);
                            } else {
#pragma unroll
                                for (int it = 0; it < NIT; ++it) if (mp + it * 8 < p.M) st4<bf16>(cp + it * rstep, x[it]);
                            }
                        }
                    }
                } else {
#pragma unroll 1
                    for (int it = 0; it < NIT; ++it) {
                        const int m = mp + it * 8;
                        if (m >= p.M) continue;
                        for (int e = 0; e < 4; ++e) {
                            if (n + e >= p.N) continue;
                            float y = x[it][e] * p.alpha + bias[e];
                            if (p.relu) y = fmaxf(y, 0.f);
                            if (has_aux) {
                                const float g = ld1(reinterpret_cast<const T*>(p.aux) + (size_t)un.b * p.sAux + (size_t)m * p.ldaux + n + e);
                                y = g > 0.f ? y * p.aux_scale : 0.f;
                            }
                            if (has_drop) {
                                y = drop_keep_rc(p.drop_seed, (uint32_t)(un.b * p.M + m), (uint32_t)(n + e), p.drop_thr) ? y * p.drop_scale : 0.f;
                            }
                            if (has_res) {
                                const size_t ro = (size_t)un.b * p.sR + (size_t)m * p.ldr + n + e;
                                y += out_f32 ? reinterpret_cast<const float*>(p.R)[ro] : (float)reinterpret_cast<const bf16*>(p.R)[ro];
                            }
                            const size_t co = cbase + (size_t)m * p.ldc + n + e;
                            if (out_f32) reinterpret_cast<float*>(p.C)[co] = y;
                            else reinterpret_cast<bf16*>(p.C)[co] = (bf16)y;
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[fn][fm][r] = 0.f;
            }
        }
    };

    // ---- item stream: DMA cursor NSTG - 1 = 2 items ahead; units in XCD-interleaved order over the row tiles ------------
    const int ustride = gridDim.x, nt = p.K / 64;
    auto unit_of = [&](int u, Unit& un) -> bool {
        const int per_b = p.tiles_m_pad * p.tiles_n;
        un.b = u / per_b; un.z = un.b;
        const int r = u - un.b * per_b;
        const int xcd = r & 7, i = r >> 3, q = i / p.tiles_n;
        un.tile_n = i - q * p.tiles_n; un.tile_m = q * 8 + xcd;
        un.t_begin = 0; un.t_end = nt;
        return un.tile_m < p.tiles_m;
    };
    auto seek = [&](int u, Unit& un) -> int { while (u < p.units && !unit_of(u, un)) u += ustride; return u; };
    Unit cun, dun;
    int cc_u = seek(blockIdx.x, cun), cc_t = 0;
    if (cc_u >= p.units) return;
    int cd_u = seek(blockIdx.x, dun), cd_t = 0;
    setup(dun);
    int sd = 0, pending = 0;
    auto issue = [&]() {
        fetch(sd);
        sd = sd + 1 == NSTG ? 0 : sd + 1;
        ++pending;
        if (++cd_t >= nt) { cd_u = seek(cd_u + ustride, dun); cd_t = 0; if (cd_u < p.units) setup(dun); }
    };
    auto wait_items = [&](int younger) {        // items are NLD DMA instructions each
        if (younger >= 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NLD) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
#pragma unroll 1
    for (int k = 0; k < NSTG - 1; ++k) if (cd_u < p.units) issue();
    wait_items(pending - 1);
    __builtin_amdgcn_s_barrier();
    int sc = 0;
    u32x4 F0[FM + FN], F1[FM + FN];
    frag(F0, lds0, 0);
    auto mma_all = [&](u32x4 (&f)[FM + FN]) {
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
#pragma unroll
            for (int fm = 0; fm < FM; ++fm) mma16B<T>(acc[fn][fm], f[FM + fn], f[fm]);
    };
    auto item = [&](auto HOT_) -> bool {
        constexpr bool HOT = decltype(HOT_)::value;
        const uint32_t st = lds0 + sc * STAGE;
        __builtin_amdgcn_s_barrier();           // barrier A: the previous item's stage may be refilled
        if constexpr (!HOT) { if (cd_u < p.units) issue(); }
        constexpr int Q = (NLD + 2) / 3;        // DMA chunks per k-step in the hot loop (all issued by the end of k-step 2)
        wait_frag(F0); frag(F1, st, 1); mma_all(F0);
        if constexpr (HOT) fetch_range(sd, std::integral_constant<int, 0>{}, std::integral_constant<int, Q>{});
        wait_frag(F1); frag(F0, st, 2); mma_all(F1);
        if constexpr (HOT) fetch_range(sd, std::integral_constant<int, Q>{}, std::integral_constant<int, (2 * Q < NLD ? 2 * Q : NLD)>{});
        wait_frag(F0); frag(F1, st, 3); mma_all(F0);
        if constexpr (HOT) {
            fetch_range(sd, std::integral_constant<int, (2 * Q < NLD ? 2 * Q : NLD)>{}, std::integral_constant<int, NLD>{});
            fetch_done(); sd = sd + 1 == NSTG ? 0 : sd + 1; ++cd_t;
        }
        const bool has_next = HOT || pending >= 2;
        wait_frag(F1);
        if (has_next) {
            if constexpr (HOT) wait_items(1); else wait_items(pending - 2);
            __builtin_amdgcn_s_barrier();       // barrier B: the next item has landed for every wave
        }
        frag(F0, lds0 + (sc + 1 == NSTG ? 0 : sc + 1) * STAGE, 0);      // (unconditional: one definition of F0 on every path, see gemm3_kernel)
        mma_all(F1);
        sc = sc + 1 == NSTG ? 0 : sc + 1;
        if constexpr (HOT) { ++cc_t; return true; }
        else {
            if (++cc_t >= nt) {
                epilogue(cun);
                cc_t = 0;
                if (has_next) cc_u = seek(cc_u + ustride, cun);
            }
            --pending;
            return has_next;
        }
    };
#pragma unroll 1
    while (true) {
        int hot = (pending == NSTG - 1 && cd_u == cc_u) ? (nt - cd_t - 1) : 0;
#pragma unroll 1
        for (; hot > 0; --hot) item(std::true_type{});
        if (!item(std::false_type{})) break;
    }
#undef PA_RD128O
}

#include "gemm8.h"

// split-K second pass: sum the slabs and apply the epilogue
// -------------------------------------------------------------------------------------------------
// "Skinny" Linear: a few hundred rows (greedy decode: M = batch 256) against a whole weight.  The tiled kernels above give
// such a launch 8 ... 32 blocks that each walk K in a serial chain of small DMA -> barrier -> MFMA steps; in f32 (the
// token-exact decode path) that chain is 32 ... 64 steps of 16 columns on 8 blocks: 43 ... 98 us per Linear, 60 % of the f32
// decode step (profiles/r03_decode_f32_kernel_trace_summary.txt).  Here a block owns a 32 x 32 output tile and K is cut into
// chunks of 1 KB per operand row (256 f32 / 512 bf16); the first TWO chunks - all of K = 512 in f32, K = 1 024 in bf16 - are
// requested before anything is waited for (direct-to-LDS DMA, one instruction per operand row and chunk: 64 lanes x 16 B),
// so a block pays one memory round trip instead of a chain of them.  M 256 x N 512 -> 128 blocks, N 1 536 -> 384.
// The four waves split each chunk's K range; their partial 32 x 32 accumulators are summed through LDS in a fixed order
// (deterministic).  LDS rows are padded to 1 040 B: a 16-lane phase of ds_read_b128 then covers all 64 banks.
// Epilogue = the other kernels' (alpha, bias, ReLU, residual in the output type); no gate / dropout (the dispatcher keeps
// those on the tiled kernels).
constexpr int SK_T = 32, SK_ROW = 1024, SK_STRIDE = SK_ROW + 16, SK_STAGE = 2 * SK_T * SK_STRIDE, SK_NSTG = 2;
constexpr int SK_RED = 33 * 4;                       // row stride of the reduction buffer (f32, padded)

// LN = true (bf16, K = one chunk = 512): A = LayerNorm(Z) folded into the product as in gemm3s_kernel's p.ln_u form - the weight is
// pre-multiplied by gamma, the block takes mean / rstd of its 32 rows from the Z tile that is resident in LDS anyway (no extra
// memory round trip: the reason the fold did not pay on the ring kernel), the epilogue applies
// rstd (acc - mean u) + v, and the blocks of column tile 0 materialise LayerNorm(Z) for the later residual add.
template <typename T, bool LN>
__global__ __launch_bounds__(256, 1) void gemm_skinny_kernel(GemmP p) {
    constexpr int esz = sizeof(T);
    constexpr int CH = SK_ROW / esz;                 // K elements per chunk
    __shared__ __attribute__((aligned(256))) char smem[SK_NSTG * SK_STAGE + 256];       // + [32] mean | [32] rstd behind the stages
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tm = blockIdx.x / p.tiles_n, tn = blockIdx.x - tm * p.tiles_n;      // neighbouring blocks share the A rows
    const int m0 = tm * SK_T, n0 = tn * SK_T;
    const int nch = p.K / CH;
    // ---- everything the epilogue needs from memory is requested FIRST (ordinary loads, older than every DMA below, so the
    // hand-counted vmcnt waits - loads return in order - also cover them): bias / u / residual / gamma / beta of this thread's
    // one row x four columns.  A load at the end would be a second, fully exposed memory round trip.
    const int er = tid >> 3, ec = (tid & 7) * 4;
    const int em = m0 + er, en = n0 + ec;
    const bool out_f32 = p.out_dtype == PA_F32;
    const bool in_tile = em < p.M && en < p.N;
    const bool full = en + 3 < p.N;
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f}, u4 = {0.f, 0.f, 0.f, 0.f}, res4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 gam4 = {0.f, 0.f, 0.f, 0.f}, bet4 = {0.f, 0.f, 0.f, 0.f};
    if (in_tile) {
        if (full && p.vec_ok) {
            if (p.bias) bias4 = *reinterpret_cast<const f32x4*>(p.bias + en);
            if (LN) u4 = *reinterpret_cast<const f32x4*>(p.ln_u + en);
            if (p.R) {
                const size_t ro = (size_t)em * p.ldr + en;
                res4 = out_f32 ? *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.R) + ro)
                               : ld4<bf16>(reinterpret_cast<const bf16*>(p.R) + ro);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (en + e < p.N) {
                    if (p.bias) bias4[e] = p.bias[en + e];
                    if (LN) u4[e] = p.ln_u[en + e];
                    if (p.R) {
                        const size_t ro = (size_t)em * p.ldr + en + e;
                        res4[e] = out_f32 ? reinterpret_cast<const float*>(p.R)[ro] : (float)reinterpret_cast<const bf16*>(p.R)[ro];
                    }
                }
        }
    }
    // LN: column tile tn materialises columns 32 tn .. 32 tn + 31 of LayerNorm(Z) (N >= K is checked by the host)
    const bool write_y = LN && p.ln_y != nullptr && n0 < p.K && em < p.M;
    if (write_y) { gam4 = *reinterpret_cast<const f32x4*>(p.ln_gamma + en); bet4 = *reinterpret_cast<const f32x4*>(p.ln_beta + en); }
    // f32 residual stream (p.ln_zf): A is only the bf16 copy of the f32 rows Z.  The statistics and LayerNorm(Z) come from the f32
    // rows, requested here with the other epilogue inputs (older than every DMA): lane -> (row 8w + l / 8, eighth l % 8), elements
    // 64 j + 8 (l % 8) .. + 7 for j = 0 .. 7 - the elements the bf16 path reads from the resident tile.
    const bool zf_on = LN && p.ln_zf != nullptr;                        // (kernel-uniform)
    f32x4 zfr[16], zy4 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (LN) {
        if (zf_on) {
            const float* zrow = p.ln_zf + (size_t)min(m0 + wave * 8 + (lane >> 3), p.M - 1) * p.ldzf + (lane & 7) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                zfr[2 * j] = *reinterpret_cast<const f32x4*>(zrow + j * 64);
                zfr[2 * j + 1] = *reinterpret_cast<const f32x4*>(zrow + j * 64 + 4);
            }
            if (write_y) zy4 = *reinterpret_cast<const f32x4*>(p.ln_zf + (size_t)em * p.ldzf + en);
        }
    }

    const char* gA = reinterpret_cast<const char*>(p.A) + (size_t)lane * 16;
    const char* gB = reinterpret_cast<const char*>(p.B) + (size_t)lane * 16;
    // wave w moves rows 8w .. 8w + 7 of both operands: 16 DMA instructions per chunk and wave
    auto issue = [&](int c, int stage) {
        char* base = smem + stage * SK_STAGE;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = wave * 8 + i;
            const char* sa = gA + ((size_t)min(m0 + r, p.M - 1) * p.lda + (size_t)c * CH) * esz;
            const char* sb = gB + ((size_t)min(n0 + r, p.N - 1) * p.ldb + (size_t)c * CH) * esz;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)sa,
                (__attribute__((address_space(3))) void*)(base + r * SK_STRIDE), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)sb,
                (__attribute__((address_space(3))) void*)(base + (SK_T + r) * SK_STRIDE), 16, 0, 0);
        }
    };
    issue(0, 0);
    if (nch > 1) issue(1, 1);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int half = lane >> 5, row = lane & 31;
    // this wave's quarter of a chunk, this lane's 16 bytes of every 32-byte (f32: 8 k, bf16: 16 k) group
    const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)smem);
    const uint32_t offA = (uint32_t)(row * SK_STRIDE + wave * (SK_ROW / 4) + half * 16);
    const uint32_t offB = offA + SK_T * SK_STRIDE;
    float* stats = reinterpret_cast<float*>(smem + SK_NSTG * SK_STAGE);   // LN: [32] mean | [32] rstd
    for (int c = 0; c < nch; ++c) {
        const int stage = c & 1;
        // counted wait + raw barrier (a __syncthreads() would also drain the newer chunk's DMA): chunk c has landed for every wave
        if (c + 1 < nch) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const uint32_t la = lds0 + stage * SK_STAGE + offA, lb = lds0 + stage * SK_STAGE + offB;
#define SK_RD(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:" #off : "=v"(dst) : "v"(addr) : "memory")
        f32x4 a[8], b[8];
        SK_RD(a[0], la, 0);   SK_RD(b[0], lb, 0);   SK_RD(a[1], la, 32);  SK_RD(b[1], lb, 32);
        SK_RD(a[2], la, 64);  SK_RD(b[2], lb, 64);  SK_RD(a[3], la, 96);  SK_RD(b[3], lb, 96);
        SK_RD(a[4], la, 128); SK_RD(b[4], lb, 128); SK_RD(a[5], la, 160); SK_RD(b[5], lb, 160);
        SK_RD(a[6], la, 192); SK_RD(b[6], lb, 192); SK_RD(a[7], la, 224); SK_RD(b[7], lb, 224);
        if (LN && c == 0) {
            // (f32 operands - two K chunks - take their statistics from the f32 rows in global memory: pa_gemm_norm_a requires zf)
            // row statistics from the resident Z tile, all 8 rows of this wave at once: lane -> (row 8w + l / 8, eighth l % 8), 64
            // elements per lane, two passes over them in registers, three lane exchanges per pass.  Issued between the fragment
            // reads and their use: the MFMAs below do not wait for it.
            const int sr = wave * 8 + (lane >> 3), part = lane & 7;
            float s1 = 0.f, s2 = 0.f, mean = 0.f;
            if (zf_on) {
#pragma unroll
                for (int j = 0; j < 16; ++j) s1 += (zfr[j][0] + zfr[j][1]) + (zfr[j][2] + zfr[j][3]);
                s1 += __shfl_xor(s1, 1); s1 += __shfl_xor(s1, 2); s1 += __shfl_xor(s1, 4);
                mean = s1 * (1.0f / (float)p.K);
#pragma unroll
                for (int j = 0; j < 16; ++j)
#pragma unroll
                    for (int w = 0; w < 4; ++w) { const float d0 = zfr[j][w] - mean; s2 += d0 * d0; }
            } else if constexpr (sizeof(T) == 2) {
                const uint32_t lz = lds0 + (uint32_t)(sr * SK_STRIDE + part * 16);
                u32x4 zz[8];
                SK_RD(zz[0], lz, 0);   SK_RD(zz[1], lz, 128); SK_RD(zz[2], lz, 256); SK_RD(zz[3], lz, 384);
                SK_RD(zz[4], lz, 512); SK_RD(zz[5], lz, 640); SK_RD(zz[6], lz, 768); SK_RD(zz[7], lz, 896);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(zz[0]), "+v"(zz[1]), "+v"(zz[2]), "+v"(zz[3]), "+v"(zz[4]), "+v"(zz[5]), "+v"(zz[6]), "+v"(zz[7]));
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int w = 0; w < 4; ++w) s1 += bf16_lo(zz[j][w]) + bf16_hi(zz[j][w]);
                s1 += __shfl_xor(s1, 1); s1 += __shfl_xor(s1, 2); s1 += __shfl_xor(s1, 4);
                mean = s1 * (1.0f / (float)p.K);
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const float d0 = bf16_lo(zz[j][w]) - mean, d1 = bf16_hi(zz[j][w]) - mean;
                        s2 += d0 * d0 + d1 * d1;
                    }
            }
            s2 += __shfl_xor(s2, 1); s2 += __shfl_xor(s2, 2); s2 += __shfl_xor(s2, 4);
            if (part == 0) { stats[sr] = mean; stats[32 + sr] = rsqrtf(s2 * (1.0f / (float)p.K) + p.ln_eps); }
        }
#undef SK_RD
        // (the operands are tied to the wait, or the MFMAs - plain builtins - could be scheduled above it)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]),
                                               "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if constexpr (esz == 4) {
#pragma unroll
                for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j][t], b[j][t], acc, 0, 0, 0);
            } else {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[j]), __builtin_bit_cast(bf16x8, b[j]), acc, 0, 0, 0);
            }
        }
        if (c + 2 < nch) {                            // the stage is free once every wave has read it (lgkmcnt(0) above)
            __builtin_amdgcn_s_barrier();
            issue(c + 2, stage);
        }
    }
    // ---- sum the four K-quarters through LDS (fixed order), then the epilogue: thread -> one row, four columns -------------
    // LN: the reduction buffer lives in the unused second stage (behind the statistics), so the Z tile in stage 0 stays readable
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem + ((LN && sizeof(T) == 2) ? SK_STAGE : 0));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rr = (r >> 2) * 8 + half * 4 + (r & 3);
        red[wave * (SK_T * 33) + rr * 33 + row] = acc[r];
    }
    float ln_mean = 0.f, ln_rstd = 1.f;
    if constexpr (LN) {
        ln_mean = stats[er]; ln_rstd = stats[32 + er];
        if (write_y) {
            f32x4 zv;
            if (zf_on) zv = zy4;
            else if constexpr (sizeof(T) == 2) {
                const u32x2 zq = *reinterpret_cast<const u32x2*>(smem + er * SK_STRIDE + (size_t)en * 2);
                zv[0] = bf16_lo(zq[0]); zv[1] = bf16_hi(zq[0]); zv[2] = bf16_lo(zq[1]); zv[3] = bf16_hi(zq[1]);
            }
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = (zv[e] - ln_mean) * ln_rstd * gam4[e] + bet4[e];
            if (p.ln_y_f32) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.ln_y) + (size_t)em * p.ldy + en) = y;
            else st4<bf16>(reinterpret_cast<bf16*>(p.ln_y) + (size_t)em * p.ldy + en, y);
        }
    }
    __syncthreads();
    if (!in_tile) return;
    f32x4 x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float* q = red + er * 33 + ec + e;
        x[e] = ((q[0] + q[SK_T * 33]) + q[2 * SK_T * 33]) + q[3 * SK_T * 33];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float y = LN ? ln_rstd * (x[e] * p.alpha - ln_mean * u4[e]) + bias4[e] : x[e] * p.alpha + bias4[e];
        if (p.relu) y = fmaxf(y, 0.f);
        x[e] = y + res4[e];
    }
    const size_t co = (size_t)em * p.ldc + en;
    if (full && p.vec_ok) {
        if (out_f32) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + co) = x;
        else st4<bf16>(reinterpret_cast<bf16*>(p.C) + co, x);
        if (p.c_lp) st4<bf16>(reinterpret_cast<bf16*>(p.c_lp) + (size_t)em * p.ldc_lp + en, x);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (en + e < p.N) {
                if (out_f32) reinterpret_cast<float*>(p.C)[co + e] = x[e];
                else reinterpret_cast<bf16*>(p.C)[co + e] = (bf16)x[e];
                if (p.c_lp) reinterpret_cast<bf16*>(p.c_lp)[(size_t)em * p.ldc_lp + en + e] = (bf16)x[e];
            }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmP p, const float* ws) {
    const size_t total = (size_t)p.batch * p.M * p.N;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int n = (int)(e % p.N);
        const size_t bm = e / p.N;
        const int m = (int)(bm % p.M), b = (int)(bm / p.M);
        float v = 0.f;
        for (int s = 0; s < p.splitk; ++s) v += ws[(((size_t)b * p.splitk + s) * p.M + m) * p.N + n];
        v = v * p.alpha + (p.bias ? p.bias[(size_t)b * p.sBias + n] : 0.f);      // (per-batch bias stride, as in the tile epilogues)
        if (p.relu) v = fmaxf(v, 0.f);
        if (p.aux) {
            float g = ld1(reinterpret_cast<const T*>(p.aux) + (size_t)b * p.sAux + (size_t)m * p.ldaux + n);
            v = g > 0.f ? v * p.aux_scale : 0.f;
        }
        if (p.drop_thr) v = drop_keep_rc(p.drop_seed, (uint32_t)(b * p.M + m), (uint32_t)n, p.drop_thr) ? v * p.drop_scale : 0.f;
        const size_t co = (size_t)b * p.sC + (size_t)m * p.ldc + n;
        if (p.out_dtype == PA_F32) {
            if (p.R) v += reinterpret_cast<const float*>(p.R)[(size_t)b * p.sR + (size_t)m * p.ldr + n];
            reinterpret_cast<float*>(p.C)[co] = v;
        } else {
            if (p.R) v += (float)reinterpret_cast<const bf16*>(p.R)[(size_t)b * p.sR + (size_t)m * p.ldr + n];
            reinterpret_cast<bf16*>(p.C)[co] = (bf16)v;
        }
    }
}

// ---- host side: runtime switches and the helpers every launch site shares ---------------------------------------------------
// Every runtime switch of the GEMM dispatch: environment, read once per process, the defaults are the measured choices (the
// comments at the kernels and in plan_gemm say what was measured).  PA_RESERVE_CUS is not here: pa_set_reserved_cus changes it.
struct GemmSwitches {
    int nst;                       // PA_GEMM_NST: stages of the pair kernel, 0 auto, 1 / 3 forced
    int epre;                      // PA_GEMM_EPRE: 0 turns the pair kernel's epilogue-prefetch variant off
    int bk;                        // PA_GEMM_BK: bf16 K tile of the pair kernel, 64 or 32
    int noglds;                    // PA_GEMM_NOGLDS: 1 = no direct-to-LDS loads (pair kernel only then)
    int grid;                      // PA_GEMM_GRID: blocks of a pair launch per 256 CUs (0 = one block per unit)
    int dbg;                       // PA_GEMM_DBG: timing-ablation bits of -DPA_GEMM_ABLATE builds (wrong results)
    int v3;                        // PA_GEMM_V3: ring kernels 0 never, 1 single-round launches, 2 every eligible launch
    int small_on, small_max, small_max_k512;        // PA_GEMM_SMALL, PA_GEMM_SMALL_MAX, PA_GEMM_SMALL_MAX_K512
    int wide, tall;                // PA_GEMM_WIDE: 0 never, 1 every eligible launch, 2 single round; PA_GEMM_TALL: opt-in
    int skinny, skinny_rows, skinny_rows_f32;       // PA_GEMM_SKINNY: 0 never, 1 f32 only, 2 bf16 too; PA_GEMM_SKINNY_ROWS[_F32]
    int big, big_minm, big_minn, big_tn;            // PA_GEMM_BIG: 0 never, 1 / 2 tile-width rule; PA_GEMM_BIG_MINM / _MINN / _TN
    int dw_xcd;                    // PA_DW_XCD: 0 = plain slot order in the grouped weight-gradient launch
};
const GemmSwitches& gemm_switches() {
    static const GemmSwitches sw = [] {
        auto env = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        GemmSwitches s;
        s.nst = env("PA_GEMM_NST", 0);
        s.epre = env("PA_GEMM_EPRE", 1);
        s.bk = env("PA_GEMM_BK", 64);
        s.noglds = env("PA_GEMM_NOGLDS", 0);
        s.grid = env("PA_GEMM_GRID", s.nst == 1 ? 1024 : s.bk == 32 ? 768 : 512);      // (two blocks per CU by default)
        s.dbg = env("PA_GEMM_DBG", 0);
        s.v3 = env("PA_GEMM_V3", 1);
        s.small_on = env("PA_GEMM_SMALL", 1);
        s.small_max = env("PA_GEMM_SMALL_MAX", 128);
        s.small_max_k512 = env("PA_GEMM_SMALL_MAX_K512", 192);
        s.wide = env("PA_GEMM_WIDE", 2);
        s.tall = env("PA_GEMM_TALL", 0);
        s.skinny = env("PA_GEMM_SKINNY", 2);
        s.skinny_rows = env("PA_GEMM_SKINNY_ROWS", 512);
        s.skinny_rows_f32 = env("PA_GEMM_SKINNY_ROWS_F32", env("PA_GEMM_SKINNY_ROWS", 2048));
        s.big = env("PA_GEMM_BIG", 0);
        s.big_minm = env("PA_GEMM_BIG_MINM", 4096);
        s.big_minn = env("PA_GEMM_BIG_MINN", 256);
        s.big_tn = env("PA_GEMM_BIG_TN", 0);
        s.dw_xcd = env("PA_DW_XCD", 1);
        return s;
    }();
    return sw;
}

// Number of NON-EMPTY contraction slices for a requested split of `nt` K tiles: slices are whole tiles, and rounding the slice
// length up can leave trailing slices empty - those must not exist, their slabs would never be written.
inline int eff_splitk(int nt, int sk) {
    if (sk > nt) sk = nt;
    if (sk < 1) sk = 1;
    const int per = (nt + sk - 1) / sk;
    return (nt + per - 1) / per;
}

// Tile counts and unit order of one launch.  UNITS_XCD: units interleave the row tiles over the eight XCDs (rows padded to a multiple
// of 8) unless there are fewer than 8 row tiles - the interleave would leave most units empty; UNITS_XCD_ALWAYS: even then.
enum UnitOrder { UNITS_PLAIN, UNITS_XCD, UNITS_XCD_ALWAYS };
struct Tiling { int tiles_m, tiles_n, tiles_m_pad, plain_order, units; };
inline Tiling tiling_of(int M, int N, int tile_h, int tile_w, int batch_times_splitk, UnitOrder order) {
    Tiling t;
    t.tiles_m = (M + tile_h - 1) / tile_h;
    t.tiles_n = (N + tile_w - 1) / tile_w;
    t.plain_order = order == UNITS_PLAIN || (order == UNITS_XCD && t.tiles_m < 8);
    t.tiles_m_pad = t.plain_order ? t.tiles_m : (t.tiles_m + 7) / 8 * 8;
    t.units = t.tiles_m_pad * t.tiles_n * batch_times_splitk;
    return t;
}
inline void set_tiling(GemmP& p, const Tiling& t) {
    p.tiles_m = t.tiles_m; p.tiles_n = t.tiles_n; p.tiles_m_pad = t.tiles_m_pad; p.plain_order = t.plain_order; p.units = t.units;
}
inline void set_tiling(GemmP& p, int tile_h, int tile_w, int batch_times_splitk, UnitOrder order) {
    set_tiling(p, tiling_of(p.M, p.N, tile_h, tile_w, batch_times_splitk, order));
}

// 4-element vector accesses of an epilogue on `q` (element size esz, row stride ld, batch stride sb) are naturally aligned
inline bool vec_ok(const void* q, long long ld, long long sb, int esz) {
    return !q || ((reinterpret_cast<uintptr_t>(q) % (4 * esz) == 0) && (ld % 4 == 0) && (sb % 4 == 0));
}

// operands, shapes, strides and epilogue scalars of an argument block (everything a kernel reads that no launch site decides)
inline void fill_operands(GemmP& p, const pa_gemm_args& a) {
    p.A = a.A; p.B = a.B; p.C = a.C; p.bias = a.bias; p.R = a.R; p.aux = a.aux;
    p.M = a.M; p.N = a.N; p.K = a.K;
    p.lda = a.lda; p.ldb = a.ldb; p.ldc = a.ldc; p.ldr = a.ldr; p.ldaux = a.ldaux;
    p.sA = a.sA; p.sB = a.sB; p.sC = a.sC; p.sR = a.sR; p.sAux = a.sAux; p.sBias = a.sBias;
    p.batch = a.batch;
    p.alpha = a.alpha; p.relu = a.relu; p.aux_scale = a.aux_scale;
    p.drop_thr = a.drop_p > 0.f ? (uint32_t)((double)a.drop_p * 4294967296.0) : 0u;    // keep <=> 32-bit product >= thr (pa_device.h drop_keep_rc)
    p.drop_scale = (float)(1.0 / (1.0 - (double)p.drop_thr / 4294967296.0));
    p.drop_seed = a.drop_seed;
    p.out_dtype = a.out_dtype;
}

template <typename T, int BK_, int OCC, bool A_KC, bool B_KC>
int launch_t(const GemmP& p, bool aligned, bool glds, dim3 grid, hipStream_t st) {
    constexpr bool CAN_TR = sizeof(T) == 2 && BK_ == 64 && !(A_KC && B_KC);
    constexpr bool ALLD = (A_KC && B_KC) || CAN_TR;        // both operands DMA'd when glds is usable
    const GemmSwitches& sw = gemm_switches();
    const bool deep = ALLD && sizeof(T) == 2 && BK_ == 64 && sw.nst == 3;
    const bool flat = ALLD && sizeof(T) == 2 && BK_ == 64 && sw.nst == 1;
    if (aligned && glds) {
        if constexpr (ALLD && sizeof(T) == 4 && BK_ == 16) {
            // f32, both operands k-contiguous: a 3-stage ring (PA_GEMM_NST=3) was measured and LOSES - 33.9 vs 31.3 ms per f32
            // train step (round 4): these launches are not waiting for their K tiles.  Opt-in only.
            if (sw.nst == 3) {
                PA_LAUNCH((gemm_kernel<T, BK_, 2, A_KC, B_KC, true, true, false, 3>), grid, dim3(NT), 0, st, p);
                return 0;
            }
        }
        if constexpr (ALLD && sizeof(T) == 2 && BK_ == 64) {
            if (deep) {
                PA_LAUNCH((gemm_kernel<T, BK_, 1, A_KC, B_KC, true, true, CAN_TR, 3>), grid, dim3(NT), 0, st, p);
                return 0;
            }
            if (flat) {
                PA_LAUNCH((gemm_kernel<T, BK_, 4, A_KC, B_KC, true, true, CAN_TR, 1>), grid, dim3(NT), 0, st, p);
                return 0;
            }
        }
        if constexpr (ALLD && sizeof(T) == 2 && BK_ == 64) {
            // bf16 residual / gate rows, bf16 output: the variant that fetches them under the last K tile.  Back-to-back launches at
            // 8704 rows, with a residual: 512 x 512 16.4 -> 15.5 us, 512 x 1024 24.4 -> 21.5, 512 x 1536 31.0 -> 27.6, 1024 x 512
            // 31.1 -> 24.4, 1536 x 512 35.8 -> 28.9; strided weight 512 x 1536 38.2 -> 36.4.  PA_GEMM_EPRE=0 turns it off.
            if (sw.epre && (p.R || p.aux) && p.splitk == 1 && p.out_dtype != PA_F32 && p.vec_ok) {
                PA_LAUNCH((gemm_kernel<T, BK_, OCC, A_KC, B_KC, true, true, CAN_TR, 2, true>), grid, dim3(NT), 0, st, p);
                return 0;
            }
        }
        if constexpr (CAN_TR) PA_LAUNCH((gemm_kernel<T, BK_, OCC, A_KC, B_KC, true, true, true, 2>), grid, dim3(NT), 0, st, p);
        else if constexpr (A_KC || B_KC) PA_LAUNCH((gemm_kernel<T, BK_, OCC, A_KC, B_KC, true, true, false, 2>), grid, dim3(NT), 0, st, p);
        else PA_LAUNCH((gemm_kernel<T, BK_, OCC, A_KC, B_KC, true, false, false, 2>), grid, dim3(NT), 0, st, p);
    }
    else if (aligned) PA_LAUNCH((gemm_kernel<T, BK_, OCC, A_KC, B_KC, true, false, false, 2>), grid, dim3(NT), 0, st, p);
    else PA_LAUNCH((gemm_kernel<T, BK_, OCC, A_KC, B_KC, false, false, false, 2>), grid, dim3(NT), 0, st, p);
    return 0;
}
template <typename T, int BK_, int OCC>
int launch_layout(const GemmP& p, bool akc, bool bkc, bool aligned, bool glds, dim3 grid, hipStream_t st) {
    if (akc && bkc) return launch_t<T, BK_, OCC, true, true>(p, aligned, glds, grid, st);
    if (akc && !bkc) return launch_t<T, BK_, OCC, true, false>(p, aligned, glds, grid, st);
    if (!akc && bkc) return launch_t<T, BK_, OCC, false, true>(p, aligned, glds, grid, st);
    return launch_t<T, BK_, OCC, false, false>(p, aligned, glds, grid, st);
}

template <typename T> bool is_aligned(const pa_gemm_args* a) {
    constexpr int EB = ET<T>::EB;
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    bool ok = al16(a->A) && al16(a->B) && (a->lda % EB == 0) && (a->ldb % EB == 0) &&
              (a->sA % EB == 0) && (a->sB % EB == 0);
    // vectors run along K for k-contiguous operands, along the row index for transposed ones; a transposed operand
    // whose last vector straddles M (N) is fine when the row stride covers it: the extra elements only feed output
    // rows (columns) that are never stored
    ok = ok && (a->a_kcontig ? (a->K % EB == 0) : (a->lda >= (a->M + EB - 1) / EB * EB));
    ok = ok && (a->b_kcontig ? (a->K % EB == 0) : (a->ldb >= (a->N + EB - 1) / EB * EB));
    return ok;
}

// ---- which kernel, which grid ----------------------------------------------------------------------------------------------------
// plan_gemm / plan_norm_a are the whole rule, as pure functions of the argument block, the switches and the CUs a launch may use:
// they call no HIP function and dereference nothing (pa_gemm_plan runs them on a machine without a GPU).
enum GemmKernel { GK_PAIR, GK_RING, GK_SMALL, GK_WIDE, GK_TALL, GK_BIG, GK_SKINNY };
struct GemmPlan {
    int status;                    // what the call returns before it launches (0: it launches)
    int kind;                      // PA_GEMM_KIND_* the recorder reports
    GemmKernel kernel;             // what the launcher switches on
    int tile_h, tile_w;
    Tiling t;
    int splitk, tiles_per_slice;   // effective split-K
    int grid, block;
    int vec_ok;                    // the epilogue may use 4-element vector accesses
    int bk; bool aligned, glds;    // pair kernel: K tile depth, 16-byte operand loads, direct-to-LDS loads
};
inline GemmPlan plan_fail(int status) { GemmPlan pl = GemmPlan(); pl.status = status; return pl; }
inline void plan_kernel(GemmPlan& pl, int kind, GemmKernel kernel, const pa_gemm_args& a, int tile_h, int tile_w, int batch_times_splitk,
                        UnitOrder order, int max_blocks, int block) {
    pl.kind = kind; pl.kernel = kernel; pl.tile_h = tile_h; pl.tile_w = tile_w;
    pl.t = tiling_of(a.M, a.N, tile_h, tile_w, batch_times_splitk, order);
    pl.grid = pl.t.units < max_blocks ? pl.t.units : max_blocks;
    pl.block = block;
}

// Precedence: big -> (a C_lp nobody but the skinny kernel writes is rejected) -> skinny -> wide -> tall -> small -> ring -> pair.
GemmPlan plan_gemm(const pa_gemm_args& a, const GemmSwitches& sw, int cus) {
    if (!a.A || !a.B || !a.C || a.M <= 0 || a.N <= 0 || a.K <= 0 || a.batch <= 0) return plan_fail(PA_EINVAL);
    if (a.in_dtype != PA_F32 && a.in_dtype != PA_BF16) return plan_fail(PA_EINVAL);
    if (a.out_dtype != PA_F32 && a.out_dtype != PA_BF16) return plan_fail(PA_EINVAL);
    if (a.drop_p < 0.f || a.drop_p >= 1.f) return plan_fail(PA_EINVAL);
    if (a.C_lp && (a.out_dtype != PA_F32 || a.ldc_lp < a.N || a.ldc_lp % 4 || (reinterpret_cast<uintptr_t>(a.C_lp) & 7))) return plan_fail(PA_EINVAL);
    GemmPlan pl = GemmPlan();
    const bool bf = a.in_dtype == PA_BF16, bk32 = bf && sw.bk == 32;
    pl.bk = bf ? (bk32 ? 32 : 64) : 16;
    const int nt = (a.K + pl.bk - 1) / pl.bk;
    const int splitk = eff_splitk(nt, a.splitk);
    if (splitk > 1 && !a.ws) return plan_fail(PA_EINVAL);
    pl.splitk = splitk;
    pl.tiles_per_slice = (nt + splitk - 1) / splitk;
    // vector epilogue: 4-element accesses on C (the slab workspace under split-K) / R / aux / bias must be naturally aligned
    const int osz = (splitk > 1 || a.out_dtype == PA_F32) ? 4 : 2, isz = bf ? 2 : 4;
    pl.vec_ok = (splitk > 1 ? vec_ok(a.ws, a.N, (long long)a.M * a.N, osz) : vec_ok(a.C, a.ldc, a.sC, osz)) && vec_ok(a.R, a.ldr, a.sR, osz) &&
                vec_ok(a.aux, a.ldaux, a.sAux, isz) && vec_ok(a.bias, 4, a.sBias, 4);
    pl.aligned = bf ? is_aligned<bf16>(&a) : is_aligned<float>(&a);
    pl.glds = ((a.K % pl.bk) == 0 || (!a.a_kcontig && !a.b_kcontig && bf && !bk32)) && !sw.noglds;

    const Tiling base = tiling_of(a.M, a.N, BM, BN, a.batch * splitk, UNITS_XCD);
    const int valid_units = base.tiles_m * base.tiles_n * a.batch * splitk;
    const bool ring_ok = bf && !bk32 && !sw.noglds && pl.aligned;                                  // the ring kernels' operands
    const bool linear = a.a_kcontig && a.b_kcontig && splitk == 1 && a.K % 64 == 0;             // a plain Linear of whole 64-deep K tiles
    // ring (one block per CU, 4-stage ring) wins while the launch is a single round of units (latency-bound shapes); with more
    // rounds the two-blocks-per-CU pair kernel overlaps better.  PA_GEMM_V3=2 forces the ring for every eligible launch.
    const bool go_v3 = sw.v3 && (valid_units <= 256 || sw.v3 == 2) && ring_ok && ((!a.a_kcontig && !a.b_kcontig) || a.K % 64 == 0);
    // small (64 x 64 tiles): plain Linears whose 128 x 128 tiling covers at most half of the CUs (measured: <= 128 units 7.05 ms/step,
    // <= 64 7.11, <= 256 7.53).  Round 6, after the small kernel's K loop was repaired: up to 192 units too while K <= 512 - 2 048 x
    // 1 536 x 512: 12.0 -> 10.8 us; from K = 1 024 on the 128 x 128 ring is ahead there, 15.6 vs 16.5 us (profiles/r06_gemm_small_tile.txt)
    const bool go_small = go_v3 && sw.small_on && linear && (valid_units <= sw.small_max || (valid_units <= sw.small_max_k512 && a.K <= 512));
    // wide (128 x 256 tiles): by default when that tiling is a single round of blocks (7 940 x 1 024: 248 tiles - measured 15.5 us
    // against 16.8 for the pair kernel once the epilogues were restructured; at N = 1 536 the 378 tiles are a round and a half and the
    // pair kernel stays ahead).  PA_GEMM_WIDE=1, every eligible launch: 0.73 us per K tile (the best of the four kernels) but 14.8 us
    // fixed cost against 11.9 us, so at the model's K = 512 it loses (20.4 vs 18.5 us at 7 940 x 1 024) and only wins from K ~ 2 048 on.
    const long long wide_tiles = (long long)((a.M + 127) / 128) * ((a.N + 255) / 256) * a.batch;
    const bool go_wide = sw.v3 && sw.wide && (sw.wide == 1 || wide_tiles <= cus) && ring_ok && linear && a.N >= 1024 && valid_units > 256;
    // tall (192 x 128 tiles, the wide kernel with 3 x 2 MFMA tiles per wave), opt-in: a Linear whose 128 x 128 tiling is a few units
    // past one round of the CUs (N = 512 at 8.2 k - 12 k packed encoder rows: 260 - 384 units) becomes ONE round of at most 256
    // bigger units (round 6).  Measured LEVEL with the pair kernel - 8 704 x 512 x 512: 16.5 vs 16.2 us, x 1 024: 22.0 vs 22.2; train
    // step 4.56-4.64 either way (profiles/r06_gemm_tile_choice.txt) - 184 units of 1.5 x the work cost what 272 units on 512 slots do.
    const int tall_units = ((a.M + 191) / 192) * ((a.N + 127) / 128) * a.batch;
    const bool go_tall = sw.v3 && sw.tall && !go_wide && ring_ok && linear && valid_units > 256 && tall_units <= cus;
    // skinny (a few hundred rows against a whole weight: the greedy-decode Linears).  Measured, greedy decode B 256 x 1024 steps: f32
    // 3.65 -> 2.03 ms/step (the f32 Linears were 43 ... 98 us each on 8 blocks), bf16 1.224 -> 1.112 ms/step (32 blocks of the small
    // kernel before).  f32 has no 64 x 64-tile kernel: a 2048-row f32 Linear (the decoder side of the f32 train step) is 64 blocks of
    // the pair kernel on 256 CUs, the K-resident 32 x 32 kernel puts it on 1024 blocks: f32 train step 31.29 -> 29.84 ms (batch 16);
    // at 8704 rows it loses (30.2 ms with the limit at 16384) - hence the f32 row limit of its own.
    const bool go_skinny = sw.skinny && (!bf || sw.skinny >= 2) && a.a_kcontig && a.b_kcontig && splitk == 1 && a.batch == 1 &&
                           a.M <= (bf ? sw.skinny_rows : sw.skinny_rows_f32) && a.K % (bf ? 512 : 256) == 0 && !a.aux && a.drop_p == 0.f &&
                           !sw.noglds && pl.aligned;
    // big (eight waves, gemm8.h), opt-in: plain bf16 Linears of at least PA_GEMM_BIG_MINM rows.  Level with the kernels below at this
    // model's shapes, never ahead (profiles/r04_step_floor_probes.txt section 8).
    const bool go_big = sw.big && !go_skinny && bf && !sw.noglds && pl.aligned && linear && a.M >= sw.big_minm && a.N >= sw.big_minn;
    if (go_big) {
        // tile width: PA_GEMM_BIG=1 (round 4): 256 from N = 1024 on, else 128.  PA_GEMM_BIG=2 (round 6): the width in {256, 192, 128}
        // that needs the fewest ROUNDS of one block per CU (ties: the wider tile) - 256 x 192 makes N = 1536 one round of 31 x 8 blocks
        // at 7.9 k rows where 256 x 256 leaves 70 CUs idle and 128-wide tiles take two rounds; PA_GEMM_BIG_TN=<n> forces.
        int tn = a.N >= 1024 ? 256 : 128;
        if (sw.big >= 2) {
            long best = -1;
            for (int w : {256, 192, 128}) {
                const long blocks = (long)((a.M + 255) / 256) * ((a.N + w - 1) / w) * a.batch;
                const long rounds = (blocks + cus - 1) / cus;
                const long cost = rounds * w * 1000 + ((a.N + w - 1) / w * w - a.N);       // time ~ rounds x tile width; then least padding
                if (best < 0 || cost < best) { best = cost; tn = w; }
            }
        }
        if (sw.big_tn == 256 || sw.big_tn == 192 || sw.big_tn == 128) tn = sw.big_tn;
        plan_kernel(pl, PA_GEMM_KIND_BIG, GK_BIG, a, 256, tn, a.batch, UNITS_XCD, cus, 512);
        return pl;
    }
    if (a.C_lp && !go_skinny) return plan_fail(PA_EINVAL);          // the bf16 copy of an f32 output exists in the skinny kernel only
    if (go_skinny) plan_kernel(pl, PA_GEMM_KIND_SKINNY, GK_SKINNY, a, SK_T, SK_T, 1, UNITS_PLAIN, INT_MAX, 256);      // one block per tile
    else if (go_wide) plan_kernel(pl, PA_GEMM_KIND_WIDE, GK_WIDE, a, 128, 256, a.batch, UNITS_XCD_ALWAYS, cus, NT);
    else if (go_tall) plan_kernel(pl, PA_GEMM_KIND_WIDE, GK_TALL, a, 192, 128, a.batch, UNITS_XCD, cus, NT);
    else if (go_small) plan_kernel(pl, PA_GEMM_KIND_SMALL, GK_SMALL, a, 64, 64, a.batch, UNITS_PLAIN, 2 * cus, NT);   // two 80 KB blocks fit a CU
    else if (go_v3) plan_kernel(pl, PA_GEMM_KIND_RING, GK_RING, a, BM, BN, a.batch * splitk, UNITS_XCD, cus, NT);
    else {
        const int pair_cap = sw.grid > 0 ? (sw.grid / 256) * cus + sw.grid % 256 : INT_MAX;
        plan_kernel(pl, PA_GEMM_KIND_PAIR, GK_PAIR, a, BM, BN, a.batch * splitk, UNITS_XCD, pair_cap, NT);
    }
    return pl;
}

// pa_gemm_norm_a: the f32 skinny form, the bf16 skinny form, or the 64 x 64 form of the small kernel
GemmPlan plan_norm_a(const pa_gemm_args& a, const pa_gemm_norm_ext& x, const GemmSwitches& sw, int cus) {
    if (!a.A || !a.B || !a.C || !a.bias || !x.u || a.M <= 0 || a.N <= 0 || a.K <= 0) return plan_fail(PA_EINVAL);
    if ((a.in_dtype != PA_BF16 && a.in_dtype != PA_F32) || (a.out_dtype != PA_BF16 && a.out_dtype != PA_F32) || !a.a_kcontig || !a.b_kcontig) return plan_fail(PA_EINVAL);
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    GemmPlan pl = GemmPlan();
    pl.splitk = 1;
    // C / bias / u as 4-element vectors
    const bool cbu_ok = vec_ok(a.C, a.ldc, 0, a.out_dtype == PA_F32 ? 4 : 2) && al16(a.bias) && al16(x.u);
    if (a.in_dtype == PA_F32) {
        // exact-f32 form (the f32 greedy-decode step): f32 rows, f32 folded weight (pa_ln_fold_weights_f32), f32 output; the statistics
        // come from the rows themselves (ext->zf, normally == args->A).  Skinny kernel only: <= 512 rows, K = 512.
        if (a.batch != 1 || a.splitk > 1 || a.R || a.aux || a.drop_p != 0.f || a.N % 32) return plan_fail(PA_ESHAPE);
        if (!x.zf || a.K != 512 || a.M > sw.skinny_rows || a.out_dtype != PA_F32 || (x.y && (!x.y_f32 || a.N < a.K))) return plan_fail(PA_ESHAPE);
        if (x.y && (!x.gamma || !x.beta || x.ldy < a.K || x.ldy % 4 || !al16(x.y))) return plan_fail(PA_EINVAL);
        if (!is_aligned<float>(&a) || x.ldzf < a.K || x.ldzf % 4 || !al16(x.zf)) return plan_fail(PA_EALIGN);
        pl.vec_ok = cbu_ok && (!x.y || (al16(x.gamma) && al16(x.beta)));
        if (!pl.vec_ok) return plan_fail(PA_EALIGN);
        plan_kernel(pl, PA_GEMM_KIND_SKINNY, GK_SKINNY, a, SK_T, SK_T, 1, UNITS_PLAIN, INT_MAX, 256);
        return pl;
    }
    if (a.batch != 1 || a.splitk > 1 || a.R || a.aux || a.drop_p != 0.f || a.K % 64 || a.N % 32) return plan_fail(PA_ESHAPE);
    if (x.y && (!x.gamma || !x.beta || x.ldy < a.K || x.ldy % 4)) return plan_fail(PA_EINVAL);
    if (x.y && (a.N + 63) / 64 * 64 < a.K) return plan_fail(PA_ESHAPE);      // column tile j materialises columns 64 j .. 64 j + 63 of LayerNorm(Z)
    if (!is_aligned<bf16>(&a)) return plan_fail(PA_EALIGN);
    if (x.zf && (x.ldzf < a.K || x.ldzf % 4 || !al16(x.zf))) return plan_fail(PA_EINVAL);
    if (x.y && x.y_f32 && !al16(x.y)) return plan_fail(PA_EALIGN);
    pl.vec_ok = cbu_ok;
    // <= 512 rows and K = 512: the skinny kernel's form (the Z tile is resident in LDS, the statistics cost no memory round trip)
    if (sw.skinny >= 2 && a.M <= sw.skinny_rows && a.K == 512 &&
        (!x.y || (a.N >= a.K && x.ldy % 8 == 0 && al16(x.y) && al16(x.gamma) && al16(x.beta)))) {
        plan_kernel(pl, PA_GEMM_KIND_SKINNY, GK_SKINNY, a, SK_T, SK_T, 1, UNITS_PLAIN, INT_MAX, 256);
        return pl;
    }
    if (x.zf || x.y_f32) return plan_fail(PA_ESHAPE);               // the f32-residual form exists in the skinny kernel only
    plan_kernel(pl, PA_GEMM_KIND_SMALL, GK_SMALL, a, 64, 64, 1, UNITS_PLAIN, INT_MAX, NT);
    if (pl.t.units > 2 * cus) return plan_fail(PA_ESHAPE);         // the row statistics live in registers: one unit per block
    if (!pl.vec_ok) return plan_fail(PA_EALIGN);
    pl.tiles_per_slice = a.K / 64;
    return pl;
}

}  // namespace

// Measurement hook: while recording, every pa_gemm() call's argument block is appended to a host-side list so that
// bench.py can replay exactly the launches of one training step under HIP events (per-launch roofline census).
namespace {
std::vector<pa_gemm_args>* g_rec = nullptr;
std::vector<int32_t>* g_rec_kind = nullptr;      // kernel each recorded launch was dispatched to (PA_GEMM_KIND_*)
std::vector<int32_t>* g_rec_group = nullptr;     // -1: launched by pa_gemm; >= 0: member of that pa_gemm_group launch
int g_rec_ngroups = 0;
std::mutex g_rec_mu;
void record_args(const pa_gemm_args& a) {
    if (g_rec) { std::lock_guard<std::mutex> lk(g_rec_mu); if (g_rec) g_rec->push_back(a); }
}
// the kernel family of the launch just recorded and the pa_gemm_group launch it belongs to (-1: pa_gemm's own)
void record_kind(int kind, int group) {
    if (!g_rec) return;
    std::lock_guard<std::mutex> lk(g_rec_mu);
    if (g_rec && g_rec_kind) g_rec_kind->push_back(kind);
    if (g_rec && g_rec_group) g_rec_group->push_back(group);
}
}
extern "C" int pa_gemm_record(int32_t enable) {
    std::lock_guard<std::mutex> lk(g_rec_mu);
    if (enable) {
        delete g_rec; g_rec = new std::vector<pa_gemm_args>();
        delete g_rec_kind; g_rec_kind = new std::vector<int32_t>();
        delete g_rec_group; g_rec_group = new std::vector<int32_t>(); g_rec_ngroups = 0;
        return 0;
    }
    return g_rec ? (int)g_rec->size() : 0;
}
extern "C" int pa_gemm_recorded(pa_gemm_args* out, int32_t cap) {
    std::lock_guard<std::mutex> lk(g_rec_mu);
    if (!g_rec) return 0;
    const int n = (int)g_rec->size() < cap ? (int)g_rec->size() : cap;
    for (int i = 0; i < n; ++i) out[i] = (*g_rec)[i];
    delete g_rec; g_rec = nullptr;
    return n;
}
extern "C" int pa_gemm_recorded_groups(int32_t* out, int32_t cap) {
    std::lock_guard<std::mutex> lk(g_rec_mu);
    if (!g_rec_group) return 0;
    const int n = (int)g_rec_group->size() < cap ? (int)g_rec_group->size() : cap;
    for (int i = 0; i < n; ++i) out[i] = (*g_rec_group)[i];
    return n;
}
extern "C" int pa_gemm_recorded_kinds(int32_t* out, int32_t cap) {
    std::lock_guard<std::mutex> lk(g_rec_mu);
    if (!g_rec_kind) return 0;
    const int n = (int)g_rec_kind->size() < cap ? (int)g_rec_kind->size() : cap;
    for (int i = 0; i < n; ++i) out[i] = (*g_rec_kind)[i];
    return n;
}

namespace {
// bf16x3 mode state (see "bf16x3 (split) products" below)
struct SplitKeep { const void* src; int rows, cols, ld, pat; bf16* dst; int made; };     // pat 0: (hi, hi, lo) parts, 1: (hi, lo, hi);
                                                                                          // made 1: written by its producer (pa_gemm_split_reserve)
// Images of the CONSTANT operands (the weights: every k-contiguous B operand of an unbatched GEMM in this mode), owned by one model
// (pa_gemm_split_cache_*): learnt during the first step - a miss cuts the operand into the cache instead of the scratch - and from
// then on re-cut all at once whenever the parameters changed (pa_gemm_split_cache_refresh), so that a Linear whose input image
// was written by its producer needs no split launch at all.
constexpr int SPLIT_CACHE_MAX = 320, SPLIT_CACHE_HEAD = 32768;         // (the head of the buffer holds the device copy of the job table)
struct SplitCache { char* buf; long long bytes, used; int n; bool table_stale; SplitKeep e[SPLIT_CACHE_MAX]; };
constexpr int KEEP_SEG_MAX = 16, KEEP_FWD_MAX = 128;
// what a cut plan advances: the scratch offsets, the lengths of the two image lists, the forward list closed by an overflow
struct SplitPos { long long long_off = 0, keep_off = 0; int nkeep = 0, nkeepL = 0; bool long_closed = false; };
struct SplitState : SplitPos {
    std::atomic<int> on{0}; char* ws = nullptr; long long bytes = 0;
    std::atomic<int> attn{0};                  // the attention launches of this context run split too (pa_attn_split_config)
    // Retained images.  A k-contiguous operand cut as [rows][3 cols] and read as [3 rows][cols] IS its stacked form with the planes
    // interleaved row by row, so the image one GEMM built serves a later GEMM that contracts over the ROWS of the same buffer:
    //   retain 1 (pa_gemm_split_config(2, ..): a backward segment): dY of every dX GEMM stays at [long_off, keep_off) until the next
    //            config call - the segment's grouped weight-gradient launch finds it already cut (plan_group_split3);
    //   retain 2 (pa_gemm_split_config(3, ..): the forward): X of every Linear stays at [0, long_off) until the next forward (config 3)
    //            or a plain config (1) - the same grouped launch finds its OTHER operand already cut as well.
    // Forward images are (hi, hi, lo); a backward segment cuts dY as (hi, lo, hi) so that the two meet in one product.
    int retain = 0; SplitKeep keep[KEEP_SEG_MAX]; SplitKeep keepL[KEEP_FWD_MAX]; SplitCache* cache = nullptr;
    // a weight gradient's dY operand is looked up among this segment's images only, its X operand among the forward's only: backward
    // buffers may reuse addresses of forward buffers that are dead by then
    static const SplitKeep* find_in(const SplitKeep* t, int n, const void* src, int rows, int cols, int ld) {
        for (int k = n - 1; k >= 0; --k) { const SplitKeep& e = t[k]; if (e.src == src && e.rows == rows && e.cols == cols && e.ld == ld) return &e; }
        return nullptr;
    }
    const SplitKeep* find_seg(const void* src, int rows, int cols, int ld) const { return find_in(keep, nkeep, src, rows, cols, ld); }
    const SplitKeep* find_fwd(const void* src, int rows, int cols, int ld) const { return retain == 2 ? nullptr : find_in(keepL, nkeepL, src, rows, cols, ld); }
    static void put(SplitKeep* t, int& n, const SplitKeep& e) {       // (a buffer cut again replaces its older image)
        for (int k = 0; k < n; ++k) if (t[k].src == e.src) { t[k] = e; return; }
        t[n++] = e;
    }
};
// The mode's state is a CONTEXT owned by one model (pa_split_ctx_*): mode, scratch, retained images, weight cache, counters.  A host
// thread ENTERS a context around that model's library calls (pa_split_ctx_enter; thread-local), so two models of different compute
// modes - on two streams, from two threads, or alternating on one - never see each other's mode or images (VERDICT r5 item 6:
// rounds 4-5 kept ONE process-global SplitState).  Calls made outside any context use the process default context: what the
// pa_gemm_split_config(...) shim of rounds 4-5 (kernel tests, tools) configures.
struct SplitCounters { std::atomic<long long> taken{0}, declined{0}, reused{0}, made_hits{0}, cache_hits{0}; };
SplitCounters g_cnt;                        // diagnostics of the whole process (every context adds to them): pa_gemm_split_stats & co
SplitState g_default_split;
thread_local SplitState* t_split = nullptr;
inline SplitState& cur_split() { return t_split ? *t_split : g_default_split; }
#define g_split (cur_split())
bool split_on() { return g_split.on.load(std::memory_order_relaxed) != 0; }
}  // namespace
extern "C" int pa_split_ctx_create(void** out) {
    if (!out) return PA_EINVAL;
    *out = new (std::nothrow) SplitState();
    return *out ? 0 : PA_EINVAL;
}
extern "C" void pa_split_ctx_destroy(void* ctx) {
    SplitState* c = static_cast<SplitState*>(ctx);
    if (t_split == c) t_split = nullptr;
    delete c;
}
extern "C" int pa_split_ctx_enter(void* ctx) { t_split = static_cast<SplitState*>(ctx); return 0; }      // NULL: leave (process default)
extern "C" void* pa_split_ctx_current(void) { return t_split; }
extern "C" int pa_split_attn_set(int32_t on) { g_split.attn.store(on ? 1 : 0, std::memory_order_relaxed); return 0; }
extern "C" int pa_split_attn_active(void) { return g_split.attn.load(std::memory_order_relaxed); }
// number of non-empty contraction slices pa_gemm uses for a requested split (whole K tiles of 64 bf16 / 16 f32 elements)
extern "C" int pa_gemm_effective_splitk(int32_t K, int32_t in_dtype, int32_t splitk) {
    // (bf16x3 mode: an f32 GEMM runs on the bf16 kernels over a 3 K long contraction - its slices are whole 64-wide tiles of THAT)
    const bool x3 = in_dtype == PA_F32 && split_on();
    const int BK = (in_dtype == PA_BF16 || x3) ? 64 : 16;
    return eff_splitk(((x3 ? 3 * K : K) + BK - 1) / BK, splitk);
}
extern "C" int pa_gemm_split_active(void) { return split_on() ? 1 : 0; }

// CUs the persistent GEMM kernels occupy.  They launch one (or two) blocks per CU that hold the whole register file, so a
// collective kernel enqueued on another stream (RCCL's all-reduce of a finished gradient slice) finds no CU to run on
// until a GEMM launch drains.  pa_set_reserved_cus(n) (or PA_RESERVE_CUS=n) makes every persistent launch leave n CUs
// alone; plankassembly_amd.distributed.GradSync sets it when the world is larger than one process.
static std::atomic<int> g_reserved_cus{-1};
static int cus_for_gemm() {
    int r = g_reserved_cus.load(std::memory_order_relaxed);
    if (r < 0) {
        const char* e = getenv("PA_RESERVE_CUS");
        r = e ? atoi(e) : 0;
        if (r < 0) r = 0;
        if (r > 192) r = 192;
        g_reserved_cus.store(r, std::memory_order_relaxed);
    }
    return 256 - r;
}
extern "C" int pa_set_reserved_cus(int32_t n) {
    if (n < 0 || n > 192) return PA_EINVAL;
    g_reserved_cus.store(n, std::memory_order_relaxed);
    return 0;
}
extern "C" int pa_get_reserved_cus(void) { return 256 - cus_for_gemm(); }

// -------------------------------------------------------------------------------------------------
// bf16x3 ("split") products: an f32-accurate GEMM on the bf16 matrix pipe.  Every f32 operand is cut into
// hi = bf16(x) and lo = bf16(x - hi) (16 mantissa bits together) and the product runs as hi*hi + hi*lo + lo*hi with f32
// accumulation - the lo*lo term, 2^-16 of the result, is dropped: ~2^-17 relative per product against 2^-9 for plain bf16 and 2^-24
// for f32, inside north_star's 1e-4 (tools/x3_sim.py: the whole train step evaluated this way sits at <= 0.2 x the f32 gate).
// Realised WITHOUT a new GEMM kernel: the three products are ONE bf16 GEMM over a three times longer contraction index,
//     A' = [A_hi | A_hi | A_lo]   B' = [B_hi | B_lo | B_hi]      (k-contiguous operand: the three parts side by side in a row;
//                                                                  operand with a strided contraction index: stacked as rows)
// built by one split_kernel launch per GEMM into a caller-owned scratch buffer (pa_gemm_split_config), so every bf16 kernel family
// (ring / pair / small / wide / skinny, split-K, every epilogue) serves the mode unchanged at 3/16 of the exact-f32 MFMA time.
// Exact f32 (v_mfma_f32_32x32x2_f32) stays the checker and the fallback for shapes the bf16 fast paths do not take.
namespace {
struct SplitJob { const float* src; bf16* dst; int rows, cols, ld, mode; long long sstride, dstride; int batch, pad_; };
struct SplitTab { SplitJob j[2 * PA_MAX_GROUP_]; int begin[2 * PA_MAX_GROUP_ + 1]; int n; };
// mode 0: [rows][cols] -> [rows][3 cols] as (hi, hi, lo);  1: as (hi, lo, hi);  2: -> [3 rows][cols] stacked (hi, hi, lo);
// 3: stacked (hi, lo, hi);  4: hi only [rows][cols] (the ReLU-backward gate: only its sign is read)
__device__ __forceinline__ void split_job(const SplitJob& J, int bid, int nb) {
    // eight consecutive f32 per thread and pass (every job has cols % 8 == 0): two 16-byte loads, 16-byte stores
    const uint32_t c8 = (uint32_t)J.cols >> 3;
    const uint32_t per = (uint32_t)J.rows * c8, total = per * (uint32_t)J.batch;          // (< 2^31: checked by the launchers)
    for (uint32_t e = (uint32_t)bid * 256u + threadIdx.x; e < total; e += (uint32_t)nb * 256u) {
        const uint32_t b = J.batch > 1 ? e / per : 0u;
        const uint32_t r_ = e - b * per;
        const int r = (int)(r_ / c8), c = (int)(r_ - (uint32_t)r * c8) << 3;
        const float* sp = J.src + (size_t)b * J.sstride + (size_t)r * J.ld + c;
        const f32x4 x = *reinterpret_cast<const f32x4*>(sp), y = *reinterpret_cast<const f32x4*>(sp + 4);
        u32x4 hi, lo;
        hi[0] = pack_bf16(x[0], x[1]); hi[1] = pack_bf16(x[2], x[3]); hi[2] = pack_bf16(y[0], y[1]); hi[3] = pack_bf16(y[2], y[3]);
        lo[0] = pack_bf16(x[0] - bf16_lo(hi[0]), x[1] - bf16_hi(hi[0]));
        lo[1] = pack_bf16(x[2] - bf16_lo(hi[1]), x[3] - bf16_hi(hi[1]));
        lo[2] = pack_bf16(y[0] - bf16_lo(hi[2]), y[1] - bf16_hi(hi[2]));
        lo[3] = pack_bf16(y[2] - bf16_lo(hi[3]), y[3] - bf16_hi(hi[3]));
        bf16* d = J.dst + (size_t)b * J.dstride;
        if (J.mode == 4) { *reinterpret_cast<u32x4*>(d + (size_t)r * J.cols + c) = hi; continue; }
        const bool a_pat = (J.mode & 1) == 0;                 // (hi, hi, lo) or (hi, lo, hi)
        if (J.mode < 2) {
            bf16* row = d + (size_t)r * 3 * J.cols + c;
            *reinterpret_cast<u32x4*>(row) = hi;
            *reinterpret_cast<u32x4*>(row + J.cols) = a_pat ? hi : lo;
            *reinterpret_cast<u32x4*>(row + 2 * J.cols) = a_pat ? lo : hi;
        } else {
            const size_t plane = (size_t)J.rows * J.cols;
            bf16* q = d + (size_t)r * J.cols + c;
            *reinterpret_cast<u32x4*>(q) = hi;
            *reinterpret_cast<u32x4*>(q + plane) = a_pat ? hi : lo;
            *reinterpret_cast<u32x4*>(q + 2 * plane) = a_pat ? lo : hi;
        }
    }
}
__global__ __launch_bounds__(256) void split_kernel(SplitTab tb) {
    int k = 0;
    while (k + 1 < tb.n && (int)blockIdx.x >= tb.begin[k + 1]) ++k;
    split_job(tb.j[k], blockIdx.x - tb.begin[k], tb.begin[k + 1] - tb.begin[k]);
}
// the same over a job table in device memory (pa_gemm_split_cache_refresh: every weight of a model in one launch)
__global__ __launch_bounds__(256) void split_many_kernel(const SplitJob* jobs, const int* begin, int n) {
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if ((int)blockIdx.x >= begin[mid]) lo = mid; else hi = mid - 1; }
    const SplitJob J = jobs[lo];
    split_job(J, blockIdx.x - begin[lo], begin[lo + 1] - begin[lo]);
}

// ---- the cut plan (DESIGN.md "bf16x3 plan"): plan_*split3 decide, commit_split3 advances the context, launch_cuts launches, pa_gemm_split_plan reports
inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
inline long long img_bytes(long long bf16_elems) { return (bf16_elems * 2 + 255) / 256 * 256; }    // regions of the scratch are 256-byte aligned
// blocks of one cut job: one 8-element vector per thread up to `cap` blocks (measured for pa_gemm: 2 per thread / 2 048 blocks 12.25 ms
// per step, 1 / 8 192 12.14).  Each call site keeps the cap it was measured with; nobody has measured one cap for all.
constexpr int CUT_CAP_GEMM = 16384, CUT_CAP_GROUP = 8192, CUT_CAP_REFRESH = 4096;
inline int cut_blocks(const SplitJob& j, int cap) {
    const long long blocks = ((long long)j.rows * (j.cols >> 3) * j.batch + 255) / 256;
    return (int)(blocks < 1 ? 1 : blocks > cap ? cap : blocks);
}
// Room to retain one more image when the call needs `need` bytes behind the retained ones.  The forward (retain 2) keeps while its list
// is open and a quarter of the buffer stays free for the segments' own cuts; a segment (retain 1) up to its list's length, and an
// image made by its producer only below 7/8 of the buffer.
inline bool keep_room(const SplitState& st, const SplitPos& p, long long need, bool producer) {
    if (st.retain == 2) return !p.long_closed && p.nkeepL < KEEP_FWD_MAX && p.long_off + need <= st.bytes - st.bytes / 4;
    return st.retain == 1 && p.nkeep < KEEP_SEG_MAX && (!producer || p.keep_off + need <= st.bytes - st.bytes / 8);
}
// the positions after an image of `src` was retained at keep_off (a buffer cut again replaces its older image), and the list entry itself
inline void keep_advance(SplitPos& p, const SplitState& st, const void* src, long long bytes) {
    const bool fwd = st.retain == 2;
    const SplitKeep* t = fwd ? st.keepL : st.keep;
    int& n = fwd ? p.nkeepL : p.nkeep;
    n += std::none_of(t, t + n, [src](const SplitKeep& e) { return e.src == src; });
    p.keep_off += bytes;
    if (fwd) p.long_off = p.keep_off;
}
inline void keep_put(SplitState& st, const SplitKeep& e) { SplitState::put(st.retain == 2 ? st.keepL : st.keep, st.retain == 2 ? st.nkeepL : st.nkeep, e); }
struct SplitPlan {
    bool taken = false, group = false, drop_seg = false, drop_fwd = false;      // drop_*: image lists the call empties to make room
    int n = 1; SplitPos after; SplitKeep kept = {}, cached = {};   // after: the positions after the call; (src != NULL) the image it retains / the cache learns
    int made_hits = 0, cache_hits = 0, reused = 0, exact_want = 0;       // counter increments; declined deferred split-K: slabs the reducer reads
    pa_split_plan_info info[PA_MAX_GROUP_];              // per member: parts pattern, and per operand (A, B, aux) source, offset, bytes cut, mode
    SplitJob job[PA_MAX_GROUP_][3];                      // .. and its cut job (info.bytes > 0) or just the image (dst)
    pa_gemm_args inner[PA_MAX_GROUP_];                   // taken: the bf16 products over 3 K; declined: the exact call
};
// operand k of member i: its image `at` an address of the scratch / cache that starts at `base`, found there (bytes 0) or cut there by job j
inline bf16* set_image(SplitPlan& p, int i, int k, int source, const char* base, const void* at, long long bytes = 0, SplitJob j = SplitJob()) {
    pa_split_plan_info& o = p.info[i];
    j.dst = static_cast<bf16*>(const_cast<void*>(at));
    o.source[k] = source; o.off[k] = static_cast<const char*>(at) - base; o.bytes[k] = bytes; o.mode[k] = j.mode;
    o.blocks[k] = bytes ? cut_blocks(j, p.group ? CUT_CAP_GROUP : CUT_CAP_GEMM) : 0;
    p.job[i][k] = j;
    return j.dst;
}
// Retained images of a product whose operands both have a strided contraction index (a weight gradient dY^T X): either may have been cut
// before as the k-contiguous operand of an earlier GEMM - dY ([K rows][M features]) by this segment's dX GEMM, X by the forward's Linear,
// in the opposite parts pattern - and [K][3 M] read as [3 K][M] IS the stacked operand with the planes interleaved row by row.  Whichever
// is missing is then cut into the matching interleaving (split modes 0 / 1) instead of the plane-stacked modes 2 / 3.
struct SplitHits { const SplitKeep *a, *b; int pat; };
inline SplitHits find_stacked(const SplitState& st, const pa_gemm_args& a, int pat_default) {
    SplitHits h{st.find_seg(a.A, a.K, a.M, a.lda), st.find_fwd(a.B, a.K, a.N, a.ldb), pat_default};
    if (h.a) h.pat = h.a->pat; else if (h.b) h.pat = 1 - h.b->pat;
    if (h.b && h.b->pat == h.pat) h.b = nullptr;
    return h;
}
// The cuts of one pa_gemm call.  false: declined (what p holds by then is still committed: images dropped for room stay dropped)
bool plan_cuts(SplitPlan& p, const pa_gemm_args& a, const SplitState& st) {
    SplitPos& pos = p.after; pa_gemm_args& b = p.inner[0];
    const bool akc = a.a_kcontig != 0, bkc = a.b_kcontig != 0;
    const int M = a.M, N = a.N, K = a.K, nb = a.batch;
    const int ar = akc ? M : K, ac = akc ? K : M, br = bkc ? N : K, bc = bkc ? K : N;             // source rows / cols of each operand as stored
    if ((ac & 7) || (bc & 7) || (a.lda & 3) || (a.ldb & 3) || (a.sA & 3) || (a.sB & 3) || !al16(a.A) || !al16(a.B)) return false;
    if ((long long)ar * ac * nb >= (1ll << 33) || (long long)br * bc * nb >= (1ll << 33) || (long long)M * N * nb >= (1ll << 33)) return false;   // (split_kernel indexes 8-element vectors in 32 bits)
    if ((akc && bkc && (K & 63)) || a.C_lp) return false;     // the bf16 fast paths want whole K tiles per part
    if (a.aux && ((N & 7) || (a.ldaux & 3) || (a.sAux & 3) || !al16(a.aux))) return false;
    const int a_nb = nb > 1 && a.sA == 0 ? 1 : nb, b_nb = nb > 1 && a.sB == 0 ? 1 : nb;            // (an operand shared by the batch is cut once)
    const long long a_el = (long long)ar * ac * 3, b_el = (long long)br * bc * 3, x_el = a.aux ? (long long)M * N : 0;
    // parts pattern: the forward and plain mode cut A as (hi, hi, lo) and B as (hi, lo, hi), a backward segment the other way round
    // (its retained dY images then meet the forward's retained X images in the weight-gradient product)
    const int pat_default = st.retain == 1 ? 1 : 0;
    const bool stacked2 = !akc && !bkc && nb == 1;
    const SplitHits none{nullptr, nullptr, pat_default};
    SplitHits h = stacked2 ? find_stacked(st, a, pat_default) : none;
    // a k-contiguous A whose image was written by the kernel that produced A (pa_gemm_split_reserve) ..
    const SplitKeep* made = !akc || nb != 1 || !st.retain ? nullptr : st.retain == 2 ? SplitState::find_in(st.keepL, st.nkeepL, a.A, ar, ac, a.lda)
                                                                                         : st.find_seg(a.A, ar, ac, a.lda);
    if (made && made->made && made->pat == h.pat) { h.a = made; p.made_hits = 1; } else made = nullptr;
    // .. and a constant k-contiguous B (a weight) held in the model's cache; a miss is cut INTO the cache
    const SplitCache* const wc = bkc && nb == 1 ? st.cache : nullptr;
    const SplitKeep* cache_b = nullptr;
    for (int k = 0; wc && k < wc->n && !cache_b; ++k) {
        const SplitKeep& e = wc->e[k];
        if (e.src == a.B && e.rows == br && e.cols == bc && e.ld == a.ldb && e.pat == 1 - h.pat) { cache_b = &e; p.cache_hits = 1; }
    }
    if (wc && !cache_b && wc->n < SPLIT_CACHE_MAX && wc->used + img_bytes(b_el) <= wc->bytes)
        p.cached = SplitKeep{a.B, br, bc, a.ldb, 1 - h.pat, reinterpret_cast<bf16*>(wc->buf + wc->used), 0};
    const long long a_bytes = img_bytes(a_el * a_nb), b_bytes = cache_b || p.cached.src ? 0 : img_bytes(b_el * b_nb), x_bytes = img_bytes(x_el * nb);
    long long all = a_bytes + b_bytes + x_bytes, need = (h.a ? 0 : a_bytes) + (h.b ? 0 : b_bytes) + x_bytes;
    if (st.retain == 2) {
        // forward: does not fit behind the retained images - drop them and close the list (the images found may be the dropped ones)
        if (pos.long_off + need > st.bytes) {
            pos.long_off = 0; pos.nkeepL = 0; pos.long_closed = true; p.drop_fwd = true; h = none; need = all;
            if (need > st.bytes) return false;
        }
        pos.keep_off = pos.long_off;
    } else if (pos.keep_off + need > st.bytes) {
        // drop this segment's images, then the forward's (stream order keeps their earlier readers safe)
        pos.keep_off = pos.long_off; pos.nkeep = 0; p.drop_seg = true; h = none; need = all;
        if (pos.keep_off + need > st.bytes) {
            pos.long_off = 0; pos.nkeepL = 0; pos.keep_off = 0; p.drop_fwd = true;
            if (need > st.bytes) return false;
        }
    }
    const bool keep_a = !h.a && akc && nb == 1 && keep_room(st, pos, need, false);
    // split-K: callers size their slabs with pa_gemm_effective_splitk(K, PA_F32, .), which in this mode already counts whole
    // 64-wide tiles of the 3 K long bf16 contraction - the request passes through unchanged
    if (a.splitk > 1 && !a.ws) return false;
    const bool inter = stacked2 && (h.a || h.b);               // row-interleaved stacking: split modes 0 / 1 instead of 2 / 3
    if (inter) p.reused = (h.a ? 1 : 0) + (h.b ? 1 : 0);
    const int a_mode = (akc || inter ? 0 : 2) + h.pat, b_mode = (bkc || inter ? 0 : 2) + (1 - h.pat);
    const SplitJob ja{static_cast<const float*>(a.A), nullptr, ar, ac, a.lda, a_mode, a.sA, a_el, a_nb, 0};
    const SplitJob jb{static_cast<const float*>(a.B), nullptr, br, bc, a.ldb, b_mode, a.sB, b_el, b_nb, 0};
    const SplitJob jx{static_cast<const float*>(a.aux), nullptr, M, N, a.ldaux, 4, a.sAux, x_el, nb, 0};
    const char* at = st.ws + pos.keep_off;
    p.info[0].pat = h.pat;
    b.A = h.a ? set_image(p, 0, 0, h.a == made ? PA_SPLIT_SRC_MADE : PA_SPLIT_SRC_SEGMENT, st.ws, h.a->dst) : set_image(p, 0, 0, PA_SPLIT_SRC_SCRATCH, st.ws, at, a_bytes, ja);
    if (keep_a) { p.kept = SplitKeep{a.A, ar, ac, a.lda, h.pat, static_cast<bf16*>(const_cast<void*>(b.A)), 0}; keep_advance(pos, st, a.A, a_bytes); }
    if (!h.a) at += a_bytes;
    if (p.cached.src) b.B = set_image(p, 0, 1, PA_SPLIT_SRC_CACHE_CUT, wc->buf, p.cached.dst, img_bytes(b_el), jb);
    else if (cache_b) b.B = set_image(p, 0, 1, PA_SPLIT_SRC_CACHE, wc->buf, cache_b->dst);
    else if (h.b) b.B = set_image(p, 0, 1, PA_SPLIT_SRC_FORWARD, st.ws, h.b->dst);
    else { b.B = set_image(p, 0, 1, PA_SPLIT_SRC_SCRATCH, st.ws, at, b_bytes, jb); at += b_bytes; }
    if (a.aux) { b.aux = set_image(p, 0, 2, PA_SPLIT_SRC_SCRATCH, st.ws, at, x_bytes, jx); b.ldaux = N; b.sAux = x_el; }
    b.in_dtype = PA_BF16; b.K = 3 * K; b.splitk = a.splitk > 1 ? a.splitk : 1;
    b.lda = akc ? 3 * K : M; b.ldb = bkc ? 3 * K : N; b.sA = a_nb < nb ? 0 : a_el; b.sB = b_nb < nb ? 0 : b_el;
    return true;
}
SplitPlan plan_split3(const pa_gemm_args& a, const SplitState& st) {
    SplitPlan p; p.after = st; p.info[0] = pa_split_plan_info(); p.inner[0] = a;
    p.taken = plan_cuts(p, a, st);
    if (!p.taken && a.splitk > 1 && a.splitk_defer && a.ws) {
        // the caller's reduction descriptor counts pa_gemm_effective_splitk(K, PA_F32, splitk) slabs in THIS mode's (bf16) tiling; the exact
        // kernel writes the f32 tiling's count: it runs with a request that yields no more than that, and the reducer gets zeros for the rest
        int& req = p.inner[0].splitk = p.exact_want = eff_splitk((3 * a.K + 63) / 64, a.splitk);
        while (req > 1 && eff_splitk((a.K + 15) / 16, req) > p.exact_want) --req;
    }
    return p;
}
// The cuts of one pa_gemm_group call: every member's two operands go into their stacked forms in consecutive regions behind the
// images this segment retained, by ONE split launch; the members then run as one grouped bf16 launch over 3 K rows each.  All or none.
SplitPlan plan_group_split3(const pa_gemm_args* args, int n, const SplitState& st) {
    SplitPlan p; p.group = true; p.n = n; p.after = st;
    long long off = st.keep_off;
    for (int i = 0; i < n; ++i) {
        const pa_gemm_args& a = args[i];
        if (a.in_dtype != PA_F32 || a.out_dtype != PA_F32 || a.a_kcontig || a.b_kcontig || a.batch != 1) return p;
        if (a.bias || a.R || a.aux || a.relu || a.drop_p > 0.f || a.alpha != 1.f || a.C_lp) return p;
        if ((a.M & 7) || (a.N & 7) || (a.lda & 3) || (a.ldb & 3) || !al16(a.A) || !al16(a.B)) return p;
        if ((long long)a.K * a.M >= (1ll << 33) || (long long)a.K * a.N >= (1ll << 33)) return p;
        const SplitHits h = find_stacked(st, a, 0);
        const long long a_bytes = h.a ? 0 : img_bytes((long long)a.K * a.M * 3), b_bytes = h.b ? 0 : img_bytes((long long)a.K * a.N * 3);
        if (off + a_bytes + b_bytes > st.bytes) return p;
        const int mode = h.a || h.b ? 0 : 2;
        pa_gemm_args& b = p.inner[i] = a;
        p.info[i] = pa_split_plan_info(); p.info[i].pat = h.pat;
        b.A = h.a ? set_image(p, i, 0, PA_SPLIT_SRC_SEGMENT, st.ws, h.a->dst) : set_image(p, i, 0, PA_SPLIT_SRC_SCRATCH, st.ws, st.ws + off, a_bytes,
                        SplitJob{static_cast<const float*>(a.A), nullptr, a.K, a.M, a.lda, mode + h.pat, 0, 0, 1, 0});
        b.B = h.b ? set_image(p, i, 1, PA_SPLIT_SRC_FORWARD, st.ws, h.b->dst) : set_image(p, i, 1, PA_SPLIT_SRC_SCRATCH, st.ws, st.ws + off + a_bytes, b_bytes,
                        SplitJob{static_cast<const float*>(a.B), nullptr, a.K, a.N, a.ldb, mode + 1 - h.pat, 0, 0, 1, 0});
        off += a_bytes + b_bytes;
        p.reused += (h.a ? 1 : 0) + (h.b ? 1 : 0);            // (counted only if the whole group is taken: commit_split3)
        b.in_dtype = PA_BF16; b.K = 3 * a.K; b.lda = a.M; b.ldb = a.N;
    }
    p.taken = true;
    return p;
}
// The only place that advances a context, its cache's list and the process counters.
void commit_split3(SplitState& st, const SplitPlan& p) {
    if (p.drop_seg) st.nkeep = 0;
    if (p.drop_fwd) st.nkeepL = 0;
    if (p.kept.src) keep_put(st, p.kept);                    // (after the drops: the kept image is the call's own)
    static_cast<SplitPos&>(st) = p.after;
    if (p.cached.src) { SplitCache& c = *st.cache; c.e[c.n++] = p.cached; c.used += img_bytes((long long)p.cached.rows * p.cached.cols * 3); c.table_stale = true; }
    if (p.taken) g_cnt.taken.fetch_add(p.n); else if (!p.group) g_cnt.declined.fetch_add(1);
    if (p.taken && p.reused) g_cnt.reused.fetch_add(p.reused);
    if (p.made_hits) g_cnt.made_hits.fetch_add(p.made_hits);
    if (p.cache_hits) g_cnt.cache_hits.fetch_add(p.cache_hits);
}
int launch_cuts(const SplitPlan& p, void* stream) {
    SplitTab tb; tb.n = 0; tb.begin[0] = 0;
    for (int i = 0; i < p.n; ++i)
        for (int k = 0; k < 3; ++k)
            if (p.info[i].bytes[k]) { tb.j[tb.n] = p.job[i][k]; tb.begin[tb.n + 1] = tb.begin[tb.n] + p.info[i].blocks[k]; ++tb.n; }
    if (tb.n) PA_LAUNCH(split_kernel, dim3(tb.begin[tb.n]), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), tb);
    return 0;
}
}  // namespace
extern "C" int pa_gemm_split_config(int32_t on, void* ws, int64_t bytes) {
    if (on && (!ws || bytes <= 0 || (reinterpret_cast<uintptr_t>(ws) & 255))) return PA_EINVAL;
    if (on == 0) { g_split.on.store(0, std::memory_order_relaxed); return 0; }       // (retained images stay: forward -> backward)
    if (on < 0 || on > 3) return PA_EINVAL;
    if (g_split.ws != static_cast<char*>(ws) || g_split.bytes != bytes) { g_split.long_off = 0; g_split.nkeepL = 0; }
    g_split.ws = static_cast<char*>(ws); g_split.bytes = bytes;
    if (on != 2) { g_split.long_off = 0; g_split.nkeepL = 0; g_split.long_closed = false; }
    g_split.retain = on == 2 ? 1 : on == 3 ? 2 : 0; g_split.keep_off = g_split.long_off; g_split.nkeep = 0;
    g_split.on.store(on ? 1 : 0, std::memory_order_relaxed);
    return 0;
}
// [0] GEMMs that ran as bf16x3 since the last reset, [1] f32 GEMMs that asked for it and ran exact (shape / alignment / scratch)
extern "C" int64_t pa_gemm_split_reused(void) { return g_cnt.reused.load(); }      // dY images the grouped dW launches found already cut
extern "C" int64_t pa_gemm_split_made_hits(void) { return g_cnt.made_hits.load(); }   // A images found written by their producer
extern "C" int64_t pa_gemm_split_cache_hits(void) { return g_cnt.cache_hits.load(); } // B (weight) images found in the model's cache
// Producer side of a retained image: the kernel about to write the f32 matrix `src` ([rows][cols], leading dimension ld) also writes
// its cut image ([rows][3 cols], parts pattern *pat: 0 (hi, hi, lo), 1 (hi, lo, hi)) to the returned address, and the GEMM that
// consumes `src` as its k-contiguous A operand skips its own cut.  NULL: no image wanted (mode off, no retain mode, no room).
extern "C" void* pa_gemm_split_reserve(const void* src, int32_t rows, int32_t cols, int32_t ld, int32_t* pat) {
    SplitState& st = cur_split();
    if (!split_on() || !st.retain || !src || rows <= 0 || cols <= 0 || (cols & 7)) return nullptr;
    const long long bytes = img_bytes((long long)rows * cols * 3);
    if (!keep_room(st, st, bytes, true)) return nullptr;
    bf16* dst = reinterpret_cast<bf16*>(st.ws + st.keep_off);  // (the forward's images lie back to back: keep_off == long_off in its mode)
    const int p = st.retain == 2 ? 0 : 1;                      // the parts pattern the consuming GEMM of this mode cuts A in
    SplitPos after = st;
    keep_advance(after, st, src, bytes);
    keep_put(st, SplitKeep{src, rows, cols, ld, p, dst, 1});
    static_cast<SplitPos&>(st) = after;
    if (pat) *pat = p;
    return dst;
}
extern "C" int pa_gemm_split_cache_create(void* buf, int64_t bytes, void** out) {
    if (!buf || !out || bytes <= SPLIT_CACHE_HEAD || (reinterpret_cast<uintptr_t>(buf) & 255)) return PA_EINVAL;
    SplitCache* c = new (std::nothrow) SplitCache();
    if (!c) return PA_EINVAL;
    c->buf = static_cast<char*>(buf); c->bytes = bytes; c->used = SPLIT_CACHE_HEAD; c->n = 0; c->table_stale = false;
    *out = c;
    return 0;
}
extern "C" void pa_gemm_split_cache_destroy(void* h) {
    if (!h) return;
    if (g_split.cache == h) g_split.cache = nullptr;
    delete static_cast<SplitCache*>(h);
}
extern "C" int pa_gemm_split_cache_use(void* h) { g_split.cache = static_cast<SplitCache*>(h); return 0; }
extern "C" int32_t pa_gemm_split_cache_entries(void* h) { return h ? static_cast<SplitCache*>(h)->n : 0; }
// the parameters changed: every image of the cache is cut again from its source, in one launch
extern "C" int pa_gemm_split_cache_refresh(void* h, void* stream) {
    SplitCache* c = static_cast<SplitCache*>(h);
    if (!c) return PA_EINVAL;
    if (c->n == 0) return 0;
    static_assert(SPLIT_CACHE_MAX * sizeof(SplitJob) + (SPLIT_CACHE_MAX + 1) * sizeof(int) <= SPLIT_CACHE_HEAD, "job table fits the head");
    SplitJob* dj = reinterpret_cast<SplitJob*>(c->buf);
    int* db = reinterpret_cast<int*>(c->buf + SPLIT_CACHE_MAX * sizeof(SplitJob));
    std::vector<int> begin(c->n + 1, 0);
    std::vector<SplitJob> jobs(c->n);
    for (int k = 0; k < c->n; ++k) {
        const SplitKeep& e = c->e[k];
        jobs[k] = SplitJob{static_cast<const float*>(e.src), e.dst, e.rows, e.cols, e.ld, e.pat, 0, 0, 1, 0};
        begin[k + 1] = begin[k] + cut_blocks(jobs[k], CUT_CAP_REFRESH);
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (c->table_stale) {
        // (only while the list is still growing: the first two steps)
        if (hipMemcpyAsync(dj, jobs.data(), jobs.size() * sizeof(SplitJob), hipMemcpyHostToDevice, st) != hipSuccess) return PA_EINVAL;
        if (hipMemcpyAsync(db, begin.data(), begin.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess) return PA_EINVAL;
        if (hipStreamSynchronize(st) != hipSuccess) return PA_EINVAL;          // (the host vectors die with this call)
        c->table_stale = false;
    }
    PA_LAUNCH(split_many_kernel, dim3(begin[c->n]), dim3(256), 0, st, dj, db, c->n);
    return 0;
}
extern "C" int pa_gemm_split_stats(int64_t* out2, int32_t reset) {
    if (out2) { out2[0] = g_cnt.taken.load(); out2[1] = g_cnt.declined.load(); }
    if (reset) { g_cnt.taken.store(0); g_cnt.declined.store(0); g_cnt.reused.store(0); g_cnt.made_hits.store(0); g_cnt.cache_hits.store(0); }
    return 0;
}
static int gemm_body(const pa_gemm_args* a, void* stream);
static int gemm_group_body(const pa_gemm_args* args, int32_t n, void* stream);
// Dry run (include/plank_hip.h): the plan pa_gemm (n == 1) / pa_gemm_group (n > 1) would make in the calling thread's context.
extern "C" int pa_gemm_split_plan(const pa_gemm_args* args, int32_t n, int32_t commit, pa_split_plan_info* out) {
    static_assert(sizeof(pa_split_plan_info) == 22 * 4 + 10 * 8, "pa_split_plan_info (plankassembly_amd/_lib.py mirrors it)");
    if (!args || !out || n <= 0 || n > PA_MAX_GROUP) return PA_EINVAL;
    const pa_gemm_args& a0 = args[0];
    if (n == 1 && (!a0.A || !a0.B || !a0.C || a0.M <= 0 || a0.N <= 0 || a0.K <= 0 || a0.batch <= 0)) return PA_EINVAL;
    SplitState& st = cur_split();
    const bool x3 = split_on() && a0.in_dtype == PA_F32;
    SplitPlan idle; idle.after = st; idle.n = n;             // (mode off / not an f32 product: nothing is planned)
    const SplitPlan p = !x3 ? idle : n == 1 ? plan_split3(a0, st) : plan_group_split3(args, n, st);     // (a copy of some KB: dry run only)
    if (x3 && commit) commit_split3(st, p);
    for (int i = 0; i < n; ++i) {
        // (only a taken plan filled info[i] and - but for a declined single call - inner[i]: otherwise zeros (source: caller) and the caller's block)
        const pa_gemm_args& b = p.taken || (x3 && n == 1) ? p.inner[i] : args[i];
        pa_split_plan_info& o = out[i] = p.taken ? p.info[i] : pa_split_plan_info();
        o.taken = p.taken; o.drop_seg = p.drop_seg; o.drop_fwd = p.drop_fwd;
        o.M = b.M; o.N = b.N; o.K = b.K; o.lda = b.lda; o.ldb = b.ldb; o.sA = b.sA; o.sB = b.sB; o.splitk = b.splitk;
        o.keep_off = p.after.keep_off; o.long_off = p.after.long_off;
        o.nkeep = p.after.nkeep; o.nkeepL = p.after.nkeepL; o.long_closed = p.after.long_closed;
    }
    return 0;
}
extern "C" int pa_gemm(const pa_gemm_args* a, void* stream) {
    if (!a || !a->A || !a->B || !a->C) return PA_EINVAL;
    if (a->in_dtype != PA_F32 || !split_on()) return gemm_body(a, stream);
    if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->batch <= 0) return PA_EINVAL;
    const SplitPlan p = plan_split3(*a, cur_split());
    commit_split3(cur_split(), p);
    const pa_gemm_args& b = p.inner[0];                      // the bf16 product over 3 K, or the exact call of a declined one
    int rc = p.taken ? launch_cuts(p, stream) : 0;           // (0, a negative PA_E* or a positive hipError_t of the cut / inner launch)
    if (!rc) rc = gemm_body(&b, stream);
    const int got = eff_splitk((b.K + 15) / 16, b.splitk);   // (declined deferred split-K: slabs the exact kernel wrote)
    if (rc || got >= p.exact_want) return rc;
    const size_t slab = (size_t)b.M * b.N * sizeof(float);
    return hipMemsetAsync(static_cast<char*>(b.ws) + got * slab, 0, (p.exact_want - got) * slab, reinterpret_cast<hipStream_t>(stream)) == hipSuccess ? 0 : PA_EINVAL;
}
// the exact / bf16 product: what pa_gemm runs outside the bf16x3 mode and what the mode's plans run inside it
static int gemm_body(const pa_gemm_args* a, void* stream) {
    record_args(*a);
    const GemmSwitches& sw = gemm_switches();
    const GemmPlan pl = plan_gemm(*a, sw, cus_for_gemm());      // (256 CUs minus those left to RCCL's kernels: pa_set_reserved_cus)
    if (pl.status) return pl.status;
    record_kind(pl.kind, -1);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    GemmP p = GemmP();                                           // (value-initialised: the LayerNorm-fold pointers stay null)
    fill_operands(p, *a);
    p.c_lp = a->C_lp; p.ldc_lp = a->ldc_lp;
    p.splitk = pl.splitk; p.tiles_per_slice = pl.tiles_per_slice;
    p.dbg = sw.dbg;
    GemmP pk = p;                                                // the product kernel's view: under split-K it writes the f32 slabs
    if (pl.splitk > 1) { pk.C = a->ws; pk.ldc = a->N; }
    pk.vec_ok = pl.vec_ok;
    set_tiling(pk, pl.t);
    const dim3 grid(pl.grid), block(pl.block);
    const bool akc = a->a_kcontig != 0, bkc = a->b_kcontig != 0;
    switch (pl.kernel) {
    case GK_BIG:
        if (pl.tile_w == 256) PA_LAUNCH((gemm8_kernel<4, 2, 2, 4, 64, 2>), grid, block, 0, st, pk);
        else if (pl.tile_w == 192) PA_LAUNCH((gemm8_kernel<4, 2, 2, 3, 64, 2>), grid, block, 0, st, pk);
        else PA_LAUNCH((gemm8_kernel<4, 2, 2, 2, 64, 2>), grid, block, 0, st, pk);
        break;
    case GK_SKINNY:
        if (a->in_dtype == PA_BF16) PA_LAUNCH((gemm_skinny_kernel<bf16, false>), grid, block, 0, st, pk);
        else PA_LAUNCH((gemm_skinny_kernel<float, false>), grid, block, 0, st, pk);
        break;
    case GK_WIDE: PA_LAUNCH((gemm3w_kernel<2, 4>), grid, block, 0, st, pk); break;
    case GK_TALL: PA_LAUNCH((gemm3w_kernel<3, 2>), grid, block, 0, st, pk); break;
    case GK_SMALL: PA_LAUNCH(gemm3s_kernel, grid, block, 0, st, pk); break;
    case GK_RING:
        if (akc && bkc) PA_LAUNCH((gemm3_kernel<true, true, GemmP>), grid, block, 0, st, pk);
        else if (akc) PA_LAUNCH((gemm3_kernel<true, false, GemmP>), grid, block, 0, st, pk);
        else if (bkc) PA_LAUNCH((gemm3_kernel<false, true, GemmP>), grid, block, 0, st, pk);
        else PA_LAUNCH((gemm3_kernel<false, false, GemmP>), grid, block, 0, st, pk);
        break;
    case GK_PAIR: {
        int rc;
        if (a->in_dtype != PA_BF16) rc = launch_layout<float, 16, 2>(pk, akc, bkc, pl.aligned, pl.glds, grid, st);
        else if (pl.bk == 32) rc = launch_layout<bf16, 32, 3>(pk, akc, bkc, pl.aligned, pl.glds, grid, st);
        else rc = launch_layout<bf16, 64, 2>(pk, akc, bkc, pl.aligned, pl.glds, grid, st);
        if (rc) return rc;
        break;
    }
    }
    // (only the ring and pair kernels take split-K: every other family is planned for splitk == 1)
    if (pl.splitk > 1 && a->splitk_defer) {
        // the caller reduces the slabs later: only plain f32 outputs qualify (no epilogue would be applied)
        if (a->out_dtype != PA_F32 || a->bias || a->R || a->aux || a->relu || a->drop_p > 0.f || a->alpha != 1.f || a->batch != 1) return PA_EINVAL;
        return 0;
    }
    if (pl.splitk > 1) {
        size_t total = (size_t)a->batch * a->M * a->N;
        int blocks = (int)((total + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        if (a->in_dtype == PA_BF16)
            PA_LAUNCH(splitk_reduce_kernel<bf16>, dim3(blocks), dim3(256), 0, st, p, (const float*)a->ws);
        else
            PA_LAUNCH(splitk_reduce_kernel<float>, dim3(blocks), dim3(256), 0, st, p, (const float*)a->ws);
    }
    return 0;
}

// Dry run (include/plank_hip.h): the status, family and grid pa_gemm / pa_gemm_norm_a would use, from the same plan functions.
extern "C" int pa_gemm_plan(const pa_gemm_args* a, const pa_gemm_norm_ext* x, pa_gemm_plan_info* out) {
    if (!a || !out) return PA_EINVAL;
    const GemmPlan pl = x ? plan_norm_a(*a, *x, gemm_switches(), cus_for_gemm()) : plan_gemm(*a, gemm_switches(), cus_for_gemm());
    *out = pa_gemm_plan_info();
    if (pl.status) return pl.status;
    out->kind = pl.kind; out->tile_h = pl.tile_h; out->tile_w = pl.tile_w;
    out->grid = pl.grid; out->block = pl.block; out->splitk = pl.splitk; out->units = pl.t.units;
    return 0;
}

// -------------------------------------------------------------------------------------------------
// Several weight-gradient GEMMs in ONE launch of the ring kernel (include/plank_hip.h: pa_gemm_group).  Every member
// must be: bf16 operands with the contraction index strided in both (dY^T X), f32 output, no epilogue beyond the
// split-K slab store (splitk > 1 requires splitk_defer), batch 1, 16-byte aligned.  Anything else: PA_EINVAL and the
// caller launches the members one by one.
// ---- Linear on LayerNorm(Z) without a LayerNorm launch (greedy-decode step: B rows, 17 LayerNorm launches per step) ------
namespace {
template <typename TW>
__global__ __launch_bounds__(256) void ln_fold_weights_kernel(TW* Wf, float* u, float* v, const float* W, const float* bias,
                                                              const float* gamma, const float* beta, int N, int K) {
    __shared__ float red[2][4];
    const int n = blockIdx.x;
    float su = 0.f, sv = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float w = W[(size_t)n * K + k];
        const TW wf = (TW)(w * gamma[k]);
        Wf[(size_t)n * K + k] = wf;
        su += (float)wf;                       // the sum of what the MFMA will really multiply by (the rounded values)
        sv += w * beta[k];
    }
    su = wave_sum(su); sv = wave_sum(sv);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = su; red[1][threadIdx.x >> 6] = sv; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u[n] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        v[n] = (bias ? bias[n] : 0.f) + (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}
}  // namespace
extern "C" int pa_ln_fold_weights(void* Wf, float* u, float* v, const float* W, const float* bias, const float* gamma,
                                  const float* beta, int32_t N, int32_t K, void* stream) {
    if (!Wf || !u || !v || !W || !gamma || !beta || N <= 0 || K <= 0) return PA_EINVAL;
    PA_LAUNCH(ln_fold_weights_kernel<bf16>, dim3(N), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (bf16*)Wf, u, v, W, bias, gamma, beta, N, K);
    return 0;
}
extern "C" int pa_ln_fold_weights_f32(float* Wf, float* u, float* v, const float* W, const float* bias, const float* gamma,
                                      const float* beta, int32_t N, int32_t K, void* stream) {
    if (!Wf || !u || !v || !W || !gamma || !beta || N <= 0 || K <= 0) return PA_EINVAL;
    PA_LAUNCH(ln_fold_weights_kernel<float>, dim3(N), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), Wf, u, v, W, bias, gamma, beta, N, K);
    return 0;
}
extern "C" int pa_gemm_norm_a(const pa_gemm_args* a, const pa_gemm_norm_ext* x, void* stream) {
    if (!a || !x) return PA_EINVAL;
    const GemmPlan pl = plan_norm_a(*a, *x, gemm_switches(), cus_for_gemm());
    if (pl.status) return pl.status;
    GemmP p = GemmP();                                     // (value-initialised: every optional pointer null)
    fill_operands(p, *a);
    p.splitk = 1; p.tiles_per_slice = pl.tiles_per_slice;
    p.vec_ok = pl.vec_ok;
    set_tiling(p, pl.t);
    p.ln_u = x->u; p.ln_gamma = x->gamma; p.ln_beta = x->beta; p.ln_y = x->y; p.ldy = x->ldy; p.ln_eps = x->eps;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (pl.kernel == GK_SMALL) { PA_LAUNCH(gemm3s_kernel, dim3(pl.grid), dim3(pl.block), 0, st, p); return 0; }
    // the skinny forms read the f32 rows behind A; the exact-f32 form always writes its LayerNorm(Z) as f32
    p.ln_zf = x->zf; p.ldzf = x->ldzf; p.ln_y_f32 = a->in_dtype == PA_F32 ? 1 : x->y_f32;
    if (a->in_dtype == PA_F32) PA_LAUNCH((gemm_skinny_kernel<float, true>), dim3(pl.grid), dim3(pl.block), 0, st, p);
    else PA_LAUNCH((gemm_skinny_kernel<bf16, true>), dim3(pl.grid), dim3(pl.block), 0, st, p);
    return 0;
}

extern "C" int pa_gemm_group(const pa_gemm_args* args, int32_t n, void* stream) {
    if (!args || n <= 0 || n > PA_MAX_GROUP) return PA_EINVAL;
    if (!split_on() || args[0].in_dtype != PA_F32) return gemm_group_body(args, n, stream);
    const SplitPlan p = plan_group_split3(args, n, cur_split());
    commit_split3(cur_split(), p);
    if (!p.taken) return PA_EINVAL;                         // the caller launches the members one by one (pa_gemm declines or splits each)
    const int rc = launch_cuts(p, stream);
    return rc ? rc : gemm_group_body(p.inner, n, stream);
}
static int gemm_group_body(const pa_gemm_args* args, int32_t n, void* stream) {
    static_assert(PA_MAX_GROUP == PA_MAX_GROUP_, "header / kernel table size");
    GemmGroup g; g.n = n; g.begin[0] = 0;
    int valid = 0;
    for (int i = 0; i < n; ++i) {
        const pa_gemm_args* a = &args[i];
        if (!a->A || !a->B || !a->C || a->M <= 0 || a->N <= 0 || a->K <= 0) return PA_EINVAL;
        if (a->in_dtype != PA_BF16 || a->out_dtype != PA_F32 || a->a_kcontig || a->b_kcontig || a->batch != 1) return PA_EINVAL;
        if (a->bias || a->R || a->aux || a->relu || a->drop_p > 0.f || a->alpha != 1.f) return PA_EINVAL;
        if (!is_aligned<bf16>(a)) return PA_EINVAL;
        const int nt = (a->K + 63) / 64, splitk = eff_splitk(nt, a->splitk);
        if (splitk > 1 && (!a->ws || !a->splitk_defer)) return PA_EINVAL;
        GemmP& p = g.p[i];
        p = GemmP{};
        fill_operands(p, *a);
        p.splitk = splitk; p.tiles_per_slice = (nt + splitk - 1) / splitk;
        set_tiling(p, BM, BN, splitk, UNITS_PLAIN);                      // plain unit order: every unit valid
        if (splitk > 1) { p.C = a->ws; p.ldc = a->N; }
        p.vec_ok = vec_ok(p.C, p.ldc, 0, 4);
        g.begin[i + 1] = g.begin[i] + p.units;
        valid += p.units;
        record_args(*a);
        record_kind(PA_GEMM_KIND_RING, g_rec_ngroups);
    }
    if (g_rec) { std::lock_guard<std::mutex> lk(g_rec_mu); if (g_rec) ++g_rec_ngroups; }
    const int cus = cus_for_gemm();
    int grid = valid < cus ? valid : cus;
    g.xcd_chunk = 0;
    if (gemm_switches().dw_xcd && valid >= 64) {                 // (a handful of units: nothing to share)
        g.xcd_chunk = (valid + 7) / 8;
        grid = (grid + 7) / 8 * 8;                  // slots of a block stay on its XCD
        if (grid > 8 * g.xcd_chunk) grid = 8 * g.xcd_chunk;
    }
    PA_LAUNCH((gemm3_kernel<false, false, GemmGroup>), dim3(grid), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), g);
    return 0;
}

// -------------------------------------------------------------------------------------------------
// deferred split-K reduction of several plain f32 outputs in one launch (include/plank_hip.h)
namespace {
struct ReduceTab { pa_reduce_desc d[PA_MAX_REDUCE]; int begin[PA_MAX_REDUCE + 1]; int n; };
__device__ __forceinline__ void reduce_block(const ReduceTab& t, int blk) {
    // block -> descriptor (few entries: linear scan), then 1024 consecutive floats of its output
    int di = 0;
    while (di + 1 < t.n && blk >= t.begin[di + 1]) ++di;
    const pa_reduce_desc d = t.d[di];
    const size_t total = (size_t)d.rows * d.cols;
    const size_t e0 = ((size_t)(blk - t.begin[di]) * 256 + threadIdx.x) * 4;
    if (e0 >= total) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if ((d.cols & 3) == 0) {
#pragma unroll 4
        for (int s = 0; s < d.splitk; ++s) acc += *reinterpret_cast<const f32x4*>(d.ws + (size_t)s * total + e0);
        const size_t m = e0 / d.cols, n = e0 - m * d.cols;
        *reinterpret_cast<f32x4*>(d.out + m * d.ld_out + n) = acc;
    } else {
        for (int j = 0; j < 4 && e0 + j < total; ++j) {
            float v = 0.f;
            for (int s = 0; s < d.splitk; ++s) v += d.ws[(size_t)s * total + e0 + j];
            const size_t m = (e0 + j) / d.cols, n = (e0 + j) - m * d.cols;
            d.out[m * d.ld_out + n] = v;
        }
    }
}
__global__ __launch_bounds__(256) void splitk_reduce_many_kernel(ReduceTab t) { reduce_block(t, blockIdx.x); }
}  // namespace
extern "C" int pa_splitk_reduce_many(const pa_reduce_desc* descs, int32_t n_desc, void* stream) {
    if (!descs || n_desc <= 0 || n_desc > PA_MAX_REDUCE) return PA_EINVAL;
    ReduceTab t; t.n = n_desc; t.begin[0] = 0;
    for (int i = 0; i < n_desc; ++i) {
        const pa_reduce_desc& d = descs[i];
        if (!d.ws || !d.out || d.rows <= 0 || d.cols <= 0 || d.splitk < 1 || d.ld_out < d.cols) return PA_EINVAL;
        if ((reinterpret_cast<uintptr_t>(d.ws) & 15) || (reinterpret_cast<uintptr_t>(d.out) & 15) || ((d.cols & 3) == 0 && (d.ld_out & 3))) return PA_EALIGN;
        t.d[i] = d;
        t.begin[i + 1] = t.begin[i] + (int)(((size_t)d.rows * d.cols + 1023) / 1024);
    }
    PA_LAUNCH(splitk_reduce_many_kernel, dim3(t.begin[n_desc]), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), t);
    return 0;
}

// -------------------------------------------------------------------------------------------------
// Linear + bias (+ dropout) + residual + LayerNorm in ONE launch, for the post-norm sublayer tails
//     z = r + drop(x W^T + b) ;  y = LN(z)           (reference torch transformer.py: x = norm(x + dropout(sublayer(x))))
// whose N is the model width (512): LayerNorm needs whole rows, so a block owns 32 rows x all 512 columns and streams the
// whole [512][K] weight through its CU (4-stage ring of 32-wide K tiles: 2 KB of A + 32 KB of W per stage, three tiles in
// flight, direct-to-LDS DMA through buffer descriptors - rows past M read as zeros).  Eight waves (two per SIMD cover each other's LDS / barrier
// waits), each 32 rows x 64 columns (two 32 x 32 MFMA tiles, the A fragment shared).  Epilogue: the f32 accumulators go through LDS (32 x 512 f32 = 64 KB, over the ring) into
// the row-per-wave layout of layernorm_fwd_kernel; bias / dropout / residual are applied there in the order of the GEMM
// epilogues, z is rounded to bf16 and the statistics are taken from the ROUNDED values in layernorm_fwd_kernel's summation
// order - z, y, mean and rstd are bit-identical to pa_gemm followed by pa_layernorm_fwd (tests/test_kernels_gpu.py).
// Per-CU arithmetic intensity is a quarter of the 128 x 128 tiling's (every block re-reads the whole weight from L2), so this
// pays where the separate launches are latency-bound: 256 ... 8 192 rows.
namespace {
struct GemmLnP {
    const void* A; const void* W; const float* bias; const void* R;
    void* Z; void* Y; const float* gamma; const float* beta; float* mean; float* rstd;
    int M, K, lda, ldw, ldr, ldz, ldy;
    float eps;
    uint32_t drop_thr; float drop_scale; uint32_t drop_seed;
};
constexpr int GL_N = 512, GL_BM = 32, GL_BK = 32, GL_NSTG = 4, GL_NT = 512;   // 8 waves: two per SIMD hide each other's waits
constexpr int GL_A = GL_BM * GL_BK * 2, GL_STAGE = GL_A + GL_N * GL_BK * 2;   // 2 KB of A + 32 KB of W per stage

__device__ __forceinline__ __amdgpu_buffer_rsrc_t gl_rsrc(const void* base, long long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(bytes < 0x7fffffffLL ? (bytes > 0 ? bytes : 0) : 0x7fffffffLL), 0x00020000);
}

__global__ __launch_bounds__(GL_NT, 2) void gemm_ln_kernel(GemmLnP p) {
    __shared__ __attribute__((aligned(256))) char smem[GL_NSTG * GL_STAGE];      // 136 KB; the epilogue's 64 KB overlay it
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                   // 0..7: columns 64 * wave .. + 63
    const int m0 = blockIdx.x * GL_BM;
    const int nt = p.K / GL_BK;
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    // ---- DMA: LDS rows are 64 bytes (32 bf16); a DMA instruction of a wave fills 16 rows.  Thread -> (row tid / 4 of a
    // 128-row group, 16-byte slot tid % 4); the slot holds source chunk slot ^ ((row >> 2) & 3), which spreads the 16 rows
    // a ds_read_b128 phase touches (64-byte stride) over all 16 bank groups.
    const __amdgpu_buffer_rsrc_t rsA = gl_rsrc(reinterpret_cast<const char*>(p.A) + (size_t)m0 * p.lda * 2, (long long)(p.M - m0) * p.lda * 2);
    const __amdgpu_buffer_rsrc_t rsW = gl_rsrc(p.W, (long long)GL_N * p.ldw * 2);
    const int drow = tid >> 2, dch = ((tid & 3) ^ (drow >> 2)) & 3;
    const int voffA = drow * p.lda * 2 + dch * 16, voffW = drow * p.ldw * 2 + dch * 16;
    const int wstep = 128 * p.ldw * 2;                              // 128 weight rows further per DMA instruction
    const bool a_wave = wave < 2;                                   // the 32 A rows are two waves' worth of chunks
    auto issue = [&](int t) {
        char* base = smem + (t & (GL_NSTG - 1)) * GL_STAGE;
        const int k0 = t * (GL_BK * 2);                             // byte offset of the K tile inside a row
        if (a_wave)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(base + wave * 1024), 16, voffA, k0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (__attribute__((address_space(3))) void*)(base + GL_A + i * 8192 + wave * 1024), 16,
                                                     voffW, k0 + i * wstep, 0, 0);
    };
    // wait until at most `younger` K tiles issued after the one needed are still in flight (5 DMA instructions per tile in
    // the two waves that also carry A, 4 in the others)
    auto wait_tiles = [&](int younger) {
        if (a_wave) {
            if (younger >= 2) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
            else if (younger == 1) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            if (younger >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else if (younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    };

    // ---- fragment addresses: row lane & 31 of a 32-row tile, k-step s reads source chunk 2s + half (swizzled slot)
    const int sw = ((lane & 31) >> 2) & 3;
    int xs[2];
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) xs[s_] = (((2 * s_ + half) ^ sw) & 3) << 4;
    const int fa = (lane & 31) * 64, fb = GL_A + (wave * 64 + (lane & 31)) * 64;

    // three K tiles ahead: a tile's DMA has three tile-times to cover the L2 latency
    int issued = 0;
#pragma unroll 1
    for (; issued < 3 && issued < nt; ++issued) issue(issued);
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
        wait_tiles(issued - t - 1);
        __builtin_amdgcn_s_barrier();                               // K tile t has landed for every wave, and every wave has
                                                                    // finished tile t - 1: its stage is free for tile t + 3
        if (issued < nt) { issue(issued); ++issued; }
        const char* st = smem + (t & (GL_NSTG - 1)) * GL_STAGE;
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
            const u32x4 a = *reinterpret_cast<const u32x4*>(st + fa + xs[s_]);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const u32x4 b = *reinterpret_cast<const u32x4*>(st + fb + j * 2048 + xs[s_]);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&b), *reinterpret_cast<const bf16x8*>(&a), acc[j], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // this wave's LDS reads of the stage are complete
    }
    __syncthreads();                                                // all stages consumed: the epilogue may overlay them

    // ---- accumulators -> LDS, [32][512] f32, 16-byte chunk c of row m at slot c ^ (m & 7) ------------------------------
    {
        const int m = lane & 31;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[j][4 * g4 + e];
                const int c = wave * 16 + 8 * j + 2 * g4 + half;  // columns 4c .. 4c + 3
                *reinterpret_cast<f32x4*>(smem + m * 2048 + ((c ^ (m & 7)) << 4)) = v;
            }
    }
    __syncthreads();

    // ---- row-per-wave tail: lane owns columns 4 * lane .. + 3 and 256 + 4 * lane .. + 3 (layernorm_fwd_kernel's mapping);
    // wave w takes rows 4w .. 4w + 3
    constexpr int RPW = GL_BM / (GL_NT / 64);
    const int c0 = lane << 2, c1 = (lane + 64) << 2;
    const f32x4 b0 = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + c0) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 b1 = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + c1) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(p.gamma + c0), g1 = *reinterpret_cast<const f32x4*>(p.gamma + c1);
    const f32x4 e0 = *reinterpret_cast<const f32x4*>(p.beta + c0), e1 = *reinterpret_cast<const f32x4*>(p.beta + c1);
    const bf16* R = reinterpret_cast<const bf16*>(p.R);
    bf16* Z = reinterpret_cast<bf16*>(p.Z);
    bf16* Y = reinterpret_cast<bf16*>(p.Y);
    f32x4 r0[RPW], r1[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int m = min(m0 + wave * RPW + i, p.M - 1);
        r0[i] = R ? ld4<bf16>(R + (size_t)m * p.ldr + c0) : f32x4{0.f, 0.f, 0.f, 0.f};
        r1[i] = R ? ld4<bf16>(R + (size_t)m * p.ldr + c1) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int lr = wave * RPW + i, m = m0 + lr;
        if (m >= p.M) break;                                        // wave-uniform
        f32x4 x0 = *reinterpret_cast<const f32x4*>(smem + lr * 2048 + ((lane ^ (lr & 7)) << 4));
        f32x4 x1 = *reinterpret_cast<const f32x4*>(smem + lr * 2048 + (((lane + 64) ^ (lr & 7)) << 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float y0 = x0[e] * 1.0f + b0[e], y1 = x1[e] * 1.0f + b1[e];
            if (p.drop_thr) {
                y0 = drop_keep_rc(p.drop_seed, (uint32_t)m, (uint32_t)(c0 + e), p.drop_thr) ? y0 * p.drop_scale : 0.f;
                y1 = drop_keep_rc(p.drop_seed, (uint32_t)m, (uint32_t)(c0 + e + 256), p.drop_thr) ? y1 * p.drop_scale : 0.f;
            }
            if (R) { y0 += r0[i][e]; y1 += r1[i][e]; }
            x0[e] = y0; x1[e] = y1;
        }
        // z in bf16 (what the backward reads); the statistics see exactly these rounded values
        u32x2 z0, z1;
        z0[0] = pack_bf16(x0[0], x0[1]); z0[1] = pack_bf16(x0[2], x0[3]);
        z1[0] = pack_bf16(x1[0], x1[1]); z1[1] = pack_bf16(x1[2], x1[3]);
        if (Z) {
            *reinterpret_cast<u32x2*>(Z + (size_t)m * p.ldz + c0) = z0;
            *reinterpret_cast<u32x2*>(Z + (size_t)m * p.ldz + c1) = z1;
        }
        f32x4 v0, v1;
        v0[0] = bf16_lo(z0[0]); v0[1] = bf16_hi(z0[0]); v0[2] = bf16_lo(z0[1]); v0[3] = bf16_hi(z0[1]);
        v1[0] = bf16_lo(z1[0]); v1[1] = bf16_hi(z1[0]); v1[2] = bf16_lo(z1[1]); v1[3] = bf16_hi(z1[1]);
        float s = 0.f;
        s += v0[0] + v0[1] + v0[2] + v0[3];
        s += v1[0] + v1[1] + v1[2] + v1[3];
        const float mu = wave_sum(s) / GL_N;
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float t_ = v0[e] - mu; q += t_ * t_; }
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float t_ = v1[e] - mu; q += t_ * t_; }
        const float rs = 1.0f / sqrtf(wave_sum(q) / GL_N + p.eps);
        if (lane == 0) { if (p.mean) p.mean[m] = mu; if (p.rstd) p.rstd[m] = rs; }
        f32x4 o0, o1;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o0[e] = (v0[e] - mu) * rs * g0[e] + e0[e]; o1[e] = (v1[e] - mu) * rs * g1[e] + e1[e]; }
        st4<bf16>(Y + (size_t)m * p.ldy + c0, o0);
        st4<bf16>(Y + (size_t)m * p.ldy + c1, o1);
    }
}
}  // namespace

extern "C" int pa_gemm_ln_max_rows(void) { return 256 * GL_BM; }

extern "C" int pa_gemm_ln(const pa_gemm_ln_args* a, void* stream) {
    if (!a || !a->A || !a->W || !a->Y || !a->gamma || !a->beta) return PA_EINVAL;
    if (a->M <= 0 || a->K <= 0 || a->N != GL_N || (a->K % 64) != 0) return PA_EINVAL;
    if (a->drop_p < 0.f || a->drop_p >= 1.f) return PA_EINVAL;
    auto al = [](const void* q, int bytes) { return !q || reinterpret_cast<uintptr_t>(q) % bytes == 0; };
    if (!al(a->A, 16) || !al(a->W, 16) || (a->lda % 8) || (a->ldw % 8) || a->lda < a->K || a->ldw < a->K) return PA_EALIGN;
    if (!al(a->R, 8) || !al(a->Z, 8) || !al(a->Y, 8) || (a->R && (a->ldr % 4)) || (a->Z && (a->ldz % 4)) || (a->ldy % 4)) return PA_EALIGN;
    if (!al(a->bias, 16) || !al(a->gamma, 16) || !al(a->beta, 16)) return PA_EALIGN;
    if ((long long)GL_N * a->ldw * 2 > 0x7fffffffLL) return PA_EINVAL;
    GemmLnP p;
    p.A = a->A; p.W = a->W; p.bias = a->bias; p.R = a->R; p.Z = a->Z; p.Y = a->Y;
    p.gamma = a->gamma; p.beta = a->beta; p.mean = a->mean; p.rstd = a->rstd;
    p.M = a->M; p.K = a->K; p.lda = a->lda; p.ldw = a->ldw; p.ldr = a->ldr; p.ldz = a->ldz; p.ldy = a->ldy;
    p.eps = a->eps;
    p.drop_thr = (uint32_t)((double)a->drop_p * 4294967296.0);           // as pa_gemm
    p.drop_scale = (float)(1.0 / (1.0 - (double)p.drop_thr / 4294967296.0));
    p.drop_seed = a->drop_seed;
    const int grid = (a->M + GL_BM - 1) / GL_BM;
    PA_LAUNCH(gemm_ln_kernel, dim3(grid), dim3(GL_NT), 0, reinterpret_cast<hipStream_t>(stream), p);
    return 0;
}

// -------------------------------------------------------------------------------------------------
// column sums (bias gradients): block = 64 sixteen-byte column chunks x 4 row lanes over CS_ROWS rows, partial rows
// combined by a second small kernel.  HBM-bound: one coalesced pass over X.
namespace {
constexpr int CS_ROWS = 128;
// out[n] += sum over this block's rows (f32 atomics: one per column per 128-row block)
template <typename T, bool VEC>
__device__ __forceinline__ void colsum_block(const T* X, int M, int N, int ldx, float* out, int bx, int by, int rows_per_block = CS_ROWS) {
    constexpr int EB = ET<T>::EB;
    __shared__ float red[4][64 * EB];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int n0 = (bx * 64 + cl) * EB;
    const int r0 = by * rows_per_block, r1 = min(M, r0 + rows_per_block);   // (rows_per_block >= M: the only contributor)
    float acc[EB];
#pragma unroll
    for (int e = 0; e < EB; ++e) acc[e] = 0.f;
    if (n0 < N) {
#pragma unroll 4
        for (int r = r0 + rl; r < r1; r += 4) {
            const T* p = X + (size_t)r * ldx + n0;
            if (VEC) {
#pragma unroll
                for (int e = 0; e < EB; e += 4) { const f32x4 v = ld4<T>(p + e); acc[e] += v[0]; acc[e + 1] += v[1]; acc[e + 2] += v[2]; acc[e + 3] += v[3]; }
            } else {
#pragma unroll
                for (int e = 0; e < EB; ++e) if (n0 + e < N) acc[e] += ld1(p + e);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < EB; ++e) red[rl][cl * EB + e] = acc[e];
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * EB; i += 256) {
        const int n = bx * 64 * EB + i;
        if (n < N) unsafeAtomicAdd(out + n, (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]));
    }
}
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void colsum_kernel(const T* X, int M, int N, int ldx, float* out, int rows_per_block) {
    colsum_block<T, VEC>(X, M, N, ldx, out, blockIdx.x, blockIdx.y, rows_per_block);
}
// The ordered form (one contributor per output element: the f32 parity path, pa_device.h pa_ordered_reductions): a block owns
// 4 sixteen-byte column chunks and walks ALL rows on 64 row lanes; the lanes' sums are combined in lane order.  (Rounds 1-3
// used the 64-chunk x 4-lane block for this too: a 512-column bias gradient was two blocks walking 8 700 rows - 280 us per
// segment tail, 11 % of the f32 step.  Same result on every run either way; the order of the additions differs from round 3.)
template <typename T>
__device__ __forceinline__ void colsum_block_ordered(const T* X, int M, int N, int ldx, float* out, int bx) {
    constexpr int EB = ET<T>::EB, CCH = 4, RL = 64;
    __shared__ float red_o[RL][CCH * EB + 1];
    const int cl = threadIdx.x & (CCH - 1), rl = threadIdx.x / CCH;
    const int n0 = (bx * CCH + cl) * EB;
    float acc[EB];
#pragma unroll
    for (int e = 0; e < EB; ++e) acc[e] = 0.f;
    if (n0 < N) {
#pragma unroll 8
        for (int r = rl; r < M; r += RL) {
            const T* p = X + (size_t)r * ldx + n0;
#pragma unroll
            for (int e = 0; e < EB; e += 4) { const f32x4 v = ld4<T>(p + e); acc[e] += v[0]; acc[e + 1] += v[1]; acc[e + 2] += v[2]; acc[e + 3] += v[3]; }
        }
    }
#pragma unroll
    for (int e = 0; e < EB; ++e) red_o[rl][cl * EB + e] = acc[e];
    __syncthreads();
    if (threadIdx.x < CCH * EB) {
        const int n = bx * CCH * EB + threadIdx.x;
        if (n < N) {
            float sum = 0.f;
            for (int i = 0; i < RL; ++i) sum += red_o[i][threadIdx.x];
            out[n] += sum;                                   // the only contributor (gradients are accumulated into)
        }
    }
}
// several matrices in one launch: block -> (descriptor, column block, row block)
struct ColsumTab { pa_colsum_desc d[PA_MAX_COLSUM]; int begin[PA_MAX_COLSUM + 1]; int n; int ordered; };
static inline int colsum_blocks(int M, int N, int EB, bool ordered) {
    return ordered ? (N + 4 * EB - 1) / (4 * EB) : ((N + 64 * EB - 1) / (64 * EB)) * ((M + CS_ROWS - 1) / CS_ROWS);
}
template <typename T>
__device__ __forceinline__ void colsum_many_block(const ColsumTab& t, int blk) {
    constexpr int EB = ET<T>::EB;
    int di = 0;
    while (di + 1 < t.n && blk >= t.begin[di + 1]) ++di;
    const pa_colsum_desc d = t.d[di];
    const int rel = blk - t.begin[di];
    if (t.ordered) { colsum_block_ordered<T>(reinterpret_cast<const T*>(d.X), d.M, d.N, d.ldx, d.out, rel); return; }
    const int nbx = (d.N + 64 * EB - 1) / (64 * EB);
    colsum_block<T, true>(reinterpret_cast<const T*>(d.X), d.M, d.N, d.ldx, d.out, rel % nbx, rel / nbx, CS_ROWS);
}
template <typename T>
__global__ __launch_bounds__(256) void colsum_many_kernel(ColsumTab t) { colsum_many_block<T>(t, blockIdx.x); }

// ---- the whole tail of a backward segment in ONE launch: LayerNorm gamma/beta finishes, bias column sums and split-K
// slab reductions are independent of each other; their blocks are simply concatenated (every dependent launch saved
// is ~5 us on this machine)
// LN_CHUNKS blocks share the partial rows of one (LayerNorm, statistic, 64-column block): with 8-row LayerNorm-backward
// blocks there are ~1 000 partial rows per LayerNorm, and 24 blocks walking them 4 at a time were the longest part of the
// tail.  The chunk sums are combined with one f32 atomic per column.
constexpr int LN_CHUNKS = 8;
struct LnTailTab { pa_ln_finish_desc d[PA_MAX_LN_FINISH]; int n; int ncols; int nbx; int nby; int chunks; };
__device__ __forceinline__ void ln_finish_block(const LnTailTab& t, int blk) {
    __shared__ float red_ln[256];
    const int ch = blk % t.chunks; blk /= t.chunks;      // (chunks == 1: ordered - this block is the only contributor)
    const int bx = blk % t.nbx, by = (blk / t.nbx) % t.nby, bz = blk / (t.nbx * t.nby);
    const pa_ln_finish_desc d = t.d[bz];
    const int c = bx * 64 + (threadIdx.x & 63), pl = threadIdx.x >> 6;
    float* o = by == 0 ? d.dgamma : (by == 1 ? d.dbeta : d.dzsum);
    const int per = (d.nparts + t.chunks - 1) / t.chunks, i0 = ch * per, i1 = min(d.nparts, i0 + per);
    float sacc = 0.f;
    if (c < t.ncols && o) {
        const float* p = d.partial + (size_t)by * t.ncols + c;
#pragma unroll 8
        for (int i = i0 + pl; i < i1; i += 4) sacc += p[(size_t)i * 3 * t.ncols];
    }
    red_ln[threadIdx.x] = sacc;
    __syncthreads();
    if (pl == 0 && c < t.ncols && o && i0 < i1)
        unsafeAtomicAdd(o + c, (red_ln[threadIdx.x] + red_ln[threadIdx.x + 64]) + (red_ln[threadIdx.x + 128] + red_ln[threadIdx.x + 192]));
}
template <typename T>
__global__ __launch_bounds__(256) void segment_tail_kernel(LnTailTab ln, int n_ln_blocks, ColsumTab cs, int n_cs_blocks, ReduceTab rd) {
    const int b = blockIdx.x;                      // block-uniform dispatch
    if (b < n_ln_blocks) ln_finish_block(ln, b);
    else if (b < n_ln_blocks + n_cs_blocks) colsum_many_block<T>(cs, b - n_ln_blocks);
    else reduce_block(rd, b - n_ln_blocks - n_cs_blocks);
}
}  // namespace
extern "C" int pa_segment_tail(const pa_ln_finish_desc* ln, int32_t n_ln, int32_t d_model, const pa_colsum_desc* cs, int32_t n_cs,
                               int32_t dtype, const pa_reduce_desc* rd, int32_t n_rd, void* stream) {
    if (n_ln < 0 || n_ln > PA_MAX_LN_FINISH || n_cs < 0 || n_cs > PA_MAX_COLSUM || n_rd < 0 || n_rd > PA_MAX_REDUCE) return PA_EINVAL;
    if ((n_ln && !ln) || (n_cs && !cs) || (n_rd && !rd) || n_ln + n_cs + n_rd == 0) return PA_EINVAL;
    if (dtype != PA_BF16 && dtype != PA_F32) return PA_EINVAL;
    const int EB = dtype == PA_BF16 ? 8 : 4;
    const bool ordered = pa_ordered_reductions(dtype);
    LnTailTab lt; lt.n = n_ln; lt.ncols = d_model; lt.nbx = (d_model + 63) / 64; lt.nby = 2; lt.chunks = ordered ? 1 : LN_CHUNKS;
    for (int i = 0; i < n_ln; ++i) {
        if (!ln[i].partial || !ln[i].dgamma || !ln[i].dbeta || ln[i].nparts <= 0 || d_model <= 0) return PA_EINVAL;
        lt.d[i] = ln[i];
        if (ln[i].dzsum) lt.nby = 3;
    }
    const int n_ln_blocks = n_ln ? lt.nbx * lt.nby * n_ln * lt.chunks : 0;
    ColsumTab ct; ct.n = n_cs; ct.begin[0] = 0; ct.ordered = ordered;
    for (int i = 0; i < n_cs; ++i) {
        const pa_colsum_desc& d = cs[i];
        if (!d.X || !d.out || d.M <= 0 || d.N <= 0) return PA_EINVAL;
        if ((reinterpret_cast<uintptr_t>(d.X) & 15) || d.ldx % EB || d.ldx < (d.N + EB - 1) / EB * EB) return PA_EALIGN;
        ct.d[i] = d;
        ct.begin[i + 1] = ct.begin[i] + colsum_blocks(d.M, d.N, EB, ordered);
    }
    ReduceTab rt; rt.n = n_rd; rt.begin[0] = 0;
    for (int i = 0; i < n_rd; ++i) {
        const pa_reduce_desc& d = rd[i];
        if (!d.ws || !d.out || d.rows <= 0 || d.cols <= 0 || d.splitk < 1 || d.ld_out < d.cols) return PA_EINVAL;
        if ((reinterpret_cast<uintptr_t>(d.ws) & 15) || (reinterpret_cast<uintptr_t>(d.out) & 15) || ((d.cols & 3) == 0 && (d.ld_out & 3))) return PA_EALIGN;
        rt.d[i] = d;
        rt.begin[i + 1] = rt.begin[i] + (int)(((size_t)d.rows * d.cols + 1023) / 1024);
    }
    const int total = n_ln_blocks + ct.begin[n_cs] + rt.begin[n_rd];
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == PA_BF16) PA_LAUNCH(segment_tail_kernel<bf16>, dim3(total), dim3(256), 0, st, lt, n_ln_blocks, ct, ct.begin[n_cs], rt);
    else PA_LAUNCH(segment_tail_kernel<float>, dim3(total), dim3(256), 0, st, lt, n_ln_blocks, ct, ct.begin[n_cs], rt);
    return 0;
}
extern "C" int pa_colsum_many(const pa_colsum_desc* descs, int32_t n_desc, int32_t dtype, void* stream) {
    if (!descs || n_desc <= 0 || n_desc > PA_MAX_COLSUM) return PA_EINVAL;
    const int EB = dtype == PA_BF16 ? 8 : 4;
    const bool ordered = pa_ordered_reductions(dtype);
    ColsumTab t; t.n = n_desc; t.begin[0] = 0; t.ordered = ordered;
    for (int i = 0; i < n_desc; ++i) {
        const pa_colsum_desc& d = descs[i];
        if (!d.X || !d.out || d.M <= 0 || d.N <= 0) return PA_EINVAL;
        // vector path only: 16-byte aligned rows whose allocation covers the last vector
        if ((reinterpret_cast<uintptr_t>(d.X) & 15) || d.ldx % EB || d.ldx < (d.N + EB - 1) / EB * EB) return PA_EALIGN;
        t.d[i] = d;
        t.begin[i + 1] = t.begin[i] + colsum_blocks(d.M, d.N, EB, ordered);
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == PA_BF16) PA_LAUNCH(colsum_many_kernel<bf16>, dim3(t.begin[n_desc]), dim3(256), 0, st, t);
    else if (dtype == PA_F32) PA_LAUNCH(colsum_many_kernel<float>, dim3(t.begin[n_desc]), dim3(256), 0, st, t);
    else return PA_EINVAL;
    return 0;
}

// -------------------------------------------------------------------------------------------------
// batched 2-D transposes (bf16/f32): dst[c][r] = src[r][c] for a table of matrices, one launch.  Used to keep a
// transposed shadow of the Linear weights so that dX = dY W runs on the k-contiguous fast path.
namespace {
template <typename T>
__global__ __launch_bounds__(256) void transpose_many_kernel(const pa_tr_desc* descs, int n_desc) {
    __shared__ T tile[64][65];
    int t = blockIdx.x, di = 0;
    while (di + 1 < n_desc && t >= descs[di + 1].tile_begin) ++di;     // few dozen descriptors: linear scan
    const pa_tr_desc d = descs[di];
    t -= d.tile_begin;
    const int tiles_c = (d.cols + 63) / 64;
    const int r0 = (t / tiles_c) * 64, c0 = (t % tiles_c) * 64;
    const T* src = reinterpret_cast<const T*>(d.src);
    T* dst = reinterpret_cast<T*>(d.dst);
    if constexpr (sizeof(T) == 2) {
        // 8-byte accesses: thread -> (row = t/16 + 16k, 4 columns).  Needs 4-element aligned rows on both sides;
        // loads are unconditional (clamped), stores are predicated per element at the edges (padding stays untouched).
        const bool wide = ((d.ld_src | d.ld_dst | d.cols) & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 7) == 0 &&
                          (reinterpret_cast<uintptr_t>(dst) & 7) == 0;
        if (wide) {
            const int tr = threadIdx.x >> 4, tc = (threadIdx.x & 15) * 4;
            u32x2 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int rr = min(r0 + tr + 16 * k, d.rows - 1), cc = min(c0 + tc, d.cols - 4);
                v[k] = *reinterpret_cast<const u32x2*>(src + (size_t)rr * d.ld_src + cc);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint16_t* row = reinterpret_cast<uint16_t*>(&tile[tr + 16 * k][tc]);
                row[0] = (uint16_t)(v[k][0] & 0xffffu); row[1] = (uint16_t)(v[k][0] >> 16);
                row[2] = (uint16_t)(v[k][1] & 0xffffu); row[3] = (uint16_t)(v[k][1] >> 16);
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int oc = c0 + tr + 16 * k;                 // destination row = source column
                const int orow = r0 + tc;                         // destination columns orow .. orow + 3 = source rows
                if (oc >= d.cols || orow >= d.rows) continue;
                const uint16_t* tp = reinterpret_cast<const uint16_t*>(&tile[0][0]);
                uint16_t e[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) e[q] = tp[(tc + q) * 65 + tr + 16 * k];
                T* o = dst + (size_t)oc * d.ld_dst + orow;
                if (orow + 3 < d.rows) {
                    u32x2 w; w[0] = (uint32_t)e[0] | ((uint32_t)e[1] << 16); w[1] = (uint32_t)e[2] | ((uint32_t)e[3] << 16);
                    *reinterpret_cast<u32x2*>(o) = w;
                } else {
                    for (int q = 0; q < 4 && orow + q < d.rows; ++q) reinterpret_cast<uint16_t*>(o)[q] = e[q];
                }
            }
            return;
        }
    }
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int cc = min(c0 + tx, d.cols - 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int rr = ty + 4 * i;
        tile[rr][tx] = src[(size_t)min(r0 + rr, d.rows - 1) * d.ld_src + cc];
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4)
        if (c0 + i < d.cols && r0 + tx < d.rows) dst[(size_t)(c0 + i) * d.ld_dst + r0 + tx] = tile[tx][i];
}
}  // namespace

extern "C" int pa_transpose_many(const pa_tr_desc* descs_dev, int32_t n_desc, int32_t total_tiles, int32_t dtype, void* stream) {
    if (!descs_dev || n_desc <= 0 || total_tiles <= 0) return PA_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == PA_BF16) PA_LAUNCH(transpose_many_kernel<bf16>, dim3(total_tiles), dim3(256), 0, st, descs_dev, n_desc);
    else if (dtype == PA_F32) PA_LAUNCH(transpose_many_kernel<float>, dim3(total_tiles), dim3(256), 0, st, descs_dev, n_desc);
    else return PA_EINVAL;
    return 0;
}

extern "C" int64_t pa_colsum_ws_floats(int32_t M, int32_t N) { (void)M; (void)N; return 64; }
extern "C" int pa_colsum(const void* X, int32_t dtype, int32_t M, int32_t N, int32_t ldx, float* out,
                         int32_t accumulate, float* partial, void* stream) {
    (void)partial;
    if (!X || !out || M <= 0 || N <= 0) return PA_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!accumulate) {
        hipError_t e = hipMemsetAsync(out, 0, (size_t)N * sizeof(float), st);
        if (e != hipSuccess) return (int)e;
    }
    const bool ordered = pa_ordered_reductions(dtype);
    const int nparts = ordered ? 1 : (M + CS_ROWS - 1) / CS_ROWS, rpb = ordered ? M : CS_ROWS;
    const int EB = dtype == PA_BF16 ? 8 : 4;
    // vector path: every 16-byte chunk of a row is fully inside the row allocation (ldx >= round-up of N) and aligned
    const bool vec = (reinterpret_cast<uintptr_t>(X) & 15) == 0 && ldx % EB == 0 && ldx >= (N + EB - 1) / EB * EB;
    dim3 grid((N + 64 * EB - 1) / (64 * EB), nparts);
    if (dtype == PA_BF16) {
        if (vec) PA_LAUNCH((colsum_kernel<bf16, true>), grid, dim3(256), 0, st, (const bf16*)X, M, N, ldx, out, rpb);
        else PA_LAUNCH((colsum_kernel<bf16, false>), grid, dim3(256), 0, st, (const bf16*)X, M, N, ldx, out, rpb);
    } else {
        if (vec) PA_LAUNCH((colsum_kernel<float, true>), grid, dim3(256), 0, st, (const float*)X, M, N, ldx, out, rpb);
        else PA_LAUNCH((colsum_kernel<float, false>), grid, dim3(256), 0, st, (const float*)X, M, N, ldx, out, rpb);
    }
    return 0;
}

#ifdef PA_GEMM_TRACE3
extern "C" int pa_gemm3_trace_read(unsigned long long* out, int32_t n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pa_gemm3_trace), sizeof(unsigned long long) * (size_t)n);
}
extern "C" int pa_gemm3_items_read(unsigned long long* out) {      // out[0..63] stamps, returns the item count
    int n = 0;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pa_gemm3_items), sizeof(unsigned long long) * 64) != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(pa_gemm3_nitems), sizeof(int)) != hipSuccess) return -1;
    return n;
}
#endif
