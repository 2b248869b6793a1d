// fp32 MFMA GEMM on v_mfma_f32_32x32x2_f32 for the two big fp32 products of the ELBO fast path:
//   K_ZX-bar = alpha [Q' | a] [A ; mu_bar^T]        dense,  A operand [M][K] or [K][M], B operand [K][N]   (M' x B' x M')
//   [G ; b^T] = tril([A ; mu_bar^T] A^T)             both operands [.][K] (k-contiguous), split-K over the minibatch axis
// 128 x 128 output tiles, 4 waves of 64 x 64 (2 x 2 MFMA tiles of 32 x 32 -> 64 accumulator registers), BK-deep stages
// through ONE LDS buffer per operand with the next stage prefetched into registers under the MFMAs of the current one;
// several workgroups per CU hide each other's stage boundaries (the recipe of gemm64.hip).  Why this MFMA shape: a
// 32 x 32 x 2 instruction does 4096 flops on ONE register of A and ONE of B per lane -- half the LDS fragment traffic per
// flop of the 16 x 16 x 4 form gemm.hip is built on -- and a 64 x 64 wave tile needs 4 fragment reads per 8 MFMAs.
//
// Fragment reads.  Lane l = 32 h + r supplies A[row r][k = h] and B[k = h][col r] to one MFMA.  A k-contiguous operand
// sits in LDS as [mn][BK + 2] floats and every lane reads the PAIR (k0 + 2h, k0 + 2h + 1) with one 8-byte read
// (row stride 34 / 18 words = 2 x odd: the 32 lanes of a read group hit 32 distinct even banks of the 64): the two MFMAs
// of a pair then cover k0 .. k0 + 3 in the order {0, 2}, {1, 3} -- any order is fine as long as both operands use the same.
// An mn-contiguous operand sits as [BK][128 + 4] and is read with two 4-byte reads at rows k0 + 2h, k0 + 2h + 1.
// Staging stores: 8-byte stores for the k-contiguous image (rows are 8-byte aligned), 16-byte for the other.
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "common.h"
#include "gram_walk.h"

namespace {

using acc16 = float __attribute__((ext_vector_type(16)));
using acc4f = float __attribute__((ext_vector_type(4)));
constexpr int TM = 128, TN = 128;

#ifndef G32_BK
#define G32_BK 32
#endif
#ifndef G32_MINW
#define G32_MINW 3          // waves per SIMD the register allocation aims at (workgroups per CU)
#endif
#ifndef G32_BAND
#define G32_BAND 8          // tile columns per XCD-local band of the dense walk
#endif
#ifndef G32_DMA_BK
#define G32_DMA_BK 32       // stage depth of the LDS-DMA kernel (32: two workgroups per CU; 16: three)
#endif
#ifndef G32_MF
#define G32_MF 32           // MFMA shape of the LDS-DMA kernel: 32 (32x32x2) or 16 (16x16x4)
#endif
#ifndef G32_SK_BELOW
#define G32_SK_BELOW 4096   // tile count below which the split-K cost model is consulted (few rounds: a ragged last round costs most)
#endif
#ifndef G32_SK_MINK
#define G32_SK_MINK 512     // shortest K that may be split (slices of >= 256)
#endif
#ifndef G32_WIDE_ROUNDS
#define G32_WIDE_ROUNDS 3   // the 256 x 192 kernel is chosen from this many rounds of 256 x 192 tiles over the CUs on ...
#endif
#ifndef G32_WIDE_FILL
#define G32_WIDE_FILL 90    // ... when the tiles fill their rounds to this many per cent
#endif
#ifndef G32_GRAM_STAGES
#define G32_GRAM_STAGES 160 // the 256 x 256 stream-K kernel is chosen for lower k-contiguous products from this many stages per workgroup on (C4: 234; the 2-rank share: 117)
#endif
#ifndef G32_GRAM_INFLIGHT
#define G32_GRAM_INFLIGHT 16 // atomics of a wave's earlier MFMA tiles that may be in flight when it issues the next tile's 16 (0..62; 63 = uncounted)
#endif
#ifndef G32_GRAM_KCHUNKS
#define G32_GRAM_KCHUNKS 1  // K chunks of the stream-K walk (gram_walk.h); DSVGP_G32_GRAM_KCHUNKS overrides it at a launch
#endif
#ifndef G32_SK_SLOTS
#define G32_SK_SLOTS 256    // work units per round in the split-K cost model: one per CU (a CU's matrix pipe is shared by its resident workgroups)
#endif

struct G32 {
    const float* A; const float* B; float* C;
    int64_t lda, ldb, ldc;
    int M, N, K, tiles_m, tiles_n, flags, splitk, kslice, ntiles;
    float alpha;
    float* slab;             // deterministic mode: K slice s stores its tiles to slab[s][M][N] (summed in a fixed order afterwards)
};

template <int BK, bool KC>
struct Stage {                       // register image of one thread's share of a 128 x BK stage of one operand
    static constexpr int NV = BK / 8;             // float4 per thread
    float4 v[NV];
};

// Ragged edges never take a scalar path: every load is a 16-byte vector load from a CLAMPED address (rows / columns past the
// edge re-read the last valid ones: their products land in output rows / columns that are never stored; the launcher
// checks that the leading dimension covers the last clamped chunk), and only the stage that crosses the end of the K
// range zeroes its k >= kend elements with selects.
// k-contiguous operand P[mn][k]: thread -> (row = tid / (BK/4) + i * 1024/BK, 4 k at 4 (tid % (BK/4)))
template <int BK>
struct FetchKC {
    static constexpr int CPR = BK / 4, RPP = 256 / CPR, NV = BK / 8;
    const float* P;
    int rowoff[NV];          // clamped row * ld
    int kc, klim;            // this thread's k offset inside a stage; last in-bounds chunk start of a row
    __device__ __forceinline__ void init(const float* P_, int64_t ld, int mn0, int MN, int K, int tid) {
        P = P_;
        kc = (tid % CPR) * 4;
        klim = ((K + 3) / 4) * 4 - 4;
#pragma unroll
        for (int i = 0; i < NV; ++i) rowoff[i] = (int)(min(mn0 + tid / CPR + i * RPP, MN - 1) * ld);
    }
    __device__ __forceinline__ void load(int k0, int kend, Stage<BK, true>& s) const {
        const int k = k0 + kc;
        const float* p = P + min(k, klim);
#pragma unroll
        for (int i = 0; i < NV; ++i) s.v[i] = *reinterpret_cast<const float4*>(p + rowoff[i]);
        if (k0 + BK > kend) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                s.v[i].x = (k < kend) ? s.v[i].x : 0.f;
                s.v[i].y = (k + 1 < kend) ? s.v[i].y : 0.f;
                s.v[i].z = (k + 2 < kend) ? s.v[i].z : 0.f;
                s.v[i].w = (k + 3 < kend) ? s.v[i].w : 0.f;
            }
        }
    }
};
// mn-contiguous operand P[k][mn]: thread -> (k = tid / 32 + 8 i, 4 columns at 4 (tid % 32))
template <int BK>
struct FetchMC {
    static constexpr int NV = BK / 8;
    const float* P;
    int64_t ld;
    int kr, K;
    __device__ __forceinline__ void init(const float* P_, int64_t ld_, int mn0, int MN, int K_, int tid) {
        ld = ld_; K = K_;
        kr = tid >> 5;
        P = P_ + min(mn0 + (tid & 31) * 4, ((MN + 3) / 4) * 4 - 4);
    }
    __device__ __forceinline__ void load(int k0, int kend, Stage<BK, false>& s) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int k = k0 + kr + 8 * i;
            s.v[i] = *reinterpret_cast<const float4*>(P + (int64_t)min(k, K - 1) * ld);
            if (k0 + BK > kend && k >= kend) s.v[i] = float4{0.f, 0.f, 0.f, 0.f};
        }
    }
};

// which (tile, K slice) this workgroup takes: consecutive blocks of one XCD (b, b + 8, ...) get consecutive units
// Tried and removed (build-variant clean-up; last present in 8a953b7): the lower triangle walked in SB x SB super-blocks (G32_TRI_SB; round 4,
// same box: Gram at C4 2.169 (1) / 2.193 (8) / 2.222 ms (4) -- no gain); lower-triangular split-K products in eight K slices, one per XCD
// (G32_XCDK; round 6, profiles/r06_b_gemm32_gram_xcd.txt: 2.29 -> 2.33-2.35 ms, the launch is not bound by its traffic).
template <int TM_ = TM, int TN_ = TN>
__device__ __forceinline__ bool pick_unit(const G32& g, int& m0, int& n0, int& kbeg, int& kend) {
    const int u = (blockIdx.x >> 3) + (blockIdx.x & 7) * ((gridDim.x + 7) >> 3);
    if (u >= g.ntiles * g.splitk) return false;
    const int slice = u / g.ntiles;
    const int t = u - slice * g.ntiles;
    int tm, tn;
    if (g.flags & DSVGP_GEMM_OUT_LOWER) {
        // tiles with tn <= tm, row by row: the triangle t = tm (tm + 1) / 2 + tn while tm < tiles_n, full rows of
        // tiles_n tiles below it (tiles_m > tiles_n: e.g. the extra row b^T of [G ; b^T] opening a tile row of its own)
        const int tri = min(g.tiles_m, g.tiles_n), t0 = tri * (tri + 1) / 2;
        if (t < t0) {
            tm = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
            while ((tm + 1) * (tm + 2) / 2 <= t) ++tm;
            while (tm * (tm + 1) / 2 > t) --tm;
            tn = t - tm * (tm + 1) / 2;
        } else {
            tm = tri + (t - t0) / g.tiles_n;
            tn = (t - t0) % g.tiles_n;
        }
    } else {                                              // G32_BAND-wide bands of tile columns, row by row inside a band
        const int band = t / (G32_BAND * g.tiles_m), q = t - band * G32_BAND * g.tiles_m;
        const int wcols = min(G32_BAND, g.tiles_n - band * G32_BAND);
        tm = q / wcols;
        tn = band * G32_BAND + q - tm * wcols;
    }
    m0 = tm * TM_; n0 = tn * TN_;
    kbeg = slice * g.kslice; kend = min(g.K, kbeg + g.kslice);
    return true;
}

// C/D layout of the 32 x 32 MFMA: col = lane & 31, row = (c & 3) + 8 (c >> 2) + 4 (lane >> 5)
template <int NI, int NJ>
__device__ __forceinline__ void store_tile(const G32& g, const acc16 (&acc)[NI][NJ], int m0, int n0, int wr, int wc, int h, int r,
                                           float* Cb, int64_t ldcb, bool atomic_) {
    const bool atomic = atomic_, out_lower = g.flags & DSVGP_GEMM_OUT_LOWER;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int m = m0 + wr * (32 * NI) + i * 32 + (c & 3) + 8 * (c >> 2) + 4 * h;
                const int n = n0 + wc * (32 * NJ) + j * 32 + r;
                if (m >= g.M || n >= g.N) continue;
                if (out_lower && n > m) continue;                // (the caller zero-fills m < n)
                const float v = g.alpha * acc[i][j][c];
                float* dst = Cb + (int64_t)m * ldcb + n;
                if (atomic) atomicAdd(dst, v);
                else *dst = v;
            }
}
// where this workgroup's tile goes: the output itself (atomics when K is split) or, in deterministic mode, its K slice's slab
#define G32_DEST()                                                                                     \
    const int slice_ = g.kslice > 0 ? kbeg / g.kslice : 0;                                             \
    float* const Cb = g.slab ? g.slab + (int64_t)slice_ * g.M * g.N : g.C;                            \
    const int64_t ldcb = g.slab ? (int64_t)g.N : g.ldc;                                                \
    const bool atomic_ = g.splitk > 1 && !g.slab

template <int BK, bool A_KC, bool B_KC>
__global__ __launch_bounds__(256, G32_MINW) void gemm32_kernel(const G32 g) {
    constexpr int SKC = BK + 2, SMC = TM + 4;            // LDS row strides (floats) of the two images
    constexpr int A_WORDS = A_KC ? TM * SKC : BK * SMC, B_WORDS = B_KC ? TN * SKC : BK * SMC;
    __shared__ __attribute__((aligned(16))) float lds[A_WORDS + B_WORDS];
    float* As = lds;
    float* Bs = lds + A_WORDS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int h = lane >> 5, r = lane & 31;
    int m0, n0, kbeg, kend;
    if (!pick_unit(g, m0, n0, kbeg, kend)) return;

    Stage<BK, A_KC> ra;
    Stage<BK, B_KC> rb;
    typename std::conditional<A_KC, FetchKC<BK>, FetchMC<BK>>::type fa;
    typename std::conditional<B_KC, FetchKC<BK>, FetchMC<BK>>::type fb;
    fa.init(g.A, g.lda, m0, g.M, g.K, tid);
    fb.init(g.B, g.ldb, n0, g.N, g.K, tid);
    auto fetch = [&](int k0) {
        fa.load(k0, kend, ra);
        fb.load(k0, kend, rb);
    };
    auto commit = [&]() {
        if constexpr (A_KC) {
            constexpr int CPR = BK / 4, RPP = 256 / CPR;
            float* p = As + (tid / CPR) * SKC + (tid % CPR) * 4;
#pragma unroll
            for (int i = 0; i < BK / 8; ++i) {
                *reinterpret_cast<float2*>(p + i * RPP * SKC) = float2{ra.v[i].x, ra.v[i].y};
                *reinterpret_cast<float2*>(p + i * RPP * SKC + 2) = float2{ra.v[i].z, ra.v[i].w};
            }
        } else {
            float* p = As + (tid >> 5) * SMC + (tid & 31) * 4;
#pragma unroll
            for (int i = 0; i < BK / 8; ++i) *reinterpret_cast<float4*>(p + 8 * i * SMC) = ra.v[i];
        }
        if constexpr (B_KC) {
            constexpr int CPR = BK / 4, RPP = 256 / CPR;
            float* p = Bs + (tid / CPR) * SKC + (tid % CPR) * 4;
#pragma unroll
            for (int i = 0; i < BK / 8; ++i) {
                *reinterpret_cast<float2*>(p + i * RPP * SKC) = float2{rb.v[i].x, rb.v[i].y};
                *reinterpret_cast<float2*>(p + i * RPP * SKC + 2) = float2{rb.v[i].z, rb.v[i].w};
            }
        } else {
            float* p = Bs + (tid >> 5) * SMC + (tid & 31) * 4;
#pragma unroll
            for (int i = 0; i < BK / 8; ++i) *reinterpret_cast<float4*>(p + 8 * i * SMC) = rb.v[i];
        }
    };

    acc16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[i][j][c] = 0.f;

    // per-lane fragment bases inside the LDS images
    const float* af = A_KC ? As + (wr * 64 + r) * SKC + 2 * h : As + (2 * h) * SMC + wr * 64 + r;
    const float* bf = B_KC ? Bs + (wc * 64 + r) * SKC + 2 * h : Bs + (2 * h) * SMC + wc * 64 + r;

    if (kbeg < kend) {
        fetch(kbeg);
        for (int k0 = kbeg; k0 < kend; k0 += BK) {
            commit();
            __syncthreads();
            if (k0 + BK < kend) fetch(k0 + BK);                 // in flight under the MFMAs of this stage
#pragma unroll
            for (int kk = 0; kk < BK / 4; ++kk) {
                float2 a[2], b[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if constexpr (A_KC) a[i] = *reinterpret_cast<const float2*>(af + i * 32 * SKC + 4 * kk);
                    else a[i] = float2{af[(4 * kk) * SMC + i * 32], af[(4 * kk + 1) * SMC + i * 32]};
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if constexpr (B_KC) b[j] = *reinterpret_cast<const float2*>(bf + j * 32 * SKC + 4 * kk);
                    else b[j] = float2{bf[(4 * kk) * SMC + j * 32], bf[(4 * kk + 1) * SMC + j * 32]};
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
                    }
            }
            __syncthreads();
        }
    }

    G32_DEST();
    store_tile(g, acc, m0, n0, wr, wc, h, r, Cb, ldcb, atomic_);
}

// -------------------------------------------------------------------------------------------------
// The same product with the stages brought in by LDS-DMA (global_load_lds_dwordx4: global -> LDS without a register
// round trip and without ds_write traffic; ablations of the register-staged kernel above: the global loads cost 12 % and
// the LDS stores 10 % of its time).  BK = 32, TWO 32 KB LDS buffers (64 KB per workgroup, two workgroups per CU): the DMA of
// stage s + 1 is issued before the 64 MFMAs of stage s and waited for (vmcnt(0) + barrier) after them.
// An LDS-DMA instruction writes 64 x 16 bytes CONTIGUOUSLY (wave-uniform base + 16 lane), so the images cannot be padded:
//   mn-contiguous operand: [32 k][128] floats, linear -- fragment reads (consecutive lanes, consecutive words) need no pad;
//   k-contiguous operand:  [128 rows][32 k] floats with the 16-byte chunks of row R stored at position c ^ ((R >> 1) & 7)
//                          (the swizzle is applied to the SOURCE address of each lane); lane (h, r) reads chunk 2 j + h of its
//                          row with ONE 16-byte read per 4 MFMAs: the 16 lanes of a read group hit 16 distinct 4-bank slots.
// k order inside a stage: MFMA e of chunk pair j takes k = 8 j + 4 h + e from both operands.
// K tail: lanes whose chunk / row lies past K read a 16-byte zero block instead; a k-contiguous operand whose K is not a
// multiple of 4 must be zero-padded up to it by the caller (DSVGP_GEMM_K_PADDED) -- otherwise the register-staged kernel runs.
// -------------------------------------------------------------------------------------------------
#ifdef G32_STAMP   // diagnostic build only (tools/gemm32_probe.cpp prints the shares): where a stage of a mid-grid wave goes
__device__ unsigned long long g32_stamps[8];
#define G32_T(var) unsigned long long var; do { __builtin_amdgcn_sched_barrier(0); \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var) :: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define G32_T(var) do { } while (0)
#endif
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;
__device__ __attribute__((aligned(16))) float g32_zero_chunk[4] = {0.f, 0.f, 0.f, 0.f};

// One LDS-DMA instruction, hidden from the compiler's s_waitcnt bookkeeping: issued through the builtin, hipcc treats the
// transfer as an LDS store that any later ds_read may alias and parks a vmcnt(0) in front of the first fragment read of
// the stage -- the DMA then overlaps nothing.  As an asm statement it is register-safe (no VGPR destination) and WE count
// it: one "s_waitcnt vmcnt(0)" before the barrier that ends the stage.  M0 (the LDS destination base) is compiler-reserved:
// saved, set and restored inside the statement.
__device__ __forceinline__ void lds_dma16(const float* gsrc, unsigned lds_byte_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_byte_addr) : "memory");
}

// Round 4, measured and taken out again (profiles/r04_b_gemm32_patterns.txt): dealing only the USEFUL 32 x 32 MFMA tiles of a
// diagonal tile of a lower output (10 of 16, as 3 / 3 / 2 / 2 per wave) and of a ragged last tile row (M' = 3000: 56 valid rows -> 2
// MFMA tiles per wave) through per-wave copies of the K loop.  Ragged rows: Gram 2.077 -> 2.083 ms, dense 3.53 -> 3.55 (nothing:
// the two workgroups of a CU alternate MFMA and DMA-issue phases in lockstep, a shorter MFMA phase of one does not shorten the
// period of the pair); diagonal tiles: Gram 2.077 -> 2.124 ms at C4 and 0.633 -> 0.774 ms at C3 (slower); the mere presence of
// the extra loop copies costs 1-2 % (2.077 -> 2.114 with the patterns switched off at run time).
// This does not carry over to gemm32_gram_kernel below, which runs ONE workgroup per CU and one wave per SIMD: there a stage takes as long as
// its MFMAs, the same dealing pays (C4 Gram alone 1.82 -> 1.66 ms) and the extra loop copies cost nothing (profiles/gram_live_ab.txt).
// MF = 32: 2 x 2 tiles of v_mfma_f32_32x32x2_f32 per wave;  MF = 16: 4 x 4 tiles of v_mfma_f32_16x16x4_f32 (same 64 x 64 wave tile,
// same LDS images and DMA; twice the fragment reads per flop, but the smaller shape holds a higher clock under load).
// Lane l = TS h + r (TS = 32 / 16 rows per tile, h = k slot 0..1 / 0..3) reads chunk (64 / MF) j + h of its row per read.
// BK (G32_DMA_BK): 32 -- two 32 KB buffers, two workgroups per CU; 16 -- two 16 KB buffers, LDS and registers (<= 129) leave room for
// three: a third wave per SIMD fills the matrix pipe while the other two sit in their DMA-issue / barrier phases (round 5).  A
// k-contiguous image then has 64-byte rows of four 16-byte chunks, chunk c of row R at position c ^ ((R >> 2) & 3) (the four rows
// of a read group that share R mod 4 -- the same quarter of the 256-byte bank row -- differ in (R >> 2) & 3), 16 rows per 1 KB piece.
template <int MF, bool A_KC, bool B_KC, int BK>
__global__ __launch_bounds__(256, BK == 16 ? 3 : 2) void gemm32_dma_kernel(const G32 g) {
    static_assert(BK == 32 || (BK == 16 && MF == 32), "the 64-byte-row swizzle is derived for the 32 x 32 x 2 shape");
    constexpr int OPW = 128 * BK;                         // words per operand image
    constexpr int NP = BK / 8;                            // 1 KB DMA pieces per operand, stage and wave
    constexpr int CH = BK / 4, RPP = 256 / BK;            // 16-byte chunks per k-contiguous row; rows per piece
    constexpr int TS = MF, NT = 64 / TS, NH = 64 / TS, NJ = BK / (4 * NH);   // tile size, tiles per wave side, k slots, chunk groups / stage
    __shared__ __attribute__((aligned(16))) float lds[2][2 * OPW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int h = lane / TS, r = lane % TS;
    int m0, n0, kbeg, kend;
    if (!pick_unit(g, m0, n0, kbeg, kend)) return;

    // ---- DMA sources: NP instructions per operand and stage, instruction i of wave w fills the 1 KB block NP w + i
    const float* asrc[NP];
    const float* bsrc[NP];
    int akk[NP], bkk[NP];                                 // k of the lane's chunk / row inside a stage (for the K tail)
    const int K4 = (g.K + 3) / 4 * 4;
    auto swz = [](int R) { return BK == 32 ? ((R >> 1) & 7) : ((R >> 2) & 3); };
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int blk = wave * NP + i;
        if constexpr (A_KC) {
            const int R = blk * RPP + lane / CH, c = (lane % CH) ^ swz(R);
            asrc[i] = g.A + (int64_t)min(m0 + R, g.M - 1) * g.lda + kbeg + 4 * c;
            akk[i] = 4 * c;
        } else {
            const int k = blk * 2 + (lane >> 5);
            asrc[i] = g.A + (int64_t)(kbeg + k) * g.lda + min(m0 + 4 * (lane & 31), (g.M + 3) / 4 * 4 - 4);
            akk[i] = k;
        }
        if constexpr (B_KC) {
            const int R = blk * RPP + lane / CH, c = (lane % CH) ^ swz(R);
            bsrc[i] = g.B + (int64_t)min(n0 + R, g.N - 1) * g.ldb + kbeg + 4 * c;
            bkk[i] = 4 * c;
        } else {
            const int k = blk * 2 + (lane >> 5);
            bsrc[i] = g.B + (int64_t)(kbeg + k) * g.ldb + min(n0 + 4 * (lane & 31), (g.N + 3) / 4 * 4 - 4);
            bkk[i] = k;
        }
    }
    const int64_t astep = A_KC ? BK : (int64_t)BK * g.lda, bstep = B_KC ? BK : (int64_t)BK * g.ldb;
    const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)&lds[0][0];
    const unsigned wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto dma = [&](int buf, int k0) {
        const unsigned dst = lds_base + (unsigned)buf * (2 * OPW * 4) + wave_u * (NP * 1024);     // byte address, wave-uniform
        const bool tail = k0 + BK > kend;                 // (only the last stage of the last K slice)
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const float* sa = asrc[i];
            const float* sb = bsrc[i];
            if (tail) {
                if (k0 + akk[i] >= (A_KC ? K4 : g.K)) sa = g32_zero_chunk;
                if (k0 + bkk[i] >= (B_KC ? K4 : g.K)) sb = g32_zero_chunk;
            }
            lds_dma16(sa, dst + i * 1024);
            lds_dma16(sb, dst + OPW * 4 + i * 1024);
            asrc[i] += astep;
            bsrc[i] += bstep;
        }
    };

    using accT = typename std::conditional<MF == 32, acc16, acc4f>::type;
    accT acc[NT][NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int c = 0; c < (MF == 32 ? 16 : 4); ++c) acc[i][j][c] = 0.f;

    // per-lane fragment offsets (words) inside an operand image; tile i of the wave adds i * TS rows / columns
    const int q7 = h ^ swz(r);
    int aoff[NJ], boff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        aoff[j] = A_KC ? (wr * 64 + r) * BK + 4 * ((NH * j) ^ q7) : (4 * NH * j + 4 * h) * 128 + wr * 64 + r;
        boff[j] = B_KC ? (wc * 64 + r) * BK + 4 * ((NH * j) ^ q7) : (4 * NH * j + 4 * h) * 128 + wc * 64 + r;
    }

    // fragments of one chunk group j (4 NH k): 4 k-values per lane for each of the NT + NT MFMA tiles
    struct Frag { float a[NT][4], b[NT][4]; };
    auto load_frag = [&](const float* As, const float* Bs, int j, Frag& f) {
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            if constexpr (A_KC) {
                const float4 v = *reinterpret_cast<const float4*>(As + aoff[j] + i * TS * BK);
                f.a[i][0] = v.x; f.a[i][1] = v.y; f.a[i][2] = v.z; f.a[i][3] = v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) f.a[i][e] = As[aoff[j] + e * 128 + i * TS];
            }
            if constexpr (B_KC) {
                const float4 v = *reinterpret_cast<const float4*>(Bs + boff[j] + i * TS * BK);
                f.b[i][0] = v.x; f.b[i][1] = v.y; f.b[i][2] = v.z; f.b[i][3] = v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) f.b[i][e] = Bs[boff[j] + e * 128 + i * TS];
            }
        }
    };

    if (kbeg < kend) {
        dma(0, kbeg);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                   // stage 0 has landed for every wave
        int buf = 0;
#ifdef G32_STAMP
        unsigned long long d_dma = 0, d_mfma = 0, d_vm = 0, d_bar = 0, n_st = 0;
#endif
        for (int k0 = kbeg; k0 < kend; k0 += BK, buf ^= 1) {
            G32_T(t0);
            if (k0 + BK < kend) dma(buf ^ 1, k0 + BK);     // lands under the MFMAs below
            G32_T(t1);
            const float* As = &lds[buf][0];
            const float* Bs = As + OPW;
            // the fragments of chunk group j + 1 are requested before the MFMAs of group j: the LDS latency rides under them
            Frag f[2];
            load_frag(As, Bs, 0, f[0]);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (j + 1 < NJ) load_frag(As, Bs, j + 1, f[(j + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);         // (hipcc otherwise sinks the reads to just before their use)
                const Frag& c = f[j & 1];
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < NT; ++i)
#pragma unroll
                        for (int jn = 0; jn < NT; ++jn) {
                            if constexpr (MF == 32)
                                acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(c.a[i][e], c.b[jn][e], acc[i][jn], 0, 0, 0);
                            else
                                acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.a[i][e], c.b[jn][e], acc[i][jn], 0, 0, 0);
                        }
                __builtin_amdgcn_sched_barrier(0);
            }
            G32_T(t2);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA of the next stage has landed ...
            G32_T(t3);
            __syncthreads();                                   // ... and every wave's; this buffer is free for stage + 2
#ifdef G32_STAMP
            G32_T(t4);
            d_dma += t1 - t0; d_mfma += t2 - t1; d_vm += t3 - t2; d_bar += t4 - t3; ++n_st;
#endif
        }
#ifdef G32_STAMP
        if (tid == 0 && blockIdx.x == gridDim.x / 2 + 8) {
            g32_stamps[0] = d_dma; g32_stamps[1] = d_mfma; g32_stamps[2] = d_vm; g32_stamps[3] = d_bar; g32_stamps[4] = n_st;
        }
#endif
    }
    G32_DEST();
    if constexpr (MF == 32) {
        store_tile(g, acc, m0, n0, wr, wc, h, r, Cb, ldcb, atomic_);
    } else {
        // C/D layout of the 16 x 16 form: col = lane & 15, row = 4 (lane >> 4) + reg
        const bool atomic = atomic_, out_lower = g.flags & DSVGP_GEMM_OUT_LOWER;
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int m = m0 + wr * 64 + i * 16 + 4 * h + c;
                    const int n = n0 + wc * 64 + j * 16 + r;
                    if (m >= g.M || n >= g.N) continue;
                    if (out_lower && n > m) continue;
                    const float v = g.alpha * acc[i][j][c];
                    float* dst = Cb + (int64_t)m * ldcb + n;
                    if (atomic) atomicAdd(dst, v);
                    else *dst = v;
                }
    }
}

// -------------------------------------------------------------------------------------------------
// Large plain dense products (K_ZX-bar at C4: 12 x 128 tiles = six rounds of the 256 CUs): 256 x 192 output tiles, ONE workgroup
// per CU, one wave per SIMD.  Waves 2 x 2, each 128 x 96 = 4 x 3 tiles of v_mfma_f32_32x32x2_f32 (192 accumulator registers): 7
// fragment registers feed 12 MFMAs (the 64 x 64 wave tile above: 4 feed 4) and a stage brings in 448 bytes per output row + column
// pair of 256 + 192 where two 128 x 128 tiles bring in 512.  Left operand k-contiguous, right operand n-contiguous, no split-K.
// Stages: the same two LDS images as gemm32_dma_kernel<32, true, false, 32> -- [256 rows][32 k] with chunk c of row R at position
// c ^ ((R >> 1) & 7) and [32 k][192] linear -- 56 KB per stage, two buffers (dynamic LDS, 112 KB).  Per stage a wave issues 14 DMA
// instructions (8 + 6 pieces of 1 KB; a piece of the right image is 64 consecutive 16-byte chunks = 1 1/3 rows of 48).
// With one wave per SIMD nothing hides a stall, so the wave's instruction stream is laid out by hand (sched_barrier(0) fences: an
// asm statement belongs to no sched_group_barrier class): after every second MFMA ONE other item -- a DMA instruction of the
// next stage (5 / 5 / 4 in k-groups 0 / 1 / 2: they have the rest of the stage to land) or a fragment read of k-group j + 1 (4
// 16-byte reads of the left image, 6 pairs of 4-byte reads of the right) -- so that the matrix pipe always has its next MFMA
// before the current one (16 passes) retires.  One vmcnt(0) and one barrier per stage; no branch inside a stage: the stage that
// issues the DMA crossing K (zero chunk selects) and the last one (no DMA) are copies of their own.
// Arithmetic: each output element meets k in the same order as in gemm32_dma_kernel<32, true, false, 32> (stage by stage, MFMA e of
// chunk pair j takes k = 8 j + 4 h + e) -- the two kernels return the same bits.
// -------------------------------------------------------------------------------------------------
constexpr int WTM = 256, WTN = 192, WBK = 32;
constexpr int W_AWORDS = WTM * WBK, W_BWORDS = WBK * WTN, W_STAGE = W_AWORDS + W_BWORDS;      // 8192 + 6144 words = 56 KB
constexpr int W_NA = W_AWORDS / 1024, W_NB = W_BWORDS / 1024;                                  // 1 KB pieces per wave and stage: 8 + 6
constexpr int W_LDS_BYTES = 2 * W_STAGE * 4;

__global__ __launch_bounds__(256, 1) void gemm32_wide_kernel(const G32 g) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];        // [2][W_STAGE]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int h = lane >> 5, r = lane & 31;
    int m0, n0, kbeg, kend;
    if (!pick_unit<WTM, WTN>(g, m0, n0, kbeg, kend)) return;

    // ---- DMA sources: piece i of wave w is the 1 KB block W_NA w + i (left image) / W_NB w + i (right image)
    const float* asrc[W_NA];
    const float* bsrc[W_NB];
    int akk[W_NA], bkk[W_NB];                             // k of the lane's chunk / row inside a stage (for the K tail)
    const int K4 = (g.K + 3) / 4 * 4;
#pragma unroll
    for (int i = 0; i < W_NA; ++i) {
        const int R = (wave * W_NA + i) * 8 + (lane >> 3), c = (lane & 7) ^ ((R >> 1) & 7);
        asrc[i] = g.A + (int64_t)min(m0 + R, g.M - 1) * g.lda + kbeg + 4 * c;
        akk[i] = 4 * c;
    }
#pragma unroll
    for (int i = 0; i < W_NB; ++i) {
        const int ch = (wave * W_NB + i) * 64 + lane, k = ch / (WTN / 4), n4 = ch % (WTN / 4);
        bsrc[i] = g.B + (int64_t)(kbeg + k) * g.ldb + min(n0 + 4 * n4, (g.N + 3) / 4 * 4 - 4);
        bkk[i] = k;
    }
    const int64_t bstep = (int64_t)WBK * g.ldb;
    const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)&wlds[0];
    const unsigned wave_u = __builtin_amdgcn_readfirstlane(wave);

    acc16 acc[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[i][j][c] = 0.f;

    // per-lane fragment offsets (words) inside the images; MFMA tile i adds 32 rows / columns, element e of the right image one row
    const int q7 = h ^ ((r >> 1) & 7);
    int aoff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) aoff[j] = (wr * 128 + r) * WBK + 4 * ((2 * j) ^ q7);
    const int boff = (4 * h) * WTN + wc * 96 + r;

    // one stage: the MFMAs on buffer buf with, between them, the DMA of the stage at knext into the other buffer.
    // MODE 0: no DMA (the last stage); 1: a whole stage; 2: the stage that may cross K (chunks / rows past it come from the zero chunk)
    auto stage = [&](auto mode_, int buf, int knext) {
        constexpr int MODE = decltype(mode_)::value;
        const float* As = wlds + buf * W_STAGE;
        const float* Bs = As + W_AWORDS;
        const unsigned dst = lds_base + (unsigned)(buf ^ 1) * (W_STAGE * 4);      // byte address, wave-uniform
        float fa[2][4][4], fb[2][3][4];                   // fragments of k-groups j (even / odd): plain arrays
        auto rd_a = [&](int j, int i) {
            const float4 v = *reinterpret_cast<const float4*>(As + aoff[j] + i * 32 * WBK);
            fa[j & 1][i][0] = v.x; fa[j & 1][i][1] = v.y; fa[j & 1][i][2] = v.z; fa[j & 1][i][3] = v.w;
        };
        auto rd_b = [&](int j, int jn, int ep) {          // elements 2 ep, 2 ep + 1 of tile jn
#pragma unroll
            for (int e = 2 * ep; e < 2 * ep + 2; ++e) fb[j & 1][jn][e] = Bs[boff + (8 * j + e) * WTN + jn * 32];
        };
        auto dma1 = [&](int d) {                          // DMA instruction d of the stage: 0..7 left image, 8..13 right image
            if (d < W_NA) {
                const float* s = asrc[d];
                if (MODE == 2) s = (knext + akk[d] >= K4) ? g32_zero_chunk : s;
                lds_dma16(s, dst + (wave_u * W_NA + d) * 1024);
                asrc[d] += WBK;
            } else {
                const int i = d - W_NA;
                const float* s = bsrc[i];
                if (MODE == 2) s = (knext + bkk[i] >= g.K) ? g32_zero_chunk : s;
                lds_dma16(s, dst + W_AWORDS * 4 + (wave_u * W_NB + i) * 1024);
                bsrc[i] += bstep;
            }
        };
#pragma unroll
        for (int i = 0; i < 4; ++i) rd_a(0, i);
#pragma unroll
        for (int q = 0; q < 6; ++q) rd_b(0, q >> 1, q & 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nd = MODE == 0 ? 0 : (j < 2 ? 5 : (j == 2 ? 4 : 0)), d0 = j < 2 ? 5 * j : 10;
#pragma unroll
            for (int n = 0; n < 48; ++n) {
                const int e = n / 12, i = (n / 3) % 4, jn = n % 3;
                acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[j & 1][i][e], fb[j & 1][jn][e], acc[i][jn], 0, 0, 0);
                if (n & 1) {
                    const int t = n >> 1;
                    __builtin_amdgcn_sched_barrier(0);
                    if (t < nd) {
                        dma1(d0 + t);
                    } else if (j < 3) {
                        const int q = t - nd;
                        if (q < 4) rd_a(j + 1, q);
                        else if (q < 10) rd_b(j + 1, (q - 4) >> 1, (q - 4) & 1);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (MODE != 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA of the next stage has landed ...
            __syncthreads();                                   // ... and every wave's; this buffer is free for stage + 2
        }
    };

    if (kbeg < kend) {
        const int nst = (kend - kbeg + WBK - 1) / WBK;
        {   // stage 0 (tail-checked: it is also the last one when K <= 32)
            const unsigned dst = lds_base;
#pragma unroll
            for (int i = 0; i < W_NA; ++i) {
                lds_dma16((kbeg + akk[i] >= K4) ? g32_zero_chunk : asrc[i], dst + (wave_u * W_NA + i) * 1024);
                asrc[i] += WBK;
            }
#pragma unroll
            for (int i = 0; i < W_NB; ++i) {
                lds_dma16((kbeg + bkk[i] >= g.K) ? g32_zero_chunk : bsrc[i], dst + W_AWORDS * 4 + (wave_u * W_NB + i) * 1024);
                bsrc[i] += bstep;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                   // stage 0 has landed for every wave
        int buf = 0, k0 = kbeg + WBK;                      // k0: the stage whose DMA the next call issues
        for (int s = 0; s + 2 < nst; ++s, buf ^= 1, k0 += WBK) stage(std::integral_constant<int, 1>{}, buf, k0);
        if (nst >= 2) { stage(std::integral_constant<int, 2>{}, buf, k0); buf ^= 1; }
        stage(std::integral_constant<int, 0>{}, buf, 0);
    }
    store_tile(g, acc, m0, n0, wr, wc, h, r, g.C, g.ldc, false);
}

// -------------------------------------------------------------------------------------------------
// Lower-triangular products of two k-contiguous operands with a long K (the Gram product [G ; b^T] = tril([A ; mu_bar^T] A^T) at C4:
// 3001 x 3000 x 24576): 256 x 256 output tiles, ONE workgroup per CU, one wave per SIMD, and a stream-K walk in place of split-K.
// Waves 2 x 2, each 128 x 128 = 4 x 4 tiles of v_mfma_f32_32x32x2_f32 (256 accumulator registers): 8 fragment registers feed 16 MFMAs.
// Stages: two images [256 rows][32 k] with chunk c of row R at position c ^ ((R >> 1) & 7) (the k-contiguous image of the kernels
// above), 64 KB per stage, two buffers (dynamic LDS, 128 KB).  Per stage a wave issues 16 DMA instructions (8 + 8 pieces of 1 KB) and,
// per k-group of 8 k, 8 fragment reads of 16 bytes for 64 MFMAs.  The stage is laid out like the one of gemm32_wide_kernel: after every
// second MFMA ONE other item -- a DMA instruction of the next stage (6 / 5 / 5 in k-groups 0 / 1 / 2) or a fragment read of k-group
// j + 1 --, one vmcnt(0) and one barrier per stage, no branch inside a stage; the stage whose DMA may cross K and the last stage of a
// unit are copies of their own.
// Work: the 256 x 256 tiles of the lower triangle (78 at M' = 3000: 13.4 % of their outputs are dead, against 9.2 % on 128 x 128
// tiles) cannot be cut evenly over the CUs by any uniform K split, so every workgroup walks an equal, contiguous share of the
// (tile, stage) sequence (gram_walk.h) and adds its accumulators into C -- atomics onto zeros, as the split-K launch does -- whenever
// its share leaves a tile and at its end.  A share may start and end mid-tile and, when K is short, span several tiles.
// Epilogue: 256 atomic instructions per wave, each 2 x 128 contiguous bytes; at most 32 of a wave are in flight (a counted vmcnt
// after every MFMA tile's 16), which is where the issue of float atomics stalls anyway.
// Patterns (gram_walk.h; DSVGP_G32_GRAM_LIVE=0 at a launch turns them off): the above is the stage of a FULL tile.  A diagonal tile has 36
// live MFMA tiles of 64 and a ragged last tile row fewer live MFMA rows than 8, and a wave that issues MFMAs for dead tiles sets the pace
// of the stage for nothing.  DIAG deals the 36 tiles 9 per wave, ROWS3 (5 or 6 live MFMA rows) 12 per wave; every live MFMA tile keeps ONE
// owner over a unit's whole stage range, so an output still receives one partial sum per unit.  A pattern's stage is the same layout with
// fewer MFMAs (144 / 192 for 256) and only the fragments its tiles need; DIAG's four lists differ, so each wave runs its own copy of the
// stage loop -- all waves still meet at one vmcnt(0) and one barrier per stage.  The walk deals equal COST (16 / 12 / 9 per stage), not
// equal stage counts.  C4: 1120 x 768 MFMA tiles per wave instead of 1248 x 768 (-10.3 %); no scratch (profiles/gram_live_resource_usage.txt).
// -------------------------------------------------------------------------------------------------
constexpr int GT = 256, GBK = 32;
constexpr int G_OPWORDS = GT * GBK, G_STAGE = 2 * G_OPWORDS;                                   // 2 x 8192 words = 64 KB
constexpr int G_NP = G_OPWORDS / 1024;                                                         // 1 KB pieces per operand, wave and stage: 8
constexpr int G_LDS_BYTES = 2 * G_STAGE * 4;

template <int PAT, int WV>
struct GramPat { static constexpr GramPatWave v = gram_pattern(PAT, WV); };     // the table of gram_walk.h, used in constant expressions only
template <class F, int... I>
__device__ __forceinline__ void g32_static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void g32_static_for(F&& f) { g32_static_for_impl(f, std::make_integer_sequence<int, N>{}); }

struct G32Gram {
    const float* A; const float* B; float* C;
    int64_t lda, ldb, ldc;
    int M, N, K, nwg;
    float alpha;
    GramWalk walk;
};

__global__ __launch_bounds__(256, 1) void gemm32_gram_kernel(const G32Gram g) {
    extern __shared__ __attribute__((aligned(16))) float glds[];        // [2][G_STAGE]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int h = lane >> 5, r = lane & 31;
    const int wg = gram_walk_wg(blockIdx.x, gridDim.x);
    if (wg >= g.nwg) return;
    long long gi, gend;
    gram_walk_range(g.walk, wg, g.nwg, gi, gend);

    const int K4 = (g.K + 3) / 4 * 4;
    const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)&glds[0];
    const unsigned wave_u = __builtin_amdgcn_readfirstlane(wave);
    // per-lane fragment offsets (words) inside an image; MFMA tile i adds 32 rows
    const int q7 = h ^ ((r >> 1) & 7);
    int aoff[4], boff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        aoff[j] = (wr * 128 + r) * GBK + 4 * ((2 * j) ^ q7);
        boff[j] = (wc * 128 + r) * GBK + 4 * ((2 * j) ^ q7);
    }
    const int frag0 = r * GBK;                             // (the patterns add their own MFMA rows: aoff[j] = frag0 + wr * 128 * GBK + 4 ((2 j) ^ q7))
    // DMA: piece i of wave w is the 1 KB block 8 w + i of either image -- rows 8 (8 w + i) .. + 7, lane -> (row, swizzled chunk)
    int drow[G_NP], dkk[G_NP];
#pragma unroll
    for (int i = 0; i < G_NP; ++i) {
        drow[i] = (wave * G_NP + i) * 8 + (lane >> 3);
        dkk[i] = 4 * ((lane & 7) ^ ((drow[i] >> 1) & 7));
    }

    while (gi < gend) {                                    // one unit: stages [s0, s1) of one tile into one accumulator set
        const GramUnit u = gram_walk_unit(g.walk, gi, gend);
        gi += u.s1 - u.s0;
        const int m0 = u.tm * GT, n0 = u.tn * GT, nst = u.s1 - u.s0, kbeg = u.s0 * GBK;
        const float* asrc[G_NP];
        const float* bsrc[G_NP];
#pragma unroll
        for (int i = 0; i < G_NP; ++i) {
            asrc[i] = g.A + (int64_t)min(m0 + drow[i], g.M - 1) * g.lda + kbeg + dkk[i];
            bsrc[i] = g.B + (int64_t)min(n0 + drow[i], g.N - 1) * g.ldb + kbeg + dkk[i];
        }
        acc16 acc[4][4];                                   // (zeroed below, where the unit's pattern is known: NT sets)
        auto zero_acc = [&](int nt) {
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (t < nt) {
#pragma unroll
                    for (int c = 0; c < 16; ++c) acc[t / 4][t % 4][c] = 0.f;
                }
        };

        // one stage: the MFMAs on buffer buf with, between them, the DMA of the stage at knext into the other buffer.
        // MODE 0: no DMA (the last stage of the unit); 1: a whole stage; 2: the stage that may cross K (chunks past it come from the zero chunk)
        auto stage = [&](auto mode_, int buf, int knext) {
            constexpr int MODE = decltype(mode_)::value;
            const float* As = glds + buf * G_STAGE;
            const float* Bs = As + G_OPWORDS;
            const unsigned dst = lds_base + (unsigned)(buf ^ 1) * (G_STAGE * 4);      // byte address, wave-uniform
            float fa[2][4][4], fb[2][4][4];                   // fragments of k-groups j (even / odd): plain arrays
            auto rd_a = [&](int j, int i) {
                const float4 v = *reinterpret_cast<const float4*>(As + aoff[j] + i * 32 * GBK);
                fa[j & 1][i][0] = v.x; fa[j & 1][i][1] = v.y; fa[j & 1][i][2] = v.z; fa[j & 1][i][3] = v.w;
            };
            auto rd_b = [&](int j, int i) {
                const float4 v = *reinterpret_cast<const float4*>(Bs + boff[j] + i * 32 * GBK);
                fb[j & 1][i][0] = v.x; fb[j & 1][i][1] = v.y; fb[j & 1][i][2] = v.z; fb[j & 1][i][3] = v.w;
            };
            auto dma1 = [&](int d) {                          // DMA instruction d of the stage: 0..7 left image, 8..15 right image
                if (d < G_NP) {
                    const float* s = asrc[d];
                    if (MODE == 2) s = (knext + dkk[d] >= K4) ? g32_zero_chunk : s;
                    lds_dma16(s, dst + (wave_u * G_NP + d) * 1024);
                    asrc[d] += GBK;
                } else {
                    const int i = d - G_NP;
                    const float* s = bsrc[i];
                    if (MODE == 2) s = (knext + dkk[i] >= K4) ? g32_zero_chunk : s;
                    lds_dma16(s, dst + G_OPWORDS * 4 + (wave_u * G_NP + i) * 1024);
                    bsrc[i] += GBK;
                }
            };
#pragma unroll
            for (int i = 0; i < 4; ++i) rd_a(0, i);
#pragma unroll
            for (int i = 0; i < 4; ++i) rd_b(0, i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int nd = MODE == 0 ? 0 : (j == 0 ? 6 : (j < 3 ? 5 : 0)), d0 = j == 0 ? 0 : (j == 1 ? 6 : 11);
#pragma unroll
                for (int n = 0; n < 64; ++n) {
                    const int e = n / 16, i = (n / 4) % 4, jn = n % 4;
                    acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[j & 1][i][e], fb[j & 1][jn][e], acc[i][jn], 0, 0, 0);
                    if (n & 1) {
                        const int t = n >> 1;
                        __builtin_amdgcn_sched_barrier(0);
                        if (t < nd) {
                            dma1(d0 + t);
                        } else if (j < 3) {
                            const int q = t - nd;
                            if (q < 4) rd_a(j + 1, q);
                            else if (q < 8) rd_b(j + 1, q - 4);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            if (MODE != 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA of the next stage has landed ...
                __syncthreads();                                   // ... and every wave's; this buffer is free for stage + 2
            }
        };

        // the same stage for a pattern of gram_walk.h: wave WV's NT tiles (accumulator set t = tile t of its list), fragments of its
        // NR MFMA rows and NC MFMA columns only, the same 16 DMA instructions in the same k-groups, one other item after every second
        // MFMA.  rbase / cbase: words of the wave's first MFMA row / column (row0, col0 of the table) inside an image
        auto live_body = [&](auto pat_, auto wv_, auto mode_, int buf, int knext, int rbase, int cbase) {
            constexpr int MODE = decltype(mode_)::value;
            using P = GramPat<decltype(pat_)::value, decltype(wv_)::value>;
            constexpr int NR = P::v.nr, NC = P::v.nc, NT = P::v.nt;
            static_assert(6 + NR + NC <= 2 * NT, "a k-group's slots hold its DMA instructions and the next k-group's fragment reads");
            const float* As = glds + buf * G_STAGE + rbase + frag0;
            const float* Bs = glds + buf * G_STAGE + G_OPWORDS + cbase + frag0;
            const unsigned dst = lds_base + (unsigned)(buf ^ 1) * (G_STAGE * 4);
            float fa[2][NR][4], fb[2][NC][4];
            auto rd = [&](auto j_, auto q_) {                 // fragment read q of k-group j: rows first, then columns
                constexpr int j = decltype(j_)::value, q = decltype(q_)::value;
                if constexpr (q < NR) {
                    constexpr int ro = P::v.rows[q] * 32 * GBK;
                    const float4 v = *reinterpret_cast<const float4*>(As + ro + 4 * ((2 * j) ^ q7));
                    fa[j & 1][q][0] = v.x; fa[j & 1][q][1] = v.y; fa[j & 1][q][2] = v.z; fa[j & 1][q][3] = v.w;
                } else if constexpr (q < NR + NC) {
                    constexpr int co = P::v.cols[q - NR] * 32 * GBK;
                    const float4 v = *reinterpret_cast<const float4*>(Bs + co + 4 * ((2 * j) ^ q7));
                    fb[j & 1][q - NR][0] = v.x; fb[j & 1][q - NR][1] = v.y; fb[j & 1][q - NR][2] = v.z; fb[j & 1][q - NR][3] = v.w;
                }
            };
            auto dma1 = [&](int d) {                          // as in the stage above
                if (d < G_NP) {
                    const float* s = asrc[d];
                    if (MODE == 2) s = (knext + dkk[d] >= K4) ? g32_zero_chunk : s;
                    lds_dma16(s, dst + (wave_u * G_NP + d) * 1024);
                    asrc[d] += GBK;
                } else {
                    const int i = d - G_NP;
                    const float* s = bsrc[i];
                    if (MODE == 2) s = (knext + dkk[i] >= K4) ? g32_zero_chunk : s;
                    lds_dma16(s, dst + G_OPWORDS * 4 + (wave_u * G_NP + i) * 1024);
                    bsrc[i] += GBK;
                }
            };
            g32_static_for<NR + NC>([&](auto q_) { rd(std::integral_constant<int, 0>{}, q_); });
            g32_static_for<4>([&](auto j_) {
                constexpr int j = decltype(j_)::value;
                constexpr int nd = MODE == 0 ? 0 : (j == 0 ? 6 : (j < 3 ? 5 : 0)), d0 = j == 0 ? 0 : (j == 1 ? 6 : 11);
                g32_static_for<4 * NT>([&](auto n_) {
                    constexpr int n = decltype(n_)::value, e = n / NT, t = n % NT, ia = P::v.tr[t], ib = P::v.tc[t];
                    acc[t / 4][t % 4] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[j & 1][ia][e], fb[j & 1][ib][e], acc[t / 4][t % 4], 0, 0, 0);
                    if constexpr (n & 1) {
                        constexpr int sl = n >> 1;
                        __builtin_amdgcn_sched_barrier(0);
                        if constexpr (sl < nd) dma1(d0 + sl);
                        else if constexpr (j < 3) rd(std::integral_constant<int, j + 1>{}, std::integral_constant<int, sl - nd>{});
                        __builtin_amdgcn_sched_barrier(0);
                    }
                });
            });
        };
        // a pattern's partial sums into C: the wave's own tiles, the predicates and the in-flight count of the FULL epilogue below
        auto live_store = [&](auto pat_, auto wv_, int mrow0, int ncol0) {
            using P = GramPat<decltype(pat_)::value, decltype(wv_)::value>;
            g32_static_for<P::v.nt>([&](auto t_) {
                constexpr int t = decltype(t_)::value, ro = P::v.rows[P::v.tr[t]] * 32, co = P::v.cols[P::v.tc[t]] * 32;
                const int mt = m0 + mrow0 + ro, nt = n0 + ncol0 + co;
                if (mt >= g.M || nt >= g.N || nt > mt + 31) return;
                const int n = nt + r;
                float* dst = g.C + (int64_t)(mt + 4 * h) * g.ldc + n;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int mo = (c & 3) + 8 * (c >> 2), m = mt + 4 * h + mo;
                    if (m < g.M && n < g.N && n <= m) atomicAdd(dst + (int64_t)mo * g.ldc, g.alpha * acc[t / 4][t % 4][c]);
                }
                if (G32_GRAM_INFLIGHT < 63) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G32_GRAM_INFLIGHT) : "memory");
            });
        };

        __syncthreads();                                   // every wave has left the buffers of the previous unit
        {   // stage 0 of the unit (tail-checked: it may be the last stage of K)
#pragma unroll
            for (int i = 0; i < G_NP; ++i) {
                const bool z = kbeg + dkk[i] >= K4;
                lds_dma16(z ? g32_zero_chunk : asrc[i], lds_base + (wave_u * G_NP + i) * 1024);
                lds_dma16(z ? g32_zero_chunk : bsrc[i], lds_base + G_OPWORDS * 4 + (wave_u * G_NP + i) * 1024);
                asrc[i] += GBK;
                bsrc[i] += GBK;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                   // stage 0 has landed for every wave
        int buf = 0, k0 = kbeg + GBK;                      // k0: the stage whose DMA the next call issues
        // The pattern is wave-uniform per unit.  DIAG's four lists differ, so each wave runs the unit in its own copy of the stage loop
        // (a scalar branch per unit, none inside a stage); every copy has the same vmcnt(0) and barrier after every stage but the last
        auto run_unit = [&](auto pat_, auto wv_, int row0, int col0) {      // row0 / col0: the wave's first MFMA row / column
            zero_acc(GramPat<decltype(pat_)::value, decltype(wv_)::value>::v.nt);
            const int rbase = row0 * 32 * GBK, cbase = col0 * 32 * GBK;
            auto st = [&](auto mode_, int b, int kn) {
                live_body(pat_, wv_, mode_, b, kn, rbase, cbase);
                if (decltype(mode_)::value != 0) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                }
            };
            for (int s = 0; s + 2 < nst; ++s, buf ^= 1, k0 += GBK) st(std::integral_constant<int, 1>{}, buf, k0);
            if (nst >= 2) { st(std::integral_constant<int, 2>{}, buf, k0); buf ^= 1; }
            st(std::integral_constant<int, 0>{}, buf, 0);
            live_store(pat_, wv_, row0 * 32, col0 * 32);
        };
        const int pat = gram_walk_pattern(g.walk, u.tm, u.tn);
        if (pat != GRAM_PAT_FULL) {
            using std::integral_constant;
            if (pat == GRAM_PAT_ROWS3) {
                run_unit(integral_constant<int, GRAM_PAT_ROWS3>{}, integral_constant<int, 0>{}, gram_pat_row0(GRAM_PAT_ROWS3, wave_u), gram_pat_col0(GRAM_PAT_ROWS3, wave_u));
            } else {
                switch (wave_u) {
                    case 0: run_unit(integral_constant<int, GRAM_PAT_DIAG>{}, integral_constant<int, 0>{}, 0, 0); break;
                    case 1: run_unit(integral_constant<int, GRAM_PAT_DIAG>{}, integral_constant<int, 1>{}, 0, 0); break;
                    case 2: run_unit(integral_constant<int, GRAM_PAT_DIAG>{}, integral_constant<int, 2>{}, 0, 0); break;
                    default: run_unit(integral_constant<int, GRAM_PAT_DIAG>{}, integral_constant<int, 3>{}, 0, 0); break;
                }
            }
            continue;
        }
        zero_acc(16);
        for (int s = 0; s + 2 < nst; ++s, buf ^= 1, k0 += GBK) stage(std::integral_constant<int, 1>{}, buf, k0);
        if (nst >= 2) { stage(std::integral_constant<int, 2>{}, buf, k0); buf ^= 1; }
        stage(std::integral_constant<int, 0>{}, buf, 0);

        // the unit's partial sum into C.  C/D layout of the 32 x 32 MFMA: col = lane & 31, row = (c & 3) + 8 (c >> 2) + 4 (lane >> 5)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int mt = m0 + wr * 128 + i * 32, nt = n0 + wc * 128 + j * 32;
                if (mt >= g.M || nt >= g.N || nt > mt + 31) continue;          // (wave-uniform: an MFMA tile with no live element)
                const int n = nt + r;
                float* dst = g.C + (int64_t)(mt + 4 * h) * g.ldc + n;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int mo = (c & 3) + 8 * (c >> 2), m = mt + 4 * h + mo;
                    if (m < g.M && n < g.N && n <= m) atomicAdd(dst + (int64_t)mo * g.ldc, g.alpha * acc[i][j][c]);
                }
                if (G32_GRAM_INFLIGHT < 63) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G32_GRAM_INFLIGHT) : "memory");
            }
    }
}

template <int BK>
int dispatch32(hipStream_t st, const G32& a, dim3 grid, bool akc, bool bkc) {
    if (akc && bkc) hipLaunchKernelGGL((gemm32_kernel<BK, true, true>), grid, dim3(256), 0, st, a);
    else if (akc) hipLaunchKernelGGL((gemm32_kernel<BK, true, false>), grid, dim3(256), 0, st, a);
    else if (bkc) hipLaunchKernelGGL((gemm32_kernel<BK, false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((gemm32_kernel<BK, false, false>), grid, dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 1 : 1000 + (int)e;
}

}  // namespace

#ifdef G32_STAMP
int g32_read_stamps(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g32_stamps), sizeof(unsigned long long) * 8); }
#endif

// returns 1 if the product was taken, 0 if the caller must use gemm.hip, > 1 on a launch error.
// Taken: plain fp32 products (no triangular operands, no Cin, no kscale, no second output) with >= 128 x 128 x 512
// of work per tile; OUT_LOWER (square tile grids) zero-fills the strict upper triangle like gemm.hip does.
int launch_gemm32(hipStream_t st, const GemmArgs& g) {
    const int fl = g.flags;
    // DSVGP_G32_GRAM (the 256 x 256 stream-K kernel for lower k-contiguous products, gemm32_gram_kernel), read at every launch:
    // 0 = never; 1 = for every product it can take; 2 = as 1, and a lower-triangular product it cannot take -- by its layout or by any
    // gate of this function -- is an error (hipErrorInvalidValue: how a test knows which kernel ran); unset = the rule below.
    const char* genv = getenv("DSVGP_G32_GRAM");
    const int gmode = genv ? atoi(genv) : 3;
    const int not_taken = (gmode == 2 && (fl & DSVGP_GEMM_OUT_LOWER)) ? 1000 + (int)hipErrorInvalidValue : 0;
    if (fl & ~(DSVGP_GEMM_TRANS_A | DSVGP_GEMM_TRANS_B | DSVGP_GEMM_OUT_LOWER | DSVGP_GEMM_K_PADDED | DSVGP_GEMM_C_ZEROED | DSVGP_GEMM_UPPER_UNDEF)) return not_taken;
    if (g.batch != 1 || g.splitk != 1 || g.Cin || g.kscale || g.C32 || !g.C || g.beta != 0.0) return not_taken;
    if (g.M < 512 || g.N < 512 || g.K < 512) return not_taken;
    if (g.lda % 4 || g.ldb % 4 || ((uintptr_t)g.A % 16) || ((uintptr_t)g.B % 16)) return not_taken;     // 16-byte vector loads
    {   // the clamped vector loads of ragged edges stay inside the rows: ld covers the minor extent rounded up to 4
        const int64_t a_minor = (fl & DSVGP_GEMM_TRANS_A) ? g.M : g.K, b_minor = (fl & DSVGP_GEMM_TRANS_B) ? g.K : g.N;
        if (g.lda < (a_minor + 3) / 4 * 4 || g.ldb < (b_minor + 3) / 4 * 4) return not_taken;
        const int64_t a_rows = (fl & DSVGP_GEMM_TRANS_A) ? g.K : g.M, b_rows = (fl & DSVGP_GEMM_TRANS_B) ? g.N : g.K;
        if (a_rows * g.lda >= (int64_t)1 << 31 || b_rows * g.ldb >= (int64_t)1 << 31) return not_taken;     // 32-bit row offsets
    }
    const bool out_lower = fl & DSVGP_GEMM_OUT_LOWER;
    G32 a{};
    a.A = (const float*)g.A; a.B = (const float*)g.B; a.C = (float*)g.C;
    a.lda = g.lda; a.ldb = g.ldb; a.ldc = g.ldc;
    a.M = g.M; a.N = g.N; a.K = g.K; a.flags = fl; a.alpha = (float)g.alpha;
    a.tiles_m = cdiv(g.M, TM); a.tiles_n = cdiv(g.N, TN);
    if (out_lower) {
        const int tri = a.tiles_m < a.tiles_n ? a.tiles_m : a.tiles_n;
        a.ntiles = tri * (tri + 1) / 2 + (a.tiles_m > tri ? (a.tiles_m - tri) * a.tiles_n : 0);
    } else {
        a.ntiles = a.tiles_m * a.tiles_n;
    }
    // split-K: few rounds of tiles and a long K (the Gram product over the minibatch axis; the [B', M'] x [M', M'] products of
    // CIQ: 1152 tiles = 4.5 per CU).  Cost model: per-CU makespan, ceil(units / 256) x (slice length + fixed cost); measured
    // against fixed slice counts: C5's K_ZZ products 1 / 2 / 3 / 4 / 6 slices -> 80.9 / 77.1 / 78.7 / 77.7 / 78.7 ms per step
    // (the model picks 2), the Gram product of C4 5 slices as before
    int sk = 1;
    if (a.ntiles < G32_SK_BELOW && g.K >= G32_SK_MINK) {
        double best = 1e300;
        const int maxsk = g.K / 256 < 64 ? g.K / 256 : 64;
        for (int c = 1; c <= maxsk; ++c) {
            const double tcost = (double)cdiv((int64_t)a.ntiles * c, G32_SK_SLOTS) * ((double)g.K / c + 384.0);
            if (tcost < best * 0.999) { best = tcost; sk = c; }
        }
    }
    const bool akc = !(fl & DSVGP_GEMM_TRANS_A), bkc = (fl & DSVGP_GEMM_TRANS_B) != 0;
    // LDS-DMA kernels: a k-contiguous operand needs K % 4 == 0 or caller-zeroed padding up to it (the chunk that straddles K
    // is read as it lies in memory)
    const bool dma_ok = !((akc || bkc) && g.K % 4 != 0 && !(g.flags & DSVGP_GEMM_K_PADDED));
    // The 256 x 192 kernel (gemm32_wide_kernel) takes plain dense products with a k-contiguous left and an n-contiguous right operand,
    // unsplit and outside deterministic mode.  The rule: the cost model above leaves K whole and the 256 x 192 tiles fill at least
    // G32_WIDE_ROUNDS rounds of the CUs to G32_WIDE_FILL per cent (one workgroup per CU: a ragged last round idles whole CUs, and
    // every tile pays its first stage and its epilogue in the open -- C3's 390 tiles = 1.5 rounds, the data-parallel shares' 192 and
    // CIQ's split products stay on the 128 x 128 kernel).  DSVGP_G32_WIDE, read at every launch: 0 = never (the launch is the one of
    // the 128 x 128 kernel alone); 1 = for every product it can take, K whole; 2 = as 1, and a product it cannot take is an error
    // (hipErrorInvalidValue: how a test knows which kernel ran); -1 = the 128 x 128 kernel, K whole, for the products 1 would take (the bitwise
    // reference of 1: split-K meets in atomics, in no fixed order); unset = the rule.
    const char* wenv = getenv("DSVGP_G32_WIDE");
    const int wmode = wenv ? atoi(wenv) : 3;
    const bool wide_can = !out_lower && akc && !bkc && dma_ok && !g.slab;
    bool wide = false;
    if (wmode == 3) {
        const int64_t wt = (int64_t)cdiv(g.M, WTM) * cdiv(g.N, WTN), rounds = (wt + G32_SK_SLOTS - 1) / G32_SK_SLOTS;
        wide = wide_can && sk == 1 && wt >= (int64_t)G32_WIDE_ROUNDS * G32_SK_SLOTS && wt * 100 >= rounds * G32_SK_SLOTS * G32_WIDE_FILL;
    } else if (wmode != 0) {
        if (wmode == 2 && !wide_can) return 1000 + (int)hipErrorInvalidValue;
        if (wide_can) sk = 1;
        wide = wide_can && wmode > 0;
    }
    if (wide) {
        a.tiles_m = cdiv(g.M, WTM); a.tiles_n = cdiv(g.N, WTN);
        a.ntiles = a.tiles_m * a.tiles_n;
        a.splitk = 1;
        a.kslice = cdiv(g.K, 32) * 32;
        // per call: the attribute belongs to the CURRENT device's copy of the kernel; a host-side table write, no device work
        hipError_t e = hipFuncSetAttribute((const void*)gemm32_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, W_LDS_BYTES);
        if (e != hipSuccess) return 1000 + (int)e;
        hipLaunchKernelGGL(gemm32_wide_kernel, dim3(cdiv(a.ntiles, 8) * 8), dim3(256), W_LDS_BYTES, st, a);
        e = hipGetLastError();
        return e == hipSuccess ? 1 : 1000 + (int)e;
    }
    // The 256 x 256 stream-K kernel (gemm32_gram_kernel) takes lower-triangular products of two k-contiguous operands outside
    // deterministic mode.  The rule, from the table of profiles/gram_wide_ab.txt section 1: every workgroup (one per CU) gets at least
    // G32_GRAM_STAGES stages of the (tile, stage) sequence -- each workgroup pays two first stages and two 256 KB atomic epilogues in
    // the open and all CUs flush together at the end, which a short walk does not earn back.
    const bool gram_can = out_lower && akc && bkc && dma_ok && !g.slab;
    if (gmode == 2 && out_lower && !gram_can) return 1000 + (int)hipErrorInvalidValue;
    if (gram_can && gmode != 0) {
        static int cus[64];                          // CUs of each device (0 = not asked yet; the same value whoever writes it)
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return 1000 + (int)e;
        int ncu = (dev >= 0 && dev < 64) ? cus[dev] : 0;
        if (ncu <= 0) {
            e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
            if (e != hipSuccess || ncu <= 0) return 1000 + (int)(e != hipSuccess ? e : hipErrorInvalidValue);
            if (dev >= 0 && dev < 64) cus[dev] = ncu;
        }
        const char* cenv = getenv("DSVGP_G32_GRAM_KCHUNKS");
        const int kchunks = cenv ? atoi(cenv) : G32_GRAM_KCHUNKS;
        // DSVGP_G32_GRAM_LIVE=0: every tile runs FULL and the workgroups get equal stage counts (the kernel before the patterns)
        const char* lenv = getenv("DSVGP_G32_GRAM_LIVE");
        const int live = lenv ? (atoi(lenv) != 0) : 1;
        G32Gram w{};
        w.walk = gram_walk_make(g.M, g.N, g.K, GT, GBK, kchunks, live);
        if (gmode != 3 || w.walk.G >= (long long)G32_GRAM_STAGES * ncu) {
            w.A = a.A; w.B = a.B; w.C = a.C; w.lda = g.lda; w.ldb = g.ldb; w.ldc = g.ldc;
            w.M = g.M; w.N = g.N; w.K = g.K; w.nwg = ncu; w.alpha = a.alpha;
            if (!(fl & DSVGP_GEMM_C_ZEROED)) {       // the units accumulate onto zeros (and the strict upper triangle is defined as zero)
                e = zero_block(a.C, sizeof(float), a.ldc, a.M, a.N, st);
                if (e != hipSuccess) return 1000 + (int)e;
            }
            e = hipFuncSetAttribute((const void*)gemm32_gram_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, G_LDS_BYTES);   // (per call: as above)
            if (e != hipSuccess) return 1000 + (int)e;
            hipLaunchKernelGGL(gemm32_gram_kernel, dim3(cdiv(ncu, 8) * 8), dim3(256), G_LDS_BYTES, st, w);
            e = hipGetLastError();
            return e == hipSuccess ? 1 : 1000 + (int)e;
        }
    }
    sk = slab_slices(g, sk, sizeof(float));         // deterministic mode: as many slices as the caller's scratch holds
    a.splitk = sk;
    a.kslice = cdiv(cdiv(g.K, sk), 32) * 32;
    a.splitk = cdiv(g.K, a.kslice);
    a.slab = (g.slab && a.splitk > 1) ? (float*)g.slab : nullptr;
    if (!a.slab && (a.splitk > 1 || (out_lower && !(fl & DSVGP_GEMM_UPPER_UNDEF))) && !(fl & DSVGP_GEMM_C_ZEROED)) {
        // atomics accumulate onto zeros / the strict upper triangle is defined as zero
        // (contiguous rows: one linear fill -- the 2-D fill kernel of the runtime takes 104 us for 36 MB, the linear one ~10)
        hipError_t e = zero_block(a.C, sizeof(float), a.ldc, a.M, a.N, st);
        if (e != hipSuccess) return 1000 + (int)e;
    }
    const dim3 grid(cdiv((int64_t)a.ntiles * a.splitk, 8) * 8);
    if (dma_ok) {
        if (akc && bkc) hipLaunchKernelGGL((gemm32_dma_kernel<G32_MF, true, true, G32_DMA_BK>), grid, dim3(256), 0, st, a);
        else if (akc) hipLaunchKernelGGL((gemm32_dma_kernel<G32_MF, true, false, G32_DMA_BK>), grid, dim3(256), 0, st, a);
        else if (bkc) hipLaunchKernelGGL((gemm32_dma_kernel<G32_MF, false, true, G32_DMA_BK>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((gemm32_dma_kernel<G32_MF, false, false, G32_DMA_BK>), grid, dim3(256), 0, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return 1000 + (int)e;
    } else
    {
        const int rc = dispatch32<G32_BK>(st, a, grid, akc, bkc);
        if (rc != 1) return rc;
    }
    if (a.slab) {
        const int rc = launch_splitk_reduce(st, 0, a.slab, a.splitk, a.M, a.N, a.C, a.ldc, nullptr, 0, out_lower ? 1 : 0, 0);
        if (rc) return rc;
    }
    return 1;
}
