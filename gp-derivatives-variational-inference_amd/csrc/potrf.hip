// Blocked right-looking Cholesky of the fp64 K_ZZ (algo 1 of dsvgp_potrf), one fused MFMA launch per 64-column block.
// reference: psd_safe_cholesky(K_ZZ.double()) -> torch.cholesky (DirectionalGradVariationalStrategy.py:72-75).
//
// rocSOLVER's dpotrf takes 8.1 ms at M' = 3000 (serial single-workgroup panel kernels + many small launches); a first
// blocked version here (diagonal-block kernel + panel GEMM + trailing GEMM per block column, 141 launches) took 4.5 ms.
// What is here: one launch per block column (chol_step_kernel) + one batched panel launch, the factor WITH the fused inverse,
// 1.085 ms at M' = 3000 and 0.174 ms at 600 (tools/potrf_inv_probe.py).  In every step launch
//   * workgroup 0 is the CRITICAL workgroup: it updates the next diagonal tile and factors it with the tile in registers, one
//     16-row strip per wave, hand-offs through LDS flag words (crit_strips_update + factor64_strips);
//   * the other workgroups take strips of update / inverse tiles: two LDS tiles and two workgroups per CU, or -- launches from
//     `pipe_from` on with more than POTRF_PIPE_MIN_TILES tiles -- the PIPE instantiation, one workgroup per CU with the strip
//     software-pipelined (strip_pipe).
// Tools: per-launch trace tools/potrf_inv_trace.sh; in-kernel stamps of the critical workgroup tools/potrf_clock.sh (-DPOTRF_DEBUG);
// per-workgroup phases tools/potrf_wgtrace.sh (-DPOTRF_TRACE).
// Tried, measured and removed in the build-variant clean-up (last present in 8a953b7), each behind a build switch until then:
//   * round 5's critical workgroup with the diagonal tile in LDS (POTRF_CRIT_STRIPS = 0):
//     see the record above factor64_strips; its column-by-column 16-column chain (POTRF_F16_BLK = 0): 1.41 / 1.67 / 0.252 ms at
//     n = 3000 / 3300 / 600 against 1.355 / 1.62 / 0.222 for the four-column blocks (round 2); both rank-1 updates of that chain
//     through w = a_ij / a_jj (POTRF_FOLD, round 4): n = 3000 1.400 / 1.406 -> 1.396 / 1.414 ms, n = 600 0.250 -> 0.252 -- latency-,
//     not issue-bound;
//   * the timing ablations POTRF_ABL_NOC / NOP / P1 (wrong numbers by construction) and the A/B switches POTRF_PIPE, POTRF_PIPE_LATE0,
//     POTRF_PIPE_FROM of the pipelined strips, which had served their measurements.
// Measured without effect on the chain (+-1 %, removed again): multipliers folded once per column of the 16-column chain, operand
// reads of the 64^3 products pipelined in chunks.
#include "common.h"

#include <type_traits>

namespace {

constexpr int NBC = 64;

// Update / inverse tiles of one tile row are dealt to workgroups in STRIPS of up to `strip` block columns: T = A_ik W_k is formed
// once per strip (1 + strip products for strip tiles instead of 2 per tile, A_ik and W_k loaded once).  The launcher picks the
// strip length per launch from the tile count: long strips only where the launch is bound by its tiles, not by the diagonal
// workgroup (a strip of 4 lasts about as long as the diagonal workgroup's load -> update -> factor chain).
#ifndef POTRF_STRIP_T6
#define POTRF_STRIP_T6 900      // tiles in the launch above which strips of 6 are used (8: slower, 1.56 vs 1.41 ms at n = 3000)
#endif
#ifndef POTRF_STRIP_T4
#define POTRF_STRIP_T4 512      // ... strips of 4
#endif
#ifndef POTRF_STRIP_T2
#define POTRF_STRIP_T2 256      // ... strips of 2
#endif
#ifndef POTRF_STRIP_V6
#define POTRF_STRIP_V6 6        // strip lengths of the three classes (probes)
#endif
#ifndef POTRF_STRIP_V4
#define POTRF_STRIP_V4 4
#endif
#ifndef POTRF_STRIP_V2
#define POTRF_STRIP_V2 2
#endif
// -------------------------------------------------------------------------------------------------
// ONE launch per block column.
//   With X_k = inv(L_kk) and W_k = X_k^T X_k = inv(A_kk) the rank-64 update of step k needs no solved panel:
//       A_ij -= L_ik L_jk^T = (A_ik W_k) A_jk^T                  (i >= j > k)
//   so kernel k does, per 64 x 64 trailing tile, T = A_ik W_k and A_ij -= T A_jk^T out of LDS (column k of A is
//   read-only in that launch: no in-place hazard), and the workgroup of tile (k+1, k+1) goes on to factor its
//   updated tile: L_{k+1,k+1}, X_{k+1}, W_{k+1}.  The solved panels L_ik = A_ik X_k^T are formed afterwards by ONE
//   batched launch.  Critical path per block column: load + update + the factorisation of one 64 x 64 tile by the critical
//   workgroup (the section above factor64_strips).
// -------------------------------------------------------------------------------------------------
using acc4 = double __attribute__((ext_vector_type(4)));
#ifdef POTRF_DEBUG
#ifndef POTRF_DEBUG_K
#define POTRF_DEBUG_K 20      // block column whose critical workgroup is stamped
#endif
__device__ unsigned long long chol_dbg[64];
// stamps pinned in place (the scalar s_memtime would otherwise be scheduled ahead of the MFMAs it is meant to follow) and kept
// in registers until the end of the kernel (a global store per stamp would sit in vmcnt and stretch the waits that follow it)
#define CHOL_STAMP_DECL unsigned long long st_[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define CHOL_STAMP(slot) do { __builtin_amdgcn_sched_barrier(0); \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_[slot]) :: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#define CHOL_STAMP_FLUSH do { if (b == 0 && k == POTRF_DEBUG_K && tid == 0) { for (int q_ = 0; q_ < 8; ++q_) chol_dbg[q_] = st_[q_]; } } while (0)
#else
#define CHOL_STAMP_DECL
#define CHOL_STAMP(slot) do { } while (0)
#define CHOL_STAMP_FLUSH do { } while (0)
#endif
// per-workgroup phase trace of ONE step launch (tools/potrf_wgtrace.py; -DPOTRF_TRACE -DPOTRF_DEBUG_K=k): thread 0 of every workgroup
// stamps s_memtime into an LDS array at phase boundaries and copies it out on exit; slot 22 = role / strip, slot 23 = hardware id
#ifdef POTRF_TRACE
#ifndef POTRF_DEBUG_K
#define POTRF_DEBUG_K 20
#endif
constexpr int TR_SLOTS = 24, TR_MAXWG = 4096;
__device__ unsigned long long chol_trace[TR_MAXWG * TR_SLOTS];
#define TR_DECL __shared__ unsigned long long trs_[TR_SLOTS]; if (threadIdx.x < TR_SLOTS) trs_[threadIdx.x] = 0
#define TR(slot) do { if (k == POTRF_DEBUG_K && threadIdx.x == 0) { __builtin_amdgcn_sched_barrier(0); \
        trs_[slot] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#define TR_VAL(slot, v) do { if (k == POTRF_DEBUG_K && threadIdx.x == 0) trs_[slot] = (unsigned long long)(v); } while (0)
#define TR_FLUSH do { if (k == POTRF_DEBUG_K && threadIdx.x == 0 && blockIdx.x < TR_MAXWG) { \
        trs_[23] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4); \
        trs_[21] = __builtin_amdgcn_s_memtime(); \
        for (int q_ = 0; q_ < TR_SLOTS; ++q_) chol_trace[(size_t)blockIdx.x * TR_SLOTS + q_] = trs_[q_]; } } while (0)
#define PIPE_TR(slot) do { if (trs && threadIdx.x == 0) { __builtin_amdgcn_sched_barrier(0); \
        trs[slot] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define PIPE_TR(slot) do { } while (0)
#define TR_DECL
#define TR(slot) do { } while (0)
#define TR_VAL(slot, v) do { } while (0)
#define TR_FLUSH do { } while (0)
#endif
constexpr int LDT = 66;                       // LDS row stride of a 64 x 64 tile (doubles)

__device__ __forceinline__ double readlane_f64(double v, int l) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, l);
    hi = __builtin_amdgcn_readlane(hi, l);
    return __hiloint2double(hi, lo);
}

// 64 x 64 x 64 product by 4 waves (wave -> 32 x 32 outputs):  acc[i][j] = sum_q Aop[m][q] * Bop(q, n)
//   B_NK: Bop(q, n) = Bs[n][q]   (B given as [n][k]);  else Bop(q, n) = Bs[q][n]
//   ACC_INIT: the caller has loaded the accumulators (acc += product)
template <bool B_NK, int NW = 4, bool ACC_INIT = false>
__device__ __forceinline__ void tile_product(const double (*As)[LDT], const double (*Bs)[LDT], int lane, int wr, int wc,
                                             acc4 (&acc)[2][8 / NW]) {
    constexpr int NJ = 8 / NW;            // 16-column sub-tiles per wave: 2 (4 waves, 32 x 32 each) or 1 (8 waves, 32 x 16 each)
    if constexpr (!ACC_INIT) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = acc4{0, 0, 0, 0};
    }
    // all operands of the wave first, then back-to-back MFMAs: the loops are
    // fully unrolled (a rolled loop moves the accumulators AGPR <-> VGPR and drains the MFMA pipe every trip)
    double a[2][16], b[NJ][16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        const int kq = 4 * ks + (lane >> 4);
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i][ks] = As[wr * 32 + i * 16 + (lane & 15)][kq];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int n = wc * (16 * NJ) + j * 16 + (lane & 15);
            b[j][ks] = B_NK ? Bs[n][kq] : Bs[kq][n];
        }
    }
#pragma unroll
    for (int ks = 0; ks < 16; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i][ks], b[j][ks], acc[i][j], 0, 0, 0);
}

// Tried and removed: the same product issuing the NEXT block column's global loads between its MFMAs (POTRF_IL;
// round 5, profiles/r05_b_potrf_tile_roles.txt: n = 3000 1.33 -> 1.27 ms, n = 3300 1.60 -> 1.54 at one wave per SIMD, 1.48 ms with 23 spilled
// registers at two, the STEP unmoved: C4 12.81 / 12.78 against 12.83 / 12.79, C3 7.055 against 7.06); removed in the build-variant clean-up; last present in 8a953b7.

// -------------------------------------------------------------------------------------------------
// Software-pipelined strip (round 5; the PIPE instantiation of chol_step_kernel: ONE workgroup per CU, three LDS tiles).
// A tile-bound launch of the chain is one strip workgroup per CU running  T = A_ik W_k  and then, per block column of its strip,
// C_c -= T B_c^T:  measured (profiles/r05_b_potrf_tile_roles.txt) 9.4k cycles per column of which 4.1k are the product's MFMAs --
// the next column's 32 loads are issued in front of the product (2.2k), its operand goes to LDS between two barriers (1.5k), the
// result is stored behind it (0.9k).  Here all of that rides INSIDE the MFMA stream of the product:
//   product(c)  reads -T (S[0]) and B_c (S[2 - c % 2]); in front of it the wave issues its 8 LDS-DMA instructions of B_{c+1} (into
//               the other B buffer: global -> LDS, no registers, no ds_write); after each of its first 8 k-steps (4 MFMAs) it
//               issues two loads of C_{c+1} and two stores of the result of column c - 1;
//   then ONE drain + barrier closes the column (everything was issued >= 8 k-steps earlier).
// Register sets rotate by NAME, not by copying (a copy of a register a load is still filling waits for the load): a C set is loaded
// in stage c - 1, accumulates in stage c, is stored in stage c + 1 -- three sets; with the two B buffers the loop body is six stages.
// (First version, measured: B rows staged through registers one stage further ahead -- 356 registers, spills whose reloads wait
// vmcnt(0); selects on loaded values became branches around the loads and cut the scheduling regions.)
// An LDS-DMA instruction writes 64 x 16 bytes CONTIGUOUSLY (two rows of a tile), so B's LDS image is rows in PAIRS with a stride of
// 132 doubles per pair, and the 16-byte granules of the odd row of a pair are stored at column c ^ 18 (applied to the SOURCE
// address): bsw below; the fragment reads of both operand orientations are then conflict-free (32 lanes, 32 distinct bank pairs).
// B_NK: B_c given as [n][k] (update role: rows of A_jk) or [k][n] (inverse role: R_kj).  ident_after: the block column BEHIND the
// ncols pipelined ones has B = I and old C = 0 (inverse role, j == k: always the strip's last): its result is -T itself, stored from
// LDS at the end, no product.  last_diag: the last column is a diagonal tile (only n <= m is stored).  All 64 rows of every C tile
// are stored (callers: interior tile rows only), ldB must be even (16-byte source granules).  On entry: T = the product A_ik W_k,
// S[0] / S[1] still being read by the other waves (the barrier is here), cs[0] = column 0's C elements (requested by the caller),
// B_0 already in S[2] (pipe_dma_tile, issued by the caller before its own loads).
// -------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* potrf_lds_ptr_t;
constexpr int BPAIR = 132;                                  // doubles per row pair of a DMA-filled B image (64 x 66 = 32 x 132)
// bsw(row, col) = (row >> 1) * BPAIR + (row & 1) * 64 + (col ^ ((row & 1) * 18)): offset (doubles) of element (row, col) in a B image
// One LDS-DMA instruction as an asm statement: no VGPR destination, and WE count it (s_waitcnt vmcnt(0) before the barrier that
// ends the stage) -- through the builtin hipcc parks a vmcnt(0) in front of the next LDS read (see gemm32.hip).  M0 (the LDS
// destination base) is compiler-reserved: saved, set and restored inside the statement.
__device__ __forceinline__ void potrf_lds_dma16(const double* gsrc, unsigned lds_byte_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_byte_addr) : "memory");
}
// the 64 x 64 tile at Bt (row stride ldB) into the B image Bs: wave w fills row pairs 8 w .. 8 w + 7
__device__ __forceinline__ void pipe_dma_tile(double (*Bs)[LDT], const double* __restrict__ Bt, int64_t ldB) {
    const int lane = threadIdx.x & 63;
    const unsigned wave_u = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int par = lane >> 5, col = ((2 * lane) & 63) ^ (par * 18);
    const double* src = Bt + (int64_t)(16 * wave_u + par) * ldB + col;
    const unsigned dst = (unsigned)(uintptr_t)(potrf_lds_ptr_t)&Bs[0][0] + wave_u * (8 * BPAIR * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) potrf_lds_dma16(src + (int64_t)(2 * i) * ldB, dst + i * (BPAIR * 8));
}

// The lane's two base addresses into a B image (the swizzle folded into them, so that every fragment read of a product is
// base + compile-time offset):  B_NK: lane (g, m) reads rows wc 32 + 16 j + m, column 4 ks + g -- for an odd row the column is
// (4 ks) ^ 16 + (g ^ 2): base[0] serves the k-steps with bit 2 clear, base[1] those with it set, + 4 ks + 1056 j doubles;
// [k][n]: rows 4 ks + g, columns wc 32 + 16 j + m -- for an odd row 16 (j ^ 1) + (m ^ 2): base[j], + 264 ks doubles.
template <bool B_NK>
__device__ __forceinline__ void pipe_bases(int lane, int wc, int (&base)[2]) {
    const int g = lane >> 4, m = lane & 15;
    if constexpr (B_NK) {
        const int odd = m & 1, r = ((wc * 32 + m) >> 1) * BPAIR + odd * 64 + (g ^ (2 * odd));
        base[0] = r + 16 * odd;
        base[1] = r - 16 * odd;
    } else {
        const int odd = g & 1, r = (g >> 1) * BPAIR + odd * 64 + wc * 32 + (m ^ (2 * odd));
        base[0] = r + 16 * odd;
        base[1] = r + 16 - 16 * odd;
    }
}

template <bool B_NK, bool HAS_PREV, typename F>
__device__ __forceinline__ void pipe_product(const double (*Ts)[LDT], const double* __restrict__ Bs, const int (&base)[2], int lane,
                                             int wr, double (&accd)[2][2][4], F&& hook) {
    const int g = lane >> 4, m = lane & 15;
    acc4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = acc4{accd[i][j][0], accd[i][j][1], accd[i][j][2], accd[i][j][3]};
    const double* ta = &Ts[wr * 32 + m][g];
    const double* b0 = Bs + base[0];
    const double* b1 = Bs + base[1];
    double a[16][2], b[16][2];
    auto rd = [&](int ks) {
#pragma unroll
        for (int i = 0; i < 2; ++i) a[ks][i] = ta[i * 16 * LDT + 4 * ks];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[ks][j] = B_NK ? ((ks & 4) ? b1 : b0)[4 * ks + j * 8 * BPAIR] : (j ? b1 : b0)[ks * 2 * BPAIR];
    };
    rd(0);
    rd(1);
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        if (ks + 2 < 16) rd(ks + 2);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks][i], b[ks][j], acc[i][j], 0, 0, 0);
        if (ks < 8) hook(ks, std::integral_constant<bool, HAS_PREV>{});
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);      // fragment reads of k-step ks + 2
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);      // the four MFMAs of k-step ks
        if (ks < 8) {
            __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);                  // two loads of C_{c+1}
            if (HAS_PREV) __builtin_amdgcn_sched_group_barrier(0x040, 2, 0);    // two stores of column c - 1
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) accd[i][j][q] = acc[i][j][q];
}

template <bool B_NK>
__device__ __forceinline__ void strip_pipe(double (*S)[64][LDT], const double* __restrict__ Bg, int64_t ldB, int64_t dB,
                                           double* __restrict__ Cg, int64_t ldC, int ncols, bool ident_after, bool last_diag,
                                           acc4 (&T)[2][2], double (&cs)[3][2][2][4], unsigned long long* trs = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int ml0 = wr * 32 + (lane >> 4), nl0 = wc * 32 + (lane & 15);
    const int64_t step4C = 4 * ldC;
    __syncthreads();                                        // every wave is done reading A_ik / W_k for T
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) S[0][wr * 32 + i * 16 + (lane >> 4) + 4 * q][wc * 32 + j * 16 + (lane & 15)] = -T[i][j][q];
    __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0): the caller's B_0 (LDS-DMA, not counted by the compiler) and C_0
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int base[2];
    pipe_bases<B_NK>(lane, wc, base);
    PIPE_TR(2);                                             // (trace: T formed and back in LDS)
    auto stage = [&](auto s_, int c) {
        constexpr int s = decltype(s_)::value;
        double (&acc)[2][2][4] = cs[s % 3];          // (plain doubles, not acc4: element writes into an array of vectors kept it in scratch)
        double (&nxt)[2][2][4] = cs[(s + 1) % 3];
        double (&prev)[2][2][4] = cs[(s + 2) % 3];
        // column c + 1 (clamped to the strip's last column: a harmless re-read at its end)
        const int c1 = min(c + 1, ncols - 1);
        pipe_dma_tile(S[1 + (s & 1)], Bg + (int64_t)c1 * dB, ldB);
        const double* pc = Cg + (int64_t)c1 * 64;
        double* pd = Cg + (int64_t)(c - 1) * 64;
        auto hook = [&](int ks, auto has_prev) {            // ks = 0..7 = the row step t of this thread's C elements
#pragma unroll
            for (int j = 0; j < 2; ++j) nxt[ks >> 2][j][ks & 3] = pc[j * 16];
            pc += step4C;
            if constexpr (decltype(has_prev)::value) {
#pragma unroll
                for (int j = 0; j < 2; ++j) pd[j * 16] = prev[ks >> 2][j][ks & 3];     // (unpredicated: a branch would cut the scheduling region)
                pd += step4C;
            }
        };
        const double* Bcur = &S[2 - (s & 1)][0][0];
        if (c < 5) PIPE_TR(3 + 3 * c);
        if (s != 0 || c > 0) pipe_product<B_NK, true>(S[0], Bcur, base, lane, wr, acc, hook);
        else pipe_product<B_NK, false>(S[0], Bcur, base, lane, wr, acc, hook);
        if (c < 5) PIPE_TR(4 + 3 * c);
        // this wave's share of B_{c+1} has landed (and C_{c+1}, and the stores).  The BUILTIN, not an asm statement: the compiler's own
        // count of its loads restarts here -- otherwise the next stage's first MFMAs wait "vmcnt(3)" for accumulators that are long
        // there, and that wait now includes five of the eight DMA instructions just issued.
        __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0) only (gfx9 encoding: expcnt 7, lgkmcnt 15 = no wait)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (and one the wait-count pass cannot weaken: the DMA is invisible to it)
        __syncthreads();                                    // B_{c+1} is complete; every wave is done with B_c
        if (c < 5) PIPE_TR(5 + 3 * c);
    };
    // the strip's last column leaves from the stage that computed it (one store loop per register set: choosing the set behind the
    // loop made its address a phi of three allocas, and the sets stayed in scratch)
    auto store_last = [&](double (&res)[2][2][4]) {
        double* pd = Cg + (int64_t)(ncols - 1) * 64;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int ml = ml0 + 4 * t, nl = nl0 + j * 16;
                if (!(last_diag && nl > ml)) pd[j * 16] = res[t >> 2][j][t & 3];
            }
            pd += step4C;
        }
    };
    for (int c = 0; c < ncols; c += 6) {
        stage(std::integral_constant<int, 0>{}, c);
        if (c + 1 >= ncols) { store_last(cs[0]); break; }
        stage(std::integral_constant<int, 1>{}, c + 1);
        if (c + 2 >= ncols) { store_last(cs[1]); break; }
        stage(std::integral_constant<int, 2>{}, c + 2);
        if (c + 3 >= ncols) { store_last(cs[2]); break; }
        stage(std::integral_constant<int, 3>{}, c + 3);
        if (c + 4 >= ncols) { store_last(cs[0]); break; }
        stage(std::integral_constant<int, 4>{}, c + 4);
        if (c + 5 >= ncols) { store_last(cs[1]); break; }
        stage(std::integral_constant<int, 5>{}, c + 5);
        if (c + 6 >= ncols) { store_last(cs[2]); break; }
    }
    if (ident_after) {                                      // C_ncols = 0 - T I: this thread's elements of -T, back from LDS
        double* pd = Cg + (int64_t)ncols * 64;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
#pragma unroll
            for (int j = 0; j < 2; ++j) pd[j * 16] = S[0][ml0 + 4 * t][nl0 + j * 16];
            pd += step4C;
        }
    }
}

// Fused inverse (Rw != nullptr): the same launches also run the forward elimination of the identity, block row by
// block row, so that Y = L^-1 is complete when the factorisation is (no separate trtri recursion):
//   R-tiles  (i > k, j <= k):  R_ij -= (A_ik W_k) R_kj,  R_kk = I     (the W_k form of  R_i -= L_ik Y_k,  Y_k = X_k R_k)
//   Y-tiles  (j <= k):         Y_kj  = X_k R_kj                        (row block k of L^-1 is final)
// Row k of R was completed by launch k-1 and is read-only here; these tiles ride on the CUs the latency-bound
// factorisation chain leaves idle.
template <int NW = 4, bool PIPE = false>
__device__ __forceinline__ void chol_inverse_tile(double (*S)[64][LDT], const double* __restrict__ A, int64_t lda, int n,
                                                  int k, int e, const double* __restrict__ Xws,
                                                  const double* __restrict__ Wws, double* __restrict__ Rw, int64_t ldr,
                                                  double* __restrict__ Y, int64_t ldy, int nblk,
                                                  double* __restrict__ YT, int strip = 1
#ifdef POTRF_TRACE
                                                  , unsigned long long* trs_ = nullptr
#endif
                                                  ) {
    constexpr int WC = NW / 2, NJ = 8 / NW, NU = 64 / NW;     // column groups of waves, 16-column sub-tiles per wave, rows per thread
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave / WC, wc = wave % WC;
    const int nt = nblk - (k + 1), spr = (k + strip) / strip, nR = nt * spr;     // strips per tile row of R
    const int k0 = k * 64;
    const bool ytile = e >= nR;
    int j = ytile ? (e - nR) : (e % spr) * strip;                    // (first) block column
    const int ncols = ytile ? 1 : min(strip, k + 1 - j);
    const int i0 = ytile ? k0 : (k + 1 + e / spr) * 64;
    int j0 = j * 64;
    const double* Lk = ytile ? (Xws + (size_t)k * 4096) : (Wws + (size_t)k * 4096);
    if constexpr (PIPE && NW == 4) {
        if (!ytile) {                                   // R strip, software-pipelined (R is padded to whole blocks: no clamping there)
            const int ml0 = wr * 32 + (lane >> 4), nl0 = wc * 32 + (lane & 15);
            const int64_t rstep = (int64_t)4 * ldr;
            double cs[3][2][2][4];
            double* const Cg = Rw + (int64_t)(i0 + ml0) * ldr + j0 + nl0;
            const double* const Bg = Rw + (int64_t)k0 * ldr + j0;
            const bool ident_after = k - j < ncols;               // the strip ends with block column j == k: R_kk = I, old R_ik = 0
            const int np = ident_after ? ncols - 1 : ncols;       // block columns that take a product
            {
                double ra[16], rw[16];
                const int64_t arow0 = (int64_t)(i0 + (tid >> 6)) * lda, alast = (int64_t)(n - 1) * lda, astep = (int64_t)4 * lda;
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int r = (tid >> 6) + 4 * u, c = tid & 63;
                    ra[u] = A[((i0 + r < n) ? arow0 + u * astep : alast) + k0 + c];
                    rw[u] = Lk[r * 64 + c];
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int r = (tid >> 6) + 4 * u;
                    S[0][r][tid & 63] = (i0 + r < n) ? ra[u] : 0.0;
                    S[1][r][tid & 63] = rw[u];
                }
            }
            __syncthreads();
            pipe_dma_tile(S[2], Bg, ldr);
#pragma unroll
            for (int t = 0; t < 8; ++t)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) cs[0][t >> 2][jj][t & 3] = Cg[t * rstep + jj * 16];
            acc4 acc[2][2];
#ifdef POTRF_TRACE
            if (trs_) { TR(1); TR_VAL(20, (ncols << 16) | (e / spr)); }
#endif
            tile_product<true, 4>(S[0], S[1], lane, wr, wc, acc);            // T = A_ik W_k (W symmetric: [n][k] == [k][n])
#ifdef POTRF_TRACE
            strip_pipe<false>(S, Bg, ldr, (int64_t)64, Cg, ldr, np, ident_after, false, acc, cs, k == POTRF_DEBUG_K ? trs_ : nullptr);
#else
            strip_pipe<false>(S, Bg, ldr, (int64_t)64, Cg, ldr, np, ident_after, false, acc, cs);
#endif
            return;
        }
    }
    // two LDS tiles only (two workgroups per CU): R_kj waits in registers until T = A_ik W_k has been formed
    double rc[NU];
    double ro[2][NJ][4];      // R-tile: the old R_ij, requested with the operands (not as 16 load -> wait -> store round trips at the end)
    double* rdst = Rw + (int64_t)(i0 + wr * 32 + (lane >> 4)) * ldr + j0 + wc * (16 * NJ) + (lane & 15);
    {
        double ra[NU], rb[NU];
        const int64_t arow0 = (int64_t)(i0 + (tid >> 6)) * lda, alast = (int64_t)(n - 1) * lda, astep = (int64_t)NW * lda;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int r = (tid >> 6) + NW * u, c = tid & 63;
            ra[u] = ytile ? 0.0 : A[((i0 + r < n) ? arow0 + u * astep : alast) + k0 + c];
            rb[u] = Lk[r * 64 + c];
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {           // (behind the operands of the first product)
            const int r = (tid >> 6) + NW * u, c = tid & 63;
            rc[u] = (j == k) ? ((r == c) ? 1.0 : 0.0) : Rw[(int64_t)(k0 + r) * ldr + j0 + c];
        }
        if (!ytile && j != k) {              // (R is padded to whole blocks: no clamping)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
                    for (int q = 0; q < 4; ++q) ro[i][jj][q] = rdst[(int64_t)(i * 16 + 4 * q) * ldr + jj * 16];
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
                    for (int q = 0; q < 4; ++q) ro[i][jj][q] = 0.0;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int r = (tid >> 6) + NW * u, c = tid & 63;
            S[0][r][c] = ytile ? rb[u] : ((i0 + r < n) ? ra[u] : 0.0);      // Y-tile: X_k is the left operand already
            S[1][r][c] = ytile ? rc[u] : rb[u];
        }
    }
    __syncthreads();
#ifdef POTRF_TRACE
    if (trs_) { TR(1); TR_VAL(20, ((ytile ? 0 : ncols) << 16) | (ytile ? 0xffff : (e / spr))); }
#endif
    acc4 acc[2][NJ];
    if (!ytile) {
        tile_product<true, NW>(S[0], S[1], lane, wr, wc, acc);          // T = A_ik W_k
#ifdef POTRF_TRACE
        if (trs_) TR(2);
#endif
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
                for (int q = 0; q < 4; ++q) {       // -T to LDS, accumulators restart from the old R_ij: the second product leaves R_ij - T R_kj
                    S[0][wr * 32 + i * 16 + (lane >> 4) + 4 * q][wc * (16 * NJ) + jj * 16 + (lane & 15)] = -acc[i][jj][q];
                    acc[i][jj][q] = ro[i][jj][q];
                }
#pragma unroll 1
        for (int cc = 0; cc < ncols; ++cc) {         // the strip: -T stays in S[0], R_kj and the old R_ij change per block column
            if (cc > 0) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[i][jj][q] = ro[i][jj][q];
            }
#pragma unroll
            for (int u = 0; u < NU; ++u) S[1][(tid >> 6) + NW * u][tid & 63] = rc[u];
            __syncthreads();
#ifdef POTRF_TRACE
            if (trs_ && cc < 5) TR(3 + 3 * cc);
#endif
            double* const rcur = rdst;
            if (cc + 1 < ncols) {                    // next block column: requested now, consumed after this product
                ++j; j0 += 64; rdst += 64;
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int r = (tid >> 6) + NW * u, c = tid & 63;
                    rc[u] = (j == k) ? ((r == c) ? 1.0 : 0.0) : Rw[(int64_t)(k0 + r) * ldr + j0 + c];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            ro[i][jj][q] = (j == k) ? 0.0 : rdst[(int64_t)(i * 16 + 4 * q) * ldr + jj * 16];
            }
            tile_product<false, NW, true>(S[0], S[1], lane, wr, wc, acc);   // R_ij - T R_kj
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        rcur[(int64_t)(i * 16 + 4 * q) * ldr + jj * 16] = acc[i][jj][q];
#ifdef POTRF_TRACE
            if (trs_ && cc < 5) TR(4 + 3 * cc);
#endif
#ifdef POTRF_TRACE
            if (trs_ && cc < 5) TR(5 + 3 * cc);
#endif
            if (cc + 1 < ncols) __syncthreads();     // every wave is done reading R_kj out of S[1]
        }
    } else {
        tile_product<false, NW>(S[0], S[1], lane, wr, wc, acc);         // X_k R_kj
        if (YT == nullptr) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int m = k0 + wr * 32 + i * 16 + (lane >> 4) + 4 * q, c = j0 + wc * (16 * NJ) + jj * 16 + (lane & 15);
                        if (m < n && c < n) Y[(int64_t)m * ldy + c] = acc[i][jj][q];
                    }
        } else {
            // the tile also goes out transposed (L^-T for the forward solves, which stream an mn-contiguous left operand):
            // through LDS, so that both images are written in full rows -- no separate transpose pass over L^-1
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        S[0][wr * 32 + i * 16 + (lane >> 4) + 4 * q][wc * (16 * NJ) + jj * 16 + (lane & 15)] = acc[i][jj][q];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int r = (tid >> 6) + NW * u, c = tid & 63;
                if (k0 + r < n && j0 + c < n) Y[(int64_t)(k0 + r) * ldy + j0 + c] = S[0][r][c];
                if (j0 + r < n && k0 + c < n) YT[(int64_t)(j0 + r) * ldy + k0 + c] = S[0][c][r];
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------
// Round 6: the critical workgroup's factorisation with the diagonal tile in registers and the inverse OFF the serial chain.
//
// Round 5 (the tile in LDS; removed in the build-variant clean-up, last present in 8a953b7): per 16-column block, ONE wave factors AND inverts the 16 x 16 diagonal block (4.4-4.7k cycles),
// then two barrier phases form the panel L_{ib,kb} = F_{ib,kb} X_d^T and the next diagonal block's update -- 6.7k cycles per block,
// 26.5k for the tile (of the critical workgroup's 37.6k).  The panel needed X_d only because it was written as an MFMA product.
// Here wave w owns rows 16 w .. 16 w + 15 of the tile for the WHOLE factorisation, in the register image
//     a[cb][t] = D[16 w + i][16 cb + 4 t + g]      (i = lane & 15, g = lane >> 4;  cb <= w)
// and block column kb is processed by all waves w >= kb together, four columns at a time:
//   * the DIAGONAL wave (w = kb) publishes the 16 x 4 column block of its strip, factors the 4 x 4 pivot block (four dependent
//     rsqrt), substitutes its rows against it and applies the rank-4 update D -= M M^T with ONE MFMA out of its own registers
//     (as round 5's one-wave chain did) -- but runs no forward elimination of the identity beside it: L only;
//   * the FOLLOWERS (w > kb) read the published block, redo the pivot factorisation (the same ten numbers in every lane), substitute
//     their own rows AND the diagonal block's rows (the B / A operands of the update D_w -= M_w M_d^T, computed transposed so that the
//     accumulator IS the a image), one block behind the diagonal wave and never waited for by it: the panel L_{w,kb} comes out of
//     the same substitution the diagonal block gets -- no inverse on the path;
//   * after the 16 columns wave w holds L_{w,kb}; it publishes the block (LDS, register image as it stands: readers use the same
//     lane map), applies  D_{w,cb} -= L_{w,kb} L_{cb,kb}^T  for cb = kb + 1 .. w (own block: both operands are its own registers),
//     and wave kb + 1 goes straight on as the next diagonal wave.
// Critical path: 4 x (16-column chain + 4 MFMAs), hopping from wave to wave.  X = L^-1 and W = X^T X are formed by the waves that
// are done with the chain: wave w inverts its diagonal block from registers (invert16_regs: the forward elimination of the old
// chain, now beside the NEXT wave's chain), wave c < r forms T_{r,c} = sum_j L_{r,j} X_{j,c} as soon as its inputs exist and
// X_{r,c} = -X_rr T_{r,c} when wave r has published X_rr; every wave accumulates its own blocks of W row by row.
// Synchronisation: LDS flags (one writer each, polled), no workgroup barrier after the update phase.  LDS: xs (packed lower
// blocks of X, row stride XB) and cpub (published column blocks) in the tile that held X_k; lpub (published L blocks) in the tile
// that holds P = A X_k^T, written only once every wave has left the update phase (FL_P flags).
// tools/crit_chain_emulator.py replays this routine lane by lane on the host (index algebra check).
// -------------------------------------------------------------------------------------------------
#ifndef POTRF_SPIN_SLEEP
#define POTRF_SPIN_SLEEP 1      // s_sleep argument between two polls of a flag word (0: none; measured: n = 600 0.194 -> 0.188 ms with 1, nothing more with 4)
#endif
constexpr int XB = 17;                                        // row stride (doubles) of a 16 x 16 block of X in LDS
constexpr int FL_C = 0, FL_P = 4, FL_L = 8, FL_X = 24, FL_N = 40;      // flag words: cflag[kb], pdone[w], lflag[r][j], xflag[r][c]
// (explicit LDS pointers: through generic pointers the volatile flag words became FLAT stores / loads with a vmcnt(0) wait behind each)
typedef __attribute__((address_space(3))) double LD;
typedef __attribute__((address_space(3))) volatile int LVI;
struct CritLds {
    LD* xs;               // 10 x 16 x XB
    LD* cpub;         // [4 kb][4 jb][80]: the pivot factors (10 words) and, from word 16, the block M of the diagonal wave, per 4-column block
    LD* lpub;             // [6][4 t][64 lanes]
    LD* own;              // [4 waves][64]
    LVI* fl;              // FL_N words, zeroed before use
#ifdef POTRF_DEBUG
    int dbg_gidx0;
    __attribute__((address_space(3))) unsigned long long* dbg;      // 64 stamp words (LDS: a stamp is one s_memtime + one ds_write of lane 0), copied to chol_dbg at the end
#endif
};
#ifdef POTRF_DEBUG
#define STRIPS_STAMP(slot) do { if (gidx0 == (POTRF_DEBUG_K + 1) * 64) { const unsigned long long t__ = __builtin_amdgcn_s_memtime(); if (lane == 0) S.dbg[slot] = t__; } } while (0)
#else
#define STRIPS_STAMP(slot) do { } while (0)
#endif
__device__ __forceinline__ int xblk(int r, int c) { return 16 * XB * (r * (r + 1) / 2 + c); }
__device__ __forceinline__ int lblk(int r, int j) { return 256 * (r * (r - 1) / 2 + j); }
// one writer per flag; LDS executes a wave's instructions in order, so the flag store behind the data stores needs no wait
__device__ __forceinline__ void fl_set(LVI* f, int v, int lane) {
    asm volatile("" ::: "memory");
    if (lane == 0) *f = v;
}
__device__ __forceinline__ void fl_wait(LVI* f, int v, int* info) {
    int n = 0;
    while (*f < v) {
        if (++n > (1 << 22)) {            // (never in a correct run: every flag is set unconditionally; a bounded spin cannot hang the card)
            if (info) *info = -777;
            break;
        }
#if POTRF_SPIN_SLEEP
        __builtin_amdgcn_s_sleep(POTRF_SPIN_SLEEP);
#endif
    }
    asm volatile("" ::: "memory");
}
struct Piv4 { double r0, r1, r2, r3, l10, l20, l30, l21, l31, l32; };
// 1 / sqrt(d) for the serial chain.  A single wave issues one fp64 instruction per ~5 cycles and a dependent one waits no longer than that
// (tools/lat_probe.cpp: dependent v_fma_f64 5.3, v_rsq_f64 16 cycles): the chain is bound by its INSTRUCTION COUNT.  v_rsq_f64 is good to
// 2.5e-8, so with e = 1 - d y^2 the step y (1 + e / 2 + 3 e^2 / 8) leaves 5 e^3 / 16 ~ 5e-24: full accuracy from five instructions.
// (Two Newton steps instead, POTRF_RSQ_HALLEY = 0 with POTRF_NEWTON = 2: 8 instructions; removed in the build-variant clean-up; last present in 8a953b7.)
__device__ __forceinline__ double rsqrt_chain(double d) {
    const double y = __builtin_amdgcn_rsq(d);
    const double gq = d * y;
    const double e = fma(-gq, y, 1.0);
    const double pq = fma(e, 0.375, 0.5);
    const double ye = y * e;
    return fma(ye, pq, y);
}
// the 4 x 4 pivot block (lower entries P_rc): reciprocal square roots of the pivots and the block's L entries
template <bool CHECK>
__device__ __forceinline__ Piv4 pivot4(double P00, double P10, double P11, double P20, double P21, double P22, double P30, double P31, double P32,
                                       double P33, int j0, int& bad) {
    Piv4 v;
    v.r0 = rsqrt_chain(P00);
    v.l10 = P10 * v.r0; v.l20 = P20 * v.r0; v.l30 = P30 * v.r0;
    const double d1 = fma(-v.l10, v.l10, P11);
    v.r1 = rsqrt_chain(d1);
    v.l21 = fma(-v.l20, v.l10, P21) * v.r1; v.l31 = fma(-v.l30, v.l10, P31) * v.r1;
    const double d2 = fma(-v.l21, v.l21, fma(-v.l20, v.l20, P22));
    v.r2 = rsqrt_chain(d2);
    v.l32 = fma(-v.l31, v.l21, fma(-v.l30, v.l20, P32)) * v.r2;
    const double d3 = fma(-v.l32, v.l32, fma(-v.l31, v.l31, fma(-v.l30, v.l30, P33)));
    v.r3 = rsqrt_chain(d3);
    if constexpr (CHECK) {
        bad = (bad < 0 && !(P00 > 0.0)) ? j0 : bad;
        bad = (bad < 0 && !(d1 > 0.0)) ? j0 + 1 : bad;
        bad = (bad < 0 && !(d2 > 0.0)) ? j0 + 2 : bad;
        bad = (bad < 0 && !(d3 > 0.0)) ? j0 + 3 : bad;
    }
    return v;
}
// one row's four block entries against the pivot block: M[row][0..3]; returns column g
__device__ __forceinline__ double subst4(double p0, double p1, double p2, double p3, const Piv4& v, int g) {
    const double m0 = p0 * v.r0;
    const double m1 = fma(-m0, v.l10, p1) * v.r1;
    const double m2 = fma(-m1, v.l21, fma(-m0, v.l20, p2)) * v.r2;
    const double m3 = fma(-m2, v.l32, fma(-m1, v.l31, fma(-m0, v.l30, p3))) * v.r3;
    asm volatile("" :: "v"(m1), "v"(m2), "v"(m3));      // (all four in every lane: left to itself hipcc sinks them under nested exec-mask branches on g)
    return (g == 0) ? m0 : ((g == 1) ? m1 : ((g == 2) ? m2 : m3));
}
typedef double __attribute__((ext_vector_type(2))) d2v;      // (a builtin vector: HIP's double2 class cannot be copied out of address space 3 in the host pass)
typedef __attribute__((address_space(3))) d2v LD2;
// The diagonal wave of block column kb (ONE copy of this code serves the four block columns: the wave that runs it for kb + 1 finds it in
// the instruction cache -- as four template instances every chain started with ~1k cycles of instruction fetch, profiles/r06_a_*).
// cur = D_kk -> L_kk (zero above the diagonal), rks[jb] = the four 1 / L_cc of block jb (the same in every lane).  Per 4-column block: the
// strip's column block goes through the wave's own LDS words once (row i's four entries for the substitution; rows j0 .. j0+3 are the pivot
// block, read as broadcasts), P_00 alone comes by v_readlane so that the first 1 / sqrt starts at once; the pivot factors (cpub[kb][jb][0..9])
// and the block M (the followers' A operand, lane for lane: cpub[..][16 + lane]) are published with ONE flag per block (cflag = jb + 1; the last block:
// 4 behind the factors, 5 behind M),
// behind the MFMA of the rank-4 update (the publication rides under its latency).
__device__ __forceinline__ void strips_diag(const CritLds& S, int kb, acc4& cur, acc4 (&rks)[4], int lane, int* info, int gidx0, int nvalid) {
    const int i = lane & 15, g = lane >> 4;
    LD* own = S.own + 64 * kb;
    int unused = -1;
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
        const int j0 = 4 * jb;
        LD* cb = S.cpub + (kb * 4 + jb) * 80;
        own[i * 4 + g] = cur[jb];                                    // D[i][j0 + g]
        __builtin_amdgcn_wave_barrier();
        const double P00 = readlane_f64(cur[jb], j0);
        const d2v p01 = *(const LD2*)(own + i * 4), p23 = *(const LD2*)(own + i * 4 + 2);
        const d2v R1 = *(const LD2*)(own + (j0 + 1) * 4), R2 = *(const LD2*)(own + (j0 + 2) * 4), R3 = *(const LD2*)(own + (j0 + 3) * 4),
                      R3b = *(const LD2*)(own + (j0 + 3) * 4 + 2);
        const double P22 = own[(j0 + 2) * 4 + 2];
        __builtin_amdgcn_sched_barrier(0);                           // (the exchange is issued HERE: its latency rides under the first 1 / sqrt)
        const Piv4 v = pivot4<false>(P00, R1.x, R1.y, R2.x, R2.y, P22, R3.x, R3.y, R3b.x, R3b.y, j0, unused);
        if (lane == 0) {
            cb[0] = v.r0; cb[1] = v.r1; cb[2] = v.r2; cb[3] = v.r3; cb[4] = v.l10; cb[5] = v.l20; cb[6] = v.l30; cb[7] = v.l21; cb[8] = v.l31;
            cb[9] = v.l32;
        }
        if (jb == 3) fl_set(S.fl + FL_C + kb, 4, lane);              // (the followers' last block needs the factors only: the next chain starts ~0.4k earlier)
        const double mraw = subst4(p01.x, p01.y, p23.x, p23.y, v, g);
        const double mg = (i >= j0 + g) ? mraw : 0.0;
        if (jb < 3) cur = __builtin_amdgcn_mfma_f64_16x16x4f64(-mg, mg, cur, 0, 0, 0);      // D -= M M^T (the last block has nothing behind it)
        cb[16 + lane] = mg;
        fl_set(S.fl + FL_C + kb, jb < 3 ? jb + 1 : 5, lane);         // (5: the last M block is out too -- the wave that forms the inverse reads it)
        cur[jb] = mg;
        rks[jb] = acc4{v.r0, v.r1, v.r2, v.r3};
        STRIPS_STAMP(32 + 4 * kb + jb);                              // (end of block jb)
    }
    // a pivot <= 0 (or NaN) makes its 1 / sqrt and everything behind it NaN: ONE test of the last one per chain; the column is looked up only then
    const double rl = rks[3][3];
    if (!(rl < 1.7e308)) {
        int bad = 15;
#pragma unroll
        for (int jb = 3; jb >= 0; --jb)
#pragma unroll
            for (int q = 3; q >= 0; --q)
                if (!(rks[jb][q] < 1.7e308)) bad = 4 * jb + q;
        if (lane == 0 && 16 * kb + bad < nvalid && *info == 0) *info = gidx0 + 16 * kb + bad + 1;      // LAPACK convention
    }
}
// A follower of block column kb: cur = D_{w,kb} -> L_{w,kb}; dg = this wave's own diagonal block D_ww.  It substitutes its own rows against the
// published pivot factors and applies, per 4-column block,
//   D_w^T -= M_d M_w^T   (A operand lane (m, k) = M_d[m][k]: the published block, lane for lane; B operand lane (n, k) = M_w[n][k]; register q of
//                         lane (n, g') receives row g' + 4 q of M_d against row n of M_w = the update of D_w[n][4 q + g']: the a image)
//   D_ww  -= M_w M_w^T   (both operands the same register; the trailing update of the wave's own diagonal block, four columns at a time: when
//                         the sixteenth column is in, the next diagonal wave starts its chain after ONE more MFMA)
// The flag poll and the factor reads of block jb + 1 are issued behind the MFMAs of block jb, in front of the exchange of the updated column
// block (which has to wait for them): a follower that has caught up is ~250 cycles behind the publication it waits for.
__device__ __forceinline__ void strips_follow(const CritLds& S, int kb, acc4& cur, acc4& dg, int wave, int lane, int* info) {
    const int i = lane & 15, g = lane >> 4;
    LD* own = S.own + 64 * wave;
    own[i * 4 + g] = cur[0];                                         // this wave's D[i][j0 + g], exchanged inside the wave
    __builtin_amdgcn_wave_barrier();
    d2v p01 = *(const LD2*)(own + i * 4), p23 = *(const LD2*)(own + i * 4 + 2);
    __builtin_amdgcn_sched_barrier(0);
    const LD* cb = S.cpub + kb * 4 * 80;
    d2v f0, f1, f2, f3, f4;
    double ng;
    // the flag word and what it guards in ONE LDS round trip: the reads are issued behind the flag read and LDS executes a wave's instructions in
    // order, so values read behind a flag that reads "set" are the published ones; otherwise the whole batch is repeated
    auto fetch = [&](int want) {
        int n = 0;
        for (;;) {
            const int fv = *(S.fl + FL_C + kb);
            asm volatile("" ::: "memory");
            f0 = *(const LD2*)(cb + 0); f1 = *(const LD2*)(cb + 2); f2 = *(const LD2*)(cb + 4); f3 = *(const LD2*)(cb + 6); f4 = *(const LD2*)(cb + 8);
            ng = cb[16 + lane];
            asm volatile("" ::: "memory");
            if (fv >= want || ++n > (1 << 22)) break;
#if POTRF_SPIN_SLEEP
            __builtin_amdgcn_s_sleep(POTRF_SPIN_SLEEP);
#endif
        }
    };
    fetch(1);
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
#ifdef POTRF_DEBUG
        if (kb == 1 && wave == 2) { const int gidx0 = S.dbg_gidx0; STRIPS_STAMP(16 + jb); }      // (factors of block jb read)
#endif
        Piv4 v;
        v.r0 = f0.x; v.r1 = f0.y; v.r2 = f1.x; v.r3 = f1.y; v.l10 = f2.x; v.l20 = f2.y; v.l30 = f3.x; v.l21 = f3.y; v.l31 = f4.x; v.l32 = f4.y;
        const double mw = subst4(p01.x, p01.y, p23.x, p23.y, v, g);  // M_w[i][g]
        if (jb < 3) cur = __builtin_amdgcn_mfma_f64_16x16x4f64(-ng, mw, cur, 0, 0, 0);
        dg = __builtin_amdgcn_mfma_f64_16x16x4f64(-mw, mw, dg, 0, 0, 0);
        if (jb < 3) {
            cb += 80;
            fetch(jb + 2);
            __builtin_amdgcn_sched_barrier(0);
        }
        cur[jb] = mw;
        if (jb < 3) {
            own[i * 4 + g] = cur[jb + 1];
            __builtin_amdgcn_wave_barrier();
            p01 = *(const LD2*)(own + i * 4); p23 = *(const LD2*)(own + i * 4 + 2);
        }
#ifdef POTRF_DEBUG
        if (kb == 1 && wave == 2) { const int gidx0 = S.dbg_gidx0; STRIPS_STAMP(20 + jb); }      // (block jb done)
#endif
    }
}
// The inverse of the diagonal block of column kb, formed by an IDLE wave one 4-column block behind the diagonal wave (round 5 ran this
// forward elimination of the identity inside the chain; as a pass of its own behind the last chain it was 2.8k cycles of the tile's tail):
// Y' -= (M diag(1 / L_cc), strictly below the diagonal) Z per block, M and the pivot factors as the diagonal wave published them;
// returns x[t] = X[4 t + g][i], the MFMA result layout.
__device__ __forceinline__ acc4 strips_invfollow(const CritLds& S, int kb, int wave, int lane, int* info) {
    const int i = lane & 15, g = lane >> 4;
    LD* own = S.own + 64 * wave;
    acc4 yt, rrx;
#pragma unroll
    for (int t = 0; t < 4; ++t) yt[t] = (4 * t + g == i) ? 1.0 : 0.0;
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
        const int j0 = 4 * jb;
        own[g * 16 + i] = yt[jb];                                    // Y'[j0 + g][i]
        __builtin_amdgcn_wave_barrier();
        const double y0 = own[0 * 16 + i], y1 = own[1 * 16 + i], y2 = own[2 * 16 + i], y3 = own[3 * 16 + i];
        __builtin_amdgcn_sched_barrier(0);
        const LD* cb = S.cpub + (kb * 4 + jb) * 80;
        fl_wait(S.fl + FL_C + kb, jb < 3 ? jb + 1 : 5, info);
        const d2v f0 = *(const LD2*)(cb + 0), f1 = *(const LD2*)(cb + 2), f2 = *(const LD2*)(cb + 4), f3 = *(const LD2*)(cb + 6), f4 = *(const LD2*)(cb + 8);
        const double mgv = cb[16 + lane];                            // M[i][g] = L[i][j0 + g] (zero above the diagonal)
        const double r0 = f0.x, r1 = f0.y, r2 = f1.x, r3 = f1.y;
        const double w10 = f2.x * r0, w20 = f2.y * r0, w30 = f3.x * r0, w21 = f3.y * r1, w31 = f4.x * r1, w32 = f4.y * r2;
        const double z1 = fma(-w10, y0, y1);
        const double z2 = fma(-w21, z1, fma(-w20, y0, y2));
        const double z3 = fma(-w32, z2, fma(-w31, z1, fma(-w30, y0, y3)));
        asm volatile("" :: "v"(z1), "v"(z2), "v"(z3));
        const double zg = (g == 0) ? y0 : ((g == 1) ? z1 : ((g == 2) ? z2 : z3));
        const double rg = (g == 0) ? r0 : ((g == 1) ? r1 : ((g == 2) ? r2 : r3));
        const double sg = (i > j0 + g) ? mgv * rg : 0.0;             // L[i][j0+g] / L[j0+g][j0+g], strictly below the diagonal
        yt = __builtin_amdgcn_mfma_f64_16x16x4f64(-sg, zg, yt, 0, 0, 0);
        rrx[jb] = rg;
    }
    acc4 x;
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = (i > 4 * t + g) ? 0.0 : yt[t] * rrx[t];
    return x;
}
// X_ww = L_ww^-1 from the register image of L_ww (a[t] = L[i][4 t + g], zero above the diagonal; rr[t] = 1 / L_cc, c = 4 t + g):
// forward elimination of the identity with unscaled rows, four rows per exchange (the Y' half of round 5's one-wave chain); returns
// x[t] = X[4 t + g][i], the MFMA result layout
__device__ __forceinline__ acc4 invert16_regs(LD* own, const acc4& a, const acc4& rr, int lane) {
    const int i = lane & 15, g = lane >> 4;
    acc4 yt;
#pragma unroll
    for (int t = 0; t < 4; ++t) yt[t] = (4 * t + g == i) ? 1.0 : 0.0;
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
        const int j0 = 4 * jb;
        own[g * 16 + i] = yt[jb];                                    // Y'[j0 + g][i]
        __builtin_amdgcn_wave_barrier();
        const double y0 = own[0 * 16 + i], y1 = own[1 * 16 + i], y2 = own[2 * 16 + i], y3 = own[3 * 16 + i];
        __builtin_amdgcn_wave_barrier();
        // L[j0 + r][j0 + c] sits in a[jb] of lane (i = j0 + r, g = c); 1 / L_cc of column j0 + k in rr[jb] of lane (., g = k)
        const double l10 = readlane_f64(a[jb], j0 + 1), l20 = readlane_f64(a[jb], j0 + 2), l30 = readlane_f64(a[jb], j0 + 3);
        const double l21 = readlane_f64(a[jb], j0 + 2 + 16), l31 = readlane_f64(a[jb], j0 + 3 + 16), l32 = readlane_f64(a[jb], j0 + 3 + 32);
        const double r0 = readlane_f64(rr[jb], 0), r1 = readlane_f64(rr[jb], 16), r2 = readlane_f64(rr[jb], 32);
        const double w10 = l10 * r0, w20 = l20 * r0, w30 = l30 * r0, w21 = l21 * r1, w31 = l31 * r1, w32 = l32 * r2;
        const double z1 = fma(-w10, y0, y1);
        const double z2 = fma(-w21, z1, fma(-w20, y0, y2));
        const double z3 = fma(-w32, z2, fma(-w31, z1, fma(-w30, y0, y3)));
        const double zg = (g == 0) ? y0 : ((g == 1) ? z1 : ((g == 2) ? z2 : z3));
        const double sg = (i > j0 + g) ? a[jb] * rr[jb] : 0.0;       // L[i][j0+g] / L[j0+g][j0+g], strictly below the diagonal
        yt = __builtin_amdgcn_mfma_f64_16x16x4f64(-sg, zg, yt, 0, 0, 0);
    }
    acc4 x;
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = (i > 4 * t + g) ? 0.0 : yt[t] * rr[t];
    return x;
}
// block (r, c) of X from its result-layout registers: LDS image [row][XB] and the 64 x 64 row-major tile in global memory
__device__ __forceinline__ void put_x(const CritLds& S, double* __restrict__ Xg, int r, int c, const acc4& x, int lane) {
    const int i = lane & 15, g = lane >> 4;
    LD* b = S.xs + xblk(r, c);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        b[(g + 4 * q) * XB + i] = x[q];
        Xg[(16 * r + g + 4 * q) * 64 + 16 * c + i] = x[q];
    }
    fl_set(S.fl + FL_X + 4 * r + c, 1, lane);
}
// one block column: the diagonal wave factors, the waves below follow, publish their panel block and update their trailing blocks
// (kb is a run-time value: one copy of the code; the strip's blocks are read and written as WHOLE vectors under wave-uniform branches --
// element writes into an array of vectors keep it in scratch)
__device__ __forceinline__ void strips_step(const CritLds& S, int kb, acc4 (&a)[4], acc4 (&rks)[4], int wave, int lane, int* info, int gidx0,
                                            int nvalid) {
    if (wave < kb) return;
    acc4 cur = a[0];
    if (kb == 1) cur = a[1];
    if (kb == 2) cur = a[2];
    if (kb == 3) cur = a[3];
    if (wave == kb) {
        STRIPS_STAMP(48 + kb);                                       // (this chain starts)
        strips_diag(S, kb, cur, rks, lane, info, gidx0, nvalid);
        STRIPS_STAMP(12 + kb);
    } else {
        acc4 dg = (wave == 1) ? a[1] : ((wave == 2) ? a[2] : a[3]);  // this wave's own diagonal block
        strips_follow(S, kb, cur, dg, wave, lane, info);
        if (wave == 1) a[1] = dg;
        else if (wave == 2) a[2] = dg;
        else a[3] = dg;
        if (wave == kb + 1) STRIPS_STAMP(52 + kb);                   // (the next diagonal wave has its panel block and its updated diagonal block)
        if (kb == 0) {                                               // lpub lives in the P tile: every wave must have left the update phase
            typedef int __attribute__((ext_vector_type(4))) i4v;
            typedef __attribute__((address_space(3))) volatile i4v LVI4;
            int n = 0;
            for (;;) {                                               // (the four FL_P words in one read)
                const i4v pd = *(LVI4*)(S.fl + FL_P);
                if ((pd.x & pd.y & pd.z & pd.w) != 0 || ++n > (1 << 22)) break;
            }
            asm volatile("" ::: "memory");
        }
        LD* lp = S.lpub + lblk(wave, kb);
#pragma unroll
        for (int t = 0; t < 4; ++t) lp[t * 64 + lane] = cur[t];
        fl_set(S.fl + FL_L + 4 * wave + kb, 1, lane);
        if (kb == 1 && wave == 2) STRIPS_STAMP(24);                  // (panel block published)
        // the blocks between: D_{w,cb} -= L_{w,kb} L_{cb,kb}^T for kb < cb < wave, in the a image: A operand = L_{cb,kb} (published image), B
        // operand = the own L_{w,kb}; two accumulators per block (dependent fp64 MFMAs wait out their latency)
#pragma unroll
        for (int cb = 1; cb < 3; ++cb) {
            if (cb <= kb || cb >= wave) continue;
            fl_wait(S.fl + FL_L + 4 * cb + kb, 1, info);
            const LD* lq = S.lpub + lblk(cb, kb);
            acc4 d0 = a[cb], d1 = acc4{0, 0, 0, 0};
            d0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lq[0 * 64 + lane], -cur[0], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f64_16x16x4f64(lq[1 * 64 + lane], -cur[1], d1, 0, 0, 0);
            d0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lq[2 * 64 + lane], -cur[2], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f64_16x16x4f64(lq[3 * 64 + lane], -cur[3], d1, 0, 0, 0);
            a[cb] = d0 + d1;
        }
    }
    if (kb == 0) a[0] = cur;
    else if (kb == 1) a[1] = cur;
    else if (kb == 2) a[2] = cur;
    else a[3] = cur;
}
// the W blocks (mb >= nb) a wave accumulates: rows of X at or below its own only (wave v's blocks have mb >= v)
__device__ __forceinline__ void w_block(int wave, int s, int& mb, int& nb) {
    //  wave 0: (0,0) (1,0) (3,0)    wave 1: (1,1) (2,0) (3,1)    wave 2: (2,1) (2,2)    wave 3: (3,2) (3,3)
    mb = -1; nb = 0;
    if (wave == 0) { mb = (s == 0) ? 0 : ((s == 1) ? 1 : 3); nb = 0; }
    else if (wave == 1) { mb = (s == 0) ? 1 : ((s == 1) ? 2 : 3); nb = (s == 1) ? 0 : 1; }
    else if (wave == 2) { if (s < 2) { mb = 2; nb = 1 + s; } }
    else { if (s < 2) { mb = 3; nb = 2 + s; } }
}
// The whole tile: a[cb] (cb <= wave) = this wave's strip of the updated diagonal tile (identity padding of a ragged tile), 256 threads.
// Ag: the tile's place in the matrix (lower triangle of its nvalid valid rows stored), Xg / Wg: X = L^-1 and W = X^T X, 64 x 64 each.
__device__ __forceinline__ void factor64_strips(const CritLds& S, acc4 (&a)[4], int tid, int* info, int gidx0, int nvalid,
                                                double* __restrict__ Ag, int64_t lda, double* __restrict__ Xg, double* __restrict__ Wg) {
    const int lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    acc4 rks[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) rks[t] = acc4{1, 1, 1, 1};
    if (wave == 0) STRIPS_STAMP(8);
#pragma unroll 1
    for (int kb = 0; kb < 4; ++kb) strips_step(S, kb, a, rks, wave, lane, info, gidx0, nvalid);
    // ---- the rest of the tile's work, in the order of urgency for the waves that wait on it.  Wave 0 inverts its own diagonal block (nobody
    // is idle beside its chain); wave w < 3 forms the inverse of the NEXT diagonal block one 4-column block behind that chain.
    if (wave == 0) {
        acc4 rr;                                                  // rr[t] = 1 / L_cc of column c = 4 t + g
#pragma unroll
        for (int t = 0; t < 4; ++t) rr[t] = (g == 0) ? rks[t][0] : ((g == 1) ? rks[t][1] : ((g == 2) ? rks[t][2] : rks[t][3]));
        const acc4 xw = invert16_regs(S.own, a[0], rr, lane);
        put_x(S, Xg, 0, 0, xw, lane);
    }
    // the zero blocks of X to the right of this wave's diagonal block, and COLUMN block `wave` of L: the diagonal block from the registers,
    // the blocks below it from the images their waves published (those waves are busy with the next chains; wave 3 has only its own block,
    // stored at the very end)
    auto store_l = [&](acc4 lv, int rb, int cbk) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int r = 16 * rb + i, c = 16 * cbk + 4 * t + g;
            if (r < nvalid && c <= r) Ag[(int64_t)r * lda + c] = lv[t];
        }
    };
    if (wave < 3) {
#pragma unroll
        for (int c = 1; c < 4; ++c) {
            if (c <= wave) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) Xg[(16 * wave + g + 4 * q) * 64 + 16 * c + i] = 0.0;
        }
        // (the diagonal block picked under wave-uniform branches with compile-time block indices: a block picked at run time -- a select of
        //  references, or of the loaded vectors -- puts the whole array in memory)
        if (wave == 0) store_l(a[0], 0, 0);
        else if (wave == 1) store_l(a[1], 1, 1);
        else store_l(a[2], 2, 2);
#pragma unroll
        for (int r = 1; r < 4; ++r) {
            if (r <= wave) continue;
            fl_wait(S.fl + FL_L + 4 * r + wave, 1, info);
            const LD* lq = S.lpub + lblk(r, wave);
            acc4 lv;
#pragma unroll
            for (int t = 0; t < 4; ++t) lv[t] = lq[t * 64 + lane];
            store_l(lv, r, wave);
        }
        // T_{w+1,w} = L_{w+1,w} X_ww BEFORE the inverse of the next diagonal block is followed (both operands exist soon after this wave's own
        // chain; for wave 2 this is T_{3,2}: X_{3,2} then leaves four MFMAs after X_33, not 2k cycles)
        fl_wait(S.fl + FL_X + 5 * wave, 1, info);                    // X_ww (wave w - 1 formed it; wave 0 its own)
        fl_wait(S.fl + FL_L + 4 * (wave + 1) + wave, 1, info);
        acc4 tn0 = acc4{0, 0, 0, 0}, tn1 = acc4{0, 0, 0, 0};
        {
            const LD* lq = S.lpub + lblk(wave + 1, wave);
            const LD* xq = S.xs + xblk(wave, wave);
            tn0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lq[0 * 64 + lane], xq[(0 + g) * XB + i], tn0, 0, 0, 0);
            tn1 = __builtin_amdgcn_mfma_f64_16x16x4f64(lq[1 * 64 + lane], xq[(4 + g) * XB + i], tn1, 0, 0, 0);
            tn0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lq[2 * 64 + lane], xq[(8 + g) * XB + i], tn0, 0, 0, 0);
            tn1 = __builtin_amdgcn_mfma_f64_16x16x4f64(lq[3 * 64 + lane], xq[(12 + g) * XB + i], tn1, 0, 0, 0);
        }
        const acc4 Tn = tn0 + tn1;
        if (wave == 2) STRIPS_STAMP(58);                             // (T_{3,2} formed)
        const acc4 xn = strips_invfollow(S, wave + 1, wave, lane, info);
        put_x(S, Xg, wave + 1, wave + 1, xn, lane);
        if (wave == 2) STRIPS_STAMP(9);
        {   // X_{w+1,w} = -X_{w+1,w+1} Tn
            const LD* xr = S.xs + xblk(wave + 1, wave + 1);
            acc4 x0 = acc4{0, 0, 0, 0}, x1 = acc4{0, 0, 0, 0};
            x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(-xr[i * XB + 0 + g], Tn[0], x0, 0, 0, 0);
            x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(-xr[i * XB + 4 + g], Tn[1], x1, 0, 0, 0);
            x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(-xr[i * XB + 8 + g], Tn[2], x0, 0, 0, 0);
            x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(-xr[i * XB + 12 + g], Tn[3], x1, 0, 0, 0);
            put_x(S, Xg, wave + 1, wave, x0 + x1, lane);
            if (wave == 2) STRIPS_STAMP(57);                         // (X_{3,2} published)
        }
    }
    // ---- X_{r,w} for the rows below (what the other waves wait for): T_{r,c} = sum_{j = c}^{r-1} L_{r,j} X_{j,c} (A operand lane (m, k) =
    // L_{r,j}[m][4 t + k], the published register image; B operand lane (n, k) = X_{j,c}[4 t + k][n]), then X_{r,c} = -X_rr T (A operand lane
    // (m, k) = X_rr[m][4 t + k], B operand = register t of T: its result layout).  Rows 1, 2 in full; of row 3 first T only -- X_33 is the last
    // thing the tile produces, the blocks of W that do not need it come in between.
    acc4 wacc[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) wacc[s] = acc4{0, 0, 0, 0};
    auto w_row = [&](int r) {       // W_{mb,nb} += X_{r,mb}^T X_{r,nb} for this wave's blocks with mb <= r: ONE poll for the row (xflag[r][0..3] in one
                                    // read: a poll is an LDS round trip, ~100 cycles), the blocks' MFMAs interleaved (independent accumulators)
        typedef int __attribute__((ext_vector_type(4))) i4v;
        typedef __attribute__((address_space(3))) volatile i4v LVI4;
        int n = 0;
        for (;;) {
            const i4v xf = *(LVI4*)(S.fl + FL_X + 4 * r);
            const int have = (xf.x != 0) + (r >= 1 ? (xf.y != 0) : 1) + (r >= 2 ? (xf.z != 0) : 1) + (r >= 3 ? (xf.w != 0) : 1);
            if (have == 4 || ++n > (1 << 22)) break;
#if POTRF_SPIN_SLEEP
            __builtin_amdgcn_s_sleep(POTRF_SPIN_SLEEP);
#endif
        }
        asm volatile("" ::: "memory");
        double wa[3][4], wb[3][4];
        bool on[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            int mb, nb;
            w_block(wave, s, mb, nb);
            on[s] = mb >= 0 && mb <= r;
            const LD* xa = S.xs + xblk(r, on[s] ? mb : 0);
            const LD* xb = S.xs + xblk(r, on[s] ? nb : 0);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                wa[s][t] = xa[(4 * t + g) * XB + i];
                wb[s][t] = xb[(4 * t + g) * XB + i];
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (on[s]) wacc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[s][t], wb[s][t], wacc[s], 0, 0, 0);      // (wave-uniform)
    };
#pragma unroll
    for (int r = 2; r < 4; ++r) {
        if (r <= wave + 1) continue;                                 // (row wave + 1: above)
        const int c = wave;
        acc4 t0 = acc4{0, 0, 0, 0}, t1 = acc4{0, 0, 0, 0};
        {   // ONE poll for the panel blocks L_{r,c..r-1} (lflag[r][0..3] in one read); X_{j,c}, j > c, are this wave's own earlier rows
            typedef int __attribute__((ext_vector_type(4))) i4v;
            typedef __attribute__((address_space(3))) volatile i4v LVI4;
            int n = 0;
            for (;;) {
                const i4v lf = *(LVI4*)(S.fl + FL_L + 4 * r);
                const int have = ((c > 0) | (lf.x != 0)) + ((c > 1 || r <= 1) | (lf.y != 0)) + ((r <= 2) | (lf.z != 0));
                if (have == 3 || ++n > (1 << 22)) break;
            }
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j < c || j >= r) continue;
            const LD* lq = S.lpub + lblk(r, j);
            const LD* xq = S.xs + xblk(j, c);
            t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lq[0 * 64 + lane], xq[(0 + g) * XB + i], t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(lq[1 * 64 + lane], xq[(4 + g) * XB + i], t1, 0, 0, 0);
            t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lq[2 * 64 + lane], xq[(8 + g) * XB + i], t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(lq[3 * 64 + lane], xq[(12 + g) * XB + i], t1, 0, 0, 0);
        }
        const acc4 T = t0 + t1;
        if (r == 3) {
            if (wave == 0) STRIPS_STAMP(60);                         // (T_{3,0} formed)
            if (wave == 1) STRIPS_STAMP(59);
#pragma unroll
            for (int rr_ = 0; rr_ < 3; ++rr_) if (rr_ >= wave) w_row(rr_);      // (waves 0, 1: the rows of W that do not need X_33, while chain 3 runs)
        }
        fl_wait(S.fl + FL_X + 4 * r + r, 1, info);
        if (r == 3 && wave == 0) STRIPS_STAMP(61);                   // (X_33 seen)
        const LD* xr = S.xs + xblk(r, r);
        acc4 x0 = acc4{0, 0, 0, 0}, x1 = acc4{0, 0, 0, 0};
        x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(-xr[i * XB + 0 + g], T[0], x0, 0, 0, 0);
        x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(-xr[i * XB + 4 + g], T[1], x1, 0, 0, 0);
        x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(-xr[i * XB + 8 + g], T[2], x0, 0, 0, 0);
        x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(-xr[i * XB + 12 + g], T[3], x1, 0, 0, 0);
        put_x(S, Xg, r, c, x0 + x1, lane);
        if (r == 3 && wave == 0) STRIPS_STAMP(62);                   // (X_{3,0} published)
        if (r == 3 && wave == 1) STRIPS_STAMP(56);
    }
    if (wave == 2) w_row(2);
    if (wave == 3) STRIPS_STAMP(25);
    w_row(3);
    if (wave == 0) STRIPS_STAMP(63);                                 // (row 3 of W taken by wave 0)
    if (wave == 3) STRIPS_STAMP(26);                                 // (... by wave 3)
    if (wave == 3) STRIPS_STAMP(27);                                 // (wave 3: its W blocks accumulated)
    // W blocks -> the 64 x 64 tile, both triangles.  The mirrored block goes through LDS (the cpub words are free now: every reader of them is
    // behind the row-3 flags), so that its stores run along rows too -- stored from the registers, one instruction touched 64 cache lines and
    // the 12 of them were ~2k cycles at the very end of the critical workgroup
    LD* tw = S.cpub + 272 * wave;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        int mb, nb;
        w_block(wave, s, mb, nb);
        if (mb < 0) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = 16 * mb + g + 4 * q, nn = 16 * nb + i;
            Wg[m * 64 + nn] = wacc[s][q];
            tw[(g + 4 * q) * XB + i] = wacc[s][q];
        }
        __builtin_amdgcn_wave_barrier();
        if (mb != nb) {
#pragma unroll
            for (int q = 0; q < 4; ++q) Wg[(16 * nb + g + 4 * q) * 64 + 16 * mb + i] = tw[i * XB + g + 4 * q];
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (wave == 3) {
        const acc4 l33 = a[3];
        store_l(l33, 3, 3);
    }
    STRIPS_STAMP(28 + wave);                                         // this wave is done
#ifdef POTRF_DEBUG
    if (gidx0 == (POTRF_DEBUG_K + 1) * 64) {                         // the stamp words of this wave's slots -> chol_dbg (slots 8 .. 63; 0 .. 7 belong to CHOL_STAMP)
        __syncthreads();
        if (tid >= 8 && tid < 64) chol_dbg[tid] = S.dbg[tid];
    }
#endif
}

// The update phase for factor64_strips: as round 5's update (P = A X_k^T strip by strip, P back to LDS, D = C - P P^T), but EVERY wave's
// blocks come out in the a image: block (w, nb) as the transposed product  D^T = C^T - P_nb P_w^T  (A operand: P_nb out of LDS, B operand:
// the registers of U = P_w^T), C loaded in the a image.  k < 0: the first tile of the matrix, loaded as it is.
__device__ __forceinline__ void crit_strips_update(double (*S)[64][LDT], const double* __restrict__ A, int64_t lda, int n, int k,
                                                   const double* __restrict__ Xk, int tid, acc4 (&a)[4], LVI* fl
#ifdef POTRF_DEBUG
                                                   , unsigned long long* st_
#endif
                                                   ) {
    const int lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int i0 = (k + 1) * 64, nr = n - i0;
    if (tid < FL_N) fl[tid] = 0;
    // this strip's blocks of C in the a image (clamped addresses, masked below): requested BEHIND the operands of the first product
    // (loads return in order: in front of them they held up the LDS fill by 1.5k cycles)
    auto load_c = [&]() {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            if (nb > wave) { a[nb] = acc4{0, 0, 0, 0}; continue; }
            acc4 cv;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int gr = min(i0 + 16 * wave + i, n - 1), gc = min(i0 + 16 * nb + 4 * q + g, n - 1);
                cv[q] = A[(int64_t)gr * lda + gc];
            }
            a[nb] = cv;
        }
    };
    if (k >= 0) {
        const int k0 = k * 64;
        {
            double ra[16], rw[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {           // (rows past the matrix: clamped row index, zeroed on the way to LDS -- no branch per load)
                const int r = (tid >> 6) + 4 * u, c = tid & 63;
                rw[u] = Xk[r * 64 + c];
                ra[u] = A[(int64_t)min(i0 + r, n - 1) * lda + k0 + c];
            }
            load_c();
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int r = (tid >> 6) + 4 * u, c = tid & 63;
                S[0][r][c] = (i0 + r < n) ? ra[u] : 0.0;
                S[1][r][c] = rw[u];
            }
        }
        __syncthreads();
        CHOL_STAMP(1);
        // U = X_k A_w^T = P_w^T (X_k lower triangular: column block cb of P needs the k blocks 0 .. cb only)
        acc4 U[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) U[cb] = acc4{0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const int kq = 4 * ks + g;
            const double bop = S[0][16 * wave + i][kq];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                if (cb < (ks >> 2)) continue;
                U[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(S[1][16 * cb + i][kq], bop, U[cb], 0, 0, 0);
            }
        }
        CHOL_STAMP(4);
        __syncthreads();                 // X_k is dead: its tile becomes xs / cpub
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) S[0][16 * wave + i][16 * cb + 4 * q + g] = U[cb][q];
        __syncthreads();
        CHOL_STAMP(5);
        if (wave == 0) {                 // one block: two accumulators
            acc4 d1 = acc4{0, 0, 0, 0};
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double aop = S[0][i][16 * cb + 4 * q + g];
                    if (q & 1) d1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aop, -U[cb][q], d1, 0, 0, 0);
                    else a[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop, -U[cb][q], a[0], 0, 0, 0);
                }
            a[0] += d1;
        } else {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb) {
                        if (nb > wave) continue;
                        a[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(S[0][16 * nb + i][16 * cb + 4 * q + g], -U[cb][q], a[nb], 0, 0, 0);
                    }
        }
        CHOL_STAMP(7);
    } else {
        load_c();
        __syncthreads();                 // (the flag words are zero for every wave)
    }
    fl_set(fl + FL_P + wave, 1, lane);   // this wave is done with the P tile
    // identity padding of a ragged tile, zero above the diagonal
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        if (nb > wave) continue;
        acc4 mv = a[nb];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = 16 * wave + i, c = 16 * nb + 4 * q + g;
            const bool in = r < nr && c <= r;
            mv[q] = in ? mv[q] : ((r == c) ? 1.0 : 0.0);
        }
        a[nb] = mv;
    }
}

constexpr int POTRF_NW = 4;         // waves per workgroup of the step launches.  8 (each 64 x 64 tile product split 32 x 16 per wave) measured slower at M' = 3000 (1.78-1.93 vs 1.70 ms); at 600 5 % faster in round 2, 28 % slower on the round-4 kernel (0.319 vs 0.249 ms)
#ifndef POTRF_MINW
#define POTRF_MINW (POTRF_NW / 2)
#endif
#ifndef POTRF_PIPE_MIN_TILES
#define POTRF_PIPE_MIN_TILES 300    // launches with fewer tiles are bound by the critical workgroup anyway: they keep the two-per-CU kernel
#endif
#ifndef POTRF_PIPE_WGS
#define POTRF_PIPE_WGS 250          // workgroups of a PIPE launch (one per CU; the critical workgroup is one of them)
#endif
#ifndef POTRF_PIPE_MINW
#define POTRF_PIPE_MINW 1           // the PIPE instantiation: 101 KB of LDS, one workgroup per CU whatever the registers (asking for 2 here to get a
                                    // 256-register budget does not take: the compiler sees the LDS size and budgets for one wave per SIMD anyway)
#endif
// PIPE: three LDS tiles and up to 512 registers -- ONE workgroup per CU -- with the strips of both tile roles software-pipelined
// (strip_pipe above); strip_e: strip length of the ragged last tile row of the update role, which keeps the two-barrier strip loop
// (its tiles need clamped addresses) and must not be the launch's longest chain.
template <int NW, bool PIPE = false>
__global__ __launch_bounds__(64 * NW, PIPE ? POTRF_PIPE_MINW : POTRF_MINW) void chol_step_kernel(double* __restrict__ A, int64_t lda, int n, int k,
                                                           double* __restrict__ Xws, double* __restrict__ Wws,
                                                           int* __restrict__ info, double* __restrict__ Rw, int64_t ldr,
                                                           double* __restrict__ Yinv, int64_t ldy, int nA,
                                                           double* __restrict__ YinvT, int strip, int strip_e) {
    // TWO 64 x 64 LDS tiles (70 KB with the factorisation scratch): two workgroups share a CU, which halves the rounds
    // the ~1100 update / inverse tiles of a mid-chain launch need.  The second right operand of every tile waits in
    // registers while the first product runs.
    __shared__ double S[PIPE ? 3 : 2][64][LDT];
    __shared__ double Xd[16][17];
    __shared__ double colbuf[64];                  // the critical workgroup's flag words (CritLds::fl)
#ifdef POTRF_DEBUG
    __shared__ double rowbuf[64];                  // ... and its stamp words
#endif
    constexpr int WC = NW / 2, NJ = 8 / NW, NU = 64 / NW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave / WC, wc = wave % WC;
    const int b = blockIdx.x;
    TR_DECL;
    TR(0);
    if (b >= nA) {                                 // fused-inverse tiles (only launched with k >= 0 and Rw != nullptr)
#ifdef POTRF_TRACE
        chol_inverse_tile<NW, PIPE>(S, A, lda, n, k, b - nA, Xws, Wws, Rw, ldr, Yinv, ldy, (n + 63) / 64, YinvT, strip, trs_);
        TR_VAL(22, 2);
        TR_FLUSH;
#else
        chol_inverse_tile<NW, PIPE>(S, A, lda, n, k, b - nA, Xws, Wws, Rw, ldr, Yinv, ldy, (n + 63) / 64, YinvT, strip);
#endif
        return;
    }
    static_assert(NW == 4, "the critical workgroup's register-strip path is written for four waves");
    // Workgroup 0 is ALWAYS the critical workgroup and returns inside this block; k = -1 (the matrix's first tile) is launched with
    // one workgroup.  So everything below runs with b != 0 and k >= 0.
    if (b == 0) {
        CHOL_STAMP_DECL;
        CHOL_STAMP(0);
        acc4 a[4];
        CritLds cl;
        cl.xs = (LD*)&S[1][0][0];                  // (the X_k tile: dead after the first product of the update)
        cl.cpub = cl.xs + 10 * 16 * XB;
        cl.lpub = (LD*)&S[0][0][0];                // (the P tile: written only behind the FL_P flags)
        cl.own = (LD*)&Xd[0][0];
        cl.fl = (LVI*)colbuf;
#ifdef POTRF_DEBUG
        cl.dbg = (__attribute__((address_space(3))) unsigned long long*)rowbuf;
        if (tid < 64) cl.dbg[tid] = 0;
        cl.dbg_gidx0 = (k + 1) * 64;
#endif
        static_assert(10 * 16 * XB + 16 * 80 <= 64 * LDT && 4 * 272 <= 16 * 80 && 6 * 256 <= 64 * LDT && 4 * 64 <= 16 * 17 && FL_N * sizeof(int) <= 64 * sizeof(double),
                      "LDS views of the critical workgroup");
#ifdef POTRF_DEBUG
        crit_strips_update(S, A, lda, n, k, Xws + (size_t)(k < 0 ? 0 : k) * 4096, tid, a, cl.fl, st_);
        st_[6] = st_[5];
#else
        crit_strips_update(S, A, lda, n, k, Xws + (size_t)(k < 0 ? 0 : k) * 4096, tid, a, cl.fl);
#endif
        CHOL_STAMP(2);
        TR(1);
        const int kk = k + 1, r0 = kk * 64, nr = (n - r0 < 64) ? (n - r0) : 64;
        factor64_strips(cl, a, tid, info, r0, nr, A + (int64_t)r0 * lda + r0, lda, Xws + (size_t)kk * 4096, Wws + (size_t)kk * 4096);
        CHOL_STAMP(3);
        CHOL_STAMP_FLUSH;
        TR(2);
        TR_VAL(22, 0);
        TR_FLUSH;
        return;
    }
    // tile row ti holds ti + 1 update tiles, dealt to workgroups in strips of strip block columns (block 0: the diagonal tile
    // of row 0, alone: the critical workgroup)
    int ti = 0, first = 0;
    const int ntr = (n + 63) / 64 - (k + 1);        // tile rows of the trailing matrix; the last one may be ragged: strips of strip_e
    while (ti < ntr - 1 && first + (ti + strip) / strip <= b) { first += (ti + strip) / strip; ++ti; }
    if (ti == ntr - 1) strip = strip_e;
    int tj = (b - first) * strip;
    const int ncols = min(strip, ti + 1 - tj);
    const int i0 = (k + 1 + ti) * 64;
    int j0 = (k + 1 + tj) * 64;
    if constexpr (PIPE && NW == 4) {
        if (k >= 0 && b != 0 && i0 + 64 <= n) {        // interior tile row (its strip's columns lie left of it: inside too)
            const int k0 = k * 64;
            const double* Wk = Wws + (size_t)k * 4096;
            const int ml0 = wr * 32 + (lane >> 4), nl0 = wc * 32 + (lane & 15);
            const int64_t astep = (int64_t)4 * lda;
            double cs[3][2][2][4];
            double* const Cg = A + (int64_t)(i0 + ml0) * lda + j0 + nl0;
            const double* const Bg = A + (int64_t)j0 * lda + k0;
            {   // the operands of T first; C_0 and B_0 (LDS-DMA, issued LAST: the compiler's count for A_ik / W_k then leaves them
                // in flight) are only waited for behind the T product (strip_pipe)
                double ra[16], rw[16];
                const double* pa = A + (int64_t)(i0 + (tid >> 6)) * lda + k0 + (tid & 63);
#pragma unroll
                for (int u = 0; u < 16; ++u) { ra[u] = pa[u * astep]; rw[u] = Wk[((tid >> 6) + 4 * u) * 64 + (tid & 63)]; }
#pragma unroll
                for (int u = 0; u < 16; ++u) { S[0][(tid >> 6) + 4 * u][tid & 63] = ra[u]; S[1][(tid >> 6) + 4 * u][tid & 63] = rw[u]; }
            }
            __syncthreads();
            pipe_dma_tile(S[2], Bg, lda);                  // B_0, C_0 requested behind the barrier: in flight under the T product
#pragma unroll
            for (int t = 0; t < 8; ++t)
#pragma unroll
                for (int j = 0; j < 2; ++j) cs[0][t >> 2][j][t & 3] = Cg[t * astep + j * 16];
            acc4 acc[2][2];
            TR(1);
            tile_product<true, 4>(S[0], S[1], lane, wr, wc, acc);            // T = A_ik W_k (W symmetric: [n][k] == [k][n])
#ifdef POTRF_TRACE
            strip_pipe<true>(S, Bg, lda, (int64_t)64 * lda, Cg, lda, ncols, false, ti == tj + ncols - 1, acc, cs, k == POTRF_DEBUG_K ? trs_ : nullptr);
            TR_VAL(20, (ncols << 16) | ti);
            TR_VAL(22, 1);
            TR_FLUSH;
#else
            strip_pipe<true>(S, Bg, lda, (int64_t)64 * lda, Cg, lda, ncols, false, ti == tj + ncols - 1, acc, cs);
#endif
            return;
        }
    }
    if (k >= 0) {
        const int k0 = k * 64;
        const double* Wk = Wws + (size_t)k * 4096;
        double cv[2][NJ][4];    // C tile, requested behind the operand loads (clamped addresses: no predicated load -> wait -> store chains)
        double rb[NU];         // A_jk, parked until T = A_ik W_k is in LDS
        {   // all 48 + 16 loads of a thread in flight at once (a rolled loop pays the global latency 16 times)
            double ra[NU], rw[NU];
            const int64_t alast = (int64_t)(n - 1) * lda, astep = (int64_t)NW * lda;
            const int64_t arow0 = (int64_t)(i0 + (tid >> 6)) * lda, brow0 = (int64_t)(j0 + (tid >> 6)) * lda;
#pragma unroll
            for (int u = 0; u < NU; ++u) {       // (rows past the matrix: clamped to the last row, zeroed on the way to LDS)
                const int r = (tid >> 6) + NW * u, c = tid & 63;
                ra[u] = A[((i0 + r < n) ? arow0 + u * astep : alast) + k0 + c];
                rw[u] = Wk[r * 64 + c];
            }
#pragma unroll
            for (int u = 0; u < NU; ++u) {       // (behind the operands of T = A_ik W_k: the first LDS fill waits for those only)
                const int r = (tid >> 6) + NW * u, c = tid & 63;
                rb[u] = A[((j0 + r < n) ? brow0 + u * astep : alast) + k0 + c];
            }
            const int m0 = i0 + wr * 32 + (lane >> 4);
            const int64_t crow0 = (int64_t)m0 * lda;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int nn = min(j0 + wc * (16 * NJ) + j * 16 + (lane & 15), n - 1);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int dm = i * 16 + 4 * q;
                        cv[i][j][q] = A[((m0 + dm < n) ? crow0 + (int64_t)dm * lda : alast) + nn];
                    }
                }
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int r = (tid >> 6) + NW * u, c = tid & 63;
                S[0][r][c] = (i0 + r < n) ? ra[u] : 0.0;
                S[1][r][c] = rw[u];
            }
        }
        __syncthreads();
        TR(1);
        acc4 acc[2][NJ];
        tile_product<true, NW>(S[0], S[1], lane, wr, wc, acc);          // T = A_ik W_k   (W symmetric: [n][k] == [k][n])
        TR(2);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {       // -T to LDS, the accumulators restart from the C tile: the second product leaves C - T A_jk^T
                    S[0][wr * 32 + i * 16 + (lane >> 4) + 4 * q][wc * (16 * NJ) + j * 16 + (lane & 15)] = -acc[i][j][q];
                    acc[i][j][q] = cv[i][j][q];
                }
        const int ml0 = wr * 32 + (lane >> 4), nl0 = wc * (16 * NJ) + (lane & 15);
#pragma unroll 1
        for (int cc = 0; cc < ncols; ++cc) {         // the strip: -T stays in S[0]; A_jk and the C tile change per block column
            if (cc > 0) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[i][j][q] = cv[i][j][q];
            }
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int r = (tid >> 6) + NW * u, c = tid & 63;
                S[1][r][c] = (j0 + r < n) ? rb[u] : 0.0;
            }
            __syncthreads();
            if (cc < 5) TR(3 + 3 * cc);
            const bool diag = ti == tj;
            const int jcur = j0;
            if (cc + 1 < ncols) {                    // next block column of the strip: requested now, consumed after this product
                ++tj; j0 += 64;
                const int64_t alast = (int64_t)(n - 1) * lda, astep = (int64_t)NW * lda;
                const int64_t brow0 = (int64_t)(j0 + (tid >> 6)) * lda;
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int r = (tid >> 6) + NW * u, c = tid & 63;
                    rb[u] = A[((j0 + r < n) ? brow0 + u * astep : alast) + k * 64 + c];
                }
                const int m0 = i0 + ml0;
                const int64_t crow0 = (int64_t)m0 * lda;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const int nn = min(j0 + nl0 + j * 16, n - 1);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int dm = i * 16 + 4 * q;
                            cv[i][j][q] = A[((m0 + dm < n) ? crow0 + (int64_t)dm * lda : alast) + nn];
                        }
                    }
            }
            tile_product<true, NW, true>(S[0], S[1], lane, wr, wc, acc);    // C - T A_jk^T
            if (cc < 5) TR(4 + 3 * cc);
            double* const cdst = A + (int64_t)(i0 + ml0) * lda + jcur + nl0;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int ml = ml0 + i * 16 + 4 * q, nl = nl0 + j * 16;
                        if (i0 + ml < n && jcur + nl < n && !(diag && nl > ml))
                            cdst[(int64_t)(i * 16 + 4 * q) * lda + j * 16] = acc[i][j][q];
                    }
            if (cc < 5) TR(5 + 3 * cc);
            if (cc + 1 < ncols) __syncthreads();     // every wave is done reading A_jk out of S[1]
        }
        TR_VAL(20, (ncols << 16) | ti);
        TR_VAL(22, 1);
        TR_FLUSH;
    }
}

// the last block row of L^-1 (its X is produced by the last step launch): Y_kj = X_k R_kj, j <= k = nblk - 1
__device__ __forceinline__ void chol_yrow_tile(double (*S)[64][LDT], int b, const double* __restrict__ A, int64_t lda, int n,
                                               const double* __restrict__ Xws, const double* __restrict__ Wws,
                                               double* __restrict__ Rw, int64_t ldr, double* __restrict__ Yinv, int64_t ldy,
                                               double* __restrict__ YinvT) {
    const int nblk = (n + 63) / 64, k = nblk - 1;
    chol_inverse_tile(S, A, lda, n, k, (nblk - (k + 1)) * (k + 1) + b, Xws, Wws, Rw, ldr, Yinv, ldy, nblk, YinvT);
}

// all solved panels in one launch:  L_ik = A_ik X_k^T  (i > k), in place, one 64 x 64 tile per workgroup
// (the same launch carries the last block row of L^-1 in its first ny workgroups: the two are independent, and at M' = 600 a
//  launch of its own costs as much as either of them)
__global__ __launch_bounds__(256) void chol_panels_kernel(double* __restrict__ A, int64_t lda, int n,
                                                          const double* __restrict__ Xws, const double* __restrict__ Wws,
                                                          double* __restrict__ Rw, int64_t ldr, double* __restrict__ Yinv,
                                                          int64_t ldy, double* __restrict__ YinvT, int ny) {
    __shared__ double S[2][64][LDT];
    if ((int)blockIdx.x < ny) {
        chol_yrow_tile(S, blockIdx.x, A, lda, n, Xws, Wws, Rw, ldr, Yinv, ldy, YinvT);
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int b = blockIdx.x - ny;
    int ti = (int)((sqrtf(8.f * (float)b + 1.f) - 1.f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= b) ++ti;
    while (ti * (ti + 1) / 2 > b) --ti;
    const int k = b - ti * (ti + 1) / 2, i0 = (ti + 1) * 64, k0 = k * 64;     // strict lower: block row ti + 1, column k
    const double* Xk = Xws + (size_t)k * 4096;
    {
        double ra[16], rx[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = (tid >> 6) + 4 * u, c = tid & 63;
            ra[u] = A[(int64_t)min(i0 + r, n - 1) * lda + k0 + c];
            rx[u] = Xk[r * 64 + c];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            S[0][(tid >> 6) + 4 * u][tid & 63] = (i0 + (tid >> 6) + 4 * u < n) ? ra[u] : 0.0;
            S[1][(tid >> 6) + 4 * u][tid & 63] = rx[u];
        }
    }
    __syncthreads();
    acc4 acc[2][2];
    tile_product<true>(S[0], S[1], lane, wr, wc, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = i0 + wr * 32 + i * 16 + (lane >> 4) + 4 * q, c = k0 + wc * 32 + j * 16 + (lane & 15);
                if (m < n) A[(int64_t)m * lda + c] = acc[i][j][q];
            }
}

}  // namespace

size_t potrf_blocked_workspace_bytes(int n) {
    const size_t nblk = (size_t)cdiv(n, NBC);
    // X_k, W_k blocks + the working matrix R of the fused inverse (padded to whole blocks)
    return sizeof(double) * (2 * nblk * NBC * NBC + nblk * NBC * nblk * NBC);
}

// one fused launch per block column + one batched panel launch (see chol_step_kernel).  Yinv != nullptr: also L^-1
// (lower triangle, leading dimension ldy) by the fused forward elimination, and (YinvT != nullptr) its transpose with the
// same leading dimension.
int launch_potrf_blocked(hipStream_t st, double* A, int n, int64_t lda, int* info, double* ws, double* Yinv, int64_t ldy,
                         double* YinvT, bool info_zeroed, const PotrfHook* hooks, int nhooks, int pipe_from) {
    if (!info_zeroed) {
        hipError_t e = hipMemsetAsync(info, 0, sizeof(int), st);
        if (e != hipSuccess) return 1000 + (int)e;
    }
    const int nblk = cdiv(n, NBC);
    double* Xws = ws;
    double* Wws = ws + (size_t)nblk * NBC * NBC;
    double* Rw = Yinv ? Wws + (size_t)nblk * NBC * NBC : nullptr;
    const int64_t ldr = (int64_t)nblk * NBC;
    for (int k = -1; k < nblk - 1; ++k) {
        const int nt = nblk - (k + 1);
        const int tiles = (k < 0) ? 1 : nt * (nt + 1) / 2 + (Yinv ? nt * (k + 1) + (k + 1) : 0);
        const int strip = tiles > POTRF_STRIP_T6 ? POTRF_STRIP_V6 : (tiles > POTRF_STRIP_T4 ? POTRF_STRIP_V4 : (tiles > POTRF_STRIP_T2 ? POTRF_STRIP_V2 : 1));
        int nA = 1;                                  // update tiles, in strips of `strip` block columns per tile row
        if (k >= 0) {
            nA = 0;
            for (int ti = 0; ti < nt; ++ti) nA += (ti + strip) / strip;
        }
        const int nI = (k >= 0 && Yinv) ? nt * ((k + strip) / strip) + (k + 1) : 0;     // R strips + Y tiles
        if (k >= 0 && k >= pipe_from && tiles > POTRF_PIPE_MIN_TILES && lda % 2 == 0 && ((uintptr_t)A % 16) == 0 &&
            (!Rw || ((uintptr_t)Rw % 16) == 0)) {      // (the B tiles arrive by 16-byte LDS-DMA pieces: base and row stride 16-byte aligned)
            // one workgroup per CU: the shortest strips that keep the launch within one round of the 256 CUs (the pipelined strip
            // costs ~13k cycles + 4.7k per column; a second round would cost a whole strip)
            int sp = 2, nAp = 0, nIp = 0, se = 2;
            for (;; ++sp) {
                se = (n % 64 == 0) ? sp : (sp < 2 ? sp : 2);           // the ragged last tile row keeps the two-barrier loop: short strips
                nAp = 0;
                for (int ti = 0; ti < nt - 1; ++ti) nAp += (ti + sp) / sp;
                nAp += (nt - 1 + se) / se;
                nIp = Yinv ? nt * ((k + sp) / sp) + (k + 1) : 0;
                if (nAp + nIp <= POTRF_PIPE_WGS || sp >= 12) break;
            }
            hipLaunchKernelGGL((chol_step_kernel<4, true>), dim3(nAp + nIp), dim3(256), 0, st, A, lda, n, k, Xws, Wws, info, Rw, ldr, Yinv,
                               ldy, nAp, YinvT, sp, se);
        } else
        hipLaunchKernelGGL((chol_step_kernel<POTRF_NW, false>), dim3(nA + nI), dim3(64 * POTRF_NW), 0, st, A, lda, n, k, Xws, Wws, info, Rw,
                           ldr, Yinv, ldy, nA, YinvT, strip, strip);
        DSVGP_LAUNCH_CHECK();
        for (int h = 0; h < nhooks; ++h)
            if (hooks[h].after_k == k) {
                const hipError_t e = hipEventRecord(hooks[h].ev, st);
                if (e != hipSuccess) return 1000 + (int)e;
            }
    }
    const int ny = Yinv ? nblk : 0, npan = nblk * (nblk - 1) / 2;
    if (ny + npan > 0) {
        hipLaunchKernelGGL(chol_panels_kernel, dim3(ny + npan), dim3(256), 0, st, A, lda, n, (const double*)Xws, (const double*)Wws, Rw,
                           ldr, Yinv, ldy, YinvT, ny);
        DSVGP_LAUNCH_CHECK();
    }
    return 0;
}

#ifdef POTRF_TRACE
extern "C" int dsvgp_debug_potrf_trace(unsigned long long* out, int nwg) {
    if (nwg > TR_MAXWG) nwg = TR_MAXWG;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(chol_trace), sizeof(unsigned long long) * (size_t)nwg * TR_SLOTS);
}
#endif
#ifdef POTRF_DEBUG
extern "C" int dsvgp_debug_potrf_clock(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(chol_dbg), sizeof(unsigned long long) * 64);
}

#endif
