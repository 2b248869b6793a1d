// The tiled kernel assembly shared by every covariance family (assemble_wide.hip: RBF, assemble_matern.hip: Matern-5/2): ONE forward
// kernel and ONE Tbar kernel, templated on a `Radial` policy and on the output / upstream element type, their launchers, and the one plan
// of tiles, grid, dynamic LDS and backward workspace.  The kernel bodies own the LDS carve-up, the staging of G / self1 / self2, the K loop
// (wide_T), the index arithmetic, the output walk with the jitter, the task loops of the row and column passes, the TB store and the
// fixed-order reduction into partials[2 bid .. + 1]; a policy owns the radial algebra alone.  With T = P1 P2^T and, per point pair (i, j),
//     nn = max(self1[i0] + self2[j0] - 2 T[i0,j0], 0)     u_a = self1[ia] - T[ia,j0]     w_b = T[i0,jb] - self2[jb]     t_ab = T[ia,jb]
// a policy (every member __device__ __forceinline__) provides
//     Hyp(hyp)                         the hyp entries it reads (the forward builds it in front of the K loop, which hides the scalar loads)
//     Radial(Hyp)                      what it derives from them
//     NPAIR                            pair arrays the forward keeps per point pair, [NPAIR][Rr Rc] in LDS (none is touched at 1 x 1 micro-blocks)
//     pair(kk, np, nn)                 forward pair stage: kk[i np], i < NPAIR
//     pair_value(kk, np)               the pair value every entry of the micro-block needs (loaded in front of t, u, w)
//     entry(k, kk, np, a, b, t, u, w)  forward value of entry (a, b) of a micro-block that has derivative rows or columns
//     value(nn)                        forward value at 1 x 1 micro-blocks
//     Row row(ssum, nn)                Tbar row pass: the radial factors of one task (ssum = self1[i0] + self2[j0])
//     row_value(R, g0, first, ps, kk, acc)              a == 0: first = sum_b G_0b w_b; writes the strip's share ps, the pair value kk
//     row_deriv(R, gr, tr, t0, s2, p2, g0, u, acc)      a >= 1: Tbar_ab and Tbar_a0 in place of G's row strip gr; returns the strip's share
//     col_value(k, kbar, s1v, s2c, tc, acc)             column pass, b == 0: Tbar_00 from kbar = the sum of the strips' shares
//     col_deriv(k, p1, s1v, s2c, tc, b, g0c, us, Rc, acc)   b >= 1: Tbar_0b
//     NSUM, partials(acc, ps)          how many of the two partial slots it fills, and with what (the others hold 0)
//     F1_0                             f1(0), the constant of the prior diagonal on ARD packs (kernel_diag_kernel, at the end): 1 RBF, 5/3 Matern
// acc[2] are a thread's two running sums over its tasks of both passes.  A policy's floating-point expressions, their operand order and
// their __builtin_fmaf calls are part of the results (exact zeros on K_ZZ's diagonal micro-blocks, K_ZZ's exact symmetry): a change there
// shows in tools/tiled_ab.py, which compares two builds bit for bit.
//
// Tiles (tile_plan): one 256-thread workgroup per tile of Rr x Rc micro-blocks, Tr = Rr q1 <= 96 rows by Tc = Rc q2 <= 96 columns,
//     Rc = 96 / q2,   Rr = max(1, (96 / q1) / 2),   Trp / Tcp = Tr / Tc padded to 16,
// the rectangular backward alone caps the column tile, Rc = min(96 / q2, 9984 / (2 Tr + Rr)) (assemble_wide.hip, header comment).
#pragma once
#include "common.h"
#include "wide_product.h"

#include <climits>

// ---- the plan -----------------------------------------------------------------------------------
struct TilePlan {
    int q1, q2, n1q, n2q, K4, DP, NP;       // row / column period, interleaved rows / columns, packed widths
    int Rr, Rc, Tr, Tc, gx, gy;             // micro-blocks per tile, tile, grid
    size_t lds_fwd, lds_tbar;               // dynamic LDS: the forward with ONE pair array (fwd_tiles_lds adds a family's others), the Tbar launch
    // the backward's two launches and its workspace, slab[ns][n1q][NP] | partials[nparts][2] | TB[n1q][n2q], floats
    int ns, kper, nparts;                   // the contraction's cut of the n2q range: ns pieces of kper columns; Tbar workgroups
    size_t slab_f, part_f, tb_f, bytes;
};
// one Tbar launch on a plan: Tbar tiles to TB, the tiles' partial sums to partials (launch_tbar_tiles<Radial>)
using TbarLauncher = int (*)(hipStream_t st, const TilePlan& t, const void* G, int64_t ldg, int g_is_double, const float* P1,
                             const float* self1, const float* P2, const float* self2, const float* hyp, float* TB, float* partials);
// assemble_wide.hip: the RBF family's Tbar launcher; the backward's launches 1 (the family's Tbar tiles) and 2 (the contraction) on plan t
// inside `workspace` (t.bytes), for a caller that brings its own points reduction
int launch_kernel_bwd_tbar_rbf(hipStream_t st, const TilePlan& t, const void* G, int64_t ldg, int g_is_double, const float* P1,
                               const float* self1, const float* P2, const float* self2, const float* hyp, float* TB, float* partials);
int launch_kernel_bwd_tiles(hipStream_t st, TbarLauncher tbar, const TilePlan& t, const void* G, int64_t ldg, int g_is_double,
                            const float* P1, const float* self1, const float* P2, const float* self2, const float* hyp, void* workspace,
                            float** slab, float** partials, float** TB);
// assemble_wide.hip: the RBF family's prior diagonal on ARD packs and its backward (kernel_diag_family<RbfRadial>, _bwd_)
int kernel_diag_rbf(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* hyp, float* out);
int kernel_diag_bwd_rbf(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* ell, const float* hyp, const float* out,
                        const float* gbar, float* d_ell, float* d_hyp);
// assemble_ard.hip: dsvgp_kernel_bwd_ard's body with a family's Tbar launcher (every launch after the Tbar tiles sees the kernel through
// Tbar alone)
int kernel_bwd_ard_family(dsvgp_ctx* ctx, TbarLauncher tbar, const void* G, int64_t ldg, int g_is_double, const float* P1,
                          const float* self1, const float* vnorm1, int n1, int p1, const float* P2, const float* self2, int n2, int p2,
                          int d, const float* ell, const float* hyp, int symmetric, float* d_x1, float* d_v1, float* d_ell, float* d_hyp,
                          void* workspace);

namespace {

constexpr int RECT_BWD_CAP = 9984;          // floats of the two [Tr][Rc] row-pass buffers and the [Rr][Rc] pair values at q1 x q2 = 6 x 1
constexpr int CM = 64, CN = 64, CK = 32;    // the contraction's output tile and K step (kernel_bwd_wide_contract_kernel, assemble_wide.hip)

// the arithmetic: the tile rule, the dynamic LDS of both launches on those tiles, the grid, and the backward's cut and workspace --
// the contraction is split over n2q until ~2048 workgroups run (a few per CU), pieces of at least 256 columns.  cap_columns: the
// rectangular backward's cap on the column tile.  Refuses nothing.
inline TilePlan tile_plan(int n1q, int q1, int n2q, int q2, int DP, bool cap_columns) {
    TilePlan t;
    t.q1 = q1; t.q2 = q2; t.n1q = n1q; t.n2q = n2q;
    t.DP = DP; t.K4 = DP - 4; t.NP = (DP + 15) & ~15;
    const int R1 = WTMAX / q1;
    t.Rr = R1 >= 2 ? R1 / 2 : R1;
    t.Tr = t.Rr * q1;
    t.Rc = WTMAX / q2;
    if (cap_columns && t.Rc > RECT_BWD_CAP / (2 * t.Tr + t.Rr)) t.Rc = RECT_BWD_CAP / (2 * t.Tr + t.Rr);      // (Tr <= 96: at least 51)
    t.Tc = t.Rc * q2;
    const int Trp = (t.Tr + 15) & ~15, Tcp = (t.Tc + 15) & ~15;
    const size_t fwd_f = wide_union_floats(Trp, Tcp) + Trp + Tcp + (size_t)t.Rr * t.Rc;
    t.lds_fwd = sizeof(float) * fwd_f;
    t.lds_tbar = sizeof(float) * (fwd_f + (size_t)Trp * WLDT + 2 * (size_t)t.Tr * t.Rc + 2 * (WNT / 64));
    t.gx = cdiv(n2q, t.Tc); t.gy = cdiv(n1q, t.Tr);
    t.nparts = (int)((int64_t)t.gx * t.gy);
    int ns = cdiv(2048, (int64_t)cdiv(n1q, CM) * cdiv(t.NP, CN));
    const int smax = cdiv(n2q, 256);
    if (ns > smax) ns = smax;
    if (ns < 1) ns = 1;
    t.kper = cdiv(cdiv(n2q, ns), CK) * CK;
    t.ns = cdiv(n2q, t.kper);
    t.slab_f = ((size_t)t.ns * n1q * t.NP + 63) & ~(size_t)63;
    t.part_f = ((size_t)2 * t.nparts + 63) & ~(size_t)63;
    t.tb_f = (size_t)n1q * n2q;
    t.bytes = sizeof(float) * (t.slab_f + t.part_f + t.tb_f) + 64;
    return t;
}

// the plan of a rectangular call from its point and direction counts -- the forward's tiles, or (backward) the rectangular backward's capped
// ones -- and the one set of refusals: 0, or DSVGP_EINVAL for a geometry or a grid the kernels do not take.  Pure host arithmetic.
inline int rect_tile_plan(int n1, int p1, int n2, int p2, int d, bool backward, TilePlan& t) {
    if (n1 <= 0 || n2 <= 0 || d < 1 || p1 < 0 || p2 < 0 || p1 + 1 > WTMAX || p2 + 1 > WTMAX) return DSVGP_EINVAL;
    const int q1 = p1 + 1, q2 = p2 + 1;
    if ((int64_t)n1 * q1 > INT_MAX || (int64_t)n2 * q2 > INT_MAX || d > INT_MAX - 64) return DSVGP_EINVAL;
    t = tile_plan(n1 * q1, q1, n2 * q2, q2, dsvgp_packed_width(d), backward);
    if (t.gy > 65535) return DSVGP_EINVAL;
    if (backward && ((int64_t)t.gx * t.gy > INT_MAX / 2 || cdiv(t.n1q, CM) > 65535)) return DSVGP_EINVAL;
    return 0;
}

__device__ __forceinline__ float pair_nn(float ssum, float t) { return fmaxf(ssum - 2.f * t, 0.f); }

// ---- forward ------------------------------------------------------------------------------------
// every T entry is ONE v_mfma_f32_16x16x4_f32 accumulator chain over the whole K loop, in k order (wide_T); the micro-block transform runs
// out of LDS and every output element is stored once, rows coalesced
template <typename Radial, typename OutT>
__global__ __launch_bounds__(WNT) void kernel_fwd_tiled_kernel(const float* __restrict__ P1, const float* __restrict__ self1, int n1q,
                                                               int q1, int Rr, const float* __restrict__ P2,
                                                               const float* __restrict__ self2, int n2q, int q2, int Rc, int K4, int DP,
                                                               const float* __restrict__ hyp, float jitter, OutT* __restrict__ out,
                                                               int64_t ld) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Tr = Rr * q1, Tc = Rc * q2;
    const int Trp = (Tr + 15) & ~15, Tcp = (Tc + 15) & ~15;
    float* Ts = smem;                                   // [Trp][WLDT], over the chunk images
    float* s1 = smem + wide_union_floats(Trp, Tcp);
    float* s2 = s1 + Trp;
    float* KK = s2 + Tcp;                               // [NPAIR][Rr * Rc] pair values
    const int np = Rr * Rc;
    const int row0 = blockIdx.y * Tr, col0 = blockIdx.x * Tc;
    const int rows = min(Tr, n1q - row0), cols = min(Tc, n2q - col0);      // (whole micro-blocks: n1q, Tr multiples of q1, ...)
    for (int r = threadIdx.x; r < Trp; r += WNT) s1[r] = r < rows ? self1[row0 + r] : 0.f;
    for (int c = threadIdx.x; c < Tcp; c += WNT) s2[c] = c < cols ? self2[col0 + c] : 0.f;
    const typename Radial::Hyp h(hyp);                  // (read here: the K loop hides the dependent scalar loads)
    wide_T(Ts, smem, P1, row0, rows, P2, col0, cols, Trp, Tcp, K4, DP);

    const Radial f(h);
    const float invq1 = 1.f / (float)q1, invq2 = 1.f / (float)q2, invRc = 1.f / (float)Rc;
    const bool blocks = q1 > 1 || q2 > 1;               // (1 x 1 micro-blocks: the pair value is the output, below)
    if (blocks) {
        for (int pid = threadIdx.x; pid < np; pid += WNT) {
            const int pi = fdiv_small(pid, invRc), pj = pid - pi * Rc;
            f.pair(KK + pid, np, pair_nn(s1[pi * q1] + s2[pj * q2], Ts[pi * q1 * WLDT + pj * q2]));
        }
        __syncthreads();
    }
    const int ngrp = WNT / Tc;                          // row groups: thread (rg, c) walks column c over the rows rg, rg + ngrp, ...
    const int c = threadIdx.x % Tc, rg = threadIdx.x / Tc;
    if (rg < ngrp && c < cols) {
        const int rj = fdiv_small(c, invq2);
        const int c0 = rj * q2, b = c - c0;
        const float s2c = s2[c];
        OutT* optr = out + (int64_t)(row0 + rg) * ld + col0 + c;
        const int64_t ostep = (int64_t)ngrp * ld;
        const int64_t gc = col0 + c;
        if (blocks) {
            int ri = fdiv_small(rg, invq1);
            int a = rg - ri * q1;
            const int da = ngrp % q1, di = ngrp / q1;
            for (int r = rg; r < rows; r += ngrp) {
                const int r0 = r - a;
                const float* kk = KK + ri * Rc + rj;
                const float k = f.pair_value(kk, np);
                const float t = Ts[r * WLDT + c];
                const float u = s1[r] - Ts[r * WLDT + c0];              // r . v1_a   (a >= 1)
                const float w = Ts[r0 * WLDT + c] - s2c;                // r . v2_b   (b >= 1)
                float val = f.entry(k, kk, np, a, b, t, u, w);
                if (row0 + r == gc) val += jitter;
                *optr = (OutT)val;
                optr += ostep;
                a += da; ri += di;
                if (a >= q1) { a -= q1; ++ri; }
            }
        } else {
            for (int r = rg; r < rows; r += ngrp) {
                float val = f.value(pair_nn(s1[r] + s2c, Ts[r * WLDT + c]));
                if (row0 + r == gc) val += jitter;
                *optr = (OutT)val;
                optr += ostep;
            }
        }
    }
}

// the forward's dynamic LDS on plan t: NPAIR - 1 more pair arrays where a micro-block has derivative rows or columns
template <typename Radial>
inline size_t fwd_tiles_lds(const TilePlan& t) {
    return t.lds_fwd + ((t.q1 > 1 || t.q2 > 1) ? (Radial::NPAIR - 1) * sizeof(float) * (size_t)t.Rr * t.Rc : 0);
}

template <typename Radial>
int launch_fwd_tiles(hipStream_t st, const TilePlan& t, const float* P1, const float* self1, const float* P2, const float* self2,
                     const float* hyp, float jitter, void* out, int64_t ld, int out_is_double) {
    if (t.gy > 65535) return DSVGP_EINVAL;
    const size_t lds = fwd_tiles_lds<Radial>(t);
    auto launch = [&](auto tag) {
        using OutT = decltype(tag);
        (void)hipFuncSetAttribute((const void*)kernel_fwd_tiled_kernel<Radial, OutT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((kernel_fwd_tiled_kernel<Radial, OutT>), dim3(t.gx, t.gy), dim3(WNT), lds, st, P1, self1, t.n1q, t.q1, t.Rr, P2,
                           self2, t.n2q, t.q2, t.Rc, t.K4, t.DP, hyp, jitter, (OutT*)out, ld);
    };
    if (out_is_double) launch(double()); else launch(float());
    DSVGP_LAUNCH_CHECK();
    return 0;
}

// ---- backward, launch 1: Tbar tiles -------------------------------------------------------------
// per tile: T over the K loop again, Tbar from the upstream tile by a row pass (one task per (tile row, column point): the strip's p2
// derivative columns) and a column pass (one task per (row point, tile column): the strip's p1 derivative rows) -- the inner loops run
// b = 1..p2 and a = 1..p1, nothing else knows a period -- Tbar to the global scratch TB[n1q, n2q], the tile's partial sums to `partials`
template <typename Radial, typename GT>
__global__ __launch_bounds__(WNT) void kernel_bwd_tbar_kernel(const GT* __restrict__ G, int64_t ldg, const float* __restrict__ P1,
                                                              const float* __restrict__ self1, int n1q, int q1, int Rr,
                                                              const float* __restrict__ P2, const float* __restrict__ self2, int n2q,
                                                              int q2, int Rc, int K4, int DP, const float* __restrict__ hyp,
                                                              float* __restrict__ TB, float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NW = WNT / 64, NSUM = Radial::NSUM;
    const int p1 = q1 - 1, p2 = q2 - 1;
    const int Tr = Rr * q1, Tc = Rc * q2;
    const int Trp = (Tr + 15) & ~15, Tcp = (Tc + 15) & ~15;
    float* Ts = smem;                                   // [Trp][WLDT], over the chunk images
    float* Gs = smem + wide_union_floats(Trp, Tcp);     // [Trp][WLDT]  Gbar, then Tbar in place
    float* s1 = Gs + Trp * WLDT;                        // [Trp]
    float* s2 = s1 + Trp;                               // [Tcp]
    float* KK = s2 + Tcp;                               // [Rr][Rc]     the policy's value per point pair (written by the row pass)
    float* Us = KK + Rr * Rc;                           // [Tr][Rc]     u_a = r . v1_a
    float* Ps = Us + Tr * Rc;                           // [Tr][Rc]     per-strip share of Tbar_00
    float* red = Ps + Tr * Rc;                          // [2 NW]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.y * Tr, col0 = blockIdx.x * Tc;
    const int rows = min(Tr, n1q - row0), cols = min(Tc, n2q - col0);      // (whole micro-blocks on both sides)
    for (int e = tid; e < Trp * Tcp; e += WNT) {
        const int r = e / Tcp, c = e - r * Tcp;
        Gs[r * WLDT + c] = (r < rows && c < cols) ? (float)G[(int64_t)(row0 + r) * ldg + col0 + c] : 0.f;
    }
    for (int r = tid; r < Trp; r += WNT) s1[r] = r < rows ? self1[row0 + r] : 0.f;
    for (int c = tid; c < Tcp; c += WNT) s2[c] = c < cols ? self2[col0 + c] : 0.f;
    wide_T(Ts, smem, P1, row0, rows, P2, col0, cols, Trp, Tcp, K4, DP);

    const Radial f{typename Radial::Hyp(hyp)};
    const float invq1 = 1.f / (float)q1, invq2 = 1.f / (float)q2, invRc = 1.f / (float)Rc, invTc = 1.f / (float)Tc;
    float acc[2] = {0.f, 0.f};
    // row pass
    for (int task = tid; task < Tr * Rc; task += WNT) {
        const int r = fdiv_small(task, invRc), pj = task - r * Rc;
        const int pi = fdiv_small(r, invq1), a = r - pi * q1;
        const int r0 = pi * q1, c0 = pj * q2;
        float* gr_ = Gs + r * WLDT + c0;
        const float* tr_ = Ts + r * WLDT + c0;
        const float* t0_ = Ts + r0 * WLDT + c0;
        const float* s2_ = s2 + c0;
        const float ssum = s1[r0] + s2_[0];
        const typename Radial::Row R = f.row(ssum, pair_nn(ssum, t0_[0]));
        const float g0 = gr_[0];
        if (a == 0) {
            float first = 0.f;
            for (int b = 1; b <= p2; ++b) first = __builtin_fmaf(gr_[b], t0_[b] - s2_[b], first);
            f.row_value(R, g0, first, Ps[task], KK[pi * Rc + pj], acc);
        } else {
            const float u = s1[r] - tr_[0];
            const float ps = f.row_deriv(R, gr_, tr_, t0_, s2_, p2, g0, u, acc);
            Us[task] = u;
            Ps[task] = ps;
        }
    }
    __syncthreads();
    // column pass
    for (int task = tid; task < Rr * Tc; task += WNT) {
        const int pi = fdiv_small(task, invTc), c = task - pi * Tc;
        const int pj = fdiv_small(c, invq2), b = c - pj * q2;
        const int r0 = pi * q1;
        const float k = KK[pi * Rc + pj];
        float* g0c = Gs + r0 * WLDT + c;
        if (b == 0) {
            float kbar = 0.f;
            for (int a = 0; a <= p1; ++a) kbar += Ps[(r0 + a) * Rc + pj];
            *g0c = f.col_value(k, kbar, s1[r0], s2 + c, Ts + r0 * WLDT + c, acc);                                     // Tbar_00
        } else {
            *g0c = f.col_deriv(k, p1, s1[r0], s2 + c, Ts + r0 * WLDT + c, b, g0c, Us + r0 * Rc + pj, Rc, acc);        // Tbar_0b
        }
    }
    __syncthreads();
    for (int r = wave; r < rows; r += NW)
        for (int c = lane; c < cols; c += 64) TB[(int64_t)(row0 + r) * n2q + col0 + c] = Gs[r * WLDT + c];
    float ps[NSUM];
    f.partials(acc, ps);
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int i = 0; i < NSUM; ++i) ps[i] += __shfl_down(ps[i], off);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NSUM; ++i) red[wave * NSUM + i] = ps[i];
    __syncthreads();
    if (tid == 0) {
        float tot[2] = {0.f, 0.f};
        for (int w = 0; w < NW; ++w)
#pragma unroll
            for (int i = 0; i < NSUM; ++i) tot[i] += red[w * NSUM + i];
        const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        partials[bid * 2] = tot[0];
        partials[bid * 2 + 1] = tot[1];
    }
}

template <typename Radial>
int launch_tbar_tiles(hipStream_t st, const TilePlan& t, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1,
                      const float* P2, const float* self2, const float* hyp, float* TB, float* partials) {
    auto launch = [&](auto tag) {
        using GT = decltype(tag);
        (void)hipFuncSetAttribute((const void*)kernel_bwd_tbar_kernel<Radial, GT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)t.lds_tbar);
        hipLaunchKernelGGL((kernel_bwd_tbar_kernel<Radial, GT>), dim3(t.gx, t.gy), dim3(WNT), t.lds_tbar, st, (const GT*)G, ldg, P1, self1, t.n1q,
                           t.q1,
                           t.Rr, P2, self2, t.n2q, t.q2, t.Rc, t.K4, t.DP, hyp, TB, partials);
    };
    if (g_is_double) launch(double()); else launch(float());
    DSVGP_LAUNCH_CHECK();
    return 0;
}

// ---- prior diagonal on ARD packs: out[i q] = s, out[i q + a] = f1(0) s |v~_ia|^2 ------------------------------
// one wave per packed row; the lanes' strided partial sums meet in a fixed shuffle tree
template <typename Radial>
__global__ __launch_bounds__(WNT) void kernel_diag_kernel(const float* __restrict__ P, int64_t nq, int q, int K4, int DP,
                                                          const float* __restrict__ hyp, float* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * (WNT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= nq) return;
    const float s = hyp[1];
    if (row % q == 0) {
        if (lane == 0) out[row] = s;
        return;
    }
    const float* Pr = P + row * DP;
    float acc = 0.f;
    for (int k = lane; k < K4; k += 64) acc = __builtin_fmaf(Pr[k], Pr[k], acc);      // (columns d..K4-1 hold zeros)
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if (lane == 0) out[row] = (float)Radial::F1_0 * s * acc;
}

// fixed-order sum of 256 doubles held one per thread; the total is valid on thread 0
__device__ __forceinline__ double block_sum64(double v, double* part) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (int off = WNT / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    return part[0];
}

// backward of the diagonal.  Block k < d: d_ell[k] += -(2 f1(0) s / ell_k) sum_{i, a >= 1} gbar_ia v~_iak^2; block d: d_hyp[1] += sum gbar out / s.
// One block per output, the rows dealt to the threads in a fixed stride, fp64 partial sums, a fixed tree (column_mean_kernel's shape).
template <typename Radial>
__global__ __launch_bounds__(WNT) void kernel_diag_bwd_kernel(const float* __restrict__ P, int64_t nq, int q, int d, int DP,
                                                              const float* __restrict__ ell, const float* __restrict__ hyp,
                                                              const float* __restrict__ out, const float* __restrict__ gbar,
                                                              float* __restrict__ d_ell, float* __restrict__ d_hyp) {
    __shared__ double part[WNT];
    const int k = blockIdx.x;
    double acc = 0.0;
    if (k < d) {
        for (int64_t r = threadIdx.x; r < nq; r += WNT) {
            if (r % q == 0) continue;
            const float pv = P[r * DP + k];
            acc += (double)gbar[r] * (double)(pv * pv);
        }
        const double tot = block_sum64(acc, part);
        if (threadIdx.x == 0) d_ell[k] += (float)(-2.0 * Radial::F1_0 * (double)hyp[1] / (double)ell[k] * tot);
    } else {
        for (int64_t r = threadIdx.x; r < nq; r += WNT) acc += (double)gbar[r] * (double)out[r];
        const double tot = block_sum64(acc, part);
        if (threadIdx.x == 0) d_hyp[1] += (float)(tot / (double)hyp[1]);
    }
}

// the one argument test of the diag entries: DSVGP_EINVAL, or 0 with the packed rows in *rows (n == 0: nothing to do, whatever d)
inline int diag_rows(const dsvgp_ctx* ctx, const float* P, int n, int p, int d, int64_t* rows) {
    if (!ctx || !P || n < 0 || d < 1 || p < 0 || p + 1 > WTMAX) return DSVGP_EINVAL;
    *rows = (int64_t)n * (p + 1);
    return (n > 0 && (*rows > INT_MAX || d > INT_MAX - 64)) ? DSVGP_EINVAL : 0;
}

template <typename Radial>
int kernel_diag_family(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* hyp, float* out) {
    int64_t rows;
    if (!hyp || !out) return DSVGP_EINVAL;
    if (int rc = diag_rows(ctx, P, n, p, d, &rows)) return rc;
    if (n == 0) return 0;
    const int DP = dsvgp_packed_width(d);
    hipLaunchKernelGGL(kernel_diag_kernel<Radial>, dim3(cdiv(rows, WNT / 64)), dim3(WNT), 0, ctx->stream, P, rows, p + 1, DP - 4, DP, hyp,
                       out);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

template <typename Radial>
int kernel_diag_bwd_family(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* ell, const float* hyp, const float* out,
                           const float* gbar, float* d_ell, float* d_hyp) {
    int64_t rows;
    if (!ell || !hyp || !out || !gbar || !d_ell || !d_hyp) return DSVGP_EINVAL;
    if (int rc = diag_rows(ctx, P, n, p, d, &rows)) return rc;
    if (n == 0) return 0;
    hipLaunchKernelGGL(kernel_diag_bwd_kernel<Radial>, dim3(d + 1), dim3(WNT), 0, ctx->stream, P, rows, p + 1, d, dsvgp_packed_width(d),
                       ell, hyp, out, gbar, d_ell, d_hyp);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

}  // namespace
