// K-looped tiled assembly, gfx950: the formulation of assemble.hip (header comment there) with T = P1 P2^T accumulated over a K loop of
// fixed 32-column chunks staged through LDS (wide_product.h), so that a workgroup's LDS does not grow with d.  Two uses, one set of kernels:
//   wide        packed width > 96 (d >= 93), both sides with the model's p directions: dsvgp_kernel_fwd / _bwd take these kernels by
//               themselves there, dsvgp_kernel_fwd_wide / _bwd_wide (assemble.hip) whatever d;
//   rectangular out[n1 (p1 + 1), n2 (p2 + 1)] = s K(x1, x2; v1, v2) when the two point sets carry DIFFERENT numbers of directions, any d --
//               the K_ZX of a model with p inducing directions at data with pd directions per point (pd = 0: function values only; pd = d:
//               the full gradient): dsvgp_kernel_fwd_rect / _bwd_rect, at the end of this file.  A packed row does not know how many
//               direction rows follow it, so each side is packed by dsvgp_pack_points with ITS OWN p (and the same centre); T then holds
//               every inner product of the micro-block (i, j),
//                   T[i0,j0] = x1~.x2~      T[i0,jb] = x1~.v2_b      T[ia,j0] = v1_a.x2~      T[ia,jb] = v1_a.v2_b        a <= p1, b <= p2
//               and only the micro-block shape changes: (p1 + 1) x (p2 + 1).
// The kernels take a row period q1 = p1 + 1 and a column period q2 = p2 + 1; the wide entries pass the same q for both.
//
// Tiles (tile_plan): one 256-thread workgroup per tile of Rr x Rc micro-blocks, Tr = Rr q1 <= 96 rows by Tc = Rc q2 <= 96 columns.  Each
// side fills the 96-wide tile with whole points on its own (the tile shapes of kernel_fwd_kernel / kernel_bwd_kernel at q1 == q2),
//     Rc = 96 / q2,   Rr = max(1, (96 / q1) / 2),   Trp / Tcp = Tr / Tc padded to 16,
// so q = 96 on one side and q = 1 on the other still gives a 96 x 96 tile.  The rectangular backward alone caps the column tile,
//     Rc = min(96 / q2, 9984 / (2 Tr + Rr)),
// 9984 floats being what the two [Tr][Rc] row-pass buffers and the [Rr][Rc] pair values take at q1 x q2 = 6 x 1 (Tr 48, Rc 96).  The cap
// bites at q2 = 1 only, for q1 <= 4 (many pair values: Rc = 69 at q1 = 1) and for q1 >= 52 (Tr > 48: Rc = 51 at q1 = 96); at p1 == p2 it
// bites at p = 0 alone, where the wide backward (no cap) keeps Rc = 96.
//
// Forward (kernel_fwd_tiled_kernel): every T entry is ONE v_mfma_f32_16x16x4_f32 accumulator chain over the whole K loop, in k order, with
// kernel_fwd_kernel's operand sequence (no split-K over d): T is bit-identical to that kernel's, so the pack's k-ordered self terms keep
// r == 0 exact on the diagonal micro-blocks of K_ZZ.  The micro-block transform is kernel_fwd_kernel's with the two periods; it runs out
// of LDS and every output element is stored once, rows coalesced.  LDS, floats:
//     max((Trp + Tcp) 33, Trp 100) + Trp + Tcp + Rr Rc                                      <= 39552 bytes (q1 x q2 = 96 x 1)
// Backward, the tile and contraction launches (the points launch of assemble.hip follows and adds the slabs in the fixed order s = 0, 1, ...):
//   1. kernel_bwd_tbar_kernel, per tile: T over the K loop again, Tbar from the upstream tile with kernel_bwd_kernel's row / column passes
//      -- the row pass's inner loops run b = 1..p2, the column pass's a = 1..p1, nothing else in the algebra knows a period -- Tbar to a
//      global scratch TB[n1q, n2q] and the tile's <Gbar, K> / lengthscale partial sums to `partials` (one pair per workgroup).  LDS, floats:
//          max((Trp + Tcp) 33, Trp 100) + Trp 100 + Trp + Tcp + Rr Rc + 2 Tr Rc + 8
//      94304 bytes at 1 x 1 without the cap; with it <= 78944 bytes (6 x 1) for every q1 <= 48: two workgroups per CU; 117372 bytes at
//      87 x 1, the maximum over all q1, q2 <= 96 (one workgroup per CU: 76.8 KB of it are the T and Tbar tiles of 96 rows, which no
//      column cap shrinks);
//   2. kernel_bwd_wide_contract_kernel: slab[s] = TB[:, K_s] . [P2 | indicator][K_s, :NP], a plain MFMA product, 64 x 64 output tiles, the
//      n2q range cut into ns contiguous pieces K_s (one slab each).  It sees n2q packed rows, no period.
// No floating-point atomics anywhere: every sum has a fixed order, two identical calls are bitwise equal.
#include "common.h"
#include "wide_product.h"

#include <climits>

namespace {

// ---- forward ------------------------------------------------------------------------------------
template <typename OutT>
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
    float* KK = s2 + Tcp;                               // Rr * Rc pair values
    const int row0 = blockIdx.y * Tr, col0 = blockIdx.x * Tc;
    const int rows = min(Tr, n1q - row0), cols = min(Tc, n2q - col0);      // (whole micro-blocks: n1q, Tr multiples of q1, ...)
    for (int r = threadIdx.x; r < Trp; r += WNT) s1[r] = r < rows ? self1[row0 + r] : 0.f;
    for (int c = threadIdx.x; c < Tcp; c += WNT) s2[c] = c < cols ? self2[col0 + c] : 0.f;
    const float ell = hyp[0], s = hyp[1];               // (read here: the K loop hides the two dependent scalar loads)
    wide_T(Ts, smem, P1, row0, rows, P2, col0, cols, Trp, Tcp, K4, DP);

    // kernel_fwd_kernel's micro-block transform (assemble.hip) with a row period q1 and a column period q2
    const float il = 1.f / ell, il2 = il * il;
    const float invq1 = 1.f / (float)q1, invq2 = 1.f / (float)q2, invRc = 1.f / (float)Rc;
    const bool blocks = q1 > 1 || q2 > 1;               // (1 x 1 micro-blocks: the pair value is the output, below)
    if (blocks) {
        for (int pid = threadIdx.x; pid < Rr * Rc; pid += WNT) {
            const int pi = fdiv_small(pid, invRc), pj = pid - pi * Rc;
            const float nn = fmaxf(s1[pi * q1] + s2[pj * q2] - 2.f * Ts[pi * q1 * WLDT + pj * q2], 0.f);
            KK[pid] = s * expf(-0.5f * nn);
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
                const float k = KK[ri * Rc + rj];
                const float t = Ts[r * WLDT + c];
                const float u = s1[r] - Ts[r * WLDT + c0];              // r . v1_a   (a >= 1)
                const float w = Ts[r0 * WLDT + c] - s2c;                // r . v2_b   (b >= 1)
                const float f0 = b ? (w * il) : 1.f;
                const float f1 = b ? ((t - u * w) * il2) : (-u * il);
                float val = (a ? f1 : f0) * k;
                if (row0 + r == gc) val += jitter;
                *optr = (OutT)val;
                optr += ostep;
                a += da; ri += di;
                if (a >= q1) { a -= q1; ++ri; }
            }
        } else {
            for (int r = rg; r < rows; r += ngrp) {
                float val = s * expf(-0.5f * fmaxf(s1[r] + s2c - 2.f * Ts[r * WLDT + c], 0.f));
                if (row0 + r == gc) val += jitter;
                *optr = (OutT)val;
                optr += ostep;
            }
        }
    }
}

// ---- backward, launch 1: Tbar tiles -------------------------------------------------------------
template <typename GT>
__global__ __launch_bounds__(WNT) void kernel_bwd_tbar_kernel(const GT* __restrict__ G, int64_t ldg, const float* __restrict__ P1,
                                                              const float* __restrict__ self1, int n1q, int q1, int Rr,
                                                              const float* __restrict__ P2, const float* __restrict__ self2, int n2q,
                                                              int q2, int Rc, int K4, int DP, const float* __restrict__ hyp,
                                                              float* __restrict__ TB, float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NW = WNT / 64;
    const int p1 = q1 - 1, p2 = q2 - 1;
    const int Tr = Rr * q1, Tc = Rc * q2;
    const int Trp = (Tr + 15) & ~15, Tcp = (Tc + 15) & ~15;
    float* Ts = smem;                                   // [Trp][WLDT], over the chunk images
    float* Gs = smem + wide_union_floats(Trp, Tcp);     // [Trp][WLDT]  Gbar, then Tbar in place
    float* s1 = Gs + Trp * WLDT;                        // [Trp]
    float* s2 = s1 + Trp;                               // [Tcp]
    float* KK = s2 + Tcp;                               // [Rr][Rc]     k per point pair
    float* Us = KK + Rr * Rc;                           // [Tr][Rc]     u_a = r . v1_a
    float* Ps = Us + Tr * Rc;                           // [Tr][Rc]     per-strip share of kbar
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

    // the ROW and COLUMN passes of kernel_bwd_kernel (assemble.hip), run-time periods
    const float ell = hyp[0], s = hyp[1];
    const float il = 1.f / ell, il2 = il * il;
    const float invq1 = 1.f / (float)q1, invq2 = 1.f / (float)q2, invRc = 1.f / (float)Rc, invTc = 1.f / (float)Tc;
    float sK_sum = 0.f, l_acc = 0.f;
    // row pass: one task per (tile row, column point); the strip's p2 derivative columns
    for (int task = tid; task < Tr * Rc; task += WNT) {
        const int r = fdiv_small(task, invRc), pj = task - r * Rc;
        const int pi = fdiv_small(r, invq1), a = r - pi * q1;
        const int r0 = pi * q1, c0 = pj * q2;
        float* gr_ = Gs + r * WLDT + c0;
        const float* tr_ = Ts + r * WLDT + c0;
        const float* t0_ = Ts + r0 * WLDT + c0;
        const float* s2_ = s2 + c0;
        const float nn = fmaxf(s1[r0] + s2_[0] - 2.f * t0_[0], 0.f);
        const float k = s * expf(-0.5f * nn);
        const float g0 = gr_[0];
        if (a == 0) {
            float first = 0.f;
            for (int b = 1; b <= p2; ++b) first = __builtin_fmaf(gr_[b], t0_[b] - s2_[b], first);
            first *= il;
            Ps[task] = g0 + first;
            KK[pi * Rc + pj] = k;
            l_acc = __builtin_fmaf(k, first, l_acc);
        } else {
            const float u = s1[r] - tr_[0];
            float hs = 0.f, gw = 0.f;
            const float kil2 = k * il2;
            for (int b = 1; b <= p2; ++b) {
                const float w = t0_[b] - s2_[b];
                const float g = gr_[b];
                hs = __builtin_fmaf(g, tr_[b] - u * w, hs);
                gw = __builtin_fmaf(g, w, gw);
                gr_[b] = kil2 * g;                                  // Tbar_ab
            }
            hs *= il2;
            const float ubar = k * (-g0 * il - gw * il2);
            gr_[0] = -ubar;                                         // Tbar_a0
            Us[task] = u;
            Ps[task] = hs - g0 * u * il;
            l_acc += k * (2.f * hs - g0 * u * il) + ubar * u;
        }
    }
    __syncthreads();
    // column pass: one task per (row point, tile column); the strip's p1 derivative rows
    for (int task = tid; task < Rr * Tc; task += WNT) {
        const int pi = fdiv_small(task, invTc), c = task - pi * Tc;
        const int pj = fdiv_small(c, invq2), b = c - pj * q2;
        const int r0 = pi * q1;
        const float k = KK[pi * Rc + pj];
        float* g0c = Gs + r0 * WLDT + c;
        if (b == 0) {
            float kbar = 0.f;
            for (int a = 0; a <= p1; ++a) kbar += Ps[(r0 + a) * Rc + pj];
            const float t00 = k * kbar;                             // Tbar_00
            const float nn = fmaxf(s1[r0] + s2[c] - 2.f * Ts[r0 * WLDT + c], 0.f);
            *g0c = t00;
            sK_sum += t00;
            l_acc = __builtin_fmaf(-t00, nn, l_acc);
        } else {
            const float w = Ts[r0 * WLDT + c] - s2[c];
            float wbar = k * il * *g0c;
            for (int a = 1; a <= p1; ++a) wbar = __builtin_fmaf(-g0c[a * WLDT], Us[(r0 + a) * Rc + pj], wbar);
            *g0c = wbar;                                            // Tbar_0b
            l_acc = __builtin_fmaf(wbar, w, l_acc);
        }
    }
    __syncthreads();
    for (int r = wave; r < rows; r += NW)
        for (int c = lane; c < cols; c += 64) TB[(int64_t)(row0 + r) * n2q + col0 + c] = Gs[r * WLDT + c];
    float l_sum = -il * l_acc;
    for (int off = 32; off > 0; off >>= 1) {
        sK_sum += __shfl_down(sK_sum, off);
        l_sum += __shfl_down(l_sum, off);
    }
    if (lane == 0) { red[wave * 2] = sK_sum; red[wave * 2 + 1] = l_sum; }
    __syncthreads();
    if (tid == 0) {
        float a0 = 0.f, a1 = 0.f;
        for (int w = 0; w < NW; ++w) { a0 += red[2 * w]; a1 += red[2 * w + 1]; }
        const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        partials[bid * 2] = a0;
        partials[bid * 2 + 1] = a1;
    }
}

// ---- backward, launch 2: slab[s][n1q][NP] = TB[:, K_s] . P2ext[K_s, :] -----------------------------------------
constexpr int CM = 64, CN = 64, CK = 32;
__global__ __launch_bounds__(WNT) void kernel_bwd_wide_contract_kernel(const float* __restrict__ TB, int n1q, int n2q,
                                                                       const float* __restrict__ P2, int DP, int NP, int kper,
                                                                       float* __restrict__ slab) {
    __shared__ float As[CM * (CK + 1)];         // [row][k]
    __shared__ float Bs[CK * (CN + 4)];         // [k][packed column]
    constexpr int LDA = CK + 1, LDB = CN + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * CM, n0 = blockIdx.x * CN;
    const int kb = blockIdx.z * kper, ke = min(n2q, kb + kper);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    f4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = kb; k0 < ke; k0 += CK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < CM * CK / WNT; ++i) {
            const int e = tid + i * WNT, r = e >> 5, c = e & 31;
            As[r * LDA + c] = (m0 + r < n1q && k0 + c < ke) ? TB[(int64_t)(m0 + r) * n2q + k0 + c] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < CK * CN / WNT; ++i) {
            const int e = tid + i * WNT, r = e >> 6, c = e & 63;
            Bs[r * LDB + c] = (k0 + r < ke && n0 + c < DP) ? P2[(int64_t)(k0 + r) * DP + n0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < CK; kk += 4) {
            const int ka = kk + (lane >> 4);
            const float a0 = As[(wm + (lane & 15)) * LDA + ka], a1 = As[(wm + 16 + (lane & 15)) * LDA + ka];
            const float b0 = Bs[ka * LDB + wn + (lane & 15)], b1 = Bs[ka * LDB + wn + 16 + (lane & 15)];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    float* out = slab + (int64_t)blockIdx.z * n1q * NP;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn + j * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm + i * 16 + (lane >> 4) * 4 + r;
                if (row < n1q && col < NP) out[(int64_t)row * NP + col] = acc[i][j][r];
            }
        }
}

// the tile rule of the header comment and the dynamic LDS of the forward and the Tbar launch on those tiles; cap_columns: the rectangular
// backward's cap on the column tile
constexpr int RECT_BWD_CAP = 9984;
struct TilePlan { int Rr, Rc, Tr, Tc, Trp, Tcp; size_t lds_fwd, lds_tbar; };
inline TilePlan tile_plan(int q1, int q2, bool cap_columns) {
    TilePlan t;
    const int R1 = WTMAX / q1;
    t.Rr = R1 >= 2 ? R1 / 2 : R1;
    t.Tr = t.Rr * q1;
    t.Rc = WTMAX / q2;
    if (cap_columns && t.Rc > RECT_BWD_CAP / (2 * t.Tr + t.Rr)) t.Rc = RECT_BWD_CAP / (2 * t.Tr + t.Rr);      // (Tr <= 96: at least 51)
    t.Tc = t.Rc * q2;
    t.Trp = (t.Tr + 15) & ~15; t.Tcp = (t.Tc + 15) & ~15;
    const size_t fwd_f = wide_union_floats(t.Trp, t.Tcp) + t.Trp + t.Tcp + (size_t)t.Rr * t.Rc;
    t.lds_fwd = sizeof(float) * fwd_f;
    t.lds_tbar = sizeof(float) * (fwd_f + (size_t)t.Trp * WLDT + 2 * (size_t)t.Tr * t.Rc + 2 * (WNT / 64));
    return t;
}

// the contraction's cut of the n2q range: ns pieces of kper columns, one slab [n1q][NP] each
struct WideContractPlan { int ns, kper; size_t slab_f; };
inline WideContractPlan wide_contract_plan(int n1q, int n2q, int NP) {
    WideContractPlan c;
    // split the contraction over n2q until ~2048 workgroups run (a few per CU), pieces of at least 256 columns
    const int tiles = cdiv(n1q, CM) * cdiv(NP, CN);
    int ns = cdiv(2048, tiles);
    const int smax = cdiv(n2q, 256);
    if (ns > smax) ns = smax;
    if (ns < 1) ns = 1;
    c.kper = cdiv(cdiv(n2q, ns), CK) * CK;
    c.ns = cdiv(n2q, c.kper);
    c.slab_f = ((size_t)c.ns * n1q * NP + 63) & ~(size_t)63;
    return c;
}

// the two launches of a backward on tiles t and its workspace: slab[ns][n1q][NP] | partials[nparts][2] | TB[n1q][n2q], floats
struct TiledBwdPlan { TilePlan t; int ns, kper, nparts, gx, gy; size_t slab_f, part_f, tb_f, bytes; };
inline TiledBwdPlan tiled_bwd_plan(int n1q, int n2q, const TilePlan& t, int NP) {
    TiledBwdPlan w;
    w.t = t;
    w.gx = cdiv(n2q, t.Tc); w.gy = cdiv(n1q, t.Tr);
    w.nparts = w.gx * w.gy;
    const WideContractPlan c = wide_contract_plan(n1q, n2q, NP);
    w.kper = c.kper; w.ns = c.ns; w.slab_f = c.slab_f;
    w.part_f = ((size_t)2 * w.nparts + 63) & ~(size_t)63;
    w.tb_f = (size_t)n1q * n2q;
    w.bytes = sizeof(float) * (w.slab_f + w.part_f + w.tb_f) + 64;
    return w;
}

int launch_bwd_tiled(hipStream_t st, const TiledBwdPlan& w, const void* G, int64_t ldg, int g_is_double, const float* P1,
                     const float* self1, int n1q, int q1, const float* P2, const float* self2, int n2q, int q2, int K4, int DP, int NP,
                     const float* hyp, void* workspace, float** slab, float** partials) {
    if (w.gy > 65535 || w.ns > 65535) return DSVGP_EINVAL;
    float* sl = (float*)workspace;
    float* pt = sl + w.slab_f;
    float* TB = pt + w.part_f;
    const TilePlan& t = w.t;
    dim3 grid(w.gx, w.gy);
    if (g_is_double) {
        (void)hipFuncSetAttribute((const void*)kernel_bwd_tbar_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds_tbar);
        hipLaunchKernelGGL(kernel_bwd_tbar_kernel<double>, grid, dim3(WNT), t.lds_tbar, st, (const double*)G, ldg, P1, self1, n1q, q1, t.Rr,
                           P2, self2, n2q, q2, t.Rc, K4, DP, hyp, TB, pt);
    } else {
        (void)hipFuncSetAttribute((const void*)kernel_bwd_tbar_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds_tbar);
        hipLaunchKernelGGL(kernel_bwd_tbar_kernel<float>, grid, dim3(WNT), t.lds_tbar, st, (const float*)G, ldg, P1, self1, n1q, q1, t.Rr,
                           P2, self2, n2q, q2, t.Rc, K4, DP, hyp, TB, pt);
    }
    DSVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(kernel_bwd_wide_contract_kernel, dim3(cdiv(NP, CN), cdiv(n1q, CM), w.ns), dim3(WNT), 0, st, TB, n1q, n2q, P2, DP, NP,
                       w.kper, sl);
    DSVGP_LAUNCH_CHECK();
    *slab = sl; *partials = pt;
    return 0;
}

}  // namespace

size_t kernel_bwd_wide_workspace(int n1q, int n2q, int q, int NP) { return tiled_bwd_plan(n1q, n2q, tile_plan(q, q, false), NP).bytes; }

int launch_kernel_fwd_tiled(hipStream_t st, const float* P1, const float* self1, int n1q, int q1, const float* P2, const float* self2,
                            int n2q, int q2, int K4, int DP, const float* hyp, float jitter, void* out, int64_t ld, int out_is_double) {
    const TilePlan t = tile_plan(q1, q2, false);
    const int gy = cdiv(n1q, t.Tr);
    if (gy > 65535) return DSVGP_EINVAL;
    dim3 grid(cdiv(n2q, t.Tc), gy);
    if (out_is_double) {
        (void)hipFuncSetAttribute((const void*)kernel_fwd_tiled_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds_fwd);
        hipLaunchKernelGGL(kernel_fwd_tiled_kernel<double>, grid, dim3(WNT), t.lds_fwd, st, P1, self1, n1q, q1, t.Rr, P2, self2, n2q, q2, t.Rc,
                           K4, DP, hyp, jitter, (double*)out, ld);
    } else {
        (void)hipFuncSetAttribute((const void*)kernel_fwd_tiled_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds_fwd);
        hipLaunchKernelGGL(kernel_fwd_tiled_kernel<float>, grid, dim3(WNT), t.lds_fwd, st, P1, self1, n1q, q1, t.Rr, P2, self2, n2q, q2, t.Rc,
                           K4, DP, hyp, jitter, (float*)out, ld);
    }
    DSVGP_LAUNCH_CHECK();
    return 0;
}

int launch_kernel_bwd_wide(hipStream_t st, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1, int n1q,
                           const float* P2, const float* self2, int n2q, int q, int K4, int DP, int NP, const float* hyp, void* workspace,
                           float** slab, int* ns, float** partials, int* nparts) {
    const TiledBwdPlan w = tiled_bwd_plan(n1q, n2q, tile_plan(q, q, false), NP);
    *ns = w.ns; *nparts = w.nparts;
    return launch_bwd_tiled(st, w, G, ldg, g_is_double, P1, self1, n1q, q, P2, self2, n2q, q, K4, DP, NP, hyp, workspace, slab, partials);
}

// ---- the rectangular entries ----------------------------------------------------------------------------------
namespace {

struct RectBwdPlan { int q1, q2, n1q, n2q, K4, DP, NP; TiledBwdPlan w; };
// 0, or DSVGP_EINVAL for a geometry or a grid the kernels do not take (pure host arithmetic)
inline int rect_bwd_plan(int n1, int p1, int n2, int p2, int d, RectBwdPlan& r) {
    if (n1 <= 0 || n2 <= 0 || d < 1 || p1 < 0 || p2 < 0 || p1 + 1 > WTMAX || p2 + 1 > WTMAX) return DSVGP_EINVAL;
    r.q1 = p1 + 1; r.q2 = p2 + 1;
    if ((int64_t)n1 * r.q1 > INT_MAX || (int64_t)n2 * r.q2 > INT_MAX || d > INT_MAX - 64) return DSVGP_EINVAL;
    r.n1q = n1 * r.q1; r.n2q = n2 * r.q2;
    r.DP = dsvgp_packed_width(d); r.K4 = r.DP - 4; r.NP = (r.DP + 15) & ~15;
    const TilePlan t = tile_plan(r.q1, r.q2, true);
    const int gy = cdiv(r.n1q, t.Tr);
    if (gy > 65535 || (int64_t)cdiv(r.n2q, t.Tc) * gy > INT_MAX / 2 || cdiv(r.n1q, CM) > 65535) return DSVGP_EINVAL;
    r.w = tiled_bwd_plan(r.n1q, r.n2q, t, r.NP);
    return 0;
}

}  // namespace

extern "C" size_t dsvgp_kernel_bwd_rect_workspace_bytes(int n1, int p1, int n2, int p2, int d) {
    RectBwdPlan r;
    return rect_bwd_plan(n1, p1, n2, p2, d, r) ? 0 : r.w.bytes;
}

// dsvgp_kernel_bwd_rect's tile and contraction launches on its own plan, for a caller that brings another points reduction
// (assemble_ard.hip): the same kernels, tiles and arithmetic; TB[n1q][n2q] is handed out as well
int kernel_bwd_rect_tiles_plan(int n1, int p1, int n2, int p2, int d, size_t* bytes, int* ns) {
    RectBwdPlan r;
    if (int rc = rect_bwd_plan(n1, p1, n2, p2, d, r)) return rc;
    *bytes = r.w.bytes; *ns = r.w.ns;
    return 0;
}
int launch_kernel_bwd_rect_tiles(hipStream_t st, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1, int n1,
                                 int p1, const float* P2, const float* self2, int n2, int p2, int d, const float* hyp, void* workspace,
                                 float** slab, int* ns, float** partials, int* nparts, float** TB) {
    RectBwdPlan r;
    if (int rc = rect_bwd_plan(n1, p1, n2, p2, d, r)) return rc;
    if (ldg < r.n2q) return DSVGP_EINVAL;
    if (int rc = launch_bwd_tiled(st, r.w, G, ldg, g_is_double, P1, self1, r.n1q, r.q1, P2, self2, r.n2q, r.q2, r.K4, r.DP, r.NP, hyp,
                                  workspace, slab, partials))
        return rc;
    *ns = r.w.ns; *nparts = r.w.nparts;
    *TB = *partials + r.w.part_f;
    return 0;
}

// the same tiles and contraction for another kernel family's tile kernels (assemble_matern.hip): the geometry and dynamic LDS of the forward
// (backward = false: this file's forward tiles) or of the rectangular backward (its capped tiles, slab cut and workspace layout), and the
// contraction launch by itself.  Refusals are those of dsvgp_kernel_fwd_rect / rect_bwd_plan.
int kernel_rect_tiles_geometry(int n1, int p1, int n2, int p2, int d, bool backward, RectTilesGeom* g) {
    if (n1 <= 0 || n2 <= 0 || d < 1 || p1 < 0 || p2 < 0 || p1 + 1 > WTMAX || p2 + 1 > WTMAX) return DSVGP_EINVAL;
    g->q1 = p1 + 1; g->q2 = p2 + 1;
    if ((int64_t)n1 * g->q1 > INT_MAX || (int64_t)n2 * g->q2 > INT_MAX || d > INT_MAX - 64) return DSVGP_EINVAL;
    g->n1q = n1 * g->q1; g->n2q = n2 * g->q2;
    g->DP = dsvgp_packed_width(d); g->K4 = g->DP - 4; g->NP = (g->DP + 15) & ~15;
    TilePlan t;
    if (backward) {
        RectBwdPlan r;
        if (int rc = rect_bwd_plan(n1, p1, n2, p2, d, r)) return rc;
        t = r.w.t;
        g->ns = r.w.ns; g->kper = r.w.kper; g->nparts = r.w.nparts; g->slab_f = r.w.slab_f; g->part_f = r.w.part_f;
    } else {
        t = tile_plan(g->q1, g->q2, false);
        g->ns = g->kper = g->nparts = 0; g->slab_f = g->part_f = 0;
    }
    g->Rr = t.Rr; g->Rc = t.Rc; g->lds_fwd = t.lds_fwd; g->lds_tbar = t.lds_tbar;
    g->gx = cdiv(g->n2q, t.Tc); g->gy = cdiv(g->n1q, t.Tr);
    if (g->gy > 65535) return DSVGP_EINVAL;
    return 0;
}
int launch_kernel_bwd_contract(hipStream_t st, const float* TB, const RectTilesGeom& g, const float* P2, float* slab) {
    if (g.ns < 1 || g.ns > 65535) return DSVGP_EINVAL;
    hipLaunchKernelGGL(kernel_bwd_wide_contract_kernel, dim3(cdiv(g.NP, CN), cdiv(g.n1q, CM), g.ns), dim3(WNT), 0, st, TB, g.n1q, g.n2q, P2,
                       g.DP, g.NP, g.kper, slab);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_kernel_bwd_rect(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1,
                                     const float* vnorm1, int n1, int p1, const float* P2, const float* self2, int n2, int p2, int d,
                                     const float* hyp, float* d_x1, float* d_v1, float* d_hyp, void* workspace) {
    if (!ctx || !G || !P1 || !self1 || !P2 || !self2 || !hyp || !d_x1 || !d_hyp || !workspace) return DSVGP_EINVAL;
    if (p1 > 0 && (!vnorm1 || !d_v1)) return DSVGP_EINVAL;
    if (d < 1 || p1 < 0 || p2 < 0 || p1 + 1 > WTMAX || p2 + 1 > WTMAX || n1 < 0 || n2 < 0) return DSVGP_EINVAL;
    if (n1 == 0 || n2 == 0) return 0;
    RectBwdPlan r;
    if (int rc = rect_bwd_plan(n1, p1, n2, p2, d, r)) return rc;
    if (ldg < r.n2q) return DSVGP_EINVAL;
    if (((uintptr_t)P1 | (uintptr_t)P2) % 16) return DSVGP_EINVAL;         // the packed rows are read 16 bytes at a time
    if ((uintptr_t)workspace % 4 || (uintptr_t)G % (g_is_double ? 8 : 4)) return DSVGP_EINVAL;
    float *slab, *partials;
    if (int rc = launch_bwd_tiled(ctx->stream, r.w, G, ldg, g_is_double, P1, self1, r.n1q, r.q1, P2, self2, r.n2q, r.q2, r.K4, r.DP, r.NP,
                                  hyp, workspace, &slab, &partials))
        return rc;
    // the points launch of every kernel backward with side 1's geometry (d, p1)
    return kernel_bwd_finish_points(ctx, d, p1, slab, r.w.ns, P1, vnorm1, n1, hyp, 1.f, d_x1, d_v1, partials, r.w.nparts, d_hyp);
}

extern "C" int dsvgp_kernel_fwd_rect(dsvgp_ctx* ctx, const float* P1, const float* self1, int n1, int p1, const float* P2,
                                     const float* self2, int n2, int p2, int d, const float* hyp, float* out, int64_t ld) {
    if (!ctx || !P1 || !self1 || !P2 || !self2 || !hyp || !out) return DSVGP_EINVAL;
    if (n1 <= 0 || n2 <= 0 || d < 1 || p1 < 0 || p2 < 0 || p1 + 1 > WTMAX || p2 + 1 > WTMAX) return DSVGP_EINVAL;
    const int q1 = p1 + 1, q2 = p2 + 1;
    if ((int64_t)n1 * q1 > INT_MAX || (int64_t)n2 * q2 > INT_MAX) return DSVGP_EINVAL;
    const int n1q = n1 * q1, n2q = n2 * q2;
    if (ld < n2q) return DSVGP_EINVAL;
    if (((uintptr_t)P1 | (uintptr_t)P2) % 16) return DSVGP_EINVAL;         // the packed rows are read 16 bytes at a time
    const int DP = dsvgp_packed_width(d);
    return launch_kernel_fwd_tiled(ctx->stream, P1, self1, n1q, q1, P2, self2, n2q, q2, DP - 4, DP, hyp, 0.f, out, ld, 0);
}
