// Rectangular kernel assembly, gfx950: out[n1 (p1 + 1), n2 (p2 + 1)] = s K(x1, x2; v1, v2) when the two point sets carry DIFFERENT
// numbers of directions -- the K_ZX of a model with p inducing directions evaluated at data with pd directions per point (pd = 0:
// function values only; pd = d: the full gradient).  Forward (predictions, and K_ZX of the training step at pd != p) and the backward with
// respect to side 1 and the two hyper-parameters (training at pd != p).
//
// The formulation is assemble.hip's (header comment there): T = P1 P2^T holds every inner product of the micro-block (i, j),
//     T[i0,j0] = x1~.x2~      T[i0,jb] = x1~.v2_b      T[ia,j0] = v1_a.x2~      T[ia,jb] = v1_a.v2_b        a <= p1, b <= p2
// and a packed row does not know how many direction rows follow it, so each side is packed by dsvgp_pack_points with ITS OWN p (and
// the same centre).  Only the micro-block shape changes: (p1 + 1) x (p2 + 1).
//
// One workgroup (256 threads) per tile of Rr x Rc micro-blocks, Rr (p1 + 1) <= 96 rows by Rc (p2 + 1) <= 96 columns: each side
// fills the 96-wide tile with whole points on its own, as kernel_fwd_wide_kernel does with one q (Rc = 96 / q2 points per column
// tile, half of 96 / q1 per row tile), so q = 96 on one side and q = 1 on the other still gives a 96 x 96 tile.  T comes from the
// K-looped MFMA product of wide_product.h (32 packed columns per chunk: the LDS does not grow with d; one accumulator chain per
// entry in k order, no split over d), the transform runs out of LDS and every output element is stored once, rows coalesced.  LDS:
// max((Trp + Tcp) 33, Trp 100) + Trp + Tcp + Rr Rc floats <= 39552 bytes (p1 = 95, p2 = 0).  No atomics; two identical calls are bitwise
// equal.  At p1 == p2 the arithmetic is kernel_fwd_wide_kernel's, operation for operation.
//
// Backward (dsvgp_kernel_bwd_rect), the three launches of the wide-input backward (assemble_wide.hip):
//   1. kernel_bwd_rect_tbar_kernel: per tile T over the K loop again, Tbar from the upstream tile with kernel_bwd_wide_tbar_kernel's
//      row / column passes -- the row pass's inner loops run b = 1..p2, the column pass's a = 1..p1, nothing else in the algebra knows
//      a period -- Tbar[n1 q1, n2 q2] to the workspace and the tile's two hyper-parameter partial sums to partials[workgroup][2];
//   2. slab[s] = Tbar[:, K_s] . [P2 | 1][K_s, :NP]: kernel_bwd_wide_contract_kernel as it is (it sees n2 q2 packed rows, no period);
//   3. the points launch of every kernel backward with side 1's geometry (d, p1): slabs and partials added in the fixed order
//      s = 0, 1, ... into d_x1 / d_v1 / d_hyp.
// No floating-point atomics: two identical calls are bitwise equal.  Tiles: the forward's rule with a cap on the column tile,
//     Rr = max(1, (96 / q1) / 2),  Tr = Rr q1,  Rc = min(96 / q2, 9984 / (2 Tr + Rr)),
// 9984 floats being what the two [Tr][Rc] row-pass buffers and the [Rr][Rc] pair values take at q1 x q2 = 6 x 1 (Tr 48, Rc 96).  The
// cap bites at q2 = 1 only, for q1 <= 4 (many pair values: Rc = 69 at q1 = 1) and for q1 >= 52 (Tr > 48: Rc = 51 at q1 = 96).  At
// p1 == p2 it bites at p = 0 alone; everywhere else tiles and arithmetic there are kernel_bwd_wide_tbar_kernel's.  LDS of launch 1,
// floats (Trp / Tcp = Tr / Tc padded to 16):
//     max((Trp + Tcp) 33, Trp 100) + Trp 100 + Trp + Tcp + Rr Rc + 2 Tr Rc + 8
// <= 78944 bytes (6 x 1) for every q1 <= 48: two workgroups per CU; 117372 bytes at 87 x 1, the maximum over all q1, q2 <= 96 (one
// workgroup per CU: 76.8 KB of it are the T and Tbar tiles of 96 rows, which no column cap shrinks).
#include "common.h"
#include "wide_product.h"

#include <climits>

namespace {

__global__ __launch_bounds__(WNT) void kernel_fwd_rect_kernel(const float* __restrict__ P1, const float* __restrict__ self1, int n1q,
                                                              int q1, int Rr, const float* __restrict__ P2,
                                                              const float* __restrict__ self2, int n2q, int q2, int Rc, int K4, int DP,
                                                              const float* __restrict__ hyp, float* __restrict__ out, int64_t ld) {
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
    wide_T(Ts, smem, P1, row0, rows, P2, col0, cols, Trp, Tcp, K4, DP);

    // kernel_fwd_kernel's micro-block transform (assemble.hip) with a row period q1 and a column period q2
    const float ell = hyp[0], s = hyp[1];
    const float il = 1.f / ell, il2 = il * il;
    const float invq1 = 1.f / (float)q1, invq2 = 1.f / (float)q2, invRc = 1.f / (float)Rc;
    for (int pid = threadIdx.x; pid < Rr * Rc; pid += WNT) {
        const int pi = fdiv_small(pid, invRc), pj = pid - pi * Rc;
        const float nn = fmaxf(s1[pi * q1] + s2[pj * q2] - 2.f * Ts[pi * q1 * WLDT + pj * q2], 0.f);
        KK[pid] = s * expf(-0.5f * nn);
    }
    __syncthreads();
    const int ngrp = WNT / Tc;                          // row groups: thread (rg, c) walks column c over the rows rg, rg + ngrp, ...
    const int c = threadIdx.x % Tc, rg = threadIdx.x / Tc;
    if (rg < ngrp && c < cols) {
        const int rj = fdiv_small(c, invq2);
        const int c0 = rj * q2, b = c - c0;
        const float s2c = s2[c];
        float* optr = out + (int64_t)(row0 + rg) * ld + col0 + c;
        const int64_t ostep = (int64_t)ngrp * ld;
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
            *optr = (a ? f1 : f0) * k;
            optr += ostep;
            a += da; ri += di;
            if (a >= q1) { a -= q1; ++ri; }
        }
    }
}

// ---- backward, launch 1: Tbar tiles (kernel_bwd_wide_tbar_kernel with a row period q1 and a column period q2) ----
template <typename GT>
__global__ __launch_bounds__(WNT) void kernel_bwd_rect_tbar_kernel(const GT* __restrict__ G, int64_t ldg,
                                                                   const float* __restrict__ P1, const float* __restrict__ self1, int n1q,
                                                                   int q1, int Rr, const float* __restrict__ P2,
                                                                   const float* __restrict__ self2, int n2q, int q2, int Rc, int K4, int DP,
                                                                   const float* __restrict__ hyp, float* __restrict__ TB,
                                                                   float* __restrict__ partials) {
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

// tiles of the backward: the forward's rule, the column tile capped so that the two [Tr][Rc] row-pass buffers and the [Rr][Rc] pair
// values hold at most the 9984 floats they take at q1 x q2 = 6 x 1 (header comment)
constexpr int RECT_BWD_CAP = 9984;
struct RectBwdPlan { int q1, q2, n1q, n2q, Rr, Rc, Tr, Tc, Trp, Tcp, gx, gy, nparts, K4, DP, NP; size_t lds, slab_f, part_f, tb_f; };
// 0, or DSVGP_EINVAL for a geometry or a grid the kernels do not take (pure host arithmetic)
inline int rect_bwd_plan(int n1, int p1, int n2, int p2, int d, RectBwdPlan& w) {
    if (n1 <= 0 || n2 <= 0 || d < 1 || p1 < 0 || p2 < 0 || p1 + 1 > WTMAX || p2 + 1 > WTMAX) return DSVGP_EINVAL;
    w.q1 = p1 + 1; w.q2 = p2 + 1;
    if ((int64_t)n1 * w.q1 > INT_MAX || (int64_t)n2 * w.q2 > INT_MAX || d > INT_MAX - 64) return DSVGP_EINVAL;
    w.n1q = n1 * w.q1; w.n2q = n2 * w.q2;
    w.DP = dsvgp_packed_width(d); w.K4 = w.DP - 4; w.NP = (w.DP + 15) & ~15;
    const int R1 = WTMAX / w.q1;
    w.Rr = R1 >= 2 ? R1 / 2 : R1;
    w.Tr = w.Rr * w.q1;
    w.Rc = WTMAX / w.q2;
    if (w.Rc > RECT_BWD_CAP / (2 * w.Tr + w.Rr)) w.Rc = RECT_BWD_CAP / (2 * w.Tr + w.Rr);          // (Tr <= 96: at least 51)
    w.Tc = w.Rc * w.q2;
    w.Trp = (w.Tr + 15) & ~15; w.Tcp = (w.Tc + 15) & ~15;
    w.lds = sizeof(float) * (wide_union_floats(w.Trp, w.Tcp) + (size_t)w.Trp * WLDT + w.Trp + w.Tcp + (size_t)w.Rr * w.Rc +
                             2 * (size_t)w.Tr * w.Rc + 2 * (WNT / 64));
    w.gx = cdiv(w.n2q, w.Tc); w.gy = cdiv(w.n1q, w.Tr);
    if (w.gy > 65535 || (int64_t)w.gx * w.gy > INT_MAX / 2 || cdiv(w.n1q, 64) > 65535) return DSVGP_EINVAL;
    w.nparts = w.gx * w.gy;
    w.slab_f = kernel_bwd_wide_slab_floats(w.n1q, w.n2q, w.NP);
    w.part_f = ((size_t)2 * w.nparts + 63) & ~(size_t)63;
    w.tb_f = (size_t)w.n1q * w.n2q;
    return 0;
}

}  // namespace

extern "C" size_t dsvgp_kernel_bwd_rect_workspace_bytes(int n1, int p1, int n2, int p2, int d) {
    RectBwdPlan w;
    if (rect_bwd_plan(n1, p1, n2, p2, d, w)) return 0;
    return sizeof(float) * (w.slab_f + w.part_f + w.tb_f) + 64;
}

extern "C" int dsvgp_kernel_bwd_rect(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1,
                                     const float* vnorm1, int n1, int p1, const float* P2, const float* self2, int n2, int p2, int d,
                                     const float* hyp, float* d_x1, float* d_v1, float* d_hyp, void* workspace) {
    if (!ctx || !G || !P1 || !self1 || !P2 || !self2 || !hyp || !d_x1 || !d_hyp || !workspace) return DSVGP_EINVAL;
    if (p1 > 0 && (!vnorm1 || !d_v1)) return DSVGP_EINVAL;
    if (d < 1 || p1 < 0 || p2 < 0 || p1 + 1 > WTMAX || p2 + 1 > WTMAX || n1 < 0 || n2 < 0) return DSVGP_EINVAL;
    if (n1 == 0 || n2 == 0) return 0;
    RectBwdPlan w;
    if (int rc = rect_bwd_plan(n1, p1, n2, p2, d, w)) return rc;
    if (ldg < w.n2q) return DSVGP_EINVAL;
    if (((uintptr_t)P1 | (uintptr_t)P2) % 16) return DSVGP_EINVAL;         // the packed rows are read 16 bytes at a time
    if ((uintptr_t)workspace % 4 || (uintptr_t)G % (g_is_double ? 8 : 4)) return DSVGP_EINVAL;
    float* slab = (float*)workspace;
    float* partials = slab + w.slab_f;
    float* TB = partials + w.part_f;
    dim3 grid(w.gx, w.gy);
    if (g_is_double) {
        (void)hipFuncSetAttribute((const void*)kernel_bwd_rect_tbar_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.lds);
        hipLaunchKernelGGL(kernel_bwd_rect_tbar_kernel<double>, grid, dim3(WNT), w.lds, ctx->stream, (const double*)G, ldg, P1, self1, w.n1q,
                           w.q1, w.Rr, P2, self2, w.n2q, w.q2, w.Rc, w.K4, w.DP, hyp, TB, partials);
    } else {
        (void)hipFuncSetAttribute((const void*)kernel_bwd_rect_tbar_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.lds);
        hipLaunchKernelGGL(kernel_bwd_rect_tbar_kernel<float>, grid, dim3(WNT), w.lds, ctx->stream, (const float*)G, ldg, P1, self1, w.n1q,
                           w.q1, w.Rr, P2, self2, w.n2q, w.q2, w.Rc, w.K4, w.DP, hyp, TB, partials);
    }
    DSVGP_LAUNCH_CHECK();
    int ns = 0;
    if (int rc = launch_kernel_bwd_wide_contract(ctx->stream, TB, w.n1q, w.n2q, P2, w.DP, w.NP, slab, &ns)) return rc;
    return kernel_bwd_finish_points(ctx, d, p1, slab, ns, P1, vnorm1, n1, hyp, 1.f, d_x1, d_v1, partials, w.nparts, d_hyp);
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
    const int DP = dsvgp_packed_width(d), K4 = DP - 4;
    const int R1 = WTMAX / q1;
    const int Rr = R1 >= 2 ? R1 / 2 : R1, Rc = WTMAX / q2;                  // (row tiles of half as many points, as wide_tiles)
    const int Tr = Rr * q1, Tc = Rc * q2, Trp = (Tr + 15) & ~15, Tcp = (Tc + 15) & ~15;
    const size_t lds = sizeof(float) * (wide_union_floats(Trp, Tcp) + Trp + Tcp + (size_t)Rr * Rc);
    const int gy = cdiv(n1q, Tr);
    if (gy > 65535) return DSVGP_EINVAL;
    (void)hipFuncSetAttribute((const void*)kernel_fwd_rect_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel_fwd_rect_kernel, dim3(cdiv(n2q, Tc), gy), dim3(WNT), lds, ctx->stream, P1, self1, n1q, q1, Rr, P2, self2,
                       n2q, q2, Rc, K4, DP, hyp, out, ld);
    DSVGP_LAUNCH_CHECK();
    return 0;
}
