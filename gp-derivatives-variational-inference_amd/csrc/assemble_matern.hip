// Matern-5/2 assembly with directional derivatives, gfx950: the second kernel family on the tiles of assemble_wide.hip.
//
// Formulation.  Matern always runs on the ARD packs of assemble_ard.hip (x~ = (x - c) ./ ell, v~_a = (v_a / |v_a|) ./ ell, hyp[0] = 1), so
// the lengthscales never appear here.  With T = P1 P2^T (wide_T) and the packs' self terms, for the point pair (i, j)
//     nn = max(self1[i0] + self2[j0] - 2 T[i0,j0], 0)     u_a = self1[ia] - T[ia,j0]     w_b = T[i0,jb] - self2[jb]     t_ab = T[ia,jb]
//     a = sqrt(5 nn), e = exp(-a):    f0 = (1 + a + a^2/3) e    f1 = (5/3)(1 + a) e    f2 = (25/3) e    f3 = (125/3) e / a
// (f_{m+1} = -2 d f_m / d nn; the RBF kernel is f0 = f1 = f2 = exp(-nn/2)) the micro-block is
//     s [[ f0, f1 w_b ], [ -f1 u_a, f1 t_ab - f2 u_a w_b ]]
// and its backward, given G on the block, in the TB conventions of kernel_bwd_tbar_kernel (every launch after the Tbar tiles -- the
// contraction, the ARD points / column-sum / self-rows / reduce kernels -- sees the kernel through Tbar alone and is shared):
//     Tbar_ab = s f1 G_ab
//     Tbar_a0 = -ubar_a    ubar_a = s (-f1 G_a0 - f2 sum_b G_ab w_b)
//     Tbar_0b =  wbar_b    wbar_b = s ( f1 G_0b - f2 sum_a G_ab u_a)
//     Tbar_00 = -2 nnbar   nnbar  = -s/2 [G_00 f1 + f2 sum_b G_0b w_b - f2 sum_a G_a0 u_a + sum_ab G_ab (f2 t_ab - f3 u_a w_b)]
// f3 only ever multiplies u_a w_b, which is exactly 0 where nn is (the k-ordered self terms: K_ZZ's diagonal micro-blocks, exact duplicate
// points), and |u_a w_b| <= nn |v~_a| |v~_b|.  The division is guarded at the rounding noise of nn itself,
//     f3 = (125/3) e rsqrt(5 max(nn, 2^-23 (self1[i0] + self2[j0]), 1e-36)),
// so the product is 0 at nn = 0 (never 0 inf) and stays of the order sqrt(noise) where cancellation has left nothing of nn; any pair whose
// nn stands above its rounding noise gets the plain quotient.  sum(G o K), which feeds d_hyp[1], is accumulated directly: the block entries
// are not proportional to one pair value, so the RBF kernel's shortcut (sum of Tbar_00) does not hold.
//
// Tiles, grid, K loop, row / column pass, TB store and the fixed-order workgroup reduction are those of kernel_fwd_tiled_kernel /
// kernel_bwd_tbar_kernel (copies: the RBF instances are not touched, profiles/matern_resource_usage.txt).  LDS:
//   forward   three pair values (s f0, s f1, s f2) per point pair: the RBF forward's bytes + 8 Rr Rc (nothing more at 1 x 1 micro-blocks, which
//             touch no pair array): at most 47424 bytes, at q1 x q2 = 2 x 1, over all q1, q2 <= 96 (dsvgp_kernel_fwd_matern52_lds_bytes)
//   Tbar      the RBF Tbar launch's bytes unchanged (<= 117372): KK holds e per pair (written by the row pass); the column pass rebuilds
//             a = sqrt(5 nn) from the tile -- one sqrt per task -- and f1 = (5/3)(1 + a) e, f2 / f1 = 5 / (1 + a) (no second exp, and no
//             division by an e that has underflowed)
// No floating-point atomics: every sum has a fixed order, two identical calls are bitwise equal.
#include "common.h"
#include "wide_product.h"

#include <climits>

namespace {

constexpr float C53 = 5.f / 3.f, C253 = 25.f / 3.f, C1253 = 125.f / 3.f;
constexpr float NN_EPS = 1.1920929e-7f;        // 2^-23: the rounding noise of nn relative to the two self terms it is the difference of

// ---- forward ------------------------------------------------------------------------------------
template <typename OutT>
__global__ __launch_bounds__(WNT) void kernel_fwd_matern52_kernel(const float* __restrict__ P1, const float* __restrict__ self1, int n1q,
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
    float* K0 = s2 + Tcp;                               // Rr * Rc pair values s f0, then s f1, then s f2
    float* K1 = K0 + Rr * Rc;
    float* K2 = K1 + Rr * Rc;
    const int row0 = blockIdx.y * Tr, col0 = blockIdx.x * Tc;
    const int rows = min(Tr, n1q - row0), cols = min(Tc, n2q - col0);      // (whole micro-blocks: n1q, Tr multiples of q1, ...)
    for (int r = threadIdx.x; r < Trp; r += WNT) s1[r] = r < rows ? self1[row0 + r] : 0.f;
    for (int c = threadIdx.x; c < Tcp; c += WNT) s2[c] = c < cols ? self2[col0 + c] : 0.f;
    const float s = hyp[1];                             // (read here: the K loop hides the dependent scalar load; hyp[0] = 1 is not read)
    wide_T(Ts, smem, P1, row0, rows, P2, col0, cols, Trp, Tcp, K4, DP);

    const float invq1 = 1.f / (float)q1, invq2 = 1.f / (float)q2, invRc = 1.f / (float)Rc;
    const bool blocks = q1 > 1 || q2 > 1;               // (1 x 1 micro-blocks: the pair value is the output, below)
    if (blocks) {
        for (int pid = threadIdx.x; pid < Rr * Rc; pid += WNT) {
            const int pi = fdiv_small(pid, invRc), pj = pid - pi * Rc;
            const float nn = fmaxf(s1[pi * q1] + s2[pj * q2] - 2.f * Ts[pi * q1 * WLDT + pj * q2], 0.f);
            const float a = sqrtf(5.f * nn);
            const float se = s * expf(-a);
            K0[pid] = (1.f + a + C53 * nn) * se;
            K1[pid] = C53 * (1.f + a) * se;
            K2[pid] = C253 * se;
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
                const int pid = ri * Rc + rj;
                const float k1 = K1[pid];
                const float t = Ts[r * WLDT + c];
                const float u = s1[r] - Ts[r * WLDT + c0];              // r . v1_a   (a >= 1)
                const float w = Ts[r0 * WLDT + c] - s2c;                // r . v2_b   (b >= 1)
                const float v0 = b ? (k1 * w) : K0[pid];
                const float v1 = b ? (k1 * t - K2[pid] * (u * w)) : (-k1 * u);      // (u w first: K_ZZ comes out exactly symmetric)
                float val = a ? v1 : v0;
                if (row0 + r == gc) val += jitter;
                *optr = (OutT)val;
                optr += ostep;
                a += da; ri += di;
                if (a >= q1) { a -= q1; ++ri; }
            }
        } else {
            for (int r = rg; r < rows; r += ngrp) {
                const float nn = fmaxf(s1[r] + s2c - 2.f * Ts[r * WLDT + c], 0.f);
                const float a = sqrtf(5.f * nn);
                float val = (1.f + a + C53 * nn) * (s * expf(-a));
                if (row0 + r == gc) val += jitter;
                *optr = (OutT)val;
                optr += ostep;
            }
        }
    }
}

// ---- backward, launch 1: Tbar tiles -------------------------------------------------------------
template <typename GT>
__global__ __launch_bounds__(WNT) void kernel_bwd_tbar_matern52_kernel(const GT* __restrict__ G, int64_t ldg, const float* __restrict__ P1,
                                                                       const float* __restrict__ self1, int n1q, int q1, int Rr,
                                                                       const float* __restrict__ P2, const float* __restrict__ self2,
                                                                       int n2q, int q2, int Rc, int K4, int DP,
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
    float* KK = s2 + Tcp;                               // [Rr][Rc]     e = exp(-a) per point pair
    float* Us = KK + Rr * Rc;                           // [Tr][Rc]     u_a = r . v1_a
    float* Ps = Us + Tr * Rc;                           // [Tr][Rc]     per-strip share of -2 nnbar / s
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

    // the ROW and COLUMN passes of kernel_bwd_tbar_kernel with the Matern radial factors
    const float s = hyp[1];
    const float invq1 = 1.f / (float)q1, invq2 = 1.f / (float)q2, invRc = 1.f / (float)Rc, invTc = 1.f / (float)Tc;
    float gk_acc = 0.f;                                 // sum(G o K) / s
    // row pass: one task per (tile row, column point); the strip's p2 derivative columns
    for (int task = tid; task < Tr * Rc; task += WNT) {
        const int r = fdiv_small(task, invRc), pj = task - r * Rc;
        const int pi = fdiv_small(r, invq1), a = r - pi * q1;
        const int r0 = pi * q1, c0 = pj * q2;
        float* gr_ = Gs + r * WLDT + c0;
        const float* tr_ = Ts + r * WLDT + c0;
        const float* t0_ = Ts + r0 * WLDT + c0;
        const float* s2_ = s2 + c0;
        const float ssum = s1[r0] + s2_[0];
        const float nn = fmaxf(ssum - 2.f * t0_[0], 0.f);
        const float ra = sqrtf(5.f * nn);
        const float e = expf(-ra);
        const float f1 = C53 * (1.f + ra) * e, f2 = C253 * e;
        const float g0 = gr_[0];
        if (a == 0) {
            float first = 0.f;
            for (int b = 1; b <= p2; ++b) first = __builtin_fmaf(gr_[b], t0_[b] - s2_[b], first);
            Ps[task] = __builtin_fmaf(f2, first, g0 * f1);
            KK[pi * Rc + pj] = e;
            gk_acc += __builtin_fmaf(g0, (1.f + ra + C53 * nn) * e, f1 * first);
        } else {
            const float u = s1[r] - tr_[0];
            const float f3 = C1253 * e * rsqrtf(5.f * fmaxf(fmaxf(nn, NN_EPS * ssum), 1e-36f));
            float gt = 0.f, gw = 0.f;
            const float sf1 = s * f1;
            for (int b = 1; b <= p2; ++b) {
                const float w = t0_[b] - s2_[b];
                const float g = gr_[b];
                gt = __builtin_fmaf(g, tr_[b], gt);
                gw = __builtin_fmaf(g, w, gw);
                gr_[b] = sf1 * g;                                   // Tbar_ab
            }
            gr_[0] = __builtin_fmaf(s * f2, gw, sf1 * g0);          // Tbar_a0 = -ubar_a
            Us[task] = u;
            Ps[task] = f2 * (gt - g0 * u) - f3 * u * gw;
            gk_acc += f1 * (gt - u * g0) - f2 * u * gw;
        }
    }
    __syncthreads();
    // column pass: one task per (row point, tile column); the strip's p1 derivative rows
    for (int task = tid; task < Rr * Tc; task += WNT) {
        const int pi = fdiv_small(task, invTc), c = task - pi * Tc;
        const int pj = fdiv_small(c, invq2), b = c - pj * q2;
        const int r0 = pi * q1;
        float* g0c = Gs + r0 * WLDT + c;
        if (b == 0) {
            float kbar = 0.f;
            for (int a = 0; a <= p1; ++a) kbar += Ps[(r0 + a) * Rc + pj];
            *g0c = s * kbar;                                        // Tbar_00 = -2 nnbar
        } else {
            const int c0 = c - b;
            const float nn = fmaxf(s1[r0] + s2[c0] - 2.f * Ts[r0 * WLDT + c0], 0.f);
            const float ra1 = 1.f + sqrtf(5.f * nn);
            float acc = 0.f;
            for (int a = 1; a <= p1; ++a) acc = __builtin_fmaf(g0c[a * WLDT], Us[(r0 + a) * Rc + pj], acc);
            // wbar_b = s f1 G_0b - (f2 / f1) sum_a Tbar_ab u_a,   f2 / f1 = 5 / (1 + a)
            *g0c = s * (C53 * ra1 * KK[pi * Rc + pj]) * *g0c - (5.f / ra1) * acc;      // Tbar_0b
        }
    }
    __syncthreads();
    for (int r = wave; r < rows; r += NW)
        for (int c = lane; c < cols; c += 64) TB[(int64_t)(row0 + r) * n2q + col0 + c] = Gs[r * WLDT + c];
    float gk_sum = s * gk_acc;
    for (int off = 32; off > 0; off >>= 1) gk_sum += __shfl_down(gk_sum, off);
    if (lane == 0) red[wave] = gk_sum;
    __syncthreads();
    if (tid == 0) {
        float a0 = 0.f;
        for (int w = 0; w < NW; ++w) a0 += red[w];
        const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        partials[bid * 2] = a0;                         // sum(G o K) of the tile
        partials[bid * 2 + 1] = 0.f;                    // (the scalar-lengthscale slot of the RBF launch: nothing reads it on ARD packs)
    }
}

// ---- prior diagonal: out[i q] = s, out[i q + a] = (5/3) s |v~_ia|^2 (kernel_diag_ard_kernel's shape) ----------------------------
constexpr int MNT = 256;
__global__ __launch_bounds__(MNT) void kernel_diag_matern52_kernel(const float* __restrict__ P, int64_t nq, int q, int K4, int DP,
                                                                   const float* __restrict__ hyp, float* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * (MNT / 64) + (threadIdx.x >> 6);
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
    if (lane == 0) out[row] = C53 * s * acc;
}

// fixed-order sum of 256 doubles held one per thread; the total is valid on thread 0
__device__ __forceinline__ double block_sum64(double v, double* part) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (int off = MNT / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    return part[0];
}

// backward of the diagonal.  Block k < d: d_ell[k] += -(2 (5/3) s / ell_k) sum_{i, a >= 1} gbar_ia v~_iak^2; block d: d_hyp[1] += sum gbar out / s.
__global__ __launch_bounds__(MNT) void kernel_diag_matern52_bwd_kernel(const float* __restrict__ P, int64_t nq, int q, int d, int DP,
                                                                       const float* __restrict__ ell, const float* __restrict__ hyp,
                                                                       const float* __restrict__ out, const float* __restrict__ gbar,
                                                                       float* __restrict__ d_ell, float* __restrict__ d_hyp) {
    __shared__ double part[MNT];
    const int k = blockIdx.x;
    double acc = 0.0;
    if (k < d) {
        for (int64_t r = threadIdx.x; r < nq; r += MNT) {
            if (r % q == 0) continue;
            const float pv = P[r * DP + k];
            acc += (double)gbar[r] * (double)(pv * pv);
        }
        const double tot = block_sum64(acc, part);
        if (threadIdx.x == 0) d_ell[k] += (float)(-2.0 * (5.0 / 3.0) * (double)hyp[1] / (double)ell[k] * tot);
    } else {
        for (int64_t r = threadIdx.x; r < nq; r += MNT) acc += (double)gbar[r] * (double)out[r];
        const double tot = block_sum64(acc, part);
        if (threadIdx.x == 0) d_hyp[1] += (float)(tot / (double)hyp[1]);
    }
}

// dynamic LDS of the Matern forward on the forward tiles of geometry g: two more pair values per point pair (none at 1 x 1 micro-blocks,
// where the pair value is the output and no pair array is touched)
inline size_t matern_lds_fwd(const RectTilesGeom& g) {
    return g.lds_fwd + ((g.q1 > 1 || g.q2 > 1) ? 2 * sizeof(float) * (size_t)g.Rr * g.Rc : 0);
}

inline int diag_args_bad(const void* ctx, const float* P, int n, int p, int d) {
    return !ctx || !P || n < 0 || d < 1 || p < 0 || p + 1 > WTMAX;
}

}  // namespace

int launch_kernel_bwd_matern52_tiles(hipStream_t st, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1,
                                     int n1, int p1, const float* P2, const float* self2, int n2, int p2, int d, const float* hyp,
                                     void* workspace, float** slab, int* ns, float** partials, int* nparts, float** TB) {
    RectTilesGeom g;
    if (int rc = kernel_rect_tiles_geometry(n1, p1, n2, p2, d, true, &g)) return rc;
    if (ldg < g.n2q) return DSVGP_EINVAL;
    float* sl = (float*)workspace;
    float* pt = sl + g.slab_f;
    float* tb = pt + g.part_f;
    dim3 grid(g.gx, g.gy);
    if (g_is_double) {
        (void)hipFuncSetAttribute((const void*)kernel_bwd_tbar_matern52_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)g.lds_tbar);
        hipLaunchKernelGGL(kernel_bwd_tbar_matern52_kernel<double>, grid, dim3(WNT), g.lds_tbar, st, (const double*)G, ldg, P1, self1, g.n1q,
                           g.q1, g.Rr, P2, self2, g.n2q, g.q2, g.Rc, g.K4, g.DP, hyp, tb, pt);
    } else {
        (void)hipFuncSetAttribute((const void*)kernel_bwd_tbar_matern52_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)g.lds_tbar);
        hipLaunchKernelGGL(kernel_bwd_tbar_matern52_kernel<float>, grid, dim3(WNT), g.lds_tbar, st, (const float*)G, ldg, P1, self1, g.n1q,
                           g.q1, g.Rr, P2, self2, g.n2q, g.q2, g.Rc, g.K4, g.DP, hyp, tb, pt);
    }
    DSVGP_LAUNCH_CHECK();
    if (int rc = launch_kernel_bwd_contract(st, tb, g, P2, sl)) return rc;
    *slab = sl; *partials = pt; *TB = tb;
    *ns = g.ns; *nparts = g.nparts;
    return 0;
}

// the forward's dynamic LDS for direction counts p1, p2 (host arithmetic; 0: refused) -- the maximum over all counts is in the header comment
extern "C" size_t dsvgp_kernel_fwd_matern52_lds_bytes(int p1, int p2) {
    RectTilesGeom g;
    return kernel_rect_tiles_geometry(1, p1, 1, p2, 1, false, &g) ? 0 : matern_lds_fwd(g);
}

extern "C" int dsvgp_kernel_fwd_matern52(dsvgp_ctx* ctx, const float* P1, const float* self1, int n1, int p1, const float* P2,
                                         const float* self2, int n2, int p2, int d, const float* hyp, float jitter, void* out, int64_t ld,
                                         int out_is_double) {
    if (!ctx || !P1 || !self1 || !P2 || !self2 || !hyp || !out) return DSVGP_EINVAL;
    RectTilesGeom g;
    if (int rc = kernel_rect_tiles_geometry(n1, p1, n2, p2, d, false, &g)) return rc;
    if (ld < g.n2q) return DSVGP_EINVAL;
    if (((uintptr_t)P1 | (uintptr_t)P2) % 16) return DSVGP_EINVAL;         // the packed rows are read 16 bytes at a time
    if ((uintptr_t)out % (out_is_double ? 8 : 4)) return DSVGP_EINVAL;
    const size_t lds = matern_lds_fwd(g);
    dim3 grid(g.gx, g.gy);
    if (out_is_double) {
        (void)hipFuncSetAttribute((const void*)kernel_fwd_matern52_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel_fwd_matern52_kernel<double>, grid, dim3(WNT), lds, ctx->stream, P1, self1, g.n1q, g.q1, g.Rr, P2, self2,
                           g.n2q, g.q2, g.Rc, g.K4, g.DP, hyp, jitter, (double*)out, ld);
    } else {
        (void)hipFuncSetAttribute((const void*)kernel_fwd_matern52_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel_fwd_matern52_kernel<float>, grid, dim3(WNT), lds, ctx->stream, P1, self1, g.n1q, g.q1, g.Rr, P2, self2,
                           g.n2q, g.q2, g.Rc, g.K4, g.DP, hyp, jitter, (float*)out, ld);
    }
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t dsvgp_kernel_bwd_matern52_workspace_bytes(int n1, int p1, int n2, int p2, int d) {
    // the same launches after the Tbar tiles and the same layout as the ARD backward's, rounded up to a multiple of 16 bytes
    return (dsvgp_kernel_bwd_ard_workspace_bytes(n1, p1, n2, p2, d) + 15) & ~(size_t)15;
}

extern "C" int dsvgp_kernel_bwd_matern52(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1,
                                         const float* vnorm1, int n1, int p1, const float* P2, const float* self2, int n2, int p2, int d,
                                         const float* ell, const float* hyp, int symmetric, float* d_x1, float* d_v1, float* d_ell,
                                         float* d_hyp, void* workspace) {
    return kernel_bwd_ard_family(ctx, 1, G, ldg, g_is_double, P1, self1, vnorm1, n1, p1, P2, self2, n2, p2, d, ell, hyp, symmetric, d_x1,
                                 d_v1, d_ell, d_hyp, workspace);
}

extern "C" int dsvgp_kernel_diag_matern52(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* hyp, float* out) {
    if (diag_args_bad(ctx, P, n, p, d) || !hyp || !out) return DSVGP_EINVAL;
    if (n == 0) return 0;
    const int64_t rows = (int64_t)n * (p + 1);
    if (rows > INT_MAX || d > INT_MAX - 64) return DSVGP_EINVAL;
    const int DP = dsvgp_packed_width(d);
    hipLaunchKernelGGL(kernel_diag_matern52_kernel, dim3(cdiv(rows, MNT / 64)), dim3(MNT), 0, ctx->stream, P, rows, p + 1, DP - 4, DP, hyp,
                       out);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_kernel_diag_matern52_bwd(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* ell, const float* hyp,
                                              const float* out, const float* gbar, float* d_ell, float* d_hyp) {
    if (diag_args_bad(ctx, P, n, p, d) || !ell || !hyp || !out || !gbar || !d_ell || !d_hyp) return DSVGP_EINVAL;
    if (n == 0) return 0;
    const int64_t rows = (int64_t)n * (p + 1);
    if (rows > INT_MAX || d > INT_MAX - 64) return DSVGP_EINVAL;
    hipLaunchKernelGGL(kernel_diag_matern52_bwd_kernel, dim3(d + 1), dim3(MNT), 0, ctx->stream, P, rows, p + 1, d, dsvgp_packed_width(d),
                       ell, hyp, out, gbar, d_ell, d_hyp);
    DSVGP_LAUNCH_CHECK();
    return 0;
}
