// Wide-input assembly (packed width > 96, i.e. d >= 93), gfx950: the formulation of assemble.hip (header comment there) with
// T = P1 P2^T accumulated over a K loop of fixed 32-column chunks staged through LDS, so that a workgroup's LDS does not grow with d.
//
// Forward: one (Tr x Tc) tile of the interleaved matrix per 256-thread workgroup (the tile shapes of kernel_fwd_kernel).  Every T entry is
// ONE v_mfma_f32_16x16x4_f32 accumulator chain over the whole K loop, in k order, with kernel_fwd_kernel's operand sequence (no
// split-K over d): T is bit-identical to that kernel's, so the pack's k-ordered self terms keep r == 0 exact on the diagonal
// micro-blocks of K_ZZ.  The micro-block transform is kernel_fwd_kernel's.
// Backward, two launches:
//   1. per tile: T over the K loop again, Tbar from the upstream tile with kernel_bwd_kernel's row / column passes, Tbar to a global
//      scratch TB[n1q, n2q] and the tile's <Gbar, K> / lengthscale partial sums to `partials` (one pair per workgroup);
//   2. slab[s] = TB[:, K_s] . [P2 | indicator][K_s, :NP]: a plain MFMA product, 64 x 64 output tiles, the n2q range cut into ns
//      contiguous pieces K_s (one slab each).  The points launch (assemble.hip) adds the slabs in the fixed order s = 0, 1, ...
// No floating-point atomics anywhere: every sum has a fixed order, the results are run-to-run identical.
#include "common.h"
#include "wide_product.h"

namespace {

// ---- forward ------------------------------------------------------------------------------------
template <typename OutT>
__global__ __launch_bounds__(WNT) void kernel_fwd_wide_kernel(const float* __restrict__ P1, const float* __restrict__ self1, int n1q,
                                                              const float* __restrict__ P2, const float* __restrict__ self2, int n2q,
                                                              int q, int Rr, int Rc, int K4, int DP, const float* __restrict__ hyp,
                                                              float jitter, OutT* __restrict__ out, int64_t ld) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Tr = Rr * q, Tc = Rc * q;
    const int Trp = (Tr + 15) & ~15, Tcp = (Tc + 15) & ~15;
    float* Ts = smem;                                   // [Trp][WLDT], over the chunk images
    float* s1 = smem + wide_union_floats(Trp, Tcp);
    float* s2 = s1 + Trp;
    float* KK = s2 + Tcp;                               // Rr * Rc pair values
    const int row0 = blockIdx.y * Tr, col0 = blockIdx.x * Tc;
    const int rows = min(Tr, n1q - row0), cols = min(Tc, n2q - col0);
    for (int r = threadIdx.x; r < Trp; r += WNT) s1[r] = r < rows ? self1[row0 + r] : 0.f;
    for (int c = threadIdx.x; c < Tcp; c += WNT) s2[c] = c < cols ? self2[col0 + c] : 0.f;
    wide_T(Ts, smem, P1, row0, rows, P2, col0, cols, Trp, Tcp, K4, DP);

    // the micro-block transform of kernel_fwd_kernel (assemble.hip)
    const float ell = hyp[0], s = hyp[1];
    const float il = 1.f / ell, il2 = il * il;
    const float invq = 1.f / (float)q, invRc = 1.f / (float)Rc;
    if (q > 1) {
        for (int pid = threadIdx.x; pid < Rr * Rc; pid += WNT) {
            const int pi = fdiv_small(pid, invRc), pj = pid - pi * Rc;
            const float nn = fmaxf(s1[pi * q] + s2[pj * q] - 2.f * Ts[pi * q * WLDT + pj * q], 0.f);
            KK[pid] = s * expf(-0.5f * nn);
        }
        __syncthreads();
    }
    const int ngrp = WNT / Tc;
    const int c = threadIdx.x % Tc, rg = threadIdx.x / Tc;
    if (rg < ngrp && c < cols) {
        const int rj = fdiv_small(c, invq);
        const int c0 = rj * q, b = c - c0;
        const float s2c = s2[c];
        OutT* optr = out + (int64_t)(row0 + rg) * ld + col0 + c;
        const int64_t ostep = (int64_t)ngrp * ld;
        const int64_t gc = col0 + c;
        if (q > 1) {
            int ri = fdiv_small(rg, invq);
            int a = rg - ri * q;
            const int da = ngrp % q, di = ngrp / q;
            for (int r = rg; r < rows; r += ngrp) {
                const int r0 = r - a;
                const float k = KK[ri * Rc + rj];
                const float t = Ts[r * WLDT + c];
                const float u = s1[r] - Ts[r * WLDT + c0];
                const float w = Ts[r0 * WLDT + c] - s2c;
                const float f0 = b ? (w * il) : 1.f;
                const float f1 = b ? ((t - u * w) * il2) : (-u * il);
                float val = (a ? f1 : f0) * k;
                if (row0 + r == gc) val += jitter;
                *optr = (OutT)val;
                optr += ostep;
                a += da; ri += di;
                if (a >= q) { a -= q; ++ri; }
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
__global__ __launch_bounds__(WNT) void kernel_bwd_wide_tbar_kernel(const GT* __restrict__ G, int64_t ldg,
                                                                   const float* __restrict__ P1, const float* __restrict__ self1, int n1q,
                                                                   const float* __restrict__ P2, const float* __restrict__ self2, int n2q,
                                                                   int q, int Rr, int Rc, int K4, int DP, const float* __restrict__ hyp,
                                                                   float* __restrict__ TB, float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NW = WNT / 64;
    const int p = q - 1;
    const int Tr = Rr * q, Tc = Rc * q;
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
    const int rows = min(Tr, n1q - row0), cols = min(Tc, n2q - col0);
    for (int e = tid; e < Trp * Tcp; e += WNT) {
        const int r = e / Tcp, c = e - r * Tcp;
        Gs[r * WLDT + c] = (r < rows && c < cols) ? (float)G[(int64_t)(row0 + r) * ldg + col0 + c] : 0.f;
    }
    for (int r = tid; r < Trp; r += WNT) s1[r] = r < rows ? self1[row0 + r] : 0.f;
    for (int c = tid; c < Tcp; c += WNT) s2[c] = c < cols ? self2[col0 + c] : 0.f;
    wide_T(Ts, smem, P1, row0, rows, P2, col0, cols, Trp, Tcp, K4, DP);

    // the ROW and COLUMN passes of kernel_bwd_kernel (assemble.hip), run-time q
    const float ell = hyp[0], s = hyp[1];
    const float il = 1.f / ell, il2 = il * il;
    const float invq = 1.f / (float)q, invRc = 1.f / (float)Rc, invTc = 1.f / (float)Tc;
    float sK_sum = 0.f, l_acc = 0.f;
    for (int task = tid; task < Tr * Rc; task += WNT) {
        const int r = fdiv_small(task, invRc), pj = task - r * Rc;
        const int pi = fdiv_small(r, invq), a = r - pi * q;
        const int r0 = pi * q, c0 = pj * q;
        float* gr_ = Gs + r * WLDT + c0;
        const float* tr_ = Ts + r * WLDT + c0;
        const float* t0_ = Ts + r0 * WLDT + c0;
        const float* s2_ = s2 + c0;
        const float nn = fmaxf(s1[r0] + s2_[0] - 2.f * t0_[0], 0.f);
        const float k = s * expf(-0.5f * nn);
        const float g0 = gr_[0];
        if (a == 0) {
            float first = 0.f;
            for (int b = 1; b <= p; ++b) first = __builtin_fmaf(gr_[b], t0_[b] - s2_[b], first);
            first *= il;
            Ps[task] = g0 + first;
            KK[pi * Rc + pj] = k;
            l_acc = __builtin_fmaf(k, first, l_acc);
        } else {
            const float u = s1[r] - tr_[0];
            float hs = 0.f, gw = 0.f;
            const float kil2 = k * il2;
            for (int b = 1; b <= p; ++b) {
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
    for (int task = tid; task < Rr * Tc; task += WNT) {
        const int pi = fdiv_small(task, invTc), c = task - pi * Tc;
        const int pj = fdiv_small(c, invq), b = c - pj * q;
        const int r0 = pi * q;
        const float k = KK[pi * Rc + pj];
        float* g0c = Gs + r0 * WLDT + c;
        if (b == 0) {
            float kbar = 0.f;
            for (int a = 0; a <= p; ++a) kbar += Ps[(r0 + a) * Rc + pj];
            const float t00 = k * kbar;                             // Tbar_00
            const float nn = fmaxf(s1[r0] + s2[c] - 2.f * Ts[r0 * WLDT + c], 0.f);
            *g0c = t00;
            sK_sum += t00;
            l_acc = __builtin_fmaf(-t00, nn, l_acc);
        } else {
            const float w = Ts[r0 * WLDT + c] - s2[c];
            float wbar = k * il * *g0c;
            for (int a = 1; a <= p; ++a) wbar = __builtin_fmaf(-g0c[a * WLDT], Us[(r0 + a) * Rc + pj], wbar);
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

// tile shapes of kernel_fwd_kernel / kernel_bwd_kernel: column tiles of R = 96 / q points, row tiles of half as many
struct WideTiles { int Rr, Rc, Tr, Tc, Trp, Tcp; };
inline WideTiles wide_tiles(int q) {
    WideTiles t;
    const int R = WTMAX / q;
    t.Rc = R; t.Rr = R >= 2 ? R / 2 : R;
    t.Tr = t.Rr * q; t.Tc = t.Rc * q;
    t.Trp = (t.Tr + 15) & ~15; t.Tcp = (t.Tc + 15) & ~15;
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

struct WideBwdPlan { int ns, kper, nparts, gx, gy; size_t slab_f, part_f, tb_f; };
inline WideBwdPlan wide_bwd_plan(int n1q, int n2q, int q, int NP) {
    WideBwdPlan w;
    const WideTiles t = wide_tiles(q);
    w.gx = cdiv(n2q, t.Tc); w.gy = cdiv(n1q, t.Tr);
    w.nparts = w.gx * w.gy;
    const WideContractPlan c = wide_contract_plan(n1q, n2q, NP);
    w.kper = c.kper; w.ns = c.ns; w.slab_f = c.slab_f;
    w.part_f = ((size_t)2 * w.nparts + 63) & ~(size_t)63;
    w.tb_f = (size_t)n1q * n2q;
    return w;
}

}  // namespace

size_t kernel_bwd_wide_workspace(int n1q, int n2q, int q, int NP) {
    const WideBwdPlan w = wide_bwd_plan(n1q, n2q, q, NP);
    return sizeof(float) * (w.slab_f + w.part_f + w.tb_f) + 64;
}

size_t kernel_bwd_wide_slab_floats(int n1q, int n2q, int NP) { return wide_contract_plan(n1q, n2q, NP).slab_f; }

int launch_kernel_bwd_wide_contract(hipStream_t st, const float* TB, int n1q, int n2q, const float* P2, int DP, int NP, float* slab,
                                    int* ns) {
    const WideContractPlan c = wide_contract_plan(n1q, n2q, NP);
    const int gy = cdiv(n1q, CM);
    if (gy > 65535 || c.ns > 65535) return DSVGP_EINVAL;
    hipLaunchKernelGGL(kernel_bwd_wide_contract_kernel, dim3(cdiv(NP, CN), gy, c.ns), dim3(WNT), 0, st, TB, n1q, n2q, P2, DP, NP, c.kper,
                       slab);
    DSVGP_LAUNCH_CHECK();
    *ns = c.ns;
    return 0;
}

int launch_kernel_fwd_wide(hipStream_t st, const float* P1, const float* self1, int n1q, const float* P2, const float* self2, int n2q,
                           int q, int K4, int DP, const float* hyp, float jitter, void* out, int64_t ld, int out_is_double) {
    const WideTiles t = wide_tiles(q);
    const size_t lds = sizeof(float) * (wide_union_floats(t.Trp, t.Tcp) + t.Trp + t.Tcp + (size_t)t.Rr * t.Rc);
    const int gy = cdiv(n1q, t.Tr);
    if (gy > 65535) return DSVGP_EINVAL;
    dim3 grid(cdiv(n2q, t.Tc), gy);
    if (out_is_double) {
        (void)hipFuncSetAttribute((const void*)kernel_fwd_wide_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel_fwd_wide_kernel<double>, grid, dim3(WNT), lds, st, P1, self1, n1q, P2, self2, n2q, q, t.Rr, t.Rc, K4, DP,
                           hyp, jitter, (double*)out, ld);
    } else {
        (void)hipFuncSetAttribute((const void*)kernel_fwd_wide_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel_fwd_wide_kernel<float>, grid, dim3(WNT), lds, st, P1, self1, n1q, P2, self2, n2q, q, t.Rr, t.Rc, K4, DP,
                           hyp, jitter, (float*)out, ld);
    }
    DSVGP_LAUNCH_CHECK();
    return 0;
}

int launch_kernel_bwd_wide(hipStream_t st, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1, int n1q,
                           const float* P2, const float* self2, int n2q, int q, int K4, int DP, int NP, const float* hyp, void* workspace,
                           float** slab, int* ns, float** partials, int* nparts) {
    const WideTiles t = wide_tiles(q);
    const WideBwdPlan w = wide_bwd_plan(n1q, n2q, q, NP);
    if (w.gy > 65535 || w.ns > 65535) return DSVGP_EINVAL;
    float* sl = (float*)workspace;
    float* pt = sl + w.slab_f;
    float* TB = pt + w.part_f;
    const size_t lds = sizeof(float) * (wide_union_floats(t.Trp, t.Tcp) + (size_t)t.Trp * WLDT + t.Trp + t.Tcp + (size_t)t.Rr * t.Rc +
                                        2 * (size_t)t.Tr * t.Rc + 2 * (WNT / 64));
    dim3 grid(w.gx, w.gy);
    if (g_is_double) {
        (void)hipFuncSetAttribute((const void*)kernel_bwd_wide_tbar_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel_bwd_wide_tbar_kernel<double>, grid, dim3(WNT), lds, st, (const double*)G, ldg, P1, self1, n1q, P2, self2,
                           n2q, q, t.Rr, t.Rc, K4, DP, hyp, TB, pt);
    } else {
        (void)hipFuncSetAttribute((const void*)kernel_bwd_wide_tbar_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel_bwd_wide_tbar_kernel<float>, grid, dim3(WNT), lds, st, (const float*)G, ldg, P1, self1, n1q, P2, self2,
                           n2q, q, t.Rr, t.Rc, K4, DP, hyp, TB, pt);
    }
    DSVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(kernel_bwd_wide_contract_kernel, dim3(cdiv(NP, CN), cdiv(n1q, CM), w.ns), dim3(WNT), 0, st, TB, n1q, n2q, P2, DP, NP,
                       w.kper, sl);
    DSVGP_LAUNCH_CHECK();
    *slab = sl; *ns = w.ns; *partials = pt; *nparts = w.nparts;
    return 0;
}
