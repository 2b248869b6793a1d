// ARD assembly for RBFKernelDirectionalGrad, gfx950: one lengthscale per input dimension, ell in R^d.
//
// Formulation.  The packed rows of assemble.hip carry the per-dimension scaling themselves,
//     x~ = (x - c) ./ ell        v~_a = (v_a / |v_a|) ./ ell        (elementwise)
// and the ARD kernel's micro-blocks are  k [[1, w~_b], [-u~_a, v~_a . v~_b - u~_a w~_b]]  with r = x~1 - x~2, u~_a = r . v~1_a,
// w~_b = r . v~2_b, k = s exp(-|r|^2 / 2): the transform of kernel_fwd_tiled_kernel / kernel_bwd_tbar_kernel (tiled_assembly.h) with
// RbfRadial (assemble_wide.hip) run with hyp[0] = 1 on these rows.  Those kernels see directions through T = P1 P2^T and the self terms alone and nothing in them assumes
// |v| = 1, so the forward (dsvgp_kernel_fwd_wide / dsvgp_kernel_fwd_rect) and the Tbar and contraction launches of the backward are
// theirs, unchanged.  New here: the hyper-parameter chain of an ell vector, the pack, the prior diagonal and its backward, and the
// points reduction of the backward with the per-dimension lengthscale gradient of BOTH sides.  The backward's body serves every family
// on these packs: kernel_bwd_ard_family takes the family's Tbar launcher (everything after the Tbar tiles sees the kernel through Tbar
// alone).  The prior diagonal's two kernels are the family-templated ones of tiled_assembly.h.
//
// Lengthscale gradient.  Every packed entry scales as 1 / ell_k, so d_ell[k] = -(1 / ell_k) sum over the rows of both sides of
// P[r, k] Pbar[r, k], Pbar the total gradient of the row.  With dP = Tbar [P2 | indicator] (the summed slabs),
// nbar_i = -dP[i0, K4] / 2 and alphabar_ia = -dP[ia, K4] (the gradients of side 1's self terms):
//     side 1:  sum_a P1[ia, k] dP[ia, k] + 2 (nbar x~_k^2 + sum_a alphabar_a x~_k v~_ak)
//     side 2:  sum_a P1[ia, k] dP[ia, k]  (the T part: Tbar^T P1 contracted with P2 is the same double sum)
//              + 2 (-cs[j0] x~2_jk^2 / 2 - sum_b cs[jb] x~2_jk v~2_jbk),   cs[c] = sum_i Tbar[i0, c]  (side 2's self terms)
// hence d_ell[k] += -(2 / ell_k) (sum_i E1[i, k] + sum_j E2[j, k]) with the per-point rows E1, E2 below; in the symmetric case
// (same pack, symmetric G) side 2's self part equals side 1's and no column sums are formed.
// No floating-point atomics: every sum has a fixed order, two identical calls are bitwise equal.
#include "common.h"
#include "tiled_assembly.h"

namespace {

constexpr int ANT = WNT;                // threads per workgroup (256: block_sum64 of tiled_assembly.h)
constexpr int AQMAX = 96;               // p + 1 <= 96
constexpr float NOISE_FLOOR = 1e-4f;    // GaussianLikelihood noise constraint GreaterThan(1e-4) (elbo.hip)

__device__ __forceinline__ float softplusf(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// ---- hyper-parameters ---------------------------------------------------------------------------
__global__ void hyp_forward_ard_kernel(const float* __restrict__ rl, int d, const float* __restrict__ rs, const float* __restrict__ rn,
                                       float* __restrict__ ell, float* __restrict__ hyp) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < d) ell[k] = softplusf(rl[k]);
    if (k == 0) {
        hyp[0] = 1.f;                   // the packed rows carry the lengthscales
        hyp[1] = softplusf(rs[0]);
        hyp[2] = softplusf(rn[0]) + NOISE_FLOOR;
        hyp[3] = 0.f;
    }
}
__global__ void hyp_backward_ard_kernel(const float* __restrict__ rl, int d, const float* __restrict__ rs, const float* __restrict__ rn,
                                        const float* __restrict__ d_ell, const float* __restrict__ dh, float* __restrict__ drl,
                                        float* __restrict__ drs, float* __restrict__ drn) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < d) drl[k] += d_ell[k] * sigmoidf(rl[k]);
    if (k == 0) {
        drs[0] += dh[1] * sigmoidf(rs[0]);
        drn[0] += dh[2] * sigmoidf(rn[0]);
    }
}

// ---- pack: pack_points_wide_kernel (assemble.hip) with a lengthscale per column -------------------------------
// One wave per packed row: the lanes write the row coalesced, lane 0 runs the serial k-ordered chains (|v|^2, the self term) that keep
// r == 0 exact on the diagonal micro-blocks of K_ZZ.
__global__ __launch_bounds__(ANT) void pack_points_ard_kernel(const float* __restrict__ x, const float* __restrict__ v, int n, int d, int p,
                                                              const float* __restrict__ ell, const float* __restrict__ center,
                                                              float* __restrict__ P, float* __restrict__ self, float* __restrict__ vnorm,
                                                              int K4, int DP) {
    const int q = p + 1;
    const int64_t row = (int64_t)blockIdx.x * (ANT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (int64_t)n * q) return;
    const int64_t i = row / q;
    const int a = (int)(row - i * q);
    float* Pr = P + row * DP;
    const float* xi = x + i * d;
    if (a == 0) {
        for (int k = lane; k < d; k += 64) Pr[k] = (xi[k] - (center ? center[k] : 0.f)) / ell[k];
        for (int k = d + lane; k < DP; k += 64) Pr[k] = k == K4 ? 1.f : 0.f;      // indicator column
        if (lane == 0) {
            float acc = 0.f;
            for (int k = 0; k < d; ++k) {
                const float xt = (xi[k] - (center ? center[k] : 0.f)) / ell[k];
                acc = __builtin_fmaf(xt, xt, acc);
            }
            self[row] = acc;
        }
    } else {
        const float* vi = v + (i * p + (a - 1)) * d;
        float nrm = 0.f;
        if (lane == 0) {
            float ss = 0.f;
            for (int k = 0; k < d; ++k) ss = __builtin_fmaf(vi[k], vi[k], ss);
            nrm = sqrtf(ss);
        }
        nrm = __shfl(nrm, 0);
        for (int k = lane; k < d; k += 64) Pr[k] = (vi[k] / nrm) / ell[k];
        for (int k = d + lane; k < DP; k += 64) Pr[k] = 0.f;
        if (lane == 0) {
            float acc = 0.f;
            for (int k = 0; k < d; ++k) acc = __builtin_fmaf((vi[k] / nrm) / ell[k], (xi[k] - (center ? center[k] : 0.f)) / ell[k], acc);
            self[row] = acc;
            vnorm[i * p + (a - 1)] = nrm;
        }
    }
}

// ---- backward, the points reduction ---------------------------------------------------------------------------
// dP[row, col] = sum_s slab[s][row][col] in the fixed order s = 0, 1, ... (four loads in flight, as assemble.hip's wide_dp)
__device__ __forceinline__ float slab_sum(const float* __restrict__ slab, int ns, int64_t off, int64_t sstride) {
    float sum = 0.f;
    int sp = 0;
    for (; sp + 4 <= ns; sp += 4) {
        const float a0 = slab[off + sp * sstride], a1 = slab[off + (sp + 1) * sstride];
        const float a2 = slab[off + (sp + 2) * sstride], a3 = slab[off + (sp + 3) * sstride];
        sum += a0; sum += a1; sum += a2; sum += a3;
    }
    for (; sp < ns; ++sp) sum += slab[off + sp * sstride];
    return sum;
}

// One workgroup per point of side 1; LDS does not depend on d (kernel_bwd_points_wide_kernel's form: the summed dP rows are not held,
// every pass re-adds the slabs of the columns it needs).  With v^ = v~ .* ell (unit) and v^bar = v~bar ./ ell the dot of the
// normalisation Jacobian is v^ . v^bar = v~ . v~bar: the lengthscales cancel.
//   d_x1[i, k] += sym x~bar_k / ell_k                      d_v1[ia, k] += sym (v~bar_ak / ell_k - v~_ak ell_k (v~_a . v~bar_a)) / |v_ia|
//   E1[i, k]    = sum_{a >= 0} P1[ia, k] dP[ia, k] + selfw (nbar x~_k^2 + sum_a alphabar_a x~_k v~_ak)        selfw = 2 when symmetric
__global__ __launch_bounds__(ANT) void kernel_bwd_points_ard_kernel(const float* __restrict__ slab, int ns, const float* __restrict__ P1,
                                                                    const float* __restrict__ vnorm1, int n1, int d, int p, int K4, int DP,
                                                                    int NP, const float* __restrict__ ell, float sym, float selfw,
                                                                    float* __restrict__ d_x1, float* __restrict__ d_v1,
                                                                    float* __restrict__ E1) {
    __shared__ float ab[AQMAX];             // dP[ia, K4] = -alphabar_a (a = 0: -2 nbar)
    __shared__ float dots[AQMAX];
    __shared__ float wred[ANT / 64];
    const int i = blockIdx.x, t = threadIdx.x, w = t >> 6, l = t & 63;
    const int q = p + 1;
    const int64_t sstride = (int64_t)n1 * q * NP;
    const int64_t r0 = (int64_t)i * q;
    for (int a = t; a < q; a += ANT) ab[a] = slab_sum(slab, ns, (r0 + a) * NP + K4, sstride);
    __syncthreads();
    const float* xt = P1 + r0 * DP;
    if (d_v1) {
        for (int a = 1; a <= p; ++a) {
            const float* vt = P1 + (r0 + a) * DP;
            const int64_t off = (r0 + a) * NP;
            float dot = 0.f;
            for (int k = t; k < d; k += ANT) dot += vt[k] * (slab_sum(slab, ns, off + k, sstride) - ab[a] * xt[k]);
            for (int o = 32; o > 0; o >>= 1) dot += __shfl_down(dot, o);
            if (l == 0) wred[w] = dot;
            __syncthreads();
            if (t == 0) {
                float s_ = 0.f;
                for (int ww = 0; ww < ANT / 64; ++ww) s_ += wred[ww];
                dots[a] = s_;
            }
            __syncthreads();
        }
    }
    const float nbar = -0.5f * ab[0];
    for (int k = t; k < d; k += ANT) {
        const float lk = ell[k], xk = xt[k];
        const float dp0 = slab_sum(slab, ns, r0 * NP + k, sstride);
        float xb = dp0 + 2.f * nbar * xk;
        float e = xk * dp0, es = nbar * xk * xk;
        for (int a = 1; a <= p; ++a) {
            const float va = P1[(r0 + a) * DP + k];
            const float dpa = slab_sum(slab, ns, (r0 + a) * NP + k, sstride);
            const float alb = -ab[a];
            xb += alb * va;
            e = __builtin_fmaf(va, dpa, e);
            es = __builtin_fmaf(alb * xk, va, es);
            if (d_v1) {
                const float vb = dpa + alb * xk;
                const int64_t o = ((int64_t)i * p + (a - 1));
                d_v1[o * d + k] += sym * (vb / lk - va * lk * dots[a]) / vnorm1[o];
            }
        }
        d_x1[(int64_t)i * d + k] += sym * xb / lk;
        if (E1) E1[(int64_t)i * d + k] = e + selfw * es;
    }
}

// cs[c] = sum_i TB[i q1, c] over the value rows of side 1, i = 0, 1, ... in order; one thread per column
__global__ __launch_bounds__(ANT) void tbar_value_colsum_kernel(const float* __restrict__ TB, int n1, int q1, int n2q, float* __restrict__ cs) {
    const int c = blockIdx.x * ANT + threadIdx.x;
    if (c >= n2q) return;
    const float* src = TB + c;
    const int64_t step = (int64_t)q1 * n2q;
    float sum = 0.f;
    int i = 0;
    for (; i + 4 <= n1; i += 4) {
        const float a0 = src[i * step], a1 = src[(i + 1) * step], a2 = src[(i + 2) * step], a3 = src[(i + 3) * step];
        sum += a0; sum += a1; sum += a2; sum += a3;
    }
    for (; i < n1; ++i) sum += src[i * step];
    cs[c] = sum;
}

// E2[j, k] = -cs[j0] x~2_jk^2 / 2 - sum_b cs[jb] x~2_jk v~2_jbk: side 2's self terms; one workgroup per point
__global__ __launch_bounds__(ANT) void self2_rows_ard_kernel(const float* __restrict__ P2, const float* __restrict__ cs, int d, int q2, int DP,
                                                             float* __restrict__ E2) {
    const int64_t r0 = (int64_t)blockIdx.x * q2;
    const float* xt = P2 + r0 * DP;
    for (int k = threadIdx.x; k < d; k += ANT) {
        const float xk = xt[k];
        float e = -0.5f * cs[r0] * xk * xk;
        for (int b = 1; b < q2; ++b) e = __builtin_fmaf(-cs[r0 + b] * xk, P2[(r0 + b) * DP + k], e);
        E2[(int64_t)blockIdx.x * d + k] = e;
    }
}

// block k < nk (nk = d, or 0 without d_ell): d_ell[k] += -(2 / ell_k) sum_r E[r, k] over the nrows rows of E (side 1's, then side 2's);
// the last block: d_hyp[1] += sum(G o K) / s from the Tbar launch's per-workgroup partials.  fp64 partial sums, fixed stride and tree.
__global__ __launch_bounds__(ANT) void ard_reduce_kernel(const float* __restrict__ E, int64_t nrows, int d, int nk, const float* __restrict__ ell,
                                                         const float* __restrict__ partials, int nparts, const float* __restrict__ hyp,
                                                         float* __restrict__ d_ell, float* __restrict__ d_hyp) {
    __shared__ double part[ANT];
    const int k = blockIdx.x;
    double acc = 0.0;
    if (k < nk) {
        for (int64_t r = threadIdx.x; r < nrows; r += ANT) acc += (double)E[r * d + k];
        const double tot = block_sum64(acc, part);
        if (threadIdx.x == 0) d_ell[k] += (float)(-2.0 / (double)ell[k] * tot);
    } else {
        for (int j = threadIdx.x; j < nparts; j += ANT) acc += (double)partials[2 * j];
        const double tot = block_sum64(acc, part);
        if (threadIdx.x == 0) d_hyp[1] += (float)(tot / (double)hyp[1]);
    }
}

// workspace: [ the rectangular backward's (slab | partials | TB) | pad to 16 bytes | cs[n2q] | E[(n1 + n2), d] ], floats
struct ArdBwdPlan { TilePlan t; size_t cs_off, e_off, bytes; };
inline int ard_bwd_plan(int n1, int p1, int n2, int p2, int d, ArdBwdPlan& a) {
    if (int rc = rect_tile_plan(n1, p1, n2, p2, d, true, a.t)) return rc;
    a.cs_off = (a.t.bytes + 15) & ~(size_t)15;
    a.e_off = a.cs_off + sizeof(float) * (((size_t)n2 * (p2 + 1) + 3) & ~(size_t)3);
    a.bytes = a.e_off + sizeof(float) * ((size_t)n1 + (size_t)n2) * (size_t)d;
    return 0;
}

}  // namespace

extern "C" int dsvgp_hyp_forward_ard(dsvgp_ctx* ctx, const float* rl, int d, const float* rs, const float* rn, float* ell, float* hyp) {
    if (!ctx || !rl || !rs || !rn || !ell || !hyp || d < 1) return DSVGP_EINVAL;
    hipLaunchKernelGGL(hyp_forward_ard_kernel, dim3(cdiv(d, ANT)), dim3(ANT), 0, ctx->stream, rl, d, rs, rn, ell, hyp);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_hyp_backward_ard(dsvgp_ctx* ctx, const float* rl, int d, const float* rs, const float* rn, const float* d_ell,
                                      const float* dh, float* drl, float* drs, float* drn) {
    if (!ctx || !rl || !rs || !rn || !d_ell || !dh || !drl || !drs || !drn || d < 1) return DSVGP_EINVAL;
    hipLaunchKernelGGL(hyp_backward_ard_kernel, dim3(cdiv(d, ANT)), dim3(ANT), 0, ctx->stream, rl, d, rs, rn, d_ell, dh, drl, drs, drn);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_pack_points_ard(dsvgp_ctx* ctx, const float* x, const float* v, int n, int d, int p, const float* ell,
                                     const float* center, float* P, float* self, float* vnorm) {
    if (!ctx || !x || !ell || !P || !self || n < 0 || d < 1 || p < 0 || p + 1 > AQMAX) return DSVGP_EINVAL;
    if (p > 0 && (!v || !vnorm)) return DSVGP_EINVAL;
    if (n == 0) return 0;
    const int64_t rows = (int64_t)n * (p + 1);
    if (rows > INT_MAX || d > INT_MAX - 64) return DSVGP_EINVAL;
    const int DP = dsvgp_packed_width(d);
    hipLaunchKernelGGL(pack_points_ard_kernel, dim3(cdiv(rows, ANT / 64)), dim3(ANT), 0, ctx->stream, x, v, n, d, p, ell, center, P, self,
                       vnorm, DP - 4, DP);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_kernel_diag_ard(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* hyp, float* out) {
    return kernel_diag_rbf(ctx, P, n, p, d, hyp, out);
}

extern "C" int dsvgp_kernel_diag_ard_bwd(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* ell, const float* hyp,
                                         const float* out, const float* gbar, float* d_ell, float* d_hyp) {
    return kernel_diag_bwd_rbf(ctx, P, n, p, d, ell, hyp, out, gbar, d_ell, d_hyp);
}

extern "C" size_t dsvgp_kernel_bwd_ard_workspace_bytes(int n1, int p1, int n2, int p2, int d) {
    ArdBwdPlan a;
    return ard_bwd_plan(n1, p1, n2, p2, d, a) ? 0 : a.bytes;
}

extern "C" int dsvgp_kernel_bwd_ard_slabs(int n1, int p1, int n2, int p2, int d) {
    ArdBwdPlan a;
    return ard_bwd_plan(n1, p1, n2, p2, d, a) ? 0 : a.t.ns;
}

int kernel_bwd_ard_family(dsvgp_ctx* ctx, TbarLauncher tbar, const void* G, int64_t ldg, int g_is_double, const float* P1,
                          const float* self1, const float* vnorm1, int n1, int p1, const float* P2, const float* self2, int n2, int p2,
                          int d, const float* ell, const float* hyp, int symmetric, float* d_x1, float* d_v1, float* d_ell, float* d_hyp,
                          void* workspace) {
    if (!ctx || !G || !P1 || !self1 || !P2 || !self2 || !ell || !hyp || !d_x1 || !d_hyp || !workspace) return DSVGP_EINVAL;
    if (d_v1 && !vnorm1) return DSVGP_EINVAL;
    if (d < 1 || p1 < 0 || p2 < 0 || p1 + 1 > AQMAX || p2 + 1 > AQMAX || n1 < 0 || n2 < 0) return DSVGP_EINVAL;
    if (symmetric && (n1 != n2 || p1 != p2)) return DSVGP_EINVAL;
    if (n1 == 0 || n2 == 0) return 0;
    ArdBwdPlan a;
    if (int rc = ard_bwd_plan(n1, p1, n2, p2, d, a)) return rc;
    if (((uintptr_t)P1 | (uintptr_t)P2) % 16) return DSVGP_EINVAL;         // the packed rows are read 16 bytes at a time
    if ((uintptr_t)workspace % 4 || (uintptr_t)G % (g_is_double ? 8 : 4)) return DSVGP_EINVAL;
    const TilePlan& t = a.t;
    if (ldg < t.n2q) return DSVGP_EINVAL;
    const int q1 = t.q1, q2 = t.q2, n2q = t.n2q, DP = t.DP, K4 = t.K4, NP = t.NP, ns = t.ns, nparts = t.nparts;
    float *slab, *partials, *TB;
    // launches 1 and 2 of dsvgp_kernel_bwd_rect with the family's Tbar tiles; the scalar lengthscale partial (partials[2 j + 1]) is not read
    if (int rc = launch_kernel_bwd_tiles(ctx->stream, tbar, t, G, ldg, g_is_double, P1, self1, P2, self2, hyp, workspace, &slab, &partials,
                                         &TB))
        return rc;
    float* cs = (float*)((char*)workspace + a.cs_off);
    float* E = (float*)((char*)workspace + a.e_off);
    const float sym = symmetric ? 2.f : 1.f;
    hipLaunchKernelGGL(kernel_bwd_points_ard_kernel, dim3(n1), dim3(ANT), 0, ctx->stream, slab, ns, P1, vnorm1, n1, d, p1, K4, DP, NP, ell, sym,
                       sym, d_x1, p1 > 0 ? d_v1 : nullptr, d_ell ? E : nullptr);
    DSVGP_LAUNCH_CHECK();
    int64_t erows = n1;
    if (d_ell && !symmetric) {
        hipLaunchKernelGGL(tbar_value_colsum_kernel, dim3(cdiv(n2q, ANT)), dim3(ANT), 0, ctx->stream, TB, n1, q1, n2q, cs);
        DSVGP_LAUNCH_CHECK();
        hipLaunchKernelGGL(self2_rows_ard_kernel, dim3(n2), dim3(ANT), 0, ctx->stream, P2, cs, d, q2, DP, E + (size_t)n1 * d);
        DSVGP_LAUNCH_CHECK();
        erows += n2;
    }
    const int nk = d_ell ? d : 0;
    hipLaunchKernelGGL(ard_reduce_kernel, dim3(nk + 1), dim3(ANT), 0, ctx->stream, E, erows, d, nk, ell, partials, nparts, hyp, d_ell, d_hyp);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_kernel_bwd_ard(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1,
                                    const float* vnorm1, int n1, int p1, const float* P2, const float* self2, int n2, int p2, int d,
                                    const float* ell, const float* hyp, int symmetric, float* d_x1, float* d_v1, float* d_ell,
                                    float* d_hyp, void* workspace) {
    return kernel_bwd_ard_family(ctx, launch_kernel_bwd_tbar_rbf, G, ldg, g_is_double, P1, self1, vnorm1, n1, p1, P2, self2, n2, p2, d, ell,
                                 hyp, symmetric, d_x1, d_v1, d_ell, d_hyp, workspace);
}
