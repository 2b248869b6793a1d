// Pathwise posterior samples (include/dsvgp.h, "pathwise posterior samples"): draws of the posterior FUNCTION with exact gradients.
//
// Matheron's rule with a random-Fourier-feature prior: with nu_s = L^-T [m + L_S eps_s - L^-1 (Phi_Z' w_s + sqrt(j) eta_s)] (fp64, per
// parameter state and sample set, formed by the caller) a path is
//     f_s(x)      = c + sum_j w_js phi_j(x) + s sum_i k_i beta_is,           phi_j(x) = sqrt(2 s / F) cos(omega_j . x / ell + b_j)
//     grad f_s(x) = -sum_j w_js sqrt(2 s / F) sin(omega_j . x / ell + b_j) omega_j / ell + (s / ell) sum_i k_i (beta_is r_i + g_is / ell)
// with the update term the posterior mean's closed form (predict_mean.hip) at alpha -> nu_s: a_is = nu_s[i(p+1)], g_is = sum_a
// nu_s[i(p+1)+a] v^_ia, r_i = (z_i - x) / ell, k_i = exp(-|r_i|^2 / 2), beta_is = a_is - r_i . g_is / ell.  k_i, r_i and the sines /
// cosines do not depend on the sample.  Both terms are scaled alike: with wq_js = sqrt(2 / (s F)) w_js and Om_j = omega_j / 2 pi
//     f_s = c + s (sum_i k_i beta_is + sum_j wq_js cos_j),   grad f_s = (s / ell) (sum_i k_i (beta_is r_i + G'_is) + sum_j wq_js (-2 pi sin_j) Om_j)
// so one accumulator per (sample, component) serves both.  The feature table is kept in REVOLUTIONS against x~ = (x - center) / ell (the
// centre's contribution folded into the phase in fp64, reduced mod 1): theta = fract(phase_j + Om_j . x~), then the hardware sine / cosine.
//
// Two routes, one algebra (index arithmetic: paths_plan.h):
//   d <= 32   ONE fused kernel.  A workgroup owns 64 test points (lane = point, x~ and r in registers) and a group of NS samples; its 8
//             waves split the entries of every LDS-staged chunk of inducing points and then of features; the waves' partial sums are
//             added in the fixed order 0, 1, .. 7 through LDS.  The result of (sample, point) is a function of that sample and that
//             point alone: no atomics, no dependence on B, n, the neighbours or the card.
//   d > 32    the same sums in GEMM shape through the caller's workspace on the fp32 MFMA GEMM (unsplit: no floating-point atomics),
//             with pointwise kernels between the products.
// dsvgp_paths_eval_own evaluates sample s at its OWN points x[s] on the same two routes (one sample per workgroup; the n B points as rows
// of one stacked problem with one product per sample), and dsvgp_paths_descend builds a device-resident projected gradient descent of
// every (sample, start) pair on it.
#include "common.h"
#include "paths_plan.h"

namespace {

constexpr float PP_TWO_PI = 6.28318530717958647692f;

__device__ __forceinline__ float wave_sum(float v) {      // butterfly: the same order on every call, the sum in every lane
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- prepare 1: header, centre, Z~, |z~|^2 (one wave per inducing point) and the feature table (one wave per feature) -------------
__global__ __launch_bounds__(256) void paths_prepare_shared_kernel(const double* __restrict__ omega, const double* __restrict__ phase,
                                                                  const float* __restrict__ Z, int M, int d, int F,
                                                                  const float* __restrict__ hyp, const float* __restrict__ constant,
                                                                  const float* __restrict__ center, float* __restrict__ w,
                                                                  PathsWeights L) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wv;
    const float ell = hyp[0];
    if (blockIdx.x == 0) {
        if (threadIdx.x < 8) {
            const float s = hyp[1];
            const float h[8] = {ell, s, constant[0], 1.f / ell, s / ell, 0.f, 0.f, 0.f};
            w[threadIdx.x] = h[threadIdx.x];
        }
        for (int k = threadIdx.x; k < L.ldw; k += 256) w[L.o_center + k] = (k < d && center) ? center[k] : 0.f;
        for (int k = M + threadIdx.x; k < L.Mr; k += 256) w[L.o_nz + k] = 0.f;
        for (int k = F + threadIdx.x; k < L.Fr; k += 256) w[L.o_ph + k] = 0.f;
    }
    if (row < M) {
        float* zr = w + L.o_z + (size_t)row * L.ldw;
        float nz = 0.f;
        for (int k = lane; k < L.ldw; k += 64) {
            const float zt = k < d ? (Z[(size_t)row * d + k] - (center ? center[k] : 0.f)) / ell : 0.f;
            zr[k] = zt;
            nz = __builtin_fmaf(zt, zt, nz);
        }
        nz = wave_sum(nz);
        if (lane == 0) w[L.o_nz + row] = nz;
    } else if (row < M + F) {
        const int j = row - M;
        float* orow = w + L.o_om + (size_t)j * L.ldw;
        const double inv2pi = 0.15915494309189533577;
        double cph = 0.0;
        for (int k = lane; k < L.ldw; k += 64) {
            const double om = k < d ? omega[(size_t)j * d + k] : 0.0;
            orow[k] = (float)(om * inv2pi);
            if (k < d && center) cph += om * (double)center[k];
        }
        cph = wave_sum(cph);
        if (lane == 0) {
            double ph = (phase[j] + cph / (double)ell) * inv2pi;
            ph -= floor(ph);
            w[L.o_ph + j] = (float)ph;
        }
    }
}

// ---- prepare 2: per sample a, a', G' (one wave per (inducing point, sample); g in fp64 from nu and the normalised directions) -----
__global__ __launch_bounds__(256) void paths_prepare_sample_kernel(const double* __restrict__ nu, const float* __restrict__ Z,
                                                                  const float* __restrict__ V, int M, int d, int p,
                                                                  const float* __restrict__ hyp, const float* __restrict__ center,
                                                                  float* __restrict__ w, PathsWeights L) {
    __shared__ double coef[4][PP_MAX_P + 1];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wv, s = blockIdx.y;
    const float ell = hyp[0];
    const double* al = nu + (size_t)s * M * (p + 1);
    if (i < M) {
        for (int a = 0; a < p; ++a) {
            const float* v = V + ((size_t)i * p + a) * d;
            double ss = 0.0;
            for (int k = lane; k < d; k += 64) ss += (double)v[k] * (double)v[k];
            ss = wave_sum(ss);
            if (lane == 0) coef[wv][a] = al[(size_t)i * (p + 1) + 1 + a] / sqrt(ss);
        }
    }
    __syncthreads();
    if (blockIdx.x == 0)
        for (int k = M + threadIdx.x; k < L.Mr; k += 256) {
            w[L.o_a + (size_t)s * L.Mr + k] = 0.f;
            w[L.o_ap + (size_t)s * L.Mr + k] = 0.f;
        }
    if (i >= M) return;
    float* gr = w + L.o_g + ((size_t)s * M + i) * L.ldw;
    float zg = 0.f;
    for (int k = lane; k < L.ldw; k += 64) {
        float zt = 0.f, gp = 0.f;
        if (k < d) {
            zt = (Z[(size_t)i * d + k] - (center ? center[k] : 0.f)) / ell;
            double acc = 0.0;
            for (int a = 0; a < p; ++a) acc += coef[wv][a] * (double)V[((size_t)i * p + a) * d + k];
            gp = (float)(acc / (double)ell);
        }
        gr[k] = gp;
        zg = __builtin_fmaf(zt, gp, zg);
    }
    zg = wave_sum(zg);
    if (lane == 0) {
        const float a = (float)al[(size_t)i * (p + 1)];
        w[L.o_a + (size_t)s * L.Mr + i] = a;
        w[L.o_ap + (size_t)s * L.Mr + i] = a - zg;
    }
}

// ---- prepare 3: wq[s][j] = sqrt(2 / (s F)) w[s][j], zero from F up to Fr -----------------------------------------------------------
__global__ __launch_bounds__(256) void paths_prepare_wq_kernel(const double* __restrict__ wd, int F, int n, const float* __restrict__ hyp,
                                                              float* __restrict__ w, PathsWeights L) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n * L.Fr) return;
    const int s = (int)(t / L.Fr), j = (int)(t - (int64_t)s * L.Fr);
    const double sc = sqrt(2.0 / ((double)hyp[1] * (double)F));
    w[L.o_wq + t] = j < F ? (float)(sc * wd[(size_t)s * F + j]) : 0.f;
}

// ---- fused route (d <= 32): D = pad4(d) = row length of Z~ / G' / Om in the weights -------------------------------------------------
template <int D>
__global__ __launch_bounds__(PP_NW * 64) void paths_fused_kernel(const float* __restrict__ w, PathsWeights L, int M, int d, int F, int n,
                                                                 const float* __restrict__ x, int64_t B, float* __restrict__ values,
                                                                 float* __restrict__ grads) {
    constexpr int NS = paths_ns(D);
    constexpr PathsLds LD = paths_lds(D);
    constexpr int NT = PP_NW * 64;
    __shared__ __align__(16) float lds[LD.floats];
    const int tid = threadIdx.x, lane = tid & 63, slice = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * PP_TP;
    const int64_t b = b0 + lane;
    const int s0 = blockIdx.y * NS;
    const float ell = w[0];
    float xt[D], r[D], acc[NS][D], sig[NS];
#pragma unroll
    for (int k = 0; k < D; ++k) xt[k] = (k < d && b < B) ? (x[b * d + k] - w[L.o_center + k]) / ell : 0.f;
#pragma unroll
    for (int g = 0; g < NS; ++g) {
        sig[g] = 0.f;
#pragma unroll
        for (int k = 0; k < D; ++k) acc[g][k] = 0.f;
    }
    // ---- update term: the inducing points in chunks of PP_CH ----
    for (int c0 = 0; c0 < M; c0 += PP_CH) {
        const int nc = M - c0 < PP_CH ? M - c0 : PP_CH;
        __syncthreads();                                  // the previous chunk has been consumed
        const float4* srcZ = reinterpret_cast<const float4*>(w + L.o_z + (size_t)c0 * D);
        for (int t = tid; t < nc * (D / 4); t += NT) reinterpret_cast<float4*>(lds + LD.o_z)[t] = srcZ[t];
#pragma unroll
        for (int g = 0; g < NS; ++g) {
            const bool live = s0 + g < n;                 // (samples past n: zeros in, nothing out)
            const int sg = live ? s0 + g : 0;
            const float4* srcG = reinterpret_cast<const float4*>(w + L.o_g + ((size_t)sg * M + c0) * D);
            float4* dstG = reinterpret_cast<float4*>(lds + LD.o_g + g * PP_CH * D);
            for (int t = tid; t < nc * (D / 4); t += NT) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (live) v = srcG[t];
                dstG[t] = v;
            }
            if (tid < nc) lds[LD.o_a + g * PP_CH + tid] = live ? w[L.o_a + (size_t)sg * L.Mr + c0 + tid] : 0.f;
        }
        __syncthreads();
        for (int i = slice; i < nc; i += PP_NW) {         // every LDS read below is one address per wave (broadcast)
            const float* z = lds + LD.o_z + i * D;
            float r2 = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                r[k] = z[k] - xt[k];
                r2 = __builtin_fmaf(r[k], r[k], r2);
            }
            const float kk = __expf(-0.5f * r2);
#pragma unroll
            for (int g = 0; g < NS; ++g) {
                const float* gp = lds + LD.o_g + (g * PP_CH + i) * D;
                float rg = 0.f;
#pragma unroll
                for (int k = 0; k < D; ++k) rg = __builtin_fmaf(r[k], gp[k], rg);
                const float P = kk * (lds[LD.o_a + g * PP_CH + i] - rg);      // k_i beta_is
                sig[g] += P;
#pragma unroll
                for (int k = 0; k < D; ++k) acc[g][k] = __builtin_fmaf(P, r[k], __builtin_fmaf(kk, gp[k], acc[g][k]));
            }
        }
    }
    // ---- prior term: the features in chunks of PP_CH ----
    for (int j0 = 0; j0 < F; j0 += PP_CH) {
        const int nf = F - j0 < PP_CH ? F - j0 : PP_CH;
        __syncthreads();
        const float4* srcO = reinterpret_cast<const float4*>(w + L.o_om + (size_t)j0 * D);
        for (int t = tid; t < nf * (D / 4); t += NT) reinterpret_cast<float4*>(lds + LD.o_om)[t] = srcO[t];
        if (tid < nf) lds[LD.o_ph + tid] = w[L.o_ph + j0 + tid];
#pragma unroll
        for (int g = 0; g < NS; ++g) {
            const bool live = s0 + g < n;
            const int sg = live ? s0 + g : 0;
            if (tid < nf) lds[LD.o_w + g * PP_CH + tid] = live ? w[L.o_wq + (size_t)sg * L.Fr + j0 + tid] : 0.f;
        }
        __syncthreads();
        for (int j = slice; j < nf; j += PP_NW) {
            const float* om = lds + LD.o_om + j * D;
            float th = lds[LD.o_ph + j];
#pragma unroll
            for (int k = 0; k < D; ++k) th = __builtin_fmaf(om[k], xt[k], th);
            th = __builtin_amdgcn_fractf(th);
            const float cs = __builtin_amdgcn_cosf(th);
            const float sn = -PP_TWO_PI * __builtin_amdgcn_sinf(th);
#pragma unroll
            for (int g = 0; g < NS; ++g) {
                const float wj = lds[LD.o_w + g * PP_CH + j];
                sig[g] = __builtin_fmaf(wj, cs, sig[g]);
                const float t = wj * sn;
#pragma unroll
                for (int k = 0; k < D; ++k) acc[g][k] = __builtin_fmaf(t, om[k], acc[g][k]);
            }
        }
    }
    // ---- the waves' partial sums, added in the fixed order 0 + 1 + .. + 7 ----
    float* red = lds + LD.o_red;
    for (int s = 1; s < PP_NW; ++s) {
        __syncthreads();
        if (slice == s) {
#pragma unroll
            for (int g = 0; g < NS; ++g) {
#pragma unroll
                for (int k = 0; k < D; ++k) red[(g * PP_TP + lane) * (D + 1) + k] = acc[g][k];
                red[(g * PP_TP + lane) * (D + 1) + D] = sig[g];
            }
        }
        __syncthreads();
        if (slice == 0) {
#pragma unroll
            for (int g = 0; g < NS; ++g) {
#pragma unroll
                for (int k = 0; k < D; ++k) acc[g][k] += red[(g * PP_TP + lane) * (D + 1) + k];
                sig[g] += red[(g * PP_TP + lane) * (D + 1) + D];
            }
        }
    }
    __syncthreads();
    const float sc = w[1], c = w[2], s_ell = w[4];
    if (slice == 0) {
#pragma unroll
        for (int g = 0; g < NS; ++g) {
#pragma unroll
            for (int k = 0; k < D; ++k) red[(g * PP_TP + lane) * (D + 1) + k] = s_ell * acc[g][k];
            red[(g * PP_TP + lane) * (D + 1) + D] = __builtin_fmaf(sc, sig[g], c);
        }
    }
    __syncthreads();
    const int npts = (int)(B - b0 < PP_TP ? B - b0 : PP_TP);
    for (int g = 0; g < NS; ++g) {
        if (s0 + g >= n) break;
        const size_t so = (size_t)(s0 + g) * (size_t)B + (size_t)b0;
        if (tid < npts) values[so + tid] = red[(g * PP_TP + tid) * (D + 1) + D];
        if (grads) {
            for (int t = tid; t < npts * d; t += NT) {
                const int pt = t / d, k = t - pt * d;
                grads[so * d + t] = red[(g * PP_TP + pt) * (D + 1) + k];
            }
        }
    }
}

// ---- composed route (any d) ---------------------------------------------------------------------------------------------------------
// X~ = (x - center) / ell, zero padded to ldw, and |x~|^2: one wave per test point
__global__ __launch_bounds__(256) void paths_pack_x_kernel(const float* __restrict__ w, PathsWeights L, const float* __restrict__ x, int B,
                                                          int d, float* __restrict__ Xt, float* __restrict__ xn) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    const float ell = w[0];
    float acc = 0.f;
    for (int k = lane; k < L.ldw; k += 64) {
        const float v = k < d ? (x[(size_t)row * d + k] - w[L.o_center + k]) / ell : 0.f;
        Xt[(size_t)row * L.ldw + k] = v;
        acc = __builtin_fmaf(v, v, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) xn[row] = acc;
}

// S1 -> k in place (formed once for all samples), zero from M up to ldM
__global__ __launch_bounds__(256) void paths_k_kernel(const float* __restrict__ w, PathsWeights L, int M, int B, float* __restrict__ K,
                                                     int ldM, const float* __restrict__ xn) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * ldM) return;
    const int b = (int)(t / ldM), i = (int)(t - (int64_t)b * ldM);
    float v = 0.f;
    if (i < M) v = __expf(-0.5f * fmaxf(xn[b] + w[L.o_nz + i] - 2.f * K[t], 0.f));
    K[t] = v;
}

// Theta -> C = cos, S = -2 pi sin of theta = fract(Theta + phase) revolutions; zero from F up to ldF
__global__ __launch_bounds__(256) void paths_feature_kernel(const float* __restrict__ w, PathsWeights L, int F, int B, float* __restrict__ Cb,
                                                           float* __restrict__ Sb, int ldF) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * ldF) return;
    const int j = (int)(t % ldF);
    float cs = 0.f, sn = 0.f;
    if (j < F) {
        const float th = __builtin_amdgcn_fractf(Cb[t] + w[L.o_ph + j]);
        cs = __builtin_amdgcn_cosf(th);
        sn = -PP_TWO_PI * __builtin_amdgcn_sinf(th);
    }
    Cb[t] = cs;
    if (Sb) Sb[t] = sn;
}

// P[g][b][i] = k[b][i] (a'_s[i] + S2[b][g M + i]), sigma[g][b] = sum_i P: one workgroup per (test point, sample), fixed-order sums
__global__ __launch_bounds__(256) void paths_pointwise_kernel(const float* __restrict__ w, PathsWeights L, int M, int B, int s0,
                                                             const float* __restrict__ K, int ldM, const float* __restrict__ S2, int ld2,
                                                             float* __restrict__ P, float* __restrict__ sigma, size_t Br) {
    __shared__ float part[4];
    const int b = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const float* ap = w + L.o_ap + (size_t)(s0 + g) * L.Mr;
    const float* Kr = K + (size_t)b * ldM;
    const float* Sr = S2 + (size_t)b * ld2 + (size_t)g * M;
    float* Pr = P + ((size_t)g * B + b) * ldM;
    float acc = 0.f;
    for (int i = tid; i < ldM; i += 256) {
        float v = 0.f;
        if (i < M) v = Kr[i] * (ap[i] + Sr[i]);
        Pr[i] = v;
        acc += v;
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) sigma[(size_t)g * Br + b] = ((part[0] + part[1]) + part[2]) + part[3];
}

// WO[j][g ldw + k] = wq[s0 + g][j] Om[j][k]
__global__ __launch_bounds__(256) void paths_wo_kernel(const float* __restrict__ w, PathsWeights L, int F, int s0, int ng,
                                                      float* __restrict__ WO) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t ldo = (int64_t)ng * L.ldw;
    if (t >= (int64_t)F * ldo) return;
    const int j = (int)(t / ldo), rem = (int)(t - (int64_t)j * ldo), g = rem / L.ldw, k = rem - g * L.ldw;
    WO[t] = w[L.o_wq + (size_t)(s0 + g) * L.Fr + j] * w[L.o_om + (size_t)j * L.ldw + k];
}

// values[s][b] = c + s (sigma + VP), grads[s][b][:] = (s / ell)(O1 + O2 - sigma x~ + GP): one wave per (test point, sample)
__global__ __launch_bounds__(256) void paths_epilogue_kernel(const float* __restrict__ w, PathsWeights L, int B, int d, int s0, int ng,
                                                            const float* __restrict__ Xt, const float* __restrict__ sigma, size_t Br,
                                                            const float* __restrict__ VP, int ldn, const float* __restrict__ O1,
                                                            const float* __restrict__ O2, const float* __restrict__ GP,
                                                            float* __restrict__ values, float* __restrict__ grads) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, g = blockIdx.y;
    if (row >= B) return;
    const float sc = w[1], c = w[2], s_ell = w[4];
    const float sg = sigma[(size_t)g * Br + row];
    const size_t so = (size_t)(s0 + g) * (size_t)B + (size_t)row;
    if (lane == 0) values[so] = __builtin_fmaf(sc, sg + VP[(size_t)row * ldn + s0 + g], c);
    if (!grads) return;
    const float* o1 = O1 + ((size_t)g * B + row) * L.ldw;
    const float* o2 = O2 + ((size_t)g * B + row) * L.ldw;
    const float* gp = GP + (size_t)row * ((size_t)ng * L.ldw) + (size_t)g * L.ldw;
    const float* xr = Xt + (size_t)row * L.ldw;
    for (int k = lane; k < d; k += 64) grads[so * d + k] = s_ell * (((o1[k] + o2[k]) - sg * xr[k]) + gp[k]);
}

template <int D>
int launch_fused(hipStream_t st, const float* w, const PathsWeights& L, int M, int d, int F, int n, const float* x, int B, float* values,
                 float* grads) {
    hipLaunchKernelGGL((paths_fused_kernel<D>), dim3(cdiv(B, PP_TP), cdiv(n, paths_ns(D))), dim3(PP_NW * 64), 0, st, w, L, M, d, F, n, x,
                       (int64_t)B, values, grads);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

// a product of the composed route on the fp32 MFMA GEMM, never split along K (an empty slab: launch_gemm keeps one slice)
int unsplit_gemm(dsvgp_ctx* ctx, int flags, int M, int N, int K, const float* A, int64_t lda, const float* Bm, int64_t ldb, float* C,
                 int64_t ldc) {
    GemmArgs g{};
    g.M = M; g.N = N; g.K = K; g.A = A; g.B = Bm; g.C = C;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.alpha = 1.0; g.beta = 0.0; g.flags = flags; g.batch = 1; g.splitk = 1;
    g.slab = C; g.slab_bytes = 0;
    return launch_gemm(ctx->stream, 0, g);
}

// ---- Hessian-vector products: hv[s][b][:] = grad^2 f_s(x_b) v_b ---------------------------------------------------------------------
//     grad^2 f_s(x) v = (s / ell^2) [ sum_i ((k_i beta_is (r_i.v) + k_i (G'_is.v)) r_i + k_i (r_i.v) G'_is)
//                                     + sum_j wq_js (-4 pi^2 cos_j)(Om_j.v) Om_j - (sum_i k_i beta_is) v ]
// (the gradient's terms differentiated once more: d r / d x~ = -I, grad k = k r, grad beta = G').  r_i.v and Om_j.v do not depend on the
// sample.  Fused route (d <= 32): the structure of paths_fused_kernel<D> with v[D] next to x~[D] and r[D] in the lane's registers and
// NS = paths_hvp_ns(D) samples per group; no sine.  The order of every sum is fixed by M, F and d.
constexpr float PP_M4PI2 = -39.4784176043574344753f;     // -4 pi^2

template <int D>
__global__ __launch_bounds__(PP_NW * 64) void paths_hvp_fused_kernel(const float* __restrict__ w, PathsWeights L, int M, int d, int F, int n,
                                                                     const float* __restrict__ x, const float* __restrict__ vin, int64_t B,
                                                                     float* __restrict__ hv) {
    constexpr int NS = paths_hvp_ns(D);
    constexpr PathsLds LD = paths_hvp_lds(D);
    constexpr int NT = PP_NW * 64;
    __shared__ __align__(16) float lds[LD.floats];
    const int tid = threadIdx.x, lane = tid & 63, slice = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * PP_TP;
    const int64_t b = b0 + lane;
    const int s0 = blockIdx.y * NS;
    const float ell = w[0];
    float xt[D], r[D], v[D], acc[NS][D], sig[NS];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const bool in = k < d && b < B;
        xt[k] = in ? (x[b * d + k] - w[L.o_center + k]) / ell : 0.f;
        v[k] = in ? vin[b * d + k] : 0.f;
    }
#pragma unroll
    for (int g = 0; g < NS; ++g) {
        sig[g] = 0.f;
#pragma unroll
        for (int k = 0; k < D; ++k) acc[g][k] = 0.f;
    }
    // ---- update term: the inducing points in chunks of PP_CH ----
    for (int c0 = 0; c0 < M; c0 += PP_CH) {
        const int nc = M - c0 < PP_CH ? M - c0 : PP_CH;
        __syncthreads();                                  // the previous chunk has been consumed
        const float4* srcZ = reinterpret_cast<const float4*>(w + L.o_z + (size_t)c0 * D);
        for (int t = tid; t < nc * (D / 4); t += NT) reinterpret_cast<float4*>(lds + LD.o_z)[t] = srcZ[t];
#pragma unroll
        for (int g = 0; g < NS; ++g) {
            const bool live = s0 + g < n;                 // (samples past n: zeros in, nothing out)
            const int sg = live ? s0 + g : 0;
            const float4* srcG = reinterpret_cast<const float4*>(w + L.o_g + ((size_t)sg * M + c0) * D);
            float4* dstG = reinterpret_cast<float4*>(lds + LD.o_g + g * PP_CH * D);
            for (int t = tid; t < nc * (D / 4); t += NT) {
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                if (live) q = srcG[t];
                dstG[t] = q;
            }
            if (tid < nc) lds[LD.o_a + g * PP_CH + tid] = live ? w[L.o_a + (size_t)sg * L.Mr + c0 + tid] : 0.f;
        }
        __syncthreads();
        for (int i = slice; i < nc; i += PP_NW) {         // every LDS read below is one address per wave (broadcast)
            const float* z = lds + LD.o_z + i * D;
            float r2 = 0.f, rv = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                r[k] = z[k] - xt[k];
                r2 = __builtin_fmaf(r[k], r[k], r2);
                rv = __builtin_fmaf(r[k], v[k], rv);
            }
            const float kk = __expf(-0.5f * r2);
            const float krv = kk * rv;
#pragma unroll
            for (int g = 0; g < NS; ++g) {
                const float* gp = lds + LD.o_g + (g * PP_CH + i) * D;
                float rg = 0.f, gv = 0.f;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    rg = __builtin_fmaf(r[k], gp[k], rg);
                    gv = __builtin_fmaf(v[k], gp[k], gv);
                }
                const float P = kk * (lds[LD.o_a + g * PP_CH + i] - rg);      // k_i beta_is
                sig[g] += P;
                const float c1 = __builtin_fmaf(P, rv, kk * gv);
#pragma unroll
                for (int k = 0; k < D; ++k) acc[g][k] = __builtin_fmaf(c1, r[k], __builtin_fmaf(krv, gp[k], acc[g][k]));
            }
        }
    }
    // ---- prior term: the features in chunks of PP_CH ----
    for (int j0 = 0; j0 < F; j0 += PP_CH) {
        const int nf = F - j0 < PP_CH ? F - j0 : PP_CH;
        __syncthreads();
        const float4* srcO = reinterpret_cast<const float4*>(w + L.o_om + (size_t)j0 * D);
        for (int t = tid; t < nf * (D / 4); t += NT) reinterpret_cast<float4*>(lds + LD.o_om)[t] = srcO[t];
        if (tid < nf) lds[LD.o_ph + tid] = w[L.o_ph + j0 + tid];
#pragma unroll
        for (int g = 0; g < NS; ++g) {
            const bool live = s0 + g < n;
            const int sg = live ? s0 + g : 0;
            if (tid < nf) lds[LD.o_w + g * PP_CH + tid] = live ? w[L.o_wq + (size_t)sg * L.Fr + j0 + tid] : 0.f;
        }
        __syncthreads();
        for (int j = slice; j < nf; j += PP_NW) {
            const float* om = lds + LD.o_om + j * D;
            float th = lds[LD.o_ph + j], ov = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                th = __builtin_fmaf(om[k], xt[k], th);
                ov = __builtin_fmaf(om[k], v[k], ov);
            }
            th = __builtin_amdgcn_fractf(th);
            const float tc = (PP_M4PI2 * __builtin_amdgcn_cosf(th)) * ov;
#pragma unroll
            for (int g = 0; g < NS; ++g) {
                const float t = lds[LD.o_w + g * PP_CH + j] * tc;
#pragma unroll
                for (int k = 0; k < D; ++k) acc[g][k] = __builtin_fmaf(t, om[k], acc[g][k]);
            }
        }
    }
    // ---- the waves' partial sums, added in the fixed order 0 + 1 + .. + 7 ----
    float* red = lds + LD.o_red;
    for (int s = 1; s < PP_NW; ++s) {
        __syncthreads();
        if (slice == s) {
#pragma unroll
            for (int g = 0; g < NS; ++g) {
#pragma unroll
                for (int k = 0; k < D; ++k) red[(g * PP_TP + lane) * (D + 1) + k] = acc[g][k];
                red[(g * PP_TP + lane) * (D + 1) + D] = sig[g];
            }
        }
        __syncthreads();
        if (slice == 0) {
#pragma unroll
            for (int g = 0; g < NS; ++g) {
#pragma unroll
                for (int k = 0; k < D; ++k) acc[g][k] += red[(g * PP_TP + lane) * (D + 1) + k];
                sig[g] += red[(g * PP_TP + lane) * (D + 1) + D];
            }
        }
    }
    __syncthreads();
    const float s_ell2 = w[4] * w[3];                    // s / ell^2
    if (slice == 0) {
#pragma unroll
        for (int g = 0; g < NS; ++g) {
#pragma unroll
            for (int k = 0; k < D; ++k) red[(g * PP_TP + lane) * (D + 1) + k] = s_ell2 * (acc[g][k] - sig[g] * v[k]);
        }
    }
    __syncthreads();
    const int npts = (int)(B - b0 < PP_TP ? B - b0 : PP_TP);
    for (int g = 0; g < NS; ++g) {
        if (s0 + g >= n) break;
        const size_t so = (size_t)(s0 + g) * (size_t)B + (size_t)b0;
        for (int t = tid; t < npts * d; t += NT) {
            const int pt = t / d, k = t - pt * d;
            hv[so * d + t] = red[(g * PP_TP + pt) * (D + 1) + k];
        }
    }
}

// composed route: V zero padded to ldw and xv = x~ . v: one wave per test point
__global__ __launch_bounds__(256) void paths_hvp_pack_v_kernel(const float* __restrict__ v, int B, int d, int ldw, const float* __restrict__ Xt,
                                                              float* __restrict__ Vp, float* __restrict__ xv) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    float acc = 0.f;
    for (int k = lane; k < ldw; k += 64) {
        const float q = k < d ? v[(size_t)row * d + k] : 0.f;
        Vp[(size_t)row * ldw + k] = q;
        acc = __builtin_fmaf(q, Xt[(size_t)row * ldw + k], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) xv[row] = acc;
}

// V Z~^T -> RV = r . v in place, C2 = k o RV; zero from M up to ldM
__global__ __launch_bounds__(256) void paths_hvp_rv_kernel(int M, int B, const float* __restrict__ K, float* __restrict__ RV,
                                                          float* __restrict__ C2, int ldM, const float* __restrict__ xv) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * ldM) return;
    const int b = (int)(t / ldM), i = (int)(t - (int64_t)b * ldM);
    float rv = 0.f;
    if (i < M) rv = RV[t] - xv[b];
    RV[t] = rv;
    C2[t] = K[t] * rv;
}

// T = -4 pi^2 cos o OV in place of the cosines; zero from F up to ldF
__global__ __launch_bounds__(256) void paths_hvp_t_kernel(int F, int B, float* __restrict__ T, const float* __restrict__ OV, int ldF) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * ldF) return;
    const int j = (int)(t % ldF);
    T[t] = j < F ? (PP_M4PI2 * T[t]) * OV[t] : 0.f;
}

// P = k (a'_s + S2), C1[g][b][i] = P RV + k GV, sigma[g][b] = sum_i P, sigma1[g][b] = sum_i C1: one workgroup per (test point,
// sample), fixed-order sums
__global__ __launch_bounds__(256) void paths_hvp_pointwise_kernel(const float* __restrict__ w, PathsWeights L, int M, int B, int s0,
                                                                 const float* __restrict__ K, const float* __restrict__ RV, int ldM,
                                                                 const float* __restrict__ S2, const float* __restrict__ GV, int ld2,
                                                                 float* __restrict__ C1, float* __restrict__ sigma,
                                                                 float* __restrict__ sigma1, size_t Br) {
    __shared__ float part[8];
    const int b = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const float* ap = w + L.o_ap + (size_t)(s0 + g) * L.Mr;
    const float* Kr = K + (size_t)b * ldM;
    const float* Rr = RV + (size_t)b * ldM;
    const float* Sr = S2 + (size_t)b * ld2 + (size_t)g * M;
    const float* Gr = GV + (size_t)b * ld2 + (size_t)g * M;
    float* Cr = C1 + ((size_t)g * B + b) * ldM;
    float acc = 0.f, acc1 = 0.f;
    for (int i = tid; i < ldM; i += 256) {
        float P = 0.f, c1 = 0.f;
        if (i < M) {
            P = Kr[i] * (ap[i] + Sr[i]);
            c1 = __builtin_fmaf(P, Rr[i], Kr[i] * Gr[i]);
        }
        Cr[i] = c1;
        acc += P;
        acc1 += c1;
    }
    acc = wave_sum(acc);
    acc1 = wave_sum(acc1);
    if ((tid & 63) == 0) {
        part[tid >> 6] = acc;
        part[4 + (tid >> 6)] = acc1;
    }
    __syncthreads();
    if (tid == 0) {
        sigma[(size_t)g * Br + b] = ((part[0] + part[1]) + part[2]) + part[3];
        sigma1[(size_t)g * Br + b] = ((part[4] + part[5]) + part[6]) + part[7];
    }
}

// hv[s][b][:] = (s / ell^2)(O1 + O2 - sigma1 x~ + GP - sigma v): one wave per (test point, sample)
__global__ __launch_bounds__(256) void paths_hvp_epilogue_kernel(const float* __restrict__ w, PathsWeights L, int B, int d, int s0, int ng,
                                                                const float* __restrict__ Xt, const float* __restrict__ Vp,
                                                                const float* __restrict__ sigma, const float* __restrict__ sigma1,
                                                                size_t Br, const float* __restrict__ O1, const float* __restrict__ O2,
                                                                const float* __restrict__ GP, float* __restrict__ hv) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, g = blockIdx.y;
    if (row >= B) return;
    const float s_ell2 = w[4] * w[3];
    const float sg = sigma[(size_t)g * Br + row], sg1 = sigma1[(size_t)g * Br + row];
    const size_t so = (size_t)(s0 + g) * (size_t)B + (size_t)row;
    const float* o1 = O1 + ((size_t)g * B + row) * L.ldw;
    const float* o2 = O2 + ((size_t)g * B + row) * L.ldw;
    const float* gp = GP + (size_t)row * ((size_t)ng * L.ldw) + (size_t)g * L.ldw;
    const float* xr = Xt + (size_t)row * L.ldw;
    const float* vr = Vp + (size_t)row * L.ldw;
    for (int k = lane; k < d; k += 64) hv[so * d + k] = s_ell2 * ((((o1[k] + o2[k]) - sg1 * xr[k]) + gp[k]) - sg * vr[k]);
}

template <int D>
int launch_hvp_fused(hipStream_t st, const float* w, const PathsWeights& L, int M, int d, int F, int n, const float* x, const float* v, int B,
                     float* hv) {
    hipLaunchKernelGGL((paths_hvp_fused_kernel<D>), dim3(cdiv(B, PP_TP), cdiv(n, paths_hvp_ns(D))), dim3(PP_NW * 64), 0, st, w, L, M, d, F,
                       n, x, v, (int64_t)B, hv);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

// ---- own-point evaluation: sample s at its own points x[s][B][d] (dsvgp_paths_eval_own) --------------------------------------------
// Fused route (d <= 32): paths_fused_kernel<D> at ONE sample per workgroup -- grid [point tiles, samples], lane = point, the lane holds
// x~[D], r[D], acc[D] and sig.  The expression sequence of a (sample, point) is the shared-point kernel's; contraction is off so that
// the instance without gradients forms the value from the same operations as the one with them.
template <int D, bool WANT_GRAD>
__global__ __launch_bounds__(PP_NW * 64) void paths_own_fused_kernel(const float* __restrict__ w, PathsWeights L, int M, int d, int F,
                                                                     const float* __restrict__ x, int64_t B, float* __restrict__ values,
                                                                     float* __restrict__ grads) {
#pragma clang fp contract(off)
    constexpr PathsLds LD = paths_own_lds(D);
    constexpr int NT = PP_NW * 64;
    __shared__ __align__(16) float lds[LD.floats];
    const int tid = threadIdx.x, lane = tid & 63, slice = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * PP_TP;
    const int64_t b = b0 + lane;
    const int s = blockIdx.y;
    const size_t so = paths_own_row(s, B, b0);             // first (sample, point) pair of this workgroup
    const float ell = w[0];
    float xt[D], r[D], acc[D], sig = 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        xt[k] = (k < d && b < B) ? (x[(so + lane) * d + k] - w[L.o_center + k]) / ell : 0.f;
        acc[k] = 0.f;
    }
    // ---- update term: the inducing points in chunks of PP_CH ----
    for (int c0 = 0; c0 < M; c0 += PP_CH) {
        const int nc = M - c0 < PP_CH ? M - c0 : PP_CH;
        __syncthreads();                                  // the previous chunk has been consumed
        const float4* srcZ = reinterpret_cast<const float4*>(w + L.o_z + (size_t)c0 * D);
        const float4* srcG = reinterpret_cast<const float4*>(w + L.o_g + ((size_t)s * M + c0) * D);
        for (int t = tid; t < nc * (D / 4); t += NT) {
            reinterpret_cast<float4*>(lds + LD.o_z)[t] = srcZ[t];
            reinterpret_cast<float4*>(lds + LD.o_g)[t] = srcG[t];
        }
        if (tid < nc) lds[LD.o_a + tid] = w[L.o_a + (size_t)s * L.Mr + c0 + tid];
        __syncthreads();
        for (int i = paths_own_first(slice); i < nc; i += PP_NW) {      // every LDS read below is one address per wave (broadcast)
            const float* z = lds + LD.o_z + i * D;
            const float* gp = lds + LD.o_g + i * D;
            float r2 = 0.f, rg = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                r[k] = z[k] - xt[k];
                r2 = __builtin_fmaf(r[k], r[k], r2);
            }
            const float kk = __expf(-0.5f * r2);
#pragma unroll
            for (int k = 0; k < D; ++k) rg = __builtin_fmaf(r[k], gp[k], rg);
            const float P = kk * (lds[LD.o_a + i] - rg);                  // k_i beta_is
            sig += P;
            if (WANT_GRAD) {
#pragma unroll
                for (int k = 0; k < D; ++k) acc[k] = __builtin_fmaf(P, r[k], __builtin_fmaf(kk, gp[k], acc[k]));
            }
        }
    }
    // ---- prior term: the features in chunks of PP_CH ----
    for (int j0 = 0; j0 < F; j0 += PP_CH) {
        const int nf = F - j0 < PP_CH ? F - j0 : PP_CH;
        __syncthreads();
        const float4* srcO = reinterpret_cast<const float4*>(w + L.o_om + (size_t)j0 * D);
        for (int t = tid; t < nf * (D / 4); t += NT) reinterpret_cast<float4*>(lds + LD.o_om)[t] = srcO[t];
        if (tid < nf) {
            lds[LD.o_ph + tid] = w[L.o_ph + j0 + tid];
            lds[LD.o_w + tid] = w[L.o_wq + (size_t)s * L.Fr + j0 + tid];
        }
        __syncthreads();
        for (int j = paths_own_first(slice); j < nf; j += PP_NW) {
            const float* om = lds + LD.o_om + j * D;
            float th = lds[LD.o_ph + j];
#pragma unroll
            for (int k = 0; k < D; ++k) th = __builtin_fmaf(om[k], xt[k], th);
            th = __builtin_amdgcn_fractf(th);
            const float cs = __builtin_amdgcn_cosf(th);
            const float wj = lds[LD.o_w + j];
            sig = __builtin_fmaf(wj, cs, sig);
            if (WANT_GRAD) {
                const float sn = -PP_TWO_PI * __builtin_amdgcn_sinf(th);
                const float t = wj * sn;
#pragma unroll
                for (int k = 0; k < D; ++k) acc[k] = __builtin_fmaf(t, om[k], acc[k]);
            }
        }
    }
    // ---- the waves' partial sums, added in the fixed order 0 + 1 + .. + 7 ----
    float* red = lds + LD.o_red;
    for (int q = 1; q < PP_NW; ++q) {
        __syncthreads();
        if (slice == q) {
            if (WANT_GRAD) {
#pragma unroll
                for (int k = 0; k < D; ++k) red[paths_own_red(lane, k, D)] = acc[k];
            }
            red[paths_own_red(lane, D, D)] = sig;
        }
        __syncthreads();
        if (slice == 0) {
            if (WANT_GRAD) {
#pragma unroll
                for (int k = 0; k < D; ++k) acc[k] += red[paths_own_red(lane, k, D)];
            }
            sig += red[paths_own_red(lane, D, D)];
        }
    }
    __syncthreads();
    const float sc = w[1], c = w[2], s_ell = w[4];
    if (slice == 0) {
        if (WANT_GRAD) {
#pragma unroll
            for (int k = 0; k < D; ++k) red[paths_own_red(lane, k, D)] = s_ell * acc[k];
        }
        red[paths_own_red(lane, D, D)] = __builtin_fmaf(sc, sig, c);
    }
    __syncthreads();
    const int npts = (int)(B - b0 < PP_TP ? B - b0 : PP_TP);
    if (tid < npts) values[so + tid] = red[paths_own_red(tid, D, D)];
    if (WANT_GRAD) {
        for (int t = tid; t < npts * d; t += NT) {
            const int pt = t / d, k = t - pt * d;
            grads[so * d + t] = red[paths_own_red(pt, k, D)];
        }
    }
}

template <int D>
int launch_own_fused(hipStream_t st, const float* w, const PathsWeights& L, int M, int d, int F, int n, const float* x, int B,
                     float* values, float* grads) {
    const dim3 grid(cdiv(B, PP_TP), n), block(PP_NW * 64);
    if (grads) hipLaunchKernelGGL((paths_own_fused_kernel<D, true>), grid, block, 0, st, w, L, M, d, F, x, (int64_t)B, values, grads);
    else hipLaunchKernelGGL((paths_own_fused_kernel<D, false>), grid, block, 0, st, w, L, M, d, F, x, (int64_t)B, values, grads);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

// composed route.  Theta -> the prior's value vp[row] = sum_j cos_j wq_s[j] (fixed order) and, with gradients, T = wq_s o (-2 pi sin)
// in place (zero from F up to ldF): one workgroup per row, s = row / B
__global__ __launch_bounds__(256) void paths_own_feature_kernel(const float* __restrict__ w, PathsWeights L, int F, int B,
                                                               float* __restrict__ T, int ldF, float* __restrict__ vp, int want_grad) {
    __shared__ float part[4];
    const int row = blockIdx.x, tid = threadIdx.x, s = row / B;
    const float* wq = w + L.o_wq + (size_t)s * L.Fr;
    float* Tr = T + (size_t)row * ldF;
    float acc = 0.f;
    for (int j = tid; j < ldF; j += 256) {
        float sn = 0.f;
        if (j < F) {
            const float th = __builtin_amdgcn_fractf(Tr[j] + w[L.o_ph + j]);
            acc = __builtin_fmaf(wq[j], __builtin_amdgcn_cosf(th), acc);
            sn = wq[j] * (-PP_TWO_PI * __builtin_amdgcn_sinf(th));
        }
        if (want_grad) Tr[j] = sn;
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) vp[row] = ((part[0] + part[1]) + part[2]) + part[3];
}

// P[row][i] = k[row][i] (a'_s[i] + S2[row][i]) in place of S2, sigma[row] = sum_i P: one workgroup per row, fixed-order sums
__global__ __launch_bounds__(256) void paths_own_pointwise_kernel(const float* __restrict__ w, PathsWeights L, int M, int B,
                                                                 const float* __restrict__ K, float* __restrict__ P, int ldM,
                                                                 float* __restrict__ sigma) {
    __shared__ float part[4];
    const int row = blockIdx.x, tid = threadIdx.x, s = row / B;
    const float* ap = w + L.o_ap + (size_t)s * L.Mr;
    const float* Kr = K + (size_t)row * ldM;
    float* Pr = P + (size_t)row * ldM;
    float acc = 0.f;
    for (int i = tid; i < ldM; i += 256) {
        float v = 0.f;
        if (i < M) v = Kr[i] * (ap[i] + Pr[i]);
        Pr[i] = v;
        acc += v;
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) sigma[row] = ((part[0] + part[1]) + part[2]) + part[3];
}

// values[row] = c + s (sigma + vp), grads[row][:] = (s / ell)(O1 + O2 - sigma x~ + GP): one wave per row
__global__ __launch_bounds__(256) void paths_own_epilogue_kernel(const float* __restrict__ w, int N, int d, int ldw,
                                                                const float* __restrict__ Xt, const float* __restrict__ sigma,
                                                                const float* __restrict__ vp, const float* __restrict__ O1,
                                                                const float* __restrict__ O2, const float* __restrict__ GP,
                                                                float* __restrict__ values, float* __restrict__ grads) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const float sc = w[1], c = w[2], s_ell = w[4];
    const float sg = sigma[row];
    if (lane == 0) values[row] = __builtin_fmaf(sc, sg + vp[row], c);
    if (!grads) return;
    const size_t o = (size_t)row * ldw;
    for (int k = lane; k < d; k += 64) grads[(size_t)row * d + k] = s_ell * (((O1[o + k] + O2[o + k]) - sg * Xt[o + k]) + GP[o + k]);
}

// ---- device-resident descent (dsvgp_paths_descend; the rule and its constants: paths_plan.h) -------------------------------------------
// x <- clamp(x, lower, upper), elementwise
__global__ __launch_bounds__(256) void paths_descend_clamp_kernel(float* __restrict__ x, int64_t total, int d, const float* __restrict__ lower,
                                                                 const float* __restrict__ upper) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int k = (int)(t % d);
    x[t] = fminf(fmaxf(x[t], lower[k]), upper[k]);
}

// one wave per (sample, start) pair, lanes over the coordinates; the dot product and the norm are a per-lane sum in the order of k and a
// butterfly over the wave.  mode 0: first step length from |g|, accepted = 0; mode 1: nothing (the state is a previous call's);
// mode 2: judge the trial (y, fy, gy) of this iteration and update the pair.  Every mode ends with the proposal of the next iteration
// y = clamp(x - sigma eta g).
__global__ __launch_bounds__(256) void paths_descend_step_kernel(const float* __restrict__ w, int mode, int N, int d, float sgn,
                                                                float initial_step, const float* __restrict__ lower,
                                                                const float* __restrict__ upper, float* __restrict__ x,
                                                                float* __restrict__ f, float* __restrict__ g, float* __restrict__ eta,
                                                                int* __restrict__ accepted, float* __restrict__ y,
                                                                const float* __restrict__ fy, const float* __restrict__ gy) {
    const int pair = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pair >= N) return;
    const size_t o = (size_t)pair * d;
    float step;
    bool take = false;
    if (mode == 0) {
        float nn = 0.f;
        for (int k = lane; k < d; k += 64) nn = __builtin_fmaf(g[o + k], g[o + k], nn);
        nn = wave_sum(nn);
        const float step0 = initial_step > 0.f ? initial_step : PP_DESCEND_STEP0 * w[0];
        step = fminf(step0 / fmaxf(sqrtf(nn), PP_DESCEND_TINY), PP_DESCEND_ETA_MAX);
        if (lane == 0) {
            eta[pair] = step;
            accepted[pair] = 0;
        }
    } else if (mode == 1) {
        step = eta[pair];
    } else {
        float dot = 0.f;
        for (int k = lane; k < d; k += 64) dot = __builtin_fmaf(g[o + k], y[o + k] - x[o + k], dot);
        dot = wave_sum(dot);
        const float f0 = f[pair], f1 = fy[pair];
        take = sgn * f1 <= sgn * f0 + PP_DESCEND_C1 * (sgn * dot);        // (a NaN f1 compares false: rejected)
        step = eta[pair];
        step = take ? fminf(PP_DESCEND_GROW * step, PP_DESCEND_ETA_MAX) : PP_DESCEND_SHRINK * step;
        if (lane == 0) {
            eta[pair] = step;
            if (take) {
                f[pair] = f1;
                accepted[pair] += 1;
            }
        }
    }
    for (int k = lane; k < d; k += 64) {
        float xk = x[o + k], gk = g[o + k];
        if (take) {
            xk = y[o + k];
            gk = gy[o + k];
            x[o + k] = xk;
            g[o + k] = gk;
        }
        y[o + k] = fminf(fmaxf(xk - sgn * (step * gk), lower[k]), upper[k]);
    }
}

bool paths_shape_ok(int M, int d, int F, int n) {
    return M >= 1 && d >= 1 && F >= 1 && n >= 1 && (long long)n * M * paths_pad4(d) <= PP_IDX_MAX * 4 &&
           (long long)F * paths_pad4(d) <= PP_IDX_MAX && (long long)n * paths_pad4(F) <= PP_IDX_MAX;
}

}  // namespace

extern "C" size_t dsvgp_paths_weights_bytes(int M, int d, int F, int n) {
    if (!paths_shape_ok(M, d, F, n)) return 0;
    return paths_weights(M, d, F, n).total * sizeof(float);
}

extern "C" size_t dsvgp_paths_workspace_bytes(int M, int d, int F, int n, int B, int want_grad) {
    if (!paths_shape_ok(M, d, F, n) || B < 1) return 0;
    if (d <= PP_FUSED_MAX_D) return 0;                    // the fused kernel keeps everything in registers and LDS
    PathsWork S;
    if (paths_work(M, d, F, n, B, want_grad != 0, S)) return 0;
    return S.total * sizeof(float);
}

extern "C" int dsvgp_paths_prepare(dsvgp_ctx* ctx, const double* nu, const double* w, const double* omega, const double* phase,
                                   const float* Z, const float* V, int M, int d, int p, int F, int n, const float* hyp,
                                   const float* constant, const float* center, float* weights) {
    if (!ctx || !nu || !w || !omega || !phase || !Z || !hyp || !constant || !weights || !paths_shape_ok(M, d, F, n) || p < 0 ||
        p > PP_MAX_P || (p > 0 && !V) || n > 65535)
        return DSVGP_EINVAL;
    if ((uintptr_t)weights % 16) return DSVGP_EALIGN;
    const PathsWeights L = paths_weights(M, d, F, n);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(paths_prepare_shared_kernel, dim3(cdiv(M + F, 4)), dim3(256), 0, st, omega, phase, Z, M, d, F, hyp, constant,
                       center, weights, L);
    DSVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(paths_prepare_sample_kernel, dim3(cdiv(M, 4), n), dim3(256), 0, st, nu, Z, V, M, d, p, hyp, center, weights, L);
    DSVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(paths_prepare_wq_kernel, dim3(cdiv((int64_t)n * L.Fr, 256)), dim3(256), 0, st, w, F, n, hyp, weights, L);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_paths_eval(dsvgp_ctx* ctx, const float* weights, int M, int d, int F, int n, const float* x, int B, float* values,
                                float* grads, void* workspace) {
    if (!ctx || !weights || !x || !values || !paths_shape_ok(M, d, F, n) || B < 1) return DSVGP_EINVAL;
    if ((int64_t)B * d > PP_IDX_MAX) return DSVGP_EINVAL;
    if ((uintptr_t)weights % 16) return DSVGP_EINVAL;
    const PathsWeights L = paths_weights(M, d, F, n);
    hipStream_t st = ctx->stream;
    if (d <= PP_FUSED_MAX_D) {
        if (cdiv(n, paths_ns(L.ldw)) > 65535) return DSVGP_EINVAL;
        switch (L.ldw) {
            case 4: return launch_fused<4>(st, weights, L, M, d, F, n, x, B, values, grads);
            case 8: return launch_fused<8>(st, weights, L, M, d, F, n, x, B, values, grads);
            case 12: return launch_fused<12>(st, weights, L, M, d, F, n, x, B, values, grads);
            case 16: return launch_fused<16>(st, weights, L, M, d, F, n, x, B, values, grads);
            case 20: return launch_fused<20>(st, weights, L, M, d, F, n, x, B, values, grads);
            case 24: return launch_fused<24>(st, weights, L, M, d, F, n, x, B, values, grads);
            case 28: return launch_fused<28>(st, weights, L, M, d, F, n, x, B, values, grads);
            default: return launch_fused<32>(st, weights, L, M, d, F, n, x, B, values, grads);
        }
    }
    if (!workspace || (uintptr_t)workspace % 16) return DSVGP_EINVAL;
    PathsWork S;
    if (paths_work(M, d, F, n, B, grads != nullptr, S)) return DSVGP_EINVAL;       // (an intermediate past 2^31 entries: split the batch)
    float* ws = (float*)workspace;
    float *Xt = ws + S.o_x, *xn = ws + S.o_xn, *K = ws + S.o_k, *Cb = ws + S.o_c, *VP = ws + S.o_vp, *Sb = grads ? ws + S.o_s : nullptr;
    float *S2 = ws + S.o_s2, *P = ws + S.o_p, *sig = ws + S.o_sig, *O1 = ws + S.o_o1, *O2 = ws + S.o_o2, *WO = ws + S.o_wo, *GP = ws + S.o_gp;
    const float *Zt = weights + L.o_z, *Om = weights + L.o_om, *WQ = weights + L.o_wq, *G = weights + L.o_g;
    const int KP = DSVGP_GEMM_TRANS_B | DSVGP_GEMM_K_PADDED;
    hipLaunchKernelGGL(paths_pack_x_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, weights, L, x, B, d, Xt, xn);
    DSVGP_LAUNCH_CHECK();
    // S1 = X~ Z~^T -> k (once for all samples)
    if (int rc = unsplit_gemm(ctx, KP, B, M, d, Xt, S.ldw, Zt, L.ldw, K, S.ldM)) return rc;
    hipLaunchKernelGGL(paths_k_kernel, dim3(cdiv((int64_t)B * S.ldM, 256)), dim3(256), 0, st, weights, L, M, B, K, S.ldM, xn);
    DSVGP_LAUNCH_CHECK();
    // Theta = X~ Om^T -> C, S (once for all samples); the prior's values for all samples: VP = C WQ^T
    if (int rc = unsplit_gemm(ctx, KP, B, F, d, Xt, S.ldw, Om, L.ldw, Cb, S.ldF)) return rc;
    hipLaunchKernelGGL(paths_feature_kernel, dim3(cdiv((int64_t)B * S.ldF, 256)), dim3(256), 0, st, weights, L, F, B, Cb, Sb, S.ldF);
    DSVGP_LAUNCH_CHECK();
    if (int rc = unsplit_gemm(ctx, KP, B, n, F, Cb, S.ldF, WQ, L.Fr, VP, S.ldn)) return rc;
    for (int s0 = 0; s0 < n; s0 += S.ng) {
        const int ng = n - s0 < S.ng ? n - s0 : S.ng;
        // S2 = X~ G'_group^T
        if (int rc = unsplit_gemm(ctx, KP, B, ng * M, d, Xt, S.ldw, G + (size_t)s0 * M * L.ldw, L.ldw, S2, S.ld2)) return rc;
        hipLaunchKernelGGL(paths_pointwise_kernel, dim3(B, ng), dim3(256), 0, st, weights, L, M, B, s0, K, S.ldM, S2, S.ld2, P, sig, S.Br);
        DSVGP_LAUNCH_CHECK();
        if (grads) {
            // O1 = P Z~ for the whole group, O2_s = k G'_s per sample, GP = S WO with WO = wq_s o Om
            if (int rc = unsplit_gemm(ctx, 0, ng * B, d, M, P, S.ldM, Zt, L.ldw, O1, S.ldw)) return rc;
            for (int g = 0; g < ng; ++g)
                if (int rc = unsplit_gemm(ctx, 0, B, d, M, K, S.ldM, G + (size_t)(s0 + g) * M * L.ldw, L.ldw, O2 + (size_t)g * B * S.ldw,
                                          S.ldw))
                    return rc;
            hipLaunchKernelGGL(paths_wo_kernel, dim3(cdiv((int64_t)F * ng * L.ldw, 256)), dim3(256), 0, st, weights, L, F, s0, ng, WO);
            DSVGP_LAUNCH_CHECK();
            if (int rc = unsplit_gemm(ctx, 0, B, ng * L.ldw, F, Sb, S.ldF, WO, (int64_t)ng * L.ldw, GP, (int64_t)ng * L.ldw)) return rc;
        }
        hipLaunchKernelGGL(paths_epilogue_kernel, dim3(cdiv(B, 4), ng), dim3(256), 0, st, weights, L, B, d, s0, ng, Xt, sig, S.Br, VP,
                           S.ldn, O1, O2, GP, values, grads);
        DSVGP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" size_t dsvgp_paths_hvp_workspace_bytes(int M, int d, int F, int n, int B) {
    if (!paths_shape_ok(M, d, F, n) || B < 1) return 0;
    if (d <= PP_FUSED_MAX_D) return 0;                    // the fused kernel keeps everything in registers and LDS
    PathsHvpWork S;
    if (paths_hvp_work(M, d, F, n, B, S)) return 0;
    return S.total * sizeof(float);
}

extern "C" int dsvgp_paths_hvp(dsvgp_ctx* ctx, const float* weights, int M, int d, int F, int n, const float* x, const float* v, int B,
                               float* hv, void* workspace) {
    if (!ctx || !weights || !x || !v || !hv || !paths_shape_ok(M, d, F, n) || B < 1) return DSVGP_EINVAL;
    if ((int64_t)B * d > PP_IDX_MAX) return DSVGP_EINVAL;
    if ((uintptr_t)weights % 16) return DSVGP_EINVAL;
    const PathsWeights L = paths_weights(M, d, F, n);
    hipStream_t st = ctx->stream;
    if (d <= PP_FUSED_MAX_D) {
        if (cdiv(n, paths_hvp_ns(L.ldw)) > 65535) return DSVGP_EINVAL;
        switch (L.ldw) {
            case 4: return launch_hvp_fused<4>(st, weights, L, M, d, F, n, x, v, B, hv);
            case 8: return launch_hvp_fused<8>(st, weights, L, M, d, F, n, x, v, B, hv);
            case 12: return launch_hvp_fused<12>(st, weights, L, M, d, F, n, x, v, B, hv);
            case 16: return launch_hvp_fused<16>(st, weights, L, M, d, F, n, x, v, B, hv);
            case 20: return launch_hvp_fused<20>(st, weights, L, M, d, F, n, x, v, B, hv);
            case 24: return launch_hvp_fused<24>(st, weights, L, M, d, F, n, x, v, B, hv);
            case 28: return launch_hvp_fused<28>(st, weights, L, M, d, F, n, x, v, B, hv);
            default: return launch_hvp_fused<32>(st, weights, L, M, d, F, n, x, v, B, hv);
        }
    }
    if (!workspace || (uintptr_t)workspace % 16) return DSVGP_EINVAL;
    PathsHvpWork S;
    if (paths_hvp_work(M, d, F, n, B, S)) return DSVGP_EINVAL;                       // (an intermediate past 2^31 entries: split the batch)
    float* ws = (float*)workspace;
    float *Xt = ws + S.o_x, *Vp = ws + S.o_v, *xn = ws + S.o_xn, *xv = ws + S.o_xv, *K = ws + S.o_k, *RV = ws + S.o_rv, *C2 = ws + S.o_c2;
    float *T = ws + S.o_t, *OV = ws + S.o_ov, *S2 = ws + S.o_s2, *GV = ws + S.o_gv, *C1 = ws + S.o_c1, *sig = ws + S.o_sig;
    float *sig1 = ws + S.o_sig1, *O1 = ws + S.o_o1, *O2 = ws + S.o_o2, *WO = ws + S.o_wo, *GP = ws + S.o_gp;
    const float *Zt = weights + L.o_z, *Om = weights + L.o_om, *G = weights + L.o_g;
    const int KP = DSVGP_GEMM_TRANS_B | DSVGP_GEMM_K_PADDED;
    hipLaunchKernelGGL(paths_pack_x_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, weights, L, x, B, d, Xt, xn);
    DSVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(paths_hvp_pack_v_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, v, B, d, S.ldw, Xt, Vp, xv);
    DSVGP_LAUNCH_CHECK();
    // S1 = X~ Z~^T -> k;  V Z~^T -> RV = r . v, C2 = k o RV (once for all samples)
    if (int rc = unsplit_gemm(ctx, KP, B, M, d, Xt, S.ldw, Zt, L.ldw, K, S.ldM)) return rc;
    hipLaunchKernelGGL(paths_k_kernel, dim3(cdiv((int64_t)B * S.ldM, 256)), dim3(256), 0, st, weights, L, M, B, K, S.ldM, xn);
    DSVGP_LAUNCH_CHECK();
    if (int rc = unsplit_gemm(ctx, KP, B, M, d, Vp, S.ldw, Zt, L.ldw, RV, S.ldM)) return rc;
    hipLaunchKernelGGL(paths_hvp_rv_kernel, dim3(cdiv((int64_t)B * S.ldM, 256)), dim3(256), 0, st, M, B, K, RV, C2, S.ldM, xv);
    DSVGP_LAUNCH_CHECK();
    // Theta = X~ Om^T -> cos;  OV = V Om^T;  T = -4 pi^2 cos o OV (once for all samples)
    if (int rc = unsplit_gemm(ctx, KP, B, F, d, Xt, S.ldw, Om, L.ldw, T, S.ldF)) return rc;
    hipLaunchKernelGGL(paths_feature_kernel, dim3(cdiv((int64_t)B * S.ldF, 256)), dim3(256), 0, st, weights, L, F, B, T, (float*)nullptr,
                       S.ldF);
    DSVGP_LAUNCH_CHECK();
    if (int rc = unsplit_gemm(ctx, KP, B, F, d, Vp, S.ldw, Om, L.ldw, OV, S.ldF)) return rc;
    hipLaunchKernelGGL(paths_hvp_t_kernel, dim3(cdiv((int64_t)B * S.ldF, 256)), dim3(256), 0, st, F, B, T, OV, S.ldF);
    DSVGP_LAUNCH_CHECK();
    for (int s0 = 0; s0 < n; s0 += S.ng) {
        const int ng = n - s0 < S.ng ? n - s0 : S.ng;
        const float* Gg = G + (size_t)s0 * M * L.ldw;
        // S2 = X~ G'_group^T, GV = V G'_group^T
        if (int rc = unsplit_gemm(ctx, KP, B, ng * M, d, Xt, S.ldw, Gg, L.ldw, S2, S.ld2)) return rc;
        if (int rc = unsplit_gemm(ctx, KP, B, ng * M, d, Vp, S.ldw, Gg, L.ldw, GV, S.ld2)) return rc;
        hipLaunchKernelGGL(paths_hvp_pointwise_kernel, dim3(B, ng), dim3(256), 0, st, weights, L, M, B, s0, K, RV, S.ldM, S2, GV, S.ld2, C1,
                           sig, sig1, S.Br);
        DSVGP_LAUNCH_CHECK();
        // O1 = C1 Z~ for the whole group, O2_s = C2 G'_s per sample, GP = T WO with WO = wq_s o Om
        if (int rc = unsplit_gemm(ctx, 0, ng * B, d, M, C1, S.ldM, Zt, L.ldw, O1, S.ldw)) return rc;
        for (int g = 0; g < ng; ++g)
            if (int rc = unsplit_gemm(ctx, 0, B, d, M, C2, S.ldM, G + (size_t)(s0 + g) * M * L.ldw, L.ldw, O2 + (size_t)g * B * S.ldw, S.ldw))
                return rc;
        hipLaunchKernelGGL(paths_wo_kernel, dim3(cdiv((int64_t)F * ng * L.ldw, 256)), dim3(256), 0, st, weights, L, F, s0, ng, WO);
        DSVGP_LAUNCH_CHECK();
        if (int rc = unsplit_gemm(ctx, 0, B, ng * L.ldw, F, T, S.ldF, WO, (int64_t)ng * L.ldw, GP, (int64_t)ng * L.ldw)) return rc;
        hipLaunchKernelGGL(paths_hvp_epilogue_kernel, dim3(cdiv(B, 4), ng), dim3(256), 0, st, weights, L, B, d, s0, ng, Xt, Vp, sig, sig1,
                           S.Br, O1, O2, GP, hv);
        DSVGP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" size_t dsvgp_paths_own_workspace_bytes(int M, int d, int F, int n, int B, int want_grad) {
    if (!paths_shape_ok(M, d, F, n) || B < 1 || n > 65535) return 0;
    if (d <= PP_FUSED_MAX_D) return 0;                    // the fused kernel keeps everything in registers and LDS
    PathsOwnWork S;
    if (paths_own_work(M, d, F, n, B, want_grad != 0, S)) return 0;
    return S.total * sizeof(float);
}

extern "C" int dsvgp_paths_eval_own(dsvgp_ctx* ctx, const float* weights, int M, int d, int F, int n, const float* x, int B, float* values,
                                    float* grads, void* workspace) {
    if (!ctx || !weights || !x || !values || !paths_shape_ok(M, d, F, n) || B < 1 || n > 65535) return DSVGP_EINVAL;
    if ((int64_t)n * B * d > PP_IDX_MAX) return DSVGP_EINVAL;
    if ((uintptr_t)weights % 16) return DSVGP_EINVAL;
    const PathsWeights L = paths_weights(M, d, F, n);
    hipStream_t st = ctx->stream;
    if (d <= PP_FUSED_MAX_D) {
        switch (L.ldw) {
            case 4: return launch_own_fused<4>(st, weights, L, M, d, F, n, x, B, values, grads);
            case 8: return launch_own_fused<8>(st, weights, L, M, d, F, n, x, B, values, grads);
            case 12: return launch_own_fused<12>(st, weights, L, M, d, F, n, x, B, values, grads);
            case 16: return launch_own_fused<16>(st, weights, L, M, d, F, n, x, B, values, grads);
            case 20: return launch_own_fused<20>(st, weights, L, M, d, F, n, x, B, values, grads);
            case 24: return launch_own_fused<24>(st, weights, L, M, d, F, n, x, B, values, grads);
            case 28: return launch_own_fused<28>(st, weights, L, M, d, F, n, x, B, values, grads);
            default: return launch_own_fused<32>(st, weights, L, M, d, F, n, x, B, values, grads);
        }
    }
    if (!workspace || (uintptr_t)workspace % 16) return DSVGP_EINVAL;
    PathsOwnWork S;
    if (paths_own_work(M, d, F, n, B, grads != nullptr, S)) return DSVGP_EINVAL;    // (an intermediate past 2^31 entries: split the points)
    float* ws = (float*)workspace;
    float *Xt = ws + S.o_x, *xn = ws + S.o_xn, *K = ws + S.o_k, *T = ws + S.o_t, *vp = ws + S.o_vp, *P = ws + S.o_p, *sig = ws + S.o_sig;
    float *O1 = ws + S.o_o1, *O2 = ws + S.o_o2, *GP = ws + S.o_gp;
    const float *Zt = weights + L.o_z, *Om = weights + L.o_om, *G = weights + L.o_g;
    const int KP = DSVGP_GEMM_TRANS_B | DSVGP_GEMM_K_PADDED;
    const int N = (int)S.N;
    // all n B points as the rows of one X~
    hipLaunchKernelGGL(paths_pack_x_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, weights, L, x, N, d, Xt, xn);
    DSVGP_LAUNCH_CHECK();
    // S1 = X~ Z~^T -> k, stacked
    if (int rc = unsplit_gemm(ctx, KP, N, M, d, Xt, S.ldw, Zt, L.ldw, K, S.ldM)) return rc;
    hipLaunchKernelGGL(paths_k_kernel, dim3(cdiv((int64_t)N * S.ldM, 256)), dim3(256), 0, st, weights, L, M, N, K, S.ldM, xn);
    DSVGP_LAUNCH_CHECK();
    // Theta = X~ Om^T, stacked -> the prior's value (a fixed-order row dot with wq_s) and wq_s o S in place
    if (int rc = unsplit_gemm(ctx, KP, N, F, d, Xt, S.ldw, Om, L.ldw, T, S.ldF)) return rc;
    hipLaunchKernelGGL(paths_own_feature_kernel, dim3(N), dim3(256), 0, st, weights, L, F, B, T, S.ldF, vp, grads ? 1 : 0);
    DSVGP_LAUNCH_CHECK();
    // S2_s = X~_s G'_s^T: one product per sample on its row block; P = k o (a'_s + S2_s) and its row sums in place
    for (int s = 0; s < n; ++s)
        if (int rc = unsplit_gemm(ctx, KP, B, M, d, Xt + (size_t)s * B * S.ldw, S.ldw, G + (size_t)s * M * L.ldw, L.ldw,
                                  P + (size_t)s * B * S.ldM, S.ldM))
            return rc;
    hipLaunchKernelGGL(paths_own_pointwise_kernel, dim3(N), dim3(256), 0, st, weights, L, M, B, K, P, S.ldM, sig);
    DSVGP_LAUNCH_CHECK();
    if (grads) {
        // O1 = P Z~ stacked, O2_s = K_s G'_s per sample, GP = (wq_s o S) Om stacked
        if (int rc = unsplit_gemm(ctx, 0, N, d, M, P, S.ldM, Zt, L.ldw, O1, S.ldw)) return rc;
        for (int s = 0; s < n; ++s)
            if (int rc = unsplit_gemm(ctx, 0, B, d, M, K + (size_t)s * B * S.ldM, S.ldM, G + (size_t)s * M * L.ldw, L.ldw,
                                      O2 + (size_t)s * B * S.ldw, S.ldw))
                return rc;
        if (int rc = unsplit_gemm(ctx, 0, N, d, F, T, S.ldF, Om, L.ldw, GP, S.ldw)) return rc;
    }
    hipLaunchKernelGGL(paths_own_epilogue_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, weights, N, d, S.ldw, Xt, sig, vp, O1, O2, GP, values,
                       grads);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t dsvgp_paths_descend_workspace_bytes(int M, int d, int F, int n, int B) {
    if (!paths_shape_ok(M, d, F, n) || B < 1 || n > 65535) return 0;
    PathsDescendWork S;
    if (paths_descend_work(M, d, F, n, B, S)) return 0;
    return S.total * sizeof(float);
}

extern "C" int dsvgp_paths_descend(dsvgp_ctx* ctx, const float* weights, int M, int d, int F, int n, float* x, int B, const float* lower,
                                   const float* upper, int iterations, float initial_step, int maximize, int resume, float* values,
                                   float* grads, float* steps, int* accepted, void* workspace) {
    if (!ctx || !weights || !x || !lower || !upper || !values || !grads || !steps || !accepted || !workspace || iterations < 0 ||
        !paths_shape_ok(M, d, F, n) || B < 1 || n > 65535)
        return DSVGP_EINVAL;
    if ((uintptr_t)weights % 16 || (uintptr_t)workspace % 16) return DSVGP_EINVAL;
    PathsDescendWork S;
    if (paths_descend_work(M, d, F, n, B, S)) return DSVGP_EINVAL;
    float* ws = (float*)workspace;
    float *y = ws + S.o_y, *gy = ws + S.o_gy, *fy = ws + S.o_fy;
    void* evw = d <= PP_FUSED_MAX_D ? nullptr : (void*)(ws + S.o_eval);
    const int N = n * B;
    const float sgn = maximize ? -1.f : 1.f;
    hipStream_t st = ctx->stream;
    auto step = [&](int mode) {
        hipLaunchKernelGGL(paths_descend_step_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, weights, mode, N, d, sgn, initial_step, lower, upper,
                           x, values, grads, steps, accepted, y, fy, gy);
    };
    if (!resume) {
        hipLaunchKernelGGL(paths_descend_clamp_kernel, dim3(cdiv((int64_t)N * d, 256)), dim3(256), 0, st, x, (int64_t)N * d, d, lower, upper);
        DSVGP_LAUNCH_CHECK();
        if (int rc = dsvgp_paths_eval_own(ctx, weights, M, d, F, n, x, B, values, grads, evw)) return rc;
    }
    step(resume ? 1 : 0);
    DSVGP_LAUNCH_CHECK();
    for (int t = 0; t < iterations; ++t) {
        if (int rc = dsvgp_paths_eval_own(ctx, weights, M, d, F, n, y, B, fy, gy, evw)) return rc;
        step(2);
        DSVGP_LAUNCH_CHECK();
    }
    return 0;
}
