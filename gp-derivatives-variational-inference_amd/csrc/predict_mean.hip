// Posterior-mean predictor of a frozen model: mean and gradient without K_ZX or a solve (include/dsvgp.h, "posterior mean").
//
// With alpha = L^-T m (fp64, one transposed solve per parameter state) the predictive mean of the Cholesky-whitened strategy
// (reference DirectionalGradVariationalStrategy.py:181-188: mu = K_XZ L^-T m + c) needs none of the [M', B'] work: the p
// directional weights of inducing point i collapse into one d-vector g_i = sum_s alpha[i(p+1)+1+s] v^_is, and with
// r_i = (z_i - x) / ell, k_i = exp(-|r_i|^2 / 2), beta_i = alpha[i(p+1)] - (r_i . g_i) / ell
//     mu_f(x)      = c + s sum_i k_i beta_i
//     grad mu_f(x) = (s / ell) sum_i k_i (beta_i r_i + g_i / ell)
//     row of direction w at x = c + w^ . grad mu_f(x)                         (RBFKernelDirectionalGrad.py:57-58,83-107; DGVS.py:126)
// an attention-shaped pass (scores -> pointwise -> weighted sum of "values") without a normaliser.
//
// Two paths, one algebra:
//   d <= 32   ONE fused kernel.  A workgroup owns 64 test points (lane = point) and its 8 waves split the inducing points of every
//             LDS-staged chunk among them; the [point, d] accumulator and sigma stay in registers; the waves' partial sums are
//             added in the fixed order wave 0, 1, .. 7 through LDS; the direction rows and both outputs leave through contiguous
//             stores.  The two small products (r . g and the weighted sum) are VALU FMAs on the DIFFERENCE r = z~ - x~: with K = d
//             <= 32 an fp32-input MFMA (which runs at the vector rate on gfx950) would only move the same flops to the matrix
//             pipe at the price of the expansion |x~|^2 + |z~|^2 - 2 x~.z~ and its cancellation; every LDS read of the loop is a
//             wave-wide broadcast of one inducing point, so the LDS is not the limit either.
//   d > 32    the same sums in GEMM shape through [B, 2M] intermediates in the caller's workspace: [S1 | S2] = X~ [Z~ ; G']^T on
//             the existing fp32 MFMA GEMM, one pointwise kernel ([P | k] in place, sigma = P 1 in a fixed-order tree), the
//             [B, 2M] x [2M, d] product, one epilogue kernel.  The products run UNSPLIT (no split-K atomics).
// No floating-point atomics anywhere; two identical calls give bitwise identical results.
#include "common.h"

namespace {

constexpr int MP_FUSED_MAX_D = 32;   // the fused kernel's bound on d (packed width dsvgp_packed_width(d) <= 36)
constexpr int MP_TP = 64;            // test points per workgroup of the fused kernel (one per lane)
constexpr int MP_NS = 8;             // waves per workgroup = slices of every chunk of inducing points
constexpr int MP_CH = 64;            // inducing points per LDS chunk
constexpr int MP_MAX_P = 95;         // directions per inducing point (the bound of dsvgp_pack_points)

inline int pad4(int v) { return (v + 3) & ~3; }

// packed weights (floats): hdr[8] = {ell, s, c, 1/ell, s/ell, 0, 0, 0} | center[ldw] | a[Mr] | a'[Mr] = a - z~.G' | nz[Mr] = |z~|^2 |
// ZG[2M][ldw] = [Z~ ; G'] with G' = g / ell; ldw = pad4(d), Mr = pad4(M); padding columns are zero
struct WLayout { int ldw, Mr; size_t o_center, o_a, o_ap, o_nz, o_zg, total; };
inline WLayout wlayout(int M, int d) {
    WLayout w;
    w.ldw = pad4(d); w.Mr = pad4(M);
    w.o_center = 8; w.o_a = w.o_center + w.ldw; w.o_ap = w.o_a + w.Mr; w.o_nz = w.o_ap + w.Mr; w.o_zg = w.o_nz + w.Mr;
    w.total = w.o_zg + (size_t)2 * M * w.ldw;
    return w;
}
// composed-path workspace (floats): X~[B][ldw] | out[B][ldw] | xn[Br] | sigma[Br] | W[B][ldW], ldW = pad4(2M), Br = pad4(B)
struct SLayout { int ldw, ldW; size_t o_x, o_out, o_xn, o_sig, o_W, total; };
inline SLayout slayout(int M, int d, int B) {
    SLayout s;
    s.ldw = pad4(d); s.ldW = pad4(2 * M);
    const size_t Br = (size_t)pad4(B);
    s.o_x = 0; s.o_out = (size_t)B * s.ldw; s.o_xn = s.o_out + (size_t)B * s.ldw; s.o_sig = s.o_xn + Br; s.o_W = s.o_sig + Br;
    s.total = s.o_W + (size_t)B * s.ldW;
    return s;
}

__device__ __forceinline__ float wave_sum(float v) {      // butterfly: the same order on every call, the sum in every lane
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- prepare: one wave per inducing point; g_i in fp64 from alpha and the normalised directions, then the fp32 weights --------
__global__ __launch_bounds__(256) void mean_prepare_kernel(const double* __restrict__ alpha, const float* __restrict__ Z,
                                                          const float* __restrict__ V, int M, int d, int p,
                                                          const float* __restrict__ hyp, const float* __restrict__ constant,
                                                          const float* __restrict__ center, float* __restrict__ w, WLayout L) {
    __shared__ double coef[4][MP_MAX_P + 1];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wv;
    const float ell = hyp[0];
    if (blockIdx.x == 0) {
        if (threadIdx.x < 8) {
            const float s = hyp[1];
            const float h[8] = {ell, s, constant[0], 1.f / ell, s / ell, 0.f, 0.f, 0.f};
            w[threadIdx.x] = h[threadIdx.x];
        }
        for (int k = threadIdx.x; k < L.ldw; k += 256) w[L.o_center + k] = (k < d && center) ? center[k] : 0.f;
    }
    if (i < M) {                                          // alpha_s / |v_is|: one wave reduction per direction
        for (int s = 0; s < p; ++s) {
            const float* v = V + ((size_t)i * p + s) * d;
            double ss = 0.0;
            for (int k = lane; k < d; k += 64) ss += (double)v[k] * (double)v[k];
            ss = wave_sum(ss);
            if (lane == 0) coef[wv][s] = alpha[(size_t)i * (p + 1) + 1 + s] / sqrt(ss);
        }
    }
    __syncthreads();
    if (i >= M) return;
    float* zr = w + L.o_zg + (size_t)i * L.ldw;
    float* gr = w + L.o_zg + (size_t)(M + i) * L.ldw;
    float nz = 0.f, zg = 0.f;
    for (int k = lane; k < L.ldw; k += 64) {
        float zt = 0.f, gp = 0.f;
        if (k < d) {
            zt = (Z[(size_t)i * d + k] - (center ? center[k] : 0.f)) / ell;
            double acc = 0.0;
            for (int s = 0; s < p; ++s) acc += coef[wv][s] * (double)V[((size_t)i * p + s) * d + k];
            gp = (float)(acc / (double)ell);
        }
        zr[k] = zt;
        gr[k] = gp;
        nz = __builtin_fmaf(zt, zt, nz);
        zg = __builtin_fmaf(zt, gp, zg);
    }
    nz = wave_sum(nz);
    zg = wave_sum(zg);
    if (lane == 0) {
        const float a = (float)alpha[(size_t)i * (p + 1)];
        w[L.o_a + i] = a;
        w[L.o_ap + i] = a - zg;
        w[L.o_nz + i] = nz;
    }
}

// ---- fused path (d <= 32): D = pad4(d) = row length of Z~ / G' in the weights --------------------------------------------------
template <int D>
__global__ __launch_bounds__(MP_NS * 64) void mean_fused_kernel(const float* __restrict__ w, WLayout L, int M, int d,
                                                                const float* __restrict__ x, int64_t B,
                                                                const float* __restrict__ Dir, int pd,
                                                                float* __restrict__ mean_out, float* __restrict__ grad_out) {
    __shared__ __align__(16) float sZ[MP_CH * D];
    __shared__ __align__(16) float sG[MP_CH * D];
    __shared__ float sA[MP_CH];
    __shared__ float sRed[MP_TP * (D + 1)];
    __shared__ float sMu[MP_TP];
    const int tid = threadIdx.x, lane = tid & 63, slice = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * MP_TP;
    const int64_t b = b0 + lane;
    const float ell = w[0];
    float xt[D], acc[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        xt[k] = (k < d && b < B) ? (x[b * d + k] - w[L.o_center + k]) / ell : 0.f;
        acc[k] = 0.f;
    }
    float sig = 0.f;
    for (int c0 = 0; c0 < M; c0 += MP_CH) {
        const int nc = M - c0 < MP_CH ? M - c0 : MP_CH;
        __syncthreads();                                  // the previous chunk has been consumed
        const float4* srcZ = reinterpret_cast<const float4*>(w + L.o_zg + (size_t)c0 * D);
        const float4* srcG = reinterpret_cast<const float4*>(w + L.o_zg + (size_t)(M + c0) * D);
        for (int t = tid; t < nc * (D / 4); t += MP_NS * 64) {
            reinterpret_cast<float4*>(sZ)[t] = srcZ[t];
            reinterpret_cast<float4*>(sG)[t] = srcG[t];
        }
        if (tid < nc) sA[tid] = w[L.o_a + c0 + tid];
        __syncthreads();
        for (int i = slice; i < nc; i += MP_NS) {         // every LDS read below is one address per wave (broadcast)
            const float* z = sZ + i * D;
            const float* g = sG + i * D;
            float r2 = 0.f, rg = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const float r = z[k] - xt[k];
                r2 = __builtin_fmaf(r, r, r2);
                rg = __builtin_fmaf(r, g[k], rg);
            }
            const float kk = __expf(-0.5f * r2);
            const float P = kk * (sA[i] - rg);            // k_i beta_i
            sig += P;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const float r = z[k] - xt[k];
                acc[k] = __builtin_fmaf(P, r, __builtin_fmaf(kk, g[k], acc[k]));
            }
        }
    }
    // the waves' partial sums, added in the fixed order 0 + 1 + .. + 7
    for (int s = 1; s < MP_NS; ++s) {
        __syncthreads();
        if (slice == s) {
#pragma unroll
            for (int k = 0; k < D; ++k) sRed[lane * (D + 1) + k] = acc[k];
            sRed[lane * (D + 1) + D] = sig;
        }
        __syncthreads();
        if (slice == 0) {
#pragma unroll
            for (int k = 0; k < D; ++k) acc[k] += sRed[lane * (D + 1) + k];
            sig += sRed[lane * (D + 1) + D];
        }
    }
    __syncthreads();
    const float sc = w[1], c = w[2], s_ell = w[4];
    if (slice == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) sRed[lane * (D + 1) + k] = s_ell * acc[k];
        sMu[lane] = c + sc * sig;
    }
    __syncthreads();
    const int npts = (int)(B - b0 < MP_TP ? B - b0 : MP_TP);
    if (grad_out) {
        for (int t = tid; t < npts * d; t += MP_NS * 64) {
            const int pt = t / d, k = t - pt * d;
            grad_out[b0 * d + t] = sRed[pt * (D + 1) + k];
        }
    }
    const int qd = pd + 1;
    for (int t = tid; t < npts * qd; t += MP_NS * 64) {
        const int pt = t / qd, j = t - pt * qd;
        float v = sMu[pt];
        if (j > 0) {
            const float* wd = Dir + ((b0 + pt) * pd + (j - 1)) * d;
            float dot = 0.f, ss = 0.f;
            for (int k = 0; k < d; ++k) {
                dot = __builtin_fmaf(wd[k], sRed[pt * (D + 1) + k], dot);
                ss = __builtin_fmaf(wd[k], wd[k], ss);
            }
            v = c + dot / sqrtf(ss);
        }
        mean_out[b0 * qd + t] = v;
    }
}

// ---- composed path (any d) -----------------------------------------------------------------------------------------------------
// X~ = (x - center) / ell, zero padded to ldw, and |x~|^2: one wave per test point
__global__ __launch_bounds__(256) void mean_pack_x_kernel(const float* __restrict__ w, WLayout L, const float* __restrict__ x, int B,
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

// [S1 | S2] -> [P | k] in place, sigma = sum_i P_i: one workgroup per test point, fixed-order sums
__global__ __launch_bounds__(256) void mean_pointwise_kernel(const float* __restrict__ w, WLayout L, int M, float* __restrict__ W,
                                                            int ldW, const float* __restrict__ xn, float* __restrict__ sigma) {
    __shared__ float part[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    float* Wr = W + (size_t)b * ldW;
    const float xnb = xn[b];
    float acc = 0.f;
    for (int i = tid; i < M; i += 256) {
        const float S1 = Wr[i], S2 = Wr[M + i];
        const float r2 = fmaxf(xnb + w[L.o_nz + i] - 2.f * S1, 0.f);
        const float kk = __expf(-0.5f * r2);
        const float P = kk * (w[L.o_ap + i] + S2);
        Wr[i] = P;
        Wr[M + i] = kk;
        acc += P;
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) sigma[b] = ((part[0] + part[1]) + part[2]) + part[3];
}

// out = P Z~ + k G' -> grad = (s / ell)(out - sigma x~), mu = c + s sigma, direction rows: one wave per test point
__global__ __launch_bounds__(256) void mean_epilogue_kernel(const float* __restrict__ w, WLayout L, int B, int d,
                                                           const float* __restrict__ Xt, float* __restrict__ out,
                                                           const float* __restrict__ sigma, const float* __restrict__ Dir, int pd,
                                                           float* __restrict__ mean_out, float* __restrict__ grad_out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    const float sc = w[1], c = w[2], s_ell = w[4], sg = sigma[row];
    float* o = out + (size_t)row * L.ldw;
    const float* xr = Xt + (size_t)row * L.ldw;
    for (int k = lane; k < d; k += 64) {                  // (lane reads back below only what it wrote here)
        const float gk = s_ell * (o[k] - sg * xr[k]);
        o[k] = gk;
        if (grad_out) grad_out[(size_t)row * d + k] = gk;
    }
    const int qd = pd + 1;
    if (lane == 0) mean_out[(size_t)row * qd] = c + sc * sg;
    for (int j = 0; j < pd; ++j) {
        const float* wd = Dir + ((size_t)row * pd + j) * d;
        float dot = 0.f, ss = 0.f;
        for (int k = lane; k < d; k += 64) {
            dot = __builtin_fmaf(wd[k], o[k], dot);
            ss = __builtin_fmaf(wd[k], wd[k], ss);
        }
        dot = wave_sum(dot);
        ss = wave_sum(ss);
        if (lane == 0) mean_out[(size_t)row * qd + 1 + j] = c + dot / sqrtf(ss);
    }
}

template <int D>
int launch_fused(hipStream_t st, const float* w, const WLayout& L, int M, int d, const float* x, int B, const float* Dir, int pd,
                 float* mean_out, float* grad_out) {
    hipLaunchKernelGGL((mean_fused_kernel<D>), dim3(cdiv(B, MP_TP)), dim3(MP_NS * 64), 0, st, w, L, M, d, x, (int64_t)B, Dir, pd,
                       mean_out, grad_out);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

// a product of the composed path on the fp32 MFMA GEMM, never split along K (an empty slab: launch_gemm keeps one slice)
int unsplit_gemm(dsvgp_ctx* ctx, int flags, int M, int N, int K, const float* A, int64_t lda, const float* Bm, int64_t ldb, float* C,
                 int64_t ldc) {
    GemmArgs g{};
    g.M = M; g.N = N; g.K = K; g.A = A; g.B = Bm; g.C = C;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.alpha = 1.0; g.beta = 0.0; g.flags = flags; g.batch = 1; g.splitk = 1;
    g.slab = C; g.slab_bytes = 0;
    return launch_gemm(ctx->stream, 0, g);
}

}  // namespace

extern "C" size_t dsvgp_mean_weights_bytes(int M, int d) {
    if (M < 1 || d < 1) return 0;
    return wlayout(M, d).total * sizeof(float);
}

extern "C" size_t dsvgp_mean_workspace_bytes(int M, int d, int B, int pd) {
    if (M < 1 || d < 1 || B < 1 || pd < 0) return 0;
    if (d <= MP_FUSED_MAX_D) return 0;                    // the fused kernel keeps everything in registers and LDS
    return slayout(M, d, B).total * sizeof(float);
}

extern "C" int dsvgp_mean_prepare(dsvgp_ctx* ctx, const double* alpha, const float* Z, const float* V, int M, int d, int p,
                                  const float* hyp, const float* constant, const float* center, float* weights) {
    if (!ctx || !alpha || !Z || !hyp || !constant || !weights || M < 1 || d < 1 || p < 0 || p > MP_MAX_P || (p > 0 && !V))
        return DSVGP_EINVAL;
    if ((uintptr_t)weights % 16) return DSVGP_EALIGN;
    const WLayout L = wlayout(M, d);
    hipLaunchKernelGGL(mean_prepare_kernel, dim3(cdiv(M, 4)), dim3(256), 0, ctx->stream, alpha, Z, V, M, d, p, hyp, constant, center,
                       weights, L);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_mean_predict(dsvgp_ctx* ctx, const float* weights, int M, int d, const float* x, int B, const float* D, int pd,
                                  float* mean_out, float* grad_out, void* workspace) {
    if (!ctx || !weights || !x || !mean_out || M < 1 || d < 1 || B < 1 || pd < 0 || (pd > 0 && !D)) return DSVGP_EINVAL;
    if ((int64_t)B * (pd + 1) >= ((int64_t)1 << 31) || (int64_t)B * d >= ((int64_t)1 << 31)) return DSVGP_EINVAL;
    if ((uintptr_t)weights % 16) return DSVGP_EALIGN;
    const WLayout L = wlayout(M, d);
    hipStream_t st = ctx->stream;
    if (d <= MP_FUSED_MAX_D) {
        switch (L.ldw) {
            case 4: return launch_fused<4>(st, weights, L, M, d, x, B, D, pd, mean_out, grad_out);
            case 8: return launch_fused<8>(st, weights, L, M, d, x, B, D, pd, mean_out, grad_out);
            case 12: return launch_fused<12>(st, weights, L, M, d, x, B, D, pd, mean_out, grad_out);
            case 16: return launch_fused<16>(st, weights, L, M, d, x, B, D, pd, mean_out, grad_out);
            case 20: return launch_fused<20>(st, weights, L, M, d, x, B, D, pd, mean_out, grad_out);
            case 24: return launch_fused<24>(st, weights, L, M, d, x, B, D, pd, mean_out, grad_out);
            case 28: return launch_fused<28>(st, weights, L, M, d, x, B, D, pd, mean_out, grad_out);
            default: return launch_fused<32>(st, weights, L, M, d, x, B, D, pd, mean_out, grad_out);
        }
    }
    if (!workspace) return DSVGP_EINVAL;
    if ((uintptr_t)workspace % 16) return DSVGP_EALIGN;
    const SLayout S = slayout(M, d, B);
    if ((int64_t)B * S.ldW >= ((int64_t)1 << 31) || (int64_t)B * S.ldw >= ((int64_t)1 << 31)) return DSVGP_EINVAL;   // (split the batch)
    float* ws = (float*)workspace;
    float *Xt = ws + S.o_x, *out = ws + S.o_out, *xn = ws + S.o_xn, *sig = ws + S.o_sig, *W = ws + S.o_W;
    const float* ZG = weights + L.o_zg;
    hipLaunchKernelGGL(mean_pack_x_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, weights, L, x, B, d, Xt, xn);
    DSVGP_LAUNCH_CHECK();
    // [S1 | S2] = X~ [Z~ ; G']^T  (both operands k-contiguous, zero-filled from d up to ldw)
    if (int rc = unsplit_gemm(ctx, DSVGP_GEMM_TRANS_B | DSVGP_GEMM_K_PADDED, B, 2 * M, d, Xt, S.ldw, ZG, L.ldw, W, S.ldW)) return rc;
    hipLaunchKernelGGL(mean_pointwise_kernel, dim3(B), dim3(256), 0, st, weights, L, M, W, S.ldW, xn, sig);
    DSVGP_LAUNCH_CHECK();
    // out = [P | k] [Z~ ; G']
    if (int rc = unsplit_gemm(ctx, 0, B, d, 2 * M, W, S.ldW, ZG, L.ldw, out, S.ldw)) return rc;
    hipLaunchKernelGGL(mean_epilogue_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, weights, L, B, d, Xt, out, sig, D, pd, mean_out,
                       grad_out);
    DSVGP_LAUNCH_CHECK();
    return 0;
}
