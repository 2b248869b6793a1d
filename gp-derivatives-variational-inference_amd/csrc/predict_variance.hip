// Posterior variance of a frozen model with its gradient, the confidence-bound / expected-improvement acquisitions on it and their
// device-resident descent (include/dsvgp.h, "posterior variance").
//
// Cholesky-whitened strategy, value rows (reference DirectionalGradVariationalStrategy.py:188-205): with K~ = s K_ZZ + j I = L L^T,
// S = L_S L_S^T, k(x) = s K_Z'x and Q = L^-T (S - I) L^-1 (fp64, symmetric, ONCE per parameter state)
//     v(x) = Q k(x),   sigma^2(x) = s + 1e-4 + k(x) . v(x),   grad sigma^2(x) = 2 (dk/dx)^T v(x)
// grad sigma^2 is the mean predictor's gradient sum (csrc/predict_mean.hip) with PER-POINT weights: a_ib = v[i(p+1), b], g_ib =
// sum_s v[i(p+1)+1+s, b] v^_is, r = (z_i - x_b) / ell, k = exp(-|r|^2 / 2), beta_ib = a_ib - (r . g_ib) / ell:
//     sigma^2_b = s + 1e-4 + s sum_i k beta_ib,   grad sigma^2_b = 2 (s / ell) sum_i k (beta_ib r + g_ib / ell)
// Q and the product V = Q K_ZX stay in float64 (Q rounded to fp32 loses three digits of sigma^2: the sum cancels); V leaves the fp64
// MFMA GEMM rounded once to fp32 and everything after it is fp32.
//
// One batch: K_ZX [M', B] by dsvgp_pack_points + dsvgp_kernel_fwd_rect (data side p = 0), V on the fp64 GEMM with the float right
// operand, UNSPLIT (no split-K atomics), then
//   fused     (d <= 32 and a chunk of >= 8 inducing points with their directions fits 48 KB of LDS: vp_chunk) ONE kernel of
//             mean_fused_kernel's structure: a workgroup owns 64 test points (lane = point), its 8 waves slice every staged chunk, the
//             lane's weights come from V[:, b] (rows of V are contiguous in b: coalesced), partial sums added in the order 0..7.
//   composed  one kernel for sigma^2 = s + 1e-4 + colsum(K_ZX o V) (fixed-order row slices, fixed-order combine) that also writes
//             G = 2 V^T through an LDS tile, then dsvgp_kernel_bwd_rect(G, side 1 = the x pack, side 2 = the inducing pack).
// No floating-point atomics anywhere; two identical calls give bitwise identical results.
#include "common.h"
#include "variance_plan.h"

namespace {

__device__ __forceinline__ float wave_sum(float v) {      // butterfly: the same order on every call, the sum in every lane
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- prepare: one wave per inducing point ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void var_prepare_kernel(const float* __restrict__ Z, const float* __restrict__ V, int M, int d, int p,
                                                         const float* __restrict__ hyp, const float* __restrict__ center,
                                                         float* __restrict__ w, VpWeights L) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wv;
    const float ell = hyp[0];
    if (blockIdx.x == 0) {
        if (threadIdx.x < 8) {
            const float s = hyp[1];
            const float h[8] = {ell, s, 1.f / ell, s / ell, 0.f, 0.f, 0.f, 0.f};
            w[threadIdx.x] = h[threadIdx.x];
        }
        for (int k = threadIdx.x; k < L.ldw; k += 256) w[L.o_center + k] = (k < d && center) ? center[k] : 0.f;
    }
    if (i >= M) return;
    float* zr = w + L.o_z + (size_t)i * L.ldw;
    for (int k = lane; k < L.ldw; k += 64) zr[k] = k < d ? (Z[(size_t)i * d + k] - (center ? center[k] : 0.f)) / ell : 0.f;
    for (int s = 0; s < p; ++s) {
        const float* v = V + ((size_t)i * p + s) * d;
        double ss = 0.0;
        for (int k = lane; k < d; k += 64) ss += (double)v[k] * (double)v[k];
        ss = sqrt(wave_sum(ss));
        float* ur = w + L.o_u + ((size_t)i * p + s) * L.ldw;
        for (int k = lane; k < L.ldw; k += 64) ur[k] = k < d ? (float)((double)v[k] / ss) : 0.f;
    }
}

// ---- fused route: D = pad4(d) = row length of Z~ / U in the weights; GRAD: the d accumulators of the gradient ----------------------
template <int D, bool GRAD>
__global__ __launch_bounds__(VP_NW * 64) void var_fused_kernel(const float* __restrict__ w, VpWeights L, int M, int d, int p, int CH,
                                                               const float* __restrict__ x, int B, const float* __restrict__ V, int ldk,
                                                               float* __restrict__ var_out, float* __restrict__ grad_out) {
    extern __shared__ __align__(16) float vp_lds[];       // Z~[CH][D] | U[CH][p][D]
    __shared__ float sRed[VP_TP * (D + 1)];
    float* sZ = vp_lds;
    float* sU = vp_lds + CH * D;
    const int tid = threadIdx.x, lane = tid & 63, slice = tid >> 6;
    const int b0 = blockIdx.x * VP_TP;
    const int b = b0 + lane;
    const int bi = b < B ? b : B - 1;                     // (a lane past the batch reads the last column and stores nothing)
    const float ell = w[0], inv_ell = w[2];
    float xt[D], acc[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        xt[k] = (k < d && b < B) ? (x[(size_t)b * d + k] - w[L.o_center + k]) / ell : 0.f;
        acc[k] = 0.f;
    }
    float sig = 0.f;
    for (int c0 = 0; c0 < M; c0 += CH) {
        const int nc = M - c0 < CH ? M - c0 : CH;
        __syncthreads();                                  // the previous chunk has been consumed
        const float4* srcZ = reinterpret_cast<const float4*>(w + L.o_z + (size_t)c0 * D);
        const float4* srcU = reinterpret_cast<const float4*>(w + L.o_u + (size_t)c0 * p * D);
        for (int t = tid; t < nc * (D / 4); t += VP_NW * 64) reinterpret_cast<float4*>(sZ)[t] = srcZ[t];
        for (int t = tid; t < nc * p * (D / 4); t += VP_NW * 64) reinterpret_cast<float4*>(sU)[t] = srcU[t];
        __syncthreads();
        for (int i = slice; i < nc; i += VP_NW) {         // every LDS read below is one address per wave (broadcast)
            const float* z = sZ + i * D;
            const size_t row = (size_t)(c0 + i) * (p + 1);
            const float a = V[row * ldk + bi];
            float g[D];
#pragma unroll
            for (int k = 0; k < D; ++k) g[k] = 0.f;
            for (int s = 0; s < p; ++s) {
                const float vs = V[(row + 1 + s) * ldk + bi];
                const float* u = sU + (i * p + s) * D;
#pragma unroll
                for (int k = 0; k < D; ++k) g[k] = __builtin_fmaf(vs, u[k], g[k]);
            }
            float r2 = 0.f, rg = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const float r = z[k] - xt[k];
                r2 = __builtin_fmaf(r, r, r2);
                rg = __builtin_fmaf(r, g[k], rg);
            }
            const float kk = __expf(-0.5f * r2);
            const float beta = __builtin_fmaf(-rg, inv_ell, a);
            sig = __builtin_fmaf(kk, beta, sig);
            if (GRAD) {
                const float P = kk * beta, kg = kk * inv_ell;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const float r = z[k] - xt[k];
                    acc[k] = __builtin_fmaf(P, r, __builtin_fmaf(kg, g[k], acc[k]));
                }
            }
        }
    }
    // the waves' partial sums, added in the fixed order 0 + 1 + .. + 7
    for (int s = 1; s < VP_NW; ++s) {
        __syncthreads();
        if (slice == s) {
            if (GRAD) {
#pragma unroll
                for (int k = 0; k < D; ++k) sRed[lane * (D + 1) + k] = acc[k];
            }
            sRed[lane * (D + 1) + D] = sig;
        }
        __syncthreads();
        if (slice == 0) {
            if (GRAD) {
#pragma unroll
                for (int k = 0; k < D; ++k) acc[k] += sRed[lane * (D + 1) + k];
            }
            sig += sRed[lane * (D + 1) + D];
        }
    }
    __syncthreads();
    const float sc = w[1], s_ell2 = 2.f * w[3];
    if (slice == 0) {
        if (GRAD) {
#pragma unroll
            for (int k = 0; k < D; ++k) sRed[lane * (D + 1) + k] = s_ell2 * acc[k];
        }
        if (b < B) var_out[b] = __builtin_fmaf(sc, sig, sc + VP_KXX_JITTER);
    }
    if (GRAD) {
        __syncthreads();
        const int npts = B - b0 < VP_TP ? B - b0 : VP_TP;
        for (int t = tid; t < npts * d; t += VP_NW * 64) {
            const int pt = t / d, k = t - pt * d;
            grad_out[(size_t)b0 * d + t] = sRed[pt * (D + 1) + k];
        }
    }
}

// ---- composed route ----------------------------------------------------------------------------------------------------------------
// grid (column tiles of 64 points, row slices of VP_RS rows): part[slice][b] = sum over the slice's rows of K_ZX o V -- per wave in the
// order of its rows (wave w: rows w, w + 4, ..), the four waves added in the order 0..3 -- and, with G, G[b][i'] = 2 V[i'][b]
__global__ __launch_bounds__(256) void var_reduce_kernel(const float* __restrict__ K, const float* __restrict__ V, int Mp, int B, int ldk,
                                                        float* __restrict__ part, float* __restrict__ G, int ldg) {
    __shared__ float tile[VP_TILE][VP_TILE + 1];
    __shared__ float red[4][VP_TILE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b0 = blockIdx.x * VP_TILE, b = b0 + lane;
    const int r0 = blockIdx.y * VP_RS, r1 = r0 + VP_RS < Mp ? r0 + VP_RS : Mp;
    float acc = 0.f;
    for (int i0 = r0; i0 < r1; i0 += VP_TILE) {
        for (int j = wv; j < VP_TILE; j += 4) {
            const int i = i0 + j;
            float v = 0.f, kz = 0.f;
            if (i < r1 && b < B) {
                v = V[(size_t)i * ldk + b];
                kz = K[(size_t)i * ldk + b];
            }
            acc = __builtin_fmaf(kz, v, acc);
            if (G) tile[j][lane] = v;
        }
        if (G) {
            __syncthreads();
            const int i = i0 + lane;
            for (int bb = wv; bb < VP_TILE; bb += 4)
                if (b0 + bb < B && i < r1) G[(size_t)(b0 + bb) * ldg + i] = 2.f * tile[lane][bb];
            __syncthreads();
        }
    }
    red[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && b < B) part[(size_t)blockIdx.y * ldk + b] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// sigma^2[b] = s + 1e-4 + sum over the row slices in the order 0, 1, ..
__global__ __launch_bounds__(256) void var_combine_kernel(const float* __restrict__ part, int ns, int B, int ldk, const float* __restrict__ hyp,
                                                         float* __restrict__ var_out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float acc = 0.f;
    for (int s = 0; s < ns; ++s) acc += part[(size_t)s * ldk + b];
    var_out[b] = (hyp[1] + VP_KXX_JITTER) + acc;
}

// ---- acquisition: one wave per point, lanes over the coordinates -------------------------------------------------------------------
// stated for minimisation; sgn = -1 (maximize) mirrors the model: mu -> -mu, best -> -best
__global__ __launch_bounds__(256) void acq_eval_kernel(int kind, float sgn, const float* __restrict__ beta_p, const float* __restrict__ best_p,
                                                      const float* __restrict__ mu, const float* __restrict__ gmu,
                                                      const float* __restrict__ var, const float* __restrict__ gvar, int B, int d,
                                                      float* __restrict__ out, float* __restrict__ gout) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const float m = sgn * mu[b], s2 = var[b];
    float val, cm, cv;                                    // value, and the gradient as cm * sgn * grad mu + cv * grad sigma^2
    if (kind == VP_ACQ_LCB_VAR) {
        const float beta = beta_p[0];
        val = __builtin_fmaf(-beta, s2, m);
        cm = 1.f;
        cv = -beta;
    } else {
        const bool clamped = !(s2 > VP_MIN_VAR);
        const float sd = sqrtf(clamped ? VP_MIN_VAR : s2);
        const float ds = clamped ? 0.f : 0.5f / sd;       // d sigma / d sigma^2 (0 where sigma^2 is clamped)
        if (kind == VP_ACQ_LCB) {
            const float beta = beta_p[0];
            val = __builtin_fmaf(-beta, sd, m);
            cm = 1.f;
            cv = -beta * ds;
        } else {
            const float imp = sgn * best_p[0] - m;
            const float z = imp / sd;
            const float Phi = 0.5f * erfcf(-z * 0.70710678118654752f);
            const float phi = 0.39894228040143268f * __expf(-0.5f * z * z);
            val = -__builtin_fmaf(imp, Phi, sd * phi);
            cm = Phi;
            cv = -phi * ds;
        }
    }
    if (lane == 0) out[b] = val;
    if (gout) {
        cm *= sgn;
        for (int k = lane; k < d; k += 64) gout[(size_t)b * d + k] = __builtin_fmaf(cm, gmu[(size_t)b * d + k], cv * gvar[(size_t)b * d + k]);
    }
}

// ---- descent (the rule of dsvgp_paths_descend with n = 1; its constants, csrc/paths_plan.h) ----------------------------------------
constexpr float AD_C1 = 1e-4f, AD_GROW = 2.f, AD_SHRINK = 0.5f, AD_ETA_MAX = 1e30f, AD_TINY = 1e-30f, AD_STEP0 = 0.25f;

__global__ __launch_bounds__(256) void acq_clamp_kernel(float* __restrict__ x, int64_t total, int d, const float* __restrict__ lower,
                                                       const float* __restrict__ upper) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int k = (int)(t % d);
    x[t] = fminf(fmaxf(x[t], lower[k]), upper[k]);
}

// one wave per start, lanes over the coordinates; fixed-order wave sums.  mode 0: first step length from |g|, accepted = 0; mode 1:
// nothing (the state is a previous call's); mode 2: judge the trial (y, fy, gy) and update the start.  Every mode ends with the proposal
// of the next iteration y = clamp(x - eta g).  The acquisition is always minimised.
__global__ __launch_bounds__(256) void acq_step_kernel(const float* __restrict__ w, int mode, int N, int d, float initial_step,
                                                      const float* __restrict__ lower, const float* __restrict__ upper,
                                                      float* __restrict__ x, float* __restrict__ f, float* __restrict__ g,
                                                      float* __restrict__ eta, int* __restrict__ accepted, float* __restrict__ y,
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
        const float step0 = initial_step > 0.f ? initial_step : AD_STEP0 * w[0];
        step = fminf(step0 / fmaxf(sqrtf(nn), AD_TINY), AD_ETA_MAX);
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
        take = f1 <= f0 + AD_C1 * dot;                    // (a NaN f1 compares false: rejected)
        step = eta[pair];
        step = take ? fminf(AD_GROW * step, AD_ETA_MAX) : AD_SHRINK * step;
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
        y[o + k] = fminf(fmaxf(xk - step * gk, lower[k]), upper[k]);
    }
}

template <int D>
int launch_fused(hipStream_t st, const float* w, const VpWeights& L, int M, int d, int p, const float* x, int B, const float* V, int ldk,
                 float* var_out, float* grad_out) {
    const int CH = vp_chunk(d, p);
    const size_t lds = vp_fused_lds(d, p);
    const dim3 grid(cdiv(B, VP_TP)), block(VP_NW * 64);
    if (grad_out) hipLaunchKernelGGL((var_fused_kernel<D, true>), grid, block, lds, st, w, L, M, d, p, CH, x, B, V, ldk, var_out, grad_out);
    else hipLaunchKernelGGL((var_fused_kernel<D, false>), grid, block, lds, st, w, L, M, d, p, CH, x, B, V, ldk, var_out, grad_out);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

size_t bwd_bytes_for(int M, int d, int p, int B, int want_grad) {
    return (want_grad && vp_route(d, p) == 2) ? dsvgp_kernel_bwd_rect_workspace_bytes(B, 0, M, p, d) : 0;
}

}  // namespace

extern "C" int dsvgp_var_route(int d, int p) { return vp_route(d, p); }
extern "C" int dsvgp_var_chunk(int d, int p) { return vp_chunk(d, p); }

extern "C" size_t dsvgp_var_weights_bytes(int M, int d, int p) {
    VpWeights L;
    return vp_weights(M, d, p, &L) ? L.total * sizeof(float) : 0;
}

extern "C" size_t dsvgp_var_workspace_bytes(int M, int d, int p, int B, int want_grad) {
    VpWork S;
    if (M < 1 || d < 1 || p < 0 || p > VP_MAX_P || B < 1) return 0;
    return vp_work(M, d, p, B, want_grad != 0, bwd_bytes_for(M, d, p, B, want_grad), &S) ? S.total * sizeof(float) : 0;
}

extern "C" int dsvgp_var_prepare(dsvgp_ctx* ctx, const float* Z, const float* V, int M, int d, int p, const float* hyp, const float* center,
                                 float* weights) {
    VpWeights L;
    if (!ctx || !Z || !hyp || !weights || (p > 0 && !V) || !vp_weights(M, d, p, &L)) return DSVGP_EINVAL;
    if ((uintptr_t)weights % 16) return DSVGP_EALIGN;
    hipLaunchKernelGGL(var_prepare_kernel, dim3(cdiv(M, 4)), dim3(256), 0, ctx->stream, Z, V, M, d, p, hyp, center, weights, L);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_var_predict(dsvgp_ctx* ctx, const float* weights, const double* Q, int64_t ldq, const float* PZ, const float* selfZ,
                                 const float* hyp, int M, int d, int p, const float* x, int B, float* var_out, float* grad_out,
                                 void* workspace) {
    VpWeights L;
    VpWork S;
    if (!ctx || !weights || !Q || !PZ || !selfZ || !hyp || !x || !var_out || !workspace || B < 1 || !vp_weights(M, d, p, &L))
        return DSVGP_EINVAL;
    if ((int64_t)B * d > VP_IDX_MAX) return DSVGP_EINVAL;
    if (!vp_work(M, d, p, B, grad_out != nullptr, bwd_bytes_for(M, d, p, B, grad_out != nullptr), &S)) return DSVGP_EINVAL;   // (split the batch)
    if (ldq < S.Mp) return DSVGP_EINVAL;
    if ((uintptr_t)weights % 16 || (uintptr_t)workspace % 16 || (uintptr_t)PZ % 16 || (uintptr_t)Q % 8) return DSVGP_EALIGN;
    hipStream_t st = ctx->stream;
    float* ws = (float*)workspace;
    float *PX = ws + S.o_px, *sX = ws + S.o_sx, *KZX = ws + S.o_k, *V32 = ws + S.o_v;
    // 1. K_ZX [M', B]: the data side carries no directions (value rows only), packed with the centre the inducing pack was made with
    if (int rc = dsvgp_pack_points(ctx, x, nullptr, B, d, 0, hyp, weights + L.o_center, PX, sX, nullptr)) return rc;
    if (int rc = dsvgp_kernel_fwd_rect(ctx, PZ, selfZ, M, p, PX, sX, B, 0, d, hyp, KZX, S.ldk)) return rc;
    // 2. V = Q K_ZX, fp64 accumulation over the float right operand, rounded once to fp32.  Never split along K: only the fp32 copy is
    //    asked for (no fp64 target for slices to meet in) and the slab is empty (launch_gemm and launch_gemm64 keep one K slice).
    //    Q is exactly symmetric: read as its transpose, both operands are contiguous along the output axes (the wide fp64 kernel's form)
    {
        GemmArgs g{};
        g.M = S.Mp; g.N = B; g.K = S.Mp; g.A = Q; g.B = KZX; g.C = nullptr; g.C32 = V32;
        g.lda = ldq; g.ldb = S.ldk; g.ldc = 0; g.ldc32 = S.ldk;
        g.alpha = 1.0; g.beta = 0.0; g.flags = DSVGP_GEMM_TRANS_A | DSVGP_GEMM_B_IS_FLOAT; g.batch = 1; g.splitk = 1;
        g.slab = V32; g.slab_bytes = 0;
        if (int rc = launch_gemm(st, 1, g)) return rc;
    }
    // 3. the contraction
    if (S.route == 1) {
        switch (L.ldw) {
            case 4: return launch_fused<4>(st, weights, L, M, d, p, x, B, V32, S.ldk, var_out, grad_out);
            case 8: return launch_fused<8>(st, weights, L, M, d, p, x, B, V32, S.ldk, var_out, grad_out);
            case 12: return launch_fused<12>(st, weights, L, M, d, p, x, B, V32, S.ldk, var_out, grad_out);
            case 16: return launch_fused<16>(st, weights, L, M, d, p, x, B, V32, S.ldk, var_out, grad_out);
            case 20: return launch_fused<20>(st, weights, L, M, d, p, x, B, V32, S.ldk, var_out, grad_out);
            case 24: return launch_fused<24>(st, weights, L, M, d, p, x, B, V32, S.ldk, var_out, grad_out);
            case 28: return launch_fused<28>(st, weights, L, M, d, p, x, B, V32, S.ldk, var_out, grad_out);
            default: return launch_fused<32>(st, weights, L, M, d, p, x, B, V32, S.ldk, var_out, grad_out);
        }
    }
    float* part = ws + S.o_part;
    float* G = grad_out ? ws + S.o_g : nullptr;
    hipLaunchKernelGGL(var_reduce_kernel, dim3(cdiv(B, VP_TILE), S.ns), dim3(256), 0, st, KZX, V32, S.Mp, B, S.ldk, part, G, S.ldg);
    DSVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(var_combine_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, part, S.ns, B, S.ldk, hyp, var_out);
    DSVGP_LAUNCH_CHECK();
    if (!grad_out) return 0;
    float* dhyp = ws + S.o_dh;
    if (hipError_t e = hipMemsetAsync(grad_out, 0, (size_t)B * d * sizeof(float), st)) return 1000 + (int)e;      // (the backward accumulates)
    if (hipError_t e = hipMemsetAsync(dhyp, 0, 4 * sizeof(float), st)) return 1000 + (int)e;
    return dsvgp_kernel_bwd_rect(ctx, G, S.ldg, 0, PX, sX, nullptr, B, 0, PZ, selfZ, M, p, d, hyp, grad_out, nullptr, dhyp, ws + S.o_bwd);
}

extern "C" int dsvgp_acq_eval(dsvgp_ctx* ctx, int kind, int maximize, const float* beta, const float* best, const float* mu, const float* gmu,
                              const float* var, const float* gvar, int B, int d, float* out, float* gout) {
    if (!ctx || !mu || !var || !out || B < 1 || d < 1 || kind < VP_ACQ_LCB_VAR || kind > VP_ACQ_EI) return DSVGP_EINVAL;
    if ((kind == VP_ACQ_EI ? !best : !beta) || (gout && (!gmu || !gvar)) || (int64_t)B * d > VP_IDX_MAX) return DSVGP_EINVAL;
    hipLaunchKernelGGL(acq_eval_kernel, dim3(cdiv(B, 4)), dim3(256), 0, ctx->stream, kind, maximize ? -1.f : 1.f, beta, best, mu, gmu, var,
                       gvar, B, d, out, gout);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t dsvgp_acq_descend_workspace_bytes(int M, int d, int p, int B) {
    VpDescend S;
    if (M < 1 || d < 1 || p < 0 || p > VP_MAX_P || B < 1) return 0;
    return vp_descend(d, B, dsvgp_mean_workspace_bytes(M, d, B, 0), dsvgp_var_workspace_bytes(M, d, p, B, 1), &S) ? S.total * sizeof(float) : 0;
}

extern "C" int dsvgp_acq_descend(dsvgp_ctx* ctx, const float* mean_weights, const float* var_weights, const double* Q, int64_t ldq,
                                 const float* PZ, const float* selfZ, const float* hyp, int M, int d, int p, float* x, int B,
                                 const float* lower, const float* upper, int kind, const float* beta, const float* best, int maximize,
                                 int iterations, float initial_step, int resume, float* values, float* grads, float* steps, int* accepted,
                                 void* workspace) {
    if (!ctx || !mean_weights || !var_weights || !Q || !PZ || !selfZ || !hyp || !x || !lower || !upper || !values || !grads || !steps ||
        !accepted || !workspace || iterations < 0 || M < 1 || d < 1 || p < 0 || p > VP_MAX_P || B < 1)
        return DSVGP_EINVAL;
    if ((uintptr_t)workspace % 16) return DSVGP_EALIGN;
    VpDescend S;
    if (!vp_descend(d, B, dsvgp_mean_workspace_bytes(M, d, B, 0), dsvgp_var_workspace_bytes(M, d, p, B, 1), &S)) return DSVGP_EINVAL;
    float* ws = (float*)workspace;
    float *y = ws + S.o_y, *gy = ws + S.o_gy, *fy = ws + S.o_fy, *mu = ws + S.o_mu, *gmu = ws + S.o_gmu, *var = ws + S.o_var,
          *gvar = ws + S.o_gvar;
    hipStream_t st = ctx->stream;
    auto eval = [&](const float* pts, float* f, float* g) -> int {
        if (int rc = dsvgp_mean_predict(ctx, mean_weights, M, d, pts, B, nullptr, 0, mu, gmu, ws + S.o_mean)) return rc;
        if (int rc = dsvgp_var_predict(ctx, var_weights, Q, ldq, PZ, selfZ, hyp, M, d, p, pts, B, var, gvar, ws + S.o_varws)) return rc;
        return dsvgp_acq_eval(ctx, kind, maximize, beta, best, mu, gmu, var, gvar, B, d, f, g);
    };
    auto step = [&](int mode) {
        hipLaunchKernelGGL(acq_step_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, var_weights, mode, B, d, initial_step, lower, upper, x, values,
                           grads, steps, accepted, y, fy, gy);
    };
    if (!resume) {
        hipLaunchKernelGGL(acq_clamp_kernel, dim3(cdiv((int64_t)B * d, 256)), dim3(256), 0, st, x, (int64_t)B * d, d, lower, upper);
        DSVGP_LAUNCH_CHECK();
        if (int rc = eval(x, values, grads)) return rc;
    }
    step(resume ? 1 : 0);
    DSVGP_LAUNCH_CHECK();
    for (int t = 0; t < iterations; ++t) {
        if (int rc = eval(y, fy, gy)) return rc;
        step(2);
        DSVGP_LAUNCH_CHECK();
    }
    return 0;
}
