// Two likelihood noises: the function-value rows of an interleaved batch (j % (p + 1) == 0) are observed under
// n_f = hyp[2], the directional-derivative rows under n_g = hyp[3].  The per-output objective is likelihood_kernel (elbo.hip) with the
// row's class noise in the place of the one noise; the collapsed statistics are the unweighted ones of columns scaled by sqrt(omega),
// omega = 1 on value rows and rho = n_f / n_g on derivative rows.  The class is read from the row index, never from a mask array.  Every
// sum has a fixed order (per-workgroup partials joined in workgroup order); no floating-point atomics, no host read.
#include <math.h>

#include "common.h"

namespace {

constexpr int NC_MAX_BLOCKS = 512;           // workgroups of the likelihood pass: one partial row each
constexpr int NC_PART = 8;                   // floats per partial row (6 used)
constexpr int NC_CS_HEAD = 8;                // doubles in front of the collapsed statistics' matrix (collapsed.hip: CS_HEAD)
constexpr float NC_MIN_VARIANCE = 1e-6f;     // gpytorch settings.min_variance (elbo.hip)
constexpr double NC_KXX_JITTER = 1e-4;       // data_data_covar.add_jitter(1e-4): what solve / evaluate add per row (collapsed.hip)

__device__ inline double block_sum_f64(double v, double* sh) {           // blockDim.x a power of two
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// likelihood_kernel (elbo.hip) with the row's class noise.  partials[b][0..5]: sum ll, d_noise of the value rows, d_constant,
// d_outputscale and d_lengthscale of the prior diagonal, d_noise of the derivative rows
__global__ __launch_bounds__(256) void likelihood_classes_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                                 const float* __restrict__ y, int ncols, int p,
                                                                 const float* __restrict__ hyp, int mll_type, float inv_rows,
                                                                 float* __restrict__ mu_bar, float* __restrict__ var_bar,
                                                                 float* __restrict__ varn_out, float* __restrict__ partials) {
    __shared__ float red[6][4];
    const float ell = hyp[0], s = hyp[1], noise_f = hyp[2], noise_g = hyp[3];
    const float LOG2PI = 1.8378770664093453f;
    const int q = p + 1;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < ncols; j += (int64_t)gridDim.x * 256) {
        const bool isf = ((int)j % q) == 0;
        const float noise = isf ? noise_f : noise_g;
        const float mj = mu[j], r = y[j] - mj;
        const float vraw = var[j] + noise;
        const bool clamped = vraw < NC_MIN_VARIANCE;
        const float vn = clamped ? NC_MIN_VARIANCE : vraw;
        float ll, dmu, dvn, dnoise;
        if (mll_type == 0) {
            ll = -0.5f * ((r * r + vn) / noise + logf(noise) + LOG2PI);
            dmu = r / noise;
            dvn = -0.5f / noise;
            dnoise = 0.5f * (r * r + vn) / (noise * noise) - 0.5f / noise;
        } else {
            const float tot = fmaxf(vn + noise, 1e-8f);
            ll = -0.5f * (r * r / tot + logf(tot) + LOG2PI);
            dmu = r / tot;
            dvn = 0.5f * (r * r / (tot * tot) - 1.f / tot);
            dnoise = dvn;
        }
        const float dvar = clamped ? 0.f : dvn;
        dnoise += dvar;
        const float mb = -dmu * inv_rows, vb = -dvar * inv_rows;
        mu_bar[j] = mb;
        var_bar[j] = vb;
        varn_out[j] = vn;
        const float dn = -dnoise * inv_rows;
        acc[0] += ll;
        acc[1] += isf ? dn : 0.f;
        acc[2] += mb;
        acc[3] += vb * (isf ? 1.f : 1.f / (ell * ell));
        acc[4] += isf ? 0.f : vb * (-2.f * s / (ell * ell * ell));
        acc[5] += isf ? 0.f : dn;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        float v = acc[c];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) red[c][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) partials[blockIdx.x * NC_PART + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

// scal[c] = sum over the workgroups in order (c < 6; scal[6..7] = 0).  One wave.
__global__ __launch_bounds__(64) void likelihood_classes_finish_kernel(const float* __restrict__ partials, int nblocks,
                                                                       float* __restrict__ scal) {
    const int c = threadIdx.x;
    if (c >= NC_PART) return;
    double s = 0.0;
    if (c < 6)
        for (int b = 0; b < nblocks; ++b) s += (double)partials[b * NC_PART + c];
    scal[c] = (float)s;
}

// collapsed_rows_kernel (collapsed.hip) with row weights: r = sqrt(omega) (y - c); workgroup 0 alone adds sum omega diag +
// 1e-4 sum (omega - 1), the row count and the count of value rows (strided chains joined by a fixed tree)
__global__ __launch_bounds__(1024) void collapsed_rows_classes_kernel(double* __restrict__ state, double* __restrict__ rrow, int Bp, int q,
                                                                      const float* __restrict__ y, const float* __restrict__ constant,
                                                                      const float* __restrict__ diag, const float* __restrict__ hyp) {
    __shared__ double sh[1024];
    const double c = (double)constant[0];
    const double rho = (double)hyp[2] / (double)hyp[3], root = sqrt(rho);
    for (int64_t j = (int64_t)blockIdx.x * 1024 + threadIdx.x; j < Bp; j += (int64_t)gridDim.x * 1024) {
        const double r = (double)y[j] - c;
        rrow[j] = ((int)j % q) == 0 ? r : root * r;
    }
    if (blockIdx.x != 0) return;
    double s = 0.0;
    for (int j = threadIdx.x; j < Bp; j += 1024) {
        const double dg = (double)diag[j];
        s += (j % q) == 0 ? dg : rho * dg + NC_KXX_JITTER * (rho - 1.0);
    }
    s = block_sum_f64(s, sh);
    if (threadIdx.x == 0) {
        state[0] += s;
        state[1] += (double)Bp;
        state[2] += (double)(Bp / q);
    }
}

// A[i, j] *= sqrt(rho) for every row i < rows of the derivative columns j (j % q != 0): one thread per column, blockIdx.y strides the
// rows; the value columns are not touched
__global__ __launch_bounds__(256) void scale_derivative_columns_kernel(double* __restrict__ A, int64_t ld, int rows, int ncols, int q,
                                                                       const float* __restrict__ hyp) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ncols || ((int)j % q) == 0) return;
    const double root = sqrt((double)hyp[2] / (double)hyp[3]);
    for (int i = blockIdx.y; i < rows; i += gridDim.y) A[(int64_t)i * ld + j] *= root;
}

}  // namespace

extern "C" size_t dsvgp_likelihood_terms_classes_workspace_bytes(void) { return sizeof(float) * NC_MAX_BLOCKS * NC_PART; }

extern "C" int dsvgp_likelihood_terms_classes(dsvgp_ctx* ctx, const float* mu, const float* var, const float* y, int ncols, int p,
                                              const float* hyp, int mll_type, double global_rows, float* mu_bar, float* var_bar,
                                              float* varn_out, float* out_scalars, void* workspace) {
    if (!ctx || !mu || !var || !y || !hyp || !mu_bar || !var_bar || !varn_out || !out_scalars || !workspace || ncols < 0 || p < 0 ||
        global_rows <= 0 || (mll_type != 0 && mll_type != 1))
        return DSVGP_EINVAL;
    if ((uintptr_t)workspace % 16) return DSVGP_EALIGN;
    if (ncols == 0) {                                   // no launch
        const hipError_t e = hipMemsetAsync(out_scalars, 0, 8 * sizeof(float), ctx->stream);
        return e == hipSuccess ? 0 : 1000 + (int)e;
    }
    int blocks = cdiv(ncols, 256);
    if (blocks > NC_MAX_BLOCKS) blocks = NC_MAX_BLOCKS;
    float* partials = (float*)workspace;
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(likelihood_classes_kernel, dim3(blocks), dim3(256), 0, s, mu, var, y, ncols, p, hyp, mll_type,
                       (float)(1.0 / global_rows), mu_bar, var_bar, varn_out, partials);
    hipLaunchKernelGGL(likelihood_classes_finish_kernel, dim3(1), dim3(64), 0, s, (const float*)partials, blocks, out_scalars);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_collapsed_accumulate_classes(dsvgp_ctx* ctx, void* state, int Mp, double* A64, int64_t lda, int Bp, int pd,
                                                  const float* y, const float* constant, const float* prior_diag, const float* hyp) {
    if (!ctx || !state || !A64 || !y || !constant || !prior_diag || !hyp || Mp <= 0 || Bp < 0 || lda < Bp || pd < 0 || Bp % (pd + 1))
        return DSVGP_EINVAL;
    if (((uintptr_t)state % 8) || ((uintptr_t)A64 % 8)) return DSVGP_EALIGN;
    if (Bp == 0) return 0;
    double* st = (double*)state;
    hipStream_t s = ctx->stream;
    const int blocks = cdiv(Bp, 1024) < 256 ? cdiv(Bp, 1024) : 256;
    hipLaunchKernelGGL(collapsed_rows_classes_kernel, dim3(blocks), dim3(1024), 0, s, st, A64 + (int64_t)Mp * lda, Bp, pd + 1, y, constant,
                       prior_diag, hyp);
    if (pd > 0)
        hipLaunchKernelGGL(scale_derivative_columns_kernel, dim3(cdiv(Bp, 256), Mp < 64 ? Mp : 64), dim3(256), 0, s, A64, lda, Mp, Bp, pd + 1,
                           hyp);
    DSVGP_LAUNCH_CHECK();
    return collapsed_gram_update(ctx, st + NC_CS_HEAD, Mp, A64, lda, Bp);
}
