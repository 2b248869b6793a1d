// Missing observations: a NaN entry of y is an observation that does not exist.  Both training objectives are
// sums over output rows and every column of A = L^-1 K_ZX is independent of the others, so a missing row is a column with zero
// upstream: these entries derive the present mask from y on the device, count the present rows there, and hand exact zeros to the
// unchanged kernels behind them.  Every kernel is one pass over B' values or over M' x (masked columns); every sum has a fixed
// order (per-workgroup partials joined in workgroup order); no floating-point atomics, no host read.
#include <math.h>

#include "common.h"

namespace {

constexpr int MS_MAX_BLOCKS = 512;           // workgroups of the likelihood pass: one partial row each
constexpr int MS_PART = 8;                   // floats per partial row (5 used)
constexpr int MS_CS_HEAD = 8;                // doubles in front of the collapsed statistics' matrix (collapsed.hip: CS_HEAD)
constexpr float MS_MIN_VARIANCE = 1e-6f;     // gpytorch settings.min_variance (elbo.hip)

__device__ __forceinline__ bool present(float y) { return !__builtin_isnan(y); }

__device__ inline int block_sum_int(int v, int* sh) {           // blockDim.x a power of two
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const int r = sh[0];
    __syncthreads();
    return r;
}

__device__ inline double block_sum_f64(double v, double* sh) {
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

// counts[b] = present entries of workgroup b's grid-stride share of y
__global__ __launch_bounds__(256) void present_count_kernel(const float* __restrict__ y, int ncols, int* __restrict__ counts) {
    __shared__ int sh[256];
    int c = 0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < ncols; j += (int64_t)gridDim.x * 256) c += present(y[j]) ? 1 : 0;
    c = block_sum_int(c, sh);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// likelihood_kernel (elbo.hip) on the present rows, normalised by their count n (integers: any order gives the same n); a missing row
// gets mu_bar = var_bar = varn = 0 and adds nothing.  partials[b][0..4]: sum ll (not normalised), d_noise, d_constant, d_outputscale
// and d_lengthscale of the prior diagonal
__global__ __launch_bounds__(256) void likelihood_masked_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                                const float* __restrict__ y, int ncols, int p,
                                                                const float* __restrict__ hyp, int mll_type,
                                                                const int* __restrict__ counts, int nblocks, float* __restrict__ mu_bar,
                                                                float* __restrict__ var_bar, float* __restrict__ varn_out,
                                                                float* __restrict__ partials) {
    __shared__ int shn[256];
    __shared__ float red[5][4];
    int c = 0;
    for (int b = threadIdx.x; b < nblocks; b += 256) c += counts[b];
    const int n = block_sum_int(c, shn);
    const float inv_rows = n > 0 ? 1.f / (float)n : 0.f;
    const float ell = hyp[0], s = hyp[1], noise = hyp[2];
    const float LOG2PI = 1.8378770664093453f;
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < ncols; j += (int64_t)gridDim.x * 256) {
        const float yj = y[j];
        if (!present(yj)) {
            mu_bar[j] = 0.f;
            var_bar[j] = 0.f;
            varn_out[j] = 0.f;
            continue;
        }
        const float r = yj - mu[j];
        const float vraw = var[j] + noise;
        const bool clamped = vraw < MS_MIN_VARIANCE;
        const float vn = clamped ? MS_MIN_VARIANCE : vraw;
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
        const bool isf = (j % (p + 1)) == 0;
        acc[0] += ll;
        acc[1] += -dnoise * inv_rows;
        acc[2] += mb;
        acc[3] += vb * (isf ? 1.f : 1.f / (ell * ell));
        acc[4] += isf ? 0.f : vb * (-2.f * s / (ell * ell * ell));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        float v = acc[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) red[q][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < 5) partials[blockIdx.x * MS_PART + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

// scal[q] = sum over the workgroups in order; scal[0] is divided by n here (0 when n = 0), so that dsvgp_step_epilogue with rows = 1
// forms the loss; n itself goes to the caller's device word.  One wave.
__global__ __launch_bounds__(64) void likelihood_masked_finish_kernel(const float* __restrict__ partials, const int* __restrict__ counts,
                                                                      int nblocks, float* __restrict__ scal, int* __restrict__ n_out) {
    const int q = threadIdx.x;
    if (q >= MS_PART) return;
    int n = 0;
    for (int b = 0; b < nblocks; ++b) n += counts[b];
    double s = 0.0;
    if (q < 5)
        for (int b = 0; b < nblocks; ++b) s += (double)partials[b * MS_PART + q];
    if (q == 0) {
        s = n > 0 ? s / (double)n : 0.0;
        n_out[0] = n;
    }
    scal[q] = (float)s;
}

// collapsed_rows_kernel (collapsed.hip) on the present rows: r = y - c, 0 on a missing row; workgroup 0 alone adds the present rows'
// prior diagonal, their count and the count of present value rows (strided chains joined by a fixed tree; the counts are exact)
__global__ __launch_bounds__(1024) void collapsed_rows_masked_kernel(double* __restrict__ state, double* __restrict__ rrow, int Bp, int q,
                                                                     const float* __restrict__ y, const float* __restrict__ constant,
                                                                     const float* __restrict__ diag) {
    __shared__ double sh[1024];
    const double c = (double)constant[0];
    for (int64_t j = (int64_t)blockIdx.x * 1024 + threadIdx.x; j < Bp; j += (int64_t)gridDim.x * 1024) {
        const float yj = y[j];
        rrow[j] = present(yj) ? (double)yj - c : 0.0;
    }
    if (blockIdx.x != 0) return;
    double s = 0.0, n = 0.0, nv = 0.0;
    for (int j = threadIdx.x; j < Bp; j += 1024) {
        if (!present(y[j])) continue;
        s += (double)diag[j];
        n += 1.0;
        if (j % q == 0) nv += 1.0;
    }
    s = block_sum_f64(s, sh);
    n = block_sum_f64(n, sh);
    nv = block_sum_f64(nv, sh);
    if (threadIdx.x == 0) {
        state[0] += s;
        state[1] += n;
        state[2] += nv;
    }
}

// Mat[i, j] = 0 for every row i < rows of the columns j whose target is missing: one thread per column, blockIdx.y strides the rows;
// only the masked columns are touched.  T = double (A) or float (K_ZX)
template <typename T>
__global__ __launch_bounds__(256) void zero_missing_columns_kernel(T* __restrict__ Mat, int64_t ld, int rows, int ncols,
                                                                   const float* __restrict__ y) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ncols || present(y[j])) return;
    for (int i = blockIdx.y; i < rows; i += gridDim.y) Mat[(int64_t)i * ld + j] = (T)0;
}

// y_clean = y on the present rows, the constant on the missing ones: the residual y_clean - c is then exactly 0 there
__global__ __launch_bounds__(256) void clean_targets_kernel(const float* __restrict__ y, const float* __restrict__ constant, int ncols,
                                                            float* __restrict__ y_clean) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ncols) return;
    const float yj = y[j];
    y_clean[j] = present(yj) ? yj : constant[0];
}

__global__ __launch_bounds__(256) void zero_missing_entries_kernel(float* __restrict__ v, int ncols, const float* __restrict__ y) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < ncols && !present(y[j])) v[j] = 0.f;
}

inline size_t chunk_clean_offset(int Mp, int Bp) { return (dsvgp_collapsed_grad_chunk_bytes(Mp, Bp) + 15) / 16 * 16; }

}  // namespace

extern "C" size_t dsvgp_likelihood_terms_masked_workspace_bytes(void) {
    return sizeof(int) * MS_MAX_BLOCKS + sizeof(float) * MS_MAX_BLOCKS * MS_PART;
}

extern "C" int dsvgp_likelihood_terms_masked(dsvgp_ctx* ctx, const float* mu, const float* var, const float* y, int ncols, int p,
                                             const float* hyp, int mll_type, float* mu_bar, float* var_bar, float* varn_out,
                                             float* out_scalars, int* n_present, void* workspace) {
    if (!ctx || !mu || !var || !y || !hyp || !mu_bar || !var_bar || !varn_out || !out_scalars || !n_present || !workspace || ncols < 0 ||
        p < 0 || (mll_type != 0 && mll_type != 1))
        return DSVGP_EINVAL;
    if ((uintptr_t)workspace % 16) return DSVGP_EALIGN;
    if (ncols == 0) {                                   // no launch: an empty batch has no present row
        hipError_t e = hipMemsetAsync(out_scalars, 0, 8 * sizeof(float), ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(n_present, 0, sizeof(int), ctx->stream);
        return e == hipSuccess ? 0 : 1000 + (int)e;
    }
    int blocks = cdiv(ncols, 256);
    if (blocks > MS_MAX_BLOCKS) blocks = MS_MAX_BLOCKS;
    int* counts = (int*)workspace;
    float* partials = (float*)(counts + MS_MAX_BLOCKS);
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(present_count_kernel, dim3(blocks), dim3(256), 0, s, y, ncols, counts);
    hipLaunchKernelGGL(likelihood_masked_kernel, dim3(blocks), dim3(256), 0, s, mu, var, y, ncols, p, hyp, mll_type, (const int*)counts,
                       blocks, mu_bar, var_bar, varn_out, partials);
    hipLaunchKernelGGL(likelihood_masked_finish_kernel, dim3(1), dim3(64), 0, s, (const float*)partials, (const int*)counts, blocks,
                       out_scalars, n_present);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_collapsed_accumulate_masked(dsvgp_ctx* ctx, void* state, int Mp, double* A64, int64_t lda, int Bp, int pd,
                                                 const float* y, const float* constant, const float* prior_diag) {
    if (!ctx || !state || !A64 || !y || !constant || !prior_diag || Mp <= 0 || Bp < 0 || lda < Bp || pd < 0 || Bp % (pd + 1))
        return DSVGP_EINVAL;
    if (((uintptr_t)state % 8) || ((uintptr_t)A64 % 8)) return DSVGP_EALIGN;
    if (Bp == 0) return 0;
    double* st = (double*)state;
    hipStream_t s = ctx->stream;
    const int blocks = cdiv(Bp, 1024) < 256 ? cdiv(Bp, 1024) : 256;
    hipLaunchKernelGGL(collapsed_rows_masked_kernel, dim3(blocks), dim3(1024), 0, s, st, A64 + (int64_t)Mp * lda, Bp, pd + 1, y, constant,
                       prior_diag);
    hipLaunchKernelGGL(zero_missing_columns_kernel<double>, dim3(cdiv(Bp, 256), Mp < 64 ? Mp : 64), dim3(256), 0, s, A64, lda, Mp, Bp, y);
    DSVGP_LAUNCH_CHECK();
    return collapsed_gram_update(ctx, st + MS_CS_HEAD, Mp, A64, lda, Bp);
}

extern "C" size_t dsvgp_collapsed_grad_chunk_masked_bytes(int Mp, int Bp) {
    if (dsvgp_collapsed_grad_chunk_bytes(Mp, Bp) == 0) return 0;
    return chunk_clean_offset(Mp, Bp) + sizeof(float) * (size_t)Bp;
}

extern "C" int dsvgp_collapsed_grad_chunk_masked(dsvgp_ctx* ctx, int Mp, int Bp, float* Kzx, int64_t ldk, const float* y,
                                                 const float* constant, const double* Q, int64_t ldq, const double* alpha,
                                                 const double* adj, float* K_bar, int64_t ldkb, float* diag_bar, double* rho_sum,
                                                 void* workspace) {
    if (!ctx || !Kzx || !y || !constant || !workspace || Mp <= 0 || Bp <= 0 || ldk < Bp) return DSVGP_EINVAL;
    const size_t off = chunk_clean_offset(Mp, Bp);
    if (off == 0) return DSVGP_EINVAL;
    if (((uintptr_t)workspace % 8) || ((uintptr_t)Kzx % 4)) return DSVGP_EALIGN;
    float* y_clean = (float*)((char*)workspace + off);
    hipStream_t s = ctx->stream;
    const int gx = cdiv(Bp, 256);
    hipLaunchKernelGGL(clean_targets_kernel, dim3(gx), dim3(256), 0, s, y, constant, Bp, y_clean);
    hipLaunchKernelGGL(zero_missing_columns_kernel<float>, dim3(gx, Mp < 64 ? Mp : 64), dim3(256), 0, s, Kzx, ldk, Mp, Bp, y);
    DSVGP_LAUNCH_CHECK();
    // zero K_ZX columns and a zero residual: the unchanged chunk call gives rho = 0 and K_ZX-bar = 2 w (Q 0 - alpha 0) = 0 there
    if (int rc = dsvgp_collapsed_grad_chunk(ctx, Mp, Bp, Kzx, ldk, y_clean, constant, Q, ldq, alpha, adj, K_bar, ldkb, diag_bar, rho_sum,
                                            workspace))
        return rc;
    if (diag_bar) {                                     // dg-bar = w was written on every row
        hipLaunchKernelGGL(zero_missing_entries_kernel, dim3(gx), dim3(256), 0, s, diag_bar, Bp, y);
        DSVGP_LAUNCH_CHECK();
    }
    return 0;
}
