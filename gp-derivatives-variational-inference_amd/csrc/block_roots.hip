// Per-point covariance roots, gfx950: what turns the [B, q, q] blocks of dsvgp_predictive_blocks (q = pd + 1 <= 96: the covariance of
// (f(x), D_1 f(x), ..., D_pd f(x)) at every point) into distributions -- the lower Cholesky factor of every block with its
// log-determinant (dsvgp_blocks_factor), draws mu + L eps (dsvgp_blocks_draw) and the whitened residual z = L^-1 (y - mu) with the joint
// log-density (dsvgp_blocks_logpdf).  B small factorisations, none of them worth a solver call, all of them wanted in fp64: without a
// likelihood the blocks are those of q(f), close to singular near the inducing points, and their float32 entries already carry 7e-6.
//
// One TEAM of T = 8 / 16 / 32 / 64 lanes per block, 256 / T teams per 256-thread workgroup (one wave = one team per workgroup at T = 64),
// the block in LDS as [q][q + 1] doubles: block_roots_plan.h.  Team lane t owns the rows t and t + T; every sum is one lane's serial
// fma chain in ascending column order, so the result for block b is a function of that block alone -- no floating-point atomics, the
// same bits whatever B, the neighbours or the card.  All loop bounds and every barrier depend on q alone (uniform over the workgroup);
// teams past B and rows past q idle through them.  float in, widened, fp64 throughout, rounded once at the float outputs.
//
// factor (left-looking, column by column, two barriers per column):  s_i = S[i][k] - sum_{c<k} L[i][c] L[k][c] for the owned rows
// i >= k; the owner of row k leaves the pivot s_k in S[k][k]; barrier; every lane reads the pivot d (d <= 0 or not finite: the team
// notes k + 1, goes on -- the NaNs that follow index nothing -- and fills the outputs with NaN at the end), L[i][k] = s_i / sqrt(d),
// the owner of row k puts sqrt(d) into the pad column; barrier.  logdet = 2 sum_i log L[i][i], the logs by the rows' owners, the sum by
// team lane 0 in row order.
// logpdf (column-oriented forward substitution, one barrier per column): the owner of row c publishes z_c = v_c / L[c][c] in the pad
// column; barrier; v_i -= L[i][c] z_c for the owned rows i > c.  |z|^2 by team lane 0 in row order.
// draw: item (draw i, row a) = one lane's chain over c <= a, eps read through the cache (the lanes of a team read the same row of eps).
#include "common.h"
#include "block_roots_plan.h"

namespace {

constexpr double LOG_2PI = 1.8378770664093454835606594728112;

__device__ __forceinline__ double br_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// roots[b] ([q][q] doubles, contiguous) -> the team's image; a NaN root (failed block) travels as it is
__device__ __forceinline__ void br_load_root(const double* __restrict__ src, double* __restrict__ Sb, int q, int ld, int t, int T) {
    const int qq = q * q;
    for (int e = t; e < qq; e += T) {
        const int i = e / q, j = e - i * q;
        Sb[i * ld + j] = src[e];
    }
}

__global__ __launch_bounds__(256) void blocks_factor_kernel(const float* __restrict__ blocks, int B, int q, int T, int G, double jitter,
                                                            double* __restrict__ roots, double* __restrict__ logdet,
                                                            int* __restrict__ info, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double br_lds[];
    const int ld = q + 1, img = q * ld, qq = q * q;
    const int team = block_roots_team_of(threadIdx.x, T), t = block_roots_lane_of(threadIdx.x, T);
    const long long b = block_roots_block(blockIdx.x, G, team);
    const bool active = b < B;
    double* Sb = br_lds + block_roots_lds(team, img, ld, 0, 0);
    if (active) {
        const float* src = blocks + b * qq;
        for (int e = t; e < qq; e += T) {
            const int i = e / q, j = e - i * q;
            const double v = (double)src[e];
            Sb[i * ld + j] = i == j ? v + jitter : v;
        }
    }
    __syncthreads();
    int bad = 0;                                                     // (the same in every lane of the team: all of them read the pivots)
    for (int k = 0; k < q; ++k) {
        double s[BR_ROWS];
#pragma unroll
        for (int h = 0; h < BR_ROWS; ++h) {
            const int i = t + h * T;
            s[h] = 0.0;
            if (active && i >= k && i < q) {
                double acc = Sb[i * ld + k];
                for (int c = 0; c < k; ++c) acc = __builtin_fma(-Sb[i * ld + c], Sb[k * ld + c], acc);
                s[h] = acc;
                if (i == k) Sb[k * ld + k] = acc;
            }
        }
        __syncthreads();
        if (active) {
            const double d = Sb[k * ld + k];
            if (!bad && (!(d > 0.0) || d > 1.7976931348623157e308)) bad = k + 1;
            const double r = sqrt(d);
#pragma unroll
            for (int h = 0; h < BR_ROWS; ++h) {
                const int i = t + h * T;
                if (i == k) Sb[k * ld + q] = r;
                else if (i > k && i < q) Sb[i * ld + k] = s[h] / r;
            }
        }
        __syncthreads();
    }
    if (active) {
#pragma unroll
        for (int h = 0; h < BR_ROWS; ++h) {
            const int i = t + h * T;
            if (i < q) Sb[i * ld + i] = log(Sb[i * ld + q]);         // (the pivots are not read again)
        }
    }
    __syncthreads();
    if (active) {
        double* dst = roots + b * qq;
        for (int e = t; e < qq; e += T) {
            const int i = e / q, j = e - i * q;
            const double v = j < i ? Sb[i * ld + j] : j == i ? Sb[i * ld + q] : 0.0;
            dst[e] = bad ? br_nan() : v;
        }
        if (t == 0) {
            double acc = 0.0;
            for (int i = 0; i < q; ++i) acc += Sb[i * ld + i];
            logdet[b] = bad ? br_nan() : 2.0 * acc;
            info[b] = bad;
            if (bad) atomicMax(status, bad);
        }
    }
}

__global__ __launch_bounds__(256) void blocks_draw_kernel(const double* __restrict__ roots, const float* __restrict__ mu,
                                                          const float* __restrict__ eps, int B, int q, int T, int G, int n,
                                                          float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double br_lds[];
    const int ld = q + 1, img = q * ld;
    const int team = block_roots_team_of(threadIdx.x, T), t = block_roots_lane_of(threadIdx.x, T);
    const long long b = block_roots_block(blockIdx.x, G, team);
    const bool active = b < B;
    double* Sb = br_lds + block_roots_lds(team, img, ld, 0, 0);
    if (active) br_load_root(roots + b * q * q, Sb, q, ld, t, T);
    __syncthreads();
    if (!active) return;
    const long long ncols = (long long)B * q, base = b * q, items = (long long)n * q;
    for (long long w = t; w < items; w += T) {
        const long long i = w / q;
        const int a = (int)(w - i * q);
        const float* er = eps + i * ncols + base;
        double acc = 0.0;
        for (int c = 0; c <= a; ++c) acc = __builtin_fma(Sb[a * ld + c], (double)er[c], acc);
        out[i * ncols + base + a] = (float)((double)mu[base + a] + acc);
    }
}

__global__ __launch_bounds__(256) void blocks_logpdf_kernel(const double* __restrict__ roots, const double* __restrict__ logdet,
                                                            const float* __restrict__ mu, const float* __restrict__ y, int B, int q,
                                                            int T, int G, float* __restrict__ z, float* __restrict__ logp) {
    extern __shared__ __attribute__((aligned(16))) double br_lds[];
    const int ld = q + 1, img = q * ld;
    const int team = block_roots_team_of(threadIdx.x, T), t = block_roots_lane_of(threadIdx.x, T);
    const long long b = block_roots_block(blockIdx.x, G, team);
    const bool active = b < B;
    const long long base = b * q;
    double* Sb = br_lds + block_roots_lds(team, img, ld, 0, 0);
    double v[BR_ROWS];
#pragma unroll
    for (int h = 0; h < BR_ROWS; ++h) {
        const int i = t + h * T;
        v[h] = active && i < q ? (double)y[base + i] - (double)mu[base + i] : 0.0;
    }
    if (active) br_load_root(roots + base * q, Sb, q, ld, t, T);
    __syncthreads();
    for (int c = 0; c < q; ++c) {
        if (active) {
#pragma unroll
            for (int h = 0; h < BR_ROWS; ++h)
                if (t + h * T == c) Sb[c * ld + q] = v[h] / Sb[c * ld + c];
        }
        __syncthreads();
        if (active) {
            const double zc = Sb[c * ld + q];
#pragma unroll
            for (int h = 0; h < BR_ROWS; ++h) {
                const int i = t + h * T;
                if (i > c && i < q) v[h] = __builtin_fma(-Sb[i * ld + c], zc, v[h]);
            }
        }
    }
    if (!active) return;
    if (z)
        for (int i = t; i < q; i += T) z[base + i] = (float)Sb[i * ld + q];
    if (t == 0) {
        double ss = 0.0;
        for (int i = 0; i < q; ++i) ss = __builtin_fma(Sb[i * ld + q], Sb[i * ld + q], ss);
        logp[b] = (float)(-0.5 * ss - 0.5 * logdet[b] - 0.5 * (double)q * LOG_2PI);
    }
}

// the LDS image of a workgroup passes 64 KB from q = 91 (and at q = 32, eight teams): the attribute belongs to the CURRENT device's copy
// of the kernel, so it is set per call (a host-side table write, no device work -- as gemm3b.hip does)
template <typename K>
int br_allow_lds(K kernel, const BlockRootsPlan& w) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.lds_bytes);
    return e == hipSuccess ? 0 : 1000 + (int)e;
}

}  // namespace

extern "C" int dsvgp_blocks_factor(dsvgp_ctx* ctx, const float* blocks, int B, int q, double jitter, double* roots, double* logdet,
                                   int* info, int* status) {
    if (!ctx || !blocks || !roots || !logdet || !info || !status || B < 0 || q < 1 || q > BR_QMAX) return DSVGP_EINVAL;
    if (hipMemsetAsync(status, 0, sizeof(int), ctx->stream) != hipSuccess) return 1000 + (int)hipGetLastError();
    if (B == 0) return 0;
    BlockRootsPlan w;
    if (block_roots_plan(B, q, w)) return DSVGP_EINVAL;
    if (int rc = br_allow_lds(blocks_factor_kernel, w)) return rc;
    hipLaunchKernelGGL(blocks_factor_kernel, dim3(w.ngroups), dim3(w.nthreads), w.lds_bytes, ctx->stream, blocks, B, q, w.T, w.G, jitter,
                       roots, logdet, info, status);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_blocks_draw(dsvgp_ctx* ctx, const double* roots, const float* mu, const float* eps, int B, int q, int n,
                                 float* out) {
    if (!ctx || !roots || !mu || !eps || !out || B < 0 || n < 0 || q < 1 || q > BR_QMAX) return DSVGP_EINVAL;
    if (B == 0 || n == 0) return 0;
    BlockRootsPlan w;
    if (block_roots_plan(B, q, w)) return DSVGP_EINVAL;
    if (int rc = br_allow_lds(blocks_draw_kernel, w)) return rc;
    hipLaunchKernelGGL(blocks_draw_kernel, dim3(w.ngroups), dim3(w.nthreads), w.lds_bytes, ctx->stream, roots, mu, eps, B, q, w.T, w.G, n,
                       out);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_blocks_logpdf(dsvgp_ctx* ctx, const double* roots, const double* logdet, const float* mu, const float* y, int B,
                                   int q, float* z, float* logp) {
    if (!ctx || !roots || !logdet || !mu || !y || !logp || B < 0 || q < 1 || q > BR_QMAX) return DSVGP_EINVAL;
    if (B == 0) return 0;
    BlockRootsPlan w;
    if (block_roots_plan(B, q, w)) return DSVGP_EINVAL;
    if (int rc = br_allow_lds(blocks_logpdf_kernel, w)) return rc;
    hipLaunchKernelGGL(blocks_logpdf_kernel, dim3(w.ngroups), dim3(w.nthreads), w.lds_bytes, ctx->stream, roots, logdet, mu, y, B, q, w.T,
                       w.G, z, logp);
    DSVGP_LAUNCH_CHECK();
    return 0;
}
