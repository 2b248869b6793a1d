// Closed-form optimal q(u) (Titsias 2009) from one-pass sufficient statistics in the whitened basis, and the full-data ELBO of any
// q(u) from the same statistics.  The M'^2 B' and M'^3 products run on the existing MFMA GEMM (launch_gemm)
// and the blocked Cholesky with its fused inverse (dsvgp_potrf_inverse); the kernels here are passes over M'^2 or B' doubles.
//
// state (doubles): [0] sum of the prior diagonal, [1] R (rows), [2..7] reserved, then the (M'+1) x (M'+1) row-major matrix
//   T = tril([A ; r^T][A ; r^T]^T): rows < M' hold tril G, row M' holds b^T and, last, yy.  Only the lower triangle is defined.
#include <math.h>

#include "common.h"

namespace {

constexpr int CS_HEAD = 8;                   // doubles in front of the matrix
constexpr int CS_NPART = 7;                  // per-row partial sums: <S,G>, tr S, m^T G m, m^T m, m^T b, tr G, sum log L_S,ii
constexpr int CS_MAX_MP = 8192;              // the explicit-inverse regime of the blocked Cholesky

inline size_t al(size_t doubles) { return (doubles + 7) / 8 * 8; }          // 64-byte pieces
inline int pow2_at_least(int n) { int b = 64; while (b < n) b *= 2; return b; }

struct Layout {                              // the workspace of solve / evaluate, in doubles
    size_t W, X, Y, v0, v1, v2, part, flags, potrf, trsm, total;
    int ldw;
};
Layout layout(int n) {
    Layout l{};
    l.ldw = (n + 1) & ~1;
    const size_t nn = al((size_t)n * l.ldw);
    size_t o = 0;
    l.W = o; o += nn;                        // J B J -> its factor   | evaluate: symmetric G
    l.X = o; o += nn;                        //                       | evaluate: fp64 tril L_S
    l.Y = o; o += nn;                        //                       | evaluate: G L_S
    l.v0 = o; o += al(n);
    l.v1 = o; o += al(n);
    l.v2 = o; o += al(n);
    l.part = o; o += al((size_t)CS_NPART * n);
    l.flags = o; o += 8;                     // int[0] potrf status, int[1] non-finite statistic, int[2] empty state
    l.potrf = o; o += al((dsvgp_potrf_workspace_bytes(n, 1) + 7) / 8);
    l.trsm = o; o += al((dsvgp_trsm_workspace_bytes(n, n, pow2_at_least(n)) + 7) / 8);
    l.total = o;
    return l;
}

__device__ inline double block_sum(double v, double* sh) {      // fixed tree over the block's threads (blockDim.x a power of two)
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

// r = y - c (float64) under A, and -- block 0 alone, strided chains joined by a fixed tree -- the prior diagonal's sum and the row count
__global__ __launch_bounds__(1024) void collapsed_rows_kernel(double* __restrict__ state, double* __restrict__ rrow, int Bp,
                                                              const float* __restrict__ y, const float* __restrict__ constant,
                                                              const float* __restrict__ diag) {
    __shared__ double sh[1024];
    const double c = (double)constant[0];
    for (int64_t j = (int64_t)blockIdx.x * 1024 + threadIdx.x; j < Bp; j += (int64_t)gridDim.x * 1024) rrow[j] = (double)y[j] - c;
    if (blockIdx.x != 0) return;
    double s = 0.0;
    for (int j = threadIdx.x; j < Bp; j += 1024) s += (double)diag[j];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) {
        state[0] += s;
        state[1] += (double)Bp;
    }
}

__device__ inline double stat(const double* T, int ldt, int i, int j) { return i >= j ? T[(int64_t)i * ldt + j] : T[(int64_t)j * ldt + i]; }

// W = J B J (full symmetric), B = I + kappa G, kappa = num_data / (R noise); v0 = J b.  A non-finite statistic (or R = 0) raises a flag
// and a harmless value takes its place, so that the factorisation behind always runs on finite numbers.
__global__ __launch_bounds__(256) void collapsed_flip_kernel(const double* __restrict__ state, int n, const float* __restrict__ hyp,
                                                             double num_data, double* __restrict__ W, int ldw, double* __restrict__ v0,
                                                             int* __restrict__ flags) {
    const double* T = state + CS_HEAD;
    const int ldt = n + 1, i = blockIdx.x, ii = n - 1 - i;
    const double R = state[1], noise = (double)hyp[2];
    const double kappa = num_data / (R * noise);
    bool bad = false;
    for (int j = threadIdx.x; j < n; j += 256) {
        const double g = stat(T, ldt, ii, n - 1 - j);
        double w = (i == j ? 1.0 : 0.0) + kappa * g;
        if (!isfinite(w)) { bad = true; w = (i == j) ? 1.0 : 0.0; }
        W[(int64_t)i * ldw + j] = w;
    }
    if (threadIdx.x == 0) {
        double b = T[(int64_t)n * ldt + ii];
        if (!isfinite(b)) { bad = true; b = 0.0; }
        v0[i] = b;
        if (i == 0) {
            if (!isfinite(T[(int64_t)n * ldt + n]) || !isfinite(state[0]) || !isfinite(kappa)) bad = true;
            if (!(R > 0.0)) atomicOr(&flags[2], 1);
        }
    }
    if (bad) atomicOr(&flags[1], 1);
}

// out[i] = sum_k Mat[i, k] v[k] over k <= i (lower != 0) or k >= i: one block per row, fixed order
__global__ __launch_bounds__(256) void collapsed_trmv_kernel(const double* __restrict__ Mat, int ld, int n, int lower,
                                                             const double* __restrict__ v, double* __restrict__ out) {
    __shared__ double sh[256];
    const int i = blockIdx.x;
    const int k0 = lower ? 0 : i, k1 = lower ? i + 1 : n;
    double s = 0.0;
    for (int k = k0 + threadIdx.x; k < k1; k += 256) s += Mat[(int64_t)i * ld + k] * v[k];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) out[i] = s;
}

// the optimum, un-flipped: L_S* = J Ltilde^-T J (strict upper triangle exactly zero), m* = kappa J u, the natural pair, and the per-row
// partial sums of the scalars.  One block per row.
__global__ __launch_bounds__(256) void collapsed_unflip_kernel(const double* __restrict__ state, int n, const float* __restrict__ hyp,
                                                               double num_data, const double* __restrict__ DinvT, const double* __restrict__ u,
                                                               const int* __restrict__ flags, float* __restrict__ m, float* __restrict__ LS,
                                                               int64_t ldls, float* __restrict__ nat_vec, float* __restrict__ nat_mat,
                                                               int64_t ldnm, double* __restrict__ part) {
    __shared__ double sh[256];
    const double* T = state + CS_HEAD;
    const int ldt = n + 1, i = blockIdx.x;
    const bool bad = flags[0] != 0 || flags[1] != 0 || flags[2] != 0;
    const double kappa = num_data / (state[1] * (double)hyp[2]);
    const float fnan = __int_as_float(0x7fc00000);
    double trs = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) {
        const double l = (j <= i) ? DinvT[(int64_t)(n - 1 - i) * n + (n - 1 - j)] : 0.0;          // Ltilde^-1[n-1-j, n-1-i], read along a row of the transposed image
        trs += l * l;
        if (LS) LS[(int64_t)i * ldls + j] = bad ? fnan : (j <= i ? (float)l : 0.f);
        if (nat_mat) nat_mat[(int64_t)i * ldnm + j] = bad ? fnan : (float)(-0.5 * ((i == j ? 1.0 : 0.0) + kappa * stat(T, ldt, i, j)));
    }
    trs = block_sum(trs, sh);
    if (threadIdx.x == 0) {
        const double mi = kappa * u[n - 1 - i], bi = T[(int64_t)n * ldt + i];
        if (m) m[i] = bad ? fnan : (float)mi;
        if (nat_vec) nat_vec[i] = bad ? fnan : (float)(kappa * bi);
        part[0 * n + i] = 0.0;                               // (closed form at the optimum: collapsed_finish_kernel)
        part[1 * n + i] = trs;
        part[2 * n + i] = 0.0;
        part[3 * n + i] = mi * mi;
        part[4 * n + i] = mi * bi;
        part[5 * n + i] = T[(int64_t)i * ldt + i];
        part[6 * n + i] = log(DinvT[(int64_t)(n - 1 - i) * n + (n - 1 - i)]);
    }
}

// evaluate, pass 1: the symmetric fp64 G and the fp64 tril L_S (strict upper triangle zero).  One block per row.
__global__ __launch_bounds__(256) void collapsed_widen_kernel(const double* __restrict__ state, int n, const float* __restrict__ LS,
                                                              int64_t ldls, double* __restrict__ Gs, double* __restrict__ L64, int ldw) {
    const double* T = state + CS_HEAD;
    const int ldt = n + 1, i = blockIdx.x;
    for (int j = threadIdx.x; j < n; j += 256) {
        Gs[(int64_t)i * ldw + j] = stat(T, ldt, i, j);
        L64[(int64_t)i * ldw + j] = j <= i ? (double)LS[(int64_t)i * ldls + j] : 0.0;
    }
}

// evaluate, pass 2: per-row partial sums from P = G L_S, L_S, G and m.  One block per row.
__global__ __launch_bounds__(256) void collapsed_rowterms_kernel(const double* __restrict__ state, int n, const float* __restrict__ m,
                                                                 const double* __restrict__ Gs, const double* __restrict__ L64,
                                                                 const double* __restrict__ P, int ldw, double* __restrict__ part) {
    __shared__ double sh[256];
    const double* T = state + CS_HEAD;
    const int ldt = n + 1, i = blockIdx.x;
    double sg = 0.0, trs = 0.0, gm = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) {
        const double l = L64[(int64_t)i * ldw + j];
        sg += P[(int64_t)i * ldw + j] * l;
        trs += l * l;
        gm += Gs[(int64_t)i * ldw + j] * (double)m[j];
    }
    sg = block_sum(sg, sh);
    trs = block_sum(trs, sh);
    gm = block_sum(gm, sh);
    if (threadIdx.x == 0) {
        const double mi = (double)m[i];
        part[0 * n + i] = sg;
        part[1 * n + i] = trs;
        part[2 * n + i] = mi * gm;
        part[3 * n + i] = mi * mi;
        part[4 * n + i] = mi * T[(int64_t)n * ldt + i];
        part[5 * n + i] = Gs[(int64_t)i * ldw + i];
        part[6 * n + i] = log(L64[(int64_t)i * ldw + i]);
    }
}

// the scalars from the per-row partials, one block, fixed order.  optimum != 0: <S,G> and m^T G m from S = B^-1, B m = kappa b.
// scalars: loss, sum ll, KL, sum |residual|^2, sum varn, R, kappa, tr G
__global__ __launch_bounds__(1024) void collapsed_finish_kernel(const double* __restrict__ state, int n, const float* __restrict__ hyp,
                                                                double num_data, const double* __restrict__ part, int optimum,
                                                                const int* __restrict__ flags, double* __restrict__ scalars,
                                                                int* __restrict__ info) {
    __shared__ double sh[1024];
    double s[CS_NPART];
    for (int c = 0; c < CS_NPART; ++c) {
        double v = 0.0;
        for (int i = threadIdx.x; i < n; i += 1024) v += part[(size_t)c * n + i];
        s[c] = block_sum(v, sh);
    }
    if (threadIdx.x != 0) return;
    int code = 0;
    if (flags) code = flags[2] ? -2 : (flags[1] ? -1 : flags[0]);
    if (info) *info = code;
    if (!scalars) return;
    const double R = state[1], noise = (double)hyp[2], yy = state[CS_HEAD + (size_t)n * (n + 1) + n];
    const double kappa = num_data / (R * noise);
    double sg = s[0], mgm = s[2];
    const double trs = s[1], mm = s[3], mb = s[4], trg = s[5], slog = s[6];
    if (optimum) {
        sg = ((double)n - trs) / kappa;
        mgm = (kappa * mb - mm) / kappa;
    }
    const double res = yy - 2.0 * mb + mgm;
    const double varn = state[0] + R * 1e-4 + sg - trg + R * noise;
    const double ll = -0.5 * ((res + varn) / noise + R * log(noise) + R * 1.8378770664093453);
    const double kl = 0.5 * (trs + mm - (double)n - 2.0 * slog);
    const double loss = -(ll / R - kl / num_data);
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const double out[8] = {loss, ll, kl, res, varn, R, kappa, trg};
    for (int c = 0; c < 8; ++c) scalars[c] = (code != 0 && c < 5) ? qnan : out[c];
}

}  // namespace

extern "C" size_t dsvgp_collapsed_state_bytes(int Mp) {
    if (Mp <= 0) return 0;
    return sizeof(double) * (CS_HEAD + (size_t)(Mp + 1) * (Mp + 1));
}

extern "C" size_t dsvgp_collapsed_workspace_bytes(int Mp) {
    if (Mp <= 0 || Mp > CS_MAX_MP) return 0;
    return sizeof(double) * layout(Mp).total + 64;
}

extern "C" int dsvgp_collapsed_reset(dsvgp_ctx* ctx, void* state, int Mp) {
    if (!ctx || !state || Mp <= 0) return DSVGP_EINVAL;
    const hipError_t e = hipMemsetAsync(state, 0, dsvgp_collapsed_state_bytes(Mp), ctx->stream);
    return e == hipSuccess ? 0 : 1000 + (int)e;
}

extern "C" int dsvgp_collapsed_accumulate(dsvgp_ctx* ctx, void* state, int Mp, double* A64, int64_t lda, int Bp, const float* y,
                                          const float* constant, const float* prior_diag) {
    if (!ctx || !state || !A64 || !y || !constant || !prior_diag || Mp <= 0 || Bp < 0 || lda < Bp) return DSVGP_EINVAL;
    if (((uintptr_t)state % 8) || ((uintptr_t)A64 % 8)) return DSVGP_EALIGN;
    if (Bp == 0) return 0;
    double* st = (double*)state;
    const int blocks = cdiv(Bp, 1024) < 256 ? cdiv(Bp, 1024) : 256;
    hipLaunchKernelGGL(collapsed_rows_kernel, dim3(blocks), dim3(1024), 0, ctx->stream, st, A64 + (int64_t)Mp * lda, Bp, y, constant,
                       prior_diag);
    DSVGP_LAUNCH_CHECK();
    return collapsed_gram_update(ctx, st + CS_HEAD, Mp, A64, lda, Bp);
}

// T += tril([A ; r^T][A ; r^T]^T) in place (beta = 1, Cin == C): one pass below the launcher's split-K threshold, its fp64 atomics
// onto the live state above it (shared with dsvgp_collapsed_accumulate_masked, missing.hip)
int collapsed_gram_update(dsvgp_ctx* ctx, double* T, int Mp, const double* A64, int64_t lda, int Bp) {
    GemmArgs g{};
    g.M = Mp + 1; g.N = Mp + 1; g.K = Bp;
    g.A = A64; g.B = A64; g.Cin = T; g.C = T;
    g.lda = lda; g.ldb = lda; g.ldcin = Mp + 1; g.ldc = Mp + 1;
    g.alpha = 1.0; g.beta = 1.0; g.flags = DSVGP_GEMM_TRANS_B | DSVGP_GEMM_OUT_LOWER | DSVGP_GEMM_KEEP_UPPER;
    g.batch = 1; g.splitk = 1;
    g.slab = ctx->det_slab; g.slab_bytes = ctx->det_bytes;
    return launch_gemm(ctx->stream, 1, g);
}

extern "C" int dsvgp_collapsed_solve(dsvgp_ctx* ctx, const void* state, int Mp, const float* hyp, double num_data, float* m, float* LS,
                                     int64_t ldls, float* nat_vec, float* nat_mat, int64_t ldnm, double* scalars, int* info,
                                     void* workspace) {
    if (!ctx || !state || !hyp || !workspace || Mp <= 0 || Mp > CS_MAX_MP || !(num_data > 0.0)) return DSVGP_EINVAL;
    if ((LS && ldls < Mp) || (nat_mat && ldnm < Mp)) return DSVGP_EINVAL;
    if (((uintptr_t)state % 8) || ((uintptr_t)workspace % 16)) return DSVGP_EALIGN;
    const int n = Mp;
    const Layout l = layout(n);
    const double* st = (const double*)state;
    double* ws = (double*)workspace;
    int* flags = (int*)(ws + l.flags);
    hipError_t e = hipMemsetAsync(flags, 0, 64, ctx->stream);
    if (e != hipSuccess) return 1000 + (int)e;
    hipLaunchKernelGGL(collapsed_flip_kernel, dim3(n), dim3(256), 0, ctx->stream, st, n, hyp, num_data, ws + l.W, l.ldw, ws + l.v0, flags);
    DSVGP_LAUNCH_CHECK();
    // J B J = Ltilde Ltilde^T with Ltilde^-1 (and its transpose) from the same launches: chol(S*) = J Ltilde^-T J needs no second factor
    const bool pz = ctx->prezeroed;
    ctx->prezeroed = false;
    const int rc = dsvgp_potrf_inverse(ctx, ws + l.W, n, l.ldw, flags, ws + l.potrf, pow2_at_least(n), ws + l.trsm);
    ctx->prezeroed = pz;
    if (rc) return rc;
    const double* Dinv = ws + l.trsm;
    const double* DinvT = Dinv + (size_t)n * n;
    // m* = kappa J Ltilde^-T Ltilde^-1 J b
    hipLaunchKernelGGL(collapsed_trmv_kernel, dim3(n), dim3(256), 0, ctx->stream, Dinv, n, n, 1, ws + l.v0, ws + l.v1);
    hipLaunchKernelGGL(collapsed_trmv_kernel, dim3(n), dim3(256), 0, ctx->stream, DinvT, n, n, 0, ws + l.v1, ws + l.v2);
    hipLaunchKernelGGL(collapsed_unflip_kernel, dim3(n), dim3(256), 0, ctx->stream, st, n, hyp, num_data, DinvT, ws + l.v2, flags, m, LS, ldls,
                       nat_vec, nat_mat, ldnm, ws + l.part);
    hipLaunchKernelGGL(collapsed_finish_kernel, dim3(1), dim3(1024), 0, ctx->stream, st, n, hyp, num_data, ws + l.part, 1, flags, scalars,
                       info);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_collapsed_evaluate(dsvgp_ctx* ctx, const void* state, int Mp, const float* m, const float* LS, int64_t ldls,
                                        const float* hyp, double num_data, double* scalars, void* workspace) {
    if (!ctx || !state || !m || !LS || !hyp || !scalars || !workspace || Mp <= 0 || Mp > CS_MAX_MP || ldls < Mp || !(num_data > 0.0))
        return DSVGP_EINVAL;
    if (((uintptr_t)state % 8) || ((uintptr_t)workspace % 16)) return DSVGP_EALIGN;
    const int n = Mp;
    const Layout l = layout(n);
    const double* st = (const double*)state;
    double* ws = (double*)workspace;
    hipLaunchKernelGGL(collapsed_widen_kernel, dim3(n), dim3(256), 0, ctx->stream, st, n, LS, ldls, ws + l.W, ws + l.X, l.ldw);
    DSVGP_LAUNCH_CHECK();
    GemmArgs g{};                                   // P = G L_S: <S, G> = tr(L_S^T G L_S) = sum(P o L_S)
    g.M = n; g.N = n; g.K = n;
    g.A = ws + l.W; g.B = ws + l.X; g.C = ws + l.Y;
    g.lda = l.ldw; g.ldb = l.ldw; g.ldc = l.ldw;
    g.alpha = 1.0; g.beta = 0.0; g.flags = DSVGP_GEMM_B_LOWER;
    g.batch = 1; g.splitk = 1;
    g.slab = ctx->det_slab; g.slab_bytes = ctx->det_bytes;
    const int rc = launch_gemm(ctx->stream, 1, g);
    if (rc) return rc;
    hipLaunchKernelGGL(collapsed_rowterms_kernel, dim3(n), dim3(256), 0, ctx->stream, st, n, m, ws + l.W, ws + l.X, ws + l.Y, l.ldw,
                       ws + l.part);
    hipLaunchKernelGGL(collapsed_finish_kernel, dim3(1), dim3(1024), 0, ctx->stream, st, n, hyp, num_data, ws + l.part, 0,
                       (const int*)nullptr, scalars, (int*)nullptr);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

// ================================================================================================================================
// Gradients of the collapsed bound with respect to hyper-parameters and inducing points at the optimum of the same statistics
// (DESIGN.md section 24).  Envelope: the total derivative equals the partial one at fixed whitened (m*, S*), so only the expected
// log-likelihood contributes.  With alpha = L^-T m, Q = L^-T (S - I) L^-1, w = 1 / (2 R noise), rho = r - K^T alpha:
//     K-bar (chunk)  = 2 w (Q K - alpha rho^T)                      K~-bar = (Q + alpha alpha^T + kappa L^-T G L^-1) / (2 num_data)
//     dg-bar = w     c-bar = -2 w sum rho                            d/d noise = -(E + V) / (2 R noise^2) + 1 / noise
// adj (doubles): [0] w, [1] d loss / d noise, [2] dg-bar, [3] loss, [4] E, [5] V, [6] kappa, [7] R
namespace {

constexpr int CG_NADJ = 8;
constexpr int CG_SLAB = 256;                 // rows of K_ZX per slab of the residual's column reduction
constexpr int CG_EROWS = 32;                 // rows of K-bar per workgroup of the epilogue

struct GradLayout { size_t Gs, T, X, Y, part, scal, flags, total; int ldw; };   // prepare's workspace, in doubles
GradLayout grad_layout(int n) {
    GradLayout l{};
    l.ldw = (n + 1) & ~1;
    const size_t nn = al((size_t)n * l.ldw);
    size_t o = 0;
    l.Gs = o; o += nn;                       // symmetric G
    l.T = o; o += nn;                        // S - I              -> L^-T G L^-1
    l.X = o; o += nn;                        // L^-T (S - I)       -> L^-T G
    l.Y = o; o += nn;                        // fp64 tril L_S      -> L^-T (S - I) L^-1
    l.part = o; o += al((size_t)CS_NPART * n);
    l.scal = o; o += 8;
    l.flags = o; o += 8;
    l.total = o;
    return l;
}

// T = S - I in place, and the per-row partials of collapsed_finish_kernel's closed forms at the optimum.  One thread per row.
__global__ __launch_bounds__(256) void cgrad_diag_kernel(const double* __restrict__ state, int n, const float* __restrict__ m,
                                                         const float* __restrict__ LS, int64_t ldls, double* __restrict__ T, int ldw,
                                                         double* __restrict__ part) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* St = state + CS_HEAD;
    const int ldt = n + 1;
    const double sii = T[(int64_t)i * ldw + i], mi = (double)m[i];
    T[(int64_t)i * ldw + i] = sii - 1.0;
    part[0 * n + i] = 0.0;
    part[1 * n + i] = sii;
    part[2 * n + i] = 0.0;
    part[3 * n + i] = mi * mi;
    part[4 * n + i] = mi * St[(int64_t)n * ldt + i];
    part[5 * n + i] = St[(int64_t)i * ldt + i];
    part[6 * n + i] = log((double)LS[(int64_t)i * ldls + i]);
}

// alpha = L^-T m from the stored transposed image of the inverse (only k >= i of its row i is read): one block per entry, fixed order
__global__ __launch_bounds__(256) void cgrad_alpha_kernel(const double* __restrict__ DinvT, int n, const float* __restrict__ m,
                                                          double* __restrict__ alpha) {
    __shared__ double sh[256];
    const int i = blockIdx.x;
    double s = 0.0;
    for (int k = i + threadIdx.x; k < n; k += 256) s += DinvT[(int64_t)i * n + k] * (double)m[k];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) alpha[i] = s;
}

// Q and K~-bar, exactly symmetric, from the two raw products; block 0 also writes the scalar adjoints.  A non-finite entry raises
// the flag (integer atomic).  One block per row.
__global__ __launch_bounds__(256) void cgrad_final_kernel(int n, const float* __restrict__ hyp, double num_data,
                                                          const double* __restrict__ Yq, const double* __restrict__ Zg, int ldw,
                                                          const double* __restrict__ alpha, const double* __restrict__ scal,
                                                          double* __restrict__ Q, int64_t ldq, double* __restrict__ Kb, int64_t ldkb,
                                                          double* __restrict__ adj, int* __restrict__ info) {
    const int i = blockIdx.x;
    const double kappa = scal[6], ai = alpha[i], half = 0.5 / num_data;
    bool bad = false;
    for (int j = threadIdx.x; j < n; j += 256) {
        const double q = 0.5 * (Yq[(int64_t)i * ldw + j] + Yq[(int64_t)j * ldw + i]);
        const double z = 0.5 * (Zg[(int64_t)i * ldw + j] + Zg[(int64_t)j * ldw + i]);
        const double k = (q + ai * alpha[j] + kappa * z) * half;
        if (!isfinite(q) || !isfinite(k)) bad = true;
        Q[(int64_t)i * ldq + j] = q;
        Kb[(int64_t)i * ldkb + j] = k;
    }
    if (i == 0 && threadIdx.x == 0) {
        const double R = scal[5], noise = (double)hyp[2], E = scal[3], V = scal[4];
        const double w = 0.5 / (R * noise);
        const double out[CG_NADJ] = {w, -(E + V) / (2.0 * R * noise * noise) + 1.0 / noise, w, scal[0], E, V, kappa, R};
        for (int c = 0; c < CG_NADJ; ++c) {
            if (!isfinite(out[c])) bad = true;
            adj[c] = out[c];
        }
        if (!(R > 0.0)) bad = true;
    }
    if (bad) atomicOr(info, 1);
}

// the residual's column reduction, pass 1: part[slab][j] = sum over the slab's rows i of alpha_i K_ij, rows in ascending order.
// One thread per column (coalesced along j), the slab's alpha in LDS.
__global__ __launch_bounds__(256) void cgrad_reduce_kernel(const float* __restrict__ K, int64_t ldk, int Mp, int Bp,
                                                           const double* __restrict__ alpha, double* __restrict__ part) {
    __shared__ double sa[CG_SLAB];
    const int i0 = blockIdx.y * CG_SLAB;
    const int rows = (Mp - i0 < CG_SLAB) ? (Mp - i0) : CG_SLAB;
    if ((int)threadIdx.x < rows) sa[threadIdx.x] = alpha[i0 + threadIdx.x];
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= Bp) return;
    const float* col = K + (int64_t)i0 * ldk + j;
    double s = 0.0;
    for (int i = 0; i < rows; ++i) s += sa[i] * (double)col[(int64_t)i * ldk];
    part[(int64_t)blockIdx.y * Bp + j] = s;
}

// pass 2: rho_j = (y_j - c) - sum over the slabs in ascending order; the constant prior-diagonal adjoint for the diagonal's backward
__global__ __launch_bounds__(256) void cgrad_combine_kernel(const double* __restrict__ part, int nslab, int Bp, const float* __restrict__ y,
                                                            const float* __restrict__ constant, const double* __restrict__ adj,
                                                            double* __restrict__ rho, float* __restrict__ diag_bar) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= Bp) return;
    double s = 0.0;
    for (int t = 0; t < nslab; ++t) s += part[(int64_t)t * Bp + j];
    rho[j] = ((double)y[j] - (double)constant[0]) - s;
    if (diag_bar) diag_bar[j] = (float)adj[2];
}

// the epilogue, in place: K-bar_ij = 2 w (V_ij - alpha_i rho_j), rounded once.  Block (0, 0) alone adds sum rho onto the accumulator:
// strided chains joined by a fixed tree, one writer.
__global__ __launch_bounds__(256) void cgrad_epilogue_kernel(float* __restrict__ Kb, int64_t ldkb, int Mp, int Bp,
                                                             const double* __restrict__ alpha, const double* __restrict__ rho,
                                                             const double* __restrict__ adj, double* __restrict__ rho_sum) {
    __shared__ double sh[256];
    const int i0 = blockIdx.y * CG_EROWS;
    const int rows = (Mp - i0 < CG_EROWS) ? (Mp - i0) : CG_EROWS;
    const double w2 = 2.0 * adj[0];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < Bp) {
        const double rj = rho[j];
        float* col = Kb + (int64_t)i0 * ldkb + j;
        for (int i = 0; i < rows; ++i) col[(int64_t)i * ldkb] = (float)(w2 * ((double)col[(int64_t)i * ldkb] - alpha[i0 + i] * rj));
    }
    if (blockIdx.x != 0 || blockIdx.y != 0) return;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < Bp; t += 256) s += rho[t];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) rho_sum[0] += s;
}

}  // namespace

extern "C" size_t dsvgp_collapsed_grad_workspace_bytes(int Mp) {
    if (Mp <= 0 || Mp > CS_MAX_MP) return 0;
    return sizeof(double) * grad_layout(Mp).total + 64;
}

extern "C" size_t dsvgp_collapsed_grad_chunk_bytes(int Mp, int Bp) {
    if (Mp <= 0 || Mp > CS_MAX_MP || Bp <= 0) return 0;
    return sizeof(double) * ((size_t)cdiv(Mp, CG_SLAB) + 1) * (size_t)Bp;
}

extern "C" int dsvgp_collapsed_grad_prepare(dsvgp_ctx* ctx, const void* state, int Mp, const float* m, const float* LS, int64_t ldls,
                                            const double* inverse, const float* hyp, double num_data, double* alpha, double* Q,
                                            int64_t ldq, double* Kzz_bar, int64_t ldkb, double* adj, int* info, void* workspace) {
    if (!ctx || !state || !m || !LS || !inverse || !hyp || !alpha || !Q || !Kzz_bar || !adj || !info || !workspace || Mp <= 0 ||
        Mp > CS_MAX_MP || ldls < Mp || ldq < Mp || ldkb < Mp || !(num_data > 0.0))
        return DSVGP_EINVAL;
    if (((uintptr_t)state % 8) || ((uintptr_t)inverse % 8) || ((uintptr_t)alpha % 8) || ((uintptr_t)Q % 8) || ((uintptr_t)Kzz_bar % 8) ||
        ((uintptr_t)adj % 8) || ((uintptr_t)workspace % 16))
        return DSVGP_EALIGN;
    const int n = Mp;
    const GradLayout l = grad_layout(n);
    const double* st = (const double*)state;
    double* ws = (double*)workspace;
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemsetAsync(info, 0, sizeof(int), s);
    if (e != hipSuccess) return 1000 + (int)e;
    hipLaunchKernelGGL(collapsed_widen_kernel, dim3(n), dim3(256), 0, s, st, n, LS, ldls, ws + l.Gs, ws + l.Y, l.ldw);
    DSVGP_LAUNCH_CHECK();
    auto product = [&](const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int flags) {
        GemmArgs g{};
        g.M = n; g.N = n; g.K = n;
        g.A = A; g.B = B; g.C = C;
        g.lda = lda; g.ldb = ldb; g.ldc = l.ldw;
        g.alpha = 1.0; g.beta = 0.0; g.flags = flags;
        g.batch = 1; g.splitk = 1;
        g.slab = ctx->det_slab; g.slab_bytes = ctx->det_bytes;
        return launch_gemm(s, 1, g);
    };
    const bool pz = ctx->prezeroed;
    ctx->prezeroed = false;
    int rc = product(ws + l.Y, l.ldw, ws + l.Y, l.ldw, ws + l.T, DSVGP_GEMM_TRANS_B);                       // S = L_S L_S^T
    if (!rc) {
        hipLaunchKernelGGL(cgrad_diag_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, st, n, m, LS, ldls, ws + l.T, l.ldw, ws + l.part);
        hipLaunchKernelGGL(collapsed_finish_kernel, dim3(1), dim3(1024), 0, s, st, n, hyp, num_data, ws + l.part, 1, (const int*)nullptr,
                           ws + l.scal, (int*)nullptr);
        hipLaunchKernelGGL(cgrad_alpha_kernel, dim3(n), dim3(256), 0, s, inverse + (size_t)n * n, n, m, alpha);
        const hipError_t el = hipGetLastError();
        if (el != hipSuccess) rc = 1000 + (int)el;
    }
    // Q = L^-T (S - I) L^-1 and L^-T G L^-1: two triangular fp64 products each, against the stored inverse
    if (!rc) rc = product(inverse, n, ws + l.T, l.ldw, ws + l.X, DSVGP_GEMM_TRANS_A | DSVGP_GEMM_A_UPPER);
    if (!rc) rc = product(ws + l.X, l.ldw, inverse, n, ws + l.Y, DSVGP_GEMM_B_LOWER);
    if (!rc) rc = product(inverse, n, ws + l.Gs, l.ldw, ws + l.X, DSVGP_GEMM_TRANS_A | DSVGP_GEMM_A_UPPER);
    if (!rc) rc = product(ws + l.X, l.ldw, inverse, n, ws + l.T, DSVGP_GEMM_B_LOWER);
    ctx->prezeroed = pz;
    if (rc) return rc;
    hipLaunchKernelGGL(cgrad_final_kernel, dim3(n), dim3(256), 0, s, n, hyp, num_data, ws + l.Y, ws + l.T, l.ldw, alpha, ws + l.scal, Q, ldq,
                       Kzz_bar, ldkb, adj, info);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_collapsed_grad_chunk(dsvgp_ctx* ctx, int Mp, int Bp, const float* Kzx, int64_t ldk, const float* y,
                                          const float* constant, const double* Q, int64_t ldq, const double* alpha, const double* adj,
                                          float* K_bar, int64_t ldkb, float* diag_bar, double* rho_sum, void* workspace) {
    if (!ctx || !Kzx || !y || !constant || !Q || !alpha || !adj || !K_bar || !rho_sum || !workspace || Mp <= 0 || Mp > CS_MAX_MP ||
        Bp <= 0 || ldk < Bp || ldkb < Bp || ldq < Mp)
        return DSVGP_EINVAL;
    {   // K_bar is written while Kzx is still being read: the two extents must not overlap anywhere
        const uintptr_t k0 = (uintptr_t)Kzx, k1 = k0 + sizeof(float) * ((size_t)(Mp - 1) * ldk + Bp);
        const uintptr_t b0 = (uintptr_t)K_bar, b1 = b0 + sizeof(float) * ((size_t)(Mp - 1) * ldkb + Bp);
        if (k0 < b1 && b0 < k1) return DSVGP_EINVAL;
    }
    if (((uintptr_t)Q % 8) || ((uintptr_t)alpha % 8) || ((uintptr_t)adj % 8) || ((uintptr_t)rho_sum % 8) || ((uintptr_t)workspace % 8) ||
        ((uintptr_t)Kzx % 4) || ((uintptr_t)K_bar % 4))
        return DSVGP_EALIGN;
    hipStream_t s = ctx->stream;
    const int nslab = cdiv(Mp, CG_SLAB), gx = cdiv(Bp, 256);
    double* part = (double*)workspace;
    double* rho = part + (size_t)nslab * Bp;
    hipLaunchKernelGGL(cgrad_reduce_kernel, dim3(gx, nslab), dim3(256), 0, s, Kzx, ldk, Mp, Bp, alpha, part);
    hipLaunchKernelGGL(cgrad_combine_kernel, dim3(gx), dim3(256), 0, s, part, nslab, Bp, y, constant, adj, rho, diag_bar);
    DSVGP_LAUNCH_CHECK();
    // V = Q K_ZX, fp64 accumulation over the float right operand, rounded once to fp32 (the form of dsvgp_var_predict): never split
    // along K -- only the fp32 copy is asked for -- so the product has one fixed order.  Q is exactly symmetric: read as its transpose
    GemmArgs g{};
    g.M = Mp; g.N = Bp; g.K = Mp; g.A = Q; g.B = Kzx; g.C = nullptr; g.C32 = K_bar;
    g.lda = ldq; g.ldb = ldk; g.ldc = 0; g.ldc32 = ldkb;
    g.alpha = 1.0; g.beta = 0.0; g.flags = DSVGP_GEMM_TRANS_A | DSVGP_GEMM_B_IS_FLOAT; g.batch = 1; g.splitk = 1;
    g.slab = K_bar; g.slab_bytes = 0;
    if (int rc = launch_gemm(s, 1, g)) return rc;
    hipLaunchKernelGGL(cgrad_epilogue_kernel, dim3(gx, cdiv(Mp, CG_EROWS)), dim3(256), 0, s, K_bar, ldkb, Mp, Bp, alpha, rho, adj, rho_sum);
    DSVGP_LAUNCH_CHECK();
    return 0;
}
