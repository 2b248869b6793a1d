// Data-driven initialisation (include/dsvgp.h, "k-means"): Lloyd's algorithm for the inducing points and the per-cluster second-moment
// matrices of the gradients for the inducing directions.
//
// Assignment, two routes with one tie rule (an exact tie goes to the lowest centroid index):
//   d <= 32   ONE fused kernel of mean_fused_kernel's shape (predict_mean.hip): a workgroup owns 64 points (lane = point, the point in
//             registers), the centroids stream through LDS in chunks of 64 read as wave-wide broadcasts, wave w takes centroids w, w + 8, ..
//             of every chunk, the distance is the DIFFERENCE form sum_k (z_k - x_k)^2 by FMAs in the order of k, a lane replaces its
//             running (best, index) on a strict < only, and the eight partial winners meet through LDS in the order 0..7.  The result of a
//             point depends on that point and on Z alone.
//   d > 32    S = X~ Z~^T on the unsplit fp32 MFMA GEMM in row blocks of KM_ROWS, X~ and Z~ centred on the column mean of Z (which keeps the
//             cancellation of the expansion |x~|^2 + |z~|^2 - 2 x~.z~ small), then one wave per row over |z~|^2 - 2 S: lanes stride the
//             centroids in index order, a butterfly that prefers the lower index on equality.
// Update: one workgroup per centroid walks ALL labels in order (they stay in L2), a wave ballots 64 labels at a time and adds the matching
// rows, in point order, lanes over the columns, into fp64 accumulators in registers; the waves' partial sums are added in the order 0, 1, ..
// The order of every sum is fixed by N and the labels alone: no sort, no floating-point atomics, two identical calls return the same bits.
// Moments: the same walk per (cluster, 32 x 32 tile of the upper triangle), fp64 accumulators, lanes over tile entries.
#include <limits.h>

#include "common.h"
#include "kmeans_plan.h"

namespace {

__device__ __forceinline__ float wave_sum(float v) {      // butterfly: the same order on every call, the sum in every lane
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- fused assignment (d <= 32): D = pad4(d) -------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(KM_NW * 64) void kmeans_assign_fused_kernel(const float* __restrict__ x, int64_t N, int d,
                                                                         const float* __restrict__ Z, int M, int wide,
                                                                         int* __restrict__ labels, float* __restrict__ dist2,
                                                                         int* __restrict__ moved) {
    __shared__ __align__(16) float sZ[KM_CH * D];
    __shared__ float sBest[KM_NW * KM_TP];
    __shared__ int sIdx[KM_NW * KM_TP];
    const int tid = threadIdx.x, lane = tid & 63, slice = tid >> 6;
    const int64_t b = (int64_t)blockIdx.x * KM_TP + lane;
    float xt[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xt[k] = (k < d && b < N) ? x[b * d + k] : 0.f;
    float best = INFINITY;
    int idx = INT_MAX;
    for (int c0 = 0; c0 < M; c0 += KM_CH) {
        const int nc = M - c0 < KM_CH ? M - c0 : KM_CH;
        __syncthreads();                                  // the previous chunk has been consumed
        if (wide) {                                       // d == D and Z 16-byte aligned: rows are whole float4s
            const float4* src = reinterpret_cast<const float4*>(Z + (size_t)c0 * D);
            for (int t = tid; t < nc * (D / 4); t += KM_NW * 64) reinterpret_cast<float4*>(sZ)[t] = src[t];
        } else {
            for (int t = tid; t < nc * D; t += KM_NW * 64) {
                const KmStage s = km_stage(t, 0, c0, d, D, false);
                sZ[s.lds] = s.glob >= 0 ? Z[s.glob] : 0.f;
            }
        }
        __syncthreads();
        for (int i = slice; i < nc; i += KM_NW) {         // every LDS read below is one address per wave (broadcast)
            const float* z = sZ + i * D;
            float r2 = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const float r = z[k] - xt[k];
                r2 = __builtin_fmaf(r, r, r2);
            }
            if (r2 < best) { best = r2; idx = c0 + i; }   // strict: within a wave the lowest index keeps a tie
        }
    }
    sBest[slice * KM_TP + lane] = best;
    sIdx[slice * KM_TP + lane] = idx;
    __syncthreads();
    if (slice != 0) return;
    for (int s = 1; s < KM_NW; ++s) {                     // the eight partial winners in the order 0..7
        const float ob = sBest[s * KM_TP + lane];
        const int oi = sIdx[s * KM_TP + lane];
        if (ob < best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    const int label = idx == INT_MAX ? 0 : idx;           // (a point with a NaN coordinate compares false everywhere)
    const bool live = b < N;
    if (moved) {
        const unsigned long long changed = __ballot(live && labels[live ? b : 0] != label);
        if (lane == 0 && changed) atomicAdd(moved, __popcll(changed));
    }
    if (live) {
        labels[b] = label;
        dist2[b] = best;
    }
}

template <int D>
int launch_assign_fused(hipStream_t st, const float* x, int N, int d, const float* Z, int M, int* labels, float* dist2, int* moved) {
    const int wide = (d == D) && ((uintptr_t)Z % 16 == 0);
    hipLaunchKernelGGL((kmeans_assign_fused_kernel<D>), dim3(cdiv(N, KM_TP)), dim3(KM_NW * 64), 0, st, x, (int64_t)N, d, Z, M, wide, labels,
                       dist2, moved);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

// ---- composed assignment (d > 32) ------------------------------------------------------------------------------------------------
// column means of Z (one block per column of the padded width, fixed summation order: column_mean_kernel's shape); padding columns zero
__global__ __launch_bounds__(256) void kmeans_center_kernel(const float* __restrict__ Z, int M, int d, float* __restrict__ center) {
    __shared__ double part[256];
    const int k = blockIdx.x;
    double acc = 0.0;
    if (k < d)
        for (int i = threadIdx.x; i < M; i += 256) acc += Z[(int64_t)i * d + k];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) center[k] = k < d ? (float)(part[0] / (double)M) : 0.f;
}

// out = src - center, zero padded to ldw, and its squared row norms: one wave per row
__global__ __launch_bounds__(256) void kmeans_pack_kernel(const float* __restrict__ src, int rows, int d, int ldw,
                                                         const float* __restrict__ center, float* __restrict__ out,
                                                         float* __restrict__ nrm) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float acc = 0.f;
    for (int k = lane; k < ldw; k += 64) {
        const float v = k < d ? src[(int64_t)row * d + k] - center[k] : 0.f;
        out[(int64_t)row * ldw + k] = v;
        acc = __builtin_fmaf(v, v, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) nrm[row] = acc;
}

// arg-min over |z~|^2 - 2 S of one row block: one wave per row, lanes stride the centroids in index order
__global__ __launch_bounds__(256) void kmeans_argmin_kernel(const float* __restrict__ S, int ldS, int rows, int M,
                                                           const float* __restrict__ nz, const float* __restrict__ xn,
                                                           int* __restrict__ labels, float* __restrict__ dist2, int* __restrict__ moved) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* Sr = S + (int64_t)row * ldS;
    float best = INFINITY;
    int idx = INT_MAX;
    for (int i = lane; i < M; i += 64) {
        const float v = __builtin_fmaf(-2.f, Sr[i], nz[i]);
        if (v < best) { best = v; idx = i; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(idx, off);
        if (ob < best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    if (lane == 0) {
        const int label = idx == INT_MAX ? 0 : idx;
        if (moved && labels[row] != label) atomicAdd(moved, 1);
        labels[row] = label;
        dist2[row] = fmaxf(xn[row] + best, 0.f);
    }
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

// ---- inertia: sum of dist2 in fp64, one workgroup, thread-strided chains joined by a fixed tree ------------------------------------
__global__ __launch_bounds__(1024) void kmeans_inertia_kernel(const float* __restrict__ dist2, int64_t N, double* __restrict__ out) {
    __shared__ double part[1024];
    double acc = 0.0;
    int64_t i = threadIdx.x;
    for (; i + 7 * 1024 < N; i += 8 * 1024) {             // eight loads in flight, added in the order of the plain loop below
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = dist2[i + u * 1024];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (double)v[u];
    }
    for (; i < N; i += 1024) acc += (double)dist2[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = part[0];
}

__global__ __launch_bounds__(256) void kmeans_count_kernel(const int* __restrict__ labels, int64_t N, int M, int* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        const int l = labels[i];
        if (l >= 0 && l < M) atomicAdd(counts + l, 1);    // (integer: the order does not change the result)
    }
}

// ---- update: one workgroup per centroid, the in-order walk of all labels ---------------------------------------------------------
template <int R>
__global__ __launch_bounds__(KM_UPD_NW * 64) void kmeans_update_kernel(const float* __restrict__ x, int64_t N, int d,
                                                                       const int* __restrict__ labels, float* __restrict__ Z,
                                                                       int* __restrict__ counts) {
    __shared__ double sAcc[KM_UPD_NW][64 * R];
    __shared__ int sCnt[KM_UPD_NW];
    const int m = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t nblk = (N + 63) / 64;
    int total = 0;
    for (int k0 = 0; k0 < d; k0 += 64 * R) {              // passes over the columns (one for d <= 64 R)
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0;
        int cnt = 0;
        for (int64_t b = (int64_t)wv * KM_UPD_UNROLL; b < nblk; b += KM_UPD_NW * KM_UPD_UNROLL) {
            int lab[KM_UPD_UNROLL];
#pragma unroll
            for (int u = 0; u < KM_UPD_UNROLL; ++u) {
                const int64_t i = (b + u) * 64 + lane;
                lab[u] = i < N ? labels[i] : -1;
            }
#pragma unroll
            for (int u = 0; u < KM_UPD_UNROLL; ++u) {
                unsigned long long mask = __ballot(lab[u] == m);
                cnt += __popcll(mask);
                while (mask) {                            // the members of this block, in point order
                    const int j = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const float* xr = x + ((b + u) * 64 + j) * d + k0;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int k = r * 64 + lane;
                        if (k0 + k < d) acc[r] += (double)xr[k];
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) sAcc[wv][r * 64 + lane] = acc[r];
        if (lane == 0) sCnt[wv] = cnt;
        __syncthreads();
        if (wv == 0) {                                    // the waves' partial sums in the order 0, 1, ..
            total = 0;
            for (int w = 0; w < KM_UPD_NW; ++w) total += sCnt[w];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int k = r * 64 + lane;
                double s = sAcc[0][k];
                for (int w = 1; w < KM_UPD_NW; ++w) s += sAcc[w][k];
                if (k0 + k < d && total > 0) Z[(int64_t)m * d + k0 + k] = (float)(s / (double)total);   // an empty cluster keeps its row
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[m] = total;
}

// ---- cluster moments: C_m = sum_{i in m} g_i g_i^T, one workgroup per (cluster, tile of the upper triangle) ------------------------
__global__ __launch_bounds__(256) void kmeans_moments_kernel(const float* __restrict__ g, int64_t N, int d, const int* __restrict__ labels,
                                                            double* __restrict__ C) {
    const int m = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int tr, tc;
    km_mom_tile(blockIdx.y, d, &tr, &tc);
    const int gc = tc * KM_MOM_T + (lane & 31);
    const int gr0 = tr * KM_MOM_T + wv * 8 + (lane >> 5);       // this lane's rows: gr0, gr0 + 2, gr0 + 4, gr0 + 6
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t nblk = (N + 63) / 64;
    for (int64_t b = 0; b < nblk; b += KM_UPD_UNROLL) {         // every wave walks every label: its entries see the points in order
        int lab[KM_UPD_UNROLL];
#pragma unroll
        for (int u = 0; u < KM_UPD_UNROLL; ++u) {
            const int64_t i = (b + u) * 64 + lane;
            lab[u] = i < N ? labels[i] : -1;
        }
#pragma unroll
        for (int u = 0; u < KM_UPD_UNROLL; ++u) {
            unsigned long long mask = __ballot(lab[u] == m);
            while (mask) {
                const int j = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const float* gi = g + ((b + u) * 64 + j) * d;
                const double bv = gc < d ? (double)gi[gc] : 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int gr = gr0 + 2 * q;
                    const double av = gr < d ? (double)gi[gr] : 0.0;
                    acc[q] += av * bv;                     // (a product of two floats is exact in fp64: C_m is symmetric to the bit)
                }
            }
        }
    }
    double* Cm = C + (int64_t)m * d * d;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int gr = gr0 + 2 * q;
        if (gr < d && gc < d) {
            Cm[(int64_t)gr * d + gc] = acc[q];
            if (tr != tc) Cm[(int64_t)gc * d + gr] = acc[q];     // the lower triangle is the mirror
        }
    }
}

bool bad_shape(int N, int d, int M) { return N < 1 || d < 1 || M < 1 || M > N; }

// the checks of the assignment that touch nothing: 0, or the refusal
int assign_check(const dsvgp_ctx* ctx, const float* x, int N, int d, const float* Z, int M, const int* labels, const float* dist2,
                 const void* workspace) {
    if (!ctx || !x || !Z || !labels || !dist2 || bad_shape(N, d, M)) return DSVGP_EINVAL;
    if (d <= KM_FUSED_MAX_D) return 0;
    KmLayout L;
    if (!workspace || (uintptr_t)workspace % 16 || !km_layout(N, d, M, &L)) return DSVGP_EINVAL;
    return 0;
}

int assign_launch(dsvgp_ctx* ctx, const float* x, int N, int d, const float* Z, int M, int* labels, float* dist2, int* moved,
                  void* workspace) {
    hipStream_t st = ctx->stream;
    if (d <= KM_FUSED_MAX_D) {
        switch (km_pad4(d)) {
            case 4: return launch_assign_fused<4>(st, x, N, d, Z, M, labels, dist2, moved);
            case 8: return launch_assign_fused<8>(st, x, N, d, Z, M, labels, dist2, moved);
            case 12: return launch_assign_fused<12>(st, x, N, d, Z, M, labels, dist2, moved);
            case 16: return launch_assign_fused<16>(st, x, N, d, Z, M, labels, dist2, moved);
            case 20: return launch_assign_fused<20>(st, x, N, d, Z, M, labels, dist2, moved);
            case 24: return launch_assign_fused<24>(st, x, N, d, Z, M, labels, dist2, moved);
            case 28: return launch_assign_fused<28>(st, x, N, d, Z, M, labels, dist2, moved);
            default: return launch_assign_fused<32>(st, x, N, d, Z, M, labels, dist2, moved);
        }
    }
    KmLayout L;
    km_layout(N, d, M, &L);
    float* ws = (float*)workspace;
    float *center = ws + L.o_center, *Zt = ws + L.o_z, *nz = ws + L.o_nz, *Xt = ws + L.o_x, *xn = ws + L.o_xn, *S = ws + L.o_S;
    hipLaunchKernelGGL(kmeans_center_kernel, dim3(L.ldw), dim3(256), 0, st, Z, M, d, center);
    DSVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(kmeans_pack_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, Z, M, d, L.ldw, center, Zt, nz);
    DSVGP_LAUNCH_CHECK();
    for (int64_t r0 = 0; r0 < N; r0 += L.R) {
        const int rows = (int)(N - r0 < L.R ? N - r0 : L.R);
        hipLaunchKernelGGL(kmeans_pack_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x + r0 * d, rows, d, L.ldw, center, Xt, xn);
        DSVGP_LAUNCH_CHECK();
        // S = X~ Z~^T  (both operands k-contiguous, zero-filled from d up to ldw)
        if (int rc = unsplit_gemm(ctx, DSVGP_GEMM_TRANS_B | DSVGP_GEMM_K_PADDED, rows, M, d, Xt, L.ldw, Zt, L.ldw, S, L.ldS)) return rc;
        hipLaunchKernelGGL(kmeans_argmin_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, S, L.ldS, rows, M, nz, xn, labels + r0, dist2 + r0,
                           moved);
        DSVGP_LAUNCH_CHECK();
    }
    return 0;
}

int update_launch(hipStream_t st, const float* x, int N, int d, const int* labels, float* Z, int M, int* counts) {
    switch (km_update_regs(d)) {
        case 1: hipLaunchKernelGGL((kmeans_update_kernel<1>), dim3(M), dim3(KM_UPD_NW * 64), 0, st, x, (int64_t)N, d, labels, Z, counts); break;
        case 2: hipLaunchKernelGGL((kmeans_update_kernel<2>), dim3(M), dim3(KM_UPD_NW * 64), 0, st, x, (int64_t)N, d, labels, Z, counts); break;
        default: hipLaunchKernelGGL((kmeans_update_kernel<KM_UPD_MAXR>), dim3(M), dim3(KM_UPD_NW * 64), 0, st, x, (int64_t)N, d, labels, Z, counts);
    }
    DSVGP_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" size_t dsvgp_kmeans_workspace_bytes(int N, int d, int M) {
    if (bad_shape(N, d, M) || d <= KM_FUSED_MAX_D) return 0;      // the fused kernel keeps everything in registers and LDS
    KmLayout L;
    if (!km_layout(N, d, M, &L)) return 0;
    return (L.total * sizeof(float) + 15) & ~(size_t)15;
}

extern "C" int dsvgp_kmeans_assign(dsvgp_ctx* ctx, const float* x, int N, int d, const float* Z, int M, int* labels, float* dist2,
                                   void* workspace) {
    if (int rc = assign_check(ctx, x, N, d, Z, M, labels, dist2, workspace)) return rc;
    return assign_launch(ctx, x, N, d, Z, M, labels, dist2, nullptr, workspace);
}

extern "C" int dsvgp_kmeans_update(dsvgp_ctx* ctx, const float* x, int N, int d, const int* labels, float* Z, int M, int* counts) {
    if (!ctx || !x || !labels || !Z || !counts || bad_shape(N, d, M)) return DSVGP_EINVAL;
    return update_launch(ctx->stream, x, N, d, labels, Z, M, counts);
}

extern "C" int dsvgp_kmeans_lloyd(dsvgp_ctx* ctx, const float* x, int N, int d, float* Z, int M, int iterations, int* labels, float* dist2,
                                  int* counts, double* inertia, int* moved, void* workspace) {
    if (iterations < 0 || !counts || !inertia || (iterations > 0 && !moved)) return DSVGP_EINVAL;
    if (int rc = assign_check(ctx, x, N, d, Z, M, labels, dist2, workspace)) return rc;
    hipStream_t st = ctx->stream;
    if (iterations > 0) {
        hipError_t e = hipMemsetAsync(moved, 0, (size_t)iterations * sizeof(int), st);
        if (e != hipSuccess) return 1000 + (int)e;
    }
    for (int t = 0; t <= iterations; ++t) {               // assign -> inertia -> update, and the closing assignment
        if (int rc = assign_launch(ctx, x, N, d, Z, M, labels, dist2, t > 0 ? moved + (t - 1) : nullptr, workspace)) return rc;
        hipLaunchKernelGGL(kmeans_inertia_kernel, dim3(1), dim3(1024), 0, st, dist2, (int64_t)N, inertia + t);
        DSVGP_LAUNCH_CHECK();
        if (t < iterations)
            if (int rc = update_launch(st, x, N, d, labels, Z, M, counts)) return rc;
    }
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)M * sizeof(int), st);     // the sizes of the clusters of the closing assignment
    if (e != hipSuccess) return 1000 + (int)e;
    hipLaunchKernelGGL(kmeans_count_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, labels, (int64_t)N, M, counts);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsvgp_cluster_moments(dsvgp_ctx* ctx, const float* g, int N, int d, const int* labels, int M, double* C, void* workspace) {
    (void)workspace;                                      // (nothing is staged outside registers)
    if (!ctx || !g || !labels || !C || bad_shape(N, d, M) || d > KM_MOM_MAX_D) return DSVGP_EINVAL;
    hipLaunchKernelGGL(kmeans_moments_kernel, dim3(M, km_mom_tiles(d)), dim3(256), 0, ctx->stream, g, (int64_t)N, d, labels, C);
    DSVGP_LAUNCH_CHECK();
    return 0;
}
