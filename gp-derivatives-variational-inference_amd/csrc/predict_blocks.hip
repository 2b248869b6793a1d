// Per-point predictive covariance blocks, gfx950: the q x q diagonal blocks (q = pd + 1) of
//     s K_XX + (1e-4 + noise) I + W^T W - A^T A
// one per data point, straight from A = L^-1 K_ZX and W = L_S^T A [Mp, B q] (interleaved columns) -- no K_XX, nothing of size
// B q x B q.  Var f(x), Cov(f(x), D f(x)) and Cov D f(x) at every point: what predict's marginal variances do not carry and what
// predict_joint pays B q x B q floats for.
//
// Launch 1 (pred_blocks_gram_kernel), one workgroup (256 threads) per (group, slice) of pred_blocks_plan.h: a group is a strip of
// G = max(1, 96 / q) whole points (Tc = G q <= 96 columns, the tile rule of assemble_wide.hip), a slice `rps` of the Mp rows.  The
// workgroup walks its rows in chunks of 32: [32][Tc] of W and of A go through registers (coalesced along the columns; the next chunk
// is in flight while the current one is multiplied) into two LDS images of row stride ld = 16 mod 32, and the strip's Gram
// accumulates on v_mfma_f32_16x16x4_f32.  For C += X^T X both operands of a tile pair are fragments of the same [k][column] image: the
// lane's read (column = lane & 15, k = lane >> 4) is conflict-free in each half-wave.  The A term enters the same accumulators with
// one operand negated.  Only the live tile pairs run (those that meet a point's diagonal block: 12 of 21 at q = 21), wave w owns the
// pairs w, w + 4, ...: at most 6 accumulators of 4 registers.  The lower part of every block goes to the workspace,
// part[slice][point][a][b <= a] -- plain vector stores, every element by exactly one lane (tools/pred_blocks_check.cpp).
// Launch 2 (pred_blocks_finish_kernel), one thread per output element (point, a, b): the slices added in the order 0, 1, ..., read at
// (max(a, b), min(a, b)) so that the block is exactly symmetric, plus the prior block at r = 0 -- s / (s / ell^2) on the diagonal as
// predictive_stats has it, s (v^_a . v^_b) / ell^2 between two derivative rows from the unit direction rows of the data pack (one
// fmaf chain over d in k order), 0 between the value and a derivative -- plus the jitter and the noise on the diagonal.
// No floating-point atomics and no sum whose order depends on anything but (Mp, B, pd, d): two identical calls are bitwise equal, on
// any card.  With a zero middle term (W null or W == A) launch 1 does not run and nothing is read from A.
// LDS: 2 x 32 x ld floats <= 28672 bytes (ld = 112 at Tcp = 96).  f32-input MFMA runs at the fp32 vector rate; it is used because it
// keeps the accumulators compact, leaves the VALU to the loads and is exact fp32, not for flops.
#include "common.h"
#include "pred_blocks_plan.h"

namespace {

constexpr float KXX_JITTER = 1e-4f;     // data_data_covar.add_jitter(1e-4), reference DGVS.py:197,203 (as elbo.hip)
using f4 = float __attribute__((ext_vector_type(4)));

constexpr int PB_RPW = PB_KC / (PB_NT / 64);       // chunk rows per wave: 8
constexpr int PB_LDMAX = PB_TMAX + 16;             // 112

__global__ __launch_bounds__(PB_NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void pred_blocks_gram_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ W,
                                                                 int64_t ldw, int Mp, int B, int q, int Tc, int Tcp, int ld, int rps,
                                                                 int G, float* __restrict__ part) {
    __shared__ float Ws[PB_KC * PB_LDMAX];
    __shared__ float As[PB_KC * PB_LDMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t col0 = (int64_t)blockIdx.x * Tc;
    const int cols = (int)min((int64_t)Tc, (int64_t)B * q - col0);           // (whole points: B q and Tc are multiples of q)
    const int r0 = blockIdx.y * rps, r1 = min(Mp, r0 + rps);
    const int ntile = Tcp >> 4;

    // this wave's live tile pairs: LDS offsets of their two fragments
    int oi[PB_MAXPAIRS], oj[PB_MAXPAIRS];
    int np = 0;
#pragma unroll
    for (int i = 0; i < PB_MAXPAIRS; ++i) {
        int ti = 0, tj = 0;
        const bool live = pred_blocks_pair(wave + 4 * i, ntile, q, Tc, ti, tj);
        oi[i] = ti * 16 + (lane & 15) + (lane >> 4) * ld;
        oj[i] = tj * 16 + (lane & 15) + (lane >> 4) * ld;
        if (live) np = i + 1;
    }

    // chunk loads: wave w takes the rows w, w + 4, ... of the chunk, lane l the columns l and l + 64
    float pw[PB_RPW][2], pa[PB_RPW][2];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < PB_RPW; ++i) {
            const int r = k0 + i * 4 + wave;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = lane + 64 * h;
                const bool in = r < r1 && c < cols;
                pw[i][h] = in ? W[(int64_t)r * ldw + col0 + c] : 0.f;
                pa[i][h] = in ? A[(int64_t)r * lda + col0 + c] : 0.f;
            }
        }
    };
    f4 acc[PB_MAXPAIRS];
#pragma unroll
    for (int i = 0; i < PB_MAXPAIRS; ++i) acc[i] = f4{0.f, 0.f, 0.f, 0.f};
    load(r0);
    for (int k0 = r0; k0 < r1; k0 += PB_KC) {
        __syncthreads();                    // the previous chunk's MFMA reads are done
#pragma unroll
        for (int i = 0; i < PB_RPW; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = lane + 64 * h;
                if (c < Tcp) {              // (columns cols .. Tcp - 1 and rows past r1 hold zeros)
                    Ws[(i * 4 + wave) * ld + c] = pw[i][h];
                    As[(i * 4 + wave) * ld + c] = pa[i][h];
                }
            }
        __syncthreads();
        if (k0 + PB_KC < r1) load(k0 + PB_KC);
#pragma unroll 2
        for (int kk = 0; kk < PB_KC; kk += 4) {
#pragma unroll
            for (int i = 0; i < PB_MAXPAIRS; ++i)
                if (i < np) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ws[kk * ld + oi[i]], Ws[kk * ld + oj[i]], acc[i], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < PB_MAXPAIRS; ++i)
                if (i < np) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(-As[kk * ld + oi[i]], As[kk * ld + oj[i]], acc[i], 0, 0, 0);
        }
    }

    // accumulator element (strip row i, strip column j) -> part[slice][point][a][b], the lower part of the point's block
    float* out = part + ((int64_t)blockIdx.y * B + (int64_t)blockIdx.x * G) * q * q;
#pragma unroll
    for (int i = 0; i < PB_MAXPAIRS; ++i) {
        if (i < np) {
            int ti = 0, tj = 0;
            pred_blocks_pair(wave + 4 * i, ntile, q, Tc, ti, tj);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int pt, a, b;
                if (pred_blocks_element(ti * 16 + (lane >> 4) * 4 + r, tj * 16 + (lane & 15), q, cols, pt, a, b))
                    out[((int64_t)pt * q + a) * q + b] = acc[i][r];
            }
        }
    }
}

__global__ __launch_bounds__(256) void pred_blocks_finish_kernel(const float* __restrict__ part, int nslices, int B, int q,
                                                                 const float* __restrict__ PX, int d, int DP,
                                                                 const float* __restrict__ hyp, int with_noise,
                                                                 float* __restrict__ blocks) {
    const int64_t n = (int64_t)B * q * q;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int64_t pt = e / (q * q);
    const int ab = (int)(e - pt * q * q);
    const int a = ab / q, b = ab - a * q;
    const int hi = max(a, b), lo = min(a, b);
    float sq = 0.f;
    const float* src = part + (pt * q + hi) * q + lo;
    for (int s = 0; s < nslices; ++s) sq += src[(int64_t)s * n];
    const float ell = hyp[0], s = hyp[1];
    float v;
    if (a == b) {
        const float dg = a == 0 ? s : s / (ell * ell);                       // (colstats_finish_kernel's closed form, elbo.hip)
        v = dg + KXX_JITTER + sq;
        if (with_noise) v += hyp[2];
    } else if (lo == 0) {
        v = sq;                                                              // Cov(f, D_a f) of the prior vanishes at r = 0
    } else {
        const float* va = PX + (pt * q + hi) * DP;
        const float* vb = PX + (pt * q + lo) * DP;
        float t = 0.f;
        for (int k = 0; k < d; ++k) t = __builtin_fmaf(va[k], vb[k], t);
        const float il = 1.f / ell;
        v = s * (t * (il * il)) + sq;
    }
    blocks[e] = v;
}

}  // namespace

extern "C" size_t dsvgp_predictive_blocks_workspace_bytes(int Mp, int B, int pd) {
    PredBlocksPlan w;
    if (pred_blocks_plan(Mp, B, pd, w)) return 0;
    return sizeof(float) * (size_t)w.nslices * (size_t)B * w.q * w.q;
}

extern "C" int dsvgp_predictive_blocks(dsvgp_ctx* ctx, const float* A, int64_t lda, const float* W, int64_t ldw, int Mp, int B, int pd,
                                       const float* PX, int d, const float* hyp, int with_noise, float* blocks, void* workspace,
                                       size_t workspace_bytes) {
    if (!ctx || !A || !blocks || !hyp || d < 1) return DSVGP_EINVAL;
    PredBlocksPlan w;
    if (pred_blocks_plan(Mp, B, pd, w)) return DSVGP_EINVAL;
    if (pd > 0 && !PX) return DSVGP_EINVAL;
    if (lda < w.ncols || (W && ldw < w.ncols)) return DSVGP_EINVAL;
    const size_t need = dsvgp_predictive_blocks_workspace_bytes(Mp, B, pd);
    if (workspace_bytes < need || !workspace || (uintptr_t)workspace % 4) return DSVGP_EINVAL;
    const int64_t n = w.ncols * w.q;
    if ((n + 255) / 256 > 0x7fffffffLL) return DSVGP_EINVAL;
    const bool middle = W && W != A;
    if (middle) {
        hipLaunchKernelGGL(pred_blocks_gram_kernel, dim3(w.ngroups, w.nslices), dim3(PB_NT), 0, ctx->stream, A, lda, W, ldw, Mp, B, w.q,
                           w.Tc, w.Tcp, w.ld, w.rps, w.G, (float*)workspace);
        DSVGP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pred_blocks_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const float*)workspace,
                       middle ? w.nslices : 0, B, w.q, PX, d, dsvgp_packed_width(d), hyp, with_noise, blocks);
    DSVGP_LAUNCH_CHECK();
    return 0;
}
