// K-looped tiled assembly, gfx950: the formulation of assemble.hip (header comment there) with T = P1 P2^T accumulated over a K loop of
// fixed 32-column chunks staged through LDS (wide_product.h), so that a workgroup's LDS does not grow with d.  The forward and the Tbar
// kernel are the family-templated ones of tiled_assembly.h, with the plan of tiles, grid, LDS and workspace and the launchers; this file
// holds the RBF family's radial algebra (RbfRadial), the contraction kernel, which no family touches, and the entries.  Two uses, one set
// of kernels:
//   wide        packed width > 96 (d >= 93), both sides with the model's p directions: dsvgp_kernel_fwd / _bwd take these kernels by
//               themselves there, dsvgp_kernel_fwd_wide / _bwd_wide (assemble.hip) whatever d;
//   rectangular out[n1 (p1 + 1), n2 (p2 + 1)] = s K(x1, x2; v1, v2) when the two point sets carry DIFFERENT numbers of directions, any d --
//               the K_ZX of a model with p inducing directions at data with pd directions per point (pd = 0: function values only; pd = d:
//               the full gradient): dsvgp_kernel_fwd_rect / _bwd_rect, at the end of this file.  A packed row does not know how many
//               direction rows follow it, so each side is packed by dsvgp_pack_points with ITS OWN p (and the same centre); T then holds
//               every inner product of the micro-block (i, j),
//                   T[i0,j0] = x1~.x2~      T[i0,jb] = x1~.v2_b      T[ia,j0] = v1_a.x2~      T[ia,jb] = v1_a.v2_b        a <= p1, b <= p2
//               and only the micro-block shape changes: (p1 + 1) x (p2 + 1).
// The kernels take a row period q1 = p1 + 1 and a column period q2 = p2 + 1; the wide entries pass the same q for both.
//
// Tiles (tile_plan): one 256-thread workgroup per tile of Rr x Rc micro-blocks, Tr = Rr q1 <= 96 rows by Tc = Rc q2 <= 96 columns.  Each
// side fills the 96-wide tile with whole points on its own (the tile shapes of kernel_fwd_kernel / kernel_bwd_kernel at q1 == q2),
//     Rc = 96 / q2,   Rr = max(1, (96 / q1) / 2),   Trp / Tcp = Tr / Tc padded to 16,
// so q = 96 on one side and q = 1 on the other still gives a 96 x 96 tile.  The rectangular backward alone caps the column tile,
//     Rc = min(96 / q2, 9984 / (2 Tr + Rr)),
// 9984 floats being what the two [Tr][Rc] row-pass buffers and the [Rr][Rc] pair values take at q1 x q2 = 6 x 1 (Tr 48, Rc 96).  The cap
// bites at q2 = 1 only, for q1 <= 4 (many pair values: Rc = 69 at q1 = 1) and for q1 >= 52 (Tr > 48: Rc = 51 at q1 = 96); at p1 == p2 it
// bites at p = 0 alone, where the wide backward (no cap) keeps Rc = 96.
//
// Forward (kernel_fwd_tiled_kernel): every T entry is ONE v_mfma_f32_16x16x4_f32 accumulator chain over the whole K loop, in k order, with
// kernel_fwd_kernel's operand sequence (no split-K over d): T is bit-identical to that kernel's, so the pack's k-ordered self terms keep
// r == 0 exact on the diagonal micro-blocks of K_ZZ.  The micro-block transform is kernel_fwd_kernel's with the two periods; it runs out
// of LDS and every output element is stored once, rows coalesced.  LDS, floats:
//     max((Trp + Tcp) 33, Trp 100) + Trp + Tcp + Rr Rc                                      <= 39552 bytes (q1 x q2 = 96 x 1)
// Backward, the tile and contraction launches (the points launch of assemble.hip follows and adds the slabs in the fixed order s = 0, 1, ...):
//   1. kernel_bwd_tbar_kernel, per tile: T over the K loop again, Tbar from the upstream tile with kernel_bwd_kernel's row / column passes
//      -- the row pass's inner loops run b = 1..p2, the column pass's a = 1..p1, nothing else in the algebra knows a period -- Tbar to a
//      global scratch TB[n1q, n2q] and the tile's <Gbar, K> / lengthscale partial sums to `partials` (one pair per workgroup).  LDS, floats:
//          max((Trp + Tcp) 33, Trp 100) + Trp 100 + Trp + Tcp + Rr Rc + 2 Tr Rc + 8
//      94304 bytes at 1 x 1 without the cap; with it <= 78944 bytes (6 x 1) for every q1 <= 48: two workgroups per CU; 117372 bytes at
//      87 x 1, the maximum over all q1, q2 <= 96 (one workgroup per CU: 76.8 KB of it are the T and Tbar tiles of 96 rows, which no
//      column cap shrinks);
//   2. kernel_bwd_wide_contract_kernel: slab[s] = TB[:, K_s] . [P2 | indicator][K_s, :NP], a plain MFMA product, 64 x 64 output tiles, the
//      n2q range cut into ns contiguous pieces K_s (one slab each).  It sees n2q packed rows, no period.
// No floating-point atomics anywhere: every sum has a fixed order, two identical calls are bitwise equal.
#include "common.h"
#include "tiled_assembly.h"

namespace {

// ---- the RBF family's radial algebra (tiled_assembly.h lists what a policy provides) ---------------------------
// k = s exp(-nn / 2) per point pair; the micro-block is k [[1, w_b / ell], [-u_a / ell, (t_ab - u_a w_b) / ell^2]] -- kernel_fwd_kernel's
// transform and kernel_bwd_kernel's row / column passes (assemble.hip) with a row period q1 and a column period q2
struct RbfRadial {
    static constexpr int NPAIR = 1, NSUM = 2;       // pair array: k; partial slots: sum(Tbar_00) = <Gbar, K>, the lengthscale sum
    static constexpr double F1_0 = 1.0;
    struct Hyp {
        float ell, s;
        __device__ __forceinline__ explicit Hyp(const float* __restrict__ hyp) : ell(hyp[0]), s(hyp[1]) {}
    };
    struct Row { float k; };
    float il, il2, s;
    __device__ __forceinline__ explicit RbfRadial(const Hyp& h) : il(1.f / h.ell), il2(il * il), s(h.s) {}

    __device__ __forceinline__ void pair(float* kk, int, float nn) const { kk[0] = s * expf(-0.5f * nn); }
    __device__ __forceinline__ float pair_value(const float* kk, int) const { return kk[0]; }
    __device__ __forceinline__ float entry(float k, const float*, int, int a, int b, float t, float u, float w) const {
        const float f0 = b ? (w * il) : 1.f;
        const float f1 = b ? ((t - u * w) * il2) : (-u * il);
        return (a ? f1 : f0) * k;
    }
    __device__ __forceinline__ float value(float nn) const { return s * expf(-0.5f * nn); }

    __device__ __forceinline__ Row row(float, float nn) const { return Row{s * expf(-0.5f * nn)}; }
    __device__ __forceinline__ void row_value(const Row& R, float g0, float first, float& ps, float& kk, float* acc) const {
        first *= il;
        ps = g0 + first;
        kk = R.k;
        acc[1] = __builtin_fmaf(R.k, first, acc[1]);
    }
    __device__ __forceinline__ float row_deriv(const Row& R, float* gr_, const float* tr_, const float* t0_, const float* s2_, int p2,
                                               float g0, float u, float* acc) const {
        const float k = R.k;
        float hs = 0.f, gw = 0.f;
        const float kil2 = k * il2;
        for (int b = 1; b <= p2; ++b) {
            const float w = t0_[b] - s2_[b];
            const float g = gr_[b];
            hs = __builtin_fmaf(g, tr_[b] - u * w, hs);
            gw = __builtin_fmaf(g, w, gw);
            gr_[b] = kil2 * g;                                  // Tbar_ab
        }
        hs *= il2;
        const float ubar = k * (-g0 * il - gw * il2);
        gr_[0] = -ubar;                                         // Tbar_a0
        acc[1] += k * (2.f * hs - g0 * u * il) + ubar * u;
        return hs - g0 * u * il;
    }
    __device__ __forceinline__ float col_value(float k, float kbar, float s1v, const float* s2c, const float* tc, float* acc) const {
        const float t00 = k * kbar;                             // Tbar_00
        const float nn = fmaxf(s1v + s2c[0] - 2.f * tc[0], 0.f);
        acc[0] += t00;
        acc[1] = __builtin_fmaf(-t00, nn, acc[1]);
        return t00;
    }
    __device__ __forceinline__ float col_deriv(float k, int p1, float, const float* s2c, const float* tc, int, const float* g0c,
                                               const float* us, int Rc, float* acc) const {
        const float w = tc[0] - s2c[0];
        float wbar = k * il * *g0c;
        for (int a = 1; a <= p1; ++a) wbar = __builtin_fmaf(-g0c[a * WLDT], us[a * Rc], wbar);
        acc[1] = __builtin_fmaf(wbar, w, acc[1]);
        return wbar;                                            // Tbar_0b
    }
    __device__ __forceinline__ void partials(const float* acc, float* ps) const { ps[0] = acc[0]; ps[1] = -il * acc[1]; }
};

// ---- backward, launch 2: slab[s][n1q][NP] = TB[:, K_s] . P2ext[K_s, :] -----------------------------------------
__global__ __launch_bounds__(WNT) void kernel_bwd_wide_contract_kernel(const float* __restrict__ TB, int n1q, int n2q,
                                                                       const float* __restrict__ P2, int DP, int NP, int kper,
                                                                       float* __restrict__ slab) {
    __shared__ float As[CM * (CK + 1)];         // [row][k]
    __shared__ float Bs[CK * (CN + 4)];         // [k][packed column]
    constexpr int LDA = CK + 1, LDB = CN + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * CM, n0 = blockIdx.x * CN;
    const int kb = blockIdx.z * kper, ke = min(n2q, kb + kper);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    f4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = kb; k0 < ke; k0 += CK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < CM * CK / WNT; ++i) {
            const int e = tid + i * WNT, r = e >> 5, c = e & 31;
            As[r * LDA + c] = (m0 + r < n1q && k0 + c < ke) ? TB[(int64_t)(m0 + r) * n2q + k0 + c] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < CK * CN / WNT; ++i) {
            const int e = tid + i * WNT, r = e >> 6, c = e & 63;
            Bs[r * LDB + c] = (k0 + r < ke && n0 + c < DP) ? P2[(int64_t)(k0 + r) * DP + n0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < CK; kk += 4) {
            const int ka = kk + (lane >> 4);
            const float a0 = As[(wm + (lane & 15)) * LDA + ka], a1 = As[(wm + 16 + (lane & 15)) * LDA + ka];
            const float b0 = Bs[ka * LDB + wn + (lane & 15)], b1 = Bs[ka * LDB + wn + 16 + (lane & 15)];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    float* out = slab + (int64_t)blockIdx.z * n1q * NP;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn + j * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm + i * 16 + (lane >> 4) * 4 + r;
                if (row < n1q && col < NP) out[(int64_t)row * NP + col] = acc[i][j][r];
            }
        }
}

// launch 2 of a backward on plan t
int launch_kernel_bwd_contract(hipStream_t st, const float* TB, const TilePlan& t, const float* P2, float* slab) {
    if (t.ns < 1 || t.ns > 65535) return DSVGP_EINVAL;
    hipLaunchKernelGGL(kernel_bwd_wide_contract_kernel, dim3(cdiv(t.NP, CN), cdiv(t.n1q, CM), t.ns), dim3(WNT), 0, st, TB, t.n1q, t.n2q, P2,
                       t.DP, t.NP, t.kper, slab);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int launch_kernel_bwd_tbar_rbf(hipStream_t st, const TilePlan& t, const void* G, int64_t ldg, int g_is_double, const float* P1,
                               const float* self1, const float* P2, const float* self2, const float* hyp, float* TB, float* partials) {
    return launch_tbar_tiles<RbfRadial>(st, t, G, ldg, g_is_double, P1, self1, P2, self2, hyp, TB, partials);
}

int launch_kernel_bwd_tiles(hipStream_t st, TbarLauncher tbar, const TilePlan& t, const void* G, int64_t ldg, int g_is_double,
                            const float* P1, const float* self1, const float* P2, const float* self2, const float* hyp, void* workspace,
                            float** slab, float** partials, float** TB) {
    if (t.gy > 65535 || t.ns > 65535) return DSVGP_EINVAL;
    *slab = (float*)workspace;
    *partials = *slab + t.slab_f;
    *TB = *partials + t.part_f;
    if (int rc = tbar(st, t, G, ldg, g_is_double, P1, self1, P2, self2, hyp, *TB, *partials)) return rc;
    return launch_kernel_bwd_contract(st, *TB, t, P2, *slab);
}

int kernel_diag_rbf(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* hyp, float* out) {
    return kernel_diag_family<RbfRadial>(ctx, P, n, p, d, hyp, out);
}
int kernel_diag_bwd_rbf(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* ell, const float* hyp, const float* out,
                        const float* gbar, float* d_ell, float* d_hyp) {
    return kernel_diag_bwd_family<RbfRadial>(ctx, P, n, p, d, ell, hyp, out, gbar, d_ell, d_hyp);
}

// ---- the wide entries' launchers (assemble.hip) ---------------------------------------------------------------
// (the workspace knows the packed width through NP alone, and NP rounded up to 16 is NP)
size_t kernel_bwd_wide_workspace(int n1q, int n2q, int q, int NP) { return tile_plan(n1q, q, n2q, q, NP, false).bytes; }

int launch_kernel_fwd_tiled(hipStream_t st, const float* P1, const float* self1, int n1q, int q1, const float* P2, const float* self2,
                            int n2q, int q2, int K4, int DP, const float* hyp, float jitter, void* out, int64_t ld, int out_is_double) {
    return launch_fwd_tiles<RbfRadial>(st, tile_plan(n1q, q1, n2q, q2, DP, false), P1, self1, P2, self2, hyp, jitter, out, ld,
                                       out_is_double);
}

int launch_kernel_bwd_wide(hipStream_t st, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1, int n1q,
                           const float* P2, const float* self2, int n2q, int q, int K4, int DP, int NP, const float* hyp, void* workspace,
                           float** slab, int* ns, float** partials, int* nparts) {
    const TilePlan t = tile_plan(n1q, q, n2q, q, DP, false);
    float* TB;
    *ns = t.ns; *nparts = t.nparts;
    return launch_kernel_bwd_tiles(st, launch_kernel_bwd_tbar_rbf, t, G, ldg, g_is_double, P1, self1, P2, self2, hyp, workspace, slab,
                                   partials, &TB);
}

// ---- the rectangular entries ----------------------------------------------------------------------------------
extern "C" size_t dsvgp_kernel_bwd_rect_workspace_bytes(int n1, int p1, int n2, int p2, int d) {
    TilePlan t;
    return rect_tile_plan(n1, p1, n2, p2, d, true, t) ? 0 : t.bytes;
}

extern "C" int dsvgp_kernel_bwd_rect(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1,
                                     const float* vnorm1, int n1, int p1, const float* P2, const float* self2, int n2, int p2, int d,
                                     const float* hyp, float* d_x1, float* d_v1, float* d_hyp, void* workspace) {
    if (!ctx || !G || !P1 || !self1 || !P2 || !self2 || !hyp || !d_x1 || !d_hyp || !workspace) return DSVGP_EINVAL;
    if (p1 > 0 && (!vnorm1 || !d_v1)) return DSVGP_EINVAL;
    if (d < 1 || p1 < 0 || p2 < 0 || p1 + 1 > WTMAX || p2 + 1 > WTMAX || n1 < 0 || n2 < 0) return DSVGP_EINVAL;
    if (n1 == 0 || n2 == 0) return 0;
    TilePlan t;
    if (int rc = rect_tile_plan(n1, p1, n2, p2, d, true, t)) return rc;
    if (ldg < t.n2q) return DSVGP_EINVAL;
    if (((uintptr_t)P1 | (uintptr_t)P2) % 16) return DSVGP_EINVAL;         // the packed rows are read 16 bytes at a time
    if ((uintptr_t)workspace % 4 || (uintptr_t)G % (g_is_double ? 8 : 4)) return DSVGP_EINVAL;
    float *slab, *partials, *TB;
    if (int rc = launch_kernel_bwd_tiles(ctx->stream, launch_kernel_bwd_tbar_rbf, t, G, ldg, g_is_double, P1, self1, P2, self2, hyp,
                                         workspace, &slab, &partials, &TB))
        return rc;
    // the points launch of every kernel backward with side 1's geometry (d, p1)
    return kernel_bwd_finish_points(ctx, d, p1, slab, t.ns, P1, vnorm1, n1, hyp, 1.f, d_x1, d_v1, partials, t.nparts, d_hyp);
}

extern "C" int dsvgp_kernel_fwd_rect(dsvgp_ctx* ctx, const float* P1, const float* self1, int n1, int p1, const float* P2,
                                     const float* self2, int n2, int p2, int d, const float* hyp, float* out, int64_t ld) {
    if (!ctx || !P1 || !self1 || !P2 || !self2 || !hyp || !out) return DSVGP_EINVAL;
    TilePlan t;
    if (int rc = rect_tile_plan(n1, p1, n2, p2, d, false, t)) return rc;
    if (ld < t.n2q) return DSVGP_EINVAL;
    if (((uintptr_t)P1 | (uintptr_t)P2) % 16) return DSVGP_EINVAL;         // the packed rows are read 16 bytes at a time
    return launch_fwd_tiles<RbfRadial>(ctx->stream, t, P1, self1, P2, self2, hyp, 0.f, out, ld, 0);
}
