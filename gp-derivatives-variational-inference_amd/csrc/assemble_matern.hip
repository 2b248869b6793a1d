// Matern-5/2 assembly with directional derivatives, gfx950: the second kernel family on the tiled assembly of tiled_assembly.h -- this file
// holds the family's radial algebra (Matern52Radial) and its entries; the kernels, the plan and the launchers are the shared ones.
//
// Formulation.  Matern always runs on the ARD packs of assemble_ard.hip (x~ = (x - c) ./ ell, v~_a = (v_a / |v_a|) ./ ell, hyp[0] = 1), so
// the lengthscales never appear here.  With T = P1 P2^T (wide_T) and the packs' self terms, for the point pair (i, j)
//     nn = max(self1[i0] + self2[j0] - 2 T[i0,j0], 0)     u_a = self1[ia] - T[ia,j0]     w_b = T[i0,jb] - self2[jb]     t_ab = T[ia,jb]
//     a = sqrt(5 nn), e = exp(-a):    f0 = (1 + a + a^2/3) e    f1 = (5/3)(1 + a) e    f2 = (25/3) e    f3 = (125/3) e / a
// (f_{m+1} = -2 d f_m / d nn; the RBF kernel is f0 = f1 = f2 = exp(-nn/2)) the micro-block is
//     s [[ f0, f1 w_b ], [ -f1 u_a, f1 t_ab - f2 u_a w_b ]]
// and its backward, given G on the block, in the TB conventions of kernel_bwd_tbar_kernel (tiled_assembly.h; every launch after the Tbar tiles -- the
// contraction, the ARD points / column-sum / self-rows / reduce kernels -- sees the kernel through Tbar alone and is shared):
//     Tbar_ab = s f1 G_ab
//     Tbar_a0 = -ubar_a    ubar_a = s (-f1 G_a0 - f2 sum_b G_ab w_b)
//     Tbar_0b =  wbar_b    wbar_b = s ( f1 G_0b - f2 sum_a G_ab u_a)
//     Tbar_00 = -2 nnbar   nnbar  = -s/2 [G_00 f1 + f2 sum_b G_0b w_b - f2 sum_a G_a0 u_a + sum_ab G_ab (f2 t_ab - f3 u_a w_b)]
// f3 only ever multiplies u_a w_b, which is exactly 0 where nn is (the k-ordered self terms: K_ZZ's diagonal micro-blocks, exact duplicate
// points), and |u_a w_b| <= nn |v~_a| |v~_b|.  The division is guarded at the rounding noise of nn itself,
//     f3 = (125/3) e rsqrt(5 max(nn, 2^-23 (self1[i0] + self2[j0]), 1e-36)),
// so the product is 0 at nn = 0 (never 0 inf) and stays of the order sqrt(noise) where cancellation has left nothing of nn; any pair whose
// nn stands above its rounding noise gets the plain quotient.  sum(G o K), which feeds d_hyp[1], is accumulated directly: the block entries
// are not proportional to one pair value, so the RBF kernel's shortcut (sum of Tbar_00) does not hold.
//
// Tiles, grid, K loop, output walk, the task loops of the row / column pass, TB store and the fixed-order workgroup reduction are
// kernel_fwd_tiled_kernel<Matern52Radial, .> / kernel_bwd_tbar_kernel<Matern52Radial, .> themselves: the same text as the RBF
// instances (profiles/tiled_family_resource_usage.txt).  LDS:
//   forward   three pair values (s f0, s f1, s f2) per point pair: the RBF forward's bytes + 8 Rr Rc (nothing more at 1 x 1 micro-blocks, which
//             touch no pair array): at most 47424 bytes, at q1 x q2 = 2 x 1, over all q1, q2 <= 96 (dsvgp_kernel_fwd_matern52_lds_bytes)
//   Tbar      the RBF Tbar launch's bytes unchanged (<= 117372): KK holds e per pair (written by the row pass); the column pass rebuilds
//             a = sqrt(5 nn) from the tile -- one sqrt per task -- and f1 = (5/3)(1 + a) e, f2 / f1 = 5 / (1 + a) (no second exp, and no
//             division by an e that has underflowed)
// No floating-point atomics: every sum has a fixed order, two identical calls are bitwise equal.
#include "common.h"
#include "tiled_assembly.h"

namespace {

constexpr float C53 = 5.f / 3.f, C253 = 25.f / 3.f, C1253 = 125.f / 3.f;
constexpr float NN_EPS = 1.1920929e-7f;        // 2^-23: the rounding noise of nn relative to the two self terms it is the difference of

// ---- the Matern-5/2 family's radial algebra (tiled_assembly.h lists what a policy provides) --------------------
struct Matern52Radial {
    static constexpr int NPAIR = 3, NSUM = 1;       // pair arrays: s f0, s f1, s f2; partial slot 0: sum(G o K) (slot 1, the scalar-
                                                    // lengthscale sum of the RBF launch, holds 0: nothing reads it on ARD packs)
    static constexpr double F1_0 = 5.0 / 3.0;
    struct Hyp {
        float s;
        __device__ __forceinline__ explicit Hyp(const float* __restrict__ hyp) : s(hyp[1]) {}      // (hyp[0] = 1 is not read)
    };
    struct Row { float ssum, nn, ra, e, f1, f2; };
    float s;
    __device__ __forceinline__ explicit Matern52Radial(const Hyp& h) : s(h.s) {}

    __device__ __forceinline__ void pair(float* kk, int np, float nn) const {
        const float a = sqrtf(5.f * nn);
        const float se = s * expf(-a);
        kk[0] = (1.f + a + C53 * nn) * se;
        kk[np] = C53 * (1.f + a) * se;
        kk[2 * np] = C253 * se;
    }
    __device__ __forceinline__ float pair_value(const float* kk, int np) const { return kk[np]; }
    __device__ __forceinline__ float entry(float k1, const float* kk, int np, int a, int b, float t, float u, float w) const {
        const float v0 = b ? (k1 * w) : kk[0];
        const float v1 = b ? (k1 * t - kk[2 * np] * (u * w)) : (-k1 * u);      // (u w first: K_ZZ comes out exactly symmetric)
        return a ? v1 : v0;
    }
    __device__ __forceinline__ float value(float nn) const {
        const float a = sqrtf(5.f * nn);
        return (1.f + a + C53 * nn) * (s * expf(-a));
    }

    __device__ __forceinline__ Row row(float ssum, float nn) const {
        const float ra = sqrtf(5.f * nn);
        const float e = expf(-ra);
        return Row{ssum, nn, ra, e, C53 * (1.f + ra) * e, C253 * e};
    }
    __device__ __forceinline__ void row_value(const Row& R, float g0, float first, float& ps, float& kk, float* acc) const {
        ps = __builtin_fmaf(R.f2, first, g0 * R.f1);
        kk = R.e;                                               // the column pass rebuilds a and f1 from e
        acc[0] += __builtin_fmaf(g0, (1.f + R.ra + C53 * R.nn) * R.e, R.f1 * first);
    }
    __device__ __forceinline__ float row_deriv(const Row& R, float* gr_, const float* tr_, const float* t0_, const float* s2_, int p2,
                                               float g0, float u, float* acc) const {
        const float f1 = R.f1, f2 = R.f2;
        const float f3 = C1253 * R.e * rsqrtf(5.f * fmaxf(fmaxf(R.nn, NN_EPS * R.ssum), 1e-36f));
        float gt = 0.f, gw = 0.f;
        const float sf1 = s * f1;
        for (int b = 1; b <= p2; ++b) {
            const float w = t0_[b] - s2_[b];
            const float g = gr_[b];
            gt = __builtin_fmaf(g, tr_[b], gt);
            gw = __builtin_fmaf(g, w, gw);
            gr_[b] = sf1 * g;                                   // Tbar_ab
        }
        gr_[0] = __builtin_fmaf(s * f2, gw, sf1 * g0);          // Tbar_a0 = -ubar_a
        acc[0] += f1 * (gt - u * g0) - f2 * u * gw;
        return f2 * (gt - g0 * u) - f3 * u * gw;
    }
    __device__ __forceinline__ float col_value(float, float kbar, float, const float*, const float*, float*) const {
        return s * kbar;                                        // Tbar_00 = -2 nnbar
    }
    __device__ __forceinline__ float col_deriv(float e, int p1, float s1v, const float* s2c, const float* tc, int b, const float* g0c,
                                               const float* us, int Rc, float*) const {
        const float nn = fmaxf(s1v + s2c[-b] - 2.f * tc[-b], 0.f);
        const float ra1 = 1.f + sqrtf(5.f * nn);
        float acc = 0.f;
        for (int a = 1; a <= p1; ++a) acc = __builtin_fmaf(g0c[a * WLDT], us[a * Rc], acc);
        // wbar_b = s f1 G_0b - (f2 / f1) sum_a Tbar_ab u_a,   f2 / f1 = 5 / (1 + a)
        return s * (C53 * ra1 * e) * *g0c - (5.f / ra1) * acc;  // Tbar_0b
    }
    __device__ __forceinline__ void partials(const float* acc, float* ps) const { ps[0] = s * acc[0]; }
};

int launch_tbar_matern52(hipStream_t st, const TilePlan& t, const void* G, int64_t ldg, int g_is_double, const float* P1,
                         const float* self1, const float* P2, const float* self2, const float* hyp, float* TB, float* partials) {
    return launch_tbar_tiles<Matern52Radial>(st, t, G, ldg, g_is_double, P1, self1, P2, self2, hyp, TB, partials);
}

}  // namespace

// the forward's dynamic LDS for direction counts p1, p2 (host arithmetic; 0: refused) -- the maximum over all counts is in the header comment
extern "C" size_t dsvgp_kernel_fwd_matern52_lds_bytes(int p1, int p2) {
    TilePlan t;
    return rect_tile_plan(1, p1, 1, p2, 1, false, t) ? 0 : fwd_tiles_lds<Matern52Radial>(t);
}

extern "C" int dsvgp_kernel_fwd_matern52(dsvgp_ctx* ctx, const float* P1, const float* self1, int n1, int p1, const float* P2,
                                         const float* self2, int n2, int p2, int d, const float* hyp, float jitter, void* out, int64_t ld,
                                         int out_is_double) {
    if (!ctx || !P1 || !self1 || !P2 || !self2 || !hyp || !out) return DSVGP_EINVAL;
    TilePlan t;
    if (int rc = rect_tile_plan(n1, p1, n2, p2, d, false, t)) return rc;
    if (ld < t.n2q) return DSVGP_EINVAL;
    if (((uintptr_t)P1 | (uintptr_t)P2) % 16) return DSVGP_EINVAL;         // the packed rows are read 16 bytes at a time
    if ((uintptr_t)out % (out_is_double ? 8 : 4)) return DSVGP_EINVAL;
    return launch_fwd_tiles<Matern52Radial>(ctx->stream, t, P1, self1, P2, self2, hyp, jitter, out, ld, out_is_double);
}

extern "C" size_t dsvgp_kernel_bwd_matern52_workspace_bytes(int n1, int p1, int n2, int p2, int d) {
    // the same launches after the Tbar tiles and the same layout as the ARD backward's, rounded up to a multiple of 16 bytes
    return (dsvgp_kernel_bwd_ard_workspace_bytes(n1, p1, n2, p2, d) + 15) & ~(size_t)15;
}

extern "C" int dsvgp_kernel_bwd_matern52(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1,
                                         const float* vnorm1, int n1, int p1, const float* P2, const float* self2, int n2, int p2, int d,
                                         const float* ell, const float* hyp, int symmetric, float* d_x1, float* d_v1, float* d_ell,
                                         float* d_hyp, void* workspace) {
    return kernel_bwd_ard_family(ctx, launch_tbar_matern52, G, ldg, g_is_double, P1, self1, vnorm1, n1, p1, P2, self2, n2, p2, d, ell, hyp,
                                 symmetric, d_x1, d_v1, d_ell, d_hyp, workspace);
}

// prior diagonal: out[i q] = s, out[i q + a] = (5/3) s |v~_ia|^2 -- f1(0) = 5/3
extern "C" int dsvgp_kernel_diag_matern52(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* hyp, float* out) {
    return kernel_diag_family<Matern52Radial>(ctx, P, n, p, d, hyp, out);
}

extern "C" int dsvgp_kernel_diag_matern52_bwd(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* ell, const float* hyp,
                                              const float* out, const float* gbar, float* d_ell, float* d_hyp) {
    return kernel_diag_bwd_family<Matern52Radial>(ctx, P, n, p, d, ell, hyp, out, gbar, d_ell, d_hyp);
}
