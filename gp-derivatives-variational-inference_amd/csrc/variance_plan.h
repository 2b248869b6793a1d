// Host-side plan of the posterior-variance kernels (csrc/predict_variance.hip): the constants, the route and chunk rule of the fused
// kernel, the layout of the packed weights and of the workspace, shared by the kernels, their launchers and tools/variance_check.cpp
// (plain C++, no HIP).
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int VP_FUSED_MAX_D = 32;       // the fused kernel's bound on d
constexpr int VP_TP = 64;                // test points per workgroup of the fused kernel (one per lane)
constexpr int VP_NW = 8;                 // waves per workgroup = slices of every chunk of inducing points
constexpr int VP_CH_MAX = 64;            // inducing points per LDS chunk, at most
constexpr int VP_MAX_P = 95;             // directions per inducing point (the bound of dsvgp_pack_points)
constexpr int VP_LDS_FLOATS = 12288;     // LDS floats of one staged chunk (48 KB): z~ and the p unit directions of every point in it
constexpr int VP_RS = 256;               // composed route: rows of K_ZX / V per row slice of the column reduction
constexpr int VP_TILE = 64;              // composed route: edge of the LDS tile that transposes V into G
constexpr long long VP_IDX_MAX = 0x7fffffffLL;   // intermediates are indexed with 32 bits

inline int vp_pad4(int v) { return (v + 3) & ~3; }
inline int vp_packed_width(int d) { return vp_pad4(d) + 4; }      // dsvgp_packed_width

// inducing points per LDS chunk of the fused kernel: as many as fit VP_LDS_FLOATS with their (p + 1) rows of D = pad4(d) floats, at most
// VP_CH_MAX, rounded down to a multiple of the VP_NW waves that slice a chunk; 0 = no chunk fits (or d > VP_FUSED_MAX_D): composed route
inline int vp_chunk(int d, int p) {
    if (d < 1 || d > VP_FUSED_MAX_D || p < 0 || p > VP_MAX_P) return 0;
    int c = VP_LDS_FLOATS / ((p + 1) * vp_pad4(d));
    c = c < VP_CH_MAX ? c : VP_CH_MAX;
    return c & ~(VP_NW - 1);
}
// 1 = fused, 2 = composed, 0 = refused arguments
inline int vp_route(int d, int p) {
    if (d < 1 || p < 0 || p > VP_MAX_P) return 0;
    return vp_chunk(d, p) > 0 ? 1 : 2;
}
// dynamic LDS bytes of the fused kernel: the staged chunk
inline size_t vp_fused_lds(int d, int p) { return (size_t)vp_chunk(d, p) * (p + 1) * vp_pad4(d) * sizeof(float); }

// packed weights (floats): hdr[8] = {ell, s, 1/ell, s/ell, 0, 0, 0, 0} | center[ldw] | Z~[M][ldw] | U[M p][ldw] (unit directions);
// ldw = pad4(d), padding columns are zero
struct VpWeights { int ldw; size_t o_center, o_z, o_u, total; };
inline bool vp_weights(int M, int d, int p, VpWeights* w) {
    if (M < 1 || d < 1 || p < 0 || p > VP_MAX_P) return false;
    w->ldw = vp_pad4(d);
    if ((long long)M * (p + 1) * w->ldw > VP_IDX_MAX) return false;
    w->o_center = 8;
    w->o_z = w->o_center + w->ldw;
    w->o_u = w->o_z + (size_t)M * w->ldw;
    w->total = w->o_u + (size_t)M * p * w->ldw;
    return true;
}

// workspace (floats; every region starts at a multiple of 4 floats = 16 bytes):
//   PX[B][DP] | selfX[pad4(B)] | K_ZX[M'][ldk] | V[M'][ldk]                                  both routes (ldk = pad4(B), DP = packed width)
//   part[ns][ldk]                                                                            composed: row-slice partial sums
//   G[B][ldg] | dhyp[4] | the workspace of dsvgp_kernel_bwd_rect (bwd_bytes)                 composed with the gradient (ldg = pad4(M'))
// `bwd_bytes`: dsvgp_kernel_bwd_rect_workspace_bytes(B, 0, M, p, d) (0 = that entry refuses the shape)
struct VpWork { int route, Mp, DP, ldk, ldg, ns; size_t o_px, o_sx, o_k, o_v, o_part, o_g, o_dh, o_bwd, total; };
inline bool vp_work(int M, int d, int p, int B, bool want_grad, size_t bwd_bytes, VpWork* s) {
    s->route = vp_route(d, p);
    if (!s->route || M < 1 || B < 1) return false;
    const long long Mp = (long long)M * (p + 1);
    s->DP = vp_packed_width(d);
    s->ldk = vp_pad4(B);
    if (Mp > VP_IDX_MAX || Mp * s->ldk > VP_IDX_MAX || (long long)B * s->DP > VP_IDX_MAX) return false;
    s->Mp = (int)Mp;
    s->ldg = vp_pad4(s->Mp);
    s->ns = (s->Mp + VP_RS - 1) / VP_RS;
    s->o_px = 0;
    s->o_sx = s->o_px + (size_t)B * s->DP;
    s->o_k = s->o_sx + (size_t)s->ldk;
    s->o_v = s->o_k + (size_t)s->Mp * s->ldk;
    s->o_part = s->o_v + (size_t)s->Mp * s->ldk;
    s->o_g = s->o_dh = s->o_bwd = s->total = s->o_part;
    if (s->route == 1) return true;
    s->o_g = s->o_part + (size_t)s->ns * s->ldk;
    s->o_dh = s->o_bwd = s->total = s->o_g;
    if (!want_grad) return true;
    if ((long long)B * s->ldg > VP_IDX_MAX || bwd_bytes == 0) return false;
    s->o_dh = s->o_g + (size_t)B * s->ldg;
    s->o_bwd = s->o_dh + 4;
    s->total = s->o_bwd + (bwd_bytes + 15) / 16 * 4;
    return true;
}

// dsvgp_acq_descend (floats): y[B][d4] .. the trial point, its gradient and value, then mu, grad mu, sigma^2, grad sigma^2 of the point set
// under evaluation, then the workspaces of dsvgp_mean_predict (mean_bytes) and dsvgp_var_predict (var_bytes); Bd = pad4(B d), Br = pad4(B)
struct VpDescend { size_t o_y, o_gy, o_fy, o_mu, o_gmu, o_var, o_gvar, o_mean, o_varws, total; };
inline bool vp_descend(int d, int B, size_t mean_bytes, size_t var_bytes, VpDescend* s) {
    if (d < 1 || B < 1 || (long long)B * d > VP_IDX_MAX || var_bytes == 0) return false;
    const size_t Bd = ((size_t)B * d + 3) & ~(size_t)3, Br = (size_t)vp_pad4(B);
    s->o_y = 0;
    s->o_gy = s->o_y + Bd;
    s->o_fy = s->o_gy + Bd;
    s->o_mu = s->o_fy + Br;
    s->o_gmu = s->o_mu + Br;
    s->o_var = s->o_gmu + Bd;
    s->o_gvar = s->o_var + Br;
    s->o_mean = s->o_gvar + Bd;
    s->o_varws = s->o_mean + (mean_bytes + 15) / 16 * 4;
    s->total = s->o_varws + (var_bytes + 15) / 16 * 4;
    return true;
}

// acquisition kinds of dsvgp_acq_eval
enum { VP_ACQ_LCB_VAR = 0, VP_ACQ_LCB = 1, VP_ACQ_EI = 2 };
constexpr float VP_MIN_VAR = 1e-6f;      // floor of sigma^2 under the square root (gpytorch settings.min_variance)
constexpr float VP_KXX_JITTER = 1e-4f;   // the 1e-4 on the predictive diagonal (DGVS.py:202-205)
