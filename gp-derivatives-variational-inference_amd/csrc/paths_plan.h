// Index arithmetic of the pathwise posterior sampler (paths.hip): the layout of the packed weights, the chunking / ownership / LDS
// offsets of the fused kernel (d <= 32) and the workspace layout and sample grouping of the GEMM-composed route (any other d).  Plain
// integer arithmetic, shared between the kernels, their launcher and the host check tools/paths_check.cpp (which emulates every thread of
// the fused kernel serially and shows that every (sample, point, i) and (sample, point, j) is visited exactly once and that every LDS
// and global offset stays in bounds).
//
// Fused kernel: a workgroup of PP_NW waves owns PP_TP = 64 test points (lane = point) and a GROUP of NS = paths_ns(D) samples
// (grid = [point tiles, sample groups]).  The M inducing points and then the F features go through LDS in chunks of PP_CH = 64; wave w
// owns the entries w, w + PP_NW, ... of every chunk.  One LDS array serves three images in turn:
//   inducing chunk   Z~[CH][D] | G'[NS][CH][D] | a[NS][CH]
//   feature chunk    Om[CH][D] | phase[CH] | wq[NS][CH]
//   reduction        red[NS][TP][D + 1]  (row stride D + 1 is odd: lane-strided accesses fall on distinct banks)
// the first is the largest.  Every rule below depends on the shapes alone, never on B, n or the card: the order of every sum of a
// (sample, point) is fixed by M, F and d.
#pragma once
#include <stddef.h>

constexpr int PP_FUSED_MAX_D = 32;  // the fused kernel's bound on d
constexpr int PP_TP = 64;           // test points per workgroup (one per lane)
constexpr int PP_NW = 8;            // waves per workgroup = slices of every chunk
constexpr int PP_CH = 64;           // inducing points / features per LDS chunk
constexpr int PP_NS_MAX = 8;        // samples per group at most
constexpr int PP_MAX_P = 95;        // directions per inducing point (the bound of dsvgp_pack_points)

constexpr int paths_pad4(int v) { return (v + 3) & ~3; }
constexpr size_t paths_pad4z(size_t v) { return (v + 3) & ~(size_t)3; }

// samples per group of the fused kernel at row length D = pad4(d): NS (D + 1) accumulators next to x~[D], r[D] and ~50 registers of
// addresses and temporaries inside the 256 a wave has at two waves per SIMD
constexpr int paths_ns(int D) {
    int ns = (176 - 2 * D) / (D + 1);
    ns = ns < PP_NS_MAX ? ns : PP_NS_MAX;
    return ns > 1 ? ns : 1;
}

// LDS float offsets of the three images (template parameter D)
struct PathsLds { int o_z, o_g, o_a, o_om, o_ph, o_w, o_red, floats; };
constexpr PathsLds paths_lds_ns(int D, int NS) {
    PathsLds l{};
    l.o_z = 0; l.o_g = PP_CH * D; l.o_a = l.o_g + NS * PP_CH * D;
    l.o_om = 0; l.o_ph = PP_CH * D; l.o_w = l.o_ph + PP_CH;
    l.o_red = 0;
    l.floats = l.o_a + NS * PP_CH;                        // >= PP_CH (D + 1 + NS) and >= NS PP_TP (D + 1)
    return l;
}
constexpr PathsLds paths_lds(int D) { return paths_lds_ns(D, paths_ns(D)); }

// Hessian-vector products (paths_hvp_fused_kernel<D>): the lane also holds v[D], so the group is narrower at the large D.  The rule
// is the one above with 3 D registers of x~, r, v; where the compiler's own temporaries (a row of G' or Om held across the inner
// loops) still pushed an instance past 256 registers the width is one less: the table is the widest at which no instance spills.
// The three LDS images are those above at this NS.
constexpr int paths_hvp_ns(int D) {
    int ns = (176 - 3 * D) / (D + 1);
    if (D == 24 || D == 32) ns -= 1;
    ns = ns < PP_NS_MAX ? ns : PP_NS_MAX;
    return ns > 1 ? ns : 1;
}
constexpr PathsLds paths_hvp_lds(int D) { return paths_lds_ns(D, paths_hvp_ns(D)); }

// packed weights (floats): hdr[8] = {ell, s, c, 1/ell, s/ell, 0, 0, 0} | center[ldw] | nz[Mr] = |z~|^2 | Z~[M][ldw] |
// Om[F][ldw] = omega / 2 pi | phase[Fr] (revolutions, in [0, 1]) | a[n][Mr] | a'[n][Mr] = a - z~.G' | wq[n][Fr] = sqrt(2 / (s F)) w |
// G'[n][M][ldw] = g / ell;   ldw = pad4(d), Mr = pad4(M), Fr = pad4(F); padding columns are zero
struct PathsWeights { int ldw, Mr, Fr; size_t o_center, o_nz, o_z, o_om, o_ph, o_a, o_ap, o_wq, o_g, total; };
inline PathsWeights paths_weights(int M, int d, int F, int n) {
    PathsWeights w{};
    w.ldw = paths_pad4(d); w.Mr = paths_pad4(M); w.Fr = paths_pad4(F);
    w.o_center = 8;
    w.o_nz = w.o_center + w.ldw;
    w.o_z = w.o_nz + w.Mr;
    w.o_om = w.o_z + (size_t)M * w.ldw;
    w.o_ph = w.o_om + (size_t)F * w.ldw;
    w.o_a = w.o_ph + w.Fr;
    w.o_ap = w.o_a + (size_t)n * w.Mr;
    w.o_wq = w.o_ap + (size_t)n * w.Mr;
    w.o_g = w.o_wq + (size_t)n * w.Fr;
    w.total = w.o_g + (size_t)n * M * w.ldw;
    return w;
}

// composed route: workspace (floats) of one call on B rows; samples go through in groups of ng.
//   shared   X~[B][ldw] | xn[Br] | K[B][ldM] | C[B][ldF] | VP[B][ldn]                       (+ S[B][ldF] with gradients)
//   group    S2[B][ld2] (ld2 = pad4(ng M)) | P[ng][B][ldM] | sigma[ng][Br]
//            (+ O1[ng][B][ldw] | O2[ng][B][ldw] | WO[F][ng ldw] | GP[B][ng ldw] with gradients)
struct PathsWork {
    int ldw, ldM, ldF, ldn, ld2, ng;
    size_t Br, o_x, o_xn, o_k, o_c, o_vp, o_s, o_s2, o_p, o_sig, o_o1, o_o2, o_wo, o_gp, total;
};
constexpr size_t PP_GROUP_FLOATS = (size_t)1 << 27;      // the group part stays under 512 MiB unless one sample alone needs more
constexpr long long PP_IDX_MAX = 0x7fffffffLL;           // intermediates are indexed with 32 bits

// 0, or -1 for a shape the composed route refuses (an intermediate would pass 2^31 entries: split the batch)
inline int paths_work(int M, int d, int F, int n, int B, int want_grad, PathsWork& s) {
    if (M < 1 || d < 1 || F < 1 || n < 1 || B < 1) return -1;
    s = PathsWork{};
    s.ldw = paths_pad4(d); s.ldM = paths_pad4(M); s.ldF = paths_pad4(F); s.ldn = paths_pad4(n);
    s.Br = paths_pad4z((size_t)B);
    const size_t per = (size_t)B * M + (size_t)B * s.ldM + s.Br +
                       (want_grad ? (size_t)3 * B * s.ldw + (size_t)F * s.ldw : 0);
    size_t ng = PP_GROUP_FLOATS / per;
    ng = ng < (size_t)n ? ng : (size_t)n;
    ng = ng < 65535 ? ng : 65535;                         // (a grid dimension)
    s.ng = ng > 1 ? (int)ng : 1;
    s.ld2 = paths_pad4(s.ng * M);
    const long long big[] = {(long long)B * s.ld2, (long long)s.ng * B * s.ldM, (long long)B * s.ldF, (long long)s.ng * B * s.ldw,
                             (long long)F * s.ng * s.ldw, (long long)B * s.ldn, (long long)B * d};
    for (long long v : big)
        if (v > PP_IDX_MAX) return -1;
    size_t o = 0;
    s.o_x = o;   o += (size_t)B * s.ldw;
    s.o_xn = o;  o += s.Br;
    s.o_k = o;   o += (size_t)B * s.ldM;
    s.o_c = o;   o += (size_t)B * s.ldF;
    s.o_vp = o;  o += (size_t)B * s.ldn;
    s.o_s = o;   o += want_grad ? (size_t)B * s.ldF : 0;
    s.o_s2 = o;  o += (size_t)B * s.ld2;
    s.o_p = o;   o += (size_t)s.ng * B * s.ldM;
    s.o_sig = o; o += (size_t)s.ng * s.Br;
    s.o_o1 = o;  o += want_grad ? (size_t)s.ng * B * s.ldw : 0;
    s.o_o2 = o;  o += want_grad ? (size_t)s.ng * B * s.ldw : 0;
    s.o_wo = o;  o += want_grad ? (size_t)F * s.ng * s.ldw : 0;
    s.o_gp = o;  o += want_grad ? (size_t)B * s.ng * s.ldw : 0;
    s.total = o;
    return 0;
}

// composed route of the Hessian-vector product: workspace (floats) of one call on B rows; samples go through in groups of ng.
//   shared   X~[B][ldw] | V[B][ldw] | xn[Br] | xv[Br] = x~.v | K[B][ldM] | RV[B][ldM] = V Z~^T - xv | C2[B][ldM] = k o RV |
//            T[B][ldF] = -4 pi^2 cos o OV | OV[B][ldF] = V Om^T
//   group    S2[B][ld2] | GV[B][ld2] (ld2 = pad4(ng M)) | C1[ng][B][ldM] | sigma[ng][Br] | sigma1[ng][Br] |
//            O1[ng][B][ldw] | O2[ng][B][ldw] | WO[F][ng ldw] | GP[B][ng ldw]
struct PathsHvpWork {
    int ldw, ldM, ldF, ld2, ng;
    size_t Br, o_x, o_v, o_xn, o_xv, o_k, o_rv, o_c2, o_t, o_ov, o_s2, o_gv, o_c1, o_sig, o_sig1, o_o1, o_o2, o_wo, o_gp, total;
};

// 0, or -1 for a shape the composed route refuses (an intermediate would pass 2^31 entries: split the batch)
inline int paths_hvp_work(int M, int d, int F, int n, int B, PathsHvpWork& s) {
    if (M < 1 || d < 1 || F < 1 || n < 1 || B < 1) return -1;
    s = PathsHvpWork{};
    s.ldw = paths_pad4(d); s.ldM = paths_pad4(M); s.ldF = paths_pad4(F);
    s.Br = paths_pad4z((size_t)B);
    const size_t per = (size_t)2 * B * M + (size_t)B * s.ldM + 2 * s.Br + (size_t)3 * B * s.ldw + (size_t)F * s.ldw;
    size_t ng = PP_GROUP_FLOATS / per;
    ng = ng < (size_t)n ? ng : (size_t)n;
    ng = ng < 65535 ? ng : 65535;                         // (a grid dimension)
    s.ng = ng > 1 ? (int)ng : 1;
    s.ld2 = paths_pad4(s.ng * M);
    const long long big[] = {(long long)B * s.ld2, (long long)s.ng * B * s.ldM, (long long)B * s.ldF, (long long)s.ng * B * s.ldw,
                             (long long)F * s.ng * s.ldw, (long long)B * d};
    for (long long v : big)
        if (v > PP_IDX_MAX) return -1;
    size_t o = 0;
    s.o_x = o;    o += (size_t)B * s.ldw;
    s.o_v = o;    o += (size_t)B * s.ldw;
    s.o_xn = o;   o += s.Br;
    s.o_xv = o;   o += s.Br;
    s.o_k = o;    o += (size_t)B * s.ldM;
    s.o_rv = o;   o += (size_t)B * s.ldM;
    s.o_c2 = o;   o += (size_t)B * s.ldM;
    s.o_t = o;    o += (size_t)B * s.ldF;
    s.o_ov = o;   o += (size_t)B * s.ldF;
    s.o_s2 = o;   o += (size_t)B * s.ld2;
    s.o_gv = o;   o += (size_t)B * s.ld2;
    s.o_c1 = o;   o += (size_t)s.ng * B * s.ldM;
    s.o_sig = o;  o += (size_t)s.ng * s.Br;
    s.o_sig1 = o; o += (size_t)s.ng * s.Br;
    s.o_o1 = o;   o += (size_t)s.ng * B * s.ldw;
    s.o_o2 = o;   o += (size_t)s.ng * B * s.ldw;
    s.o_wo = o;   o += (size_t)F * s.ng * s.ldw;
    s.o_gp = o;   o += (size_t)B * s.ng * s.ldw;
    s.total = o;
    return 0;
}

// ---- own-point evaluation (paths_own_fused_kernel<D, WANT_GRAD>, dsvgp_paths_eval_own): sample s at its OWN points x[s][B][d] ------
// Fused kernel (d <= 32): a workgroup of PP_NW waves owns PP_TP = 64 points of ONE sample (grid = [point tiles, samples], lane = point);
// there is no sample group, so the lane holds x~[D], r[D], acc[D] and sig only.  The chunking and the ownership are those above (wave w
// owns the entries w, w + PP_NW, ... of every chunk of PP_CH); the three LDS images are the ones above at NS = 1:
//   inducing chunk   Z~[CH][D] | G'_s[CH][D] | a_s[CH]
//   feature chunk    Om[CH][D] | phase[CH] | wq_s[CH]
//   reduction        red[TP][D + 1]
constexpr PathsLds paths_own_lds(int D) { return paths_lds_ns(D, 1); }
constexpr int paths_own_first(int wave) { return wave; }                 // first entry of a chunk a wave owns; the stride is PP_NW
constexpr int paths_own_red(int point, int k, int D) { return point * (D + 1) + k; }      // k = D: the value
// global float offsets of (sample, point tile): the first point of the tile in x / grads ([n][B][d]) and in values ([n][B])
constexpr size_t paths_own_row(int s, long long B, long long b0) { return (size_t)s * (size_t)B + (size_t)b0; }

// Composed route (any other d): all N = n B (sample, point) pairs are rows of ONE stacked problem; the per-sample operands G'_s enter
// through one product per sample on the sample's row block.  Workspace (floats):
//   X~[N][ldw] | xn[Nr] | K[N][ldM] | T[N][ldF] (Theta, then wq_s o S in place) | vp[Nr] | P[N][ldM] (S2, then P in place) | sigma[Nr]
//   (+ O1[N][ldw] | O2[N][ldw] | GP[N][ldw] with gradients)
struct PathsOwnWork {
    int ldw, ldM, ldF;
    long long N;
    size_t Nr, o_x, o_xn, o_k, o_t, o_vp, o_p, o_sig, o_o1, o_o2, o_gp, total;
};

// 0, or -1 for a shape the composed route refuses (an intermediate would pass 2^31 entries: split the points)
inline int paths_own_work(int M, int d, int F, int n, int B, int want_grad, PathsOwnWork& s) {
    if (M < 1 || d < 1 || F < 1 || n < 1 || B < 1) return -1;
    s = PathsOwnWork{};
    s.ldw = paths_pad4(d); s.ldM = paths_pad4(M); s.ldF = paths_pad4(F);
    s.N = (long long)n * B;
    if (s.N > PP_IDX_MAX) return -1;
    s.Nr = paths_pad4z((size_t)s.N);
    const long long big[] = {s.N * s.ldw, s.N * s.ldM, s.N * s.ldF};
    for (long long v : big)
        if (v > PP_IDX_MAX) return -1;
    const size_t N = (size_t)s.N;
    size_t o = 0;
    s.o_x = o;   o += N * s.ldw;
    s.o_xn = o;  o += s.Nr;
    s.o_k = o;   o += N * s.ldM;
    s.o_t = o;   o += N * s.ldF;
    s.o_vp = o;  o += s.Nr;
    s.o_p = o;   o += N * s.ldM;
    s.o_sig = o; o += s.Nr;
    s.o_o1 = o;  o += want_grad ? N * s.ldw : 0;
    s.o_o2 = o;  o += want_grad ? N * s.ldw : 0;
    s.o_gp = o;  o += want_grad ? N * s.ldw : 0;
    s.total = o;
    return 0;
}

// ---- device-resident descent (dsvgp_paths_descend): projected gradient steps of every (sample, start) pair on its own path ----------
// One trial per iteration, a step length per pair: accept iff  sigma f_y <= sigma f + c1 sigma g.(y - x)  (sigma = +1 to minimise, -1 to
// maximise), then eta <- min(GROW eta, ETA_MAX), else eta <- SHRINK eta.  Workspace (floats): y[N d'] | gy[N d'] | fy[Nr] and behind them
// the evaluation's own (d' = N d padded to 4 floats; N = n B).
constexpr float PP_DESCEND_C1 = 1e-4f;
constexpr float PP_DESCEND_GROW = 2.f;
constexpr float PP_DESCEND_SHRINK = 0.5f;
constexpr float PP_DESCEND_ETA_MAX = 1e30f;              // the finite ceiling of a step length
constexpr float PP_DESCEND_TINY = 1e-30f;                // floor of |g| in the first step length
constexpr float PP_DESCEND_STEP0 = 0.25f;                // initial_step <= 0: this many lengthscales
struct PathsDescendWork { size_t o_y, o_gy, o_fy, o_eval, total; };
inline int paths_descend_work(int M, int d, int F, int n, int B, PathsDescendWork& s) {
    if (M < 1 || d < 1 || F < 1 || n < 1 || B < 1) return -1;
    s = PathsDescendWork{};
    const long long N = (long long)n * B;
    if (N > PP_IDX_MAX || N * d > PP_IDX_MAX) return -1;
    size_t ev = 0;
    if (d > PP_FUSED_MAX_D) {
        PathsOwnWork w;
        if (paths_own_work(M, d, F, n, B, 1, w)) return -1;
        ev = w.total;
    }
    const size_t nd = paths_pad4z((size_t)N * d), nr = paths_pad4z((size_t)N);
    s.o_y = 0; s.o_gy = nd; s.o_fy = 2 * nd; s.o_eval = 2 * nd + nr;
    s.total = s.o_eval + ev;
    return 0;
}
