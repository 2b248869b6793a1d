/*
 * dsvgp.h -- C ABI of the MI355X (gfx950) DSVGP minibatch-ELBO hot path.
 *
 * The reference (mishapadidar/GP-Derivatives-Variational-Inference) is pure Python on top of
 * GPyTorch; it has no FFI.  These entry points are what a native binding for the hot path
 * would expose: every function takes plain device pointers, sizes and the context (which carries
 * the HIP stream), returns 0 on success, a negative DSVGP_E* code for bad arguments and a positive
 * hipError_t / rocblas_status (offset by 1000) for runtime failures.  No torch types.
 *
 * Conventions
 *   - all matrices are dense ROW-MAJOR with an explicit leading dimension (elements, not bytes);
 *   - all pointers are DEVICE pointers unless the name ends in _host;
 *   - the library never allocates or frees caller-visible memory; workspaces are passed in and
 *     sized by the *_workspace_bytes helpers;
 *   - kernels are enqueued on the stream given to dsvgp_set_stream and do not synchronise
 *     (exceptions are documented);
 *   - "interleaved" layout: row i*(p+1) is the function value at point i, rows i*(p+1)+1+a the
 *     derivative along point i's a-th direction (reference RBFKernelDirectionalGrad.py:105-107).
 *   - hyp is a device float[4] = { lengthscale, outputscale, noise, unused } produced by
 *     dsvgp_hyp_forward from the raw (softplus-constrained) parameters.
 *
 * Reference interface replaced by each entry point is cited as file:line under /root/reference.
 */
#ifndef DSVGP_H
#define DSVGP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsvgp_ctx dsvgp_ctx;

enum {
    DSVGP_OK = 0,
    DSVGP_EINVAL = -1,     /* bad argument / unsupported shape        */
    DSVGP_ENOTPD = -2,     /* Cholesky failed (matrix not PD)         */
    DSVGP_EALIGN = -3,     /* pointer / leading dimension misaligned  */
    DSVGP_ENOSPACE = -4    /* a caller-sized buffer filled up: call again with a larger one */
};

/* ---- context ------------------------------------------------------------------------------- */
int dsvgp_create(dsvgp_ctx** ctx);                 /* creates the rocBLAS handle used by rocSOLVER potrf */
int dsvgp_destroy(dsvgp_ctx* ctx);
int dsvgp_set_stream(dsvgp_ctx* ctx, void* hip_stream);
/* Deterministic mode (round 3).  With a caller-owned scratch buffer set, every split-K product stores its K slices to slabs in
 * the scratch and adds them in a fixed order instead of meeting in floating-point atomics (fp32 Gram product, the fp64 M' x M' x M'
 * products, the small-problem split-K products), and the scalar reductions of the step (residual / likelihood sums) go through
 * per-workgroup partials: two runs on the same inputs are bitwise equal.  scratch == NULL: back to atomics (the default; their
 * rounding depends on the order in which workgroups retire).  The scratch serves the launches queued on the context's current
 * stream, one stream at a time; a product whose slices do not fit it runs with fewer, longer slices (unsplit below two).
 * The reference (CPU torch) is deterministic for a fixed seed; this mode gives the HIP path the same property.          */
int dsvgp_set_deterministic(dsvgp_ctx* ctx, void* scratch, size_t bytes);
/* Scratch size for the FLOAT64 model mode under dsvgp_set_deterministic (pure host function, no device call): enough for the largest
 * user on any float64 path of an (M inducing points, d, p directions, B data points) step -- split-K slabs of the [M', M' + 1]
 * products, the per-chunk partial rows of the column sums over B' (dsvgp_colstats_f64, dsvgp_gemv_f64 transposed), the per-workgroup
 * partials of the scalar sums, and the tiled kernel backward's dP1 slabs, one per sweep group (p > 16).  0 for a shape the float64
 * entry points do not take.  A smaller scratch is legal: a launcher whose partials do not fit runs unsplit (one writer per address)
 * or returns DSVGP_EINVAL; none falls back to atomics while the mode is on.                                                        */
size_t dsvgp_deterministic_f64_scratch_bytes(int M, int d, int p, int B);
const char* dsvgp_version(void);

/* ---- hyper-parameters: gpytorch Positive / GreaterThan(1e-4) softplus constraints ------------
 * replaces ScaleKernel.outputscale, RBFKernel.lengthscale, GaussianLikelihood.noise
 * (directionalvi/directional_vi.py:56,172).  raw = {raw_lengthscale, raw_outputscale, raw_noise}. */
int dsvgp_hyp_forward(dsvgp_ctx* ctx, const float* raw_lengthscale, const float* raw_outputscale,
                      const float* raw_noise, float* hyp);
/* chain rule back to the raw parameters: d_raw += d_hyp * sigmoid(raw) */
int dsvgp_hyp_backward(dsvgp_ctx* ctx, const float* raw_lengthscale, const float* raw_outputscale,
                       const float* raw_noise, const float* d_hyp, float* d_raw_lengthscale,
                       float* d_raw_outputscale, float* d_raw_noise);
/* The scalar tail of one step in a single launch: d_hyp += data-term scalars (scal[4], scal[3], scal[1] of
 * dsvgp_likelihood_terms / dsvgp_elbo_fast_finalize), the softplus chain rule of dsvgp_hyp_backward, d constant +=
 * scal[2], and loss = -scal[0] / rows + kl0[0] / num_data  (VariationalELBO, directional_vi.py:217,245-246).  */
int dsvgp_step_epilogue(dsvgp_ctx* ctx, const float* scal, const float* kl0, double rows, double num_data,
                        const float* raw_lengthscale, const float* raw_outputscale, const float* raw_noise,
                        float* d_hyp, float* d_raw_lengthscale, float* d_raw_outputscale, float* d_raw_noise,
                        float* d_constant, float* loss);

/* ---- kernel assembly: RBFKernelDirectionalGrad.forward (directionalvi/RBFKernelDirectionalGrad.py:41-119)
 *
 * dsvgp_pack_points: x[n,d], v[n*p,d] (raw directions, normalised here, :57-58) ->
 *   P[n*(p+1), DP] packed operand rows (x/ell and unit directions, zero padded, plus the indicator
 *   column used by the backward), self[n*(p+1)] (|x/ell|^2 and (x/ell).v), vnorm[n*p].
 *   DP = dsvgp_packed_width(d).  center[d] (may be NULL = 0): common shift subtracted from x before
 *   the 1/ell scaling; both operands of one kernel call must be packed with the SAME center.  The
 *   kernel is shift invariant; centering (gpytorch 1.4.0 Kernel.covar_dist: `adjustment =
 *   x1.mean(-2)`, reached from RBFKernelDirectionalGrad.py:71) keeps |x~|^2 small so that the fp32
 *   quadratic expansion |x~1|^2 + |x~2|^2 - 2 x~1.x~2 loses ~4x fewer digits.
 * dsvgp_column_mean: out[d] = mean over the n rows of x[n,d] (the center above).                 */
int dsvgp_packed_width(int d);
int dsvgp_column_mean(dsvgp_ctx* ctx, const float* x, int n, int d, float* out);
int dsvgp_pack_points(dsvgp_ctx* ctx, const float* x, const float* v, int n, int d, int p,
                      const float* hyp, const float* center, float* P, float* self, float* vnorm);

/* out[n1*(p+1), n2*(p+1)] = hyp.outputscale * K(x1,x2;v1,v2) (+ jitter on the global diagonal).
 * out_is_double: 0 -> float output, 1 -> double output (fp32 values widened, as the reference's
 * `.double()` cast, DirectionalGradVariationalStrategy.py:74,181).                               */
int dsvgp_kernel_fwd(dsvgp_ctx* ctx, const float* P1, const float* self1, int n1, const float* P2,
                     const float* self2, int n2, int d, int p, const float* hyp, float jitter,
                     void* out, int64_t ld, int out_is_double);
/* The same product when the directions of side 2 are CANONICAL unit vectors shared by all its points -- what the reference's callers
 * pass for K_ZX: select_cols_of_y's E_canonical[idx - 1] tiled over the minibatch (directional_vi.py:81-88, 238), eye(d)[:p] tiled in
 * eval_gp (:292-294).  dir_idx[p] (device memory): direction b is the unit vector of coordinate dir_idx[b] - idx_base (idx_base = 1 takes
 * idx_y[1:] of select_cols_of_y as it stands).  P2 / self2: the packed rows of side 2 (only the value rows are read).  float output, no
 * jitter.  Returns DSVGP_EINVAL for geometries the canonical kernels do not take (p + 1 not in {3, 6} or d > 28): use dsvgp_kernel_fwd. */
int dsvgp_kernel_fwd_canon(dsvgp_ctx* ctx, const float* P1, const float* self1, int n1, const float* P2,
                           const float* self2, int n2, int d, int p, const int* dir_idx, int idx_base,
                           const float* hyp, float* out, int64_t ld);
/* diag=True branch (:110-119): out[n*(p+1)] = outputscale * [1, 1/ell^2, ...]                    */
int dsvgp_kernel_diag(dsvgp_ctx* ctx, int n, int p, const float* hyp, float* out);

/* backward of dsvgp_kernel_fwd w.r.t. (x1, v1, lengthscale, outputscale), given G = dLoss/dOut.
 * symmetric != 0: x1==x2, v1==v2 and G symmetric (the K_ZZ case) -> point/direction grads doubled.
 * Accumulates (+=) into d_x1[n1,d], d_v1[n1*p,d] and d_hyp[0..1].  g_is_double selects G's dtype. */
size_t dsvgp_kernel_bwd_workspace_bytes(int n1, int n2, int d, int p);
int dsvgp_kernel_bwd(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1,
                     const float* self1, const float* vnorm1, int n1, const float* P2,
                     const float* self2, int n2, int d, int p, const float* hyp, int symmetric,
                     float* d_x1, float* d_v1, float* d_hyp, void* workspace);
/* Packed width dsvgp_packed_width(d) > 96 (d >= 93): dsvgp_pack_points, dsvgp_kernel_fwd, dsvgp_kernel_bwd and
 * dsvgp_kernel_bwd_workspace_bytes route to the wide-input kernels, which accumulate T = P1 P2^T over a K loop of fixed column chunks
 * (workgroup LDS independent of d).  The _wide entries below run those kernels for ANY d >= 1, with the arguments and contracts of
 * dsvgp_kernel_fwd / dsvgp_kernel_bwd (workspace: dsvgp_kernel_bwd_wide_workspace_bytes).  The backward uses no floating-point atomics. */
int dsvgp_kernel_fwd_wide(dsvgp_ctx* ctx, const float* P1, const float* self1, int n1, const float* P2,
                          const float* self2, int n2, int d, int p, const float* hyp, float jitter,
                          void* out, int64_t ld, int out_is_double);
size_t dsvgp_kernel_bwd_wide_workspace_bytes(int n1, int n2, int d, int p);
int dsvgp_kernel_bwd_wide(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1,
                          const float* self1, const float* vnorm1, int n1, const float* P2,
                          const float* self2, int n2, int d, int p, const float* hyp, int symmetric,
                          float* d_x1, float* d_v1, float* d_hyp, void* workspace);
/* Rectangular assembly (csrc/assemble_wide.hip): the two sides carry DIFFERENT numbers of directions.
 *   out[n1*(p1+1), n2*(p2+1)] (float, leading dimension ld >= n2*(p2+1)) = hyp.outputscale * K(x1, x2; v1, v2), interleaved as
 *   dsvgp_kernel_fwd: micro-block (i, j) is k [[1, w_b/ell], [-u_a/ell, (G_ab - u_a w_b)/ell^2]] for a = 1..p1, b = 1..p2, with
 *   r = (x1_i - x2_j)/ell, k = exp(-|r|^2/2), u_a = r.v1_ia, w_b = r.v2_jb, G_ab = v1_ia.v2_jb (unit directions).
 * P1 / self1 and P2 / self2: what dsvgp_pack_points wrote for each side WITH THAT SIDE'S OWN p and the same center; p = 0 on a
 * side: value rows only.  Float output, no jitter (backward: dsvgp_kernel_bwd_rect below).  Any d >= 1 (the workgroup's LDS does not depend on d) and any
 * 0 <= p1, p2 <= 95, independently.  One launch, no intermediate in device memory, every element stored once, no atomics: two
 * identical calls give bitwise equal results; at p1 == p2 the arithmetic is that of dsvgp_kernel_fwd_wide.
 * Alignment: P1 and P2 must be 16-byte aligned (their rows, dsvgp_packed_width(d) floats, are read 16 bytes at a time); `out` and
 * `ld` carry no requirement beyond ld >= n2*(p2+1) (element-wise stores).
 * DSVGP_EINVAL: a null pointer, n1 <= 0 or n2 <= 0, d < 1, p1 or p2 outside [0, 95], n*(p+1) beyond INT_MAX on a side, more than
 * 65535 row tiles (n1*(p1+1) above ~3.1e6 at the 48-row tile), ld too small, P1 or P2 misaligned.                                */
int dsvgp_kernel_fwd_rect(dsvgp_ctx* ctx, const float* P1, const float* self1, int n1, int p1, const float* P2,
                          const float* self2, int n2, int p2, int d, const float* hyp, float* out, int64_t ld);
/* Backward of dsvgp_kernel_fwd_rect with respect to side 1 (x1, v1) and (lengthscale, outputscale), given G = dLoss/dOut
 * [n1*(p1+1), n2*(p2+1)] with leading dimension ldg >= n2*(p2+1); g_is_double selects G's dtype (float / double).  Side 2 is data and
 * receives no gradient; there is no symmetric case (the square K_ZZ goes through dsvgp_kernel_bwd).
 * Accumulates (+=) into d_x1[n1, d], d_v1[n1*p1, d] and d_hyp[0..1] (lengthscale, outputscale), as dsvgp_kernel_bwd does; p1 = 0 needs
 * neither vnorm1 nor d_v1 (both may be null).  P1 / self1 / vnorm1 and P2 / self2: what dsvgp_pack_points wrote for each side with that
 * side's own p and the same center.  Any d >= 1 and any 0 <= p1, p2 <= 95, independently.
 * Three launches -- Tbar tiles [n1*(p1+1), n2*(p2+1)] into the workspace, their contraction with the packed rows of side 2 into split
 * slabs, the points launch that adds slabs and per-workgroup partial sums in a fixed order -- and no floating-point atomics: two
 * identical calls give bitwise equal results.  At p1 == p2 > 0 tiles and arithmetic are those of dsvgp_kernel_bwd_wide (symmetric = 0).
 * workspace: dsvgp_kernel_bwd_rect_workspace_bytes bytes of device memory for these shapes, 4-byte aligned (a pure host function; 0 for
 * n1 <= 0, n2 <= 0, d < 1, p1 or p2 outside [0, 95] or a grid beyond the limits below).  Alignment: P1 and P2 16 bytes, G its element size.
 * DSVGP_EINVAL: a null pointer, d < 1, p1 or p2 outside [0, 95], negative n1 / n2, n*(p+1) beyond INT_MAX on a side, more than 65535
 * row tiles or 64-row contraction tiles, ldg too small, P1 or P2 misaligned.  n1 == 0 or n2 == 0: returns 0, nothing is touched. */
size_t dsvgp_kernel_bwd_rect_workspace_bytes(int n1, int p1, int n2, int p2, int d);
int dsvgp_kernel_bwd_rect(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1,
                          const float* vnorm1, int n1, int p1, const float* P2, const float* self2, int n2, int p2, int d,
                          const float* hyp, float* d_x1, float* d_v1, float* d_hyp, void* workspace);
/* ---- ARD: one lengthscale per input dimension (csrc/assemble_ard.hip) --------------------------------------------------------------
 * The packed rows carry the per-dimension scaling, x~ = (x - c) ./ ell and v~_a = (v_a / |v_a|) ./ ell with ell[d], and the kernels
 * run with hyp[0] = 1: micro-block (i, j) of the ARD kernel is k [[1, w~_b], [-u~_a, v~_a.v~_b - u~_a w~_b]], r = x~1 - x~2,
 * u~_a = r.v~1_a, w~_b = r.v~2_b, k = s exp(-|r|^2/2).  The FORWARD is dsvgp_kernel_fwd_wide (K_ZZ: double output, jitter) or
 * dsvgp_kernel_fwd_rect on ARD packs with the hyp below; the _canon / _canon2 kernels (unit one-hot data directions) are not for ARD.
 * All entries: fixed summation orders, no floating-point atomics, two identical calls are bitwise equal.
 *
 * dsvgp_hyp_forward_ard: ell[k] = softplus(raw_lengthscale[k]), k < d; hyp[4] as dsvgp_hyp_forward writes it except hyp[0] = 1.
 * dsvgp_hyp_backward_ard: d_raw_lengthscale[k] += d_ell[k] sigmoid(raw_lengthscale[k]); d_raw_outputscale / d_raw_noise += as
 *   dsvgp_hyp_backward from d_hyp[1], d_hyp[2] (d_hyp[0] is not read).  DSVGP_EINVAL: a null pointer, d < 1.                         */
int dsvgp_hyp_forward_ard(dsvgp_ctx* ctx, const float* raw_lengthscale, int d, const float* raw_outputscale, const float* raw_noise,
                          float* ell, float* hyp);
int dsvgp_hyp_backward_ard(dsvgp_ctx* ctx, const float* raw_lengthscale, int d, const float* raw_outputscale, const float* raw_noise,
                           const float* d_ell, const float* d_hyp, float* d_raw_lengthscale, float* d_raw_outputscale,
                           float* d_raw_noise);
/* dsvgp_pack_points with ell[d] in place of hyp: the same layout (P[n*(p+1), DP], DP = dsvgp_packed_width(d), zero padding, indicator
 * column DP - 4 on value rows), rows x~ and v~_a as above, self = |x~|^2 and x~.v~_a by the k-ordered fma chain of the kernels' MFMA
 * product (r == 0 stays exact on the diagonal micro-blocks of K_ZZ), vnorm = |v|.  One wave per row: any d >= 1.  Both sides of a kernel
 * call are packed with the same ell and center (center may be null = 0); v and vnorm may be null at p = 0.
 * DSVGP_EINVAL: a null pointer, n < 0, d < 1, p outside [0, 95], n*(p+1) beyond INT_MAX.  n == 0: returns 0.                          */
int dsvgp_pack_points_ard(dsvgp_ctx* ctx, const float* x, const float* v, int n, int d, int p, const float* ell, const float* center,
                          float* P, float* self, float* vnorm);
/* The prior diagonal of the ARD kernel from a pack: out[i*(p+1)] = s, out[i*(p+1) + a] = s |v~_ia|^2 (in place of s / ell^2), and its
 * backward given gbar[n*(p+1)] and the forward's out: d_hyp[1] += sum gbar out / s, d_ell[k] += -(2 s / ell_k) sum_{i, a >= 1}
 * gbar_ia v~_iak^2 (one workgroup per k, fp64 partial sums in a fixed order).  Same refusals as dsvgp_pack_points_ard.                */
int dsvgp_kernel_diag_ard(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* hyp, float* out);
int dsvgp_kernel_diag_ard_bwd(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* ell, const float* hyp, const float* out,
                              const float* gbar, float* d_ell, float* d_hyp);
/* Backward of the ARD kernel out[n1*(p1+1), n2*(p2+1)] with respect to side 1 (x1, v1), the lengthscale vector and the outputscale,
 * given G = dLoss/dOut (leading dimension ldg >= n2*(p2+1); g_is_double selects float / double).  Accumulates (+=) into d_x1[n1, d],
 * d_v1[n1*p1, d], d_ell[d] (through BOTH sides' packed rows) and d_hyp[1]; d_hyp[0] is not touched.  d_ell may be null (a second call
 * with the sides swapped, for side 2's point gradients, must not count d_ell and d_hyp twice: pass d_ell = null there and a scratch
 * d_hyp); d_v1 may be null (vnorm1 is then not read; p1 = 0 needs neither).  The other outputs do not depend on whether d_ell is given.
 * symmetric != 0: n1 == n2, p1 == p2, side 2 IS side 1 (the same pack) and G is symmetric -- the K_ZZ case: point and direction
 * gradients doubled, side 2's share of d_ell taken from side 1.
 * Launches: the Tbar tiles and their contraction with side 2's rows exactly as dsvgp_kernel_bwd_rect runs them (hyp[0] = 1), a points
 * reduction per point of side 1, for d_ell and symmetric == 0 the column sums of Tbar over side 1's value rows and side 2's self-term
 * rows, and a fixed-order column reduction (fp64 partial sums).
 * workspace: dsvgp_kernel_bwd_ard_workspace_bytes bytes, 4-byte aligned (a pure host function; 0 for shapes that
 * dsvgp_kernel_bwd_rect_workspace_bytes refuses).  dsvgp_kernel_bwd_ard_slabs: how many split slabs the contraction writes for these
 * shapes (0: refused).  Alignment: P1 and P2 16 bytes, G its element size.
 * DSVGP_EINVAL: a null pointer other than the optional ones, d < 1, p1 or p2 outside [0, 95], negative n1 / n2, symmetric with n1 != n2
 * or p1 != p2, n*(p+1) beyond INT_MAX on a side, more than 65535 row tiles or 64-row contraction tiles, ldg too small, P1 or P2
 * misaligned.  n1 == 0 or n2 == 0: returns 0, nothing is touched.                                                                     */
size_t dsvgp_kernel_bwd_ard_workspace_bytes(int n1, int p1, int n2, int p2, int d);
int dsvgp_kernel_bwd_ard_slabs(int n1, int p1, int n2, int p2, int d);
int dsvgp_kernel_bwd_ard(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1,
                         const float* vnorm1, int n1, int p1, const float* P2, const float* self2, int n2, int p2, int d,
                         const float* ell, const float* hyp, int symmetric, float* d_x1, float* d_v1, float* d_ell, float* d_hyp,
                         void* workspace);
/* ---- Matern-5/2 with directional derivatives (csrc/assemble_matern.hip) -------------------------------------------------------------
 * The second kernel family, on the ARD packs above (dsvgp_pack_points_ard; a scalar lengthscale is ell[d] with equal entries) and
 * dsvgp_hyp_forward_ard's hyp (hyp[0] = 1 is not read).  With r = x~1 - x~2, nn = |r|^2, a = sqrt(5 nn), e = exp(-a) and
 *   f0 = (1 + a + a^2/3) e,  f1 = (5/3)(1 + a) e,  f2 = (25/3) e
 * micro-block (i, j) is s [[f0, f1 w~_b], [-f1 u~_a, f1 v~_a.v~_b - f2 u~_a w~_b]] (u~_a = r.v~1_a, w~_b = r.v~2_b); the RBF kernel is the
 * case f0 = f1 = f2 = exp(-nn/2).  All entries: fixed summation orders, no floating-point atomics, two identical calls are bitwise equal.
 *
 * dsvgp_kernel_fwd_matern52: out[n1*(p1+1), n2*(p2+1)] (float, or double when out_is_double), leading dimension ld, `jitter` added on the
 * global diagonal (row index == column index: pass 0 unless both sides are the same pack -- K_ZZ).  Any d >= 1 and any 0 <= p1, p2 <= 95,
 * independently; one launch on the tiles of dsvgp_kernel_fwd_rect, every element stored once.  On K_ZZ the value diagonal is s + jitter
 * exactly.  DSVGP_EINVAL, nothing touched: whatever dsvgp_kernel_fwd_rect refuses, or `out` not aligned to its element size.
 * dsvgp_kernel_fwd_matern52_lds_bytes: the dynamic LDS of that launch for the direction counts (host arithmetic; 0: refused).        */
int dsvgp_kernel_fwd_matern52(dsvgp_ctx* ctx, const float* P1, const float* self1, int n1, int p1, const float* P2,
                              const float* self2, int n2, int p2, int d, const float* hyp, float jitter, void* out, int64_t ld,
                              int out_is_double);
size_t dsvgp_kernel_fwd_matern52_lds_bytes(int p1, int p2);
/* Backward of dsvgp_kernel_fwd_matern52: the arguments, optional pointers, `symmetric`, += semantics, alignment and refusals of
 * dsvgp_kernel_bwd_ard.  Launches: the Matern Tbar tiles (the LDS of dsvgp_kernel_bwd_rect's Tbar launch), then the contraction and the
 * points / column-sum / self-rows / reduce launches of dsvgp_kernel_bwd_ard unchanged.  d_hyp[1] += sum(G o K) / s, accumulated
 * directly per tile.  A pair at distance 0 (K_ZZ's diagonal blocks, duplicate points) contributes finite, exact terms.
 * workspace: dsvgp_kernel_bwd_matern52_workspace_bytes bytes: dsvgp_kernel_bwd_ard_workspace_bytes (the same layout) rounded up to a
 * multiple of 16; 0 where that returns 0.                                                                                              */
size_t dsvgp_kernel_bwd_matern52_workspace_bytes(int n1, int p1, int n2, int p2, int d);
int dsvgp_kernel_bwd_matern52(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* self1,
                              const float* vnorm1, int n1, int p1, const float* P2, const float* self2, int n2, int p2, int d,
                              const float* ell, const float* hyp, int symmetric, float* d_x1, float* d_v1, float* d_ell, float* d_hyp,
                              void* workspace);
/* The prior diagonal out[i*(p+1)] = s, out[i*(p+1) + a] = (5/3) s |v~_ia|^2 and its backward: d_hyp[1] += sum gbar out / s,
 * d_ell[k] += -(2 (5/3) s / ell_k) sum_{i, a >= 1} gbar_ia v~_iak^2.  Signatures and refusals of dsvgp_kernel_diag_ard / _bwd.        */
int dsvgp_kernel_diag_matern52(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* hyp, float* out);
int dsvgp_kernel_diag_matern52_bwd(dsvgp_ctx* ctx, const float* P, int n, int p, int d, const float* ell, const float* hyp,
                                   const float* out, const float* gbar, float* d_ell, float* d_hyp);
/* 1 when dsvgp_kernel_fwd_canon / _bwd_canon take the geometry (d, p), 0 otherwise */
int dsvgp_kernel_canon_supported(int d, int p);
/* The dynamic LDS, in bytes, of the launch that dsvgp_kernel_fwd (launch = 0), dsvgp_kernel_bwd (1), dsvgp_kernel_fwd_canon (2) or
 * dsvgp_kernel_bwd_canon (3: upstream through registers, 4: float upstream by LDS-DMA) makes at (d, p): host arithmetic on the kernels'
 * own LDS layouts.  0: a geometry the entry refuses, or a packed width > 96 (the wide-input kernels).                                */
size_t dsvgp_kernel_lds_bytes(int d, int p, int launch);
/* backward of dsvgp_kernel_fwd_canon (symmetric = 0 semantics; same workspace size as dsvgp_kernel_bwd) */
int dsvgp_kernel_bwd_canon(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1,
                           const float* self1, const float* vnorm1, int n1, const float* P2,
                           const float* self2, int n2, int d, int p, const int* dir_idx, int idx_base,
                           const float* hyp, float* d_x1, float* d_v1, float* d_hyp, void* workspace);

/* One-hot directions on BOTH sides, the same index list for every point of both: the full-gradient SVGP (reference
 * directionalvi/GradVariationalStrategy.py:89-99 builds RBFKernelGrad over cat([Z, x]) -- the directional kernel with p = d and the
 * directions I_d at every inducing and data point; BASELINE config 3) or inducing directions fixed to the data's canonical columns.
 * Every block is then an elementwise function of x1 - x2 (no products): K00 = k, K0b = k delta_b / ell, Ka0 = -k delta_a / ell,
 * Kab = k ([a == b] - delta_a delta_b) / ell^2.  P1 / P2: packed rows (only the value rows are read); dir_idx / idx_base as above.
 * _supported: 1 for the geometries taken (p + 1 = 11, d <= 12), else 0 -- the entry points return DSVGP_EINVAL and the caller uses the
 * general kernels.  fwd: float / double output, jitter on the global diagonal as dsvgp_kernel_fwd.  bwd: accumulates (+=) d_x1,
 * d_hyp[0..1] as dsvgp_kernel_bwd (symmetric != 0: K_ZZ, point gradients doubled); d_v1 receives nothing (fixed directions); G's rows
 * must consist of 16-byte pieces (ldg % 4 == 0 floats / % 2 == 0 doubles, base 16-byte aligned), DSVGP_EINVAL otherwise; workspace of
 * dsvgp_kernel_bwd_workspace_bytes(n1, n2, d, p).                                                                                   */
int dsvgp_kernel_canon2_supported(int d, int p);
int dsvgp_kernel_fwd_canon2(dsvgp_ctx* ctx, const float* P1, int n1, const float* P2, int n2, int d, int p, const int* dir_idx,
                            int idx_base, const float* hyp, float jitter, void* out, int64_t ld, int out_is_double);
int dsvgp_kernel_bwd_canon2(dsvgp_ctx* ctx, const void* G, int64_t ldg, int g_is_double, const float* P1, const float* vnorm1, int n1,
                            const float* P2, int n2, int d, int p, const int* dir_idx, int idx_base, const float* hyp, int symmetric,
                            float* d_x1, float* d_v1, float* d_hyp, void* workspace);

/* ---- fp64 model mode (the reference's experiments set torch.set_default_dtype(torch.float64),
 * experiments/synthetic/exp_script.py:56): RBFKernelDirectionalGrad.forward / backward in double precision.
 * Same packed-row formulation as the fp32 assembly; the two contractions T = P1 P2^T and dP1 = Tbar P2 go through
 * dsvgp_gemm (fp64 MFMA), these entry points do the rest:
 *   dsvgp_pack_points_f64           x[n,d], v[n*p,d] -> P[n(p+1), DP] (DP = dsvgp_packed_width(d)), self, vnorm (doubles)
 *   dsvgp_kernel_transform_f64      T[n1(p+1), n2(p+1)] -> outputscale * K in place (+ jitter on the global diagonal)
 *   dsvgp_kernel_bwd_transform_f64  (G = dLoss/dK, T) -> Tbar in place of T; d_hyp[0] += d lengthscale, d_hyp[1] += d outputscale
 *   dsvgp_kernel_bwd_points_f64     dP1[n1(p+1), DP] = Tbar [P2 | indicator] -> d_x1 +=, d_v1 += (x2 when symmetric)
 * hyp: device double[3+] = {lengthscale, outputscale, noise}.  The two transform entries keep the directions of a micro-block in
 * per-thread registers and take p <= 16; dsvgp_pack_points_f64 and dsvgp_kernel_bwd_points_f64 take p <= 95.               */
int dsvgp_pack_points_f64(dsvgp_ctx* ctx, const double* x, const double* v, int n, int d, int p, const double* hyp,
                          const double* center, double* P, double* self, double* vnorm);
int dsvgp_kernel_transform_f64(dsvgp_ctx* ctx, double* T, int64_t ld, const double* self1, int n1, const double* self2,
                               int n2, int p, const double* hyp, double jitter);
int dsvgp_kernel_bwd_transform_f64(dsvgp_ctx* ctx, const double* G, int64_t ldg, double* T, int64_t ldt, const double* self1,
                                   int n1, const double* self2, int n2, int p, const double* hyp, double* d_hyp);
 /* fp64 column statistics and their backward (DGVS.py:188,192-205): mu_j = sum_i A_ij m_i, cs_j = sum_i (W_ij^2 - A_ij^2) (W may be
 * NULL: mean only);  Abar = m mu_bar^T + 2 (U - A) diag(var_bar), Av = 2 A diag(var_bar) (U NULL: U = A; Av may be NULL) */
int dsvgp_colstats_f64(dsvgp_ctx* ctx, const double* A, int64_t lda, const double* W, int64_t ldw, const double* m, int Mp, int Bp,
                       double* mu, double* cs);
int dsvgp_abar_f64(dsvgp_ctx* ctx, const double* A, int64_t lda, const double* U, int64_t ldu, const double* m, const double* mu_bar,
                   const double* var_bar, int Mp, int Bp, double* Abar, int64_t ldo, double* Av, int64_t ldv);
/* likelihood terms of the fp64 model (GaussianLikelihood + VariationalELBO mll_type 0 / PredictiveLogLikelihood 1,
 * directional_vi.py:172,217,245-246): mu = mu0 + constant, varn = max(s dg + 1e-4 + cs + noise, 1e-6) per output (p derivative
 * outputs per point), mu_bar / var_bar = d loss / d mu0, d cs with loss = -(sum ll) / rows, and
 * scal[8] (zeroed here) = {sum ll, d/d noise, d/d constant, d/d outputscale, d/d lengthscale (prior-diagonal parts), 0, 0, 0}  */
int dsvgp_likelihood_terms_f64(dsvgp_ctx* ctx, const double* mu0, const double* cs, const double* y, const double* constant,
                               int ncols, int p, const double* hyp, int mll_type, double rows, double* mu, double* varn,
                               double* mu_bar, double* var_bar, double* scal);
/* scalar tail of the fp64 ELBO fast path (the variances enter the ELBO only through their sum: tvar[0] = tr(L_S^T G L_S) - tr G on
 * the device): mu = mu0 + constant, mu_bar = d loss / d mu0, and scal[8] = {sum ll, d loss / d noise, d / d constant, d / d outputscale,
 * d / d lengthscale (prior-diagonal parts), vbar = d loss / d tvar = 1 / (2 noise rows), sum r^2, sum r}; ncols = npts (pd + 1) outputs
 * (GaussianLikelihood.expected_log_prob summed, VariationalELBO: directional_vi.py:217,245-246)                                   */
int dsvgp_elbo_fast_tail_f64(dsvgp_ctx* ctx, const double* mu0, const double* y, const double* constant, int ncols, int npts, int pd,
                             const double* hyp, const double* tvar, double rows, double* mu, double* mu_bar, double* scal);
int dsvgp_kernel_bwd_points_f64(dsvgp_ctx* ctx, const double* dP, const double* P1, const double* vnorm1, int n1, int d,
                                int p, const double* hyp, int symmetric, double* d_x1, double* d_v1);
/* Tiled fp64 assembly (csrc/assemble64_tiled.hip): the same kernel matrix and the same backward from the packs of
 * dsvgp_pack_points_f64, for ANY 0 <= p <= 95 and any d >= 1 (workgroup LDS independent of d), with T = P1 P2^T computed on the fp64
 * MFMA inside the assembly kernels -- no [n1 (p+1), n2 (p+1)] intermediate.  DSVGP_EINVAL for p > 95, ld / ldg < n2 (p+1), bases that
 * are not 8-byte aligned, symmetric != 0 with n1 != n2.
 *   dsvgp_kernel_fwd_f64   out[n1(p+1), n2(p+1)] (leading dimension ld) = outputscale * K; symmetric != 0 (x1 == x2, v1 == v2: K_ZZ)
 *                          adds jitter on the global diagonal, symmetric == 0 ignores jitter.
 *   dsvgp_kernel_bwd_f64   G = dLoss/dOut -> d_x1[n1,d] +=, d_v1[n1*p,d] +=, d_hyp[0] += d lengthscale, d_hyp[1] += d outputscale, as
 *                          the sequence gemm, dsvgp_kernel_bwd_transform_f64, gemm, dsvgp_kernel_bwd_points_f64 (symmetric != 0: point
 *                          and direction gradients doubled).  workspace: dsvgp_kernel_bwd_f64_workspace_bytes(n1, n2, d, p) bytes of
 *                          device memory (0 = geometry not taken), cleared here; sums meet in fp64 atomics (run-order rounding),
 *                          or, under dsvgp_set_deterministic, in per-sweep-group slabs of the scratch added in a fixed order.        */
int dsvgp_kernel_fwd_f64(dsvgp_ctx* ctx, const double* P1, const double* self1, int n1, const double* P2, const double* self2,
                         int n2, int d, int p, const double* hyp, double jitter, int symmetric, double* out, int64_t ld);
size_t dsvgp_kernel_bwd_f64_workspace_bytes(int n1, int n2, int d, int p);
int dsvgp_kernel_bwd_f64(dsvgp_ctx* ctx, const double* G, int64_t ldg, const double* P1, const double* self1, const double* vnorm1,
                         int n1, const double* P2, const double* self2, int n2, int d, int p, const double* hyp, int symmetric,
                         double* d_x1, double* d_v1, double* d_hyp, void* workspace, size_t workspace_bytes);

/* ---- Cholesky: psd_safe_cholesky(K_ZZ.double()) (DirectionalGradVariationalStrategy.py:72-75)
 * In-place lower Cholesky of the row-major fp64 matrix A[n,n] (rocSOLVER dpotrf); only the lower
 * triangle is read/written.  info_dev is a device int (0 = ok, k>0 = leading minor k not PD).   */
/* algo 0: rocSOLVER dpotrf (no workspace).  algo 1: blocked right-looking Cholesky, one fused fp64 MFMA launch per
 * 64-column block (trailing update + factorisation / inversion of the next diagonal block out of LDS) and one
 * batched panel launch; workspace of dsvgp_potrf_workspace_bytes.                                           */
size_t dsvgp_potrf_workspace_bytes(int n, int algo);
int dsvgp_potrf(dsvgp_ctx* ctx, double* A, int n, int64_t lda, int* info_dev, int algo, void* workspace);
/* A.diagonal() += delta   (the jitter retries of psd_safe_cholesky)                              */
int dsvgp_add_diag(dsvgp_ctx* ctx, double* A, int n, int64_t lda, double delta);

/* ---- panel triangular solve on MFMA: TriangularLazyTensor.inv_matmul (:181,183)
 * Solves op(L) X = B for the lower-triangular fp64 L[n,n]; trans=0: op(L)=L, trans=1: op(L)=L^T.
 * B[n,nrhs] is float or double (b_is_double); X64[n,nrhs] double output (may alias B when B is
 * double); X32 optional float copy (NULL to skip); X64 may be NULL when X32 is given and nb >= n
 * (single product with the explicit inverse).  Diagonal blocks of size nb are inverted
 * (stored in the workspace) and every update is a v_mfma_f64_16x16x4 GEMM.
 * WORKSPACE SIZE: `workspace` must hold dsvgp_trsm_workspace_bytes(n, nrhs OF THIS CALL, nb) bytes, ALSO with
 * reuse_inverse=1 and ALSO when X64 is NULL: besides the inverted blocks it carries an n x nrhs double scratch that
 * a small fp32-only solve (nb >= n, fewer than 1024 output tiles) uses as the fp64 target of its split-K product.
 * The entry point has no size argument; an undersized workspace is an out-of-bounds write.                       */
size_t dsvgp_trsm_workspace_bytes(int n, int nrhs, int nb);
int dsvgp_trsm(dsvgp_ctx* ctx, const double* L, int64_t ldl, int n, int trans, const void* B,
               int64_t ldb, int b_is_double, int nrhs, double* X64, int64_t ldx64, float* X32,
               int64_t ldx32, int nb, void* workspace, int reuse_inverse);
/* The inversion phase of dsvgp_trsm alone (later solves pass reuse_inverse=1).  potrf_workspace: NULL, or
 * the workspace dsvgp_potrf(algo 1) factored THIS L with (its inverted 64x64 diagonal blocks are reused). */
int dsvgp_trtri(dsvgp_ctx* ctx, const double* L, int64_t ldl, int n, int nb, const void* potrf_workspace,
                void* workspace);
/* dsvgp_potrf(algo 1) and the inversion phase in the SAME launches (blocked Cholesky with a fused forward elimination of
 * the identity): A <- L in place, L^-1 and its transpose into `workspace` (the dsvgp_trsm workspace; later solves pass
 * reuse_inverse=1).  Only for the single-product regime nb >= n; potrf_workspace sized by
 * dsvgp_potrf_workspace_bytes(n, 1).                                                                              */
int dsvgp_potrf_inverse(dsvgp_ctx* ctx, double* A, int n, int64_t lda, int* info_dev, void* potrf_workspace, int nb,
                        void* workspace);

/* ---- generic MFMA GEMM used by the predictive / backward contractions
 *   C = alpha * op(A) op(B) + beta * Cin,   compute type = double (is_double=1) or float.
 * flags: see DSVGP_GEMM_* ; kscale (optional, length K, float) multiplies op(A)[:,k].             */
enum {
    DSVGP_GEMM_TRANS_A = 1,      /* A stored [K,M]                                             */
    DSVGP_GEMM_TRANS_B = 2,      /* B stored [N,K]                                             */
    DSVGP_GEMM_A_LOWER = 4,      /* op(A)[m,k] == 0 for k > m (masked, memory above ignored)   */
    DSVGP_GEMM_A_UPPER = 8,      /* op(A)[m,k] == 0 for k < m                                  */
    DSVGP_GEMM_B_LOWER = 16,     /* op(B)[k,n] == 0 for n > k                                  */
    DSVGP_GEMM_B_UPPER = 32,     /* op(B)[k,n] == 0 for n < k                                  */
    DSVGP_GEMM_OUT_LOWER = 64,   /* only m >= n is computed; m < n is written as 0             */
    DSVGP_GEMM_B_IS_FLOAT = 128, /* (double compute only) B is float                           */
    DSVGP_GEMM_CIN_IS_FLOAT = 256,/* (double compute only) Cin is float                        */
    DSVGP_GEMM_K_PADDED = 512,   /* (float compute) operands stored with K as their minor axis are zero-filled by the
                                    caller from K up to the next multiple of 4 (lets the LDS-DMA kernel take K % 4 != 0) */
    DSVGP_GEMM_BACKGROUND = 1024 /* filler product overlapped with a latency-bound chain on another stream: launched with one
                                    workgroup per CU, so that every CU keeps LDS room for a workgroup of the chain */
};
/* dst[M, N] (double) = src[M, N] (float): the fp64 copy of [S - I | m / (2 vbar)] that the Cholesky backward multiplies with
 * [G ; b^T] under fp64 accumulation ("Phi(L^T L-bar) without L-bar")                              */
int dsvgp_widen_f32_f64(dsvgp_ctx* ctx, const float* src, int64_t ld, double* dst, int64_t ldd, int M, int N);
int dsvgp_gemm(dsvgp_ctx* ctx, int is_double, int flags, int M, int N, int K, double alpha,
               const void* A, int64_t lda, const void* B, int64_t ldb, double beta, const void* Cin,
               int64_t ldcin, void* C, int64_t ldc, float* C32, int64_t ldc32, const float* kscale);

/* ---- ELBO terms: GaussianLikelihood.expected_log_prob / log_marginal + VariationalELBO
 * (directional_vi.py:217-219,245-246) on top of the predictive of
 * DirectionalGradVariationalStrategy.py:188-205.
 *
 * dsvgp_predictive_stats: mu[j] = sum_i A[i,j] m[i] + c ; var[j] = s*dg_j + 1e-4 + sum_i (W^2 - A^2)
 * with A = L^-1 K_ZX, W = L_S^T A, both [Mp, nb] float.                                          */
size_t dsvgp_stats_workspace_bytes(int Mp, int ncols);
int dsvgp_predictive_stats(dsvgp_ctx* ctx, const float* A, int64_t lda, const float* W, int64_t ldw,
                           int Mp, int ncols, int p, const float* m, const float* constant,
                           const float* hyp, float* mu, float* var, void* workspace);
/* dsvgp_predictive_blocks: the q x q DIAGONAL BLOCKS (q = pd + 1) of the joint predictive covariance, one per data point, without
 * K_XX and without anything of size B q x B q:
 *   blocks[b] = s K_bb + (1e-4 + (with_noise ? noise : 0)) I + W_b^T W_b - A_b^T A_b        [B, q, q] float, contiguous
 * with A = L^-1 K_ZX, W = L_S^T A, both [Mp, B q] float with interleaved columns (point b owns columns b q .. b q + pd), and the RBF
 * block at r = 0, K_bb = [[1, 0], [0, v^_a . v^_b / ell^2]] (RBFKernelDirectionalGrad.py:96-102 with x1 = x2); its diagonal is the
 * closed form of dsvgp_predictive_stats (s for the value row, s / ell^2 for a derivative row), so blocks[b][a][a] is var + noise of
 * that call up to the order of the sums.  W == NULL or W == A: zero middle term (shared directions), nothing is read from A.
 * PX: the data pack of dsvgp_pack_points made with pd directions per point ([B q, dsvgp_packed_width(d)]; only its unit direction
 * rows are read; may be NULL at pd = 0).  The Gram of every strip of max(1, 96 / q) points runs on v_mfma_f32_16x16x4_f32 over
 * row slices whose partial blocks go to `workspace` (dsvgp_predictive_blocks_workspace_bytes; 4-byte aligned) and are added in slice
 * order: no floating-point atomics, every sum in an order fixed by (Mp, B, pd) alone -- two identical calls are bitwise equal and the
 * result does not depend on the card.  The blocks are exactly symmetric.  The helper is a pure host function and returns 0 for
 * arguments the entry refuses; the entry returns DSVGP_EINVAL for a null A / blocks / hyp (PX at pd > 0), Mp < 1, B < 1, d < 1, pd
 * outside [0, 95], lda (ldw, with a W) below B q, or a workspace smaller than the helper's answer.                                 */
size_t dsvgp_predictive_blocks_workspace_bytes(int Mp, int B, int pd);
int dsvgp_predictive_blocks(dsvgp_ctx* ctx, const float* A, int64_t lda, const float* W, int64_t ldw, int Mp, int B, int pd,
                            const float* PX, int d, const float* hyp, int with_noise, float* blocks, void* workspace,
                            size_t workspace_bytes);
/* Per-point covariance roots (csrc/block_roots.hip): B blocks of q x q (q = pd + 1 in [1, 96]), such as those of
 * dsvgp_predictive_blocks, used as distributions.  One team of 8 / 16 / 32 / 64 lanes per block, the block in LDS as [q][q + 1]
 * doubles; float inputs are widened, every sum is a serial fp64 fma chain in ascending column order, the float outputs are rounded
 * once.  A block's result is a function of that block alone: no floating-point atomics, two identical calls are bitwise equal, and the
 * result of a sub-batch is bitwise the corresponding part of the whole batch's, on any card.
 * dsvgp_blocks_factor: roots[b] = lower Cholesky factor (fp64, [B, q, q] contiguous, strict upper part written as 0) of
 *   (double)blocks[b] + jitter I;  logdet[b] = 2 sum_i log roots[b][i][i];  info[b] = 0, or k + 1 when pivot k is <= 0 or not finite --
 *   a numerical outcome: roots[b] and logdet[b] are then NaN and every other block is unaffected.  *status (device int, zeroed by the
 *   call): max over info.
 * dsvgp_blocks_draw: out[i, b q + a] = mu[b q + a] + sum_{c <= a} roots[b][a][c] eps[i, b q + c], i < n (mu [B q], eps and out
 *   [n, B q] float, contiguous).
 * dsvgp_blocks_logpdf: z[b] = roots[b]^-1 (y[b] - mu[b]) ([B, q] float; z may be NULL) and
 *   logp[b] = -0.5 |z[b]|^2 - 0.5 logdet[b] - 0.5 q log(2 pi) ([B] float; |z|^2 from the unrounded z).
 * DSVGP_EINVAL for a null pointer (z excepted), q outside [1, 96], B < 0 or n < 0; B == 0 or n == 0 returns 0 without a launch.   */
int dsvgp_blocks_factor(dsvgp_ctx* ctx, const float* blocks, int B, int q, double jitter, double* roots, double* logdet, int* info,
                        int* status);
int dsvgp_blocks_draw(dsvgp_ctx* ctx, const double* roots, const float* mu, const float* eps, int B, int q, int n, float* out);
int dsvgp_blocks_logpdf(dsvgp_ctx* ctx, const double* roots, const double* logdet, const float* mu, const float* y, int B, int q,
                        float* z, float* logp);
/* per-output log-likelihood terms and their gradients.  mll_type 0 = ELBO, 1 = PLL.
 * out_scalars (device float[8]): {sum_ll, d_noise, d_constant, d_outputscale(diag part),
 *  d_lengthscale(diag part), 0,0,0}; mu_bar/var_bar are dLoss/dmu, dLoss/dvar with
 *  loss = -(sum_ll/global_rows - KL/num_data).  varn_out = clamp(var + noise) (likelihood variance). */
int dsvgp_likelihood_terms(dsvgp_ctx* ctx, const float* mu, const float* var, const float* y,
                           int ncols, int p, const float* hyp, int mll_type, double global_rows,
                           float* mu_bar, float* var_bar, float* varn_out, float* out_scalars);
/* Abar[i,j] = m[i]*mu_bar[j] + 2*var_bar[j]*(U[i,j] - A[i,j]),   U = L_S W                       */
int dsvgp_abar(dsvgp_ctx* ctx, const float* A, int64_t lda, const float* U, int64_t ldu, int Mp,
               int ncols, const float* m, const float* mu_bar, const float* var_bar, float* Abar,
               int64_t ldab);
/* d_m[i] += sum_j A[i,j]*mu_bar[j]                                                                */
int dsvgp_rowdot(dsvgp_ctx* ctx, const float* A, int64_t lda, int Mp, int ncols, const float* vec,
                 float* out_accum);
/* KL(q(u)||N(0,I)) and its gradients (gpytorch kl_mvn_mvn with the whitened prior of
 * DirectionalGradVariationalStrategy.py:77-87): kl_out (1+Mp floats): kl_out[0] = KL, rest scratch;
 * d_m += m/num_data ; d_LS(lower) += (L_S - diag(1/L_S_ii))/num_data ; d_LS(upper) = 0.          */
int dsvgp_kl_terms(dsvgp_ctx* ctx, const float* m, const float* LS, int64_t ldls, int Mp,
                   double num_data, float* kl_out, float* d_m, float* d_LS, int64_t lddls);
/* Cholesky backward helper: S = Phi(G) + Phi(G)^T from the lower triangle of G (in place).        */
int dsvgp_phi_symmetrize(dsvgp_ctx* ctx, double* G, int n, int64_t ldg);
/* out[cols, rows] = in[rows, cols]^T (out of place)                                              */
int dsvgp_transpose_f64(dsvgp_ctx* ctx, const double* in, int64_t ldi, int rows, int cols, double* out,
                        int64_t ldo);
int dsvgp_transpose_f32(dsvgp_ctx* ctx, const float* in, int64_t ldi, int rows, int cols, float* out,
                        int64_t ldo);
/* fp64 matrix-vector product on a row-major M x N matrix: trans = 0: y[M] = A x[N];  trans = 1: y[N] = A^T x[M] (sums meet in
 * fp64 atomics: run-order rounding).  The float64 model mode's predictive mean A^T m and b = A mu-bar
 * (DirectionalGradVariationalStrategy.py:181-183 under torch.set_default_dtype(torch.float64), experiments/synthetic/exp_script.py:56). */
int dsvgp_gemv_f64(dsvgp_ctx* ctx, int trans, const double* A, int64_t lda, int M, int N, const double* x, double* y);

/* ---- ELBO-mode fast path.  With mll_type == ELBO, dLoss/dvar_j = 1/(2 noise rows) is the same for every
 * output, so the data term only needs  sum_j (y_j - mu_j)^2  and  sum_j var_j = prior + |L_S^T A|_F^2 - |A|_F^2,
 * i.e. the M' x M' Gram matrix G = A A^T instead of W = L_S^T A, U = L_S W and the [M', B'] fp64 products of the
 * backward (same quantities as DirectionalGradVariationalStrategy.py:188-205 + directional_vi.py:245-246).
 * sums (device float[4]) = { sum r^2, sum mu_bar, sum_{i>=j} L_S_ij (G L_S)_ij, trace G }.                    */
int dsvgp_residual_terms(dsvgp_ctx* ctx, const float* mu, const float* y, int ncols, const float* hyp,
                         double global_rows, float* mu_bar, float* sums);          /* zeroes sums first  */
int dsvgp_trace_terms(dsvgp_ctx* ctx, const float* LS, int64_t ldls, const float* T1, int64_t ldt,
                      const float* G, int64_t ldg, int n, float t1_scale,          /* T1 = t1_scale * given */
                      float* sums);                                                /* adds to sums[2..3] */
/* out_scalars: same layout as dsvgp_likelihood_terms                                                    */
int dsvgp_elbo_fast_finalize(dsvgp_ctx* ctx, const float* sums, const float* hyp, int npts, int p,
                             double global_rows, float* out_scalars);
/* copy the lower triangle of the float matrix onto its upper triangle (symmetrise a tril GEMM result)   */
int dsvgp_mirror_lower_f32(dsvgp_ctx* ctx, float* G, int n, int64_t ldg);
int dsvgp_add_diag_f32(dsvgp_ctx* ctx, float* A, int n, int64_t lda, float delta);
/* A[n, n + 1] (lda >= n + 1): A[i][i] -= 1, A[i][n] = m[i] * noise * rows -- [S - I | m / (2 vbar)], the right-hand side of the
 * [Q' | a] solve of the ELBO fast path (DGVS.py:192-205: the (S - I) middle term and the mean term) in one pass            */
int dsvgp_sminus_i_col(dsvgp_ctx* ctx, float* A, int n, int64_t lda, const float* m, const float* hyp, double rows);

/* ---- data-parallel all-reduce operand (the reference is single-process and has no counterpart):
 * dst = [ packed lower triangle of src[n,n] (row i at offset i(i+1)/2) | extra[nextra] ], i.e. n(n+1)/2 + nextra floats
 * instead of n*n + nextra ([tril(G) ; b^T] or [tril(L_S-bar) ; m-bar]: 18 MB instead of 36 MB at M' = 3000).
 * dsvgp_tril_unpack_f32 writes the lower triangle of dst (the strict upper part is left untouched) and extra back.  */
int dsvgp_tril_pack_f32(dsvgp_ctx* ctx, const float* src, int64_t ld, int n, const float* extra, int nextra,
                        float* dst);
int dsvgp_tril_unpack_f32(dsvgp_ctx* ctx, const float* src, int n, float* dst, int64_t ld, float* extra, int nextra);

/* ---- minibatch gather: DataLoader batch + select_cols_of_y (directional_vi.py:68-90,229-241)
 * xb[b,:] = X[idx[b],:] ; yb[b*(p+1)+c] = Y[idx[b], cols[c]]  (cols[0] == 0); with E[d, d] != NULL also the batch's
 * derivative directions Db[(b p + a), :] = E[cols[a+1] - 1, :]  (derivative_directions.repeat(n_samples, 1), :238)  */
int dsvgp_gather_batch(dsvgp_ctx* ctx, const float* X, const float* Y, const int64_t* idx, int nb,
                       int d, int ycols, const int* cols, int p, float* xb, float* yb, const float* E, float* Db);

/* ---- fused Adam (torch.optim.Adam semantics, directional_vi.py:193-199,251-254)
 * lr_dev / step_dev are device scalars so the update is graph-capturable.                         */
int dsvgp_adam_step(dsvgp_ctx* ctx, float* param, const float* grad, float* exp_avg,
                    float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2, float eps,
                    int step);

/* the same update for up to DSVGP_ADAM_MAX_TENSORS tensors that share (lr, betas, eps, step) in ONE launch: the parameter
 * groups of one torch.optim.Adam (directional_vi.py:193-199); the arrays are HOST arrays of device pointers / element counts
 * (round 6) sizes[k] = -n names an n x n row-major matrix of which only the LOWER TRIANGLE is a parameter (chol_variational_covar: the
 * reference masks the rest in its forward -- variational_strategy / CholeskyVariationalDistribution -- so gradient, both moments and the
 * update are exactly zero there): the strict upper triangle is then not read or written (dsvgp_adam_step_multi only).             */
#define DSVGP_ADAM_MAX_TENSORS 16
int dsvgp_adam_step_multi(dsvgp_ctx* ctx, int count, float* const* params, const float* const* grads,
                          float* const* exp_avgs, float* const* exp_avg_sqs, const int64_t* sizes, float lr,
                          float beta1, float beta2, float eps, int step);
/* the same update for the float64 model mode (parameters, gradients and moments in double) */
/* dsvgp_adam_step_multi skipped ON THE DEVICE while *guard_dev != 0 (round 6): guard_dev = the status word of the one-call step that made the
 * gradients (dsvgp_elbo_step_locate, which = 5): a host that queues the update without waiting for the factorisation's status leaves the
 * parameters untouched when it failed, reads the status later (dsvgp_elbo_step_status) and repeats the step through the jitter ladder. */
int dsvgp_adam_step_multi_guarded(dsvgp_ctx* ctx, int count, float* const* params, const float* const* grads,
                                  float* const* exp_avgs, float* const* exp_avg_sqs, const int64_t* sizes, float lr,
                                  float beta1, float beta2, float eps, int step, const int* guard_dev);
int dsvgp_adam_step_multi_f64(dsvgp_ctx* ctx, int count, double* const* params, const double* const* grads,
                              double* const* exp_avgs, double* const* exp_avg_sqs, const int64_t* sizes, double lr,
                              double beta1, double beta2, double eps, int step);

/* ---- graph-capturable variants (HIP-graph replay of the steady-state step: every per-step scalar lives in device memory)
 * dsvgp_adam_step_multi_dev: dsvgp_adam_step_multi with {lr, step} read from the device float[2] lr_step_dev (the host
 *   refreshes it through a captured copy; directional_vi.py:251-254 steps the LR schedulers every iteration) and an optional
 *   guard: while *guard_dev != 0 (the potrf status word) nothing is updated.
 * dsvgp_scale_by_vbar: x_k *= 1 / (noise * global_rows) (= 2 dLoss/dvar of the ELBO) for up to three arrays.
 * dsvgp_kl_terms_scaled: dsvgp_kl_terms with d_LS(lower) first multiplied by 1 / (noise * global_rows); add_kl = 0 leaves the
 *   KL value and gradients out (kl_out[0] = 0).                                                                          */
int dsvgp_adam_step_multi_dev(dsvgp_ctx* ctx, int count, float* const* params, const float* const* grads,
                              float* const* exp_avgs, float* const* exp_avg_sqs, const int64_t* sizes,
                              const float* lr_step_dev, float beta1, float beta2, float eps, const int* guard_dev);
int dsvgp_scale_by_vbar(dsvgp_ctx* ctx, float* x0, int64_t n0, float* x1, int64_t n1, float* x2, int64_t n2,
                        const float* hyp, double global_rows);
int dsvgp_kl_terms_scaled(dsvgp_ctx* ctx, const float* m, const float* LS, int64_t ldls, int Mp, double num_data, int add_kl,
                          const float* hyp, double global_rows, float* kl_out, float* d_m, float* d_LS, int64_t lddls);
/* The variational block of the ELBO fast path in ONE pass over (L_S, T = tril(G L_S)) (round 3; replaces the sequence
 * dsvgp_trace_terms + dsvgp_kl_terms[_scaled] on the hot path): sums[2] = t1_scale * sum_{i>=j} L_S,ij T_ij, sums[3] = trace(G),
 * d_LS <- [T / (noise rows) when flags & 1] + [dKL/dL_S / num_data when flags & 2], d_m += m / num_data (flags & 2),
 * kl_out[0] = KL (0 without flag 2).  kl_out: 1 + 2 Mp floats.  One wave per row, 16-byte accesses, no atomics: the per-row
 * partial sums are added in a fixed order (bitwise reproducible).  Reference: gpytorch kl_divergence of the whitened prior
 * (DGVS.py:77-87) + the trace terms of the expected log-likelihood (directional_vi.py:217,245).                            */
int dsvgp_variational_terms(dsvgp_ctx* ctx, const float* m, const float* LS, int64_t ldls, int Mp, double num_data,
                            int flags, const float* hyp, double global_rows, const float* G, int64_t ldg,
                            float t1_scale, float* kl_out, float* sums, float* d_m, float* d_LS, int64_t lddls);

/* ---- fp32-equivalent products on the bf16 matrix pipe (round 4, OPT-IN; the default step computes in fp32 MFMA).  An fp32 operand
 * is cut once into three bf16 planes x = h + m + l (dsvgp_split3_bf16; remainder < 2^-26 |x|) and a product keeps the six terms
 * down to 2^-16 of (h + m + l)(h' + m' + l') on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (csrc/gemm3b.hip).
 *   planes of a [rows_out, K] operand: 3 x rows_out x dsvgp_split3_kpad(K) bf16, plane after plane (dsvgp_split3_bytes), 16-byte
 *   aligned; transpose = 1 splits the TRANSPOSE of src[R, Cc] (rows_out = Cc, K = R): both operands of dsvgp_gemm3b are
 *   k-contiguous.   dsvgp_gemm3b: C[M, N] = alpha A B^T, flags 0 or DSVGP_GEMM_OUT_LOWER.              */
int dsvgp_split3_kpad(int K);
size_t dsvgp_split3_bytes(int rows_out, int K);
int dsvgp_split3_bf16(dsvgp_ctx* ctx, const float* src, int64_t ld, int R, int Cc, int transpose, void* planes);
int dsvgp_gemm3b(dsvgp_ctx* ctx, int flags, int M, int N, int K, float alpha, const void* Aplanes, int a_rows, const void* Bplanes,
                 int b_rows, float* C, int64_t ldc);

/* Plain dense fp32 GEMM through rocBLAS (row-major, flags: DSVGP_GEMM_TRANS_A / _TRANS_B only): for products without
 * structure or fused epilogue (the dense K_ZX-bar product of the ELBO fast path); everything else is dsvgp_gemm.      */
int dsvgp_gemm_lib_f32(dsvgp_ctx* ctx, int flags, int M, int N, int K, float alpha, const float* A, int64_t lda,
                       const float* B, int64_t ldb, float beta, float* C, int64_t ldc);

/* ---- contour-integral-quadrature whitening: lazify(K_ZZ).sqrt_inv_matmul(K_ZX)
 * (directionalvi/CiqDirectionalGradVariationalStrategy.py:255-256; quadrature + msMINRES of gpytorch 1.4.0
 * utils/contour_integral_quad.py, utils/minres.py).  Layout: one right-hand side per ROW, R[t, n], K[n, n] symmetric.
 * dsvgp_ciq_lanczos: `iters` Lanczos steps from v0 -> alpha[iters], beta[iters] (host takes the Ritz values of the
 *   tridiagonal as eigenvalue bounds, max_lanczos_iter = 20).  workspace: 3 n + 2 floats.
 * dsvgp_ciq_solve: out[t, n] = sum_q omega_q (K + sigma_q I)^-1 R for all shifts from one Lanczos process per row; stops
 *   when the mean of |update| / |solution| over (shift, row) < tol, tested every `check_every` iterations (gpytorch: tol 1e-4,
 *   every 10, at most 1000).  Basis-resident msMINRES: basis[cap + 1][t][n] receives the Lanczos rows q_0 .. q_J, the
 *   per-shift solutions are not stored but left as coefficients, x_q[row] = rnorm[row] sum_j ycoef[row][j][q] q_j[row]
 *   (ycoef[t][cap][QP], QP = Q rounded up to a multiple of 4); DSVGP_ENOSPACE when J would exceed cap.
 *   workspace: dsvgp_ciq_workspace_bytes(Q, t, n, cap).
 * dsvgp_ciq_mix: out[k][row][:] = rowscale[row] sum_{j<J} C[row][j][k] basis[j][row][:], k < Kout (C[t][ldj][KP], KP % 4 == 0):
 *   materialises solves (C = ycoef) or any per-row combination of them.
 * dsvgp_ciq_cross: C[t][Jb][KPa] = rn_a rn_b sum_q omega_q ya[.][ia][q] yb[.][jb][q] (KPa = Ja rounded up to 4): with it the
 *   backward's sum_q omega_q A_q^T B_q = stack_ia(basisA)^T stack_ia(mix(basisB, C)) is ONE product of depth Ja t instead of Q
 *   products of depth t (gpytorch's sqrt_inv_matmul backward, utils/contour_integral_quad.py + functions/_sqrt_inv_matmul.py).
 * dsvgp_ciq_rowstats / dsvgp_ciq_tbar: the mean / variance interpolation terms of _NgdInterpTerms (:65-69,265-266)
 *   and the gradient factors of its backward (:94-118) for rows of T = (K^-1/2 K_ZX)^T and ST = T S.
 * dsvgp_sym_average_f32: out = (A + A^T) / 2.                                                                  */
size_t dsvgp_ciq_workspace_bytes(int Q, int t, int n, int cap);
int dsvgp_ciq_lanczos(dsvgp_ctx* ctx, const float* K, int64_t ldk, const float* v0, int n, int iters, float* alpha,
                      float* beta, void* workspace);
int dsvgp_ciq_solve(dsvgp_ctx* ctx, const float* K, int64_t ldk, const float* R, int64_t ldr, int t, int n,
                    const float* sigma, const float* omega, int Q, float tol, int max_iter, int check_every, float* basis,
                    int cap, float* ycoef, float* rnorm, float* out, int64_t ldo, void* workspace, int* iters_out);
int dsvgp_ciq_mix(dsvgp_ctx* ctx, const float* basis, int J, int t, int n, const float* C, int ldj, int KP, int Kout,
                  const float* rowscale, float* out, int64_t ldo);
int dsvgp_ciq_cross(dsvgp_ctx* ctx, const float* ya, int Ja, int lda, const float* yb, int Jb, int ldb, const float* omega,
                    int Q, int t, const float* rn_a, const float* rn_b, float* Cout);
int dsvgp_ciq_rowstats(dsvgp_ctx* ctx, const float* T, const float* ST, int t, int n, int p, const float* m,
                       const float* constant, const float* hyp, float kxx_jitter, float* imean, float* mu, float* var,
                       float* live);   /* kxx_jitter: 0 for the directional strategy (:235-239), 1e-4 for gpytorch's plain
                                          CiqVariationalStrategy (its forward is quoted at :243-251)                    */
int dsvgp_ciq_tbar(dsvgp_ctx* ctx, const float* T, const float* ST, int t, int n, const float* m, const float* mu_bar,
                   const float* var_bar, const float* live, const float* imean, float* Tbar, float* VT, float* cvec);
int dsvgp_sym_average_f32(dsvgp_ctx* ctx, const float* A, int n, int64_t lda, float* out, int64_t ldo);
/* The same entry points in double precision, for a model built under torch.set_default_dtype(torch.float64) with
 * use_ciq=True (reference experiments/bunny/exp_bunny.py:66,78): every array is double, the arithmetic is the float64
 * msMINRES of gpytorch run on a float64 LazyTensor; workspace of dsvgp_ciq_lanczos_f64: 3 n + 2 doubles.            */
size_t dsvgp_ciq_workspace_bytes_f64(int Q, int t, int n, int cap);
int dsvgp_ciq_lanczos_f64(dsvgp_ctx* ctx, const double* K, int64_t ldk, const double* v0, int n, int iters, double* alpha,
                          double* beta, void* workspace);
int dsvgp_ciq_solve_f64(dsvgp_ctx* ctx, const double* K, int64_t ldk, const double* R, int64_t ldr, int t, int n,
                        const double* sigma, const double* omega, int Q, double tol, int max_iter, int check_every,
                        double* basis, int cap, double* ycoef, double* rnorm, double* out, int64_t ldo, void* workspace,
                        int* iters_out);
int dsvgp_ciq_mix_f64(dsvgp_ctx* ctx, const double* basis, int J, int t, int n, const double* C, int ldj, int KP, int Kout,
                      const double* rowscale, double* out, int64_t ldo);
int dsvgp_ciq_cross_f64(dsvgp_ctx* ctx, const double* ya, int Ja, int lda, const double* yb, int Jb, int ldb,
                        const double* omega, int Q, int t, const double* rn_a, const double* rn_b, double* Cout);
int dsvgp_ciq_rowstats_f64(dsvgp_ctx* ctx, const double* T, const double* ST, int t, int n, int p, const double* m,
                           const double* constant, const double* hyp, double kxx_jitter, double* imean, double* mu,
                           double* var, double* live);
int dsvgp_ciq_tbar_f64(dsvgp_ctx* ctx, const double* T, const double* ST, int t, int n, const double* m, const double* mu_bar,
                       const double* var_bar, const double* live, const double* imean, double* Tbar, double* VT,
                       double* cvec);
int dsvgp_sym_average_f64(dsvgp_ctx* ctx, const double* A, int n, int64_t lda, double* out, int64_t ldo);

/* ---- the whole ELBO step from ONE host call (round 3; csrc/step.hip)
 * dsvgp_elbo_step_f32 queues forward + backward of one minibatch ELBO evaluation -- `output = model(x, derivative_directions=D);
 * loss = -mll(output, y); loss.backward()` of the reference's train_gp (directionalvi/directional_vi.py:245-249) with the
 * composition of DirectionalGradVariationalStrategy.forward (DGVS.py:89-208) -- as ~70 launches on two HIP streams, without a
 * host synchronisation: the ELBO fast path (Gram formulation) of the Cholesky-whitened strategy, every data
 * point with its p directional derivatives, explicit-inverse regime (M(p+1) <= 8192).
 *   plan       host object for one (M, d, p, B): workspace layout, the second stream, events, pinned status word
 *   workspace  caller-owned device memory of dsvgp_elbo_step_workspace_bytes(M, d, p, B) bytes, 256-byte aligned, kept between steps
 *              and used by THIS plan only (the plan clears the zero padding of one operand once per workspace address; pass
 *              flag 8 whenever anything else may have written to the buffer since this plan's last step)
 *   io         device pointers (below); io->flat[0 .. flat_floats) is cleared by the call and must contain every gradient slot
 *   flags      1: overlap on the plan's second stream; 2: include the KL term (data-parallel ranks > 0 leave it out); 4: record
 *              HIP-event timings (dsvgp_elbo_step_timings); 8: the workspace contents are undefined (re-clear the paddings);
 *              16 (with 1): the Cholesky backward on the second stream under the dense K_ZX-bar product (probe: no gain);
 *              32: the two big fp32 products as bf16 x 3 split products (io->split_ws; opt-in, see dsvgp_split3_bf16);
 *              64: tril(L^T L-bar) = -tril([S - I | m'][G ; b^T]) with fp64 accumulation (default: both operands are fp32 data, the
 *              product runs on the fp32 MFMA kernel and its result is widened for the fp64 Cholesky backward)
 * Gradients are those of loss = -(sum_j ll_j / global_rows - KL / num_data); a factorisation that fails leaves NaNs in the
 * outputs and a non-zero status word: read it with dsvgp_elbo_step_status (waits for the factorisation only, not for the step)
 * and run the jitter ladder on the piecewise path.  Threading: one host thread per context.                                  */
typedef struct dsvgp_step_plan dsvgp_step_plan;
typedef struct dsvgp_elbo_step_io {
    /* parameters (float32, device): inducing points [M,d], directions [M p,d], q(u) mean [M'], Cholesky factor [M',M'] (lower
     * triangle read), constant mean [1], raw hyper-parameters [1] each                                                       */
    const float *Z, *V, *m, *LS; int64_t ldls;
    const float *constant, *raw_lengthscale, *raw_outputscale, *raw_noise;
    /* minibatch: x [B,d], interleaved targets y [B(p+1)], derivative directions D [B p, d]                                    */
    const float *x, *y, *D;
    /* outputs: the flat gradient buffer (cleared here) and the slots inside it; d_hyp[4] is scratch inside flat as well       */
    float* flat; size_t flat_floats;
    float *dZ, *dV, *dm, *dLS; int64_t lddls;
    float *d_hyp, *d_constant, *d_raw_lengthscale, *d_raw_outputscale, *d_raw_noise, *loss;
    float* mu;                       /* [B(p+1)] predictive mean of q(f) at the batch (constant mean included)                  */
    double num_data, global_rows;    /* VariationalELBO num_data ((d+1) N); B'(global) of the minibatch                          */
    float kzz_jitter;                /* LazyTensor.add_jitter() default 1e-3 (DGVS.py:144)                                      */
    /* flag 32 (opt-in): scratch of dsvgp_elbo_step_split_bytes(M, d, p, B) bytes for the bf16 plane triples of [A ; mu_bar^T],
     * its transpose and [Q' | a] -- the Gram product and the dense K_ZX-bar product then run on the bf16 matrix pipe as six
     * bf16 products per fp32 product (csrc/gemm3b.hip); NULL / flag clear: v_mfma_f32_32x32x2_f32 (the default)                */
    void* split_ws; size_t split_ws_bytes;
    /* optional (NULL: not stated): the minibatch's derivative directions as an INDEX LIST.  The reference's training step builds D as
     * E_canonical[idx - 1] tiled over the minibatch (directional_vi.py:81-88, 238: the same p coordinates for every point), its
     * evaluation as eye(d)[:p] tiled (:292-294).  dir_idx [p] (device, int32): row j p + b of D is e_{dir_idx[b] - dir_idx_base}
     * for every point j -- the caller's statement about D (which is still read: the packed rows).  K_ZX and its backward then run
     * on the canonical-direction kernels (dsvgp_kernel_fwd_canon / _bwd_canon) where those take the geometry (p + 1 in {3, 6},
     * d <= 28), on the general ones otherwise.  Appended in round 6: callers that zero-initialise the struct keep the old meaning. */
    const int* dir_idx; int dir_idx_base;
    /* non-zero: the inducing directions V are the SAME unit vectors (row m p + a of V is e_{dir_idx[a] - dir_idx_base} for every
     * inducing point m) and are not parameters -- the full-gradient SVGP (reference GradVariationalStrategy.py:89-99).  K_ZZ, K_ZX
     * and their backwards then run on dsvgp_kernel_fwd_canon2 / _bwd_canon2 where those take the geometry; dV is left zero.        */
    int v_one_hot;
} dsvgp_elbo_step_io;
size_t dsvgp_elbo_step_split_bytes(int M, int d, int p, int B);
size_t dsvgp_elbo_step_workspace_bytes(int M, int d, int p, int B);
int dsvgp_elbo_step_plan_create(dsvgp_ctx* ctx, int M, int d, int p, int B, dsvgp_step_plan** out);
int dsvgp_elbo_step_plan_destroy(dsvgp_step_plan* plan);
size_t dsvgp_elbo_step_plan_bytes(const dsvgp_step_plan* plan);
/* Which of its clearing regimes the step queued last on this plan used for its split-K / OUT_LOWER targets: 0 every launcher cleared
 * its own target; 1 one memset over the whole arena at the start of the step (small problems); 2 the targets of the later products
 * were cleared on the second stream at the start of the step (large problems with flag 1), + 4 when the Gram product's target
 * was among them.  Read-only; 0 before the first step and after a per-output or data-parallel step.                            */
int dsvgp_elbo_step_clear_mode(const dsvgp_step_plan* plan);
int dsvgp_elbo_step_f32(dsvgp_ctx* ctx, dsvgp_step_plan* plan, const dsvgp_elbo_step_io* io, void* workspace,
                        size_t workspace_bytes, int flags);
int dsvgp_elbo_step_status(dsvgp_step_plan* plan, float* hyp4, int* info);
/* The PER-OUTPUT step from one host call (round 5): objectives that read every output's own predictive variance -- mll_type = "PLL"
 * (PredictiveLogLikelihood, reference directionalvi/directional_vi.py:218-219; what tests/test_grad_svgp.py:19-36 trains with) or the
 * ELBO with the per-output variances returned -- for which the Gram formulation of dsvgp_elbo_step_f32 does not apply: forward
 * A = L^-1 K_ZX, W = L_S^T A, mu / var per output (DGVS.py:181-205), likelihood terms, and the backward through U = L_S W,
 * A-bar, K_ZX-bar = L^-T A-bar, L-bar = -tril(K_ZX-bar A^T), the Cholesky factor and both kernel assemblies.  Same io as above;
 * plan from dsvgp_elbo_step_po_plan_create, workspace of dsvgp_elbo_step_po_workspace_bytes; varn [B(p+1)] (device) receives
 * var + noise per output (what likelihood(model(x)).variance returns).  flags: bit 0 overlap, bit 1 include the KL term,
 * bit 8 (256) PLL objective (clear: ELBO).  Status word / jitter ladder as for dsvgp_elbo_step_f32.                            */
size_t dsvgp_elbo_step_po_workspace_bytes(int M, int d, int p, int B);
int dsvgp_elbo_step_po_plan_create(dsvgp_ctx* ctx, int M, int d, int p, int B, dsvgp_step_plan** out);
int dsvgp_elbo_step_po_f32(dsvgp_ctx* ctx, dsvgp_step_plan* plan, const dsvgp_elbo_step_io* io, float* varn, void* workspace,
                           size_t workspace_bytes, int flags);
/* Where an intermediate of the step queued last lies inside the caller's workspace (valid until the next step on it): which = 0:
 * [A ; mu_bar^T], A = L^-1 K_ZX (float [M'+1, B']); 1: K_ZX (float [M', B']); 2: the Cholesky factor L (double [M', M'], lower);
 * 3: L^-1 (double [M', M'], lower); 4: the constrained {lengthscale, outputscale, noise, 0} (float [1, 4]); 5: the factorisation's status word
 * (int32 [1], 0 = positive definite; valid from the step's factorisation until the next step on the workspace clears it).  The reference's every-50th-step nll print (directional_vi.py:255-260) reads the predictive
 * variance of the function-value rows of the forward pass it has just differentiated: W = L_S^T A[:, ::p+1] is all it takes.  */
int dsvgp_elbo_step_locate(const dsvgp_step_plan* plan, int which, size_t* offset_bytes, int* rows, int* cols, int64_t* ld);
/* ---- one RANK of a data-parallel job (the reference is single-process): the same step in five pieces with
 * the caller's collectives (RCCL through whatever binding the host uses) between them -- global-Gram schedule: the ranks sum
 * [tril(G) | b] instead of the L_S gradient, every rank forms the identical L_S-bar / m-bar itself, the replicated M'^3 stage
 * is sharded (columns of [Q' | a], rows of L-bar, column blocks of K_ZZ-bar) and met again by two all-gathers.
 *   plan      dsvgp_elbo_step_dp_plan_create(M, d, p, B = THIS RANK's rows, world); workspace of dsvgp_elbo_step_dp_workspace_bytes
 *   io        as above with global_rows = B'(global); io->flat is cleared in phase 0
 *   dp        rank / world and the collective operands (caller-owned device memory, float):
 *               wire       [wire_floats >= M'(M'+1)/2 + M'] packed [tril(G) | b]; anything beyond that count is the caller's
 *                          padding (keep it zero)             phase 0 writes it -> ALL-REDUCE(sum) -> phase 2 reads it
 *               q_local    [M', wq], wq = roundup4(ceil((M'+1)/world)), ZERO-INITIALISED once (the pad columns stay zero)
 *                                                              phase 1 writes it -> ALL-GATHER -> q_all [world, M', wq], phase 3 reads
 *               lbar_local [wr, M'], wr = roundup2(ceil(M'/world)), zero-initialised once
 *                                                              phase 2 writes it -> ALL-GATHER -> lbar_all [world wr, M'], phase 4 reads
 *   phase     0 .. 4 in this order, all on the context's stream (the collectives must be ordered against it by the caller);
 *             after phase 4: ALL-REDUCE(sum) of the slots of io->flat that hold Z-bar, V-bar, the hyper-parameter gradients and
 *             the loss; m-bar and L_S-bar are final and identical on every rank after phase 2 / 4 (do not reduce them).
 *   flags     as dsvgp_elbo_step_f32; bit 1 (value 2) on exactly ONE rank (it counts the KL value and the trace terms of the
 *             global Gram matrix; every rank adds the KL gradient).  Status word as above (dsvgp_elbo_step_status after phase 0).  */
typedef struct dsvgp_elbo_step_dp {
    int rank, world;
    float* wire; size_t wire_floats;
    float* q_local; const float* q_all;
    float* lbar_local; const float* lbar_all;
} dsvgp_elbo_step_dp;
size_t dsvgp_elbo_step_dp_workspace_bytes(int M, int d, int p, int B, int world);
int dsvgp_elbo_step_dp_plan_create(dsvgp_ctx* ctx, int M, int d, int p, int B, int world, dsvgp_step_plan** out);
int dsvgp_elbo_step_dp_f32(dsvgp_ctx* ctx, dsvgp_step_plan* plan, const dsvgp_elbo_step_io* io, const dsvgp_elbo_step_dp* dp,
                           void* workspace, size_t workspace_bytes, int flags, int phase);
/* flags & 4 in dsvgp_elbo_step_f32: HIP-event pairs around the forward solve, the K_ZX assembly and K_ZX-bar's kernel backward,
 * each on the stream its kernel runs on; ms3 = their durations in ms (waits for the step) -- bench.py's roofline entries      */
int dsvgp_elbo_step_timings(dsvgp_step_plan* plan, int steps_back, float* ms3);   /* the plan keeps the last 128 timed steps */
/* the same three durations plus ms5[3]: the Gram product [tril(G) ; b^T] = tril([A ; mu_bar^T] A^T) and ms5[4]: the dense product
 * K_ZX-bar = [Q' | a][A ; mu_bar^T] (the two fp32 [M', B'] products of the step; no counterpart in the reference, whose autograd runs
 * them inside DGVS.py:192-205's backward) */
int dsvgp_elbo_step_timings5(dsvgp_step_plan* plan, int steps_back, float* ms5);
long dsvgp_elbo_step_timed_count(const dsvgp_step_plan* plan);   /* steps queued with flag 4 so far (index of the last: count - 1) */

/* ---- the whole ELBO step of the FLOAT64 model mode from one host call (csrc/step64.hip) -- the reference's experiment scripts run
 * under torch.set_default_dtype(torch.float64) (experiments/synthetic/exp_script.py:56): parameters, minibatch, kernel matrices, the
 * whitening solve and the ELBO all in double.  dsvgp_elbo_step_f64 queues forward + backward of one minibatch ELBO evaluation
 * (directionalvi/directional_vi.py:245-249 with DirectionalGradVariationalStrategy.forward, DGVS.py:89-208) without a host read, a
 * host synchronisation or a device allocation: Gram formulation of the ELBO, Cholesky variational distribution, Cholesky whitening,
 * every data point with its p directional derivatives, one rank, explicit-inverse regime M(p+1) <= 8192, any d >= 1, 0 <= p <= 95
 * (p <= 16: register assembly of csrc/assemble64.hip, its T scratch in the workspace; more directions: csrc/assemble64_tiled.hip).
 *   io         device pointers, all double.  THE CALLER ZEROES THE STRUCT (memset / = {0}) and sets struct_size = sizeof(struct):
 *              fields appended in later versions are read only when struct_size covers them, and an older caller's zeroed struct
 *              keeps its meaning.  io->flat[0 .. flat_doubles) is cleared by the call and must contain every gradient slot, the
 *              loss and d_hyp[4].  There are no dir_idx fields: the fp64 assembly has no canonical-direction kernels.
 *   plan       host object of one (M, d, p, B): workspace layout, second stream, events, pinned status word
 *   workspace  caller-owned device memory of dsvgp_elbo_step_f64_workspace_bytes(M, d, p, B) bytes, 256-byte aligned
 *   flags      1: second stream (K_ZX's assembly and S = L_S L_S^T under the Cholesky chain); 2: include the KL term; 4: record
 *              HIP-event timings (dsvgp_elbo_step_f64_timings); 8: the workspace contents are undefined (accepted for symmetry
 *              with dsvgp_elbo_step_f32: this step keeps nothing in the workspace between calls)
 * Under dsvgp_set_deterministic (scratch of dsvgp_deterministic_f64_scratch_bytes(M, d, p, B)) every sum of the step is formed in a
 * fixed order -- losses and gradients are bitwise equal run to run -- and flag 1 is ignored: the scratch serves one stream.
 * Gradients are those of loss = -(sum_j ll_j / global_rows - KL / num_data).  A factorisation that fails leaves NaNs in the outputs
 * and a non-zero status word: dsvgp_elbo_step_f64_status waits for the factorisation only and returns it (and the constrained
 * hyper-parameters); the caller then runs psd_safe_cholesky's jitter ladder on the piecewise entry points.
 * dsvgp_elbo_step_f64_supported: 1 when the call takes (M, d, p, B), 0 otherwise (then _workspace_bytes is 0 as well); both are
 * pure host functions.  dsvgp_elbo_step_f64_timings: ms5 = HIP-event durations (ms) of the step queued with flag 4 `steps_back`
 * timed steps before the last one (the plan keeps 128): forward solve A = L^-1 K_ZX, K_ZX assembly, K_ZX-bar kernel backward, Gram
 * product, dense K_ZX-bar product; waits for that step.                                                                         */
typedef struct dsvgp_step_plan_f64 dsvgp_step_plan_f64;
typedef struct dsvgp_elbo_step_io_f64 {
    size_t struct_size;              /* sizeof(dsvgp_elbo_step_io_f64) of the CALLER's header                                    */
    /* parameters: inducing points [M,d], directions [M p,d], q(u) mean [M'], Cholesky factor [M',M'] (lower triangle read),
     * constant mean [1], raw hyper-parameters [1] each                                                                          */
    const double *Z, *V, *m, *LS; int64_t ldls;
    const double *constant, *raw_lengthscale, *raw_outputscale, *raw_noise;
    /* minibatch: x [B,d], interleaved targets y [B(p+1)], derivative directions D [B p, d]                                       */
    const double *x, *y, *D;
    /* outputs: the flat gradient buffer (cleared here) and the slots inside it                                                   */
    double* flat; size_t flat_doubles;
    double *dZ, *dV, *dm, *dLS; int64_t lddls;
    double *d_hyp, *d_constant, *d_raw_lengthscale, *d_raw_outputscale, *d_raw_noise, *loss;
    double* mu;                      /* [B(p+1)] predictive mean of q(f) at the batch (constant mean included); not inside flat  */
    double num_data, global_rows;    /* VariationalELBO num_data ((d+1) N); B'(global) of the minibatch                          */
    double kzz_jitter;               /* LazyTensor.add_jitter() default 1e-3 (DGVS.py:144)                                      */
} dsvgp_elbo_step_io_f64;
int dsvgp_elbo_step_f64_supported(int M, int d, int p, int B);
size_t dsvgp_elbo_step_f64_workspace_bytes(int M, int d, int p, int B);
int dsvgp_elbo_step_f64_plan_create(dsvgp_ctx* ctx, int M, int d, int p, int B, dsvgp_step_plan_f64** out);
int dsvgp_elbo_step_f64_plan_destroy(dsvgp_step_plan_f64* plan);
int dsvgp_elbo_step_f64(dsvgp_ctx* ctx, dsvgp_step_plan_f64* plan, const dsvgp_elbo_step_io_f64* io, void* workspace,
                        size_t workspace_bytes, int flags);
int dsvgp_elbo_step_f64_status(dsvgp_step_plan_f64* plan, double* hyp4, int* info);
int dsvgp_elbo_step_f64_timings(dsvgp_step_plan_f64* plan, int steps_back, float* ms5);
long dsvgp_elbo_step_f64_timed_count(const dsvgp_step_plan_f64* plan);
/* minibatch gather of the float64 model mode (dsvgp_gather_batch in double): xb[b,:] = X[idx[b],:], yb[b(p+1)+c] = Y[idx[b], cols[c]],
 * and with E[d,d] != NULL the tiled one-hot directions Db[(b p + a), :] = E[cols[a+1] - 1, :]                                   */
int dsvgp_gather_batch_f64(dsvgp_ctx* ctx, const double* X, const double* Y, const int64_t* idx, int nb, int d, int ycols,
                           const int* cols, int p, double* xb, double* yb, const double* E, double* Db);

/* ---- posterior mean of a frozen model (csrc/predict_mean.hip): mean and gradient without K_ZX or a solve.
 * What the reference's mean-only callers read from `likelihood(model(x, derivative_directions=D)).mean`
 * (experiments/bunny/exp_bunny.py:189-195 `means, _ = eval_gp(...)`, experiments/rover/bo_traditional.py:214 `preds.mean`) for the
 * Cholesky-whitened strategy (DirectionalGradVariationalStrategy.py:181-188: mu = K_XZ L^-T m + c).  With alpha = L^-T m (fp64: one
 * dsvgp_trsm with trans = 1 per parameter state), a_i = alpha[i(p+1)], g_i = sum_s alpha[i(p+1)+1+s] v^_is (v^: L2-normalised inducing
 * directions, RBFKernelDirectionalGrad.py:57), r_i = (z_i - x) / ell, k_i = exp(-|r_i|^2 / 2), beta_i = a_i - (r_i . g_i) / ell:
 *     mu_f(x) = c + s sum_i k_i beta_i,   grad mu_f(x) = s sum_i k_i (beta_i r_i / ell + g_i / ell^2),
 *     row of direction w at x (interleaved after the value row) = c + w^ . grad mu_f(x)          (the constant on every row: DGVS.py:126)
 * O(M d) per point instead of O(M'^2); nothing of size M' x B' exists; the directions at the data (pd per point) are independent of the
 * model's p (p = 0: plain SVGP, p = d: full-gradient SVGP).
 *   dsvgp_mean_prepare   alpha[M(p+1)] (double), Z[M,d], V[M*p,d] (raw directions, normalised here; NULL when p = 0; p <= 95), hyp,
 *                        constant (device float), center[d] (NULL = 0; the column mean of Z keeps the composed path's fp32 expansion
 *                        accurate, as in dsvgp_pack_points) -> weights: dsvgp_mean_weights_bytes(M, d) bytes, 16-byte aligned, fp32:
 *                        {ell, s, c, ..}, center, a, a - z~.g/ell, |z~|^2, [Z~ ; G/ell].  One launch.
 *   dsvgp_mean_predict   x[B,d], D (NULL or [B*pd, d] raw directions, normalised here) -> mean_out[B(pd+1)] interleaved, grad_out (NULL
 *                        or [B,d]) = grad mu_f (without the constant).  One call per batch: no host read, no synchronisation, no
 *                        allocation, queued on the context's stream.  d <= 32: ONE fused kernel (a workgroup owns 64 test points, walks
 *                        the inducing points in LDS-staged chunks, accumulator in registers; workspace may be NULL).  Any other d: the
 *                        same sums through [B, 2M] intermediates in `workspace` (dsvgp_mean_workspace_bytes(M, d, B, pd) bytes, 16-byte
 *                        aligned; 0 for d <= 32): [S1 | S2] = X~ [Z~ ; G']^T on the fp32 MFMA GEMM, a pointwise kernel, the
 *                        [B, 2M] x [2M, d] product, an epilogue kernel; at most 2 B M + 2 B (d + 3) + 4 B + 8 floats.
 *                        DSVGP_EINVAL when B * 2M reaches 2^31 there (split the batch).
 * No floating-point atomics and fixed-order reductions on both paths: two identical calls return bitwise identical results.
 * DSVGP_EINVAL for M, B or d < 1.  The two size helpers are pure host functions (0 for a shape not taken).                          */
size_t dsvgp_mean_weights_bytes(int M, int d);
size_t dsvgp_mean_workspace_bytes(int M, int d, int B, int pd);
int dsvgp_mean_prepare(dsvgp_ctx* ctx, const double* alpha, const float* Z, const float* V, int M, int d, int p, const float* hyp,
                       const float* constant, const float* center, float* weights);
int dsvgp_mean_predict(dsvgp_ctx* ctx, const float* weights, int M, int d, const float* x, int B, const float* D, int pd,
                       float* mean_out, float* grad_out, void* workspace);

/* ---- pathwise posterior samples (csrc/paths.hip): draws of the posterior FUNCTION, evaluated with their exact gradient at any number
 * of points in any number of batches -- what the reference's Thompson samplers take from `preds.sample(torch.Size([n]))`
 * (experiments/rover/test_turbo.py:138, experiments/GNN_bo/gcn_turbo.py:239,341, turbo1*.py:216-227), without anything of size B' x B'.
 * Matheron's rule with a random-Fourier-feature prior (K~ = s K_ZZ + j I = L L^T, j the TOTAL diagonal added; u = L (m + L_S eps)):
 *     f_s(x) = c + sum_j w_js phi_j(x) + K_xZ' nu_s,   nu_s = L^-T [m + L_S eps_s - L^-1 (Phi_Z' w_s + sqrt(j) eta_s)]
 *     phi_j(x) = sqrt(2 s / F) cos(omega_j . x / ell + b_j),   omega_j ~ N(0, I_d), b_j ~ U[0, 2 pi), w_s, eps_s, eta_s standard normal
 * The update term K_xZ' nu_s is the posterior mean's closed form above with alpha -> nu_s; the caller forms nu [n, M(p+1)] in fp64 (two
 * dsvgp_trsm calls per parameter state and sample set).
 *   dsvgp_paths_prepare   nu[n, M(p+1)], w[n, F], omega[F, d], phase[F] (double), Z, V (raw directions, normalised here; NULL when
 *                         p = 0; p <= 95), hyp, constant, center[d] (NULL = 0) -> weights: dsvgp_paths_weights_bytes(M, d, F, n) bytes,
 *                         16-byte aligned, fp32 from fp64 sums: {ell, s, c, ..}, center, |z~|^2, Z~, the feature table in REVOLUTIONS
 *                         (omega_j / 2 pi against x~ = (x - center) / ell; b_j plus the centre's contribution reduced mod 1 in fp64), and
 *                         per sample a, a - z~.g/ell, sqrt(2 / (s F)) w, G/ell.  Rows padded to multiples of 4 floats.  Three launches.
 *   dsvgp_paths_eval      x[B, d] -> values[n, B], grads (NULL or [n, B, d]) = grad f_s (without the constant).  No host read, no
 *                         synchronisation, no allocation, queued on the context's stream.  d <= 32: ONE fused kernel (a workgroup owns 64
 *                         points and a group of samples, inducing points and features in LDS chunks, accumulators in registers;
 *                         workspace may be NULL): the result of (sample, point) is a function of that sample and that point alone, so a
 *                         path evaluated in batches, or prepared with other samples, returns the same bits.  Any other d: the same sums
 *                         in GEMM shape through `workspace` (dsvgp_paths_workspace_bytes(M, d, F, n, B, want_grad) bytes, 16-byte aligned;
 *                         0 for d <= 32) on the fp32 MFMA GEMM, unsplit, with pointwise kernels between the products; samples go through
 *                         in groups sized by the helper.  Sines and cosines: the hardware instructions after a fract.
 * No floating-point atomics on either route: two identical calls return bitwise identical results.  DSVGP_EINVAL for M, d, F, n or
 * B < 1, a null required pointer, a misaligned `weights` (dsvgp_paths_eval) or an intermediate that would pass 2^31 entries (split the
 * batch).  The two size helpers are pure host functions (0 for arguments the entries refuse).                                        */
size_t dsvgp_paths_weights_bytes(int M, int d, int F, int n);
size_t dsvgp_paths_workspace_bytes(int M, int d, int F, int n, int B, int want_grad);
int dsvgp_paths_prepare(dsvgp_ctx* ctx, const double* nu, const double* w, const double* omega, const double* phase, const float* Z,
                        const float* V, int M, int d, int p, int F, int n, const float* hyp, const float* constant, const float* center,
                        float* weights);
int dsvgp_paths_eval(dsvgp_ctx* ctx, const float* weights, int M, int d, int F, int n, const float* x, int B, float* values,
                     float* grads, void* workspace);

/* ---- Hessian-vector products of the paths (csrc/paths.hip): second-order information for a Newton or trust-region refinement of a
 * candidate on its own sampled function, or the curvature of a fitted implicit surface.  With x~ = (x - center) / ell, r_i = z~_i - x~,
 * k_i = exp(-|r_i|^2 / 2), G'_is = g_is / ell, beta_is = a_is - r_i . G'_is, theta_j = Om_j . x~ + ph_j (revolutions) and wq_js as above
 *     grad^2 f_s(x) v = (s / ell^2) [ sum_i ((k_i beta_is (r_i.v) + k_i (G'_is.v)) r_i + k_i (r_i.v) G'_is)
 *                                     + sum_j wq_js (-4 pi^2 cos 2 pi theta_j)(Om_j.v) Om_j - (sum_i k_i beta_is) v ]
 * -- the terms the gradient already uses; r_i.v and Om_j.v do not depend on the sample, no sine is needed, and nothing of size d x d is
 * formed (d accumulators per sample, as for the gradient; 4 d FMAs per (point, i, sample) where the gradient takes 3 d).
 *   dsvgp_paths_hvp       `weights` as dsvgp_paths_prepare wrote them (unchanged); x[B, d]; v[B, d]: ONE vector per point, shared by
 *                         all samples, used as given (not normalised) -> hv[n, B, d] = grad^2 f_s(x_b) v_b.  The host contract is
 *                         dsvgp_paths_eval's: no host read, no synchronisation, no allocation, queued on the context's stream.
 *                         d <= 32: ONE fused kernel of dsvgp_paths_eval's structure with v next to x~ and r in the lane's registers
 *                         (narrower sample groups at the large d; workspace may be NULL): the result of (sample, point) is a function
 *                         of that sample, that point and its vector alone.  Any other d: the same sums in GEMM shape through `workspace`
 *                         (dsvgp_paths_hvp_workspace_bytes(M, d, F, n, B) bytes, 16-byte aligned; 0 for d <= 32) on the unsplit fp32
 *                         MFMA GEMM, samples in groups sized by the helper.
 * No floating-point atomics on either route: two identical calls return bitwise identical results.  DSVGP_EINVAL as for
 * dsvgp_paths_eval: M, d, F, n or B < 1, a null required pointer (v included), a misaligned `weights`, or an intermediate that would
 * pass 2^31 entries (split the batch).  The size helper is a pure host function (0 for d <= 32 and for arguments the entry refuses). */
size_t dsvgp_paths_hvp_workspace_bytes(int M, int d, int F, int n, int B);
int dsvgp_paths_hvp(dsvgp_ctx* ctx, const float* weights, int M, int d, int F, int n, const float* x, const float* v, int B, float* hv,
                    void* workspace);

/* ---- paths at their OWN points (csrc/paths.hip): sample s evaluated at x[s], and a device-resident projected-gradient descent of every
 * (sample, start) pair on its own path -- the refinement of a Thompson candidate on its own sampled function.  dsvgp_paths_eval shares
 * one point set among the n samples; after one step of a per-path refinement the n point sets differ.
 *   dsvgp_paths_eval_own  `weights` as dsvgp_paths_prepare wrote them (unchanged); x[n, B, d] -> values[n, B] = f_s(x[s][b]), grads (NULL
 *                         or [n, B, d]) = grad f_s (without the constant).  The host contract is dsvgp_paths_eval's: no host read, no
 *                         synchronisation, no allocation, queued on the context's stream.  d <= 32: ONE fused kernel; a workgroup of 8
 *                         waves owns 64 points of ONE sample (grid [ceil(B / 64), n], lane = point; x~, r, the d accumulators and the
 *                         value in registers; inducing points, then features through LDS in chunks of 64; the waves' partial sums added
 *                         in the order 0..7); the arithmetic of a (sample, point) is dsvgp_paths_eval's and its result depends on that
 *                         sample and that point alone (not on B, n, the neighbours or the card); workspace may be NULL.  Any other d:
 *                         the n B points as rows of one stacked problem on the unsplit fp32 MFMA GEMM through `workspace`
 *                         (dsvgp_paths_own_workspace_bytes(M, d, F, n, B, want_grad) bytes, 16-byte aligned; 0 for d <= 32): X~ Z~^T,
 *                         X~ Om^T, P Z~ and S Om stacked, X~_s G'_s^T and K_s G'_s one product per sample, pointwise kernels and
 *                         fixed-order row sums between them: 10 + 2 n launches with gradients (the per-sample products are small at the
 *                         B a refinement uses).  grads = NULL returns the same values bits.
 *   dsvgp_paths_descend   x[n, B, d] (in: starts, out: iterates), lower[d], upper[d]; sigma = +1 to minimise, -1 with `maximize`.
 *                         resume = 0: x <- clamp(x); (f, g) by dsvgp_paths_eval_own; eta = step0 / max(|g|, 1e-30) with
 *                         step0 = initial_step, or 0.25 ell read from the weights on the device when initial_step <= 0; accepted = 0.
 *                         resume = 1: x, values, grads, steps, accepted are the state a previous call left (no first evaluation).
 *                         Then `iterations` times, per pair: y = clamp(x - sigma eta g); (f_y, g_y) by the own-point evaluation of all
 *                         pairs; accept iff sigma f_y <= sigma f + 1e-4 sigma g.(y - x) (a NaN f_y rejects): x, f, g <- y, f_y, g_y,
 *                         eta <- min(2 eta, 1e30), accepted += 1; else eta <- eta / 2.  One step kernel (one wave per pair, fixed-order
 *                         wave sums) judges iteration t and proposes iteration t + 1: a call is a clamp, 1 + iterations evaluations
 *                         (`iterations` when resuming) and 1 + iterations step launches, no host read.  sigma values never increases;
 *                         iterates stay in the box; iterations = 0 gives the start state.  values[n, B], grads[n, B, d], steps[n, B],
 *                         accepted[n, B] (int) are outputs (and inputs when resuming).  `workspace`:
 *                         dsvgp_paths_descend_workspace_bytes(M, d, F, n, B) bytes, 16-byte aligned, never 0 for a shape the entry takes
 *                         (the trial point, its value and gradient live there on both routes).
 * No floating-point atomics.  DSVGP_EINVAL as for dsvgp_paths_eval (M, d, F, n or B < 1, a null required pointer, a misaligned `weights`
 * or workspace, an intermediate that would pass 2^31 entries), for n > 65535, and in dsvgp_paths_descend for iterations < 0.  The size
 * helpers are pure host functions (0 for arguments the entries refuse).                                                              */
size_t dsvgp_paths_own_workspace_bytes(int M, int d, int F, int n, int B, int want_grad);
int dsvgp_paths_eval_own(dsvgp_ctx* ctx, const float* weights, int M, int d, int F, int n, const float* x, int B, float* values,
                         float* grads, void* workspace);
size_t dsvgp_paths_descend_workspace_bytes(int M, int d, int F, int n, int B);
int dsvgp_paths_descend(dsvgp_ctx* ctx, const float* weights, int M, int d, int F, int n, float* x, int B, const float* lower,
                        const float* upper, int iterations, float initial_step, int maximize, int resume, float* values, float* grads,
                        float* steps, int* accepted, void* workspace);

/* ---- data-driven initialisation (csrc/kmeans.hip): k-means for the inducing points, per-cluster second moments of the gradients for the
 * inducing directions.  Every entry queues on the context's stream: no host read, no allocation, no synchronisation, no floating-point
 * atomics; two identical calls return identical bits.  Data are fp32 (x[N, d], Z[M, d], dist2), labels and counts int32, sums fp64.
 *   dsvgp_kmeans_assign   per point the nearest centroid (labels) and the squared distance to it (dist2); an exact tie goes to the lowest
 *                         centroid index.  d <= 32: ONE fused kernel (a workgroup owns 64 points, lane = point in registers; centroids
 *                         through LDS in chunks of 64 split over 8 waves; distance in the difference form sum_k (z_k - x_k)^2 by FMAs in
 *                         the order of k; the waves' winners combined in the order 0..7): the result of a point depends on that point and
 *                         on Z alone; workspace may be NULL.  Any other d: S = X~ Z~^T on the unsplit fp32 MFMA GEMM in row blocks of
 *                         32768, X~ and Z~ centred on the column mean of Z, then a row-wise arg-min over |z~|^2 - 2 S (one wave per row,
 *                         the lower index on equality), dist2 = max(|x~|^2 + min, 0); `workspace`: dsvgp_kmeans_workspace_bytes(N, d, M)
 *                         bytes, 16-byte aligned (0 for d <= 32).
 *   dsvgp_kmeans_update   Z[m] <- mean of the rows labelled m (fp64 sums, rounded once); an empty cluster keeps its row and reports
 *                         count 0.  One workgroup per centroid walks all N labels in order; the order of every sum is fixed by N and
 *                         `labels` alone.
 *   dsvgp_kmeans_lloyd    `iterations` times assign -> inertia -> update, then a closing assignment against the final centroids:
 *                         labels, dist2 and counts[M] (the cluster sizes) belong to that closing assignment; inertia[t] = sum dist2 of
 *                         assignment t (double, iterations + 1 entries, fixed-order fp64 sum); moved[t] = number of labels that differ
 *                         between assignments t and t + 1 (int, `iterations` entries; may be NULL when iterations = 0).  The iteration
 *                         count is fixed: the caller reads `moved` afterwards if it wants to.  iterations = 0 is one assignment.  k calls
 *                         of one iteration, each resumed from the previous call's Z, return the bits of one call of k.
 *   dsvgp_cluster_moments C[M, d, d] (double) = sum_{i in m} g_i g_i^T per cluster (uncentred), exactly symmetric; d <= 128; grid
 *                         (cluster, 32 x 32 tile of the upper triangle), the update's in-order walk; workspace is not used (may be NULL).
 * DSVGP_EINVAL, with nothing touched: a null required pointer; N, d or M < 1; M > N; iterations < 0; on the composed route a missing or
 * misaligned workspace or an intermediate that would pass 2^31 entries; d > 128 for the moments.  dsvgp_kmeans_workspace_bytes is a pure
 * host function (0 for d <= 32 and for arguments the entries refuse).                                                               */
size_t dsvgp_kmeans_workspace_bytes(int N, int d, int M);
int dsvgp_kmeans_assign(dsvgp_ctx* ctx, const float* x, int N, int d, const float* Z, int M, int* labels, float* dist2, void* workspace);
int dsvgp_kmeans_update(dsvgp_ctx* ctx, const float* x, int N, int d, const int* labels, float* Z, int M, int* counts);
int dsvgp_kmeans_lloyd(dsvgp_ctx* ctx, const float* x, int N, int d, float* Z, int M, int iterations, int* labels, float* dist2,
                       int* counts, double* inertia, int* moved, void* workspace);
int dsvgp_cluster_moments(dsvgp_ctx* ctx, const float* g, int N, int d, const int* labels, int M, double* C, void* workspace);

/* ---- posterior variance of a frozen model with its gradient, acquisitions and their descent (csrc/predict_variance.hip): what the
 * reference's confidence-bound callers read from `preds.variance` (experiments/rover/bo_traditional.py:214 `preds.mean - lcb_beta *
 * preds.variance`, experiments/GNN_bo/bo.py:171-173 `preds.variance.sqrt()`), plus the gradient the reference does not have.
 * Cholesky-whitened strategy, value rows (DirectionalGradVariationalStrategy.py:188-205).  With K~ = s K_ZZ + j I = L L^T, S = L_S L_S^T,
 * k(x) = s K_Z'x and Q = L^-T (S - I) L^-1 [M', M'] (double, exactly symmetric, formed by the caller ONCE per parameter state: two
 * dsvgp_trsm calls with trans = 1):
 *     v(x) = Q k(x),   sigma^2(x) = s + 1e-4 + k(x) . v(x)   (q(f), no likelihood noise),   grad sigma^2(x) = 2 (dk/dx)^T v(x)
 * Q stays in double and V = Q K_ZX is accumulated in double (Q rounded to float costs three digits of sigma^2: the sum cancels);
 * V is rounded once to float and everything after it is float.
 *   dsvgp_var_prepare    Z[M,d], V[M*p,d] (raw directions, normalised here; NULL when p = 0; p <= 95), hyp, center[d] (NULL = 0; MUST be
 *                        the centre the inducing pack below was made with) -> weights: dsvgp_var_weights_bytes(M, d, p) bytes, 16-byte
 *                        aligned, fp32: {ell, s, 1/ell, s/ell, ..}, center, Z~ = (Z - center) / ell, the unit directions; rows padded to
 *                        multiples of 4 floats.  One launch.
 *   dsvgp_var_predict    Q (leading dimension ldq >= M' = M(p+1)), PZ / selfZ = what dsvgp_pack_points wrote for (Z, V, p), x[B,d] ->
 *                        var_out[B], grad_out (NULL or [B,d]).  One batch: K_ZX [M', B] by dsvgp_pack_points + dsvgp_kernel_fwd_rect
 *                        (data side p = 0), V = Q K_ZX on the fp64 MFMA GEMM with the float right operand, never split along K (no
 *                        atomics), then one of two routes (dsvgp_var_route(d, p): 1 = fused, 2 = composed, 0 = refused arguments):
 *                        fused: d <= 32 and dsvgp_var_chunk(d, p) = min(64, floor(12288 / ((p + 1) pad4(d)))) rounded down to a multiple
 *                        of 8 is >= 8 (a chunk of that many inducing points with their unit directions is staged in 48 KB of LDS): ONE
 *                        kernel, a workgroup of 8 waves owns 64 points (lane = point, weights read from V[:, b]), partial sums added in
 *                        the order 0..7; grad_out = NULL returns the same values bits.  composed (any other shape): one kernel for
 *                        sigma^2 = s + 1e-4 + colsum(K_ZX o V) (row slices of 256, fixed order) that also writes G = 2 V^T [B, M'], a
 *                        fixed-order combine, then dsvgp_kernel_bwd_rect(G, side 1 = the x pack, side 2 = the inducing pack) into the
 *                        zeroed grad_out.  `workspace`: dsvgp_var_workspace_bytes(M, d, p, B, want_grad) bytes, 16-byte aligned, never 0
 *                        for a shape the entry takes: the x pack (B (pad4(d) + 4) + pad4(B) floats), K_ZX and V (M' pad4(B) floats
 *                        each) on both routes; composed adds ceil(M' / 256) pad4(B) floats and, with the gradient, B pad4(M') + 4 floats
 *                        and dsvgp_kernel_bwd_rect's workspace.
 *   dsvgp_acq_eval       mu[B], gmu[B,d], var[B], gvar[B,d] -> out[B] and gout (NULL or [B,d]; gmu / gvar may be NULL without it).  All
 *                        kinds are stated for MINIMISATION of the modelled function; maximize != 0 mirrors the model (mu -> -mu,
 *                        best -> -best).  kind 0 "lcb_var": mu - beta sigma^2 (the reference's literal form); 1 "lcb": mu - beta sigma,
 *                        sigma = sqrt(max(sigma^2, 1e-6)); 2 "ei": -[(best - mu) Phi(z) + sigma phi(z)], z = (best - mu) / sigma, with
 *                        gradient Phi(z) grad mu - phi(z) grad sigma, grad sigma = grad sigma^2 / (2 sigma), taken as 0 where sigma^2 is
 *                        clamped.  beta / best: device floats (the one the kind does not use may be NULL).  One pointwise launch.
 *   dsvgp_acq_descend    dsvgp_paths_descend's rule with n = 1 on the acquisition of B starts x[B,d] (in: starts, out: iterates) inside
 *                        [lower, upper]: resume = 0: x <- clamp(x); (f, g) by dsvgp_mean_predict + dsvgp_var_predict + dsvgp_acq_eval;
 *                        eta = step0 / max(|g|, 1e-30), step0 = initial_step, or 0.25 ell when initial_step <= 0; accepted = 0.
 *                        resume = 1: x, values, grads, steps, accepted are the state a previous call left.  Then `iterations` times, per
 *                        start: y = clamp(x - eta g); accept iff f_y <= f + 1e-4 g.(y - x) (a NaN f_y rejects): x, f, g <- y, f_y, g_y,
 *                        eta <- min(2 eta, 1e30), accepted += 1; else eta <- eta / 2.  One step kernel (one wave per start, fixed-order
 *                        wave sums).  The acquisition is always minimised (`maximize` goes to dsvgp_acq_eval); values never increase;
 *                        iterates stay in the box; iterations = 0 gives the start state.  mean_weights: dsvgp_mean_prepare's, of the
 *                        same state.  `workspace`: dsvgp_acq_descend_workspace_bytes(M, d, p, B) bytes, 16-byte aligned.
 * Every entry queues on the context's stream: no host read, no allocation, no synchronisation, no floating-point atomics, fixed summation
 * orders; two identical calls return identical bits.  DSVGP_EINVAL: a null required pointer, M, d or B < 1, p outside [0, 95], a kind
 * outside 0..2, iterations < 0, ldq < M', or an intermediate that would pass 2^31 entries (split the batch); DSVGP_EALIGN: a misaligned
 * weights, workspace, PZ or Q.  The size, route and chunk helpers are pure host functions (0 for arguments the entries refuse). */
int dsvgp_var_route(int d, int p);
int dsvgp_var_chunk(int d, int p);
size_t dsvgp_var_weights_bytes(int M, int d, int p);
size_t dsvgp_var_workspace_bytes(int M, int d, int p, int B, int want_grad);
int dsvgp_var_prepare(dsvgp_ctx* ctx, const float* Z, const float* V, int M, int d, int p, const float* hyp, const float* center,
                      float* weights);
int dsvgp_var_predict(dsvgp_ctx* ctx, const float* weights, const double* Q, int64_t ldq, const float* PZ, const float* selfZ,
                      const float* hyp, int M, int d, int p, const float* x, int B, float* var_out, float* grad_out, void* workspace);
int dsvgp_acq_eval(dsvgp_ctx* ctx, int kind, int maximize, const float* beta, const float* best, const float* mu, const float* gmu,
                   const float* var, const float* gvar, int B, int d, float* out, float* gout);
size_t dsvgp_acq_descend_workspace_bytes(int M, int d, int p, int B);
int dsvgp_acq_descend(dsvgp_ctx* ctx, const float* mean_weights, const float* var_weights, const double* Q, int64_t ldq, const float* PZ,
                      const float* selfZ, const float* hyp, int M, int d, int p, float* x, int B, const float* lower, const float* upper,
                      int kind, const float* beta, const float* best, int maximize, int iterations, float initial_step, int resume,
                      float* values, float* grads, float* steps, int* accepted, void* workspace);

/* ---- closed-form optimal q(u) (Titsias 2009) from one-pass statistics, and the full-data ELBO of any q(u) (csrc/collapsed.hip,
 * DESIGN.md section 23).  With the Gaussian likelihood and fixed hyper-parameters / inducing points the maximiser of the ELBO over q(u) is
 *   B = I + kappa G,  S* = B^-1,  m* = kappa B^-1 b,  kappa = num_data / (R noise),   G = sum A A^T, b = sum A r, yy = sum r^T r, r = y - c
 * in the whitened basis A = L^-1 K_ZX, R = rows accumulated.  The statistics live in a caller-owned `state` of
 * dsvgp_collapsed_state_bytes(Mp) bytes (8-byte aligned): doubles [0] = sum of the prior diagonal, [1] = R, [2..7] reserved, then the
 * row-major (Mp+1) x (Mp+1) matrix tril([A ; r^T][A ; r^T]^T): rows < Mp hold tril G, row Mp holds b^T and, last, yy; its strict upper
 * triangle stays zero.
 *   dsvgp_collapsed_reset       state <- 0 (one memset).
 *   dsvgp_collapsed_accumulate  A64: (Mp + 1) x Bp doubles, leading dimension lda >= Bp, rows < Mp = A as dsvgp_trsm wrote it (X64); row Mp
 *                               is WRITTEN here: r = y - constant[0] in float64.  Then the matrix += tril([A ; r^T][A ; r^T]^T) in place on the
 *                               fp64 MFMA GEMM (beta = 1; its split-K slices meet in fp64 atomics on the live state: run-order rounding of G,
 *                               b and yy), and [0] += sum prior_diag[Bp], [1] += Bp in one launch with a fixed summation order (no atomics).
 *                               prior_diag: dsvgp_kernel_diag / _ard / _matern52 of the chunk (without the 1e-4 jitter).  Bp = 0: returns 0,
 *                               nothing is touched.
 *   dsvgp_collapsed_solve       the optimum for hyp[2] = noise and num_data (> 0): m[Mp], LS[Mp, ldls] = chol(S*) (lower, strict upper triangle
 *                               exactly zero), nat_vec[Mp] = kappa b, nat_mat[Mp, ldnm] = -B / 2 (exactly symmetric) as float32 -- gpytorch's
 *                               natural parameters -- and scalars[8] (float64): loss, sum ll, KL, sum |residual|^2, sum varn at the optimum,
 *                               then R, kappa, tr G.  loss = -(sum ll / R - KL / num_data), the objective of dsvgp_likelihood_terms +
 *                               dsvgp_kl_terms with all R rows as one batch.  J B J = Lt Lt^T is factored by dsvgp_potrf_inverse (J = exchange
 *                               matrix) and chol(S*) = J Lt^-T J is read off its inverse: no second factorisation.  Every output pointer may be
 *                               NULL.  *info (device int): 0, k > 0 (leading minor k of J B J not positive definite), -1 (a non-finite
 *                               statistic), -2 (R = 0); with info != 0 the float outputs and scalars[0..4] are NaN.  Never reads the host.
 *   dsvgp_collapsed_evaluate    scalars[8] as above for the caller's float32 (m, tril LS): <S, G> = sum(G L_S o L_S) with G L_S on the fp64 MFMA
 *                               GEMM, m^T G m, KL -- float64 arithmetic, fixed summation orders, no M' x B' object.
 * `workspace`: dsvgp_collapsed_workspace_bytes(Mp) bytes, 16-byte aligned, for solve and evaluate.  DSVGP_EINVAL: a null required pointer,
 * Mp <= 0, Mp > 8192 (solve / evaluate: the explicit-inverse regime), lda < Bp, ldls / ldnm < Mp, num_data <= 0 -- nothing is touched.   */
size_t dsvgp_collapsed_state_bytes(int Mp);
size_t dsvgp_collapsed_workspace_bytes(int Mp);
int dsvgp_collapsed_reset(dsvgp_ctx* ctx, void* state, int Mp);
int dsvgp_collapsed_accumulate(dsvgp_ctx* ctx, void* state, int Mp, double* A64, int64_t lda, int Bp, const float* y,
                               const float* constant, const float* prior_diag);
int dsvgp_collapsed_solve(dsvgp_ctx* ctx, const void* state, int Mp, const float* hyp, double num_data, float* m, float* LS, int64_t ldls,
                          float* nat_vec, float* nat_mat, int64_t ldnm, double* scalars, int* info, void* workspace);
int dsvgp_collapsed_evaluate(dsvgp_ctx* ctx, const void* state, int Mp, const float* m, const float* LS, int64_t ldls, const float* hyp,
                             double num_data, double* scalars, void* workspace);

/* ---- gradients of the collapsed bound at the optimum (csrc/collapsed.hip): SGPR training, the second pass.
 * Valid ONLY for (m, LS) = the result of dsvgp_collapsed_solve on the same statistics, hyp and num_data: by the envelope theorem the total
 * derivative then equals the partial one at fixed whitened q(u), and the upstream of K~ = s K_ZZ + jitter I needs no Cholesky backward.
 * With alpha = L^-T m, Q = L^-T (S - I) L^-1, w = 1 / (2 R noise), rho = (y - c) - K_ZX^T alpha:
 *   K_ZX-bar = 2 w (Q K_ZX - alpha rho^T)        K~-bar = (Q + alpha alpha^T + kappa L^-T G L^-1) / (2 num_data)        dg-bar = w
 *   c-bar = -2 w sum rho                          d loss / d noise = -(E + V) / (2 R noise^2) + 1 / noise
 *   dsvgp_collapsed_grad_prepare   once per backward pass.  inverse: L^-1 | L^-T of the factor of K~, 2 Mp^2 doubles with leading dimension Mp
 *                                  (the head of dsvgp_trsm's workspace after dsvgp_potrf_inverse).  Writes alpha[Mp], Q[Mp, ldq] and
 *                                  Kzz_bar[Mp, ldkb] (float64, both exactly symmetric; four triangular fp64 MFMA products and S = L_S L_S^T),
 *                                  adj[8] (float64): w, d loss / d noise, dg-bar, loss, E = sum |residual|^2, V = sum varn, kappa, R; and
 *                                  *info (device int): 0, or 1 when a statistic, (m, LS) or a result is not finite or R = 0 (nothing faults;
 *                                  the outputs are then not to be used).  workspace: dsvgp_collapsed_grad_workspace_bytes(Mp), 16-byte aligned.
 *   dsvgp_collapsed_grad_chunk     per chunk: K_bar[Mp, ldkb] (float32, must not overlap Kzx) = K_ZX-bar of the chunk's float32 Kzx[Mp, ldk],
 *                                  ready for dsvgp_kernel_bwd_rect / _ard / _matern52 with the inducing side as side 1; diag_bar[Bp] (may be
 *                                  NULL) = dg-bar for the prior diagonal's backward; rho_sum[0] += sum rho (one writer, fixed order).
 *                                  Launches: the residual's column reduction in row slabs of 256 and its fixed-order combine, Q Kzx on the
 *                                  fp64 MFMA GEMM over the float operand (one K slice, rounded once), the in-place epilogue.  No
 *                                  floating-point atomics, no host read, no allocation: two identical calls give bitwise equal results.
 *                                  workspace: dsvgp_collapsed_grad_chunk_bytes(Mp, Bp), 8-byte aligned.
 * The size helpers return 0 for refused arguments (Mp <= 0, Mp > 8192, Bp <= 0).  DSVGP_EINVAL: a null required pointer, Mp <= 0, Mp > 8192,
 * Bp <= 0, a leading dimension below its row length, num_data <= 0, the extents of K_bar and Kzx overlapping anywhere; DSVGP_EALIGN: a misaligned pointer.    */
size_t dsvgp_collapsed_grad_workspace_bytes(int Mp);
size_t dsvgp_collapsed_grad_chunk_bytes(int Mp, int Bp);
int dsvgp_collapsed_grad_prepare(dsvgp_ctx* ctx, const void* state, int Mp, const float* m, const float* LS, int64_t ldls,
                                 const double* inverse, const float* hyp, double num_data, double* alpha, double* Q, int64_t ldq,
                                 double* Kzz_bar, int64_t ldkb, double* adj, int* info, void* workspace);
int dsvgp_collapsed_grad_chunk(dsvgp_ctx* ctx, int Mp, int Bp, const float* Kzx, int64_t ldk, const float* y, const float* constant,
                               const double* Q, int64_t ldq, const double* alpha, const double* adj, float* K_bar, int64_t ldkb,
                               float* diag_bar, double* rho_sum, void* workspace);

/* ---- missing observations (csrc/missing.hip): a NaN entry of y is an observation that does not exist.  The present
 * mask is derived from y inside the kernels, the present rows are counted on the device, and the unchanged kernels behind these entries see
 * exact zeros on the missing rows.  Inf is not a mask value: it propagates as before.  Fixed-order sums (per-workgroup partials joined in
 * workgroup order), no floating-point atomics, no host read, no allocation: two identical calls give bitwise equal results.
 *   dsvgp_likelihood_terms_masked      dsvgp_likelihood_terms over the present rows with global_rows = n, their count: mu_bar, var_bar and
 *                                      varn_out are exactly 0 on a missing row; out_scalars[1..4] carry the 1 / n of the loss as before and
 *                                      out_scalars[0] = sum ll / n is ALREADY normalised, so dsvgp_step_epilogue takes rows = 1.  n = 0: every
 *                                      output is 0 (the loss is then KL / num_data).  *n_present (device int) = n.  workspace:
 *                                      dsvgp_likelihood_terms_masked_workspace_bytes() bytes, 16-byte aligned.  ncols = 0: out_scalars and
 *                                      *n_present are cleared, no launch.
 *   dsvgp_collapsed_accumulate_masked  dsvgp_collapsed_accumulate with: the columns of A64 whose target is missing set to exactly 0 before the
 *                                      (unchanged) fp64 MFMA product, r = 0 there, [0] += the PRESENT entries of prior_diag, [1] += the present
 *                                      count and the reserved word [2] += the present count of value rows (j % (pd + 1) == 0; the scalar RBF
 *                                      prior diagonal's backward needs it).  Bp must be a multiple of pd + 1.
 *   dsvgp_collapsed_grad_chunk_masked  dsvgp_collapsed_grad_chunk with K_bar's columns, diag_bar and the contribution to rho_sum exactly 0 on the
 *                                      missing rows: the missing columns of Kzx are zeroed IN PLACE and y is copied with the constant in the
 *                                      missing entries (residual exactly 0), the unchanged chunk call runs on them, and dg-bar is cleared on
 *                                      the missing rows.  workspace: dsvgp_collapsed_grad_chunk_masked_bytes(Mp, Bp) bytes, 8-byte aligned.
 * DSVGP_EINVAL: a null pointer (diag_bar excepted), a negative size, mll_type outside {0, 1}, Bp not a multiple of pd + 1, whatever the
 * unmasked sibling refuses; DSVGP_EALIGN: a misaligned pointer.  Size 0 returns 0 without a launch where the sibling does.                    */
size_t dsvgp_likelihood_terms_masked_workspace_bytes(void);
int dsvgp_likelihood_terms_masked(dsvgp_ctx* ctx, const float* mu, const float* var, const float* y, int ncols, int p, const float* hyp,
                                  int mll_type, float* mu_bar, float* var_bar, float* varn_out, float* out_scalars, int* n_present,
                                  void* workspace);
int dsvgp_collapsed_accumulate_masked(dsvgp_ctx* ctx, void* state, int Mp, double* A64, int64_t lda, int Bp, int pd, const float* y,
                                      const float* constant, const float* prior_diag);
size_t dsvgp_collapsed_grad_chunk_masked_bytes(int Mp, int Bp);
int dsvgp_collapsed_grad_chunk_masked(dsvgp_ctx* ctx, int Mp, int Bp, float* Kzx, int64_t ldk, const float* y, const float* constant,
                                      const double* Q, int64_t ldq, const double* alpha, const double* adj, float* K_bar, int64_t ldkb,
                                      float* diag_bar, double* rho_sum, void* workspace);

/* ---- two likelihood noises (csrc/noise_classes.hip): the function-value rows of an interleaved batch
 * (j % (p + 1) == 0) are observed under n_f = hyp[2], the derivative rows under n_g = hyp[3] (the caller writes hyp[3] behind
 * dsvgp_hyp_forward / _ard, which leave 0 there).  The class is read from the row index.  Fixed-order sums (per-workgroup partials joined
 * in workgroup order), no floating-point atomics, no host read, no allocation: two identical calls give bitwise equal results.
 *   dsvgp_likelihood_terms_classes      dsvgp_likelihood_terms with the row's class noise in every per-row formula (ELBO and PLL, the
 *                                       clamp at 1e-6 included).  out_scalars[0], [2..4] as there; out_scalars[1] = d loss / d n_f from the
 *                                       value rows only, out_scalars[5] = d loss / d n_g from the derivative rows only (exactly 0 at p = 0),
 *                                       out_scalars[6..7] = 0.  workspace: dsvgp_likelihood_terms_classes_workspace_bytes() bytes, 16-byte
 *                                       aligned.  ncols = 0: out_scalars is cleared, no launch.
 *   dsvgp_collapsed_accumulate_classes  dsvgp_collapsed_accumulate with row weights omega = 1 on value rows and rho = hyp[2] / hyp[3] on
 *                                       derivative rows: the derivative columns of A64 (rows < Mp) and of the residual row are scaled by
 *                                       sqrt(rho) (float64) IN PLACE before the unchanged fp64 MFMA product; [0] += sum omega prior_diag +
 *                                       1e-4 sum (omega - 1), [1] += Bp, the reserved word [2] += the number of value rows.  Bp must be a
 *                                       multiple of pd + 1.  dsvgp_collapsed_solve / _evaluate run unchanged on this state with hyp[2] = n_f;
 *                                       their sum ll lacks (R_g / 2) log rho, R_g = [1] - [2], which the caller adds.
 * DSVGP_EINVAL: a null pointer, a negative size, global_rows <= 0, mll_type outside {0, 1}, Bp not a multiple of pd + 1, whatever the
 * single-noise sibling refuses; DSVGP_EALIGN: a misaligned pointer.  Size 0 returns 0 without a launch where the sibling does.         */
size_t dsvgp_likelihood_terms_classes_workspace_bytes(void);
int dsvgp_likelihood_terms_classes(dsvgp_ctx* ctx, const float* mu, const float* var, const float* y, int ncols, int p, const float* hyp,
                                   int mll_type, double global_rows, float* mu_bar, float* var_bar, float* varn_out, float* out_scalars,
                                   void* workspace);
int dsvgp_collapsed_accumulate_classes(dsvgp_ctx* ctx, void* state, int Mp, double* A64, int64_t lda, int Bp, int pd, const float* y,
                                       const float* constant, const float* prior_diag, const float* hyp);

/* ---- measurement aid (bench.py `roofline.sustained`): the MFMA rate this card holds with no memory traffic, ~`millis` ms of
 * v_mfma_f64_16x16x4_f64 (is_double = 1) or v_mfma_f32_32x32x2_f32 (0) on every CU; synchronises the stream.
 * scratch: 2 MiB of device memory.  Not part of the reference's interface (SURVEY.md 8d asks for achieved-vs-peak; the
 * data-sheet peak is at 2.4 GHz, which the card does not hold under matrix load).                                        */
int dsvgp_mfma_rate(dsvgp_ctx* ctx, int is_double, int millis, void* scratch, double* tflops);
/* mode bit 0 = is_double, bit 1 = ONE wave per SIMD (one 256-thread workgroup per CU; four otherwise); burst_tflops (may be NULL): the rate
 * of the very first ~2 ms launch from an idle card, before the power management lowers the clock; clock_ghz (may be NULL): the in-kernel clock
 * of the last launch (delta s_memtime / delta s_memrealtime x 100 MHz, median over workgroups).                                            */
int dsvgp_mfma_rate2(dsvgp_ctx* ctx, int mode, int millis, void* scratch, double* tflops, double* burst_tflops, double* clock_ghz);

#ifdef __cplusplus
}
#endif
#endif /* DSVGP_H */
