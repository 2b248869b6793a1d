// Rectangular kernel assembly, gfx950: out[n1 (p1 + 1), n2 (p2 + 1)] = s K(x1, x2; v1, v2) when the two point sets carry DIFFERENT
// numbers of directions -- the K_ZX of a model with p inducing directions evaluated at data with pd directions per point (pd = 0:
// function values only; pd = d: the full gradient).  Forward only.
//
// The formulation is assemble.hip's (header comment there): T = P1 P2^T holds every inner product of the micro-block (i, j),
//     T[i0,j0] = x1~.x2~      T[i0,jb] = x1~.v2_b      T[ia,j0] = v1_a.x2~      T[ia,jb] = v1_a.v2_b        a <= p1, b <= p2
// and a packed row does not know how many direction rows follow it, so each side is packed by dsvgp_pack_points with ITS OWN p (and
// the same centre).  Only the micro-block shape changes: (p1 + 1) x (p2 + 1).
//
// One workgroup (256 threads) per tile of Rr x Rc micro-blocks, Rr (p1 + 1) <= 96 rows by Rc (p2 + 1) <= 96 columns: each side
// fills the 96-wide tile with whole points on its own, as kernel_fwd_wide_kernel does with one q (Rc = 96 / q2 points per column
// tile, half of 96 / q1 per row tile), so q = 96 on one side and q = 1 on the other still gives a 96 x 96 tile.  T comes from the
// K-looped MFMA product of wide_product.h (32 packed columns per chunk: the LDS does not grow with d; one accumulator chain per
// entry in k order, no split over d), the transform runs out of LDS and every output element is stored once, rows coalesced.  LDS:
// max((Trp + Tcp) 33, Trp 100) + Trp + Tcp + Rr Rc floats <= 39552 bytes (p1 = 95, p2 = 0).  No atomics; two identical calls are bitwise
// equal.  At p1 == p2 the arithmetic is kernel_fwd_wide_kernel's, operation for operation.
#include "common.h"
#include "wide_product.h"

#include <climits>

namespace {

__global__ __launch_bounds__(WNT) void kernel_fwd_rect_kernel(const float* __restrict__ P1, const float* __restrict__ self1, int n1q,
                                                              int q1, int Rr, const float* __restrict__ P2,
                                                              const float* __restrict__ self2, int n2q, int q2, int Rc, int K4, int DP,
                                                              const float* __restrict__ hyp, float* __restrict__ out, int64_t ld) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Tr = Rr * q1, Tc = Rc * q2;
    const int Trp = (Tr + 15) & ~15, Tcp = (Tc + 15) & ~15;
    float* Ts = smem;                                   // [Trp][WLDT], over the chunk images
    float* s1 = smem + wide_union_floats(Trp, Tcp);
    float* s2 = s1 + Trp;
    float* KK = s2 + Tcp;                               // Rr * Rc pair values
    const int row0 = blockIdx.y * Tr, col0 = blockIdx.x * Tc;
    const int rows = min(Tr, n1q - row0), cols = min(Tc, n2q - col0);      // (whole micro-blocks: n1q, Tr multiples of q1, ...)
    for (int r = threadIdx.x; r < Trp; r += WNT) s1[r] = r < rows ? self1[row0 + r] : 0.f;
    for (int c = threadIdx.x; c < Tcp; c += WNT) s2[c] = c < cols ? self2[col0 + c] : 0.f;
    wide_T(Ts, smem, P1, row0, rows, P2, col0, cols, Trp, Tcp, K4, DP);

    // kernel_fwd_kernel's micro-block transform (assemble.hip) with a row period q1 and a column period q2
    const float ell = hyp[0], s = hyp[1];
    const float il = 1.f / ell, il2 = il * il;
    const float invq1 = 1.f / (float)q1, invq2 = 1.f / (float)q2, invRc = 1.f / (float)Rc;
    for (int pid = threadIdx.x; pid < Rr * Rc; pid += WNT) {
        const int pi = fdiv_small(pid, invRc), pj = pid - pi * Rc;
        const float nn = fmaxf(s1[pi * q1] + s2[pj * q2] - 2.f * Ts[pi * q1 * WLDT + pj * q2], 0.f);
        KK[pid] = s * expf(-0.5f * nn);
    }
    __syncthreads();
    const int ngrp = WNT / Tc;                          // row groups: thread (rg, c) walks column c over the rows rg, rg + ngrp, ...
    const int c = threadIdx.x % Tc, rg = threadIdx.x / Tc;
    if (rg < ngrp && c < cols) {
        const int rj = fdiv_small(c, invq2);
        const int c0 = rj * q2, b = c - c0;
        const float s2c = s2[c];
        float* optr = out + (int64_t)(row0 + rg) * ld + col0 + c;
        const int64_t ostep = (int64_t)ngrp * ld;
        int ri = fdiv_small(rg, invq1);
        int a = rg - ri * q1;
        const int da = ngrp % q1, di = ngrp / q1;
        for (int r = rg; r < rows; r += ngrp) {
            const int r0 = r - a;
            const float k = KK[ri * Rc + rj];
            const float t = Ts[r * WLDT + c];
            const float u = s1[r] - Ts[r * WLDT + c0];              // r . v1_a   (a >= 1)
            const float w = Ts[r0 * WLDT + c] - s2c;                // r . v2_b   (b >= 1)
            const float f0 = b ? (w * il) : 1.f;
            const float f1 = b ? ((t - u * w) * il2) : (-u * il);
            *optr = (a ? f1 : f0) * k;
            optr += ostep;
            a += da; ri += di;
            if (a >= q1) { a -= q1; ++ri; }
        }
    }
}

}  // namespace

extern "C" int dsvgp_kernel_fwd_rect(dsvgp_ctx* ctx, const float* P1, const float* self1, int n1, int p1, const float* P2,
                                     const float* self2, int n2, int p2, int d, const float* hyp, float* out, int64_t ld) {
    if (!ctx || !P1 || !self1 || !P2 || !self2 || !hyp || !out) return DSVGP_EINVAL;
    if (n1 <= 0 || n2 <= 0 || d < 1 || p1 < 0 || p2 < 0 || p1 + 1 > WTMAX || p2 + 1 > WTMAX) return DSVGP_EINVAL;
    const int q1 = p1 + 1, q2 = p2 + 1;
    if ((int64_t)n1 * q1 > INT_MAX || (int64_t)n2 * q2 > INT_MAX) return DSVGP_EINVAL;
    const int n1q = n1 * q1, n2q = n2 * q2;
    if (ld < n2q) return DSVGP_EINVAL;
    if (((uintptr_t)P1 | (uintptr_t)P2) % 16) return DSVGP_EINVAL;         // the packed rows are read 16 bytes at a time
    const int DP = dsvgp_packed_width(d), K4 = DP - 4;
    const int R1 = WTMAX / q1;
    const int Rr = R1 >= 2 ? R1 / 2 : R1, Rc = WTMAX / q2;                  // (row tiles of half as many points, as wide_tiles)
    const int Tr = Rr * q1, Tc = Rc * q2, Trp = (Tr + 15) & ~15, Tcp = (Tc + 15) & ~15;
    const size_t lds = sizeof(float) * (wide_union_floats(Trp, Tcp) + Trp + Tcp + (size_t)Rr * Rc);
    const int gy = cdiv(n1q, Tr);
    if (gy > 65535) return DSVGP_EINVAL;
    (void)hipFuncSetAttribute((const void*)kernel_fwd_rect_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel_fwd_rect_kernel, dim3(cdiv(n2q, Tc), gy), dim3(WNT), lds, ctx->stream, P1, self1, n1q, q1, Rr, P2, self2,
                       n2q, q2, Rc, K4, DP, hyp, out, ld);
    DSVGP_LAUNCH_CHECK();
    return 0;
}
