// One packed row of the fp64 kernel assembly (shared by assemble64.hip's pack kernel and the one-call step's prologue, step64.hip):
// point i as the (p+1) rows [(x - c)/ell ; v_1/|v_1| ; ... ; v_p/|v_p|] of width DP (zero padded, indicator column K4 on the value row),
// self = |x~|^2 (value row) or x~ . vhat_a (direction rows), vnorm = |v_a|  (reference RBFKernelDirectionalGrad.py:57-58,67-68)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ void pack64_row(const double* __restrict__ x, const double* __restrict__ v, int row, int d, int p, double ell,
                                           const double* __restrict__ center, double* __restrict__ P, double* __restrict__ self,
                                           double* __restrict__ vnorm, int K4, int DP) {
    const int q = p + 1;
    const int i = row / q, a = row - i * q;
    double* Pr = P + (int64_t)row * DP;
    const double* xi = x + (int64_t)i * d;
    for (int k = 0; k < DP; ++k) Pr[k] = 0.0;
    if (a == 0) {
        double acc = 0.0;
        for (int k = 0; k < d; ++k) {
            const double xt = (xi[k] - (center ? center[k] : 0.0)) / ell;    // x.div(lengthscale), :67-68
            Pr[k] = xt;
            acc = fma(xt, xt, acc);
        }
        Pr[K4] = 1.0;                                   // indicator column (row sums in the backward)
        self[row] = acc;
    } else {
        const double* vi = v + ((int64_t)i * p + (a - 1)) * d;
        double ss = 0.0;
        for (int k = 0; k < d; ++k) ss = fma(vi[k], vi[k], ss);
        const double nrm = sqrt(ss);                    // :57-58
        double acc = 0.0;
        for (int k = 0; k < d; ++k) {
            const double vh = vi[k] / nrm;
            Pr[k] = vh;
            acc = fma(vh, (xi[k] - (center ? center[k] : 0.0)) / ell, acc);
        }
        self[row] = acc;
        vnorm[(int64_t)i * p + (a - 1)] = nrm;
    }
}
