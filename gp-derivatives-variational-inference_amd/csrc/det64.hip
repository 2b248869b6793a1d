// Fixed-order sums of the float64 model mode under dsvgp_set_deterministic, and the size of the scratch they need.
//
// By default the fp64 kernels add their per-workgroup partial sums with fp64 atomics: the rounding of such a sum depends on the order
// in which the workgroups retire.  With ctx->det_slab set every such kernel stores its partial to the caller's scratch instead (plain
// vector stores; a null partials pointer selects the atomic epilogue, so the default mode's code is what it was), and one of the two
// passes below adds the partials in an order that depends on the launch geometry alone.
#include "common.h"

namespace {

// out[j] = sum_s parts[s][j], s ascending: one thread per element (column sums over row chunks, dP1 slabs over sweep groups)
__global__ __launch_bounds__(256) void det_sum_rows64_kernel(const double* __restrict__ parts, int ns, int64_t n, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int k = 0; k < ns; ++k) s += parts[(int64_t)k * n + j];
    out[j] = s;
}

// out[c] += sum_i parts[i][c]: workgroup c; thread t adds i = t, t + 256, ... in ascending order, the 256 chains meet in a fixed tree
__global__ __launch_bounds__(256) void det_sum_scalars64_kernel(const double* __restrict__ parts, int n, int nc, double* __restrict__ out) {
    __shared__ double red[256];
    const int c = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n; i += 256) s += parts[(int64_t)i * nc + c];
    red[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) out[c] += red[0];
}

}  // namespace

int launch_det_sum_rows64(hipStream_t st, const double* parts, int ns, int64_t n, double* out) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(det_sum_rows64_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, parts, ns, n, out);
    DSVGP_LAUNCH_CHECK();
    return 0;
}
int launch_det_sum_scalars64(hipStream_t st, const double* parts, int n, int nc, double* out) {
    if (n <= 0 || nc <= 0) return 0;
    hipLaunchKernelGGL(det_sum_scalars64_kernel, dim3(nc), dim3(256), 0, st, parts, n, nc, out);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t dsvgp_deterministic_f64_scratch_bytes(int M, int d, int p, int B) {
    if (M <= 0 || d <= 0 || p < 0 || p > 95 || B <= 0) return 0;
    const int64_t q = p + 1, Mp = M * q, Bp = B * q;
    if (Mp > INT32_MAX || Bp > INT32_MAX) return 0;
    const size_t D8 = sizeof(double);
    auto up = [](size_t a, size_t b) { return a > b ? a : b; };
    size_t need = (size_t)1 << 20;
    need = up(need, (size_t)5 * D8 * Mp * (Mp + 4));                     // five split-K slabs of an [M', M' + 1] product (as the float32 mode)
    need = up(need, (size_t)2 * 64 * D8 * Bp);                           // column sums over B': mu and cs partial rows of up to 64 row chunks
    need = up(need, (size_t)2 * D8 * Mp);                                // tvar / KL partials per row of L_S
    need = up(need, (size_t)2 * D8 * (size_t)cdiv((int64_t)M * (B > M ? B : M), 256));     // d_hyp partials of the register path's transform
    need = up(need, (size_t)5 * D8 * 256);                               // likelihood sums
    if (p > 16) {                                                        // tiled backward: one dP1 slab per sweep group + d_hyp partials
        need = up(need, kernel_bwd64_tiled_det_bytes(M, B, d, p));
        need = up(need, kernel_bwd64_tiled_det_bytes(M, M, d, p));
    }
    return (need + 255) / 256 * 256;
}
