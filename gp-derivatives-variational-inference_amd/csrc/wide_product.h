// The K-looped operand product of the wide-input assembly kernels (assemble_wide.hip): T = P1 P2^T per
// workgroup tile on v_mfma_f32_16x16x4_f32, over fixed 32-column chunks staged through LDS.
#pragma once
#include "common.h"

namespace {

constexpr int WNT = 256;            // threads per workgroup (4 waves)
constexpr int WTMAX = 96;           // tile rows / columns of the interleaved matrix (as assemble.hip)
constexpr int WLDT = 100;           // LDS row stride of the T / Tbar tiles
constexpr int WKC = 32;             // packed columns per K-loop chunk
constexpr int WLDK = WKC + 1;       // LDS row stride of a staged chunk
constexpr int WMAXT = (WTMAX / 16) * (WTMAX / 16) / 4;      // 16x16 T tiles per wave, worst case (96 x 96 tile): 9
constexpr int WPV = (2 * WTMAX * (WKC / 4) + WNT - 1) / WNT;  // 4-wide chunk loads per thread: 6

using f4 = float __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int fdiv_small(int e, float inv) { return (int)(((float)e + 0.5f) * inv); }

// T[Trp x Tcp] = P1[row0 + r] . P2[col0 + c] (r < nr, c < nc; zero outside) into Ts (row stride WLDT).  `buf` holds the staged
// chunk images, (Trp + Tcp) x WLDK floats, and may alias Ts: T is written after the last chunk has been consumed.  Wave w owns the
// 16x16 tiles w, w + 4, ...; their accumulators live in registers over the whole K loop, the next chunk's loads are in flight while
// the current one is multiplied.  Ends with a barrier (Ts complete).
__device__ __forceinline__ void wide_T(float* Ts, float* buf, const float* __restrict__ P1, int row0, int nr,
                                       const float* __restrict__ P2, int col0, int nc, int Trp, int Tcp, int K4, int DP) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntc = Tcp >> 4, nt = (Trp >> 4) * ntc;
    float* As = buf;
    float* Bs = buf + Trp * WLDK;
    const int nvec = (Trp + Tcp) * (WKC / 4);
    f4 pre[WPV];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < WPV; ++i) {
            const int e = tid + i * WNT;
            const int r = e >> 3, k = k0 + (e & 7) * 4;
            f4 v = {0.f, 0.f, 0.f, 0.f};
            if (e < nvec && k < K4) {
                if (r < Trp) { if (r < nr) v = *reinterpret_cast<const f4*>(P1 + (int64_t)(row0 + r) * DP + k); }
                else if (r - Trp < nc) v = *reinterpret_cast<const f4*>(P2 + (int64_t)(col0 + r - Trp) * DP + k);
            }
            pre[i] = v;
        }
    };
    f4 acc[WMAXT];
#pragma unroll
    for (int i = 0; i < WMAXT; ++i) acc[i] = f4{0.f, 0.f, 0.f, 0.f};
    load(0);
    for (int k0 = 0; k0 < K4; k0 += WKC) {
        __syncthreads();                    // the previous chunk's MFMA reads are done
#pragma unroll
        for (int i = 0; i < WPV; ++i) {
            const int e = tid + i * WNT;
            if (e < nvec) {
                const int r = e >> 3, c = (e & 7) * 4;
                float* dst = buf + r * WLDK + c;          // (As and Bs are contiguous: row r of the stacked image)
#pragma unroll
                for (int t = 0; t < 4; ++t) dst[t] = pre[i][t];
            }
        }
        __syncthreads();
        if (k0 + WKC < K4) load(k0 + WKC);
        const int kn = min(WKC, K4 - k0);
#pragma unroll
        for (int i = 0; i < WMAXT; ++i) {
            const int id = wave + 4 * i;
            if (id < nt) {
                const int tr = id / ntc, tc = id - tr * ntc;
                const float* pa = As + (tr * 16 + (lane & 15)) * WLDK + (lane >> 4);
                const float* pb = Bs + (tc * 16 + (lane & 15)) * WLDK + (lane >> 4);
                f4 a4 = acc[i];
                for (int kk = 0; kk < kn; kk += 4) a4 = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[kk], pb[kk], a4, 0, 0, 0);
                acc[i] = a4;
            }
        }
    }
    __syncthreads();                        // Ts may overlay the chunk images
#pragma unroll
    for (int i = 0; i < WMAXT; ++i) {
        const int id = wave + 4 * i;
        if (id < nt) {
            const int tr = id / ntc, tc = id - tr * ntc;
#pragma unroll
            for (int r = 0; r < 4; ++r) Ts[(tr * 16 + (lane >> 4) * 4 + r) * WLDT + tc * 16 + (lane & 15)] = acc[i][r];
        }
    }
    __syncthreads();
}

__host__ __device__ inline size_t wide_union_floats(int Trp, int Tcp) {
    const size_t a = (size_t)(Trp + Tcp) * WLDK, b = (size_t)Trp * WLDT;
    return ((a > b ? a : b) + 3) & ~(size_t)3;
}

}  // namespace
