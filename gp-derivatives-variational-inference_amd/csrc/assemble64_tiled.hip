// Tiled fp64 assembly of the directional-derivative kernel matrix, gfx950: the formulation of assemble64.hip (header comment
// there) on the packs of dsvgp_pack_points_f64, with the contractions on v_mfma_f64_16x16x4_f64 INSIDE the assembly kernels --
// T = P1 P2^T never reaches HBM -- and the directions of a micro-block in LDS instead of per-thread arrays: any p <= 95.
//
// Tiles: R x R whole micro-blocks, R = 64 / q for q = p + 1 <= 64 and 1 above (tile edge Tt = R q <= 96, padded to Tp = multiple
// of 16 for the MFMA).  T of a tile is accumulated over a K loop of 16-column chunks of the packed rows staged through LDS, so
// the workgroup's LDS does not grow with d.
//
// Forward, one launch: T tile -> LDS, pair values k = s exp(-|r|^2 / 2) once per micro-block, transform per entry (one wave
// per tile row, lanes along the columns: coalesced stores), K written once.
// Backward, one tile launch + the points launch of assemble64.hip: a workgroup owns one tile row and sweeps S column tiles;
// per tile it recomputes T, reads the upstream tile Gbar once into LDS, forms Tbar in place of T:
//   phase 0  k, u_a = alpha_a - T_a0, w_b = T_0b - beta_b of every micro-block
//   phase 1  row sums  gw_a = sum_b G_ab w_b, gt_a = sum_b G_ab T_ab  -> Tbar_a0;  column sums wbar_b = sum_a G_ab u_a -> Tbar_0b
//   phase 2  per micro-block: Tbar_00 = k q and the two hyper-parameter partials
//   phase 3  Tbar_ab = k G_ab / ell^2
//   phase 4  dP1[tile rows, :] += Tbar [P2 | indicator] on the MFMA, 64 packed columns at a time; the accumulators stay in
//            registers across the sweep when the packed width is <= 64, and meet in fp64 vector atomics on the zeroed
//            dP1[n1 q, DP] workspace (run-order rounding: the default).
// Deterministic mode (dsvgp_set_deterministic): every sweep group owns one slab [n1 q][DP] of the caller's scratch and writes it with
// plain stores -- once at the end of its sweep when the accumulators stay in registers, tile by tile in column order (its own earlier
// value read back and added to) at packed widths above 64 -- and its two hyper-parameter partials go to partials[workgroup][2]; a
// fixed-order pass (det64.hip) adds the slabs in sweep order into dP1 for the points launch.  A scratch too small for all slabs takes
// longer sweeps, down to one workgroup per tile row writing dP1 itself.
// fp64 MFMA layouts: A[m = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15], C/D row = (lane >> 4) + 4 reg, col = lane & 15.
#include <limits.h>

#include "common.h"

namespace {

constexpr int NT = 256;             // threads per workgroup (4 waves)
constexpr int QMAX = 96;            // largest micro-block (the float32 bound)
constexpr int KC = 16;              // packed columns per K-loop chunk
constexpr int LDK = KC + 2;         // LDS row stride of a staged chunk: 18 m + k hits 32 distinct 8-byte banks per half wave
constexpr int MAXT = (QMAX / 16) * (QMAX / 16) / 4;         // 16 x 16 T tiles per wave, worst case: 9
constexpr int PV = (2 * QMAX * (KC / 2) + NT - 1) / NT;     // 2-wide chunk loads per thread: 6
constexpr int NCH = 64;             // packed columns per step of the dP1 contraction
constexpr int LDB = NCH + 16;       // its LDS row stride (80 k + n: conflict-free fragment reads)
constexpr int MAXD = (QMAX / 16) * (NCH / 16) / 4;          // 16 x 16 dP1 tiles per wave: 6
constexpr int GB = QMAX / 16;                               // 16 x 16 pieces of the upstream tile per thread and direction: 6
constexpr int BV = QMAX * NCH / NT;                         // values of a [P2 | indicator] chunk per thread: 24

using acc4 = double __attribute__((ext_vector_type(4)));

struct Geo { int R, Tt, Tp, LDT; };
__host__ __device__ inline Geo geo_of(int q) {
    Geo g;
    g.R = q <= 64 ? 64 / q : 1;
    g.Tt = g.R * q;
    g.Tp = (g.Tt + 15) & ~15;
    g.LDT = g.Tp + 2;               // (Tp + 2) m + k: conflict-free A-fragment reads of Tbar
    return g;
}
__host__ __device__ inline size_t umax(size_t a, size_t b) { return a > b ? a : b; }

// T[Tp x Tp] = P1[row0 + r] . P2[col0 + c] (r < nr, c < nc; zero outside) into Ts (row stride LDT).  `buf` holds the staged chunk
// images, 2 Tp x LDK doubles, and may alias Ts: T is written after the last chunk has been consumed.  Wave w owns the 16 x 16
// tiles w, w + 4, ...; the next chunk's loads are in flight while the current one is multiplied.  Ends with a barrier.
__device__ __forceinline__ void tile_T(double* Ts, int LDT, double* buf, const double* __restrict__ P1, int row0, int nr,
                                       const double* __restrict__ P2, int col0, int nc, int Tp, int K4, int DP) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntc = Tp >> 4, nt = ntc * ntc;
    const double* As = buf;
    const double* Bs = buf + Tp * LDK;
    const int nvec = 2 * Tp * (KC / 2);
    double pre[PV][2];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < PV; ++i) {
            const int e = tid + i * NT;
            const int r = e >> 3, k = k0 + (e & 7) * 2;
            double v0 = 0.0, v1 = 0.0;
            if (e < nvec && k < K4) {
                const double* src = nullptr;
                if (r < Tp) { if (r < nr) src = P1 + (int64_t)(row0 + r) * DP + k; }
                else if (r - Tp < nc) src = P2 + (int64_t)(col0 + r - Tp) * DP + k;
                if (src) { v0 = src[0]; v1 = src[1]; }
            }
            pre[i][0] = v0; pre[i][1] = v1;
        }
    };
    acc4 acc[MAXT];
#pragma unroll
    for (int i = 0; i < MAXT; ++i) acc[i] = acc4{0.0, 0.0, 0.0, 0.0};
    load(0);
    for (int k0 = 0; k0 < K4; k0 += KC) {
        __syncthreads();                    // the previous users of buf are done
#pragma unroll
        for (int i = 0; i < PV; ++i) {
            const int e = tid + i * NT;
            if (e < nvec) {
                double* dst = buf + (e >> 3) * LDK + (e & 7) * 2;      // (As and Bs are contiguous: row r of the stacked image)
                dst[0] = pre[i][0]; dst[1] = pre[i][1];
            }
        }
        __syncthreads();
        if (k0 + KC < K4) load(k0 + KC);
        const int kn = min(KC, K4 - k0);
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            const int id = wave + 4 * i;
            if (id < nt) {
                const int tr = id / ntc, tc = id - tr * ntc;
                const double* pa = As + (tr * 16 + (lane & 15)) * LDK + (lane >> 4);
                const double* pb = Bs + (tc * 16 + (lane & 15)) * LDK + (lane >> 4);
                acc4 a4 = acc[i];
                for (int kk = 0; kk < kn; kk += 4) a4 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kk], pb[kk], a4, 0, 0, 0);
                acc[i] = a4;
            }
        }
    }
    __syncthreads();                        // Ts may overlay the chunk images
#pragma unroll
    for (int i = 0; i < MAXT; ++i) {
        const int id = wave + 4 * i;
        if (id < nt) {
            const int tr = id / ntc, tc = id - tr * ntc;
#pragma unroll
            for (int r = 0; r < 4; ++r) Ts[(tr * 16 + (lane >> 4) + 4 * r) * LDT + tc * 16 + (lane & 15)] = acc[i][r];
        }
    }
    __syncthreads();
}

__host__ __device__ inline size_t fwd_union(const Geo& g) { return umax((size_t)g.Tp * g.LDT, (size_t)2 * g.Tp * LDK); }
inline size_t fwd_lds_bytes(int q) {
    const Geo g = geo_of(q);
    const size_t dbl = fwd_union(g) + 2 * (size_t)g.Tp + (q > 1 ? (size_t)g.R * g.R : 0);
    return dbl * sizeof(double) + (size_t)g.Tp * sizeof(int);
}

// ---- forward ------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void kernel_fwd64_tiled_kernel(const double* __restrict__ P1, const double* __restrict__ self1, int n1q,
                                                               const double* __restrict__ P2, const double* __restrict__ self2, int n2q,
                                                               int q, int ntc, int K4, int DP, const double* __restrict__ hyp,
                                                               double jitter, double* __restrict__ out, int64_t ld) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const Geo g = geo_of(q);
    const int Tt = g.Tt, Tp = g.Tp, LDT = g.LDT, R = g.R;
    double* Ts = smem;                                  // [Tp][LDT], over the chunk images
    double* s1 = smem + fwd_union(g);
    double* s2 = s1 + Tp;
    double* KK = s2 + Tp;                               // R * R pair values (q > 1)
    int* pjc = (int*)(KK + (q > 1 ? R * R : 0));        // column -> micro-block column
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tr = blockIdx.x / ntc, tc = blockIdx.x - tr * ntc;
    const int row0 = tr * Tt, col0 = tc * Tt;
    const int rows = min(Tt, n1q - row0), cols = min(Tt, n2q - col0);
    for (int r = tid; r < Tp; r += NT) {
        s1[r] = r < rows ? self1[row0 + r] : 0.0;
        s2[r] = r < cols ? self2[col0 + r] : 0.0;
        pjc[r] = r / q;
    }
    tile_T(Ts, LDT, smem, P1, row0, rows, P2, col0, cols, Tp, K4, DP);

    const double ell = hyp[0], s = hyp[1];
    const double il = 1.0 / ell, il2 = il * il;
    if (q == 1) {
        for (int r = wave; r < rows; r += 4)
            for (int c = lane; c < cols; c += 64) {
                const double nn = fmax(s1[r] + s2[c] - 2.0 * Ts[r * LDT + c], 0.0);       // covar_dist clamps at 0
                out[(int64_t)(row0 + r) * ld + col0 + c] = s * exp(-0.5 * nn) + ((jitter != 0.0 && row0 + r == col0 + c) ? jitter : 0.0);
            }
        return;
    }
    for (int pid = tid; pid < R * R; pid += NT) {
        const int pi = pid / R, pj = pid - pi * R;
        const double nn = fmax(s1[pi * q] + s2[pj * q] - 2.0 * Ts[pi * q * LDT + pj * q], 0.0);
        KK[pid] = s * exp(-0.5 * nn);                   // postprocess_rbf, ScaleKernel
    }
    __syncthreads();
    for (int r = wave; r < rows; r += 4) {
        const int pi = r / q, a = r - pi * q;
        const double* trow = Ts + r * LDT;
        const double* t0 = Ts + pi * q * LDT;
        for (int c = lane; c < cols; c += 64) {
            const int pj = pjc[c], c0 = pj * q, b = c - c0;
            const double k = KK[pi * R + pj];
            double v;
            if (a == 0) {
                v = b == 0 ? k : (t0[c] - s2[c]) * k * il;                                 // w_b k / ell
            } else {
                const double u = s1[r] - trow[c0];                                         // r . v1_a
                v = b == 0 ? -u * k * il : (trow[c] - u * (t0[c] - s2[c])) * k * il2;
            }
            if (jitter != 0.0 && row0 + r == col0 + c) v += jitter;
            out[(int64_t)(row0 + r) * ld + col0 + c] = v;
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------
__host__ __device__ inline size_t bwd_gs(const Geo& g) { return (size_t)g.Tp * umax((size_t)g.LDT, umax((size_t)2 * LDK, (size_t)LDB)); }
inline size_t bwd_lds_bytes(int q) {
    const Geo g = geo_of(q);
    size_t dbl = (size_t)g.Tp * g.LDT + bwd_gs(g) + 2 * (size_t)g.Tp;
    if (q > 1) dbl += (size_t)g.R * g.R + 3 * (size_t)g.R * g.Tt;
    return dbl * sizeof(double) + (size_t)g.Tp * sizeof(int) + 2 * 4 * sizeof(double);
}

__global__ __launch_bounds__(NT) void kernel_bwd64_tiled_kernel(const double* __restrict__ G, int64_t ldg, const double* __restrict__ P1,
                                                               const double* __restrict__ self1, int n1q,
                                                               const double* __restrict__ P2, const double* __restrict__ self2, int n2q,
                                                               int q, int ntc, int sweep, int nsg, int K4, int DP,
                                                               const double* __restrict__ hyp, double* __restrict__ dP,
                                                               double* __restrict__ d_hyp, int64_t slab_stride,
                                                               double* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const Geo g = geo_of(q);
    const int Tt = g.Tt, Tp = g.Tp, LDT = g.LDT, R = g.R;
    double* Ts = smem;                                  // [Tp][LDT]: T, then Tbar
    double* Gs = Ts + (size_t)Tp * LDT;                 // the upstream tile; before it the chunk images of T, after it the [P2 | indicator] chunk
    double* s1 = Gs + bwd_gs(g);
    double* s2 = s1 + Tp;
    double* KK = s2 + Tp;                               // [R][R]        pair values
    double* U = KK + (q > 1 ? R * R : 0);               // [R (pj)][Tt]  u_a = r . v1_a
    double* RW = U + (q > 1 ? R * Tt : 0);              // [R (pj)][Tt]  row sums: a = 0 first-order term, a > 0 second-order term
    double* Wt = RW + (q > 1 ? R * Tt : 0);             // [R (pi)][Tt]  w_b = r . v2_b
    double* red = Wt + (q > 1 ? R * Tt : 0);            // [2][4]
    int* pjc = (int*)(red + 8);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tr = blockIdx.x / nsg, sg = blockIdx.x - tr * nsg;
    const int row0 = tr * Tt;
    const int rows = min(Tt, n1q - row0);
    const double ell = hyp[0], s = hyp[1];
    const double il = 1.0 / ell, il2 = il * il;
    for (int r = tid; r < Tp; r += NT) {
        s1[r] = r < rows ? self1[row0 + r] : 0.0;
        pjc[r] = r / q;
    }
    const bool keep = DP <= NCH;                        // dP1 accumulators live in registers across the sweep
    double* const slab = partials ? dP + (int64_t)sg * slab_stride : nullptr;      // deterministic mode: this sweep group's own dP1
    const int mt = Tp >> 4;
    acc4 acc[MAXD];
#pragma unroll
    for (int i = 0; i < MAXD; ++i) acc[i] = acc4{0.0, 0.0, 0.0, 0.0};
    double ds = 0.0, dl = 0.0;
    const int ct0 = sg * sweep, ct1 = min(ntc, ct0 + sweep);
    for (int ct = ct0; ct < ct1; ++ct) {
        const int col0 = ct * Tt;
        const int cols = min(Tt, n2q - col0);
        for (int c = tid; c < Tp; c += NT) s2[c] = c < cols ? self2[col0 + c] : 0.0;
        // the upstream tile: all loads of a thread issued before T is computed (16 x 16 pieces, 128-byte row segments), stored behind it
        double greg[GB * GB];
#pragma unroll
        for (int jr = 0; jr < GB; ++jr)
#pragma unroll
            for (int jc = 0; jc < GB; ++jc) {
                const int r = jr * 16 + (tid >> 4), c = jc * 16 + (tid & 15);
                greg[jr * GB + jc] = (jr < mt && jc < mt && r < rows && c < cols) ? G[(int64_t)(row0 + r) * ldg + col0 + c] : 0.0;
            }
        tile_T(Ts, LDT, Gs, P1, row0, rows, P2, col0, cols, Tp, K4, DP);
#pragma unroll
        for (int jr = 0; jr < GB; ++jr)
#pragma unroll
            for (int jc = 0; jc < GB; ++jc)
                if (jr < mt && jc < mt) Gs[(jr * 16 + (tid >> 4)) * LDT + jc * 16 + (tid & 15)] = greg[jr * GB + jc];
        // ... and the first chunk of [P2 | indicator], in flight under the transform phases
        double breg[BV];
        auto load_chunk = [&](int n0) {
#pragma unroll
            for (int i = 0; i < BV; ++i) {
                const int e = tid + i * NT, c = e >> 6, n = n0 + (e & 63);
                breg[i] = (c < cols && n < DP) ? P2[(int64_t)(col0 + c) * DP + n] : 0.0;
            }
        };
        load_chunk(0);
        if (q == 1) {
            __syncthreads();
            for (int r = wave; r < Tt; r += 4)
                for (int c = lane; c < Tt; c += 64) {
                    const double nn = fmax(s1[r] + s2[c] - 2.0 * Ts[r * LDT + c], 0.0);
                    const double kg = s * exp(-0.5 * nn) * Gs[r * LDT + c];
                    Ts[r * LDT + c] = kg;               // Tbar_00 = k q
                    ds += kg / s;
                    dl += kg * nn * il;
                }
        } else {
            // phase 0
            for (int pid = tid; pid < R * R; pid += NT) {
                const int pi = pid / R, pj = pid - pi * R;
                const double nn = fmax(s1[pi * q] + s2[pj * q] - 2.0 * Ts[pi * q * LDT + pj * q], 0.0);
                KK[pid] = s * exp(-0.5 * nn);
            }
            for (int e = tid; e < R * Tt; e += NT) {
                const int pp = e / Tt, x = e - pp * Tt;                 // (pj, r) for U, (pi, c) for Wt
                U[e] = s1[x] - Ts[x * LDT + pp * q];
                Wt[e] = Ts[pp * q * LDT + x] - s2[x];
            }
            __syncthreads();
            // phase 1: rows (r, pj), then columns (pi, c)
            for (int e = tid; e < R * Tt; e += NT) {
                const int pj = e / Tt, r = e - pj * Tt;
                const int pi = pjc[r], a = r - pi * q, c0 = pj * q;
                const double* grow = Gs + r * LDT + c0;
                const double* trow = Ts + r * LDT + c0;
                const double* w = Wt + pi * Tt + c0;
                double gw = 0.0, gt = 0.0;
                for (int b = 1; b < q; ++b) {
                    const double gab = grow[b];
                    gw = fma(gab, w[b], gw);
                    gt = fma(gab, trow[b], gt);
                }
                if (a == 0) {
                    RW[e] = gw;                                         // sum_b G0b w_b
                } else {
                    RW[e] = gt - U[e] * gw;                             // sum_b Gab (T_ab - u_a w_b)
                    Ts[r * LDT + c0] = KK[pi * R + pj] * (grow[0] * il + gw * il2);     // Tbar_a0 = -ubar_a
                }
            }
            for (int e = tid; e < R * Tt; e += NT) {
                const int pi = e / Tt, c = e - pi * Tt;
                const int pj = pjc[c], b = c - pj * q;
                if (b == 0) continue;
                const double* u = U + pj * Tt + pi * q;
                const double* gcol = Gs + pi * q * LDT + c;
                double wbar = 0.0;
                for (int a = 1; a < q; ++a) wbar = fma(gcol[a * LDT], u[a], wbar);    // sum_a Gab u_a
                Ts[pi * q * LDT + c] = KK[pi * R + pj] * (gcol[0] * il - wbar * il2);   // Tbar_0b = wbar_b
            }
            __syncthreads();
            // phase 2: one micro-block per thread (small q) or per wave (q >= 16)
            const bool per_wave = q >= 16;
            for (int pid = per_wave ? wave : tid; pid < R * R; pid += per_wave ? 4 : NT) {
                const int pi = pid / R, pj = pid - pi * R;
                const int r0 = pi * q, c0 = pj * q;
                const double* u = U + pj * Tt + r0;
                const double* rw = RW + pj * Tt + r0;
                const double* w = Wt + pi * Tt + c0;
                double hess = 0.0, second = 0.0, dots = 0.0;
                for (int a = per_wave ? 1 + lane : 1; a < q; a += per_wave ? 64 : 1) {
                    hess += rw[a];
                    second = fma(Gs[(r0 + a) * LDT + c0], u[a], second);
                    dots = fma(-Ts[(r0 + a) * LDT + c0], u[a], dots);   // ubar_a u_a
                }
                for (int b = per_wave ? 1 + lane : 1; b < q; b += per_wave ? 64 : 1) dots = fma(Ts[r0 * LDT + c0 + b], w[b], dots);
                if (per_wave) {
                    for (int off = 32; off > 0; off >>= 1) {
                        hess += __shfl_down(hess, off);
                        second += __shfl_down(second, off);
                        dots += __shfl_down(dots, off);
                    }
                }
                if (!per_wave || lane == 0) {
                    const double first = rw[0];
                    const double nn = fmax(s1[r0] + s2[c0] - 2.0 * Ts[r0 * LDT + c0], 0.0);
                    const double k = KK[pid];
                    const double qq = Gs[r0 * LDT + c0] + first * il - second * il + hess * il2;       // dL/dk
                    Ts[r0 * LDT + c0] = k * qq;                         // Tbar_00 = -2 nn-bar
                    ds += k * qq / s;                                   // <Gbar, K> / s
                    // d ell: -(rbar . r)/ell - (sum G0b K0b + sum Ga0 Ka0)/ell - 2 sum Gab Kab / ell,  rbar . r = -k q |r|^2 + dots
                    dl += -(-k * qq * nn + dots) * il - k * (first * il - second * il) * il - 2.0 * k * hess * il2 * il;
                }
            }
            __syncthreads();
            // phase 3
            for (int r = wave; r < Tt; r += 4) {
                const int pi = r / q;
                if (r == pi * q) continue;
                for (int c = lane; c < Tt; c += 64) {
                    const int pj = pjc[c];
                    if (c != pj * q) Ts[r * LDT + c] = KK[pi * R + pj] * il2 * Gs[r * LDT + c];
                }
            }
        }
        // phase 4: dP1[tile rows, :] += Tbar [P2 | indicator]
        for (int n0 = 0; n0 < DP; n0 += NCH) {
            __syncthreads();                            // Tbar complete; Gs / the previous chunk are free
            const int ncol = min(NCH, DP - n0);
            if (n0) load_chunk(n0);
#pragma unroll
            for (int i = 0; i < BV; ++i) {
                const int e = tid + i * NT;
                if (e < Tp * NCH) Gs[(e >> 6) * LDB + (e & 63)] = breg[i];
            }
            __syncthreads();
            const int ntn = (ncol + 15) >> 4, ntile = mt * ntn;
            const bool last = !keep || ct == ct1 - 1;
#pragma unroll
            for (int i = 0; i < MAXD; ++i) {
                const int id = wave + 4 * i;
                if (id < ntile) {
                    const int tm = id / ntn, tn = id - tm * ntn;
                    const double* pa = Ts + (tm * 16 + (lane & 15)) * LDT + (lane >> 4);
                    const double* pb = Gs + (lane >> 4) * LDB + tn * 16 + (lane & 15);
                    acc4 a4 = acc[i];
                    for (int kk = 0; kk < Tp; kk += 4) a4 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kk], pb[kk * LDB], a4, 0, 0, 0);
                    if (last) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int m = tm * 16 + (lane >> 4) + 4 * r, n = n0 + tn * 16 + (lane & 15);
                            if (m < rows && n < DP) {
                                if (slab) {             // one writer per address: store, then (no register sweep) add in column-tile order
                                    double* dst = slab + (int64_t)(row0 + m) * DP + n;
                                    *dst = (keep || ct == ct0) ? a4[r] : *dst + a4[r];
                                } else {
                                    atomicAdd(dP + (int64_t)(row0 + m) * DP + n, a4[r]);
                                }
                            }
                        }
                        a4 = acc4{0.0, 0.0, 0.0, 0.0};
                    }
                    acc[i] = a4;
                }
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) { ds += __shfl_down(ds, off); dl += __shfl_down(dl, off); }
    __syncthreads();
    if (lane == 0) { red[wave] = ds; red[4 + wave] = dl; }
    __syncthreads();
    if (tid == 0) {
        const double vs = red[0] + red[1] + red[2] + red[3];            // d outputscale
        const double vl = red[4] + red[5] + red[6] + red[7];            // d lengthscale
        if (partials) { partials[2 * (int64_t)blockIdx.x] = vl; partials[2 * (int64_t)blockIdx.x + 1] = vs; }
        else { atomicAdd(&d_hyp[1], vs); atomicAdd(&d_hyp[0], vl); }
    }
}

inline bool misaligned8(const void* p) { return ((uintptr_t)p & 7) != 0; }
inline bool bad_geometry(int n1, int n2, int d, int p) {
    if (n1 < 0 || n2 < 0 || d <= 0 || p < 0 || p >= QMAX) return true;
    const int64_t q = p + 1;
    return n1 * q > INT_MAX || n2 * q > INT_MAX || d > INT_MAX - 8;
}

}  // namespace

extern "C" int dsvgp_kernel_fwd_f64(dsvgp_ctx* ctx, const double* P1, const double* self1, int n1, const double* P2,
                                    const double* self2, int n2, int d, int p, const double* hyp, double jitter, int symmetric,
                                    double* out, int64_t ld) {
    if (!ctx || !hyp || bad_geometry(n1, n2, d, p) || ld < (int64_t)n2 * (p + 1) || !(jitter == jitter)) return DSVGP_EINVAL;
    if (symmetric && n1 != n2) return DSVGP_EINVAL;
    if (n1 == 0 || n2 == 0) return 0;
    if (!P1 || !self1 || !P2 || !self2 || !out) return DSVGP_EINVAL;
    if (misaligned8(P1) || misaligned8(self1) || misaligned8(P2) || misaligned8(self2) || misaligned8(hyp) || misaligned8(out)) return DSVGP_EINVAL;
    const int q = p + 1, K4 = (d + 3) & ~3, DP = K4 + 4;
    const Geo g = geo_of(q);
    const int ntr = cdiv((int64_t)n1 * q, g.Tt), ntc = cdiv((int64_t)n2 * q, g.Tt);
    if ((int64_t)ntr * ntc > INT_MAX) return DSVGP_EINVAL;
    const size_t lds = fwd_lds_bytes(q);
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel_fwd64_tiled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel_fwd64_tiled_kernel, dim3(ntr * ntc), dim3(NT), lds, ctx->stream, P1, self1, n1 * q, P2, self2, n2 * q, q, ntc,
                       K4, DP, hyp, symmetric ? jitter : 0.0, out, ld);
    DSVGP_LAUNCH_CHECK();
    return 0;
}

// deterministic mode: bytes of scratch that hold every sweep group's dP1 slab and the d_hyp partials of one backward -- an upper bound
// that does not shrink when n1 or n2 grows (the exact count does: a longer sweep can mean fewer groups).  From bwd64_tiled_sweep:
// nsg = ntc while ntr ntc < 2048, nsg <= 2048 / ntr + 2 while the sweep is below its cap of 32, nsg = ceil(ntc / 32) above.
size_t kernel_bwd64_tiled_det_bytes(int n1, int n2, int d, int p) {
    if (bad_geometry(n1, n2, d, p) || n1 == 0 || n2 == 0) return 0;
    const int q = p + 1;
    const Geo g = geo_of(q);
    const size_t n1q = (size_t)n1 * q, ntr = cdiv((int64_t)n1 * q, g.Tt), ntc = cdiv((int64_t)n2 * q, g.Tt);
    const size_t DP = (size_t)((d + 3) & ~3) + 4;
    auto lo = [](size_t a, size_t b) { return a < b ? a : b; };
    const size_t capped = (ntc + 31) / 32;
    const size_t rows = umax(lo(ntc * n1q, (size_t)2048 * g.Tt + 2 * n1q), capped * n1q);       // >= nsg n1 q
    const size_t parts = umax(lo(ntc * ntr, 2048 + 2 * ntr), capped * ntr);                       // >= nsg ntr
    return (rows * DP + 2 * parts) * sizeof(double);
}

extern "C" size_t dsvgp_kernel_bwd_f64_workspace_bytes(int n1, int n2, int d, int p) {
    if (bad_geometry(n1, n2, d, p) || n1 == 0) return 0;
    const size_t DP = (size_t)((d + 3) & ~3) + 4;
    return (size_t)n1 * (p + 1) * DP * sizeof(double);               // dP1[n1 q, DP]
}

extern "C" int dsvgp_kernel_bwd_f64(dsvgp_ctx* ctx, const double* G, int64_t ldg, const double* P1, const double* self1,
                                    const double* vnorm1, int n1, const double* P2, const double* self2, int n2, int d, int p,
                                    const double* hyp, int symmetric, double* d_x1, double* d_v1, double* d_hyp, void* workspace,
                                    size_t workspace_bytes) {
    if (!ctx || !hyp || !d_hyp || bad_geometry(n1, n2, d, p) || ldg < (int64_t)n2 * (p + 1)) return DSVGP_EINVAL;
    if (symmetric && n1 != n2) return DSVGP_EINVAL;
    if (n1 == 0 || n2 == 0) return 0;
    if (!G || !P1 || !self1 || !P2 || !self2 || !d_x1 || (p > 0 && (!vnorm1 || !d_v1)) || !workspace) return DSVGP_EINVAL;
    if (misaligned8(G) || misaligned8(P1) || misaligned8(self1) || misaligned8(P2) || misaligned8(self2) || misaligned8(hyp) ||
        misaligned8(d_x1) || misaligned8(d_v1) || misaligned8(d_hyp) || misaligned8(vnorm1) || misaligned8(workspace))
        return DSVGP_EINVAL;
    const size_t need = dsvgp_kernel_bwd_f64_workspace_bytes(n1, n2, d, p);
    if (workspace_bytes < need) return DSVGP_EINVAL;
    const int q = p + 1, K4 = (d + 3) & ~3, DP = K4 + 4;
    const Geo g = geo_of(q);
    const int ntr = cdiv((int64_t)n1 * q, g.Tt), ntc = cdiv((int64_t)n2 * q, g.Tt);
    int nsg;
    int sweep = bwd64_tiled_sweep(ntr, ntc, &nsg);
    if ((int64_t)ntr * nsg > INT_MAX) return DSVGP_EINVAL;
    double* dP = (double*)workspace;
    const size_t slab_doubles = need / sizeof(double);
    double *target = dP, *partials = nullptr;
    int64_t slab_stride = 0;
    if (ctx->det_slab) {
        // deterministic mode: slabs[nsg][n1 q][DP] | partials[ntr nsg][2] in the scratch; fewer, longer sweeps if it is small; with one
        // sweep group per tile row that workgroup is the only writer of its dP1 rows and writes them in place (never back to atomics)
        const size_t have = ctx->det_bytes / sizeof(double);
        if (((uintptr_t)ctx->det_slab & 7) || have < (size_t)2 * ntr) return DSVGP_EINVAL;
        while (nsg > 1 && (size_t)nsg * (slab_doubles + (size_t)2 * ntr) > have) {
            ++sweep;
            nsg = cdiv(ntc, sweep);
        }
        if (nsg > 1) {
            target = (double*)ctx->det_slab;
            slab_stride = (int64_t)slab_doubles;
            partials = target + (size_t)nsg * slab_doubles;
        } else {
            sweep = ntc;
            partials = (double*)ctx->det_slab;
        }
    } else {
        hipError_t e = hipMemsetAsync(dP, 0, need, ctx->stream);
        if (e != hipSuccess) return 1000 + (int)e;
    }
    const size_t lds = bwd_lds_bytes(q);
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel_bwd64_tiled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel_bwd64_tiled_kernel, dim3(ntr * nsg), dim3(NT), lds, ctx->stream, G, ldg, P1, self1, n1 * q, P2, self2, n2 * q,
                       q, ntc, sweep, nsg, K4, DP, hyp, target, d_hyp, slab_stride, partials);
    DSVGP_LAUNCH_CHECK();
    if (partials) {
        int rc = 0;
        if (nsg > 1) rc = launch_det_sum_rows64(ctx->stream, target, nsg, (int64_t)slab_doubles, dP);
        if (!rc) rc = launch_det_sum_scalars64(ctx->stream, partials, ntr * nsg, 2, d_hyp);
        if (rc) return rc;
    }
    return dsvgp_kernel_bwd_points_f64(ctx, dP, P1, vnorm1, n1, d, p, hyp, symmetric, d_x1, d_v1);
}
