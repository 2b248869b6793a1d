// The parts shared by the one-wave 48 x 48 kernels of assemble.hip: kernel_fwd_pair / _split / _canon and kernel_bwd_pair / _split
// (kernel_bwd_canon keeps its own text and shares only the LDS description on the host side: DESIGN section 29).
// ONE WAVE per workgroup (no barriers) owns R = 48 / Q points of side 1 (T = R Q <= 48 rows) and sweeps T-column tiles of side 2:
//   - the A fragments of its 48 packed side-1 rows stay in registers for the whole sweep (load_a_fragments), the self terms folded into
//     two extra packed columns:  P1'[r, K4+1] = [a == 0],  P2'[c, K4+1] = -self2[c]       =>  T'[r0, cb] = x1~.v2_b - beta_b = w_b
//                                P1'[r, K4+2] = -self1[r] [a > 0],  P2'[c, K4+2] = [b == 0]  =>  T'[ra, c0] = v1_a.x2~ - alpha_a = -u_a
//     (the canon kernels, one B column per POINT of side 2, fold only the second);
//   - the packed side-2 rows of a column tile travel through registers into an LDS image (Side2Stager);
//   - T' = P1' P2'^T on v_mfma_f32_16x16x4_f32, one straight-line copy per K depth (tprime_product), then to LDS (store_tprime);
//   - lane <-> point pair(s) (pair_geometry); a lane reads the Q x Q values of its pair (read_block) and turns them into the kernel
//     micro-block with one exp (RbfPair) -- or into Tbar, the A operand of dP1 += Tbar P2ext (dp1_product), which leaves through the
//     split slabs and the two partial sums per workgroup (flush_slab, flush_partials).
// What a kernel keeps for itself: the order of these steps and its WAVE_SYNCs, its output / upstream paths and its Tbar algebra.
// Every floating-point expression here is the text the six kernels had, operand order included: tools/tiled_ab.py --narrow compares two
// builds bit for bit.  The *Lds structs are the ONE description of each kernel pair's dynamic LDS: the kernel takes its pointers from the
// float offsets, the host its byte count from `floats`.
#pragma once
#include "common.h"
#include <type_traits>

// One-wave workgroups (64 threads) exchange through LDS, which serves a wave's instructions in issue order: all they need between a write
// and another lane's read is that the COMPILER keeps the order.  __syncthreads() would add "s_waitcnt vmcnt(0)" (its fence covers global
// memory too), i.e. drain the tile's global stores and the next tile's prefetch at every exchange (profiles/r06_c_*).
#define WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                         __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

namespace {

using f4 = float __attribute__((ext_vector_type(4)));

constexpr int FWD_PAIR_LDT = 52;   // LDS row stride of the forward's 48 x 48 T' / output tile
constexpr int PAIR_LDT = 52;       // ... of the backward's T' / Tbar tile (even: 8-byte strips) and of the split backward's upstream tile
constexpr int CAN_LDT = 52;        // ... of the canon kernels' output / U^T tile (even: 8-byte strips; 16-byte aligned rows)

// ---- dynamic LDS, in floats -------------------------------------------------------------------------
// forward pair / split: [49][K4 + 5] packed side-2 rows (row 48: scratch of the predicate-free staging), overlaid by the [48][LDT] T' tile
struct FwdPairLds {
    int p2, tt, floats;
    __host__ __device__ explicit FwdPairLds(int K4) : p2(0), tt(0), floats(49 * (K4 + 5) > 48 * FWD_PAIR_LDT ? 49 * (K4 + 5) : 48 * FWD_PAIR_LDT) {}
};
// backward pair / split: [49][NP + 1] extended side-2 packs | [48][LDT] T', then Tbar (16-byte aligned) | split: [grows][LDT] upstream tile
struct BwdPairLds {
    int p2, tt, gg, floats;
    __host__ __device__ BwdPairLds(int NP, int grows) : p2(0), tt((49 * (NP + 1) + 3) & ~3), gg(tt + 48 * PAIR_LDT), floats(gg + grows * PAIR_LDT) {}
};
// canon forward: [16][K4 + 5] side-2 value rows | [48][LDT] U^T, then the output tile
struct CanFwdLds {
    int xs, tt, floats;
    __host__ __device__ explicit CanFwdLds(int K4) : xs(0), tt((16 * (K4 + 5) + 3) & ~3), floats(tt + 48 * CAN_LDT) {}
};
// canon backward: [16][NP + 1] side-2 value rows | [16][LDT] U^T, then Tbar's value columns | [48][8] column sums | DMA: [48][48] upstream tile
struct CanBwdLds {
    int xs, tt, cs, gs, floats;
    __host__ __device__ CanBwdLds(int NP, bool dma) : xs(0), tt((16 * (NP + 1) + 3) & ~3), cs(tt + 16 * CAN_LDT), gs(cs + 48 * 8), floats(gs + (dma ? 48 * 48 : 0)) {}
};

// ---- A fragments: areg[i][ks] = P1'[row0 + 16 i + m16][4 ks + kg]  (KS <= KSM since DP <= 4 KSM) --------------
// CANON: only extension column K4 + 2
template <int Q, int KSM, bool CANON = false>
__device__ __forceinline__ void load_a_fragments(float (&areg)[3][KSM], const float* P1, const float* self1,
                                                 int row0, int n1q, int K4, int DP, int m16, int kg) {
    constexpr int T = (48 / Q) * Q;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int gr = row0 + i * 16 + m16;
        const bool ok = i * 16 + m16 < T && gr < n1q;
        const int a = (i * 16 + m16) % Q;
        const float sf = ok ? self1[gr] : 0.f;
#pragma unroll
        for (int ks = 0; ks < KSM; ++ks) {
            float v = 0.f;
            if (ks < K4 / 4) v = ok ? P1[(int64_t)gr * DP + ks * 4 + kg] : 0.f;
            else if (ks == K4 / 4 && ok) v = (!CANON && kg == 1) ? (a == 0 ? 1.f : 0.f) : ((kg == 2) ? (a == 0 ? 0.f : -sf) : 0.f);
            areg[i][ks] = v;
        }
    }
}

// ---- the packed side-2 rows of a column tile: HBM -> registers (fetch) -> LDS image [49][LDP] (store, extend) ---------
// The packed rows of a column tile are ONE contiguous piece of P2 (T rows of DP floats): float4 number e = lane + 64 u of it goes to row
// e / pch of the image.  LEAN: per-lane constants, the element index (clamped to the tile for the lanes past its end) and the LDS offset
// (those lanes write to the scratch row behind the image) -- a tile that lies inside the matrix is then fetched and staged without a
// single predicate (the guarded form spends ~15 instructions per float4 on masks, zero fills and 64-bit address arithmetic: PMC,
// profiles/r03_c_pmc_assemble_fwd_*.txt).  Not LEAN (the split kernels): the guarded fetch and a predicated store.
template <int Q, int KSM, bool LEAN>
struct Side2Stager {
    static constexpr int T = (48 / Q) * Q, NPF = (T * KSM + 63) / 64;     // float4 per lane of one tile (DP <= 4 KSM)
    const float* P2;
    const float* self2;
    int n2q, K4, DP, pch, LDP, lane;
    f4 pf[NPF];
    float pselfv = 0.f;
    int pf_e[NPF], pf_lds[NPF];
    __device__ __forceinline__ Side2Stager(const float* P2_, const float* self2_, int n2q_, int K4_, int DP_, int LDP_,
                                           int lane_) : P2(P2_), self2(self2_), n2q(n2q_), K4(K4_), DP(DP_), pch(DP_ / 4), LDP(LDP_), lane(lane_) {
        if constexpr (LEAN) {
#pragma unroll
            for (int u = 0; u < NPF; ++u) {
                const int e = lane + 64 * u;
                const int ec = min(e, T * pch - 1);
                const int r = ec / pch, k = (ec - r * pch) * 4;
                pf_e[u] = ec;
                pf_lds[u] = (e < T * pch ? r : 48) * LDP + k;
            }
        }
    }
    __device__ inline void fetch(int ct) {
        const int c0 = ct * T;
        if constexpr (LEAN) {
            if (c0 + T <= n2q) {               // a tile inside the matrix: no predicates
                const f4* src = reinterpret_cast<const f4*>(P2 + (int64_t)c0 * DP);
#pragma unroll
                for (int u = 0; u < NPF; ++u) pf[u] = src[pf_e[u]];
                pselfv = -self2[c0 + min(lane, T - 1)];
                return;
            }
        }
#pragma unroll
        for (int u = 0; u < NPF; ++u) {
            const int e = lane + 64 * u;
            const int r = e / pch, k = (e - r * pch) * 4;
            pf[u] = f4{0.f, 0.f, 0.f, 0.f};
            if (e < T * pch && c0 + r < n2q) pf[u] = *reinterpret_cast<const f4*>(P2 + (int64_t)(c0 + r) * DP + k);
        }
        pselfv = (lane < T && c0 + lane < n2q) ? -self2[c0 + lane] : 0.f;
    }
    __device__ __forceinline__ void store(float* P2s) const {
#pragma unroll
        for (int u = 0; u < NPF; ++u) {
            if constexpr (LEAN) {              // (lanes past the end of the tile: the scratch row behind the image)
#pragma unroll
                for (int t = 0; t < 4; ++t) P2s[pf_lds[u] + t] = pf[u][t];
            } else {
                const int e = lane + 64 * u, r = e / pch, k = (e - r * pch) * 4;
                if (e < T * pch) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) P2s[r * LDP + k + t] = pf[u][t];
                }
            }
        }
    }
    // the two extension columns, on top of the packed zeros (a WAVE_SYNC after store)
    __device__ __forceinline__ void extend(float* P2s, int col0) const {
        if (lane < T) {
            P2s[lane * LDP + K4 + 1] = pselfv;
            P2s[lane * LDP + K4 + 2] = (col0 + lane < n2q && lane % Q == 0) ? 1.f : 0.f;
        }
    }
};

// ---- T' = P1' P2'^T: 3 row tiles x NB column tiles of 16 x 16, K = 4 KS; pb = image + m16 * LDP + kg ---------
template <int KS_, int KSM, int NB>
__device__ inline void tprime_steps(f4 (&t)[3][NB], const float (&areg)[3][KSM], const float* pb, int LDP) {
#pragma unroll
    for (int ks = 0; ks < KS_; ++ks) {
        float bv[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) bv[j] = pb[j * 16 * LDP + ks * 4];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j)
                t[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[i][ks], bv[j], ks == 0 ? f4{0.f, 0.f, 0.f, 0.f} : t[i][j], 0, 0, 0);
    }
}
// STRAIGHT: one straight-line copy per K depth -- no per-step branches, the first product starts from the inline zero; otherwise (the
// split kernels) one predicated loop
template <int KSM, int NB, bool STRAIGHT = true>
__device__ __forceinline__ void tprime_product(f4 (&t)[3][NB], const float (&areg)[3][KSM], const float* pb, int LDP, int KS) {
    if constexpr (!STRAIGHT) {
#pragma unroll
        for (int ks = 0; ks < KSM; ++ks) {
            if (ks < KS) {
                float bv[NB];
#pragma unroll
                for (int j = 0; j < NB; ++j) bv[j] = pb[j * 16 * LDP + ks * 4];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < NB; ++j)
                        t[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[i][ks], bv[j], ks == 0 ? f4{0.f, 0.f, 0.f, 0.f} : t[i][j], 0, 0, 0);
            }
        }
    } else {
#define WT_DEPTH(n) case n: tprime_steps<n>(t, areg, pb, LDP); break;
        switch (KS) {
            WT_DEPTH(1) WT_DEPTH(2) WT_DEPTH(3) WT_DEPTH(4) WT_DEPTH(5) WT_DEPTH(6) WT_DEPTH(7) WT_DEPTH(8)
            default:
                if constexpr (KSM > 8) {
                    switch (KS) {
                        WT_DEPTH(9) WT_DEPTH(10) WT_DEPTH(11) WT_DEPTH(12) WT_DEPTH(13) WT_DEPTH(14) WT_DEPTH(15)
                        default: tprime_steps<16>(t, areg, pb, LDP); break;
                    }
                } else tprime_steps<8>(t, areg, pb, LDP);
                break;
        }
#undef WT_DEPTH
    }
}
template <int LDT2>
__device__ __forceinline__ void store_tprime(float* TT, const f4 (&t)[3][3], int m16, int kg) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) TT[(i * 16 + kg * 4 + r) * LDT2 + j * 16 + m16] = t[i][j][r];
}

// ---- lane <-> point pair(s): pair pid = lane + 64 pp = (pi, pj), micro-block origin (pr0, pc0) in the tile --------
// prow: the pair exists and its rows lie inside side 1; s1r0 = |x1~|^2 of its point
template <int Q, int PPL>
__device__ __forceinline__ void pair_geometry(int (&pr0)[PPL], int (&pc0)[PPL], bool (&prow)[PPL], float (&s1r0)[PPL],
                                              const float* self1, int row0, int n1q, int lane) {
    constexpr int R = 48 / Q, NPAIR = R * R;
#pragma unroll
    for (int pp = 0; pp < PPL; ++pp) {
        const int pid = lane + 64 * pp;
        const int pi = pid / R, pj = pid - pi * R;
        pr0[pp] = pi * Q; pc0[pp] = pj * Q;
        prow[pp] = pid < NPAIR && row0 + pr0[pp] < n1q;
        s1r0[pp] = prow[pp] ? self1[row0 + pr0[pp]] : 0.f;
    }
}

// ---- one row strip of a micro-block in LDS (8-byte strips for even Q) and the whole Q x Q block ----------------
template <int Q>
__device__ __forceinline__ void read_strip(float (&v)[Q], const float* p) {
    if constexpr (Q % 2 == 0) {
        using F2 = float __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int b = 0; b < Q; b += 2) {
            const F2 x = *reinterpret_cast<const F2*>(p + b);
            v[b] = x[0]; v[b + 1] = x[1];
        }
    } else {
#pragma unroll
        for (int b = 0; b < Q; ++b) v[b] = p[b];
    }
}
template <int Q>
__device__ __forceinline__ void write_strip(float* p, const float (&v)[Q]) {
    if constexpr (Q % 2 == 0) {
        using F2 = float __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int b = 0; b < Q; b += 2) *reinterpret_cast<F2*>(p + b) = F2{v[b], v[b + 1]};
    } else {
#pragma unroll
        for (int b = 0; b < Q; ++b) p[b] = v[b];
    }
}
template <int Q, int LD>
__device__ __forceinline__ void read_block(float (&tq)[Q][Q], const float* blk) {
#pragma unroll
    for (int a = 0; a < Q; ++a) read_strip<Q>(tq[a], blk + a * LD);
}

// ---- the RBF pair value from T'[r0, c0] and the forward rows of its micro-block ------------------------------------
struct RbfPair {
    float nn, k, kil, kil2;
    __device__ __forceinline__ RbfPair(float s1r0, float s2c0, float t00, float s, float il, float il2) {
        nn = fmaxf(s1r0 - s2c0 - 2.f * t00, 0.f);     // covar_dist clamps at 0
        k = s * expf(-0.5f * nn);                     // postprocess_rbf, ScaleKernel
        kil = k * il; kil2 = k * il2;
    }
    // row a of the micro-block from row a (ta) and row 0 (t0) of T'
    template <int Q>
    __device__ __forceinline__ void fwd_row(float (&v)[Q], bool row0, const float (&ta)[Q], const float (&t0)[Q]) const {
        if (row0) {
            v[0] = k;
#pragma unroll
            for (int b = 1; b < Q; ++b) v[b] = t0[b] * kil;                          // w_b k / ell
        } else {
            v[0] = ta[0] * kil;                                                      // -u_a k / ell
#pragma unroll
            for (int b = 1; b < Q; ++b) v[b] = (ta[b] + ta[0] * t0[b]) * kil2;       // (G_ab - u_a w_b) k / ell^2
        }
    }
};

// ---- backward: dP1[48, NP] += Tbar[48, 48] . P2ext[48, NP], accumulators over the sweep, the closing flush ----------
template <int NNP>
__device__ __forceinline__ void zero_acc(f4 (&acc)[3][NNP]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < NNP; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
}
template <int NNP>
__device__ __forceinline__ void dp1_product(f4 (&acc)[3][NNP], const float* TT, const float* P2s, int LDP, int nnp, int m16, int kg) {
    const float* pa = TT + m16 * PAIR_LDT + kg;
    const float* pb = P2s + kg * LDP + m16;
#pragma unroll
    for (int kk = 0; kk < 48; kk += 4) {
        float av[3], bv[NNP];
#pragma unroll
        for (int i = 0; i < 3; ++i) av[i] = pa[i * 16 * PAIR_LDT + kk];
#pragma unroll
        for (int j = 0; j < NNP; ++j) bv[j] = (j < nnp) ? pb[kk * LDP + 16 * j] : 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < NNP; ++j)
                if (j < nnp) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
}
// partial slab: slab[split][row][NP]
template <int T, int NNP>
__device__ __forceinline__ void flush_slab(const f4 (&acc)[3][NNP], float* slab, int row0, int n1q, int NP, int nnp, int m16, int kg) {
    float* myslab = slab + ((int64_t)blockIdx.x * n1q) * NP;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < NNP; ++j)
            if (j < nnp) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = i * 16 + kg * 4 + r;
                    const int64_t gr = row0 + rr;
                    if (rr < T && gr < n1q) myslab[gr * NP + j * 16 + m16] = acc[i][j][r];
                }
            }
}
// the workgroup's two scalars: sum(G o K) and the lengthscale sum
__device__ __forceinline__ void flush_partials(float sK_sum, float l_acc, float il, float* partials, int lane) {
    float l_sum = -il * l_acc;
    for (int off = 32; off > 0; off >>= 1) {
        sK_sum += __shfl_down(sK_sum, off);
        l_sum += __shfl_down(l_sum, off);
    }
    if (lane == 0) {
        const int bid = blockIdx.y * gridDim.x + blockIdx.x;
        partials[bid * 2] = sK_sum;
        partials[bid * 2 + 1] = l_sum;
    }
}

// ---- host: the workgroup count per row tile of a forward sweep, and the instance of a pair kernel --------------------
inline int sweep_nsplit(int wgs, int rt, int ctiles) {
    int ns = wgs / rt;
    if (ns < 1) ns = 1;
    if (ns > ctiles) ns = ctiles;
    return ns;
}
// launch(element type, Q, KSM) for q in {3, 6}; KSM = 8 for packed widths NP <= 32, 16 for NP <= 64
template <typename F>
inline void pair_instance(bool is_double, int q, int NP, F&& launch) {
    auto typed = [&](auto et) {
        using I3 = std::integral_constant<int, 3>; using I6 = std::integral_constant<int, 6>;
        using I8 = std::integral_constant<int, 8>; using I16 = std::integral_constant<int, 16>;
        if (NP <= 32) { if (q == 6) launch(et, I6{}, I8{}); else launch(et, I3{}, I8{}); }
        else { if (q == 6) launch(et, I6{}, I16{}); else launch(et, I3{}, I16{}); }
    };
    if (is_double) typed(double{}); else typed(float{});
}

}  // namespace
