// Host-side plan of the k-means kernels (csrc/kmeans.hip): the constants, the staging and walk arithmetic and the workspace layout of the
// composed assignment, shared by the kernels, their launchers and tools/kmeans_check.cpp (plain C++, no HIP).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define KM_HD __host__ __device__
#else
#define KM_HD
#endif

constexpr int KM_FUSED_MAX_D = 32;       // the fused assignment's bound on d
constexpr int KM_TP = 64;                // points per workgroup of the fused assignment (one per lane)
constexpr int KM_NW = 8;                 // waves per workgroup = slices of every chunk of centroids
constexpr int KM_CH = 64;                // centroids per LDS chunk
constexpr int KM_ROWS = 32768;           // rows of X per block of the composed assignment
constexpr int KM_UPD_NW = 8;             // waves per workgroup of the update walk
constexpr int KM_UPD_UNROLL = 4;         // label blocks a wave loads before it ballots them
constexpr int KM_UPD_MAXR = 4;           // fp64 accumulators per lane and pass: a pass covers 64 * R columns
constexpr int KM_MOM_MAX_D = 128;        // bound on d of the cluster moments
constexpr int KM_MOM_T = 32;             // tile edge of the moments' upper triangle

inline int km_pad4(int v) { return (v + 3) & ~3; }

// fused assignment: element t of the staging copy of a chunk of nc centroids starting at c0 -> (LDS float offset, global float offset in
// Z[M, d]); `wide`: the copy moves 16 bytes (d == D and Z 16-byte aligned), t counts float4s, else single floats with the padding columns
// (k >= d) written as zero (global offset -1)
struct KmStage { int lds; long long glob; };
KM_HD inline KmStage km_stage(int t, int e, int c0, int d, int D, bool wide) {
    if (wide) return {4 * t + e, (long long)c0 * d + 4 * t + e};
    const int i = t / D, k = t - i * D;
    return {t, k < d ? (long long)(c0 + i) * d + k : -1};
}
inline int km_stage_count(int nc, int D, bool wide) { return wide ? nc * (D / 4) : nc * D; }

// accumulators per lane of the update walk, and its passes over the columns
inline int km_update_regs(int d) { return d <= 64 ? 1 : d <= 128 ? 2 : KM_UPD_MAXR; }
inline int km_update_passes(int d) { const int w = 64 * km_update_regs(d); return (d + w - 1) / w; }
// label blocks (64 labels each) of N points
inline long long km_label_blocks(long long N) { return (N + 63) / 64; }

// composed assignment (d > 32), floats: center[ldw] | Z~[M][ldw] | nz[Mr] | X~[R][ldw] | xn[Rr] | S[R][ldS]; R = min(N, KM_ROWS)
struct KmLayout { int ldw, ldS, R; size_t o_center, o_z, o_nz, o_x, o_xn, o_S, total; };
inline bool km_layout(long long N, int d, int M, KmLayout* L) {
    if (N < 1 || d < 1 || M < 1 || M > N) return false;
    L->ldw = km_pad4(d);
    L->ldS = km_pad4(M);
    L->R = (int)(N < KM_ROWS ? N : KM_ROWS);
    if ((long long)L->R * L->ldS >= (1ll << 31) || (long long)L->R * L->ldw >= (1ll << 31) || (long long)M * L->ldw >= (1ll << 31))
        return false;
    const size_t Rr = (size_t)km_pad4(L->R);
    L->o_center = 0;
    L->o_z = L->o_center + L->ldw;
    L->o_nz = L->o_z + (size_t)M * L->ldw;
    L->o_x = L->o_nz + (size_t)km_pad4(M);
    L->o_xn = L->o_x + (size_t)L->R * L->ldw;
    L->o_S = L->o_xn + Rr;
    L->total = L->o_S + (size_t)L->R * L->ldS;
    return true;
}

// cluster moments: tile t of the upper triangle of the T x T tile grid (T = ceil(d / 32)), row-major over tr <= tc
inline int km_mom_tiles(int d) { const int T = (d + KM_MOM_T - 1) / KM_MOM_T; return T * (T + 1) / 2; }
KM_HD inline void km_mom_tile(int t, int d, int* tr, int* tc) {
    const int T = (d + KM_MOM_T - 1) / KM_MOM_T;
    int r = 0;
    while (t >= T - r) { t -= T - r; ++r; }
    *tr = r;
    *tc = r + t;
}
