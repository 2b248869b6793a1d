// Host check of the index algebra of the k-means kernels (csrc/kmeans.hip: kmeans_assign_fused_kernel<D>, kmeans_update_kernel<R>,
// kmeans_moments_kernel, the composed assignment's workspace): includes the arithmetic the kernels and their launchers use
// (csrc/kmeans_plan.h) and emulates, for the shapes of tests/test_gpu_kmeans.py and of tools/kmeans_probe.py and for every d <= 32, every
// thread of the fused assignment and of the update walk serially.  Shows that
//   * every (point, centroid) pair is visited exactly once: the chunk walk is shared by all lanes of all workgroups, so the count is
//     formed over the centroids, and every float a wave reads from LDS was staged exactly once in that chunk;
//   * every LDS offset lies inside the kernel's arrays and every global offset inside x[N, d], Z[M, d], labels[N] and dist2[N];
//   * points past N load and store nothing, centroids past M are never staged or compared;
//   * the update walk loads every label once per pass, adds every (row, column) exactly once over the passes, and stores every column of
//     a centroid once; the moment tiles cover every entry of a d x d matrix exactly once;
//   * the workspace regions of the composed assignment are 16-byte aligned, disjoint, in order, inside the bytes the helper reports,
//     and large enough for every row block, with every intermediate under 2^31 entries.
// No GPU.
//   g++ -O2 -std=c++17 -I gp-derivatives-variational-inference_amd/csrc tools/kmeans_check.cpp -o kmeans_check && ./kmeans_check
#include <cstdio>
#include <vector>

#include "kmeans_plan.h"

static long long bad_total = 0;

static long long check_fused(long long N, int d, int M, bool wide) {
    const int D = km_pad4(d), NT = KM_NW * 64, LDS = KM_CH * D;
    long long bad = 0;
    if (d > KM_FUSED_MAX_D || D > 32 || (wide && d != D)) ++bad;
    if ((LDS + 2 * KM_NW * KM_TP) * 4 > 65536) ++bad;
    std::vector<int> visited((size_t)M, 0), zread((size_t)M * d, 0);
    for (int c0 = 0; c0 < M; c0 += KM_CH) {
        const int nc = M - c0 < KM_CH ? M - c0 : KM_CH;
        std::vector<int> staged((size_t)LDS, 0);
        for (int tid = 0; tid < NT; ++tid)
            for (int t = tid; t < km_stage_count(nc, D, wide); t += NT)
                for (int e = 0; e < (wide ? 4 : 1); ++e) {
                    const KmStage s = km_stage(t, e, c0, d, D, wide);
                    if (s.lds < 0 || s.lds >= LDS) { ++bad; continue; }
                    ++staged[s.lds];
                    if (s.lds / D >= nc) ++bad;                                 // a centroid past M is never staged
                    if (s.glob < 0) { if (s.lds % D < d) ++bad; continue; }     // only padding columns are written as zero
                    if (s.glob >= (long long)M * d) { ++bad; continue; }
                    if (s.glob != (long long)(c0 + s.lds / D) * d + s.lds % D) ++bad;
                    ++zread[(size_t)s.glob];
                }
        for (int slice = 0; slice < KM_NW; ++slice)
            for (int i = slice; i < nc; i += KM_NW) {
                for (int k = 0; k < D; ++k) if (staged[(size_t)i * D + k] != 1) ++bad;
                ++visited[(size_t)c0 + i];
            }
    }
    for (int c = 0; c < M; ++c) bad += visited[c] != 1;
    for (size_t o = 0; o < zread.size(); ++o) bad += zread[o] != 1;
    // the winners' image, the loads of x and the two stores of every workgroup
    const long long ntiles = (N + KM_TP - 1) / KM_TP;
    std::vector<unsigned char> xseen((size_t)N * d, 0), lseen((size_t)N, 0);
    for (long long blk = 0; blk < ntiles; ++blk)
        for (int tid = 0; tid < NT; ++tid) {
            const int lane = tid & 63, slice = tid >> 6;
            const long long b = blk * KM_TP + lane;
            if (slice * KM_TP + lane >= KM_NW * KM_TP) ++bad;
            if (b >= N) continue;                                               // a point past N loads and stores nothing
            if (slice == 0) {
                for (int k = 0; k < d; ++k) {
                    const long long o = b * d + k;
                    if (o >= N * d) ++bad; else ++xseen[(size_t)o];
                }
                ++lseen[(size_t)b];
            }
        }
    for (size_t o = 0; o < xseen.size(); ++o) bad += xseen[o] != 1;
    for (size_t o = 0; o < lseen.size(); ++o) bad += lseen[o] != 1;
    return bad;
}

static long long check_update(long long N, int d, int M) {
    const int R = km_update_regs(d), passes = km_update_passes(d);
    const long long nblk = km_label_blocks(N);
    long long bad = 0;
    if (R < 1 || R > KM_UPD_MAXR || (long long)passes * 64 * R < d) ++bad;
    if ((KM_UPD_NW * 64 * R * 8 + KM_UPD_NW * 4) > 65536) ++bad;
    std::vector<unsigned char> added((size_t)N * d, 0);
    std::vector<int> zstore((size_t)d, 0);
    int pass = 0;
    for (int k0 = 0; k0 < d; k0 += 64 * R, ++pass) {
        std::vector<unsigned char> lab((size_t)N, 0);
        for (int wv = 0; wv < KM_UPD_NW; ++wv)
            for (long long b = (long long)wv * KM_UPD_UNROLL; b < nblk; b += KM_UPD_NW * KM_UPD_UNROLL)
                for (int u = 0; u < KM_UPD_UNROLL; ++u)
                    for (int j = 0; j < 64; ++j) {
                        const long long row = (b + u) * 64 + j;                 // lane j loads this label; its ballot bit names this row
                        if (row >= N) continue;                                 // (label -1 there: never a member)
                        ++lab[(size_t)row];
                        for (int r = 0; r < R; ++r)
                            for (int lane = 0; lane < 64; ++lane) {
                                const int k = r * 64 + lane;
                                if (r * 64 + lane >= 64 * R) ++bad;             // the wave's LDS image
                                if (k0 + k >= d) continue;
                                const long long o = row * d + k0 + k;
                                if (o >= N * d) ++bad; else ++added[(size_t)o];
                            }
                    }
        for (size_t o = 0; o < lab.size(); ++o) bad += lab[o] != 1;
        for (int r = 0; r < R; ++r)
            for (int lane = 0; lane < 64; ++lane)
                if (k0 + r * 64 + lane < d) ++zstore[(size_t)k0 + r * 64 + lane];
    }
    if (pass != passes) ++bad;
    for (size_t o = 0; o < added.size(); ++o) bad += added[o] != 1;
    for (int k = 0; k < d; ++k) bad += zstore[k] != 1;
    (void)M;
    return bad;
}

static long long check_moments(int d) {
    long long bad = 0;
    if (d > KM_MOM_MAX_D) return 1;
    const int T = (d + KM_MOM_T - 1) / KM_MOM_T;
    std::vector<int> seen((size_t)d * d, 0);
    for (int t = 0; t < km_mom_tiles(d); ++t) {
        int tr, tc;
        km_mom_tile(t, d, &tr, &tc);
        if (tr < 0 || tr > tc || tc >= T) { ++bad; continue; }
        for (int tid = 0; tid < 256; ++tid) {
            const int wv = tid >> 6, lane = tid & 63;
            const int gc = tc * KM_MOM_T + (lane & 31), gr0 = tr * KM_MOM_T + wv * 8 + (lane >> 5);
            for (int q = 0; q < 4; ++q) {
                const int gr = gr0 + 2 * q;
                if (gr >= (tr + 1) * KM_MOM_T) ++bad;
                if (gr >= d || gc >= d) continue;
                ++seen[(size_t)gr * d + gc];
                if (tr != tc) ++seen[(size_t)gc * d + gr];
            }
        }
    }
    for (size_t o = 0; o < seen.size(); ++o) bad += seen[o] != 1;
    return bad;
}

static long long check_composed(long long N, int d, int M) {
    KmLayout L;
    long long bad = 0;
    if (!km_layout(N, d, M, &L)) return 1;
    const size_t bytes = (L.total * 4 + 15) & ~(size_t)15;
    const size_t Rr = (size_t)km_pad4(L.R);
    if (L.ldw % 4 || L.ldS % 4 || L.ldw < d || L.ldS < M) ++bad;
    const size_t off[7] = {L.o_center, L.o_z, L.o_nz, L.o_x, L.o_xn, L.o_S, L.total};
    const size_t len[6] = {(size_t)L.ldw, (size_t)M * L.ldw, (size_t)M, (size_t)L.R * L.ldw, (size_t)L.R, (size_t)L.R * L.ldS};
    for (int i = 0; i < 6; ++i) {
        if (off[i] % 4) ++bad;                                                  // 16-byte aligned
        if (off[i] + len[i] > off[i + 1]) ++bad;                                // disjoint, in order
    }
    if (L.total * 4 > bytes || Rr < (size_t)L.R) ++bad;
    if ((long long)L.R * L.ldS >= (1ll << 31) || (long long)L.R * L.ldw >= (1ll << 31)) ++bad;
    long long covered = 0;
    for (long long r0 = 0; r0 < N; r0 += L.R) {
        const long long rows = N - r0 < L.R ? N - r0 : L.R;
        if (rows < 1 || rows > L.R || r0 + rows > N) ++bad;
        covered += rows;
    }
    if (covered != N) ++bad;
    return bad;
}

int main() {
    struct Shape { long long N; int d, M; };
    const Shape fused[] = {{3000, 3, 37}, {4133, 5, 130}, {2000, 20, 70}, {70, 32, 16}, {40, 5, 40}, {1, 4, 1}, {1000000, 20, 500}, {400, 5, 24}};
    for (const Shape& s : fused) {
        long long bad = check_fused(s.N, s.d, s.M, false);
        if (s.d % 4 == 0) bad += check_fused(s.N, s.d, s.M, true);
        bad += check_update(s.N, s.d, s.M);
        printf("fused   N %7lld d %3d M %4d: %s\n", s.N, s.d, s.M, bad ? "FAILED" : "ok");
        bad_total += bad;
    }
    for (int d = 1; d <= KM_FUSED_MAX_D; ++d) {
        long long bad = check_fused(200, d, 70, false) + check_fused(129, d, 129, false);
        if (d % 4 == 0) bad += check_fused(200, d, 70, true) + check_fused(129, d, 129, true);
        bad += check_update(200, d, 70);
        printf("fused   every width: d %2d D %2d: %s\n", d, km_pad4(d), bad ? "FAILED" : "ok");
        bad_total += bad;
    }
    const Shape composed[] = {{1500, 33, 40}, {600, 200, 24}, {300, 33, 20}, {24, 200, 24}, {100000, 200, 512}, {70000, 257, 300}, {1000, 4035, 8}};
    for (const Shape& s : composed) {
        const long long bad = check_composed(s.N, s.d, s.M) + (s.N * s.d <= 30000000 ? check_update(s.N, s.d, s.M) : 0);
        printf("composed N %7lld d %4d M %4d: %s\n", s.N, s.d, s.M, bad ? "FAILED" : "ok");
        bad_total += bad;
    }
    {   // refused shapes: no layout
        KmLayout L;
        long long bad = 0;
        bad += km_layout(0, 40, 1, &L) || km_layout(10, 0, 1, &L) || km_layout(10, 40, 0, &L) || km_layout(10, 40, 11, &L);
        bad += km_layout(1000000, 40, 70000, &L);                               // 32768 x 70000 passes 2^31 entries
        printf("composed refusals: %s\n", bad ? "FAILED" : "ok");
        bad_total += bad;
    }
    for (int d = 1; d <= KM_MOM_MAX_D; ++d) bad_total += check_moments(d);
    printf("moments  d 1..%d: tiles cover every entry once\n", KM_MOM_MAX_D);
    if (bad_total) { printf("FAILED: %lld violations\n", bad_total); return 1; }
    printf("every (point, centroid) pair visited exactly once, every offset in bounds\n");
    return 0;
}
