// Host check of the index algebra of the paths' Hessian-vector product (dsvgp_paths_hvp, csrc/paths.hip): includes the arithmetic the
// kernels and their launcher use (csrc/paths_plan.h: paths_hvp_ns, paths_hvp_lds, paths_hvp_work) and emulates, for the shapes of
// tests/test_gpu_paths_hvp.py, of tools/paths_hvp_probe.py and for every d <= 32, every thread of paths_hvp_fused_kernel<D> serially --
// the loads of x and v, the staging copies of every chunk, every wave's walk over the chunk, the reduction image and the output stores.
// Shows that
//   * every (sample, point, i) and every (sample, point, j) is visited exactly once;
//   * every LDS offset lies inside the kernel's array (at most 64 KiB for every D) and every global offset inside the weights, x, v, hv;
//   * every element of hv is stored exactly once, and points past B and samples past n store nothing.
// A workgroup applies one (i, j) walk to all of its lanes and samples, so the count is formed per workgroup over (g, i) and (g, j) and
// per output element over the grid; for the small shapes the 3-D counts are also formed outright.  For the composed route it checks
// that the workspace regions are 16-byte aligned, disjoint, inside the bytes the helper reports, and large enough for every launch.
// No GPU.
//   g++ -O2 -std=c++17 -I gp-derivatives-variational-inference_amd/csrc tools/paths_hvp_check.cpp -o paths_hvp_check && ./paths_hvp_check
#include <cstdio>
#include <vector>

#include "paths_plan.h"

static long long bad_total = 0;

static int check_fused(int d, int M, int F, int n, int B) {
    const int D = paths_pad4(d), NS = paths_hvp_ns(D), NT = PP_NW * 64;
    const PathsLds LD = paths_hvp_lds(D);
    const PathsWeights L = paths_weights(M, d, F, n);
    long long bad = 0;
    if (d > PP_FUSED_MAX_D || D != L.ldw || NS < 1 || NS > PP_NS_MAX || NS > paths_ns(D)) ++bad;
    if (LD.floats * 4 > 65536 || LD.o_w + NS * PP_CH > LD.floats || NS * PP_TP * (D + 1) > LD.floats || LD.o_a + NS * PP_CH > LD.floats) ++bad;
    const int ntiles = (B + PP_TP - 1) / PP_TP, ngroups = (n + NS - 1) / NS;
    if (ngroups > 65535) ++bad;
    const bool brute = (double)n * B * (M + F) < 4e7;
    std::vector<unsigned char> full_i, full_j;
    if (brute) { full_i.assign((size_t)n * B * M, 0); full_j.assign((size_t)n * B * F, 0); }
    std::vector<int> hseen((size_t)n * B * d, 0);
    auto lds_ok = [&](long long off) { if (off < 0 || off >= LD.floats) ++bad; };
    auto w_ok = [&](size_t off) { if (off >= L.total) ++bad; };
    // the loads of x and v: lane = point, only k < d of points b < B
    for (int tile = 0; tile < ntiles; ++tile)
        for (int lane = 0; lane < 64; ++lane) {
            const long long b = (long long)tile * PP_TP + lane;
            for (int k = 0; k < D; ++k) {
                if (!(k < d && b < B)) continue;
                if (b * d + k < 0 || b * d + k >= (long long)B * d) ++bad;
                w_ok(L.o_center + k); if (L.o_center + k >= L.o_nz) ++bad;
            }
        }
    // the (i, j) walk does not depend on the tile: emulate it for one tile per sample group, the outputs for every workgroup
    for (int grp = 0; grp < ngroups; ++grp) {
        const int s0 = grp * NS;
        std::vector<int> ci((size_t)NS * M, 0), cj((size_t)NS * F, 0);
        for (int c0 = 0; c0 < M; c0 += PP_CH) {
            const int nc = M - c0 < PP_CH ? M - c0 : PP_CH;
            std::vector<int> staged((size_t)LD.floats, 0);
            for (int tid = 0; tid < NT; ++tid) {
                for (int t = tid; t < nc * (D / 4); t += NT) {
                    for (int e = 0; e < 4; ++e) {
                        lds_ok(LD.o_z + 4 * t + e); ++staged[LD.o_z + 4 * t + e];
                        w_ok(L.o_z + (size_t)c0 * D + 4 * t + e); if (L.o_z + (size_t)c0 * D + 4 * t + e >= L.o_om) ++bad;
                    }
                    if (LD.o_z + 4 * t + 3 >= LD.o_g) ++bad;
                }
                for (int g = 0; g < NS; ++g) {
                    const bool live = s0 + g < n;
                    const int sg = live ? s0 + g : 0;
                    for (int t = tid; t < nc * (D / 4); t += NT)
                        for (int e = 0; e < 4; ++e) {
                            const long long o = LD.o_g + (long long)g * PP_CH * D + 4 * t + e;
                            lds_ok(o); if (o >= LD.o_a) ++bad; else ++staged[o];
                            if (live) w_ok(L.o_g + ((size_t)sg * M + c0) * D + 4 * t + e);
                        }
                    if (tid < nc) {
                        lds_ok(LD.o_a + g * PP_CH + tid); ++staged[LD.o_a + g * PP_CH + tid];
                        if (live) { w_ok(L.o_a + (size_t)sg * L.Mr + c0 + tid); if (L.o_a + (size_t)sg * L.Mr + c0 + tid >= L.o_ap) ++bad; }
                    }
                }
            }
            for (int slice = 0; slice < PP_NW; ++slice)
                for (int i = slice; i < nc; i += PP_NW)
                    for (int g = 0; g < NS; ++g) {
                        for (int k = 0; k < D; ++k)                         // every float read was staged exactly once in this chunk
                            if (staged[LD.o_z + i * D + k] != 1 || staged[LD.o_g + (g * PP_CH + i) * D + k] != 1) ++bad;
                        if (staged[LD.o_a + g * PP_CH + i] != 1) ++bad;
                        ++ci[(size_t)g * M + c0 + i];
                    }
        }
        for (int j0 = 0; j0 < F; j0 += PP_CH) {
            const int nf = F - j0 < PP_CH ? F - j0 : PP_CH;
            std::vector<int> staged((size_t)LD.floats, 0);
            for (int tid = 0; tid < NT; ++tid) {
                for (int t = tid; t < nf * (D / 4); t += NT)
                    for (int e = 0; e < 4; ++e) {
                        const long long o = LD.o_om + 4 * t + e;
                        lds_ok(o); if (o >= LD.o_ph) ++bad; else ++staged[o];
                        w_ok(L.o_om + (size_t)j0 * D + 4 * t + e); if (L.o_om + (size_t)j0 * D + 4 * t + e >= L.o_ph) ++bad;
                    }
                if (tid < nf) { lds_ok(LD.o_ph + tid); ++staged[LD.o_ph + tid]; if (L.o_ph + j0 + tid >= L.o_a) ++bad; }
                for (int g = 0; g < NS; ++g) {
                    const bool live = s0 + g < n;
                    const int sg = live ? s0 + g : 0;
                    if (tid < nf) {
                        lds_ok(LD.o_w + g * PP_CH + tid); ++staged[LD.o_w + g * PP_CH + tid];
                        if (live && L.o_wq + (size_t)sg * L.Fr + j0 + tid >= L.o_g) ++bad;
                    }
                }
            }
            for (int slice = 0; slice < PP_NW; ++slice)
                for (int j = slice; j < nf; j += PP_NW)
                    for (int g = 0; g < NS; ++g) {
                        for (int k = 0; k < D; ++k) if (staged[LD.o_om + j * D + k] != 1) ++bad;
                        if (staged[LD.o_ph + j] != 1 || staged[LD.o_w + g * PP_CH + j] != 1) ++bad;
                        ++cj[(size_t)g * F + j0 + j];
                    }
        }
        for (int g = 0; g < NS; ++g) {
            for (int i = 0; i < M; ++i) bad += ci[(size_t)g * M + i] != 1;
            for (int j = 0; j < F; ++j) bad += cj[(size_t)g * F + j] != 1;
        }
        // reduction image and output stores of every workgroup of this sample group
        for (int lane = 0; lane < 64; ++lane)
            for (int g = 0; g < NS; ++g)
                for (int k = 0; k <= D; ++k) lds_ok(LD.o_red + (long long)(g * PP_TP + lane) * (D + 1) + k);
        for (int tile = 0; tile < ntiles; ++tile) {
            const long long b0 = (long long)tile * PP_TP;
            const int npts = (int)(B - b0 < PP_TP ? B - b0 : PP_TP);
            if (npts < 1) ++bad;
            for (int g = 0; g < NS; ++g) {
                if (s0 + g >= n) break;
                const size_t so = (size_t)(s0 + g) * (size_t)B + (size_t)b0;
                if (brute)
                    for (int pt = 0; pt < npts; ++pt) {
                        for (int i = 0; i < M; ++i) full_i[(so + pt) * M + i] += ci[(size_t)g * M + i];
                        for (int j = 0; j < F; ++j) full_j[(so + pt) * F + j] += cj[(size_t)g * F + j];
                    }
                for (int tid = 0; tid < NT; ++tid)
                    for (int t = tid; t < npts * d; t += NT) {
                        const int pt = t / d, k = t - pt * d;
                        lds_ok(LD.o_red + (long long)(g * PP_TP + pt) * (D + 1) + k);
                        if (pt >= npts || k >= d || so * d + t >= (size_t)n * B * d) ++bad; else ++hseen[so * d + t];
                    }
            }
        }
    }
    for (int v : hseen) bad += v != 1;
    if (brute) {
        for (unsigned char v : full_i) bad += v != 1;
        for (unsigned char v : full_j) bad += v != 1;
    }
    printf("fused    d %4d M %4d F %5d n %3d B %6d: D %2d NS %d, %5d tiles x %2d groups, LDS %5d B%s  %s\n", d, M, F, n, B, D, NS, ntiles,
           ngroups, LD.floats * 4, brute ? ", 3-D counts formed" : "", bad ? "FAILED" : "ok");
    bad_total += bad;
    return bad ? 1 : 0;
}

static int check_composed(int d, int M, int F, int n, int B) {
    PathsHvpWork S;
    long long bad = 0;
    if (paths_hvp_work(M, d, F, n, B, S)) { printf("composed d %4d M %4d F %5d n %3d B %6d: refused\n", d, M, F, n, B); ++bad_total; return 1; }
    struct Reg { size_t off, len; } regs[] = {
        {S.o_x, (size_t)B * S.ldw}, {S.o_v, (size_t)B * S.ldw}, {S.o_xn, S.Br}, {S.o_xv, S.Br}, {S.o_k, (size_t)B * S.ldM},
        {S.o_rv, (size_t)B * S.ldM}, {S.o_c2, (size_t)B * S.ldM}, {S.o_t, (size_t)B * S.ldF}, {S.o_ov, (size_t)B * S.ldF},
        {S.o_s2, (size_t)B * S.ld2}, {S.o_gv, (size_t)B * S.ld2}, {S.o_c1, (size_t)S.ng * B * S.ldM}, {S.o_sig, (size_t)S.ng * S.Br},
        {S.o_sig1, (size_t)S.ng * S.Br}, {S.o_o1, (size_t)S.ng * B * S.ldw}, {S.o_o2, (size_t)S.ng * B * S.ldw},
        {S.o_wo, (size_t)F * S.ng * S.ldw}, {S.o_gp, (size_t)B * S.ng * S.ldw}};
    size_t end = 0;
    for (auto& r : regs) {
        if (r.off % 4 || r.off != end) ++bad;                                   // aligned, back to back: disjoint
        end = r.off + r.len;
    }
    if (end != S.total || S.ng < 1 || S.ng > n || S.ld2 < S.ng * M || S.ldM < M || S.ldF < F || S.ldw < d) ++bad;
    const size_t group = S.total - S.o_s2;
    if (S.ng > 1 && group > PP_GROUP_FLOATS + (size_t)8 * B) ++bad;             // the group part stays under 512 MiB (ld2's padding apart)
    // the largest index of every launch, for the last (possibly ragged) group
    for (int s0 = 0; s0 < n; s0 += S.ng) {
        const int ng = n - s0 < S.ng ? n - s0 : S.ng;
        if ((size_t)(B - 1) * S.ld2 + (size_t)ng * M > (size_t)B * S.ld2) ++bad;                                 // S2, GV: N = ng M columns
        if (((size_t)(ng - 1) * B + (B - 1)) * S.ldM + S.ldM > (size_t)S.ng * B * S.ldM) ++bad;                   // C1
        if ((size_t)(ng - 1) * S.Br + B > (size_t)S.ng * S.Br) ++bad;                                            // sigma, sigma1
        if ((size_t)(ng * B - 1) * S.ldw + d > (size_t)S.ng * B * S.ldw) ++bad;                                  // O1, O2
        if ((size_t)(F - 1) * ng * S.ldw + (size_t)ng * S.ldw > (size_t)F * S.ng * S.ldw) ++bad;                 // WO
        if ((size_t)(B - 1) * ng * S.ldw + (size_t)ng * S.ldw > (size_t)B * S.ng * S.ldw) ++bad;                 // GP
        if (s0 + ng > n) ++bad;                                                                                  // samples past n: none
    }
    printf("composed d %4d M %4d F %5d n %3d B %6d: groups of %3d samples, workspace %8.1f MiB  %s\n", d, M, F, n, B, S.ng,
           S.total * 4.0 / 1048576.0, bad ? "FAILED" : "ok");
    bad_total += bad;
    return bad ? 1 : 0;
}

int main() {
    // the plan of every instance: sample-group width and LDS bytes
    for (int D = 4; D <= PP_FUSED_MAX_D; D += 4) {
        const PathsLds LD = paths_hvp_lds(D);
        printf("plan D %2d: NS %d, LDS %5d bytes\n", D, paths_hvp_ns(D), LD.floats * 4);
        bad_total += LD.floats * 4 > 65536;
    }
    // (d, M, F, n, B): the shapes of tests/test_gpu_paths_hvp.py (its consistency slices and the one-sample mean included) and of
    // tools/paths_hvp_probe.py
    const int fused[][5] = {{3, 12, 64, 3, 70}, {5, 40, 100, 5, 130}, {20, 70, 128, 9, 33}, {32, 16, 96, 2, 65}, {5, 19, 1, 1, 67},
                            {3, 12, 64, 3, 40}, {3, 12, 64, 2, 70}, {5, 40, 100, 2, 130}, {20, 70, 128, 2, 33}, {5, 40, 1, 1, 130},
                            {2, 20, 1, 1, 50}, {20, 500, 2048, 64, 4096}, {1, 1, 1, 1, 1}, {32, 129, 65, 17, 129}};
    const int composed[][5] = {{33, 16, 128, 4, 40}, {200, 24, 160, 3, 40}, {200, 24, 160, 3, 30}, {200, 24, 1, 1, 40},
                               {200, 512, 2048, 8, 5000}, {4035, 512, 2048, 64, 512}, {33, 1, 1, 1, 1}, {200, 500, 2048, 64, 65536}};
    for (auto& s : fused) check_fused(s[0], s[1], s[2], s[3], s[4]);
    for (int d = 1; d <= 32; ++d) check_fused(d, 67, 70, 11, 67);
    for (auto& s : composed) check_composed(s[0], s[1], s[2], s[3], s[4]);
    PathsHvpWork S;
    bad_total += (paths_hvp_work(0, 40, 8, 1, 1, S) == 0) + (paths_hvp_work(8, 40, 8, 1, 0, S) == 0) +
                 (paths_hvp_work(500, 200, 2048, 1, 2000000, S) == 0);             // B ldF passes 2^31: refused
    printf(bad_total ? "paths hvp: FAILED\n"
                     : "paths hvp: every (sample, point, i) and (sample, point, j) visited exactly once, every offset in bounds\n");
    return bad_total ? 1 : 0;
}
