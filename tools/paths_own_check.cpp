// Host check of the index algebra of the own-point evaluation of the sample paths and of the descent built on it (csrc/paths.hip:
// paths_own_fused_kernel<D, WANT_GRAD>, dsvgp_paths_eval_own, dsvgp_paths_descend): includes the arithmetic the kernels and their
// launchers use (csrc/paths_plan.h) and emulates, for the shapes of tests/test_gpu_paths_own.py and of tools/paths_own_probe.py and for
// every d <= 32, every thread of the fused kernel serially -- the staging copies of every chunk, every wave's walk over the chunk, the
// reduction image, the loads of x and the output stores.  Shows that
//   * every (sample, point, i) and every (sample, point, j) is visited exactly once;
//   * every LDS offset lies inside the kernel's array and every global offset inside the weights, `x`, `values` and `grads`;
//   * every output element is stored exactly once, and points past B load and store nothing.
// A workgroup applies one (i, j) walk to all of its lanes, so the count is formed per sample over i and j and per output element over
// the grid; for the small shapes the 3-D counts are also formed outright.  For the composed route and the descent it checks that the
// workspace regions are 16-byte aligned, disjoint, inside the bytes the helpers report, and large enough for every launch.  No GPU.
//   g++ -O2 -std=c++17 -I gp-derivatives-variational-inference_amd/csrc tools/paths_own_check.cpp -o paths_own_check && ./paths_own_check
#include <cstdio>
#include <vector>

#include "paths_plan.h"

static long long bad_total = 0;

static int check_fused(int d, int M, int F, int n, int B, bool want_grad) {
    const int D = paths_pad4(d), NT = PP_NW * 64;
    const PathsLds LD = paths_own_lds(D);
    const PathsWeights L = paths_weights(M, d, F, n);
    long long bad = 0;
    if (d > PP_FUSED_MAX_D || D != L.ldw || n > 65535) ++bad;
    if (LD.floats * 4 > 65536 || LD.o_w + PP_CH > LD.floats || PP_TP * (D + 1) > LD.floats || LD.o_a + PP_CH > LD.floats) ++bad;
    if ((D + 1) % 2 != 1) ++bad;                                                 // the reduction image's row stride is odd
    if (LD.o_z % 4 || LD.o_g % 4 || LD.o_om % 4) ++bad;                          // 16-byte LDS copies
    if (L.o_z % 4 || L.o_om % 4 || L.o_g % 4) ++bad;                             // 16-byte global loads
    const int ntiles = (B + PP_TP - 1) / PP_TP;
    const bool brute = (double)n * B * (M + F) < 4e7;
    std::vector<unsigned char> full_i, full_j;
    if (brute) { full_i.assign((size_t)n * B * M, 0); full_j.assign((size_t)n * B * F, 0); }
    std::vector<int> vseen((size_t)n * B, 0), gseen(want_grad ? (size_t)n * B * d : 0, 0), xseen((size_t)n * B * d, 0);
    auto lds_ok = [&](long long off) { if (off < 0 || off >= LD.floats) ++bad; };
    auto w_ok = [&](size_t off) { if (off >= L.total) ++bad; };
    // the (i, j) walk does not depend on the tile: emulate it once per sample, the loads of x and the outputs for every workgroup
    for (int s = 0; s < n; ++s) {
        std::vector<int> ci((size_t)M, 0), cj((size_t)F, 0);
        for (int c0 = 0; c0 < M; c0 += PP_CH) {
            const int nc = M - c0 < PP_CH ? M - c0 : PP_CH;
            std::vector<int> staged((size_t)LD.floats, 0);
            for (int tid = 0; tid < NT; ++tid) {
                for (int t = tid; t < nc * (D / 4); t += NT)
                    for (int e = 0; e < 4; ++e) {
                        const long long oz = LD.o_z + 4 * t + e, og = LD.o_g + 4 * t + e;
                        lds_ok(oz); lds_ok(og);
                        if (oz >= LD.o_g || og >= LD.o_a) ++bad; else { ++staged[oz]; ++staged[og]; }
                        w_ok(L.o_z + (size_t)c0 * D + 4 * t + e); if (L.o_z + (size_t)c0 * D + 4 * t + e >= L.o_om) ++bad;
                        w_ok(L.o_g + ((size_t)s * M + c0) * D + 4 * t + e);
                    }
                if (tid < nc) {
                    lds_ok(LD.o_a + tid); ++staged[LD.o_a + tid];
                    w_ok(L.o_a + (size_t)s * L.Mr + c0 + tid); if (L.o_a + (size_t)s * L.Mr + c0 + tid >= L.o_ap) ++bad;
                }
            }
            for (int slice = 0; slice < PP_NW; ++slice)
                for (int i = paths_own_first(slice); i < nc; i += PP_NW) {
                    for (int k = 0; k < D; ++k)                                 // every float read was staged exactly once in this chunk
                        if (staged[LD.o_z + i * D + k] != 1 || staged[LD.o_g + i * D + k] != 1) ++bad;
                    if (staged[LD.o_a + i] != 1) ++bad;
                    ++ci[(size_t)c0 + i];
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
                if (tid < nf) {
                    lds_ok(LD.o_ph + tid); ++staged[LD.o_ph + tid]; if (L.o_ph + j0 + tid >= L.o_a) ++bad;
                    lds_ok(LD.o_w + tid); ++staged[LD.o_w + tid];
                    if (L.o_wq + (size_t)s * L.Fr + j0 + tid >= L.o_g || L.o_wq + (size_t)s * L.Fr + j0 + tid < L.o_wq) ++bad;
                }
            }
            for (int slice = 0; slice < PP_NW; ++slice)
                for (int j = paths_own_first(slice); j < nf; j += PP_NW) {
                    for (int k = 0; k < D; ++k) if (staged[LD.o_om + j * D + k] != 1) ++bad;
                    if (staged[LD.o_ph + j] != 1 || staged[LD.o_w + j] != 1) ++bad;
                    ++cj[(size_t)j0 + j];
                }
        }
        for (int i = 0; i < M; ++i) bad += ci[i] != 1;
        for (int j = 0; j < F; ++j) bad += cj[j] != 1;
        // reduction image, loads of x and output stores of every workgroup of this sample
        for (int lane = 0; lane < 64; ++lane)
            for (int k = 0; k <= D; ++k) lds_ok(LD.o_red + paths_own_red(lane, k, D));
        for (int tile = 0; tile < ntiles; ++tile) {
            const long long b0 = (long long)tile * PP_TP;
            const int npts = (int)(B - b0 < PP_TP ? B - b0 : PP_TP);
            if (npts < 1) ++bad;
            const size_t so = paths_own_row(s, B, b0);
            for (int tid = 0; tid < NT; ++tid) {
                const int lane = tid & 63;
                if (tid < 64)                                                  // (every wave loads the same x; counted for wave 0)
                    for (int k = 0; k < D; ++k)
                        if (k < d && b0 + lane < B) {
                            if ((so + lane) * d + k >= (size_t)n * B * d) ++bad; else ++xseen[(so + lane) * d + k];
                        }
                if (tid < npts) {
                    lds_ok(LD.o_red + paths_own_red(tid, D, D));
                    if (so + tid >= (size_t)n * B) ++bad; else ++vseen[so + tid];
                    if (brute) {
                        for (int i = 0; i < M; ++i) full_i[(so + tid) * M + i] += ci[i];
                        for (int j = 0; j < F; ++j) full_j[(so + tid) * F + j] += cj[j];
                    }
                }
                if (want_grad)
                    for (int t = tid; t < npts * d; t += NT) {
                        const int pt = t / d, k = t - pt * d;
                        lds_ok(LD.o_red + paths_own_red(pt, k, D));
                        if (pt >= npts || k >= d || so * d + t >= (size_t)n * B * d) ++bad; else ++gseen[so * d + t];
                    }
            }
        }
    }
    for (int v : vseen) bad += v != 1;
    for (int v : gseen) bad += v != 1;
    for (int v : xseen) bad += v != 1;
    if (brute) {
        for (unsigned char v : full_i) bad += v != 1;
        for (unsigned char v : full_j) bad += v != 1;
    }
    printf("fused    d %4d M %4d F %5d n %3d B %6d%s: D %2d, %5d tiles x %3d samples, LDS %5d B%s  %s\n", d, M, F, n, B,
           want_grad ? " +grad" : "      ", D, ntiles, n, LD.floats * 4, brute ? ", 3-D counts formed" : "", bad ? "FAILED" : "ok");
    bad_total += bad;
    return bad ? 1 : 0;
}

static int check_composed(int d, int M, int F, int n, int B, bool want_grad) {
    PathsOwnWork S;
    long long bad = 0;
    if (paths_own_work(M, d, F, n, B, want_grad, S)) { printf("composed d %4d M %4d F %5d n %3d B %6d: refused\n", d, M, F, n, B); ++bad_total; return 1; }
    const size_t N = (size_t)S.N;
    struct Reg { size_t off, len; } regs[] = {
        {S.o_x, N * S.ldw}, {S.o_xn, S.Nr}, {S.o_k, N * S.ldM}, {S.o_t, N * S.ldF}, {S.o_vp, S.Nr}, {S.o_p, N * S.ldM}, {S.o_sig, S.Nr},
        {S.o_o1, want_grad ? N * S.ldw : 0}, {S.o_o2, want_grad ? N * S.ldw : 0}, {S.o_gp, want_grad ? N * S.ldw : 0}};
    size_t end = 0;
    for (auto& r : regs) {
        if (r.off % 4 || r.off != end) ++bad;                                   // aligned, back to back: disjoint
        end = r.off + r.len;
    }
    if (end != S.total || S.N != (long long)n * B || S.Nr < N || S.ldM < M || S.ldF < F || S.ldw < d) ++bad;
    // the per-sample products: the row block of sample s starts 16-byte aligned and ends inside its region
    for (int s = 0; s < n; ++s) {
        if (((size_t)s * B * S.ldw) % 4 || ((size_t)s * B * S.ldM) % 4) ++bad;
        if ((size_t)s * B * S.ldM + (size_t)(B - 1) * S.ldM + M > N * S.ldM) ++bad;                              // S2_s, K_s
        if ((size_t)s * B * S.ldw + (size_t)(B - 1) * S.ldw + d > N * S.ldw) ++bad;                              // X~_s, O2_s
    }
    printf("composed d %4d M %4d F %5d n %3d B %6d%s: %8lld rows, %3d launches, workspace %8.1f MiB  %s\n", d, M, F, n, B,
           want_grad ? " +grad" : "      ", S.N, want_grad ? 10 + 2 * n : 7 + n, S.total * 4.0 / 1048576.0, bad ? "FAILED" : "ok");
    bad_total += bad;
    return bad ? 1 : 0;
}

static int check_descend(int d, int M, int F, int n, int B) {
    PathsDescendWork S;
    long long bad = 0;
    if (paths_descend_work(M, d, F, n, B, S)) { printf("descend  d %4d M %4d F %5d n %3d B %6d: refused\n", d, M, F, n, B); ++bad_total; return 1; }
    const size_t N = (size_t)n * B;
    if (S.o_y != 0 || S.o_gy < N * d || S.o_fy < S.o_gy + N * d || S.o_eval < S.o_fy + N || S.o_gy % 4 || S.o_fy % 4 || S.o_eval % 4) ++bad;
    size_t ev = 0;
    if (d > PP_FUSED_MAX_D) {
        PathsOwnWork W;
        if (paths_own_work(M, d, F, n, B, 1, W)) ++bad; else ev = W.total;
    }
    if (S.total != S.o_eval + ev) ++bad;
    // the step kernel: one wave per pair, lanes over k -- every (pair, k) once, nothing past N
    const int blocks = (int)((N + 3) / 4);
    std::vector<int> seen(N * d < 4000000 ? N * d : 0, 0);
    if (!seen.empty()) {
        for (int blk = 0; blk < blocks; ++blk)
            for (int tid = 0; tid < 256; ++tid) {
                const size_t pair = (size_t)blk * 4 + (tid >> 6);
                if (pair >= N) continue;
                for (int k = tid & 63; k < d; k += 64) ++seen[pair * d + k];
            }
        for (int v : seen) bad += v != 1;
    }
    printf("descend  d %4d M %4d F %5d n %3d B %6d: workspace %8.1f MiB  %s\n", d, M, F, n, B, S.total * 4.0 / 1048576.0, bad ? "FAILED" : "ok");
    bad_total += bad;
    return bad ? 1 : 0;
}

int main() {
    // (d, M, F, n, B): the shapes of tests/test_gpu_paths_own.py (its slices and descent sub-cases included) and of tools/paths_own_probe.py
    const int fused[][5] = {{3, 12, 64, 3, 70}, {5, 40, 100, 5, 130}, {20, 70, 128, 4, 33}, {32, 16, 96, 2, 65}, {5, 19, 1, 1, 67},
                            {3, 12, 64, 3, 40}, {3, 12, 64, 2, 70}, {5, 40, 100, 2, 130}, {20, 70, 128, 2, 33}, {3, 12, 64, 3, 20},
                            {5, 40, 100, 5, 32}, {32, 16, 96, 2, 20}, {5, 40, 100, 5, 4}, {20, 500, 2048, 64, 64}, {20, 500, 2048, 5, 5000},
                            {20, 500, 2048, 64, 4096}, {1, 1, 1, 1, 1}, {32, 129, 65, 17, 129}};
    const int composed[][5] = {{33, 16, 128, 4, 40}, {200, 24, 160, 3, 40}, {33, 16, 128, 4, 20}, {200, 24, 160, 3, 12}, {33, 16, 128, 2, 40},
                               {200, 512, 2048, 5, 64}, {4035, 512, 2048, 5, 64}, {33, 1, 1, 1, 1}, {200, 512, 2048, 64, 512}};
    for (auto& s : fused) { check_fused(s[0], s[1], s[2], s[3], s[4], true); check_fused(s[0], s[1], s[2], s[3], s[4], false); }
    for (int d = 1; d <= 32; ++d) { check_fused(d, 67, 70, 11, 67, true); check_fused(d, 67, 70, 11, 67, false); }
    for (auto& s : composed) { check_composed(s[0], s[1], s[2], s[3], s[4], true); check_composed(s[0], s[1], s[2], s[3], s[4], false); }
    for (auto& s : fused) check_descend(s[0], s[1], s[2], s[3], s[4]);
    for (auto& s : composed) check_descend(s[0], s[1], s[2], s[3], s[4]);
    PathsOwnWork S;
    PathsDescendWork T;
    bad_total += (paths_own_work(0, 40, 8, 1, 1, 1, S) == 0) + (paths_own_work(8, 40, 8, 1, 0, 1, S) == 0) +
                 (paths_own_work(500, 200, 2048, 64, 40000, 1, S) == 0) +           // n B ldF passes 2^31: refused
                 (paths_descend_work(8, 40, 8, 1, 0, T) == 0) + (paths_descend_work(500, 200, 2048, 64, 40000, T) == 0) +
                 (paths_descend_work(12, 3, 64, 65535, 65535, T) == 0);             // n B passes 2^31: refused
    printf(bad_total ? "paths own: FAILED\n"
                     : "paths own: every (sample, point, i) and (sample, point, j) visited exactly once, every offset in bounds\n");
    return bad_total ? 1 : 0;
}
