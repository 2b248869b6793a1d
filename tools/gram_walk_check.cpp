// Host check of the stream-K walk of gemm32_gram_kernel: includes the arithmetic the kernel uses (csrc/gram_walk.h) and emulates, for
// the shapes of tests/test_gpu_gemm32_gram.py and the flagship, every workgroup's list of units.  Shows that every (tile, stage) is
// covered exactly once, that every unit stays inside one tile (and one K chunk), that tiles lie in the lower triangle, and that the
// block -> workgroup map is a bijection.  No GPU.
//   g++ -O2 -std=c++17 -I gp-derivatives-variational-inference_amd/csrc tools/gram_walk_check.cpp -o gram_walk_check && ./gram_walk_check
#include <cstdio>
#include <vector>

#include "gram_walk.h"

static int check(int M, int N, int K, int nwg, int kchunks, bool verbose) {
    const GramWalk w = gram_walk_make(M, N, K, 256, 32, kchunks);
    std::vector<int> seen((size_t)w.tiles_m * w.tiles_n * w.S, 0);
    int bad = 0, max_units = 0, min_st = 1 << 30, max_st = 0;
    long long covered = 0, units = 0;
    const int grid = (nwg + 7) / 8 * 8;
    std::vector<int> wgs(grid, 0);
    for (int b = 0; b < grid; ++b) {
        const int wg = gram_walk_wg(b, grid);
        if (wg < 0 || wg >= grid || wgs[wg]++) { ++bad; continue; }
        if (wg >= nwg) continue;
        long long g, g1;
        gram_walk_range(w, wg, nwg, g, g1);
        if (g < 0 || g1 > w.G || g > g1) ++bad;
        int nu = 0;
        while (g < g1) {
            const GramUnit u = gram_walk_unit(w, g, g1);
            const int n = u.s1 - u.s0;
            if (n < 1 || u.s0 < 0 || u.s1 > w.S || u.tm < 0 || u.tm >= w.tiles_m || u.tn < 0 || u.tn >= w.tiles_n || u.tn > u.tm) { ++bad; break; }
            if (u.s0 / w.Sc != (u.s1 - 1) / w.Sc) ++bad;                       // one K chunk
            for (int s = u.s0; s < u.s1; ++s) ++seen[((size_t)u.tm * w.tiles_n + u.tn) * w.S + s];
            if (verbose) printf("    wg %3d: tile (%d, %d) stages [%d, %d)\n", wg, u.tm, u.tn, u.s0, u.s1);
            g += n; covered += n; ++nu; ++units;
            if (n < min_st) min_st = n;
            if (n > max_st) max_st = n;
        }
        if (nu > max_units) max_units = nu;
    }
    long long want = 0;
    for (int tm = 0; tm < w.tiles_m; ++tm)
        for (int tn = 0; tn < w.tiles_n; ++tn)
            for (int s = 0; s < w.S; ++s) {
                const int expect = tn <= tm ? 1 : 0;
                want += expect;
                if (seen[((size_t)tm * w.tiles_n + tn) * w.S + s] != expect) ++bad;
            }
    if (covered != w.G || want != w.G) ++bad;
    printf("M %5d N %5d K %6d  W %3d  chunks %d: %3d tiles x %4d stages = %7lld, %5lld units (<= %d per workgroup, %d..%d stages)  %s\n", M, N, K, nwg,
           w.nchunk, w.ntiles, w.S, w.G, units, max_units, units ? min_st : 0, max_st, bad ? "FAILED" : "ok");
    return bad;
}

int main(int argc, char** argv) {
    const int shapes[][3] = {{512, 512, 512}, {601, 600, 1300}, {601, 600, 16384}, {3001, 3000, 1024}, {640, 640, 1024},
                             {3001, 3000, 24576}, {3301, 3300, 5632}, {3001, 3000, 3072}, {700, 520, 545}, {520, 700, 545}};
    const int wgs[] = {1, 7, 256, 304};
    int bad = 0;
    for (auto& s : shapes)
        for (int kc : {1, 3})
            for (int w : wgs) bad += check(s[0], s[1], s[2], w, kc, false);
    if (argc > 1) check(601, 600, 1300, 7, 1, true);
    printf(bad ? "gram walk: FAILED\n" : "gram walk: every (tile, stage) covered exactly once\n");
    return bad ? 1 : 0;
}
