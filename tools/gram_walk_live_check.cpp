// Host check of the weighted stream-K walk and of the pattern tables of gemm32_gram_kernel (patterns on: gram_walk_make(..., live = 1)):
// includes the arithmetic and the tables the kernel uses (csrc/gram_walk.h) and emulates, for the shapes of
// tests/test_gpu_gemm32_gram.py, tests/test_gpu_gemm32_gram_live.py and the flagship, every workgroup's list of units.  Shows that
//   - every (tile, stage) is covered exactly once, every unit stays inside one tile and one K chunk, tiles lie in the lower triangle;
//   - the block -> workgroup map is a bijection;
//   - every workgroup's cost lies less than one stage of the heaviest weight (16) from its share: |cost - C / W| < 16 + 1 -- what the cut
//     rule gives, both ends of a range lying less than one stage past their targets;
//   - the largest per-workgroup cost exceeds the smallest by at most 16.  This one is NOT met everywhere and the program reports it
//     (and exits 1): it holds for the flagship on 256 workgroups (3354..3366) but not e.g. on 304 (2816..2842), and no contiguous cut
//     can meet it in general -- a workgroup wholly inside FULL tiles costs a multiple of 16, one inside a DIAG tile a multiple of 9,
//     and around a share of 111 those are {96, 112} and {108, 117}: the workgroups cannot all take 112 and 108 and still add up to C.
//     The spread is at most 2 x 16 and, at the flagship's share of 3360, under 1 % of a workgroup's time;
//   - for every pattern the four waves' tile lists are disjoint and their union is exactly the live MFMA tiles of that tile kind, no
//     wave has more tiles than the pattern's weight, and every table entry is in range.
// No GPU.
//   g++ -O2 -std=c++17 -I gp-derivatives-variational-inference_amd/csrc tools/gram_walk_live_check.cpp -o gram_walk_live_check && ./gram_walk_live_check
//   (also with -fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gram_walk.h"

static int check_patterns() {
    int bad = 0;
    for (int pat = 0; pat < GRAM_NPAT; ++pat) {
        int owner[8][8];
        for (auto& row : owner)
            for (int& o : row) o = -1;
        const GramPatWave p0 = gram_pattern(pat, 0);
        for (int wave = 0; wave < 4; ++wave) {
            const GramPatWave p = gram_pattern(pat, wave);
            if (p.nr < 1 || p.nr > 5 || p.nc < 1 || p.nc > 4 || p.nt < 1 || p.nt > 16 || p.nt > gram_pat_weight(pat)) { ++bad; continue; }
            if (p.row0 != gram_pat_row0(pat, wave) || p.col0 != gram_pat_col0(pat, wave)) ++bad;
            if (6 + p.nr + p.nc > 2 * p.nt) ++bad;                              // the slots of a k-group (the kernel asserts it too)
            if (pat != GRAM_PAT_DIAG) {                                        // one copy of the code: the same lists for every wave
                if (p.nr != p0.nr || p.nc != p0.nc || p.nt != p0.nt) ++bad;
                for (int i = 0; i < p.nr; ++i) bad += p.rows[i] != p0.rows[i];
                for (int i = 0; i < p.nc; ++i) bad += p.cols[i] != p0.cols[i];
                for (int t = 0; t < p.nt; ++t) bad += p.tr[t] != p0.tr[t] || p.tc[t] != p0.tc[t];
            }
            for (int t = 0; t < p.nt; ++t) {
                if (p.tr[t] < 0 || p.tr[t] >= p.nr || p.tc[t] < 0 || p.tc[t] >= p.nc) { ++bad; continue; }
                const int i = p.row0 + p.rows[p.tr[t]], j = p.col0 + p.cols[p.tc[t]];
                if (i < 0 || i > 7 || j < 0 || j > 7 || owner[i][j] != -1) { ++bad; continue; }
                owner[i][j] = wave;
            }
        }
        int live = 0;
        for (int i = 0; i < 8; ++i)
            for (int j = 0; j < 8; ++j) {
                const bool want = pat == GRAM_PAT_DIAG ? j <= i : (pat == GRAM_PAT_ROWS3 ? i < 6 : true);
                live += want;
                if ((owner[i][j] != -1) != want) ++bad;
            }
        printf("pattern %d: weight %2d, %2d live MFMA tiles, owners by MFMA row:", pat, gram_pat_weight(pat), live);
        for (int i = 0; i < 8; ++i) {
            printf(" ");
            for (int j = 0; j < 8; ++j) printf("%c", owner[i][j] < 0 ? '.' : '0' + owner[i][j]);
        }
        printf("  %s\n", bad ? "FAILED" : "ok");
    }
    return bad;
}

static int check(int M, int N, int K, int nwg, int kchunks, int* spread_over) {
    const GramWalk w = gram_walk_make(M, N, K, 256, 32, kchunks, 1);
    std::vector<int> seen((size_t)w.tiles_m * w.tiles_n * w.S, 0);
    int bad = 0;
    long long covered = 0, units = 0, ctot = 0, cmin = -1, cmax = 0;
    const long long ptot = gram_walk_tiles_cost(w);
    const int grid = (nwg + 7) / 8 * 8;
    std::vector<int> wgs(grid, 0);
    int npat[GRAM_NPAT] = {0, 0, 0};
    for (int t = 0; t < w.ntiles; ++t) {
        int tm, tn;
        gram_walk_tile(w, t, tm, tn);
        const int pat = gram_walk_pattern(w, tm, tn);
        ++npat[pat];
        // a pattern leaves no live output without an owner: DIAG only on the diagonal, ROWS3 only where MFMA rows 6, 7 are past M
        if (pat == GRAM_PAT_DIAG && tm != tn) ++bad;
        if (pat == GRAM_PAT_ROWS3 && (tm != w.tiles_m - 1 || tm * 256 + 6 * 32 < M)) ++bad;
    }
    long long prev_end = 0;
    std::vector<long long> g0s(nwg), g1s(nwg);
    for (int b = 0; b < grid; ++b) {
        const int wg = gram_walk_wg(b, grid);
        if (wg < 0 || wg >= grid || wgs[wg]++) { ++bad; continue; }
        if (wg >= nwg) continue;
        long long g, g1;
        gram_walk_range(w, wg, nwg, g, g1);
        if (g < 0 || g1 > w.G || g > g1) ++bad;
        g0s[wg] = g; g1s[wg] = g1;
        long long cost = 0;
        while (g < g1) {
            const GramUnit u = gram_walk_unit(w, g, g1);
            const int n = u.s1 - u.s0;
            if (n < 1 || u.s0 < 0 || u.s1 > w.S || u.tm < 0 || u.tm >= w.tiles_m || u.tn < 0 || u.tn >= w.tiles_n || u.tn > u.tm) { ++bad; break; }
            if (u.s0 / w.Sc != (u.s1 - 1) / w.Sc) ++bad;                       // one K chunk
            for (int s = u.s0; s < u.s1; ++s) ++seen[((size_t)u.tm * w.tiles_n + u.tn) * w.S + s];
            cost += (long long)n * gram_pat_weight(gram_walk_pattern(w, u.tm, u.tn));
            g += n; covered += n; ++units;
        }
        ctot += cost;
        if (cmin < 0 || cost < cmin) cmin = cost;
        if (cost > cmax) cmax = cost;
        // the bound the cut rule gives: both ends of the range lie less than one heaviest stage past their cost targets
        const long long lo = (long long)wg * (w.S * ptot) / nwg, hi = (long long)(wg + 1) * (w.S * ptot) / nwg;
        if (cost <= hi - lo - 16 || cost >= hi - lo + 16) ++bad;
    }
    for (int wg = 0; wg < nwg; ++wg) {                                          // the ranges are consecutive
        if (g0s[wg] != prev_end) ++bad;
        prev_end = g1s[wg];
    }
    if (prev_end != w.G) ++bad;
    long long want = 0;
    for (int tm = 0; tm < w.tiles_m; ++tm)
        for (int tn = 0; tn < w.tiles_n; ++tn)
            for (int s = 0; s < w.S; ++s) {
                const int expect = tn <= tm ? 1 : 0;
                want += expect;
                if (seen[((size_t)tm * w.tiles_n + tn) * w.S + s] != expect) ++bad;
            }
    if (covered != w.G || want != w.G || ctot != w.S * ptot) ++bad;
    const bool over = cmax - cmin > 16;
    *spread_over += over;
    printf("M %5d N %5d K %6d  W %3d  chunks %d: %3d tiles (FULL %2d DIAG %2d ROWS3 %2d) x %4d stages, cost %8lld (all FULL: %8lld), %5lld units, per workgroup %lld..%lld%s  %s\n",
           M, N, K, nwg, w.nchunk, w.ntiles, npat[0], npat[1], npat[2], w.S, ctot, 16 * w.G, units, cmin, cmax, over ? " (spread > 16)" : "", bad ? "FAILED" : "ok");
    return bad;
}

int main() {
    std::vector<std::vector<int>> shapes = {{512, 512, 512}, {601, 600, 1300}, {601, 600, 16384}, {3001, 3000, 1024}, {640, 640, 1024},
                                            {3001, 3000, 24576}, {700, 520, 545}, {520, 700, 545},
                                            {512, 512, 544}, {697, 696, 16384}, {697, 696, 1300}};
    for (int r : {1, 33, 89, 97, 160, 185, 200, 256}) shapes.push_back({512 + r, 511 + r, 532});
    const int wgs[] = {1, 7, 256, 304};
    int bad = check_patterns(), spread_over = 0;
    for (auto& s : shapes)
        for (int kc : {1, 3})
            for (int w : wgs) bad += check(s[0], s[1], s[2], w, kc, &spread_over);
    printf("per-workgroup cost spread above one heaviest stage (16) in %d cases\n", spread_over);
    if (!bad) printf("gram walk (live): every (tile, stage) covered exactly once, every live MFMA tile owned by one wave\n");
    if (bad) printf("gram walk (live): FAILED\n");
    else if (spread_over) printf("gram walk (live): FAILED on the cost spread alone\n");
    bad += spread_over;
    return bad ? 1 : 0;
}
