// Host check of the team / group / LDS index algebra of the per-point covariance roots (csrc/block_roots.hip): includes the arithmetic
// the three kernels and their launchers use (csrc/block_roots_plan.h) and emulates every thread of every workgroup serially, for every
// q in 1..96 at ragged batch sizes.  Shows that
//   * every element (i, j) of every block b < B is staged exactly once and written exactly once (the e = t, t + T, ... walk), every row
//     is owned by exactly one (team lane, h), and logdet / info / logp of a block are written by exactly one thread;
//   * every item (draw i, row a) of the draw is computed exactly once;
//   * every LDS offset the kernels form -- the staged elements, the rows and columns of the factorisation, the pad column -- lies inside
//     the team's own image and inside the dynamic LDS the launcher asks for, which stays below the CU's 160 KB;
//   * every global offset lies inside [B, q, q], [B q], [B] or [n, B q];
//   * teams past B touch nothing.
// No GPU.
//   g++ -O2 -std=c++17 -I gp-derivatives-variational-inference_amd/csrc tools/block_roots_check.cpp -o block_roots_check && ./block_roots_check
#include <cstdio>
#include <vector>

#include "block_roots_plan.h"

static long long g_bad = 0;
#define EXPECT(c) do { if (!(c)) { if (g_bad < 10) printf("  line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

static int check(int B, int q, int n, bool quiet) {
    const long long bad0 = g_bad;
    BlockRootsPlan w;
    if (block_roots_plan(B, q, w)) { printf("B %5d q %2d: refused\n", B, q); return 1; }
    const int T = w.T, G = w.G, ld = w.ld, img = w.img, qq = q * q;
    EXPECT(T >= q || T == 64);
    EXPECT(q <= BR_ROWS * T);
    EXPECT(w.nthreads == G * T && (w.nthreads == 256 || w.nthreads == 64));
    EXPECT(ld == q + 1 && img == q * ld);
    EXPECT(w.lds_bytes == sizeof(double) * (size_t)G * img && w.lds_bytes <= 160u * 1024u);
    EXPECT((long long)w.ngroups * G >= B && (long long)(w.ngroups - 1) * G < B);
    const long long lds_doubles = (long long)G * img;
    const long long ncols = (long long)B * q;

    std::vector<int> staged((size_t)B * qq, 0), written((size_t)B * qq, 0), rows((size_t)B * q, 0), scal(B, 0), zout((size_t)B * q, 0);
    std::vector<int> items((size_t)B * q * n, 0);
    for (int group = 0; group < w.ngroups; ++group)
        for (int tid = 0; tid < w.nthreads; ++tid) {
            const int team = block_roots_team_of(tid, T), t = block_roots_lane_of(tid, T);
            EXPECT(team >= 0 && team < G && t >= 0 && t < T && team * T + t == tid);
            const long long b = block_roots_block(group, G, team);
            if (b >= B) continue;                                                  // the team idles through the barriers
            const long long lo = (long long)team * img, hi = lo + img;             // the team's own image
            auto lds = [&](int i, int j) {
                const long long o = block_roots_lds(team, img, ld, i, j);
                EXPECT(o >= lo && o < hi && o < lds_doubles);
            };
            // staging and the output walk: e = t, t + T, ...
            for (int e = t; e < qq; e += T) {
                const int i = e / q, j = e - i * q;
                EXPECT(i >= 0 && i < q && j >= 0 && j < q);
                lds(i, j);
                const long long g = b * qq + e;
                EXPECT(g >= 0 && g < (long long)B * qq);
                ++staged[g];
                ++written[g];
            }
            // rows: factorisation columns k, substitution columns c
            for (int h = 0; h < BR_ROWS; ++h) {
                const int i = t + h * T;
                if (i >= q) continue;
                ++rows[b * q + i];
                lds(i, q);                                                         // pad column: sqrt(pivot), z_i
                lds(i, i);
                for (int k = 0; k <= i; ++k) {                                     // s_i of column k reads (i, 0..k) and (k, 0..k-1)
                    lds(i, k);
                    lds(k, k);
                    lds(k, q);
                    if (k > 0) { lds(i, k - 1); lds(k, k - 1); }
                    lds(i, 0);
                    lds(k, 0);
                }
                EXPECT(b * q + i < ncols);                                         // y, mu
            }
            for (int i = t; i < q; i += T) { EXPECT(b * q + i < ncols); ++zout[b * q + i]; }
            if (t == 0) {
                ++scal[b];
                for (int i = 0; i < q; ++i) { lds(i, i); lds(i, q); }
            }
            // draw items
            const long long nitems = (long long)n * q;
            for (long long it = t; it < nitems; it += T) {
                const long long i = it / q;
                const int a = (int)(it - i * q);
                EXPECT(i >= 0 && i < n && a >= 0 && a < q);
                lds(a, 0);
                lds(a, a);
                const long long g = i * ncols + b * q + a;                         // eps (c <= a: below it) and out
                EXPECT(g >= 0 && g < (long long)n * ncols && i * ncols + b * q >= 0);
                ++items[g];
            }
        }
    for (int v : staged) EXPECT(v == 1);
    for (int v : written) EXPECT(v == 1);
    for (int v : rows) EXPECT(v == 1);
    for (int v : scal) EXPECT(v == 1);
    for (int v : zout) EXPECT(v == 1);
    for (int v : items) EXPECT(v == 1);
    const bool bad = g_bad != bad0;
    if (!quiet || bad)
        printf("B %5d q %2d n %2d: team %2d lanes, %2d blocks x %3d threads per workgroup, %5d workgroups, LDS %6u bytes  %s\n", B, q, n, T, G,
               w.nthreads, w.ngroups, w.lds_bytes, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main() {
    int bad = 0;
    // the shapes of tests/test_gpu_block_roots.py: both sides of every team width, one and two rows per lane, the largest image
    const int qs[] = {1, 2, 3, 6, 8, 9, 16, 17, 21, 32, 33, 64, 65, 96};
    for (int q : qs)
        for (int B : {1, 37, 130}) bad += check(B, q, 5, B != 37);
    int badq = 0;
    for (int q = 1; q <= 96; ++q) badq += check(37, q, 3, true) + check(263, q, 1, true);
    printf("B 37 / 263, q 1..96: %s\n", badq ? "FAILED" : "ok");
    bad += badq + check(4096, 6, 2, false) + check(4096, 96, 1, false) + check(65536, 4, 1, false);
    BlockRootsPlan w;
    bad += (block_roots_plan(10, 97, w) == 0) + (block_roots_plan(10, 0, w) == 0) + (block_roots_plan(0, 5, w) == 0);
    printf(bad ? "block roots: FAILED\n" : "block roots: every element, row and draw item owned exactly once, every offset in bounds\n");
    return bad ? 1 : 0;
}
