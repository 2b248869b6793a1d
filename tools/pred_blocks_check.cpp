// Host check of the tile / group / slice index algebra of the per-point predictive covariance blocks (csrc/predict_blocks.hip): includes
// the arithmetic the kernel uses (csrc/pred_blocks_plan.h) and emulates, for the shapes of tests/test_gpu_blocks.py and of
// tools/blocks_probe.py, every workgroup's (group, slice), every wave's live tile pairs, every lane's four accumulator elements and the
// chunk walk over the slice's rows.  Shows that every (point, a, b <= a, row) is covered exactly once, that no wave holds more than 6
// pairs, that every global read stays inside [Mp, B q], every LDS offset inside the 32 x 112 image and every workspace write inside
// the bytes the helper reports.  A workgroup applies one element map to all of its rows, so the 4-D count is the product of the
// group's element count and the slice's row count; both are checked to be 1 everywhere, and for the small shapes the 4-D count is
// also formed outright.  No GPU.
//   g++ -O2 -std=c++17 -I gp-derivatives-variational-inference_amd/csrc tools/pred_blocks_check.cpp -o pred_blocks_check && ./pred_blocks_check
#include <cstdio>
#include <vector>

#include "pred_blocks_plan.h"

static int check(int Mp, int B, int pd, bool quiet = false) {
    PredBlocksPlan w;
    if (pred_blocks_plan(Mp, B, pd, w)) { printf("Mp %5d B %5d pd %2d: refused\n", Mp, B, pd); return 1; }
    const int q = w.q;
    long long bad = 0;
    int max_pairs = 0, live = 0;
    if (w.Tc > PB_TMAX || w.Tcp > PB_TMAX || w.ld % 32 != 16 || w.ld < w.Tcp || w.ld > PB_TMAX + 16 || w.rps % PB_KC || w.nslices > 32) ++bad;
    const size_t ws_floats = (size_t)w.nslices * B * q * q;
    const bool brute = (double)B * q * (q + 1) / 2 * Mp < 5e7;
    std::vector<unsigned char> full;
    if (brute) full.assign((size_t)B * q * q * Mp, 0);

    // rows: every slice walks its rows in chunks of 32, wave w the rows w, w + 4, ... of a chunk
    std::vector<int> rowseen(Mp, 0);
    for (int s = 0; s < w.nslices; ++s) {
        const int r0 = s * w.rps, r1 = r0 + w.rps < Mp ? r0 + w.rps : Mp;
        if (r0 >= Mp) ++bad;
        for (int k0 = r0; k0 < r1; k0 += PB_KC)
            for (int wave = 0; wave < 4; ++wave)
                for (int i = 0; i < PB_KC / 4; ++i) {
                    const int r = k0 + i * 4 + wave;
                    if ((i * 4 + wave) * w.ld + w.Tcp > PB_KC * (PB_TMAX + 16)) ++bad;       // LDS store
                    if (r < r1) ++rowseen[r];                                              // (rows past r1 are staged as zeros)
                }
    }
    for (int r = 0; r < Mp; ++r) bad += rowseen[r] != 1;

    // elements: per group, every wave's pairs and every lane's four accumulator elements
    for (int g = 0; g < w.ngroups; ++g) {
        const long long col0 = (long long)g * w.Tc;
        const int cols = (int)(w.Tc < w.ncols - col0 ? w.Tc : w.ncols - col0);
        if (cols <= 0 || cols % q || col0 + cols > w.ncols) ++bad;                          // global reads: columns col0 .. col0 + cols - 1
        const int npts = cols / q;
        std::vector<int> seen((size_t)npts * q * q, 0);
        live = 0;
        for (int wave = 0; wave < 4; ++wave) {
            int np = 0;
            for (int i = 0; i < PB_MAXPAIRS + 2; ++i) {
                int ti = 0, tj = 0;
                if (!pred_blocks_pair(wave + 4 * i, w.ntile, q, w.Tc, ti, tj)) continue;
                if (i >= PB_MAXPAIRS || i != np) { ++bad; continue; }                       // at most 6, and a prefix of the slots
                ++np; ++live;
                if (tj > ti || ti >= w.ntile) ++bad;
                for (int lane = 0; lane < 64; ++lane) {
                    const int oi = ti * 16 + (lane & 15) + (lane >> 4) * w.ld, oj = tj * 16 + (lane & 15) + (lane >> 4) * w.ld;
                    if ((PB_KC - 4) * w.ld + oi >= PB_KC * (PB_TMAX + 16) || (PB_KC - 4) * w.ld + oj >= PB_KC * (PB_TMAX + 16)) ++bad;
                    if ((ti * 16 + (lane & 15)) >= w.Tcp) ++bad;                            // fragments read staged columns only
                    for (int r = 0; r < 4; ++r) {
                        int pt, a, b;
                        if (!pred_blocks_element(ti * 16 + (lane >> 4) * 4 + r, tj * 16 + (lane & 15), q, cols, pt, a, b)) continue;
                        if (pt < 0 || pt >= npts || a < 0 || a >= q || b < 0 || b > a) { ++bad; continue; }
                        ++seen[((size_t)pt * q + a) * q + b];
                        for (int s = 0; s < w.nslices; ++s) {
                            const size_t off = (((size_t)s * B + (size_t)g * w.G + pt) * q + a) * q + b;
                            if (off >= ws_floats || (size_t)g * w.G + pt >= (size_t)B) ++bad;
                        }
                    }
                }
            }
            if (np > max_pairs) max_pairs = np;
        }
        for (int pt = 0; pt < npts; ++pt)
            for (int a = 0; a < q; ++a)
                for (int b = 0; b < q; ++b) {
                    const int n = seen[((size_t)pt * q + a) * q + b];
                    bad += n != (b <= a ? 1 : 0);
                    if (brute && n)
                        for (int r = 0; r < Mp; ++r) full[((((size_t)g * w.G + pt) * q + a) * q + b) * Mp + r] += n * rowseen[r];
                }
    }
    if (brute)
        for (int pt = 0; pt < B; ++pt)
            for (int a = 0; a < q; ++a)
                for (int b = 0; b < q; ++b)
                    for (int r = 0; r < Mp; ++r) bad += full[(((size_t)pt * q + a) * q + b) * Mp + r] != (b <= a ? 1 : 0);
    if (!quiet || bad)
        printf("Mp %5d B %5d pd %2d: G %2d strip %2d (%d tiles, ld %3d), %2d live pairs of %2d (<= %d per wave), %5d groups x %2d slices of %4d rows%s  %s\n",
           Mp, B, pd, w.G, w.Tc, w.ntile, w.ld, live, w.ntile * (w.ntile + 1) / 2, max_pairs, w.ngroups, w.nslices, w.rps,
           brute ? ", 4-D count formed" : "", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main() {
    // (Mp = M (p + 1), B, pd): the nine shapes of tests/test_gpu_blocks.py, its memory test, the probe's shapes, every q at a ragged B
    const int shapes[][3] = {{120, 128, 0}, {120, 128, 2}, {120, 67, 5}, {132, 70, 1}, {19, 67, 5}, {384, 33, 20}, {96, 40, 7}, {27, 5, 95},
                             {1200, 9, 5}, {32, 4096, 5}, {3000, 4096, 0}, {3000, 4096, 5}, {3000, 4096, 20}, {600, 512, 5},
                             {2048, 2048, 0}, {2048, 2048, 3}};
    int bad = 0;
    for (auto& s : shapes) bad += check(s[0], s[1], s[2]);
    int badq = 0;
    for (int pd = 0; pd <= 95; ++pd) badq += check(257, 37, pd, true);
    printf("Mp   257 B    37 pd 0..95: %s\n", badq ? "FAILED" : "ok");
    PredBlocksPlan w;
    bad += badq + (pred_blocks_plan(100, 10, 96, w) == 0) + (pred_blocks_plan(0, 10, 1, w) == 0) + (pred_blocks_plan(10, 0, 1, w) == 0);
    printf(bad ? "pred blocks: FAILED\n" : "pred blocks: every (point, a, b <= a, row) covered exactly once\n");
    return bad ? 1 : 0;
}
