// The stream-K walk of gemm32_gram_kernel (gemm32.hip): which (tile, stage range) units a workgroup computes, and which MFMA tiles of a
// 256 x 256 tile each of its four waves owns.  Plain arithmetic on integers, shared between the kernel, its launcher and the host checks
// tools/gram_walk_check.cpp (the equal-count walk) and tools/gram_walk_live_check.cpp (the weighted walk and the pattern tables): for the
// shapes of the tests and workgroup counts 1 / 7 / 256 / 304 every (tile, stage) is covered exactly once.
//
// A lower-triangular output of tiles_m x tiles_n tiles has its tiles numbered as pick_unit numbers them: tn <= tm row by row while
// tm < tiles_n, full rows of tiles_n tiles below.  A tile has S = ceil(K / 32) stages of 32 k.  The K range may be cut into chunks of
// Sc stages (the last one shorter): the global stage index runs chunk by chunk, inside a chunk tile by tile, inside a tile stage by
// stage -- with one chunk (Sc = S) it is g = t S + s.  A workgroup walks a contiguous range of g < G = ntiles S; a range is cut into
// units at every (tile, chunk) boundary, and a unit is what one accumulator set holds: its partial sum is added into the output when
// the unit ends.
//
// Patterns (live = 1).  A tile is 8 x 8 MFMA tiles of 32 x 32; a pattern deals the MFMA tiles that hold live outputs to the four waves,
// every one to exactly ONE wave (an output element still receives one partial sum per unit), and its weight is the MFMA tiles per wave
// and k-step -- what a stage of the tile costs:
//   FULL   16  every wave its 4 x 4 quadrant (all tiles when live = 0; off-diagonal tiles of full tile rows)
//   DIAG    9  tm == tn: the 36 tiles of the lower triangle, 9 per wave (the ragged corner tile too: its dead tiles are skipped when stored)
//   ROWS3  12  off-diagonal tiles of a last tile row with 5 or 6 live MFMA rows: wave row 0 takes MFMA rows 0..2, wave row 1 rows 3..5
// Ranges (live = 1): stages are ordered as above and carry a prefix cost; with C the total cost, workgroup w of W owns the stages whose
// STARTING cost lies in [w C / W, (w + 1) C / W) -- every stage has one starting cost, hence one owner.  With live = 0 workgroup w
// walks [w G / W, (w + 1) G / W), equal stage counts.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define GRAM_WALK_FN __host__ __device__ __forceinline__
#else
#define GRAM_WALK_FN inline
#endif

struct GramWalk {
    int tiles_m, tiles_n, ntiles;
    int S, Sc, nchunk;              // stages per tile, per K chunk, chunks (the last chunk has S - (nchunk - 1) Sc stages)
    long long G;                    // ntiles * S
    int live, rows3;                // patterns on; the last tile row's off-diagonal tiles run ROWS3 (it has 5 or 6 live MFMA rows)
};
struct GramUnit { int tm, tn, s0, s1; };      // stages [s0, s1) of tile (tm, tn), s counted from the start of K

GRAM_WALK_FN GramWalk gram_walk_make(int M, int N, int K, int tile, int bk, int kchunks, int live = 0) {
    GramWalk w;
    w.tiles_m = (M + tile - 1) / tile;
    w.tiles_n = (N + tile - 1) / tile;
    const int tri = w.tiles_m < w.tiles_n ? w.tiles_m : w.tiles_n;
    w.ntiles = tri * (tri + 1) / 2 + (w.tiles_m > tri ? (w.tiles_m - tri) * w.tiles_n : 0);
    w.S = (K + bk - 1) / bk;
    if (kchunks < 1) kchunks = 1;
    w.Sc = (w.S + kchunks - 1) / kchunks;
    if (w.Sc < 1) w.Sc = 1;
    w.nchunk = (w.S + w.Sc - 1) / w.Sc;
    w.G = (long long)w.ntiles * w.S;
    w.live = live ? 1 : 0;
    const int r_last = (M - (w.tiles_m - 1) * tile + 31) / 32;       // live MFMA rows of the last tile row
    w.rows3 = (w.live && tile == 256 && (r_last == 5 || r_last == 6)) ? 1 : 0;
    return w;
}

// tile number -> (tm, tn)
GRAM_WALK_FN void gram_walk_tile(const GramWalk& w, int t, int& tm, int& tn) {
    const int tri = w.tiles_m < w.tiles_n ? w.tiles_m : w.tiles_n, t0 = tri * (tri + 1) / 2;
    if (t < t0) {
        tm = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
        while ((tm + 1) * (tm + 2) / 2 <= t) ++tm;
        while (tm * (tm + 1) / 2 > t) --tm;
        tn = t - tm * (tm + 1) / 2;
    } else {
        tm = tri + (t - t0) / w.tiles_n;
        tn = (t - t0) % w.tiles_n;
    }
}

// block index -> workgroup number: the blocks of one XCD (b, b + 8, ...) get consecutive ranges (grid: a multiple of 8 >= W;
// numbers >= W have no range)
GRAM_WALK_FN int gram_walk_wg(int block, int grid) { return (block >> 3) + (block & 7) * (grid >> 3); }

// ---- patterns: which MFMA tiles of a 256 x 256 tile a wave owns (wave = 2 wr + wc)
enum { GRAM_PAT_FULL = 0, GRAM_PAT_DIAG = 1, GRAM_PAT_ROWS3 = 2, GRAM_NPAT = 3 };
// a wave reads nr row fragments and nc column fragments per k-group: MFMA rows row0 + rows[.] of the left image, MFMA columns
// col0 + cols[.] of the right one; its tile t is (row0 + rows[tr[t]], col0 + cols[tc[t]]) and lives in accumulator set t.
// FULL and ROWS3 have the same rows / cols / tr / tc for every wave (one copy of the code, row0 / col0 at run time); DIAG has row0 = col0 = 0
struct GramPatWave { int nr, nc, nt, row0, col0; int rows[5], cols[4], tr[16], tc[16]; };

constexpr GRAM_WALK_FN int gram_pat_weight(int pat) { return pat == GRAM_PAT_DIAG ? 9 : (pat == GRAM_PAT_ROWS3 ? 12 : 16); }
constexpr GRAM_WALK_FN int gram_pat_row0(int pat, int wave) { return pat == GRAM_PAT_FULL ? 4 * (wave >> 1) : (pat == GRAM_PAT_ROWS3 ? 3 * (wave >> 1) : 0); }
constexpr GRAM_WALK_FN int gram_pat_col0(int pat, int wave) { return pat == GRAM_PAT_DIAG ? 0 : 4 * (wave & 1); }

constexpr GRAM_WALK_FN GramPatWave gram_pattern(int pat, int wave) {
    GramPatWave p{};
    p.row0 = gram_pat_row0(pat, wave);
    p.col0 = gram_pat_col0(pat, wave);
    if (pat != GRAM_PAT_DIAG) {                       // FULL: 4 x 4, ROWS3: 3 x 4, row-major
        p.nr = pat == GRAM_PAT_ROWS3 ? 3 : 4;
        p.nc = 4;
        for (int i = 0; i < p.nr; ++i) p.rows[i] = i;
        for (int j = 0; j < 4; ++j) p.cols[j] = j;
        for (int i = 0; i < p.nr; ++i)
            for (int j = 0; j < 4; ++j) { p.tr[p.nt] = i; p.tc[p.nt] = j; ++p.nt; }
    } else if (wave == 0 || wave == 3) {              // the triangle of MFMA rows o .. o + 3 without its last diagonal tile
        const int o = wave == 0 ? 0 : 4;
        p.nr = 4;
        p.nc = 3;
        for (int i = 0; i < 4; ++i) p.rows[i] = o + i;
        for (int j = 0; j < 3; ++j) p.cols[j] = o + j;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j <= i && j < 3; ++j) { p.tr[p.nt] = i; p.tc[p.nt] = j; ++p.nt; }
    } else {                                          // rows 4..7 x two columns of the block below the diagonal, and one diagonal tile
        const int c = wave == 2 ? 0 : 2, dg = wave == 2 ? 3 : 7;      // wave 2: columns 0, 1 and (3, 3); wave 1: columns 2, 3 and (7, 7)
        p.nc = 3;
        for (int i = 0; i < 4; ++i) p.rows[i] = 4 + i;
        p.cols[0] = c; p.cols[1] = c + 1; p.cols[2] = dg;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 2; ++j) { p.tr[p.nt] = i; p.tc[p.nt] = j; ++p.nt; }
        if (dg == 7) { p.nr = 4; p.tr[p.nt] = 3; } else { p.nr = 5; p.rows[4] = 3; p.tr[p.nt] = 4; }
        p.tc[p.nt] = 2;
        ++p.nt;
    }
    return p;
}

// the pattern of tile (tm, tn); wave-uniform
GRAM_WALK_FN int gram_walk_pattern(const GramWalk& w, int tm, int tn) {
    if (!w.live) return GRAM_PAT_FULL;
    if (tm == tn) return GRAM_PAT_DIAG;
    return (w.rows3 && tm == w.tiles_m - 1) ? GRAM_PAT_ROWS3 : GRAM_PAT_FULL;
}

// cost of one stage of every tile of tile row tm: n_off off-diagonal tiles of weight w_off first, then (has_diag) the diagonal one
GRAM_WALK_FN void gram_walk_row(const GramWalk& w, int tm, int& n_off, int& w_off, int& has_diag) {
    has_diag = tm < w.tiles_n ? 1 : 0;
    n_off = has_diag ? tm : w.tiles_n;
    w_off = gram_pat_weight(gram_walk_pattern(w, tm, -1));
}
GRAM_WALK_FN long long gram_walk_tiles_cost(const GramWalk& w) {     // one stage of every tile
    long long c = 0;
    for (int tm = 0; tm < w.tiles_m; ++tm) {
        int n_off, w_off, has_diag;
        gram_walk_row(w, tm, n_off, w_off, has_diag);
        c += (long long)n_off * w_off + (has_diag ? gram_pat_weight(gram_walk_pattern(w, tm, tm)) : 0);
    }
    return c;
}
// the first global stage index whose starting cost is >= x (0 <= x <= S * tiles_cost; ptot = gram_walk_tiles_cost(w))
GRAM_WALK_FN long long gram_walk_cut(const GramWalk& w, long long ptot, long long x) {
    const long long per = (long long)w.Sc * ptot;                 // cost of a full chunk
    int c = (int)(x / per);
    if (c > w.nchunk - 1) c = w.nchunk - 1;
    long long y = x - (long long)c * per;
    const int len = c == w.nchunk - 1 ? w.S - c * w.Sc : w.Sc;    // stages of this chunk
    long long t = 0, s = 0;                                       // tile and stage inside the chunk
    int tm = 0;
    for (; tm < w.tiles_m; ++tm) {
        int n_off, w_off, has_diag;
        gram_walk_row(w, tm, n_off, w_off, has_diag);
        const long long c_off = (long long)len * w_off, w_dg = has_diag ? gram_pat_weight(gram_walk_pattern(w, tm, tm)) : 0;
        const long long c_row = n_off * c_off + (long long)len * w_dg;
        if (y >= c_row) { y -= c_row; t += n_off + has_diag; continue; }
        long long i = y / c_off, wt = w_off;
        if (i >= n_off) { i = n_off; wt = w_dg; }
        y -= i * c_off;
        t += i;
        s = (y + wt - 1) / wt;                                    // <= len: s == len is stage 0 of the next tile
        break;
    }
    return (long long)c * w.ntiles * w.Sc + t * len + s;
}

GRAM_WALK_FN void gram_walk_range(const GramWalk& w, int wg, int nwg, long long& g0, long long& g1) {
    if (!w.live) {
        g0 = (long long)wg * w.G / nwg;
        g1 = (long long)(wg + 1) * w.G / nwg;
        return;
    }
    const long long ptot = gram_walk_tiles_cost(w), ctot = (long long)w.S * ptot;
    g0 = gram_walk_cut(w, ptot, (long long)wg * ctot / nwg);
    g1 = gram_walk_cut(w, ptot, (long long)(wg + 1) * ctot / nwg);
}

// the unit that starts at global index g of a range that ends at g1 (g < g1 <= G); it has u.s1 - u.s0 >= 1 stages
GRAM_WALK_FN GramUnit gram_walk_unit(const GramWalk& w, long long g, long long g1) {
    const long long per = (long long)w.ntiles * w.Sc;          // global indices per full chunk
    int c = (int)(g / per);
    if (c > w.nchunk - 1) c = w.nchunk - 1;
    const long long rem = g - (long long)c * per;
    const int len = c == w.nchunk - 1 ? w.S - c * w.Sc : w.Sc;   // stages of this chunk
    const int t = (int)(rem / len), sl = (int)(rem - (long long)t * len);
    long long n = len - sl;
    if (n > g1 - g) n = g1 - g;
    GramUnit u;
    gram_walk_tile(w, t, u.tm, u.tn);
    u.s0 = c * w.Sc + sl;
    u.s1 = u.s0 + (int)n;
    return u;
}
