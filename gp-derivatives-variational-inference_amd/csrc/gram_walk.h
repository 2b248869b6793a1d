// The stream-K walk of gemm32_gram_kernel (gemm32.hip): which (tile, stage range) units a workgroup computes.  Plain arithmetic on
// integers, shared between the kernel, its launcher and the host check tools/gram_walk_check.cpp (which shows, for the shapes of the
// tests and workgroup counts 1 / 7 / 256 / 304, that every (tile, stage) is covered exactly once).
//
// A lower-triangular output of tiles_m x tiles_n tiles has its tiles numbered as pick_unit numbers them: tn <= tm row by row while
// tm < tiles_n, full rows of tiles_n tiles below.  A tile has S = ceil(K / 32) stages of 32 k.  The K range may be cut into chunks of
// Sc stages (the last one shorter): the global stage index runs chunk by chunk, inside a chunk tile by tile, inside a tile stage by
// stage -- with one chunk (Sc = S) it is g = t S + s.  Workgroup w of W walks the contiguous range [w G / W, (w + 1) G / W) of
// g < G = ntiles S; a range is cut into units at every (tile, chunk) boundary, and a unit is what one accumulator set holds: its
// partial sum is added into the output when the unit ends.
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
};
struct GramUnit { int tm, tn, s0, s1; };      // stages [s0, s1) of tile (tm, tn), s counted from the start of K

GRAM_WALK_FN GramWalk gram_walk_make(int M, int N, int K, int tile, int bk, int kchunks) {
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

GRAM_WALK_FN void gram_walk_range(const GramWalk& w, int wg, int nwg, long long& g0, long long& g1) {
    g0 = (long long)wg * w.G / nwg;
    g1 = (long long)(wg + 1) * w.G / nwg;
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
