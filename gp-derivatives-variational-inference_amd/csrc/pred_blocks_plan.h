// Tile, group and slice arithmetic of the per-point predictive covariance blocks (predict_blocks.hip).  Plain arithmetic on integers,
// shared between the kernel, its launcher and the host check tools/pred_blocks_check.cpp (which shows, for the shapes of
// tests/test_gpu_blocks.py and of the probe, that every (point, a, b <= a, row) is covered exactly once).
//
// The interleaved columns j = point * q + a of A / W [Mp, B q] (q = pd + 1) are cut into GROUPS of G = max(1, 96 / q) whole points:
// a strip of Tc = G q <= 96 columns, Tcp = Tc rounded up to 16, Tcp / 16 column TILES.  The Gram of a strip is wanted on the q x q
// diagonal block of every point alone, so of the lower-triangular tile pairs (ti, tj <= ti) only those that meet such a block are
// computed: ti == tj, or one point owns both the last column of tile tj and the first column of tile ti (a point's columns are
// contiguous, so a point that reaches into both tiles owns both).  The live pairs are numbered in the order (ti, tj) row by row; wave w
// of the four owns the pairs w, w + 4, ...: at most 6 each (all 21 pairs live at q >= 81).  The Mp rows are cut into SLICES of `rps`
// rows (a multiple of the 32-row chunk) -- as many as give about 1024 workgroups, at least 128 rows each, at most 32 -- by a rule of
// the shapes alone: the order of every sum, and so every bit of the result, is the same on every card.
#pragma once

#if defined(__HIPCC__)
#define PRED_BLOCKS_FN __host__ __device__ __forceinline__
#else
#define PRED_BLOCKS_FN inline
#endif

constexpr int PB_TMAX = 96;         // strip columns at most (the tile rule of assemble_wide.hip)
constexpr int PB_KC = 32;           // rows per staged chunk
constexpr int PB_MAXPAIRS = 6;      // live tile pairs per wave at most: ceil(21 / 4)
constexpr int PB_NT = 256;          // threads per workgroup (4 waves)

struct PredBlocksPlan {
    int q, G, Tc, Tcp, ntile, ld;   // ld: LDS row stride of a chunk image, = 16 mod 32 (the k = lane >> 4 rows of one read fall on disjoint banks)
    int ngroups, nslices, rps;
    long long ncols;                // B q
};

// 0, or -1 for arguments the kernel does not take
PRED_BLOCKS_FN int pred_blocks_plan(int Mp, int B, int pd, PredBlocksPlan& w) {
    if (Mp < 1 || B < 1 || pd < 0 || pd > PB_TMAX - 1) return -1;
    w.q = pd + 1;
    w.ncols = (long long)B * w.q;
    if (w.ncols > 0x7fffffffLL) return -1;
    w.G = PB_TMAX / w.q;
    w.Tc = w.G * w.q;
    w.Tcp = (w.Tc + 15) & ~15;
    w.ntile = w.Tcp >> 4;
    w.ld = (w.Tcp & 31) == 16 ? w.Tcp : w.Tcp + 16;
    w.ngroups = (B + w.G - 1) / w.G;
    int ns = (1024 + w.ngroups - 1) / w.ngroups;
    const int cap = (Mp + 127) / 128;
    ns = ns < cap ? ns : cap;
    ns = ns < 32 ? ns : 32;
    ns = ns > 1 ? ns : 1;
    w.rps = (((Mp + ns - 1) / ns) + PB_KC - 1) / PB_KC * PB_KC;
    w.nslices = (Mp + w.rps - 1) / w.rps;
    return 0;
}

// is the tile pair (ti, tj <= ti) of a strip live (does it meet a point's diagonal block)?
PRED_BLOCKS_FN bool pred_blocks_pair_live(int ti, int tj, int q, int Tc) {
    if (ti * 16 >= Tc) return false;                        // (padding tiles do not exist: Tcp - Tc < 16)
    return ti == tj || (tj * 16 + 15) / q == (ti * 16) / q;
}

// the idx-th live pair of the strip, in the order (ti, tj) row by row: false when there are not that many
PRED_BLOCKS_FN bool pred_blocks_pair(int idx, int ntile, int q, int Tc, int& ti, int& tj) {
    int n = 0;
    for (int i = 0; i < ntile; ++i)
        for (int j = 0; j <= i; ++j)
            if (pred_blocks_pair_live(i, j, q, Tc)) {
                if (n == idx) { ti = i; tj = j; return true; }
                ++n;
            }
    return false;
}

// accumulator element (row i, column j of the strip's Gram) -> its place in the lower part of a point's block: false when it is none
// (another point's column, the strict upper part, or past the `cols` live columns of a ragged last group)
PRED_BLOCKS_FN bool pred_blocks_element(int i, int j, int q, int cols, int& pt, int& a, int& b) {
    if (i >= cols || j > i) return false;
    pt = i / q;
    if (j < pt * q) return false;
    a = i - pt * q;
    b = j - pt * q;
    return true;
}
