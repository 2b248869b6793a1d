// Team, group and LDS arithmetic of the per-point covariance roots (block_roots.hip).  Plain arithmetic on integers, shared between the
// three kernels, their launchers and the host check tools/block_roots_check.cpp (which shows, for every q in 1..96 at a ragged B,
// that every element of every block is owned exactly once and that every LDS and global offset stays in bounds).
//
// A block of q x q (q = pd + 1 <= 96) is the work of one TEAM of T lanes, T = 8 / 16 / 32 / 64 the smallest of these that is >= q
// (64 above 32).  Team lane t owns the rows t and t + T of its block (the second one only at q > 64): a row's arithmetic is one lane's
// serial loop, whatever else the workgroup holds.  A workgroup is 256 threads = 256 / T teams at T < 64 and ONE wave = one team at
// T = 64 (two such workgroups fit a CU's LDS at q = 96).  The block lives in LDS as [q][q + 1] doubles: the odd row stride puts the
// rows of one column on disjoint 8-byte bank pairs, and the pad column j = q carries the per-row scalars (the diagonal of the root, the
// entries of z).  The rule depends on q alone: block b's bits do not depend on B, on its neighbours or on the card.
#pragma once

#if defined(__HIPCC__)
#define BLOCK_ROOTS_FN __host__ __device__ __forceinline__
#else
#define BLOCK_ROOTS_FN inline
#endif

constexpr int BR_QMAX = 96;         // q = pd + 1 at most
constexpr int BR_ROWS = 2;          // rows per team lane at most: ceil(96 / 64)

struct BlockRootsPlan {
    int q, T, G, nthreads;          // lanes per team, teams (= blocks) per workgroup, threads per workgroup
    int ld, img;                    // LDS row stride (q + 1) and doubles per block image (q ld)
    int ngroups;                    // workgroups: ceil(B / G)
    unsigned lds_bytes;             // dynamic LDS per workgroup: G img doubles
};

BLOCK_ROOTS_FN int block_roots_team(int q) { return q <= 8 ? 8 : q <= 16 ? 16 : q <= 32 ? 32 : 64; }

// 0, or -1 for arguments the kernels do not take (B >= 1 here: the entries answer B == 0 themselves)
BLOCK_ROOTS_FN int block_roots_plan(int B, int q, BlockRootsPlan& w) {
    if (B < 1 || q < 1 || q > BR_QMAX) return -1;
    w.q = q;
    w.T = block_roots_team(q);
    w.nthreads = w.T == 64 ? 64 : 256;
    w.G = w.nthreads / w.T;
    w.ld = q + 1;
    w.img = q * w.ld;
    w.ngroups = (B + w.G - 1) / w.G;
    w.lds_bytes = (unsigned)(sizeof(double) * (size_t)w.G * w.img);
    return 0;
}

// thread -> (team of its workgroup, lane of its team); workgroup `group`, team -> block (>= B: the team idles)
BLOCK_ROOTS_FN int block_roots_team_of(int tid, int T) { return tid / T; }
BLOCK_ROOTS_FN int block_roots_lane_of(int tid, int T) { return tid % T; }
BLOCK_ROOTS_FN long long block_roots_block(int group, int G, int team) { return (long long)group * G + team; }
// element (i, j <= q) of a team's image, in doubles from the start of the workgroup's LDS
BLOCK_ROOTS_FN int block_roots_lds(int team, int img, int ld, int i, int j) { return team * img + i * ld + j; }
