// One C entry point for the whole ELBO step of the FLOAT64 model mode (the reference's experiment scripts run under
// torch.set_default_dtype(torch.float64), experiments/synthetic/exp_script.py:56).
//
// dsvgp_elbo_step_f64 queues forward + backward of one DSVGP minibatch ELBO evaluation -- train_gp's iteration body
// (directionalvi/directional_vi.py:245-249) with the composition of DirectionalGradVariationalStrategy.forward (DGVS.py:89-208),
// every array in double -- from ONE host call: no host read, no host synchronisation, no device allocation, every intermediate in
// one caller-owned workspace, the factorisation's status word through pinned memory.  It is the sequence that
// `_step64.ElboEngine64._elbo_fast64` issues through ~40 ctypes calls and ~60 eager torch operations; the products, the
// factorisation, the two assembly paths and the scalar tail are the library's own entry points, and the elementwise passes that
// torch ran between them are the kernels of this file:
//   prologue64_kernel      column mean of Z, the three softplus constraints, the packed rows of (Z, V) and of (x, D): one launch
//   gemv64t_acc_kernel     mu0 += A^T m onto the step's cleared head (no fill launch of its own)
// (deterministic mode, dsvgp_set_deterministic: one stream, and every sum that meets in fp64 atomics by default -- mu0, tvar, the KL
// sum, the scalar tail, the kernel backwards' d_hyp and dP1, the split-K products -- goes through the caller's scratch in a fixed order)
//   gram_epilogue64_kernel tril(G) -> symmetric G in one pass, tr G on the way
//   variational64_kernel   one pass over the lower triangle of (L_S, H = tril(G L_S)): tr(L_S^T G L_S), the KL value, L_S-bar
//   bvec64_kernel          b = A mu_bar into the extra row of [G ; b^T], m-bar = b + KL gradient
//   sminus64_kernel        tril(S) -> [2 vbar (S - I) | m] in place (mirror, identity, scaling, the m column): one pass
//   epilogue64_kernel      softplus slopes, raw-parameter gradients, the constant's gradient, the loss
//
// Scope: the Gram formulation of the ELBO, Cholesky variational distribution, Cholesky whitening, every data point with its p
// directional derivatives, one rank, explicit-inverse regime (M' <= 8192), any d, 0 <= p <= 95.  Everything else (PLL, per-output
// variances, CIQ, shared directions, derivative-free data, the jitter ladder after a failed factorisation) stays on the
// Python-orchestrated path.
#include "common.h"
#include "pack64.h"

#include <string.h>

#include <new>

namespace {

struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) / 256 * 256;
        return o;
    }
};

inline int auto_nb(int Mp) {          // _step.ElboEngine._problem_size: the explicit-inverse regime up to M' = 8192
    int b = 64;
    while (b < Mp) b <<= 1;
    return b;
}

constexpr int F64_REGISTER_P = 16;    // directions per point that assemble64.hip's transform kernels hold in registers
constexpr int F64_MAX_P = 95;         // ... that the tiled kernels (assemble64_tiled.hip) and the pack / points kernels take
constexpr int WIDE_DP = 96;           // packed width above which a workgroup of the prologue no longer forms all d column means itself

__device__ __forceinline__ double softplus64(double v) { return v > 20.0 ? v : log1p(exp(v)); }     // F.softplus (threshold 20)

// The step's first launch: every workgroup forms the centre (column means of Z: one wave per column, lanes over the rows, the lanes
// added in a fixed order -- the same in every workgroup) and the lengthscale for itself, workgroup 0 publishes centre and
// hyp[4] = {lengthscale, outputscale, noise, 0} (gpytorch Positive / GreaterThan(1e-4) constraints), and each packs 256 rows of
// (Z, V) (workgroups < nbz) or of (x, D).
__global__ __launch_bounds__(256) void prologue64_kernel(const double* __restrict__ Z, const double* __restrict__ V, int M,
                                                         const double* __restrict__ X, const double* __restrict__ Dm, int B, int d, int p,
                                                         const double* rl, const double* rs, const double* rn, double* __restrict__ hyp,
                                                         double* __restrict__ center, double* __restrict__ PZ, double* __restrict__ sZ,
                                                         double* __restrict__ vZ, double* __restrict__ PX, double* __restrict__ sX,
                                                         double* __restrict__ vX, int K4, int DP, int nbz) {
    extern __shared__ double cs64[];        // [d] centre, then ell
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    for (int k = wave; k < d; k += 4) {
        double acc = 0.0;
        for (int i = lane; i < M; i += 64) acc += Z[(int64_t)i * d + k];
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
        if (lane == 0) cs64[k] = acc / (double)M;
    }
    if (t == 0) {
        const double ell = softplus64(rl[0]);
        cs64[d] = ell;
        if (blockIdx.x == 0) { hyp[0] = ell; hyp[1] = softplus64(rs[0]); hyp[2] = softplus64(rn[0]) + 1e-4; hyp[3] = 0.0; }
    }
    __syncthreads();
    if (blockIdx.x == 0)
        for (int k = t; k < d; k += 256) center[k] = cs64[k];
    const int q = p + 1;
    if ((int)blockIdx.x < nbz) {
        const int row = blockIdx.x * 256 + t;
        if (row < M * q) pack64_row(Z, V, row, d, p, cs64[d], cs64, PZ, sZ, vZ, K4, DP);
    } else {
        const int row = ((int)blockIdx.x - nbz) * 256 + t;
        if (row < B * q) pack64_row(X, Dm, row, d, p, cs64[d], cs64, PX, sX, vX, K4, DP);
    }
}

// wide inputs: centre (one workgroup per column) and hyp; the two point sets are then packed by dsvgp_pack_points_f64
__global__ __launch_bounds__(256) void colmean_hyp64_kernel(const double* __restrict__ Z, int M, int d, double* __restrict__ center,
                                                            const double* rl, const double* rs, const double* rn, double* __restrict__ hyp) {
    __shared__ double part[4];
    const int k = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    for (int i = threadIdx.x; i < M; i += 256) acc += Z[(int64_t)i * d + k];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        center[k] = (part[0] + part[1] + part[2] + part[3]) / (double)M;
        if (k == 0) { hyp[0] = softplus64(rl[0]); hyp[1] = softplus64(rs[0]); hyp[2] = softplus64(rn[0]) + 1e-4; hyp[3] = 0.0; }
    }
}

// y[N] += A^T x on a row-major M x N matrix (y cleared by the caller: the step's head): a thread per pair of columns, the rows in
// chunks over blockIdx.y, fp64 atomics -- or (deterministic mode) plain stores to the partial rows parts[gridDim.y][N]
__global__ __launch_bounds__(256) void gemv64t_acc_kernel(const double* __restrict__ A, int64_t lda, int M, int N,
                                                          const double* __restrict__ x, int rows_per_chunk, double* __restrict__ y,
                                                          double* __restrict__ parts) {
    const int j = (blockIdx.x * 256 + threadIdx.x) * 2;
    if (j >= N) return;
    const int i0 = blockIdx.y * rows_per_chunk, i1 = min(M, i0 + rows_per_chunk);
    const bool two = j + 1 < N, vec = two && (lda % 2 == 0) && (((uintptr_t)A % 16) == 0);
    double s0 = 0.0, s1 = 0.0;
    if (vec) {
#pragma unroll 4
        for (int i = i0; i < i1; ++i) {
            const double2 av = *reinterpret_cast<const double2*>(A + (int64_t)i * lda + j);
            const double xi = x[i];
            s0 = fma(av.x, xi, s0);
            s1 = fma(av.y, xi, s1);
        }
    } else {
        for (int i = i0; i < i1; ++i) {
            const double xi = x[i];
            s0 = fma(A[(int64_t)i * lda + j], xi, s0);
            if (two) s1 = fma(A[(int64_t)i * lda + j + 1], xi, s1);
        }
    }
    if (parts) {
        double* dst = parts + (int64_t)blockIdx.y * N + j;
        dst[0] = s0;
        if (two) dst[1] = s1;
        return;
    }
    atomicAdd(&y[j], s0);
    if (two) atomicAdd(&y[j + 1], s1);
}

// Gram epilogue: G[i][j] (i < j) = G[j][i] from the lower triangle the OUT_LOWER product wrote, and tvar -= tr G (the diagonal blocks
// pass their 32 diagonal entries on the way).  32 x 32 blocks through LDS, as phi_sym_kernel.  Deterministic mode: parts[diagonal block].
__global__ __launch_bounds__(256) void gram_epilogue64_kernel(double* __restrict__ G, int n, int64_t ldg, double* __restrict__ tvar,
                                                              double* __restrict__ parts) {
    __shared__ double tile[32][33];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;                       // upper block (bi, bj), bj >= bi, from lower block (bj, bi)
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int r = ty; r < 32; r += 8) {
        const int gi = bj * 32 + r, gj = bi * 32 + tx;
        tile[r][tx] = (gi < n && gj < n) ? G[(int64_t)gi * ldg + gj] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int gi = bi * 32 + r, gj = bj * 32 + tx;
        if (gi < n && gj < n && gj > gi) G[(int64_t)gi * ldg + gj] = tile[tx][r];
    }
    if (bi == bj && tx == 0 && ty == 0) {
        double tr = 0.0;
        for (int k = 0; k < 32; ++k) tr += tile[k][k];          // (rows past n were staged as zero)
        if (parts) parts[bi] = -tr;
        else atomicAdd(tvar, -tr);
    }
}

// The variational block in one pass over the lower triangle (the fp64 form of ls_rows_kernel and its reduce): one wave per row i,
//   tvar  += sum_{j <= i} L_S,ij H_ij                   (tr(L_S^T G L_S); the Gram epilogue has subtracted tr G)
//   klsum += m_i^2 + sum_{j <= i} L_S,ij^2 - log(L_S,ii^2)              (with the KL term: KL = (klsum - M') / 2)
//   dLS_ij = 2 vbar H_ij [+ (L_S,ij - [i == j] / L_S,ii) / num_data]   for j <= i; the strict upper triangle is not touched
// 2 vbar = 1 / (noise rows): the expression dsvgp_elbo_fast_tail_f64 evaluates for scal[5], from the same hyp[2].
// Deterministic mode: the two row sums go to parts[i][2] (tvar and klsum are neighbours in the head: one fixed-order pass adds both).
__global__ __launch_bounds__(256) void variational64_kernel(const double* __restrict__ m, const double* __restrict__ LS, int64_t ldls,
                                                            const double* __restrict__ H, int64_t ldh, int Mp, double inv_nd, int add_kl,
                                                            const double* __restrict__ hyp, double inv_rows, double* __restrict__ tvar,
                                                            double* __restrict__ klsum, double* __restrict__ dLS, int64_t lddls,
                                                            double* __restrict__ parts) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= Mp) return;
    const double two_vbar = 2.0 * (0.5 * inv_rows / hyp[2]);
    const double* l = LS + (int64_t)i * ldls;
    const double* h = H + (int64_t)i * ldh;
    double* g = dLS + (int64_t)i * lddls;
    const double lii = l[i];
    double at = 0.0, al = 0.0;
    for (int j = lane; j <= i; j += 64) {
        const double lv = l[j], hv = h[j];
        at = fma(lv, hv, at);
        al = fma(lv, lv, al);
        double gv = two_vbar * hv;
        if (add_kl) gv += (lv - (j == i ? 1.0 / lii : 0.0)) * inv_nd;
        g[j] = gv;
    }
    for (int off = 32; off > 0; off >>= 1) { at += __shfl_down(at, off); al += __shfl_down(al, off); }
    if (lane == 0) {
        const double kv = add_kl ? al + m[i] * m[i] - log(lii * lii) : 0.0;
        if (parts) {
            parts[2 * i] = at;
            parts[2 * i + 1] = kv;
        } else {
            atomicAdd(tvar, at);
            if (add_kl) atomicAdd(klsum, kv);
        }
    }
}

// b = A mu_bar (one wave per row, 16-byte loads): into the extra row of [G ; b^T], and m-bar = b [+ m / num_data] into the (cleared) dm
__global__ __launch_bounds__(256) void bvec64_kernel(const double* __restrict__ A, int64_t lda, int M, int N, const double* __restrict__ x,
                                                     const double* __restrict__ m, double kl_scale, double* __restrict__ b,
                                                     double* __restrict__ dm) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const double* a = A + (int64_t)row * lda;
    double s = 0.0;
    const bool vec = (lda % 2 == 0) && (((uintptr_t)A % 16) == 0) && (((uintptr_t)x % 16) == 0);
    if (vec) {
        const int n2 = N / 2;
        for (int j = lane; j < n2; j += 64) {
            const double2 av = *reinterpret_cast<const double2*>(a + 2 * j);
            const double2 xv = *reinterpret_cast<const double2*>(x + 2 * j);
            s = fma(av.x, xv.x, s);
            s = fma(av.y, xv.y, s);
        }
        if ((N & 1) && lane == 0) s = fma(a[N - 1], x[N - 1], s);
    } else {
        for (int j = lane; j < N; j += 64) s = fma(a[j], x[j], s);
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (lane == 0) {
        b[row] = s;
        dm[row] = s + kl_scale * m[row];
    }
}

// tril(S) (what the OUT_LOWER product S = L_S L_S^T wrote) -> Se = [2 vbar (S - I) | m] in place, n x (n + 1) with leading dimension
// lds: the lower blocks are scaled where they lie, their transposes fill the upper blocks, the diagonal loses the identity, column n
// receives m.  It is the one operand both later products read: [2 vbar Q' | a]^T = Se^T L^-1 (L^-T is linear: scaling S - I before
// the solve is scaling Q' after it) and tril(L^T L-bar) = -tril(Se [G ; b^T]).
__global__ __launch_bounds__(256) void sminus64_kernel(double* __restrict__ S, int n, int64_t lds, const double* __restrict__ m,
                                                       const double* __restrict__ hyp, double inv_rows) {
    __shared__ double tile[32][33];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;                       // lower block (bj, bi) and its mirror (bi, bj)
    const int tx = threadIdx.x, ty = threadIdx.y;
    const double c = 2.0 * (0.5 * inv_rows / hyp[2]);
    for (int r = ty; r < 32; r += 8) {
        const int gi = bj * 32 + r, gj = bi * 32 + tx;
        tile[r][tx] = (gi < n && gj < n && gj <= gi) ? S[(int64_t)gi * lds + gj] - (gi == gj ? 1.0 : 0.0) : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int gi = bj * 32 + r, gj = bi * 32 + tx;          // the lower block, in place
        if (gi < n && gj < n && gj <= gi) S[(int64_t)gi * lds + gj] = c * tile[r][tx];
        const int ui = bi * 32 + r, uj = bj * 32 + tx;          // its mirror
        if (ui < n && uj < n && uj > ui) S[(int64_t)ui * lds + uj] = c * tile[tx][r];
    }
    if (bi == bj && ty == 0) {
        const int gi = bi * 32 + tx;
        if (gi < n) S[(int64_t)gi * lds + n] = m[gi];
    }
}

// scalar tail: softplus slopes (Positive: d raw = d * sigmoid(raw); GreaterThan(1e-4): the same slope), the likelihood / prior-diagonal
// parts of scal (dsvgp_elbo_fast_tail_f64) + the kernel parts d_hyp, the constant's gradient, loss = -sum ll / rows + KL / num_data
__global__ void epilogue64_kernel(const double* __restrict__ scal, const double* __restrict__ klsum, int Mp, int add_kl, double inv_rows,
                                  double inv_nd, const double* rl, const double* rs, const double* rn, const double* __restrict__ d_hyp,
                                  double* drl, double* drs, double* drn, double* dconst, double* loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    auto sg = [](double v) { return 1.0 / (1.0 + exp(-v)); };
    drl[0] = (scal[4] + d_hyp[0]) * sg(rl[0]);
    drs[0] = (scal[3] + d_hyp[1]) * sg(rs[0]);
    drn[0] = scal[1] * sg(rn[0]);
    dconst[0] = scal[2];
    double l = -scal[0] * inv_rows;
    if (add_kl) l += 0.5 * (klsum[0] - (double)Mp) * inv_nd;
    loss[0] = l;
}

__global__ void gather64_kernel(const double* __restrict__ X, const double* __restrict__ Y, const int64_t* __restrict__ idx, int nb, int d,
                                int ycols, const int* __restrict__ cols, int p, double* __restrict__ xb, double* __restrict__ yb,
                                const double* __restrict__ E, double* __restrict__ Db) {
    const int b = blockIdx.x;
    const int64_t src = idx[b];
    for (int k = threadIdx.x; k < d; k += blockDim.x) xb[(int64_t)b * d + k] = X[src * d + k];
    for (int c = threadIdx.x; c <= p; c += blockDim.x) yb[(int64_t)b * (p + 1) + c] = Y[src * ycols + cols[c]];
    if (E)      // the batch's derivative directions: row a of point b = row cols[a + 1] - 1 of E (directional_vi.py:238)
        for (int e = threadIdx.x; e < p * d; e += blockDim.x) {
            const int a = e / d, k = e - a * d;
            Db[((int64_t)b * p + a) * d + k] = E[(int64_t)(cols[a + 1] - 1) * d + k];
        }
}

}  // namespace

struct dsvgp_step_plan_f64 {
    int M, d, p, B, Mp, Bp, DP, K4, nb, ldS;
    size_t bytes;
    // workspace offsets (bytes)
    size_t o_center, o_PZ, o_sZ, o_vZ, o_PX, o_sX, o_vX, o_L, o_potrf, o_trsm, o_Kzx, o_bwd;
    // the arena: every target of a product that may split K or leaves part of its output to a fill (OUT_LOWER), each written by ONE
    // product per step, and the head -- contiguous, so that a small problem clears all of it with one memset
    size_t o_arena, arena_bytes;
    size_t o_Se, o_Ae, o_Ge, o_H, o_QeT, o_Kb, o_G1, o_Yt, o_Kbar, o_dPzx, o_dPzz;
    size_t o_head, head_bytes;        // hyp[4] | info | tvar | klsum | scal[8] | mu0[B']  (cleared every step)
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_side = nullptr, ev_fork2 = nullptr, ev_status = nullptr;
    static constexpr int TM_RING = 128, TM_PAIRS = 5;
    hipEvent_t tm_ring[TM_RING][2 * TM_PAIRS] = {};
    long timed_steps = 0;
    double* host_status = nullptr;    // pinned: hyp[4] + info (the int in the first four bytes of the fifth slot)
};

// workspace layout of one (M, d, p, B); returns the total byte count (0: the call does not take the shape)
static size_t step64_layout(int M, int d, int p, int B, dsvgp_step_plan_f64* pl) {
    if (M <= 0 || d <= 0 || p < 0 || p > F64_MAX_P || B <= 0 || d > (1 << 24)) return 0;
    const int64_t q = p + 1;
    if (M * q > 8192 || B * q > INT32_MAX || M * q * B * q >= ((int64_t)1 << 31)) return 0;
    const int Mp = (int)(M * q), Bp = (int)(B * q), K4 = (d + 3) & ~3, DP = K4 + 4;
    if ((int64_t)Bp * DP >= ((int64_t)1 << 31)) return 0;
    pl->M = M; pl->d = d; pl->p = p; pl->B = B; pl->Mp = Mp; pl->Bp = Bp; pl->K4 = K4; pl->DP = DP; pl->nb = auto_nb(Mp);
    pl->ldS = (Mp + 2) / 2 * 2;
    const size_t D8 = sizeof(double);
    Carve c;
    pl->o_center = c.take((size_t)d * D8);
    pl->o_PZ = c.take((size_t)Mp * DP * D8); pl->o_sZ = c.take((size_t)Mp * D8); pl->o_vZ = c.take((size_t)(M * p > 0 ? M * p : 1) * D8);
    pl->o_PX = c.take((size_t)Bp * DP * D8); pl->o_sX = c.take((size_t)Bp * D8); pl->o_vX = c.take((size_t)(B * p > 0 ? B * p : 1) * D8);
    pl->o_L = c.take((size_t)Mp * Mp * D8);
    pl->o_potrf = c.take(potrf_blocked_workspace_bytes(Mp));
    pl->o_trsm = c.take(dsvgp_trsm_workspace_bytes(Mp, Bp > Mp + 1 ? Bp : Mp + 1, pl->nb));
    // K_ZX is dead after the forward solve: its place serves the register assembly's T scratch of the K_ZX-bar backward (p <= 16)
    pl->o_Kzx = c.take((size_t)Mp * Bp * D8);
    pl->o_bwd = 0;
    pl->o_arena = c.off;
    pl->o_Se = c.take((size_t)Mp * pl->ldS * D8);
    pl->o_Ae = c.take((size_t)(Mp + 1) * Bp * D8);
    pl->o_Ge = c.take((size_t)(Mp + 1) * Mp * D8);
    pl->o_H = c.take((size_t)Mp * Mp * D8);             // tril(G L_S); later the T scratch of the K_ZZ-bar backward (p <= 16)
    pl->o_QeT = c.take((size_t)(Mp + 1) * Mp * D8);
    pl->o_Kb = c.take((size_t)Mp * Bp * D8);
    pl->o_G1 = c.take((size_t)Mp * Mp * D8); pl->o_Yt = c.take((size_t)Mp * Mp * D8); pl->o_Kbar = c.take((size_t)Mp * Mp * D8);
    pl->o_dPzx = c.take((size_t)Mp * DP * D8); pl->o_dPzz = c.take((size_t)Mp * DP * D8);
    pl->o_head = c.off;
    pl->head_bytes = ((size_t)(4 + 1 + 1 + 1 + 8 + Bp) * D8 + 255) / 256 * 256;
    c.take(pl->head_bytes);
    pl->arena_bytes = c.off - pl->o_arena;
    pl->bytes = c.off + 256;
    return pl->bytes;
}

extern "C" int dsvgp_elbo_step_f64_supported(int M, int d, int p, int B) {
    dsvgp_step_plan_f64 pl{};
    return step64_layout(M, d, p, B, &pl) ? 1 : 0;
}
extern "C" size_t dsvgp_elbo_step_f64_workspace_bytes(int M, int d, int p, int B) {
    dsvgp_step_plan_f64 pl{};
    return step64_layout(M, d, p, B, &pl);
}

static void plan64_release(dsvgp_step_plan_f64* pl) {
    hipEvent_t evs[] = {pl->ev_fork, pl->ev_side, pl->ev_fork2, pl->ev_status};
    for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
    for (auto& slot : pl->tm_ring) for (hipEvent_t e : slot) if (e) (void)hipEventDestroy(e);
    if (pl->side) (void)hipStreamDestroy(pl->side);
    if (pl->host_status) (void)hipHostFree(pl->host_status);
    delete pl;
}

extern "C" int dsvgp_elbo_step_f64_plan_create(dsvgp_ctx* ctx, int M, int d, int p, int B, dsvgp_step_plan_f64** out) {
    if (!ctx || !out) return DSVGP_EINVAL;
    dsvgp_step_plan_f64* pl = new (std::nothrow) dsvgp_step_plan_f64();
    if (!pl) return DSVGP_EINVAL;
    if (!step64_layout(M, d, p, B, pl)) { delete pl; return DSVGP_EINVAL; }
    bool ok = hipStreamCreateWithFlags(&pl->side, hipStreamNonBlocking) == hipSuccess;
    hipEvent_t* evs[] = {&pl->ev_fork, &pl->ev_side, &pl->ev_fork2, &pl->ev_status};
    for (hipEvent_t* e : evs) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    for (auto& slot : pl->tm_ring) for (hipEvent_t& e : slot) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&pl->host_status, 5 * sizeof(double), hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        plan64_release(pl);
        return 1000 + (int)hipErrorOutOfMemory;
    }
    memset(pl->host_status, 0, 5 * sizeof(double));
    *out = pl;
    return 0;
}
extern "C" int dsvgp_elbo_step_f64_plan_destroy(dsvgp_step_plan_f64* pl) {
    if (!pl) return DSVGP_EINVAL;
    plan64_release(pl);
    return 0;
}

extern "C" long dsvgp_elbo_step_f64_timed_count(const dsvgp_step_plan_f64* pl) { return pl ? pl->timed_steps : 0; }

extern "C" int dsvgp_elbo_step_f64_timings(dsvgp_step_plan_f64* pl, int back, float* ms5) {
    if (!pl || !ms5 || back < 0 || back >= dsvgp_step_plan_f64::TM_RING || back >= pl->timed_steps) return DSVGP_EINVAL;
    hipEvent_t* tm = pl->tm_ring[(pl->timed_steps - 1 - back) % dsvgp_step_plan_f64::TM_RING];
    for (int k = 0; k < dsvgp_step_plan_f64::TM_PAIRS; ++k) {
        hipError_t e = hipEventSynchronize(tm[2 * k + 1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms5[k], tm[2 * k], tm[2 * k + 1]);
        if (e != hipSuccess) return 1000 + (int)e;
    }
    return 0;
}

// Wait for the factorisation of the step queued last (NOT for the rest of the step): its status word (0 = positive definite) and the
// constrained hyper-parameters {lengthscale, outputscale, noise, 0} of that step
extern "C" int dsvgp_elbo_step_f64_status(dsvgp_step_plan_f64* pl, double* hyp4, int* info) {
    if (!pl || !info) return DSVGP_EINVAL;
    hipError_t e = hipEventSynchronize(pl->ev_status);
    if (e != hipSuccess) return 1000 + (int)e;
    if (hyp4) for (int i = 0; i < 4; ++i) hyp4[i] = pl->host_status[i];
    int v;
    memcpy(&v, &pl->host_status[4], sizeof(int));
    *info = v;
    return 0;
}

#define S64_CALL(expr)                  \
    do {                                \
        const int rc__ = (expr);        \
        if (rc__) { ctx->stream = main; return rc__; } \
    } while (0)
#define S64_HIP(expr)                   \
    do {                                \
        const hipError_t e__ = (expr);  \
        if (e__ != hipSuccess) { ctx->stream = main; return 1000 + (int)e__; } \
    } while (0)
#define S64_LAUNCHED() S64_HIP(hipGetLastError())

namespace {
struct Zeroed64 {                             // ctx->prezeroed around ONE call whose target lies, untouched so far, in the cleared arena
    dsvgp_ctx* c; bool prev;
    Zeroed64(dsvgp_ctx* c_, bool on) : c(c_), prev(c_->prezeroed) { c->prezeroed = on; }
    ~Zeroed64() { c->prezeroed = prev; }
};
inline int gemm64(dsvgp_ctx* ctx, int flags, int M, int N, int K, double alpha, const double* A, int64_t lda, const double* B, int64_t ldb,
                  double* C, int64_t ldc) {
    return dsvgp_gemm(ctx, 1, flags, M, N, K, alpha, A, lda, B, ldb, 0.0, nullptr, 0, C, ldc, nullptr, 0, nullptr);
}
// outputscale * K(x1, x2; v1, v2) [+ jitter I]: the dispatch of _ops.kernel_fwd_f64
int fwd64(dsvgp_ctx* ctx, const dsvgp_step_plan_f64* pl, const double* P1, const double* s1, int n1, const double* P2, const double* s2,
          int n2, const double* hyp, double jitter, double* out, int64_t ld) {
    const int p = pl->p, q = p + 1;
    if (p > F64_REGISTER_P) return dsvgp_kernel_fwd_f64(ctx, P1, s1, n1, P2, s2, n2, pl->d, p, hyp, jitter, jitter != 0.0 ? 1 : 0, out, ld);
    const int rc = gemm64(ctx, DSVGP_GEMM_TRANS_B, n1 * q, n2 * q, pl->K4, 1.0, P1, pl->DP, P2, pl->DP, out, ld);
    if (rc) return rc;
    return dsvgp_kernel_transform_f64(ctx, out, ld, s1, n1, s2, n2, p, hyp, jitter);
}
// its backward: the dispatch of _ops.kernel_bwd_f64 (T: [n1 q, n2 q] scratch of the register path; dP: [n1 q, DP], cleared, in the arena)
int bwd64(dsvgp_ctx* ctx, const dsvgp_step_plan_f64* pl, bool prezero, const double* G, int64_t ldg, const double* P1, const double* s1,
          const double* v1, int n1, const double* P2, const double* s2, int n2, const double* hyp, int symmetric, double* dx, double* dv,
          double* d_hyp, double* T, double* dP) {
    const int p = pl->p, q = p + 1, d = pl->d, DP = pl->DP;
    if (p > F64_REGISTER_P)
        return dsvgp_kernel_bwd_f64(ctx, G, ldg, P1, s1, v1, n1, P2, s2, n2, d, p, hyp, symmetric, dx, dv, d_hyp, dP,
                                    (size_t)n1 * q * DP * sizeof(double));
    const int64_t ldt = (int64_t)n2 * q;
    int rc = gemm64(ctx, DSVGP_GEMM_TRANS_B, n1 * q, n2 * q, pl->K4, 1.0, P1, DP, P2, DP, T, ldt);
    if (rc) return rc;
    rc = dsvgp_kernel_bwd_transform_f64(ctx, G, ldg, T, ldt, s1, n1, s2, n2, p, hyp, d_hyp);
    if (rc) return rc;
    {
        Zeroed64 z(ctx, prezero);
        rc = gemm64(ctx, 0, n1 * q, DP, n2 * q, 1.0, T, ldt, P2, DP, dP, DP);              // Tbar [P2 | indicator]
    }
    if (rc) return rc;
    return dsvgp_kernel_bwd_points_f64(ctx, dP, P1, v1, n1, d, p, hyp, symmetric, dx, dv);
}
}  // namespace

extern "C" int dsvgp_elbo_step_f64(dsvgp_ctx* ctx, dsvgp_step_plan_f64* pl, const dsvgp_elbo_step_io_f64* io, void* workspace,
                                   size_t workspace_bytes, int flags) {
    if (!ctx || !pl || !io || !workspace || workspace_bytes < pl->bytes || ((uintptr_t)workspace % 256)) return DSVGP_EINVAL;
    // versioned struct: the fields of this version end at kzz_jitter; a larger struct_size is a newer caller whose extra fields this
    // library does not know (and ignores), a smaller one cannot hold the fields read below
    if (io->struct_size < offsetof(dsvgp_elbo_step_io_f64, kzz_jitter) + sizeof(double)) return DSVGP_EINVAL;
    if (!io->Z || !io->m || !io->LS || !io->constant || !io->raw_lengthscale || !io->raw_outputscale || !io->raw_noise || !io->x ||
        !io->y || !io->flat || !io->dZ || !io->dm || !io->dLS || !io->d_hyp || !io->d_constant || !io->d_raw_lengthscale ||
        !io->d_raw_outputscale || !io->d_raw_noise || !io->loss || !io->mu || !(io->num_data > 0) || !(io->global_rows > 0) ||
        !(io->kzz_jitter >= 0))
        return DSVGP_EINVAL;
    const int M = pl->M, d = pl->d, p = pl->p, B = pl->B, Mp = pl->Mp, Bp = pl->Bp, DP = pl->DP, K4 = pl->K4, nb = pl->nb, ldS = pl->ldS;
    if (p > 0 && (!io->V || !io->D || !io->dV)) return DSVGP_EINVAL;
    if (io->ldls < Mp || io->lddls < Mp) return DSVGP_EINVAL;
    char* w = (char*)workspace;
    double* center = (double*)(w + pl->o_center);
    double *PZ = (double*)(w + pl->o_PZ), *sZ = (double*)(w + pl->o_sZ), *vZ = (double*)(w + pl->o_vZ);
    double *PX = (double*)(w + pl->o_PX), *sX = (double*)(w + pl->o_sX), *vX = (double*)(w + pl->o_vX);
    double* L = (double*)(w + pl->o_L);
    void* potrf_ws = w + pl->o_potrf;
    void* trsm_ws = w + pl->o_trsm;
    const double* Linv = (const double*)trsm_ws;        // (dsvgp_potrf_inverse: L^-1, then its transpose)
    double* Kzx = (double*)(w + pl->o_Kzx);
    double* Se = (double*)(w + pl->o_Se);
    double* Ae = (double*)(w + pl->o_Ae);
    double* A = Ae;
    double* mu_bar = Ae + (size_t)Mp * Bp;
    double* Ge = (double*)(w + pl->o_Ge);
    double* bvec = Ge + (size_t)Mp * Mp;
    double* H = (double*)(w + pl->o_H);
    double* QeT = (double*)(w + pl->o_QeT);
    double* Kb = (double*)(w + pl->o_Kb);
    double *G1 = (double*)(w + pl->o_G1), *Yt = (double*)(w + pl->o_Yt), *Kbar = (double*)(w + pl->o_Kbar);
    double *dPzx = (double*)(w + pl->o_dPzx), *dPzz = (double*)(w + pl->o_dPzz);
    double* hyp = (double*)(w + pl->o_head);
    int* info = (int*)(hyp + 4);
    double *tvar = hyp + 5, *klsum = hyp + 6, *scal = hyp + 7, *mu0 = hyp + 15;
    const double rows = io->global_rows, inv_rows = 1.0 / rows, inv_nd = 1.0 / io->num_data;
    // deterministic mode (dsvgp_set_deterministic): the scratch serves one stream at a time, so flag 1 is ignored -- the whole step is
    // queued on the context's stream; every launcher below then adds its partial sums in a fixed order
    double* const det = (double*)ctx->det_slab;
    const size_t det_doubles = ctx->det_bytes / sizeof(double);
    if (det && (((uintptr_t)det & 7) || det_doubles < (size_t)2 * Mp)) return DSVGP_EINVAL;       // (the row partials of the variational block)
    const bool overlap = (flags & 1) && !det, add_kl = flags & 2, timed = flags & 4;
    const hipStream_t main = ctx->stream, side = pl->side;
    hipEvent_t* tm = nullptr;
    if (timed) { tm = pl->tm_ring[pl->timed_steps % dsvgp_step_plan_f64::TM_RING]; ++pl->timed_steps; }
#define S64_TIME(slot) do { if (timed) S64_HIP(hipEventRecord(tm[slot], ctx->stream)); } while (0)

    // ---- clears: the gradient slots + loss, and ONE memset for everything else that must start from zero -- the head (status word,
    // tvar, KL sum, mu0) and, for small problems, the whole arena of split-K / OUT_LOWER targets (their launchers are told so and
    // queue no fill of their own between the products).  Large problems keep the launchers' own clears.
    const bool prezero = pl->arena_bytes <= ((size_t)48 << 20);
    S64_HIP(hipMemsetAsync(io->flat, 0, io->flat_doubles * sizeof(double), main));
    if (prezero) S64_HIP(hipMemsetAsync(w + pl->o_arena, 0, pl->arena_bytes, main));
    else S64_HIP(hipMemsetAsync(w + pl->o_head, 0, pl->head_bytes, main));

    // ---- prologue: centre, hyper-parameters, the packed rows of both point sets
    if (DP > WIDE_DP) {
        hipLaunchKernelGGL(colmean_hyp64_kernel, dim3(d), dim3(256), 0, main, io->Z, M, d, center, io->raw_lengthscale, io->raw_outputscale,
                           io->raw_noise, hyp);
        S64_LAUNCHED();
        S64_CALL(dsvgp_pack_points_f64(ctx, io->Z, io->V, M, d, p, hyp, center, PZ, sZ, vZ));
        S64_CALL(dsvgp_pack_points_f64(ctx, io->x, io->D, B, d, p, hyp, center, PX, sX, vX));
    } else {
        const int nbz = cdiv(Mp, 256), nbx = cdiv(Bp, 256);
        hipLaunchKernelGGL(prologue64_kernel, dim3(nbz + nbx), dim3(256), sizeof(double) * (d + 1), main, io->Z, io->V, M, io->x, io->D, B, d,
                           p, io->raw_lengthscale, io->raw_outputscale, io->raw_noise, hyp, center, PZ, sZ, vZ, PX, sX, vX, K4, DP, nbz);
        S64_LAUNCHED();
    }
    if (overlap) S64_HIP(hipEventRecord(pl->ev_fork, main));

    // ---- K_ZZ + jitter, Cholesky with the fused inverse: queued ahead of the side stream's work, so that the chain -- the step's
    // critical path -- starts as soon as the packs exist
    S64_CALL(fwd64(ctx, pl, PZ, sZ, M, PZ, sZ, M, hyp, io->kzz_jitter, L, Mp));
    {
        Zeroed64 z(ctx, prezero);                     // (the status word lies in the cleared head)
        S64_CALL(dsvgp_potrf_inverse(ctx, L, Mp, Mp, info, potrf_ws, nb, trsm_ws));
    }

    // ---- what does not depend on L -- K_ZX, S = L_S L_S^T, [2 vbar (S - I) | m] -- under the chain on the second stream (flag 1)
    if (overlap) {
        S64_HIP(hipStreamWaitEvent(side, pl->ev_fork, 0));
        ctx->stream = side;
    }
    S64_TIME(2);
    S64_CALL(fwd64(ctx, pl, PZ, sZ, M, PX, sX, B, hyp, 0.0, Kzx, Bp));
    S64_TIME(3);
    {
        Zeroed64 z(ctx, prezero);
        S64_CALL(gemm64(ctx, DSVGP_GEMM_A_LOWER | DSVGP_GEMM_TRANS_B | DSVGP_GEMM_B_UPPER | DSVGP_GEMM_OUT_LOWER, Mp, Mp, Mp, 1.0, io->LS,
                        io->ldls, io->LS, io->ldls, Se, ldS));                            // tril(L_S) tril(L_S)^T, lower triangle
    }
    {
        const int nbk = cdiv(Mp, 32);
        hipLaunchKernelGGL(sminus64_kernel, dim3(nbk, nbk), dim3(32, 8), 0, ctx->stream, Se, Mp, ldS, io->m, hyp, inv_rows);
        S64_LAUNCHED();
    }
    if (overlap) {
        S64_HIP(hipEventRecord(pl->ev_side, side));
        ctx->stream = main;
        // the status word leaves through the side stream, behind an event the main stream records after the factorisation
        S64_HIP(hipEventRecord(pl->ev_fork2, main));
        S64_HIP(hipStreamWaitEvent(side, pl->ev_fork2, 0));
        S64_HIP(hipMemcpyAsync(pl->host_status, hyp, 5 * sizeof(double), hipMemcpyDeviceToHost, side));     // hyp[4] | info: contiguous
        S64_HIP(hipEventRecord(pl->ev_status, side));
        S64_HIP(hipStreamWaitEvent(main, pl->ev_side, 0));
    } else {
        S64_HIP(hipMemcpyAsync(pl->host_status, hyp, 5 * sizeof(double), hipMemcpyDeviceToHost, main));
        S64_HIP(hipEventRecord(pl->ev_status, main));
    }

    // ---- A = L^-1 K_ZX (one product with the explicit inverse), mu0 = A^T m
    S64_TIME(0);
    {
        Zeroed64 z(ctx, prezero);
        S64_CALL(dsvgp_trsm(ctx, L, Mp, Mp, 0, Kzx, Bp, 1, Bp, A, Bp, nullptr, 0, nb, trsm_ws, 1));
    }
    S64_TIME(1);
    {
        int nch = cdiv(Mp, 64);
        if (nch > 64) nch = 64;
        double* parts = nullptr;
        if (det) {              // as many row chunks as the scratch holds partial rows for; below two, one chunk that stores mu0 itself
            const size_t fit = det_doubles / (size_t)Bp;
            if ((size_t)nch > fit) nch = fit >= 2 ? (int)fit : 1;
            parts = nch >= 2 ? det : mu0;
        }
        const int rpc = cdiv(Mp, nch);
        nch = cdiv(Mp, rpc);
        hipLaunchKernelGGL(gemv64t_acc_kernel, dim3(cdiv(Bp, 512), nch), dim3(256), 0, main, A, (int64_t)Bp, Mp, Bp, io->m, rpc, mu0, parts);
        S64_LAUNCHED();
        if (parts && parts != mu0) S64_CALL(launch_det_sum_rows64(main, parts, nch, Bp, mu0));
    }
    // ---- G = A A^T (lower triangle), mirrored with tr G on the way; H = tril(G L_S); the variational block
    S64_TIME(6);
    {
        Zeroed64 z(ctx, prezero);
        S64_CALL(gemm64(ctx, DSVGP_GEMM_TRANS_B | DSVGP_GEMM_OUT_LOWER, Mp, Mp, Bp, 1.0, A, Bp, A, Bp, Ge, Mp));
    }
    S64_TIME(7);
    {
        const int nbk = cdiv(Mp, 32);
        hipLaunchKernelGGL(gram_epilogue64_kernel, dim3(nbk, nbk), dim3(32, 8), 0, main, Ge, Mp, (int64_t)Mp, tvar, det);
        S64_LAUNCHED();
        if (det) S64_CALL(launch_det_sum_scalars64(main, det, nbk, 1, tvar));     // (before the next product takes the scratch for its slabs)
    }
    {
        Zeroed64 z(ctx, prezero);
        S64_CALL(gemm64(ctx, DSVGP_GEMM_B_LOWER | DSVGP_GEMM_OUT_LOWER, Mp, Mp, Mp, 1.0, Ge, Mp, io->LS, io->ldls, H, Mp));
    }
    hipLaunchKernelGGL(variational64_kernel, dim3(cdiv(Mp, 4)), dim3(256), 0, main, io->m, io->LS, io->ldls, H, (int64_t)Mp, Mp, inv_nd,
                       add_kl ? 1 : 0, hyp, inv_rows, tvar, klsum, io->dLS, io->lddls, det);
    S64_LAUNCHED();
    if (det) S64_CALL(launch_det_sum_scalars64(main, det, Mp, 2, tvar));          // tvar | klsum
    // ---- scalar tail (mu, mu_bar into the extra row of [A ; mu_bar^T], scal), b = A mu_bar and m-bar
    S64_CALL(dsvgp_elbo_fast_tail_f64(ctx, mu0, io->y, io->constant, Bp, B, p, hyp, tvar, rows, io->mu, mu_bar, scal));
    hipLaunchKernelGGL(bvec64_kernel, dim3(cdiv(Mp, 4)), dim3(256), 0, main, A, (int64_t)Bp, Mp, Bp, mu_bar, io->m, add_kl ? inv_nd : 0.0, bvec,
                       io->dm);
    S64_LAUNCHED();
    // ---- [2 vbar Q' | a]^T = Se^T L^-1, K_ZX-bar = [2 vbar Q' | a][A ; mu_bar^T] (the one dense [M', B'] product),
    //      tril(L^T L-bar) = -tril(Se [G ; b^T])
    {
        Zeroed64 z(ctx, prezero);
        S64_CALL(gemm64(ctx, DSVGP_GEMM_TRANS_A | DSVGP_GEMM_B_LOWER, Mp + 1, Mp, Mp, 1.0, Se, ldS, Linv, Mp, QeT, Mp));
    }
    S64_TIME(8);
    {
        Zeroed64 z(ctx, prezero);
        S64_CALL(gemm64(ctx, DSVGP_GEMM_TRANS_A, Mp, Bp, Mp + 1, 1.0, QeT, Mp, Ae, Bp, Kb, Bp));
    }
    S64_TIME(9);
    {
        Zeroed64 z(ctx, prezero);
        S64_CALL(gemm64(ctx, DSVGP_GEMM_OUT_LOWER, Mp, Mp, Mp + 1, -1.0, Se, ldS, Ge, Mp, G1, Mp));
    }
    // ---- K_ZX-bar -> Z, V, lengthscale, outputscale
    S64_TIME(4);
    S64_CALL(bwd64(ctx, pl, prezero, Kb, Bp, PZ, sZ, vZ, M, PX, sX, B, hyp, 0, io->dZ, io->dV, io->d_hyp, Kzx, dPzx));
    S64_TIME(5);
    // ---- Cholesky backward: K_ZZ-bar = 1/2 L^-T (Phi + Phi^T) L^-1 from the explicit inverse (_step.ElboEngine._chol_backward)
    S64_CALL(dsvgp_phi_symmetrize(ctx, G1, Mp, Mp));
    {
        Zeroed64 z(ctx, prezero);
        S64_CALL(gemm64(ctx, DSVGP_GEMM_TRANS_A | DSVGP_GEMM_B_LOWER | DSVGP_GEMM_OUT_LOWER, Mp, Mp, Mp, 1.0, G1, Mp, Linv, Mp, Yt, Mp));
    }
    {
        Zeroed64 z(ctx, prezero);
        S64_CALL(gemm64(ctx, DSVGP_GEMM_TRANS_A | DSVGP_GEMM_A_UPPER | DSVGP_GEMM_OUT_LOWER, Mp, Mp, Mp, 0.5, Linv, Mp, Yt, Mp, Kbar, Mp));
    }
    S64_CALL(dsvgp_phi_symmetrize(ctx, Kbar, Mp, Mp));
    S64_CALL(bwd64(ctx, pl, prezero, Kbar, Mp, PZ, sZ, vZ, M, PZ, sZ, M, hyp, 1, io->dZ, io->dV, io->d_hyp, H, dPzz));
    // ---- scalar epilogue
    hipLaunchKernelGGL(epilogue64_kernel, dim3(1), dim3(64), 0, main, scal, klsum, Mp, add_kl ? 1 : 0, inv_rows, inv_nd, io->raw_lengthscale,
                       io->raw_outputscale, io->raw_noise, io->d_hyp, io->d_raw_lengthscale, io->d_raw_outputscale, io->d_raw_noise,
                       io->d_constant, io->loss);
    S64_LAUNCHED();
    // (the status copy on the side stream has long finished; the wait orders the next step's clear of the head behind it)
    if (overlap) S64_HIP(hipStreamWaitEvent(main, pl->ev_status, 0));
#undef S64_TIME
    return 0;
}

extern "C" int dsvgp_gather_batch_f64(dsvgp_ctx* ctx, const double* X, const double* Y, const int64_t* idx, int nb, int d, int ycols,
                                      const int* cols, int p, double* xb, double* yb, const double* E, double* Db) {
    if (!ctx || !X || !Y || !idx || !cols || !xb || !yb || nb < 0 || d <= 0 || p < 0 || ycols <= p || (E && !Db)) return DSVGP_EINVAL;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(gather64_kernel, dim3(nb), dim3(64), 0, ctx->stream, X, Y, idx, nb, d, ycols, cols, p, xb, yb, E, Db);
    DSVGP_LAUNCH_CHECK();
    return 0;
}
