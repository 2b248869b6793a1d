"""Data-driven initialisation of a sparse derivative GP: k-means centroids for the inducing points, and for the inducing directions of
every point the leading eigenvectors of the second-moment matrix of the gradients observed in its cluster -- the subspace a directional
inducing point should carry.  Not in the reference, which starts from the first M data rows and the first p canonical axes.

The clustering and the moment matrices are HIP kernels (csrc/kmeans.hip: no floating-point atomics, fixed-order sums, no host read
inside a call); the M small symmetric eigenproblems run on the CPU in float64 -- initialisation is not the hot path, and the CPU result
is the same on every machine.  There is no CPU fallback for the kernels: a CPU tensor raises ``DsvgpError``.
"""
from collections import namedtuple

import torch

from . import _lib, _ops

KMeansResult = namedtuple("KMeansResult", ["centroids", "labels", "distances", "counts", "inertia", "moved"])

MOMENTS_MAX_DIM = 128          # csrc/kmeans_plan.h: KM_MOM_MAX_D
# an eigenvalue counts towards the numerical rank of C_m when it exceeds this share of the largest one: the gradients are float32, so a
# direction that only their rounding populates carries about (2^-24)^2 of the largest eigenvalue per point; 1e-10 is far above that and
# far below any direction the data populate
RANK_TOLERANCE = 1e-10


def _seeds(X, num_inducing, generator, init):
    N, d = X.shape
    if init is not None:
        if init.dim() != 2 or init.shape != (num_inducing, d):
            raise ValueError("init must be [num_inducing, d] = [%d, %d], got %s" % (num_inducing, d, tuple(init.shape)))
        return init.to(device=X.device, dtype=torch.float32).contiguous().clone()
    perm = torch.randperm(N, generator=generator)          # on the CPU: a seed gives the same start everywhere
    return X[perm[:num_inducing].to(X.device)].to(torch.float32).contiguous()


def kmeans_inducing_points(X, num_inducing, iterations=20, generator=None, init=None):
    """Lloyd's algorithm with a fixed iteration count on the GPU: ``KMeansResult(centroids [M, d], labels [N] int32, distances [N]
    (squared, to the assigned centroid), counts [M] int32, inertia [iterations + 1] float64, moved [iterations] int32)``; labels,
    distances and counts belong to the closing assignment against the returned centroids.  Seeds: ``init`` [M, d], or the rows
    ``X[torch.randperm(N, generator=generator)[:M]]`` (the permutation is drawn on the CPU).  An exact tie goes to the lowest centroid
    index; an emptied cluster keeps its centroid.  A float64 ``X`` is clustered on its float32 copy and the result is cast back."""
    if not torch.is_tensor(X) or X.dim() != 2:
        raise ValueError("X must be a [N, d] tensor")
    N, d = X.shape
    num_inducing, iterations = int(num_inducing), int(iterations)
    if N < 1 or d < 1 or not 1 <= num_inducing <= N:
        raise ValueError("k-means needs 1 <= num_inducing <= N and d >= 1, got N = %d, d = %d, num_inducing = %d" % (N, d, num_inducing))
    if iterations < 0:
        raise ValueError("iterations must be >= 0, got %d" % iterations)
    if X.dtype not in (torch.float32, torch.float64):
        raise ValueError("X must be float32 or float64, got %s" % X.dtype)
    if init is not None and (not torch.is_tensor(init) or init.dim() != 2 or init.shape != (num_inducing, d)):
        raise ValueError("init must be [num_inducing, d] = [%d, %d]" % (num_inducing, d))
    if not X.is_cuda:
        raise _lib.DsvgpError("X must live on the GPU: the k-means kernels have no CPU fallback")
    x32 = X.to(torch.float32).contiguous()
    Z = _seeds(x32, num_inducing, generator, init)
    ctx = _ops.Context.get(X.device)
    labels, dist2, counts, inertia, moved = _ops.kmeans_lloyd_(ctx, x32, Z, iterations)
    return KMeansResult(Z.to(X.dtype), labels, dist2.to(X.dtype), counts, inertia, moved)


def _canonical_fill(kept, d, p):
    """``kept`` [r, d] orthonormal rows (float64) -> [p, d]: the kept rows, then canonical e_0, e_1, .. Gram-Schmidt-orthogonalised
    (twice) against everything before them, skipping an e_k that lies in the span already"""
    rows = [kept[i] for i in range(kept.shape[0])]
    k = 0
    while len(rows) < p:
        if k >= d:
            raise ValueError("cannot complete %d orthonormal directions in dimension %d" % (p, d))
        e = torch.zeros(d, dtype=torch.float64)
        e[k] = 1.0
        k += 1
        for _ in range(2):
            for r in rows:
                e = e - (e @ r) * r
        nrm = e.norm()
        if nrm > 1e-3:
            rows.append(e / nrm)
    return torch.stack(rows) if rows else torch.zeros(0, d, dtype=torch.float64)


def directions_from_moments(C, num_directions):
    """C [M, d, d] (CPU float64, symmetric) -> [M p, d] float64: per cluster the p leading eigenvectors by descending eigenvalue, each
    signed so that its largest-magnitude entry is positive; a cluster whose C has numerical rank below p (an empty one has rank 0) is
    completed with canonical directions orthogonalised against the kept ones.  Rows are unit length, orthonormal per cluster."""
    M, d, _ = C.shape
    p = int(num_directions)
    if not 0 <= p <= d:
        raise ValueError("num_directions must lie in [0, d] = [0, %d], got %d" % (d, p))
    lam, U = torch.linalg.eigh(C)                          # ascending
    out = torch.empty(M, p, d, dtype=torch.float64)
    for m in range(M):
        top = lam[m, -1].item()
        r = 0
        while r < p and top > 0.0 and lam[m, d - 1 - r].item() > RANK_TOLERANCE * top:
            r += 1
        kept = U[m, :, d - r:].flip(-1).t().contiguous() if r else torch.zeros(0, d, dtype=torch.float64)
        if r:
            big = kept.abs().argmax(dim=1)
            sign = torch.sign(kept[torch.arange(r), big])
            kept = kept * sign[:, None]
        out[m] = kept if r == p else _canonical_fill(kept, d, p)
    return out.reshape(M * p, d)


def gradient_directions(G, labels, num_inducing, num_directions):
    """Inducing directions [M p, d] from the gradients G [N, d] of the points and their cluster labels [N]: per cluster the p leading
    eigenvectors of C_m = sum_{i in m} g_i g_i^T (uncentred: the subspace the gradients live in, not their scatter).  C_m is formed on
    the GPU (dsvgp_cluster_moments, d <= 128), the eigenvectors on the CPU in float64 (``directions_from_moments``)."""
    if not torch.is_tensor(G) or G.dim() != 2 or not torch.is_tensor(labels) or labels.dim() != 1 or labels.shape[0] != G.shape[0]:
        raise ValueError("G must be [N, d] with one label per row")
    N, d = G.shape
    M, p = int(num_inducing), int(num_directions)
    if not 1 <= M <= N or not 0 <= p <= d:
        raise ValueError("gradient_directions needs 1 <= num_inducing <= N and 0 <= num_directions <= d")
    if d > MOMENTS_MAX_DIM:
        raise ValueError("gradient_directions is built for d <= %d, got %d (keep canonical directions there)" % (MOMENTS_MAX_DIM, d))
    if not G.is_cuda or not labels.is_cuda:
        raise _lib.DsvgpError("G and labels must live on the GPU: the moment kernel has no CPU fallback")
    ctx = _ops.Context.get(G.device)
    C = _ops.cluster_moments(ctx, G.to(torch.float32).contiguous(), labels.to(torch.int32).contiguous(), M)
    return directions_from_moments(C.cpu(), p).to(device=G.device, dtype=G.dtype)


def canonical_directions(num_inducing, num_directions, d):
    """the first p canonical axes tiled over the points, [M p, d] (directional_vi.setup_training)"""
    return torch.eye(d)[:num_directions].repeat(num_inducing, 1)


def initialize_inducing(X, Y, num_inducing, num_directions, iterations=20, generator=None):
    """(Z [M, d], V [M p, d]) for a model on the data (X [N, d], Y): k-means centroids, and gradient directions from ``Y[:, 1:]`` when
    Y carries d + 1 columns (value, gradient) and d <= 128 -- canonical directions otherwise (value-only data, or a wider input)."""
    km = kmeans_inducing_points(X, num_inducing, iterations=iterations, generator=generator)
    d = X.shape[1]
    if torch.is_tensor(Y) and Y.dim() == 2 and Y.shape[1] == d + 1 and Y.shape[0] == X.shape[0] and d <= MOMENTS_MAX_DIM:
        V = gradient_directions(Y[:, 1:].to(device=X.device), km.labels, num_inducing, num_directions)
    else:
        V = canonical_directions(num_inducing, num_directions, d)
    return km.centroids, V.to(X)
