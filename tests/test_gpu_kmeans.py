"""GPU: the k-means kernels, the cluster moments and the initialisation built on them (csrc/kmeans.hip, initialization.py) against the
float64 restatement of tests/test_kmeans_host.py.

Shapes (N, d, M): (3000, 3, 37) fused D = 4; (4133, 5, 130) ragged last tile, three centroid chunks, the last one ragged; (2000, 20, 70)
C4's width; (70, 32, 16) the widest fused instance, N just past one tile; (1500, 33, 40) the first composed width; (600, 200, 24) composed.
Label comparisons run on uniform data and leave out the points inside the band (test_kmeans_host.py: at most 1 % there, shown on the
CPU); dist2 is held to 2e-4 of its largest value (the project's float32 tolerance); an update to 1e-6 max|X| (fp64 sums rounded once:
about 6e-8 is achievable); the moments to 1e-12 of their largest entry (fp64 sums of exact products in another order).

"Rows 10:50 assigned alone": the entries refuse M > N, so where M > 40 the slice is rows 10 : 10 + M + 3 (it contains rows 10:50).
M = N on the composed route: the difference form gives exactly zero, the expansion max(|x~|^2 + |z~|^2 - 2 x~.z~, 0) gives a rounding of
the norms: held to the band's own measure, 1e-5 (|x~|^2 + |z~|^2)."""
import ctypes as C
import functools
import math

import pytest
import torch

from test_kmeans_host import (BAND, SHAPE_IDS, SHAPES, assign_reference, blobs, case, distances, in_band, lloyd_reference,
                              moments_reference, update_reference)

pytestmark = pytest.mark.gpu
f32, f64, i32 = torch.float32, torch.float64, torch.int32
TOL = 2e-4
GUARD = 16
EINVAL = -1
ROUTES = [(130, 5), (130, 40)]          # (N, d) of the edge cases: the fused and the composed route
ROUTE_IDS = ["fused", "composed"]


class Guarded:
    """an output with a guard band on either side: NaN for floating point, -777 for integers"""

    def __init__(self, shape, dtype, dev, init=None):
        n = int(math.prod(shape))
        self.fill = float("nan") if dtype.is_floating_point else -777
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        edge = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        return bool(torch.isnan(edge).all()) if self.buf.dtype.is_floating_point else bool((edge == self.fill).all())

    def untouched(self):
        return self.intact() and (bool(torch.isnan(self.t).all()) if self.buf.dtype.is_floating_point else bool((self.t == self.fill).all()))


@pytest.fixture(scope="module")
def env(dsvgp, gpu_device):
    return dsvgp, dsvgp._ops, dsvgp._ops.Context.get(gpu_device), gpu_device


@functools.lru_cache(maxsize=None)
def after_five(N, d, M):
    """the float32 rounding of the restatement's centroids after five iterations: once per shape, shared, never changed"""
    X, Z0 = case(N, d, M)
    return lloyd_reference(X, Z0, 5)[0].float()


def labels_agree(X, Z, labels):
    """labels (GPU) against the restatement's arg-min over the same float32 centroids, outside the band"""
    ref, _ = assign_reference(X, Z)
    keep = ~in_band(X, Z)
    return bool((labels.cpu().long()[keep] == ref[keep]).all()), int((~keep).sum())


def own_inertia(X, Z, labels):
    return ((X.double() - Z.double().cpu()[labels.cpu().long()]) ** 2).sum().item()


# ------------------------------------------------------------------ assignment
@pytest.mark.parametrize("start", ["seeds", "five"])
@pytest.mark.parametrize("N,d,M", SHAPES, ids=SHAPE_IDS)
def test_assignment_matches_the_restatement(env, N, d, M, start):
    dsvgp, ops, ctx, dev = env
    X, Z0 = case(N, d, M)
    Z = Z0 if start == "seeds" else after_five(N, d, M)
    lab, d2 = Guarded((N,), i32, dev), Guarded((N,), f32, dev)
    ops.kmeans_assign(ctx, X.to(dev), Z.to(dev), labels=lab.t, dist2=d2.t)
    ref_l, ref_d = assign_reference(X, Z)
    ok, skipped = labels_agree(X, Z, lab.t)
    err = (d2.t.cpu().double() - ref_d).abs().max().item() / ref_d.max().item()
    print("[kmeans assign] N=%d d=%d M=%d %s: dist2 error %.2e of its largest value, %d points in the band" % (N, d, M, start, err, skipped))
    assert ok
    assert err <= TOL, err
    assert lab.intact() and d2.intact()
    assert int(lab.t.min()) >= 0 and int(lab.t.max()) < M


# ------------------------------------------------------------------ update
@pytest.mark.parametrize("N,d,M", SHAPES, ids=SHAPE_IDS)
def test_update_is_the_float64_mean_of_the_same_labels(env, N, d, M):
    dsvgp, ops, ctx, dev = env
    X, Z0 = case(N, d, M)
    Xg = X.to(dev)
    labels, _ = ops.kmeans_assign(ctx, Xg, Z0.to(dev))
    labels[labels == 1] = 0                                                    # cluster 1 emptied: it keeps its row
    Z, counts = Guarded((M, d), f32, dev, init=Z0), Guarded((M,), i32, dev)
    ops.kmeans_update_(ctx, Xg, labels, Z.t, counts=counts.t)
    ref, ref_counts = update_reference(X, labels.cpu(), Z0)
    err = (Z.t.cpu().double() - ref).abs().max().item()
    print("[kmeans update] N=%d d=%d M=%d: error %.2e (bound %.2e)" % (N, d, M, err, 1e-6 * X.abs().max().item()))
    assert err <= 1e-6 * X.abs().max().item(), err
    assert torch.equal(counts.t.cpu().long(), ref_counts) and int(counts.t[1]) == 0
    assert torch.equal(Z.t[1].cpu(), Z0[1])
    assert Z.intact() and counts.intact()
    again = Z0.to(dev).clone()
    ops.kmeans_update_(ctx, Xg, labels, again)
    assert torch.equal(again, Z.t)


# ------------------------------------------------------------------ Lloyd
@pytest.mark.parametrize("N,d,M", SHAPES, ids=SHAPE_IDS)
def test_lloyd_resumes_matches_the_restatement_and_is_reproducible(env, N, d, M):
    dsvgp, ops, ctx, dev = env
    X, Z0 = case(N, d, M)
    Xg, T = X.to(dev), 4
    out = dict(Z=Guarded((M, d), f32, dev, init=Z0), labels=Guarded((N,), i32, dev), dist2=Guarded((N,), f32, dev),
               counts=Guarded((M,), i32, dev), inertia=Guarded((T + 1,), f64, dev), moved=Guarded((T,), i32, dev))
    ops.kmeans_lloyd_(ctx, Xg, out["Z"].t, T, labels=out["labels"].t, dist2=out["dist2"].t, counts=out["counts"].t,
                      inertia=out["inertia"].t, moved=out["moved"].t)
    assert all(g.intact() for g in out.values())
    inertia, moved = out["inertia"].t.cpu(), out["moved"].t.cpu()
    # two identical calls
    Z2 = Z0.to(dev).clone()
    l2, d2, c2, in2, mv2 = ops.kmeans_lloyd_(ctx, Xg, Z2, T)
    assert torch.equal(Z2, out["Z"].t) and torch.equal(l2, out["labels"].t) and torch.equal(d2, out["dist2"].t)
    assert torch.equal(c2, out["counts"].t) and torch.equal(in2, out["inertia"].t) and torch.equal(mv2, out["moved"].t)
    # four resumed calls of one iteration; every returned state against one step of the restatement
    Zr = Z0.to(dev).clone()
    lab0, _ = ops.kmeans_assign(ctx, Xg, Zr)
    states = [(Z0.clone(), lab0.cpu())]
    for t in range(T):
        lr, dr, cr, inr, mvr = ops.kmeans_lloyd_(ctx, Xg, Zr, 1)
        assert torch.equal(inr.cpu(), inertia[t:t + 2]) and int(mvr[0]) == int(moved[t])
        ok, _ = labels_agree(X, Zr.cpu(), lr)
        assert ok, t
        states.append((Zr.cpu().clone(), lr.cpu()))
    assert torch.equal(Zr, out["Z"].t) and torch.equal(lr, out["labels"].t) and torch.equal(dr, out["dist2"].t)
    assert torch.equal(cr, out["counts"].t)
    assert torch.equal(out["counts"].t.cpu().long(), torch.bincount(out["labels"].t.cpu().long(), minlength=M))
    for t in range(T):
        assert inertia[t + 1].item() <= inertia[t].item() * (1 + 1e-5), (t, inertia)
        assert int(moved[t]) == int((states[t][1] != states[t + 1][1]).sum()), t
    for t in range(T + 1):
        own = own_inertia(X, *states[t])
        assert abs(inertia[t].item() - own) <= TOL * own, (t, inertia[t].item(), own)
    print("[kmeans lloyd] N=%d d=%d M=%d: inertia %s, moved %s" % (N, d, M, ["%.4f" % v for v in inertia.tolist()], moved.tolist()))
    # a slice of the rows assigned alone
    hi = 50 if M <= 40 else 10 + M + 3
    ls, ds = ops.kmeans_assign(ctx, Xg[10:hi].contiguous(), Zr)
    if d <= 32:
        assert torch.equal(ls, out["labels"].t[10:hi]) and torch.equal(ds, out["dist2"].t[10:hi])
    else:
        ok, _ = labels_agree(X[10:hi], Zr.cpu(), ls)
        assert ok
        assert (ds - out["dist2"].t[10:hi]).abs().max().item() <= TOL * out["dist2"].t.max().item()


# ------------------------------------------------------------------ edges, on both routes
@pytest.mark.parametrize("N,d", ROUTES, ids=ROUTE_IDS)
def test_one_centroid_and_one_centroid_per_point(env, N, d):
    dsvgp, ops, ctx, dev = env
    X, _ = case(N, d, 7)
    Xg = X.to(dev)
    Z = X[3:4].to(dev).clone()                                                 # M = 1
    labels, dist2, counts, inertia, moved = ops.kmeans_lloyd_(ctx, Xg, Z, 2)
    assert bool((labels == 0).all()) and counts.tolist() == [N] and moved.tolist() == [0, 0]
    assert (Z.cpu().double() - X.double().mean(0)).abs().max().item() <= 1e-6 * X.abs().max().item()
    ref = distances(X, Z.cpu())[:, 0]
    assert (dist2.cpu().double() - ref).abs().max().item() <= TOL * ref.max().item()
    assert inertia[1].item() <= inertia[0].item() and abs(inertia[2].item() - ref.sum().item()) <= TOL * ref.sum().item()
    Z = Xg.clone()                                                             # M = N: each point its own centroid
    labels, dist2, counts, inertia, moved = ops.kmeans_lloyd_(ctx, Xg, Z, 1)
    assert torch.equal(labels.cpu().long(), torch.arange(N)) and bool((counts == 1).all()) and moved.tolist() == [0]
    assert torch.equal(Z, Xg)
    if d <= 32:
        assert inertia.tolist() == [0.0, 0.0] and bool((dist2 == 0).all())
    else:
        c = X.double().mean(0)
        assert bool((dist2.cpu().double() <= BAND * 2 * ((X.double() - c) ** 2).sum(-1)).all())


@pytest.mark.parametrize("N,d", ROUTES, ids=ROUTE_IDS)
def test_exact_ties_go_to_the_lowest_index(env, N, d):
    dsvgp, ops, ctx, dev = env
    X, Zs = case(N, d, 7)
    Xd = torch.cat([X, X[:70]]).to(dev)                                        # duplicated points
    Zd = torch.cat([Zs, Zs, Zs[:3]]).to(dev)                                   # duplicated centroids: every distance is tied exactly
    labels, dist2 = ops.kmeans_assign(ctx, Xd, Zd)
    assert int(labels.max()) < 7
    ok, _ = labels_agree(Xd.cpu(), Zs, labels)
    assert ok
    if d <= 32:
        alone, d_alone = ops.kmeans_assign(ctx, Xd, Zs.to(dev))
        assert torch.equal(labels, alone) and torch.equal(dist2, d_alone)
        assert torch.equal(labels[:70], labels[N:]) and torch.equal(dist2[:70], dist2[N:])
    same = torch.full((100, d), 0.25, device=dev)                              # all-equal points, all-equal centroids
    labels, dist2, counts, _, _ = ops.kmeans_lloyd_(ctx, same, same[:5].clone(), 1)
    assert bool((labels == 0).all()) and counts.tolist() == [100, 0, 0, 0, 0]


@pytest.mark.parametrize("N,d", ROUTES, ids=ROUTE_IDS)
def test_zero_iterations_is_one_assignment(env, N, d):
    dsvgp, ops, ctx, dev = env
    X, Z0 = case(N, d, 7)
    Xg, Z = X.to(dev), Guarded((7, d), f32, dev, init=Z0)
    labels, dist2, counts, inertia, moved = ops.kmeans_lloyd_(ctx, Xg, Z.t, 0)
    la, da = ops.kmeans_assign(ctx, Xg, Z0.to(dev))
    assert torch.equal(labels, la) and torch.equal(dist2, da) and torch.equal(Z.t.cpu(), Z0) and Z.intact()
    assert moved.numel() == 0 and inertia.shape == (1,)
    assert abs(inertia[0].item() - da.double().sum().item()) <= 1e-12 * da.double().sum().item()
    assert torch.equal(counts.cpu().long(), torch.bincount(la.cpu().long(), minlength=7))


@pytest.mark.parametrize("N,d", ROUTES, ids=ROUTE_IDS)
def test_refusals_touch_nothing(env, N, d):
    dsvgp, ops, ctx, dev = env
    lib = dsvgp._lib.lib
    X, Z0 = case(N, d, 7)
    M = 7
    Xg = X.to(dev)
    Z = Guarded((M, d), f32, dev, init=Z0)
    lab, d2, cnt = Guarded((N,), i32, dev), Guarded((N,), f32, dev), Guarded((M,), i32, dev)
    ine, mov = Guarded((3,), f64, dev), Guarded((2,), i32, dev)
    nbytes = ops.kmeans_workspace_bytes(N, d, M)
    assert (nbytes == 0) == (d <= 32)
    wsbuf = torch.zeros(nbytes + 64, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    ws, null = p(wsbuf), C.c_void_p(0)
    good = dict(ctx=ctx.h, x=p(Xg), N=N, d=d, Z=p(Z.t), M=M, it=2, labels=p(lab.t), dist2=p(d2.t), counts=p(cnt.t), inertia=p(ine.t),
                moved=p(mov.t), ws=ws)
    assign = lambda a: lib.dsvgp_kmeans_assign(a["ctx"], a["x"], a["N"], a["d"], a["Z"], a["M"], a["labels"], a["dist2"], a["ws"])
    lloyd = lambda a: lib.dsvgp_kmeans_lloyd(a["ctx"], a["x"], a["N"], a["d"], a["Z"], a["M"], a["it"], a["labels"], a["dist2"], a["counts"],
                                             a["inertia"], a["moved"], a["ws"])
    update = lambda a: lib.dsvgp_kmeans_update(a["ctx"], a["x"], a["N"], a["d"], a["labels"], a["Z"], a["M"], a["counts"])
    bad = [dict(ctx=null), dict(x=null), dict(Z=null), dict(labels=null), dict(dist2=null), dict(N=0), dict(d=0), dict(M=0), dict(M=N + 1),
           dict(N=-3), dict(M=-1)]
    bad_ws = [] if d <= 32 else [dict(ws=null), dict(ws=C.c_void_p(wsbuf.data_ptr() + 4)), dict(N=1000000, M=70000)]
    for change in bad + bad_ws:
        assert assign(dict(good, **change)) == EINVAL, change
        assert lloyd(dict(good, **change)) == EINVAL, change
    for change in (dict(it=-1), dict(counts=null), dict(inertia=null), dict(moved=null)):
        assert lloyd(dict(good, **change)) == EINVAL, change
    for change in (dict(ctx=null), dict(x=null), dict(Z=null), dict(labels=null), dict(counts=null), dict(N=0), dict(d=0), dict(M=0),
                   dict(M=N + 1)):
        assert update(dict(good, **change)) == EINVAL, change
    torch.cuda.synchronize()
    assert all(g.untouched() for g in (lab, d2, cnt, ine, mov))
    assert Z.intact() and torch.equal(Z.t.cpu(), Z0) and not bool(wsbuf.any())
    with pytest.raises(ValueError):
        ops.kmeans_assign(ctx, Xg, Xg.repeat(2, 1))                            # M > N: the wrapper refuses before the call


# ------------------------------------------------------------------ moments
@pytest.mark.parametrize("N,d,M", [(2000, 20, 70), (600, 128, 24)], ids=["N2000-d20-M70", "N600-d128-M24"])
def test_cluster_moments(env, N, d, M):
    dsvgp, ops, ctx, dev = env
    g = torch.Generator().manual_seed(7 * d + M)
    G = torch.randn(N, d, generator=g)
    labels = torch.randint(0, M - 1, (N,), generator=g).int()                  # the last cluster is empty
    out = Guarded((M, d, d), f64, dev)
    ops.cluster_moments(ctx, G.to(dev), labels.to(dev), M, out=out.t)
    Cg, ref = out.t.cpu(), moments_reference(G, labels, M)
    err = (Cg - ref).abs().max().item() / ref.abs().max().item()
    print("[kmeans moments] N=%d d=%d M=%d: error %.2e of the largest entry" % (N, d, M, err))
    assert err <= 1e-12, err
    assert torch.equal(Cg, Cg.transpose(1, 2)) and out.intact()
    assert not bool(Cg[M - 1].any())
    again = ops.cluster_moments(ctx, G.to(dev), labels.to(dev), M)
    assert torch.equal(again, out.t)


def test_cluster_moments_refusals(env):
    dsvgp, ops, ctx, dev = env
    lib = dsvgp._lib.lib
    G, labels = torch.randn(40, 129, device=dev), torch.zeros(40, dtype=i32, device=dev)
    out = Guarded((2, 129, 129), f64, dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    assert lib.dsvgp_cluster_moments(ctx.h, p(G), 40, 129, p(labels), 2, p(out.t), null) == EINVAL              # d = 129
    for args in ((null, 40, 128, p(labels), 2, p(out.t)), (p(G), 40, 128, null, 2, p(out.t)), (p(G), 40, 128, p(labels), 2, null),
                 (p(G), 0, 128, p(labels), 2, p(out.t)), (p(G), 40, 0, p(labels), 2, p(out.t)), (p(G), 40, 128, p(labels), 0, p(out.t)),
                 (p(G), 40, 128, p(labels), 41, p(out.t))):
        assert lib.dsvgp_cluster_moments(ctx.h, *args, null) == EINVAL, args
    torch.cuda.synchronize()
    assert out.untouched()
    with pytest.raises(ValueError):
        ops.cluster_moments(ctx, G, labels, 2)
    with pytest.raises(ValueError):
        dsvgp.gradient_directions(G, labels, 2, 2)


# ------------------------------------------------------------------ directions
def subspace_gradients(N, d, M, p, seed=11):
    """gradients of cluster m = i mod M inside a known p-dimensional subspace (orthonormal basis B[m], coefficient scales 3, 2, 1, ..)
    plus 1e-3 noise; float32"""
    g = torch.Generator().manual_seed(seed)
    B = torch.stack([torch.linalg.qr(torch.randn(d, p, generator=g, dtype=f64))[0] for _ in range(M)])
    labels = (torch.arange(N) % M).int()
    scales = torch.arange(p, 0, -1, dtype=f64)
    coef = torch.randn(N, p, generator=g, dtype=f64) * scales
    G = torch.einsum("ndp,np->nd", B[labels.long()], coef) + 1e-3 * torch.randn(N, d, generator=g, dtype=f64)
    return G.float(), labels, B


def test_gradient_directions_recover_the_subspace(env):
    dsvgp, ops, ctx, dev = env
    N, d, M, p = 1200, 12, 6, 3
    G, labels, B = subspace_gradients(N, d, M, p)
    Cref = moments_reference(G, labels, M)
    lam = torch.linalg.eigvalsh(Cref)
    assert bool((lam[:, d - p] / lam[:, d - p - 1] >= 10).all())               # the construction: lambda_p / lambda_{p+1} >= 10
    V = dsvgp.gradient_directions(G.to(dev), labels.to(dev), M, p)
    assert V.shape == (M * p, d) and V.dtype == f32 and V.device.type == "cuda"
    V = V.cpu().double().reshape(M, p, d)
    assert (V.norm(dim=-1) - 1).abs().max().item() <= 1e-6
    for m in range(M):
        assert (V[m] @ V[m].t() - torch.eye(p, dtype=f64)).abs().max().item() <= 1e-6
        assert (V[m].t() @ V[m] - B[m] @ B[m].t()).norm().item() <= 1e-3
        quotients = torch.einsum("sd,de,se->s", V[m], Cref[m], V[m])
        assert bool((quotients[:-1] > quotients[1:]).all())                    # descending eigenvalue
        for s in range(p):
            assert V[m, s][V[m, s].abs().argmax()] > 0                         # the sign rule


def test_gradient_directions_fill_canonically(env):
    dsvgp, ops, ctx, dev = env
    N, d, M, p = 600, 8, 4, 3
    G, labels, B = subspace_gradients(N, d, M, p, seed=13)
    labels = (torch.arange(N) % 3).int()                                       # cluster 3 is empty
    u = torch.tensor([0.0, -3.0, 0.0, 4.0, 0.0, 0.0, 0.0, 0.0]) / 5.0
    G[labels == 1] = torch.randn(int((labels == 1).sum()), 1, generator=torch.Generator().manual_seed(2)) * u        # cluster 1: rank 1
    V = dsvgp.gradient_directions(G.to(dev), labels.to(dev), M, p).cpu().double().reshape(M, p, d)
    eye = torch.eye(d, dtype=f64)
    assert torch.equal(V[3], eye[:p])                                          # empty: e_0, e_1, e_2
    ud = u.double() / u.double().norm()
    assert (V[1, 0] - ud).abs().max().item() <= 1e-6                           # its one direction, the largest entry positive
    assert (V[1, 1] - eye[0]).abs().max().item() <= 1e-6                       # e_0 is orthogonal to it already
    e1 = eye[1] - (eye[1] @ ud) * ud
    assert (V[1, 2] - e1 / e1.norm()).abs().max().item() <= 1e-6               # e_1 made orthogonal to it
    for m in range(M):
        assert (V[m] @ V[m].t() - torch.eye(p, dtype=f64)).abs().max().item() <= 1e-6


def test_python_entry_points(env):
    dsvgp, ops, ctx, dev = env
    N, d, M = 2000, 20, 70
    X, _ = case(N, d, M)
    a = dsvgp.kmeans_inducing_points(X.to(dev), M, iterations=3, generator=torch.Generator().manual_seed(4))
    b = dsvgp.kmeans_inducing_points(X.to(dev), M, iterations=3, generator=torch.Generator().manual_seed(4))
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    seeds = X[torch.randperm(N, generator=torch.Generator().manual_seed(4))[:M]]
    c = dsvgp.kmeans_inducing_points(X.to(dev), M, iterations=3, init=seeds)
    assert all(torch.equal(s, t) for s, t in zip(a, c))
    assert a.centroids.shape == (M, d) and a.inertia.shape == (4,) and a.moved.shape == (3,) and a.counts.sum().item() == N
    ref = lloyd_reference(X, seeds, 3)
    assert abs(a.inertia[-1].item() - ref[4][-1]) <= 1e-3 * ref[4][-1]
    e = dsvgp.kmeans_inducing_points(X.double().to(dev), M, iterations=3, init=seeds.double())
    assert e.centroids.dtype == f64 and e.distances.dtype == f64 and torch.equal(e.centroids.float(), a.centroids)
    Xb, which = blobs(600, 5, 6)                                               # outcome on blobs: one seed per blob brings the blobs back
    r = dsvgp.kmeans_inducing_points(Xb.to(dev), 6, iterations=3, init=Xb[:6])
    assert torch.equal(r.labels.cpu().long(), which) and r.moved[-1].item() == 0
    Y = torch.cat([X[:, :1], torch.randn(N, d, generator=torch.Generator().manual_seed(1))], 1)
    Zi, Vi = dsvgp.initialize_inducing(X.to(dev), Y.to(dev), M, 2, iterations=3, generator=torch.Generator().manual_seed(4))
    assert torch.equal(Zi, a.centroids) and Vi.shape == (2 * M, d)
    assert torch.equal(Vi, dsvgp.gradient_directions(Y[:, 1:].to(dev), a.labels, M, 2))
    Zv, Vv = dsvgp.initialize_inducing(X.to(dev), Y[:, 0].to(dev), M, 2, iterations=3, generator=torch.Generator().manual_seed(4))
    assert torch.equal(Zv, a.centroids) and torch.equal(Vv.cpu(), torch.eye(d)[:2].repeat(M, 1))        # value-only data: canonical


# ------------------------------------------------------------------ harness
def dataset(n, d, seed=0):
    """f(x) = sin(a.x) + 0.5 cos(b.x) with its gradient: (X [n, d], Y [n, d + 1])"""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g)
    a, b = torch.randn(d, generator=g) * (3.0 / math.sqrt(d)), torch.randn(d, generator=g) * (3.0 / math.sqrt(d))
    f = torch.sin(X @ a) + 0.5 * torch.cos(X @ b)
    grad = torch.cos(X @ a)[:, None] * a - 0.5 * torch.sin(X @ b)[:, None] * b
    return X, torch.cat([f[:, None], grad], 1)


def start_of(loop):
    vs = loop.model.variational_strategy
    return vs.inducing_points.detach().clone(), vs.inducing_directions.detach().clone()


@pytest.mark.parametrize("n,d", [(400, 5), (300, 33)], ids=["n400-d5", "n300-d33"])
def test_harness_trains_from_the_kmeans_start(env, n, d):
    from torch.utils.data import TensorDataset
    dsvgp, ops, ctx, dev = env
    from dsvgp_amd import directional_vi
    X, Y = dataset(n, d)
    kw = dict(num_inducing=16, num_directions=2, minibatch_size=100, minibatch_dim=2, num_epochs=2, learning_rate_hypers=0.05, seed=3)
    torch.manual_seed(0)
    loop = directional_vi.setup_training(TensorDataset(X, Y), inducing_data_initialization="kmeans", **kw)
    Z, V = start_of(loop)
    gen = torch.Generator().manual_seed(3)
    Zi, Vi = dsvgp.initialize_inducing(X.to(dev), Y.to(dev), 16, 2, generator=gen)
    assert torch.equal(Z, Zi) and torch.equal(V, Vi)
    torch.manual_seed(0)
    again = directional_vi.setup_training(TensorDataset(X, Y), inducing_data_initialization="kmeans", **kw)
    assert all(torch.equal(s, t) for s, t in zip(start_of(again), (Z, V)))
    losses = []
    for _ in range(2):
        perm = loop.epoch_permutation()
        for start in range(0, n, 100):
            losses.append(loop.step(perm[start:start + 100])[0].item())
    loop.finish()
    per = len(losses) // 2
    first, last = sum(losses[:per]) / per, sum(losses[per:]) / per
    print("[kmeans harness] n=%d d=%d: mean loss of the first epoch %.4f, of the second %.4f" % (n, d, first, last))
    assert all(math.isfinite(l) for l in losses) and last < first
    model, likelihood = dsvgp.train_gp(TensorDataset(X, Y), inducing_data_initialization="kmeans", verbose=False, **kw)
    assert bool(torch.isfinite(model.variational_strategy.inducing_points).all())
    # fixed_inducing_locations wins, as it wins today
    fixed = X[50:66].clone()
    lf = directional_vi.setup_training(TensorDataset(X, Y), inducing_data_initialization="kmeans", fixed_inducing_locations=fixed, **kw)
    assert torch.equal(start_of(lf)[0].cpu(), fixed) and torch.equal(start_of(lf)[1].cpu(), torch.eye(d)[:2].repeat(16, 1))


def test_true_and_false_start_where_they_started(env):
    from torch.utils.data import TensorDataset
    dsvgp, ops, ctx, dev = env
    from dsvgp_amd import directional_vi
    X, Y = dataset(400, 5)
    kw = dict(num_inducing=16, num_directions=2, minibatch_size=100, minibatch_dim=2, seed=3)
    canon = torch.eye(5)[:2].repeat(16, 1)
    Z, V = start_of(directional_vi.setup_training(TensorDataset(X, Y), inducing_data_initialization=True, **kw))
    assert torch.equal(Z.cpu(), X[:16]) and torch.equal(V.cpu(), canon)
    torch.manual_seed(21)
    Z, V = start_of(directional_vi.setup_training(TensorDataset(X, Y), inducing_data_initialization=False, **kw))
    torch.manual_seed(21)
    assert torch.equal(Z.cpu(), torch.rand(16, 5)) and torch.equal(V.cpu(), canon)


def test_the_other_harnesses_construct_and_take_one_step(env):
    from torch.utils.data import TensorDataset
    dsvgp, ops, ctx, dev = env
    from dsvgp_amd import dfree_directional_vi, directional_vi, grad_svgp, shared_directional_vi
    n, d = 400, 5
    X, Y = dataset(n, d)
    kw = dict(num_inducing=16, num_directions=2, minibatch_size=100, minibatch_dim=2, seed=3, inducing_data_initialization="kmeans")
    km = dsvgp.kmeans_inducing_points(X.to(dev), 16, generator=torch.Generator().manual_seed(3))
    idx = torch.arange(100, device=dev)
    # derivative-free data: points only
    loop = directional_vi.setup_training(TensorDataset(X, Y[:, 0].contiguous()), model_class=dfree_directional_vi.GPModel, dfree=True, **kw)
    Z, V = start_of(loop)
    assert torch.equal(Z, km.centroids) and torch.equal(V.cpu(), torch.eye(d)[:2].repeat(16, 1))
    assert math.isfinite(loop.step(idx)[0].item())
    loop.finish()
    model, _ = dfree_directional_vi.train_gp(TensorDataset(X, Y[:, 0].contiguous()), verbose=False, max_steps=1, **kw)
    assert model.variational_strategy.inducing_points.shape == (16, d)
    # shared directions: one set from the moments of all gradients
    loop = directional_vi.setup_training(TensorDataset(X, Y), model_class=shared_directional_vi.GPModel, shared=True, **kw)
    Z, V = start_of(loop)
    one = torch.zeros(n, dtype=i32, device=dev)
    assert torch.equal(Z, km.centroids) and torch.equal(V, dsvgp.gradient_directions(Y[:, 1:].to(dev), one, 1, 2))
    assert math.isfinite(loop.step(idx)[0].item())
    loop.finish()
    # full gradient (grad_svgp): the keyword goes through **args
    loop = grad_svgp.setup_training(TensorDataset(X, Y), d, num_inducing=16, minibatch_size=100, seed=3, inducing_data_initialization="kmeans")
    assert torch.equal(loop.model.variational_strategy.inducing_points.detach(), km.centroids)
    assert math.isfinite(loop.step(idx)[0].item())
    loop.finish()
    with pytest.raises(ValueError):
        grad_svgp.setup_training(TensorDataset(X, Y), d, num_inducing=16, minibatch_size=100, seed=3, inducing_data_initialization="first")
    # full gradient through the directional harness, and the Matern kernel: initialisation is upstream of the engine
    for extra in (dict(num_directions=d, minibatch_dim=d), dict(kernel="matern52"), dict(ard_num_dims=d)):
        loop = directional_vi.setup_training(TensorDataset(X, Y), **dict(kw, **extra))
        assert torch.equal(start_of(loop)[0], km.centroids)
        assert math.isfinite(loop.step(idx)[0].item())
        loop.finish()
