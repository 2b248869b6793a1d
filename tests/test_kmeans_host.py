"""CPU: the surface and the float64 restatement of the data-driven initialisation (csrc/kmeans.hip, initialization.py: dsvgp_kmeans_assign /
_update / _lloyd, dsvgp_cluster_moments, ``kmeans_inducing_points``, ``gradient_directions``, ``initialize_inducing``,
``setup_training(..., inducing_data_initialization="kmeans")``).

``lloyd_reference`` restates Lloyd's algorithm in float64: full-matrix DIFFERENCE-form distances, the lowest index on a tie, exact means,
an empty cluster keeps its centroid.  tests/test_gpu_kmeans.py imports the helpers and holds the kernels to them one step at a time.

The band.  A float32 kernel cannot be held to the float64 arg-min where the best and the second-best squared distance nearly agree.  The
GPU test leaves out the points whose two distances differ by no more than 1e-5 d2_second (fused route, d <= 32: the difference form's
error is relative to the distance) or 1e-5 (|x~|^2 + |z~|^2) (composed route: the expansion's error is relative to the norms about the
centre of Z).  This file shows, on the inputs the GPU test uses, that those points are at most 1 % in the restatement itself: a condition
on the inputs, not a measurement of the kernels."""
import functools
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = torch.float64
#          N     d    M
SHAPES = [(3000, 3, 37), (4133, 5, 130), (2000, 20, 70), (70, 32, 16), (1500, 33, 40), (600, 200, 24)]
SHAPE_IDS = ["N%d-d%d-M%d" % s for s in SHAPES]
BAND = 1e-5
BAND_SHARE = 0.01


@functools.lru_cache(maxsize=None)
def case(N, d, M):
    """(X float32 [N, d] uniform on [0, 1]^d, seeds float32 [M, d] drawn from its rows): once per shape, shared, never changed"""
    g = torch.Generator().manual_seed(1000 * d + M)
    X = torch.rand(N, d, generator=g)
    return X, X[torch.randperm(N, generator=g)[:M]].clone()


def blobs(N, d, M, seed=0):
    """a mixture of M tight blobs (outcome tests only: near-ties between centroids inside a blob are frequent)"""
    g = torch.Generator().manual_seed(seed)
    centres = torch.rand(M, d, generator=g)
    which = torch.arange(N) % M
    return (centres[which] + 0.01 * torch.randn(N, d, generator=g)).float(), which


def distances(X, Z):
    """[N, M] float64 squared distances in the difference form"""
    X, Z = X.to(f64), Z.to(f64)
    return torch.stack([((X - Z[m]) ** 2).sum(-1) for m in range(Z.shape[0])], dim=1)


def lowest_argmin(D2):
    """row-wise arg-min, the LOWEST index on an exact tie, and the minimum"""
    best = D2.min(dim=1, keepdim=True).values
    idx = torch.arange(D2.shape[1]).expand_as(D2).masked_fill(D2 != best, D2.shape[1])
    return idx.min(dim=1).values, best.squeeze(1)


def assign_reference(X, Z):
    return lowest_argmin(distances(X, Z))


def update_reference(X, labels, Z):
    """(means float64 [M, d], counts): exact means of the members; an empty cluster keeps its row"""
    X, out = X.to(f64), Z.to(f64).clone()
    counts = torch.bincount(labels.long(), minlength=Z.shape[0])
    sums = torch.zeros_like(out).index_add_(0, labels.long(), X)
    live = counts > 0
    out[live] = sums[live] / counts[live].to(f64)[:, None]
    return out, counts


def lloyd_reference(X, Z0, T):
    """float64 Lloyd: T times assign -> inertia -> update, then a closing assignment.  Returns (Z, labels, dist2, counts of the closing
    assignment, inertia [T + 1], moved [T], the list of the T + 1 label arrays)"""
    Z = Z0.to(f64).clone()
    inertia, moved, history = [], [], []
    for t in range(T + 1):
        labels, d2 = assign_reference(X, Z)
        inertia.append(d2.sum().item())
        if history:
            moved.append(int((labels != history[-1]).sum()))
        history.append(labels)
        if t < T:
            Z, _ = update_reference(X, labels, Z)
    counts = torch.bincount(labels, minlength=Z.shape[0])
    return Z, labels, d2, counts, inertia, moved, history


def moments_reference(G, labels, M):
    """C [M, d, d] float64 = sum over the members of g g^T"""
    G = G.to(f64)
    C = torch.zeros(M, G.shape[1], G.shape[1], dtype=f64)
    for m in range(M):
        Gm = G[labels.long() == m]
        C[m] = Gm.t() @ Gm
    return C


def in_band(X, Z):
    """bool [N]: the points whose best and second-best squared distances differ by no more than the band (module docstring)"""
    X, Z = X.to(f64), Z.to(f64)
    if Z.shape[0] < 2:
        return torch.zeros(X.shape[0], dtype=torch.bool)
    D2 = distances(X, Z)
    two, idx = D2.topk(2, dim=1, largest=False)
    gap = two[:, 1] - two[:, 0]
    if X.shape[1] <= 32:
        return gap <= BAND * two[:, 1]
    c = Z.mean(dim=0)
    xn = ((X - c) ** 2).sum(-1)
    zn = ((Z - c) ** 2).sum(-1)
    return gap <= BAND * (xn + torch.maximum(zn[idx[:, 0]], zn[idx[:, 1]]))


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("N,d,M", SHAPES, ids=SHAPE_IDS)
def test_reference_inertia_never_increases_and_the_band_is_thin(N, d, M):
    X, Z0 = case(N, d, M)
    Z, labels, d2, counts, inertia, moved, history = lloyd_reference(X, Z0, 5)
    assert all(b <= a * (1 + 1e-12) for a, b in zip(inertia, inertia[1:])), inertia
    assert int(counts.sum()) == N and len(moved) == 5 and len(history) == 6
    for name, Zs in (("seeds", Z0), ("after five iterations", Z)):
        share = in_band(X, Zs).double().mean().item()
        print("[band] N=%d d=%d M=%d %s: share %.5f" % (N, d, M, name, share))
        assert share <= BAND_SHARE, (name, share)


def test_reference_edges():
    X, _ = case(70, 32, 16)
    Z, labels, d2, counts, inertia, _, _ = lloyd_reference(X, X, 2)              # M = N: each point its own centroid
    assert inertia == [0.0, 0.0, 0.0] and torch.equal(labels, torch.arange(70)) and bool((counts == 1).all())
    same = torch.full((50, 4), 0.25)
    Z, labels, d2, counts, inertia, _, _ = lloyd_reference(same, same[:5], 1)    # all-equal points: label 0, the others keep their rows
    assert bool((labels == 0).all()) and counts.tolist() == [50, 0, 0, 0, 0] and torch.equal(Z, same[:5].double())
    Xb, which = blobs(600, 5, 6)
    Z, labels, *_ = lloyd_reference(Xb, Xb[:6], 3)                               # one seed per blob: the blobs come back
    assert torch.equal(labels, which)
    C = moments_reference(Xb, labels, 6)
    assert torch.allclose(C, C.transpose(1, 2), rtol=1e-12) and torch.allclose(C.sum(0), Xb.double().t() @ Xb.double(), rtol=1e-12)


# ------------------------------------------------------------------ the surface
NEW = {"dsvgp_kmeans_workspace_bytes": 3, "dsvgp_kmeans_assign": 9, "dsvgp_kmeans_update": 8, "dsvgp_kmeans_lloyd": 13,
       "dsvgp_cluster_moments": 8}


def test_library_exports_declares_and_binds_the_new_entries(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n, nargs in NEW.items():
        assert hasattr(dsvgp._lib.lib, n), "missing export: " + n
        assert n in dsvgp._lib.SIGNATURES, "missing binding: " + n
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, hdr, flags=re.S)
        assert decl, "not declared in include/dsvgp.h: " + n
        assert len(decl.group(1).split(",")) == len(dsvgp._lib.SIGNATURES[n][1]) == nargs, n


def test_size_helper_is_a_host_function_and_refuses_with_zero(dsvgp):
    ws = dsvgp._ops.kmeans_workspace_bytes
    assert ws(1000, 3, 10) == 0 and ws(1000, 32, 10) == 0                         # fused route: registers and LDS only
    for bad in ((0, 33, 1), (10, 0, 1), (10, 33, 0), (10, 33, 11), (-5, 33, 2), (1000000, 40, 70000)):
        assert ws(*bad) == 0, bad
    assert 0 < ws(100, 33, 10) < ws(200, 33, 10) < ws(200, 33, 20) < ws(400, 33, 40)
    assert ws(100, 33, 10) % 16 == 0
    assert ws(10 ** 6, 200, 512) == ws(10 ** 5, 200, 512) < (1 << 28)             # row blocks: nothing of size N x M


def test_python_surface(dsvgp):
    params = lambda f: list(inspect.signature(f).parameters)
    sig = inspect.signature(dsvgp.kmeans_inducing_points)
    assert params(dsvgp.kmeans_inducing_points) == ["X", "num_inducing", "iterations", "generator", "init"]
    assert [sig.parameters[k].default for k in ("iterations", "generator", "init")] == [20, None, None]
    assert dsvgp.KMeansResult._fields == ("centroids", "labels", "distances", "counts", "inertia", "moved")
    assert params(dsvgp.gradient_directions) == ["G", "labels", "num_inducing", "num_directions"]
    assert params(dsvgp.initialize_inducing) == ["X", "Y", "num_inducing", "num_directions", "iterations", "generator"]
    assert dsvgp.initialization.kmeans_inducing_points is dsvgp.kmeans_inducing_points


def test_python_refusals_before_any_device_work(dsvgp):
    X = torch.rand(20, 3)
    with pytest.raises(dsvgp._lib.DsvgpError):
        dsvgp.kmeans_inducing_points(X, 4)
    with pytest.raises(dsvgp._lib.DsvgpError):
        dsvgp.gradient_directions(X, torch.zeros(20, dtype=torch.int32), 4, 2)
    for call in (lambda: dsvgp.kmeans_inducing_points(X[0], 4), lambda: dsvgp.kmeans_inducing_points(X, 21),
                 lambda: dsvgp.kmeans_inducing_points(X, 0), lambda: dsvgp.kmeans_inducing_points(X, 4, iterations=-1),
                 lambda: dsvgp.kmeans_inducing_points(X, 4, init=torch.zeros(4, 2)),
                 lambda: dsvgp.gradient_directions(X, torch.zeros(19, dtype=torch.int32), 4, 2),
                 lambda: dsvgp.gradient_directions(X, torch.zeros(20, dtype=torch.int32), 4, 4),
                 lambda: dsvgp.gradient_directions(torch.rand(20, 129), torch.zeros(20, dtype=torch.int32), 4, 2)):
        with pytest.raises(ValueError):
            call()


def test_directions_from_moments_rule(dsvgp):
    """the CPU half of ``gradient_directions``: descending eigenvalues, the sign rule, the canonical fill"""
    dfm = dsvgp.initialization.directions_from_moments
    g = torch.Generator().manual_seed(5)
    Q, _ = torch.linalg.qr(torch.randn(6, 6, generator=g, dtype=f64))
    lam = torch.tensor([9.0, 4.0, 1.0, 1e-3, 1e-4, 1e-5], dtype=f64)
    u = torch.tensor([0.0, -3.0, 0.0, 4.0, 0.0, 0.0], dtype=f64) / 5.0
    C = torch.stack([Q @ torch.diag(lam) @ Q.t(), torch.zeros(6, 6, dtype=f64), torch.outer(u, u)])
    V = dfm(C, 3).reshape(3, 3, 6)
    for m in range(3):
        assert torch.allclose(V[m] @ V[m].t(), torch.eye(3, dtype=f64), atol=1e-12)
    for s in range(3):
        assert abs(abs((V[0, s] @ Q[:, s]).item()) - 1.0) < 1e-10
        assert V[0, s][V[0, s].abs().argmax()] > 0
    assert torch.equal(V[1], torch.eye(6, dtype=f64)[:3])                        # an empty cluster: canonical directions
    assert torch.allclose(V[2, 0], u, atol=1e-12)                                # rank 1: its direction, largest entry positive ..
    assert torch.allclose(V[2, 1], torch.eye(6, dtype=f64)[0]) and V[2, 2][1] > 0.0        # .. then e_0, then e_1 made orthogonal to it
    assert abs((V[2, 2] @ u).item()) < 1e-12


def test_setup_training_refuses_unknown_strings_and_a_collective_before_any_device_work(dsvgp, monkeypatch):
    from dsvgp_amd import directional_vi, grad_svgp
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("device work")))
    with pytest.raises(ValueError, match="kmeans"):
        directional_vi.setup_training(None, 4, 1, 8, 1, inducing_data_initialization="k-means")
    with pytest.raises(ValueError, match="kmeans"):
        directional_vi.train_gp(None, 4, 1, 8, 1, inducing_data_initialization="first", verbose=False)
    for mod in (directional_vi, grad_svgp):
        monkeypatch.setattr(mod.dist, "is_available", lambda: True)
        monkeypatch.setattr(mod.dist, "is_initialized", lambda: True)
        monkeypatch.setattr(mod.dist, "get_world_size", lambda: 2)
    with pytest.raises(ValueError, match="one rank"):
        directional_vi.setup_training(None, 4, 1, 8, 1, inducing_data_initialization="kmeans")
    sig = inspect.signature(directional_vi.setup_training)
    assert sig.parameters["inducing_data_initialization"].default is True          # a new VALUE of the keyword, no new parameter
    assert list(sig.parameters)[-3:] == ["data_directions", "kernel", "ard_num_dims"]


def test_host_check_of_the_plan_builds_and_passes(tmp_path):
    """tools/kmeans_check.cpp on csrc/kmeans_plan.h: every (point, centroid) pair once, every offset in bounds, nothing past N or M"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tools/kmeans_check.cpp")
    exe = str(tmp_path / "kmeans_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "gp-derivatives-variational-inference_amd", "csrc"),
                           os.path.join(ROOT, "tools", "kmeans_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert len(re.findall(r"fused   every width: d +\d+ D +\d+: ok", out.stdout)) == 32
    for N, d, M in SHAPES:
        assert re.search(r"(fused  |composed) N +%d d +%d M +%d: ok" % (N, d, M), out.stdout), (N, d, M)
    assert "every (point, centroid) pair visited exactly once, every offset in bounds" in out.stdout
    assert "FAILED" not in out.stdout
