"""GPU tests of the tiled fp64 kernel assembly (csrc/assemble64_tiled.hip): float64 models with more than 16 directions per
point -- the full-gradient SVGP at d = 20 (Welch) and d = 45 (stellarator), num_directions > 16, micro-blocks up to q = 96.

Tolerances are the stated float64 tolerances of tests/test_gpu_fp64.py, not loosened for p > 16: kernel entries 1e-12,
kernel backward 1e-10, loss and predictive moments 1e-9, gradients 1e-7 relative in max-norm per parameter; old path against
tiled path on the same packs (reordered double sums only): forward 1e-13, backward 1e-11."""
import contextlib
import glob
import io
import os

import numpy as np
import pytest
import torch

import dsvgp_oracle as O
from _golden import GOLDEN, kernel_error
from test_gpu_fp64 import make_problem64, relmax

pytestmark = pytest.mark.gpu
f64 = torch.float64
EINVAL = -1                                             # DSVGP_EINVAL of include/dsvgp.h
FP64DIRS = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "fp64dirs_*.npz")))

# (n1, n2, d, p): the seven shapes of test_kernel_f64_forward_backward_random_shapes ...
OLD_SHAPES = [(37, 53, 5, 2), (16, 16, 20, 5), (9, 130, 3, 0), (20, 11, 10, 10), (7, 40, 45, 1), (130, 7, 2, 1), (5, 6, 17, 16)]
# ... more than 16 directions, wide inputs, p = 0 at a wide d, ragged tiles, single points
NEW_SHAPES = [(12, 14, 20, 20), (30, 30, 20, 20), (11, 13, 24, 17), (9, 11, 45, 31), (9, 11, 45, 45), (7, 9, 95, 95),
              (5, 6, 20, 95), (10, 12, 200, 30), (6, 7, 200, 45), (4, 5, 95, 20), (6, 7, 1030, 3), (33, 70, 200, 0),
              (67, 131, 20, 5), (1, 9, 20, 20), (9, 1, 24, 17), (1, 1, 45, 45), (23, 3, 7, 64), (3, 23, 7, 32)]
SHAPES = OLD_SHAPES + NEW_SHAPES


def _packs(dsvgp, dev, x1, x2, v1, v2, ell, s=1.0):
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    n1, d = x1.shape
    p = v1.shape[0] // n1 if n1 else 0
    hyp = torch.tensor([ell, s, 0.1, 0.0], dtype=f64, device=dev)
    x1d = x1.double().to(dev).contiguous()
    center = x1d.mean(0).contiguous()
    p1 = ops.pack_points_f64(ctx, x1d, v1.double().to(dev).contiguous(), p, hyp, center)
    p2 = ops.pack_points_f64(ctx, x2.double().to(dev).contiguous(), v2.double().to(dev).contiguous(), p, hyp, center)
    return ctx, hyp, p1, p2


def _random_inputs(n1, n2, d, p):
    g = torch.Generator().manual_seed(n1 * 1000 + n2 + 7 * p)
    x1, x2 = torch.rand(n1, d, generator=g, dtype=f64), torch.rand(n2, d, generator=g, dtype=f64)
    v1 = torch.randn(n1 * p, d, generator=g, dtype=f64)
    v2 = torch.randn(n2 * p, d, generator=g, dtype=f64)
    # lengthscale 0.9 as tests/test_gpu_fp64.py; at wide d it grows with sqrt(d) so that the kernel values stay of unit scale
    return g, x1, x2, v1, v2, 0.9 if d <= 50 else 0.9 * (d / 20.0) ** 0.5, 1.7


def _bwd_errors(dx, dv, d_hyp, xr, vr, er, sr, p):
    errs = dict(dx=relmax(dx, xr.grad), dell=abs(d_hyp[0].item() - er.grad.item()) / abs(er.grad.item()),
                ds=abs(d_hyp[1].item() - sr.grad.item()) / abs(sr.grad.item()))
    if p:
        errs["dv"] = relmax(dv, vr.grad)
    return errs


@pytest.mark.parametrize("n1,n2,d,p", SHAPES)
def test_tiled_forward_and_backward_match_the_oracle(dsvgp, gpu_device, n1, n2, d, p):
    """forward vs the oracle's pair-wise kernel (1e-12); backward (x1, v1, lengthscale, outputscale) vs autograd through it (1e-10)"""
    ops = dsvgp._ops
    g, x1, x2, v1, v2, ell, s = _random_inputs(n1, n2, d, p)
    ctx, hyp, p1, p2 = _packs(dsvgp, gpu_device, x1, x2, v1, v2, ell, s)
    K = ops.kernel_fwd_f64_tiled(ctx, p1, n1, p2, n2, d, p, hyp)
    xr, vr = x1.clone().requires_grad_(True), v1.clone().requires_grad_(True)
    er, sr = torch.tensor(ell, dtype=f64, requires_grad=True), torch.tensor(s, dtype=f64, requires_grad=True)
    Kref = sr * O.kernel_matrix(xr, x2, vr, v2, er)
    e_fwd = relmax(K, Kref.detach())
    print("[parity] kernel_fwd_f64_tiled %s: %.2e" % ((n1, n2, d, p), e_fwd))
    assert e_fwd < 1e-12
    G = torch.randn(K.shape, generator=g, dtype=f64)
    (Kref * G).sum().backward()
    dx = torch.zeros(n1, d, dtype=f64, device=gpu_device)
    dv = torch.zeros(max(n1 * p, 1), d, dtype=f64, device=gpu_device)[:n1 * p]
    d_hyp = torch.zeros(4, dtype=f64, device=gpu_device)
    ops.kernel_bwd_f64_tiled(ctx, G.to(gpu_device), p1, n1, p2, n2, d, p, hyp, False, dx, dv, d_hyp)
    errs = _bwd_errors(dx, dv, d_hyp, xr, vr, er, sr, p)
    print("[parity] kernel_bwd_f64_tiled %s: %s" % ((n1, n2, d, p), errs))
    assert max(errs.values()) < 1e-10
    assert d_hyp[2].item() == 0.0 and d_hyp[3].item() == 0.0
    if p > 16:                                          # the public entries take the same geometry by themselves
        K2 = ops.kernel_fwd_f64(ctx, p1, n1, p2, n2, d, p, hyp)
        assert torch.equal(K2, K)


def test_tiled_forward_into_a_strided_view_at_an_odd_offset(dsvgp, gpu_device):
    """ld > n2 q, base 8-byte but not 16-byte aligned: the entries outside the view keep their sentinel"""
    ops = dsvgp._ops
    n1, n2, d, p = 13, 11, 20, 20
    g, x1, x2, v1, v2, ell, s = _random_inputs(n1, n2, d, p)
    ctx, hyp, p1, p2 = _packs(dsvgp, gpu_device, x1, x2, v1, v2, ell, s)
    q = p + 1
    rows, cols, ld = n1 * q, n2 * q, n2 * q + 5
    sentinel = -777.25
    buf = torch.full((rows * ld + 64,), sentinel, dtype=f64, device=gpu_device)
    view = buf.as_strided((rows, cols), (ld, 1), 3)
    assert view.data_ptr() % 16 == 8
    ops.kernel_fwd_f64_tiled(ctx, p1, n1, p2, n2, d, p, hyp, out=view)
    Kref = s * O.kernel_matrix(x1, x2, v1, v2, torch.tensor(ell, dtype=f64))
    assert relmax(view, Kref) < 1e-12
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask.as_strided((rows, cols), (ld, 1), 3).fill_(False)
    assert int(mask.sum()) == buf.numel() - rows * cols and bool((buf[mask] == sentinel).all())
    # an upstream matrix read through such a view
    G = torch.randn(rows, cols, generator=g, dtype=f64)
    gbuf = torch.full((rows * ld + 64,), float("nan"), dtype=f64, device=gpu_device)
    gview = gbuf.as_strided((rows, cols), (ld, 1), 3)
    gview.copy_(G)
    out = []
    for Gd in (G.to(gpu_device), gview):
        dx = torch.zeros(n1, d, dtype=f64, device=gpu_device)
        dv = torch.zeros(n1 * p, d, dtype=f64, device=gpu_device)
        d_hyp = torch.zeros(4, dtype=f64, device=gpu_device)
        ops.kernel_bwd_f64_tiled(ctx, Gd, p1, n1, p2, n2, d, p, hyp, False, dx, dv, d_hyp)
        out.append((dx, dv, d_hyp))
    for a, b in zip(*out):
        assert bool(torch.isfinite(b).all()) and relmax(b, a) < 1e-11


@pytest.mark.parametrize("path", GOLDEN + FP64DIRS, ids=[os.path.basename(p) for p in GOLDEN + FP64DIRS])
def test_tiled_forward_matches_reference_kernel_file(dsvgp, gpu_device, path):
    """every vector of the reference's own kernel file (the existing ones and the p > 16 ones of tools/make_fp64dirs_fixtures.py)"""
    ops = dsvgp._ops
    g = np.load(path)
    t = lambda k: torch.from_numpy(g[k])
    x1, x2, v1, v2, ell = t("x1"), t("x2"), t("v1"), t("v2"), float(g["lengthscale"])
    n1, d = x1.shape
    n2, p = x2.shape[0], int(g["p"])
    ctx, hyp, p1, p2 = _packs(dsvgp, gpu_device, x1, x2, v1, v2, ell)
    K = ops.kernel_fwd_f64_tiled(ctx, p1, n1, p2, n2, d, p, hyp)
    e_sub, e_sum = kernel_error(K, g)
    print("kernel_fwd_f64_tiled %s: error %.2e (row/col sums %s)" % (os.path.basename(path), e_sub,
                                                                      "%.2e" % e_sum if e_sum is not None else "-"))
    assert e_sub < 1e-12 and (e_sum is None or e_sum < 1e-12)
    if "Kdiag" in g:
        assert relmax(torch.diagonal(K), t("Kdiag")) < 1e-12


@pytest.mark.parametrize("p,n,d", [(3, 23, 6), (20, 23, 20)])
def test_tiled_symmetric_backward_and_jitter(dsvgp, gpu_device, p, n, d):
    """K_ZZ: the same points on both sides (gradient flows through both arguments), jitter on the diagonal only"""
    ops = dsvgp._ops
    g = torch.Generator().manual_seed(3 + p)
    x = torch.rand(n, d, generator=g, dtype=f64)
    v = torch.randn(n * p, d, generator=g, dtype=f64)
    ctx, hyp, p1, _ = _packs(dsvgp, gpu_device, x, x, v, v, 0.7, 1.3)
    K = ops.kernel_fwd_f64_tiled(ctx, p1, n, p1, n, d, p, hyp, jitter=1e-3)
    xr, vr = x.clone().requires_grad_(True), v.clone().requires_grad_(True)
    er, sr = torch.tensor(0.7, dtype=f64, requires_grad=True), torch.tensor(1.3, dtype=f64, requires_grad=True)
    Kref = sr * O.kernel_matrix(xr, xr, vr, vr, er)
    assert relmax(K, Kref.detach() + 1e-3 * torch.eye(K.shape[0], dtype=f64)) < 1e-12
    G = torch.randn(K.shape, generator=g, dtype=f64)
    G = G + G.t()                                      # the engine's K_ZZ-bar is symmetric
    (Kref * G).sum().backward()
    # accumulation: the entries add to what the outputs hold
    dx0, dv0 = torch.randn(n, d, generator=g, dtype=f64), torch.randn(n * p, d, generator=g, dtype=f64)
    h0 = torch.tensor([0.5, -2.0, 3.0, 4.0], dtype=f64)
    dx, dv, d_hyp = dx0.to(gpu_device), dv0.to(gpu_device), h0.to(gpu_device)
    ops.kernel_bwd_f64_tiled(ctx, G.to(gpu_device), p1, n, p1, n, d, p, hyp, True, dx, dv, d_hyp)
    errs = _bwd_errors(dx.cpu() - dx0, dv.cpu() - dv0, d_hyp.cpu() - h0, xr, vr, er, sr, p)
    print("[parity] kernel_bwd_f64_tiled symmetric p = %d: %s" % (p, errs))
    assert max(errs.values()) < 1e-10
    assert d_hyp[2].item() == 3.0 and d_hyp[3].item() == 4.0


@pytest.mark.parametrize("n1,n2,d,p", [s for s in SHAPES if s[3] <= 16] + [(60, 90, 20, 16), (40, 70, 10, 10), (50, 50, 5, 0)])
def test_register_path_and_tiled_path_agree_at_p_le_16(dsvgp, gpu_device, n1, n2, d, p):
    """the same packs through both paths: reordered double sums only"""
    ops = dsvgp._ops
    g, x1, x2, v1, v2, ell, s = _random_inputs(n1, n2, d, p)
    ctx, hyp, p1, p2 = _packs(dsvgp, gpu_device, x1, x2, v1, v2, ell, s)
    K_old = ops.kernel_fwd_f64(ctx, p1, n1, p2, n2, d, p, hyp)
    K_new = ops.kernel_fwd_f64_tiled(ctx, p1, n1, p2, n2, d, p, hyp)
    e_fwd = relmax(K_new, K_old)
    G = torch.randn(K_old.shape, generator=g, dtype=f64).to(gpu_device)
    res = []
    for bwd in (ops.kernel_bwd_f64, ops.kernel_bwd_f64_tiled):
        dx = torch.zeros(n1, d, dtype=f64, device=gpu_device)
        dv = torch.zeros(max(n1 * p, 1), d, dtype=f64, device=gpu_device)[:n1 * p]
        d_hyp = torch.zeros(4, dtype=f64, device=gpu_device)
        bwd(ctx, G, p1, n1, p2, n2, d, p, hyp, False, dx, dv, d_hyp)
        res.append((dx, dv, d_hyp[:2]))
    errs = [relmax(b, a) for a, b in zip(*res) if a.numel()]
    print("[parity] fp64 register path vs tiled path %s: forward %.2e, backward %s" % ((n1, n2, d, p), e_fwd, ["%.2e" % e for e in errs]))
    assert e_fwd < 1e-13 and max(errs) < 1e-11


@pytest.mark.parametrize("n1,n2,d,p", [(150, 130, 24, 17), (150, 130, 100, 17), (840, 1265, 5, 2)])
def test_tiled_backward_column_sweep_adds_up(dsvgp, gpu_device, n1, n2, d, p):
    """more than 2048 tiles: a workgroup sweeps several column tiles (accumulators in registers across the sweep at packed widths
    <= 64, atomics per tile above).  The backward is linear in the upstream matrix, so it must equal the sum of the backwards over
    column pieces small enough for one tile per workgroup (the regime checked against the oracle above); and, at p <= 16, the
    register path on the same packs"""
    ops = dsvgp._ops
    g, x1, x2, v1, v2, ell, s = _random_inputs(n1, n2, d, p)
    ctx, hyp, p1, _ = _packs(dsvgp, gpu_device, x1, x2, v1, v2, ell, s)
    q = p + 1
    x1d = x1.to(gpu_device)
    center = x1d.mean(0).contiguous()
    pack2 = lambda lo, hi: ops.pack_points_f64(ctx, x2[lo:hi].to(gpu_device).contiguous(), v2[lo * p:hi * p].to(gpu_device).contiguous(),
                                               p, hyp, center)
    G = torch.randn(n1 * q, n2 * q, generator=g, dtype=f64).to(gpu_device)

    def run(bwd, pieces):
        dx = torch.zeros(n1, d, dtype=f64, device=gpu_device)
        dv = torch.zeros(n1 * p, d, dtype=f64, device=gpu_device)
        d_hyp = torch.zeros(4, dtype=f64, device=gpu_device)
        for lo, hi in pieces:
            bwd(ctx, G[:, lo * q:hi * q], p1, n1, pack2(lo, hi), hi - lo, d, p, hyp, False, dx, dv, d_hyp)
        return dx, dv, d_hyp[:2]
    whole = run(ops.kernel_bwd_f64_tiled, [(0, n2)])
    step = max(1, n2 // 12)
    parts = run(ops.kernel_bwd_f64_tiled, [(lo, min(n2, lo + step)) for lo in range(0, n2, step)])
    errs = [relmax(a, b) for a, b in zip(whole, parts)]
    if p <= 16:
        errs += [relmax(a, b) for a, b in zip(whole, run(ops.kernel_bwd_f64, [(0, n2)]))]
    print("[parity] kernel_bwd_f64_tiled sweep %s: %s" % ((n1, n2, d, p), ["%.2e" % e for e in errs]))
    assert max(errs) < 1e-11


STEP_CASES = [(300, 20, 12, 20, 24), (300, 45, 8, 45, 16), (400, 24, 20, 17, 40), (300, 95, 4, 95, 6)]      # N, d, M, p, B


@pytest.mark.parametrize("N,d,M,p,B", STEP_CASES)
@pytest.mark.parametrize("mll", ["ELBO", "PLL", "ELBO-gram"])
def test_fp64_step_matches_oracle_beyond_16_directions(dsvgp, gpu_device, N, d, M, p, B, mll):
    from dsvgp_amd._step64 import ElboEngine64
    fast = mll == "ELBO-gram"
    mll = "ELBO" if fast else mll
    P, x, y, D, nd = make_problem64(N, d, M, p, B, seed=N + d)
    l_ref, g_ref, mu_ref, var_ref = O.elbo_loss_and_grads(P, x, y, D, nd, mll)
    eng = ElboEngine64(gpu_device)
    eng.fast_min_work = 0
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    loss, grads, mu, varn = eng.loss_and_grads(Pg, x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd, mll, fast=fast)
    torch.cuda.synchronize()
    assert loss.dtype == f64 and all(v.dtype == f64 for v in grads.values())
    if fast:
        assert varn.numel() == 0
        varn = var_ref.to(gpu_device)
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref), "var": relmax(varn, var_ref)}
    for k in O.PARAM_NAMES:
        if k == "chol_variational_covar":
            assert torch.triu(grads[k], 1).abs().max().item() == 0.0
        errs[k] = relmax(grads[k], g_ref[k])
    print("[parity] fp64 step %s %s%s: %s" % ((N, d, M, p, B), mll, " (Gram)" if fast else "", ", ".join("%s %.1e" % kv for kv in errs.items())))
    assert errs["loss"] < 1e-9 and errs["mu"] < 1e-9 and errs["var"] < 1e-9, errs
    assert max(errs[k] for k in O.PARAM_NAMES) < 1e-7, errs


def test_fp64_predict_and_joint_covariance_at_p20(dsvgp, gpu_device):
    from dsvgp_amd._step64 import ElboEngine64
    P, x, y, D, nd = make_problem64(300, 20, 12, 20, 24, seed=4)
    eng = ElboEngine64(gpu_device)
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    xg, Dg = x.to(gpu_device), D.to(gpu_device)
    mu_ref, var_ref = O.predictive(P, x, D)
    mu_j_ref, Sigma_ref = O.predictive_joint(P, x, D)
    _, _, noise = O.constrained(P)
    mu, varn = eng.predict(Pg, xg, Dg)
    assert relmax(mu, mu_ref) < 1e-9 and relmax(varn, var_ref + noise) < 1e-9
    mu_j, Sigma = eng.predict_joint(Pg, xg, Dg)
    assert relmax(mu_j, mu_j_ref) < 1e-9
    assert relmax(Sigma, Sigma_ref + noise * torch.eye(Sigma_ref.shape[0], dtype=f64)) < 1e-9


def test_fp64_dfree_data_outputs_at_p17(dsvgp, gpu_device):
    from dsvgp_amd._step64 import ElboEngine64
    N, d, M, p, B = 400, 24, 10, 17, 30
    P, x, y, D, nd = make_problem64(N, d, M, p, B, seed=9)
    y = y.reshape(B, p + 1)[:, 0].contiguous()
    l_ref, g_ref, mu_ref, var_ref = O.elbo_loss_and_grads(P, x, y, D, nd, "ELBO", data_outputs="values")
    eng = ElboEngine64(gpu_device)
    eng.data_outputs, eng.fast_min_work = "values", 0
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    for fast in (False, True):
        loss, grads, mu, varn = eng.loss_and_grads(Pg, x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd, "ELBO", fast=fast)
        assert abs(loss.item() - l_ref.item()) / abs(l_ref.item()) < 1e-9
        assert relmax(mu, mu_ref) < 1e-9 and (fast or relmax(varn, var_ref) < 1e-9)
        for k in O.PARAM_NAMES:
            assert relmax(grads[k], g_ref[k]) < 1e-7, (fast, k, relmax(grads[k], g_ref[k]))


@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
def test_fp64_shared_directions_at_p17(dsvgp, gpu_device, mll):
    from dsvgp_amd._step64 import ElboEngine64
    N, d, M, p, B = 400, 24, 14, 17, 30
    P, x, y, D, nd = make_problem64(N, d, M, p, B, seed=21)
    g = torch.Generator().manual_seed(4)
    P["inducing_directions"] = torch.eye(d, dtype=f64)[:p] + 0.2 * torch.randn(p, d, generator=g, dtype=f64)
    P["variational_mean"] = 0.3 * torch.randn(M + p, generator=g, dtype=f64)
    P["chol_variational_covar"] = torch.eye(M + p, dtype=f64) + 0.05 * torch.randn(M + p, M + p, generator=g, dtype=f64)
    l_ref, g_ref, mu_ref, var_ref = O.shared_loss_and_grads(P, x, y, D, nd, mll)
    eng = ElboEngine64(gpu_device)
    eng.shared_directions = True
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    loss, grads, mu, varn = eng.loss_and_grads(Pg, x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd, mll)
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref), "var": relmax(varn, var_ref)}
    for k in O.PARAM_NAMES:
        assert grads[k].shape == g_ref[k].shape and grads[k].dtype == f64, k
        errs[k] = relmax(grads[k], g_ref[k])
    print("[parity] fp64 shared directions p = 17 %s: %s" % (mll, ", ".join("%s %.1e" % kv for kv in errs.items())))
    assert errs["loss"] < 1e-9 and errs["mu"] < 1e-9 and errs["var"] < 1e-9, errs
    assert max(errs[k] for k in O.PARAM_NAMES) < 1e-7, errs
    mu2, varn2 = eng.predict(Pg, x.to(gpu_device), D.to(gpu_device))
    assert relmax(mu2, mu_ref) < 1e-9 and relmax(varn2, var_ref) < 1e-9


@pytest.mark.parametrize("mll,fast", [("ELBO", False), ("ELBO", True), ("PLL", False)])
def test_fp64_natural_parameters_at_p20(dsvgp, gpu_device, mll, fast):
    from dsvgp_amd._step64 import ElboEngine64
    from test_ngd import make_ngd_problem
    P, x, y, D, nd = make_ngd_problem(300, 20, 10, 20, 24, seed=7, dtype=f64)
    P["natural_mat"] = 0.5 * (P["natural_mat"] + P["natural_mat"].t())
    l_ref, g_ref, mu_ref, var_ref = O.ngd_loss_and_grads(P, x, y, D, nd, mll)
    eng = ElboEngine64(gpu_device)
    eng.fast_min_work = 0
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    loss, grads, mu, varn = eng.loss_and_grads(Pg, x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd, mll, fast=fast)
    assert set(grads) == set(O.NGD_PARAM_NAMES) and all(v.dtype == f64 for v in grads.values())
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref)}
    if not fast:
        errs["var"] = relmax(varn, var_ref)
    for k in O.NGD_PARAM_NAMES:
        errs[k] = relmax(grads[k], g_ref[k])
    print("[parity] fp64 natural parameters p = 20 %s%s: %s" % (mll, " (Gram)" if fast else "", ", ".join("%s %.1e" % kv for kv in errs.items())))
    assert errs["loss"] < 1e-9 and errs["mu"] < 1e-9 and errs.get("var", 0.0) < 1e-9, errs
    assert max(errs[k] for k in O.NGD_PARAM_NAMES) < 1e-7, errs
    mu_p, var_p = eng.predict(Pg, x.to(gpu_device), D.to(gpu_device))
    assert relmax(mu_p, mu_ref) < 1e-9 and relmax(var_p, var_ref) < 1e-9


def test_operator_forward_backward_fp64_at_p20(dsvgp, gpu_device):
    """RBFKernelDirectionalGrad on float64 inputs with 20 directions per point, forward and autograd"""
    g = torch.Generator().manual_seed(5)
    n1, n2, d, p = 9, 7, 20, 20
    x1, x2 = torch.rand(n1, d, generator=g, dtype=f64), torch.rand(n2, d, generator=g, dtype=f64)
    v1, v2 = torch.randn(n1 * p, d, generator=g, dtype=f64), torch.randn(n2 * p, d, generator=g, dtype=f64)
    k = dsvgp._rbf_mod.RBFKernelDirectionalGrad().to(device=gpu_device, dtype=f64)
    K = k(x1.to(gpu_device), x2.to(gpu_device), v1=v1.to(gpu_device), v2=v2.to(gpu_device))
    ell = torch.nn.functional.softplus(torch.zeros((), dtype=f64))
    assert K.dtype == f64 and relmax(K, O.kernel_matrix(x1, x2, v1, v2, ell)) < 1e-12


def _losses(fn):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn()
    ls = [float(l.split("loss: ")[1].split(",")[0]) for l in buf.getvalue().splitlines() if l.startswith(("Epoch", "Done! loss"))]
    return out, ls


def test_harnesses_under_float64_default_beyond_16_directions(dsvgp, gpu_device):
    """the reference's experiment setting (torch.set_default_dtype(torch.float64)): the full-gradient SVGP at dim = 20 and
    directional_vi with 17 directions at dim = 24"""
    from torch.utils.data import TensorDataset
    from dsvgp_amd._step64 import ElboEngine64
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(0)
        n, dim = 300, 20
        X, Xt = torch.rand(n, dim), torch.rand(40, dim)
        Y, Yt = O.testfun(X), O.testfun(Xt)
        assert X.dtype == f64 and Y.shape == (n, dim + 1)
        G = dsvgp.grad_svgp
        (model, lik), ls = _losses(lambda: G.train_gp(TensorDataset(X, Y), dim, num_inducing=12, minibatch_size=100, num_epochs=10,
                                                       tqdm=False, seed=1))
        print("grad_svgp float64 dim = 20 losses:", ls)
        assert isinstance(model.engine, ElboEngine64) and len(ls) >= 2 and ls[-1] < ls[0]
        means, variances = G.eval_gp(TensorDataset(Xt, Yt), model, lik, minibatch_size=20)
        assert means.dtype == f64 and means.shape == (40 * 21,) and bool(torch.isfinite(means).all()) and bool((variances > 0).all())

        dim, p = 24, 17
        X, Xt = torch.rand(n, dim), torch.rand(40, dim)
        Y, Yt = O.testfun(X), O.testfun(Xt)
        (model, lik), ls = _losses(lambda: dsvgp.train_gp(TensorDataset(X, Y), num_inducing=12, num_directions=p, minibatch_size=100,
                                                           minibatch_dim=p, num_epochs=10, seed=0))
        print("directional_vi float64 dim = 24, 17 directions, losses:", ls)
        assert isinstance(model.engine, ElboEngine64) and len(ls) >= 2 and ls[-1] < ls[0]
        means, variances = dsvgp.eval_gp(TensorDataset(Xt, Yt), model, lik, num_directions=p, minibatch_size=20, minibatch_dim=p)
        assert means.dtype == f64 and means.shape == (40 * (p + 1),) and bool(torch.isfinite(means).all()) and bool((variances > 0).all())
    finally:
        torch.set_default_dtype(prev)


def test_fp64_ciq_step_at_p17(dsvgp, gpu_device):
    """one CIQ step (use_ciq=True under a float64 default) with 17 directions per point: finite loss and gradients"""
    from dsvgp_amd._step64 import ElboEngine64
    from test_ngd import make_ngd_problem
    P, x, y, D, nd = make_ngd_problem(300, 24, 8, 17, 20, seed=402, dtype=f64)
    P["natural_mat"] = 0.5 * (P["natural_mat"] + P["natural_mat"].t())
    eng = ElboEngine64(gpu_device)
    eng.whitening = "ciq"
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    loss, grads, mu, varn = eng.loss_and_grads(Pg, x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd)
    torch.cuda.synchronize()
    assert loss.dtype == f64 and bool(torch.isfinite(loss)) and bool(torch.isfinite(mu).all()) and bool((varn > 0).all())
    for k, v in grads.items():
        assert v.dtype == f64 and bool(torch.isfinite(v).all()), k
    assert grads["inducing_directions"].abs().max().item() > 0.0


def test_tiled_entries_refuse_what_they_do_not_take(dsvgp, gpu_device):
    ops = dsvgp._ops
    n, d, p = 3, 8, 20
    g, x1, x2, v1, v2, ell, s = _random_inputs(n, n, d, p)
    ctx, hyp, p1, p2 = _packs(dsvgp, gpu_device, x1, x2, v1, v2, ell, s)
    q = p + 1
    # p = 96: the packs of the supported geometry stand in, the entries must refuse before touching them
    big = torch.zeros(n * 97, n * 97, dtype=f64, device=gpu_device)
    with pytest.raises(dsvgp._lib.DsvgpError):
        ops.kernel_fwd_f64_tiled(ctx, p1, n, p2, n, d, 96, hyp, out=big)
    dx, dv, d_hyp = (torch.zeros(n, d, dtype=f64, device=gpu_device), torch.zeros(n * 96, d, dtype=f64, device=gpu_device),
                     torch.zeros(4, dtype=f64, device=gpu_device))
    with pytest.raises(dsvgp._lib.DsvgpError):
        ops.kernel_bwd_f64_tiled(ctx, big, p1, n, p2, n, d, 96, hyp, False, dx, dv, d_hyp)
    # ld < n2 q: a column slice with the rows packed closer than n2 q cannot be expressed by a tensor; call the C entries
    lib, _ptr = dsvgp._lib.lib, ops._ptr
    out = torch.zeros(n * q, n * q, dtype=f64, device=gpu_device)
    rc = lib.dsvgp_kernel_fwd_f64(ctx.h, _ptr(p1[0]), _ptr(p1[1]), n, _ptr(p2[0]), _ptr(p2[1]), n, d, p, _ptr(hyp), 0.0, 0,
                                  _ptr(out), n * q - 1)
    assert rc == EINVAL
    with pytest.raises(dsvgp._lib.DsvgpError):
        ops.check(rc, "dsvgp_kernel_fwd_f64")
    ws = torch.zeros(int(lib.dsvgp_kernel_bwd_f64_workspace_bytes(n, n, d, p)), dtype=torch.uint8, device=gpu_device)
    dv = torch.zeros(n * p, d, dtype=f64, device=gpu_device)
    rc = lib.dsvgp_kernel_bwd_f64(ctx.h, _ptr(out), n * q - 1, _ptr(p1[0]), _ptr(p1[1]), _ptr(p1[2]), n, _ptr(p2[0]), _ptr(p2[1]), n,
                                  d, p, _ptr(hyp), 0, _ptr(dx), _ptr(dv), _ptr(d_hyp), _ptr(ws), ws.numel())
    assert rc == EINVAL
    # a workspace that is too small
    rc = lib.dsvgp_kernel_bwd_f64(ctx.h, _ptr(out), n * q, _ptr(p1[0]), _ptr(p1[1]), _ptr(p1[2]), n, _ptr(p2[0]), _ptr(p2[1]), n,
                                  d, p, _ptr(hyp), 0, _ptr(dx), _ptr(dv), _ptr(d_hyp), _ptr(ws), ws.numel() - 8)
    assert rc == EINVAL
    assert float(dx.abs().max()) == 0.0 and float(d_hyp.abs().max()) == 0.0
