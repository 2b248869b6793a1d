"""CPU: the float64 radial-family yardstick (tests/_matern_yardstick.py) pinned to what it must equal -- with the RBF family the ARD
yardstick of tests/_ard_yardstick.py, with the Matern-5/2 family directional derivatives of s (1 + a + a^2/3) exp(-a) taken by autograd --
and its behaviour at distance zero, where a = sqrt(5 nn) has a cusp."""
import math

import pytest
import torch

import dsvgp_oracle as O
from _ard_yardstick import ard_elbo, ard_kernel, ard_lengthscales, ard_predictive
from _matern_yardstick import matern52_family, matern_elbo, matern_kernel, matern_predictive, matern_prior_diag, radial_kernel, rbf_family
from test_gpu_rect_train import relmax

f64 = torch.float64


# ---- (a) the RBF family reproduces the ARD yardstick ----------------------------------------------------------------------------
@pytest.mark.parametrize("n1,p1,n2,p2,d", [(5, 2, 7, 3, 4), (4, 0, 6, 2, 3), (6, 3, 5, 0, 5), (4, 2, 4, 2, 3)])
def test_rbf_family_gives_the_ard_kernel(n1, p1, n2, p2, d):
    g = torch.Generator().manual_seed(3 + n1 + d)
    x1, x2 = torch.rand(n1, d, generator=g, dtype=f64), torch.rand(n2, d, generator=g, dtype=f64)
    v1, v2 = torch.randn(n1 * p1, d, generator=g, dtype=f64), torch.randn(n2 * p2, d, generator=g, dtype=f64)
    ell = ard_lengthscales(d)
    K = radial_kernel(x1, v1, p1, x2, v2, p2, ell, rbf_family)
    assert K.shape == (n1 * (p1 + 1), n2 * (p2 + 1))
    assert relmax(K, ard_kernel(x1, v1, p1, x2, v2, p2, ell)) <= 1e-12


def _ard_problem(pd):
    from test_gpu_step import make_problem
    N, d, M, p, B = 400, 3, 16, 2, 96
    P, x, _, _, nd = make_problem(N, d, M, p, B, seed=11)
    g = torch.Generator().manual_seed(5 + pd)
    y = torch.randn(B * (pd + 1), generator=g, dtype=f64)
    D = torch.randn(B * pd, d, generator=g, dtype=f64)
    P64 = {k: v.double() for k, v in P.items()}
    P64["raw_lengthscale"] = torch.log(torch.expm1(ard_lengthscales(d))).reshape(1, d)
    return P64, x.double(), y, D, nd


@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
@pytest.mark.parametrize("pd", [0, 2, 3])
def test_rbf_family_gives_the_ard_objective_and_predictions(mll, pd):
    P64, x, y, D, nd = _ard_problem(pd)
    ref = ard_elbo(P64, x, y, D, pd, nd, mll)
    mine = matern_elbo(P64, x, y, D, pd, nd, mll, family=rbf_family)
    assert abs(mine[0].item() - ref[0].item()) <= 1e-12 * abs(ref[0].item())
    assert relmax(mine[2], ref[2]) <= 1e-12 and relmax(mine[3], ref[3]) <= 1e-12
    for k in O.PARAM_NAMES:
        assert relmax(mine[1][k], ref[1][k]) <= 1e-12, k
    if mll == "ELBO":
        mu, Sigma = matern_predictive(P64, x, D, pd, family=rbf_family)
        mu_ref, Sigma_ref = ard_predictive(P64, x, D, pd)
        assert relmax(mu, mu_ref) <= 1e-12 and relmax(Sigma, Sigma_ref) <= 1e-12


def test_a_scalar_lengthscale_is_d_equal_ones_and_its_gradient_their_sum():
    P64, x, y, D, nd = _ard_problem(2)
    d = x.shape[1]
    Ps = dict(P64, raw_lengthscale=torch.tensor([[0.3]], dtype=f64))
    Pv = dict(P64, raw_lengthscale=torch.full((1, d), 0.3, dtype=f64))
    a, b = matern_elbo(Ps, x, y, D, 2, nd, "ELBO"), matern_elbo(Pv, x, y, D, 2, nd, "ELBO")
    assert a[0].item() == b[0].item() and a[1]["raw_lengthscale"].shape == (1, 1)
    assert abs(a[1]["raw_lengthscale"].item() - b[1]["raw_lengthscale"].sum().item()) <= 1e-12 * abs(a[1]["raw_lengthscale"].item())


# ---- (b) the Matern family: every block entry is a directional derivative of the scalar function --------------------------------
def test_every_block_is_a_directional_derivative_of_the_matern52_function():
    n, d, p = 3, 3, 2
    g = torch.Generator().manual_seed(0)
    x, z = torch.rand(n, d, generator=g, dtype=f64), torch.rand(n, d, generator=g, dtype=f64)
    vx, vz = torch.randn(n * p, d, generator=g, dtype=f64), torch.randn(n * p, d, generator=g, dtype=f64)
    ell = torch.tensor([0.3, 0.8, 1.7], dtype=f64)
    s = 1.3
    K = s * matern_kernel(x, vx, p, z, vz, p, ell).reshape(n, p + 1, n, p + 1)
    ux, uz = O.normalize_rows(vx).reshape(n, p, d), O.normalize_rows(vz).reshape(n, p, d)
    worst = 0.0
    for i in range(n):
        for j in range(n):
            xi, zj = x[i].clone().requires_grad_(True), z[j].clone().requires_grad_(True)
            a = torch.sqrt(5.0 * (((xi - zj) / ell) ** 2).sum())
            k = s * (1.0 + a + a * a / 3.0) * torch.exp(-a)
            gx, gz = torch.autograd.grad(k, (xi, zj), create_graph=True)
            want = torch.zeros(p + 1, p + 1, dtype=f64)
            want[0, 0] = k.detach()
            for b in range(p):
                want[0, 1 + b] = (gz @ uz[j, b]).detach()
            for a_ in range(p):
                da = gx @ ux[i, a_]
                want[1 + a_, 0] = da.detach()
                hz, = torch.autograd.grad(da, zj, retain_graph=True)
                for b in range(p):
                    want[1 + a_, 1 + b] = hz @ uz[j, b]
            worst = max(worst, (K[i, :, j, :] - want).abs().max().item())
    print("[parity] matern_kernel vs autograd of s (1 + a + a^2/3) exp(-a): %.2e" % worst)
    assert worst <= 1e-10 * max(1.0, K.abs().max().item())
    assert math.isfinite(worst)


def test_the_family_obeys_its_recurrence():
    """f_{m+1} = -2 d f_m / d nn, by autograd at generic nn"""
    nn = torch.tensor([0.01, 0.3, 1.7, 9.0], dtype=f64, requires_grad=True)
    f0, f1, f2 = matern52_family(nn)
    d0, = torch.autograd.grad(f0.sum(), nn, retain_graph=True)
    d1, = torch.autograd.grad(f1.sum(), nn, retain_graph=True)
    assert relmax(-2 * d0, f1.detach()) <= 1e-12 and relmax(-2 * d1, f2.detach()) <= 1e-12


# ---- (c) distance zero ----------------------------------------------------------------------------------------------------------
def test_at_coincident_points_the_block_is_the_prior_block_and_gradients_are_finite():
    n, d, p = 4, 3, 2
    g = torch.Generator().manual_seed(2)
    x = torch.rand(n, d, generator=g, dtype=f64)
    v1, v2 = torch.randn(n * p, d, generator=g, dtype=f64), torch.randn(n * p, d, generator=g, dtype=f64)
    ell = torch.tensor([0.4, 0.9, 1.5], dtype=f64)
    s = 1.3
    x1, x2 = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    v1r, v2r, ellr = v1.clone().requires_grad_(True), v2.clone().requires_grad_(True), ell.clone().requires_grad_(True)
    K = s * matern_kernel(x1, v1r, p, x2, v2r, p, ellr)
    Kb = K.reshape(n, p + 1, n, p + 1)
    t1, t2 = O.normalize_rows(v1).reshape(n, p, d) / ell, O.normalize_rows(v2).reshape(n, p, d) / ell
    for i in range(n):
        blk = Kb[i, :, i, :].detach()
        want = torch.zeros(p + 1, p + 1, dtype=f64)
        want[0, 0] = s
        want[1:, 1:] = s * (5.0 / 3.0) * t1[i] @ t2[i].t()
        assert (blk - want).abs().max().item() <= 1e-14, i
    G = torch.randn(K.shape, generator=g, dtype=f64)
    grads = torch.autograd.grad((K * G).sum(), (x1, x2, v1r, v2r, ellr))
    assert all(bool(torch.isfinite(t).all()) for t in grads)
    diag = s * matern_prior_diag(v1, n, p, ell)
    Kd = (s * matern_kernel(x, v1, p, x, v1, p, ell)).diagonal()
    assert relmax(diag, Kd) <= 1e-14


# ---- (d) K_ZZ at the GPU test shapes is positive definite with the engine's jitter ----------------------------------------------
def _gpu_step_shapes():
    from test_gpu_ard import STEPS, STEP_IDS
    return [pytest.param(s, id=i) for s, i in zip(STEPS, STEP_IDS)]


@pytest.mark.parametrize("shape", _gpu_step_shapes())
def test_kzz_is_positive_definite_at_the_gpu_step_shapes(shape):
    """the inducing sets, lengthscales and outputscale of the step / prediction tests of tests/test_gpu_matern.py (``_problem`` of
    tests/test_gpu_ard.py), and with a scalar lengthscale as well"""
    from test_gpu_ard import _problem
    N, d, M, p, pd, B = shape
    P = _problem(*shape)[0]
    Z, V = P["inducing_points"].double(), P["inducing_directions"].double()
    s = torch.nn.functional.softplus(P["raw_outputscale"].double()).reshape(())
    ell = torch.nn.functional.softplus(P["raw_lengthscale"].double()).reshape(-1)
    assert relmax(ell, ard_lengthscales(d)) < 1e-6
    Ks = s * matern_kernel(Z, V, p, Z, V, p, torch.nn.functional.softplus(torch.full((d,), 0.3, dtype=f64)))
    assert torch.linalg.eigvalsh(Ks + O.KZZ_JITTER * torch.eye(M * (p + 1), dtype=f64))[0].item() >= 0.5 * O.KZZ_JITTER
    K = s * matern_kernel(Z, V, p, Z, V, p, ell) + O.KZZ_JITTER * torch.eye(M * (p + 1), dtype=f64)
    assert relmax(K, K.t()) <= 1e-14
    lam = torch.linalg.eigvalsh(K)
    print("[parity] Matern K_ZZ + jitter d=%d M=%d p=%d: eigenvalues in [%.3e, %.3e]" % (d, M, p, lam[0].item(), lam[-1].item()))
    assert lam[0].item() >= 0.5 * O.KZZ_JITTER
    torch.linalg.cholesky(K)
