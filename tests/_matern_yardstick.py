"""The float64 yardstick of a radial kernel family with directional derivatives on ARD-scaled inputs: differentiable torch, written from
the closed form and independent of the HIP code.

A family is a function nn -> (f0, f1, f2) with f_{m+1} = -2 d f_m / d nn, nn = |r|^2, r = (x1_i - x2_j) ./ ell.  With
v~_a = (v_a / |v_a|) ./ ell, u~_a = r . v~1_ia, w~_b = r . v~2_jb, micro-block (i, j) of the kernel is

    [[f0, f1 w~_b], [-f1 u~_a, f1 v~1_a . v~2_b - f2 u~_a w~_b]]

``rbf_family`` (f0 = f1 = f2 = exp(-nn/2)) gives ``ard_kernel`` of tests/_ard_yardstick.py, ``matern52_family`` the Matern-5/2 kernel
(1 + a + a^2/3) exp(-a), a = sqrt(5 nn) (tests/test_matern_host.py checks both).  ``matern_elbo`` / ``matern_predictive`` have the
structure of ``ard_elbo`` / ``ard_predictive``; the prior diagonal is [1, f1(0) |v~|^2]; Cholesky, KL and constants are the oracle's."""
import math

import torch

import dsvgp_oracle as O
from _ard_yardstick import ard_constrained, ard_scaled


def rbf_family(nn):
    k = torch.exp(-0.5 * nn)
    return k, k, k


def matern52_family(nn):
    a = torch.sqrt(5.0 * nn + 1e-300)           # (safe at nn = 0: value and gradient finite)
    e = torch.exp(-a)
    return (1.0 + a + a * a / 3.0) * e, (5.0 / 3.0) * (1.0 + a) * e, (25.0 / 3.0) * e


def family_f1_at_zero(family):
    return family(torch.zeros((), dtype=torch.float64))[1]


def radial_kernel(x1, v1, p1, x2, v2, p2, ell_vec, family):
    """K(x1, x2; v1, v2) [n1 (p1 + 1), n2 (p2 + 1)], interleaved as ``O.kernel_matrix``; outputscale 1"""
    n1, n2 = x1.shape[0], x2.shape[0]
    ell_vec = ell_vec.reshape(-1)
    V1, V2 = ard_scaled(v1, n1, p1, ell_vec), ard_scaled(v2, n2, p2, ell_vec)
    r = (x1[:, None, :] - x2[None, :, :]) / ell_vec
    f0, f1, f2 = family((r * r).sum(-1))                             # [i, j]
    u = torch.einsum("ijd,iad->iaj", r, V1)                         # [i, a, j]
    w = torch.einsum("ijd,jbd->ijb", r, V2)                         # [i, j, b]
    T = torch.einsum("iad,jbd->iajb", V1, V2)
    top = torch.cat([f0[:, None, :, None], (w * f1[..., None])[:, None, :, :]], dim=3)                      # [i, 1, j, q2]
    low = torch.cat([(-u * f1[:, None, :])[..., None],
                     T * f1[:, None, :, None] - u[..., None] * w[:, None, :, :] * f2[:, None, :, None]], dim=3)
    return torch.cat([top, low], dim=1).reshape(n1 * (p1 + 1), n2 * (p2 + 1))


def radial_prior_diag(D, B, pd, ell_vec, family):
    """diag K(x, D; x, D) / s = [1, f1(0) |v~_1|^2, ..., f1(0) |v~_pd|^2] per point"""
    V = ard_scaled(D, B, pd, ell_vec.reshape(-1))
    return torch.cat([ell_vec.new_ones(B, 1), family_f1_at_zero(family).to(ell_vec) * (V * V).sum(-1)], dim=1).reshape(-1)


def matern_kernel(x1, v1, p1, x2, v2, p2, ell_vec, family=matern52_family):
    return radial_kernel(x1, v1, p1, x2, v2, p2, ell_vec, family)


def matern_prior_diag(D, B, pd, ell_vec, family=matern52_family):
    return radial_prior_diag(D, B, pd, ell_vec, family)


def _ell(P, d):
    """(ell [d], s, noise): a scalar raw_lengthscale is d equal lengthscales (expand keeps the gradient summed into the scalar)"""
    ell, s, noise = ard_constrained(P)
    return (ell.expand(d) if ell.numel() == 1 else ell), s, noise


def matern_forward(P, x, y, D, pd, num_data, mll, family=matern52_family):
    """(loss, mu, varn) of one minibatch objective; P["raw_lengthscale"] is [1, d] or [1, 1].  Differentiable."""
    Z, V, m = P["inducing_points"], P["inducing_directions"], P["variational_mean"]
    L_S = torch.tril(P["chol_variational_covar"])
    c = P["constant"].reshape(())
    ell, s, noise = _ell(P, Z.shape[1])
    M, B = Z.shape[0], x.shape[0]
    p = V.shape[0] // M
    K_ZZ = s * radial_kernel(Z, V, p, Z, V, p, ell, family)
    L = O.psd_safe_cholesky(K_ZZ + O.KZZ_JITTER * torch.eye(K_ZZ.shape[0], dtype=K_ZZ.dtype))
    K_ZX = s * radial_kernel(Z, V, p, x, D, pd, ell, family)
    A = torch.linalg.solve_triangular(L, K_ZX, upper=False)
    mu = A.t() @ m + c
    SA = L_S @ (L_S.t() @ A) - A
    var = s * radial_prior_diag(D, B, pd, ell, family) + O.KXX_JITTER + (A * SA).sum(0)
    varn = (var + noise).clamp_min(O.MIN_VARIANCE)
    if mll == "ELBO":
        ll = -0.5 * (((y - mu) ** 2 + varn) / noise + torch.log(noise) + math.log(2 * math.pi))
    elif mll == "PLL":
        tot = (varn + noise).clamp_min(1e-8)
        ll = -0.5 * ((y - mu) ** 2 / tot + torch.log(tot) + math.log(2 * math.pi))
    else:
        raise ValueError(mll)
    loss = -(ll.sum() / y.shape[0] - O.kl_whitened(m, L_S) / num_data)
    return loss, mu, varn


def matern_elbo(P64, x, y, D, pd, num_data, mll, family=matern52_family):
    """(loss, grads, mu, varn) in float64, gradients by autograd"""
    ps = {k: v.detach().clone().requires_grad_(True) for k, v in P64.items()}
    loss, mu, varn = matern_forward(ps, x, y, D, pd, num_data, mll, family)
    loss.backward()
    grads = {k: (ps[k].grad if ps[k].grad is not None else torch.zeros_like(ps[k])) for k in ps}
    return loss.detach(), grads, mu.detach(), varn.detach()


def matern_predictive(P64, x, D, pd, family=matern52_family):
    """(mu, Sigma) of q(f) over the B (pd + 1) outputs, no likelihood noise"""
    Z, V, m = P64["inducing_points"], P64["inducing_directions"], P64["variational_mean"]
    L_S = torch.tril(P64["chol_variational_covar"])
    c = P64["constant"].reshape(())
    ell, s, _ = _ell(P64, Z.shape[1])
    p = V.shape[0] // Z.shape[0]
    K_ZZ = s * radial_kernel(Z, V, p, Z, V, p, ell, family)
    L = O.psd_safe_cholesky(K_ZZ + O.KZZ_JITTER * torch.eye(K_ZZ.shape[0], dtype=K_ZZ.dtype))
    K_ZX = s * radial_kernel(Z, V, p, x, D, pd, ell, family)
    K_XX = s * radial_kernel(x, D, pd, x, D, pd, ell, family) + O.KXX_JITTER * torch.eye(x.shape[0] * (pd + 1), dtype=x.dtype)
    A = torch.linalg.solve_triangular(L, K_ZX, upper=False)
    W = L_S.t() @ A
    return A.t() @ m + c, K_XX + W.t() @ W - A.t() @ A
