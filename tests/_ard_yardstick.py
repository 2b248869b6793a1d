"""The float64 yardstick of the ARD kernel (one lengthscale per input dimension): differentiable torch, written from the closed form and
independent of the HIP code.

With x~ = x ./ ell, v~_a = (v_a / |v_a|) ./ ell (elementwise, ell in R^d) and r = x~1_i - x~2_j, micro-block (i, j) of the kernel is

    k [[1, w~_b], [-u~_a, v~1_a . v~2_b - u~_a w~_b]],    k = exp(-|r|^2 / 2),  u~_a = r . v~1_ia,  w~_b = r . v~2_jb

which is what differentiating exp(-sum_k ((x - z)_k / ell_k)^2 / 2) along the unit directions gives (tests/test_ard_host.py checks that
by autograd).  ``ard_forward`` / ``ard_elbo`` are ``rect_forward`` / ``rect_elbo`` of tests/test_gpu_rect_train.py with this kernel and
the prior diagonal s [1, |v~|^2]; Cholesky, KL and constants are the oracle's."""
import math

import torch
import torch.nn.functional as F

import dsvgp_oracle as O


def ard_scaled(v, n, p, ell_vec):
    """v~ [n, p, d]: the normalised directions divided elementwise by the lengthscales"""
    d = ell_vec.shape[0]
    if p == 0:
        return ell_vec.new_zeros(n, 0, d)
    return (O.normalize_rows(v) / ell_vec).reshape(n, p, d)


def ard_kernel(x1, v1, p1, x2, v2, p2, ell_vec):
    """K(x1, x2; v1, v2) [n1 (p1 + 1), n2 (p2 + 1)], interleaved as ``O.kernel_matrix``; outputscale 1"""
    n1, n2 = x1.shape[0], x2.shape[0]
    ell_vec = ell_vec.reshape(-1)
    V1, V2 = ard_scaled(v1, n1, p1, ell_vec), ard_scaled(v2, n2, p2, ell_vec)
    r = (x1[:, None, :] - x2[None, :, :]) / ell_vec
    k = torch.exp(-0.5 * (r * r).sum(-1))                           # [i, j]
    u = torch.einsum("ijd,iad->iaj", r, V1)                         # [i, a, j]
    w = torch.einsum("ijd,jbd->ijb", r, V2)                         # [i, j, b]
    T = torch.einsum("iad,jbd->iajb", V1, V2)
    top = torch.cat([k[:, None, :, None], (w * k[..., None])[:, None, :, :]], dim=3)                       # [i, 1, j, q2]
    low = torch.cat([(-u * k[:, None, :])[..., None], (T - u[..., None] * w[:, None, :, :]) * k[:, None, :, None]], dim=3)
    return torch.cat([top, low], dim=1).reshape(n1 * (p1 + 1), n2 * (p2 + 1))


def ard_prior_diag(D, B, pd, ell_vec):
    """diag K(x, D; x, D) / s = [1, |v~_1|^2, ..., |v~_pd|^2] per point"""
    V = ard_scaled(D, B, pd, ell_vec.reshape(-1))
    return torch.cat([ell_vec.new_ones(B, 1), (V * V).sum(-1)], dim=1).reshape(-1)


def ard_constrained(P):
    ell = F.softplus(P["raw_lengthscale"]).reshape(-1)
    s = F.softplus(P["raw_outputscale"]).reshape(())
    noise = F.softplus(P["raw_noise"]).reshape(()) + O.NOISE_FLOOR
    return ell, s, noise


def ard_forward(P, x, y, D, pd, num_data, mll):
    """(loss, mu, varn) of one minibatch objective; P["raw_lengthscale"] is [1, d].  Differentiable."""
    Z, V, m = P["inducing_points"], P["inducing_directions"], P["variational_mean"]
    L_S = torch.tril(P["chol_variational_covar"])
    c = P["constant"].reshape(())
    ell, s, noise = ard_constrained(P)
    M, B = Z.shape[0], x.shape[0]
    p = V.shape[0] // M
    K_ZZ = s * ard_kernel(Z, V, p, Z, V, p, ell)
    L = O.psd_safe_cholesky(K_ZZ + O.KZZ_JITTER * torch.eye(K_ZZ.shape[0], dtype=K_ZZ.dtype))
    K_ZX = s * ard_kernel(Z, V, p, x, D, pd, ell)
    A = torch.linalg.solve_triangular(L, K_ZX, upper=False)
    mu = A.t() @ m + c
    SA = L_S @ (L_S.t() @ A) - A
    var = s * ard_prior_diag(D, B, pd, ell) + O.KXX_JITTER + (A * SA).sum(0)
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


def ard_elbo(P64, x, y, D, pd, num_data, mll):
    """(loss, grads, mu, varn) in float64, gradients by autograd"""
    ps = {k: v.detach().clone().requires_grad_(True) for k, v in P64.items()}
    loss, mu, varn = ard_forward(ps, x, y, D, pd, num_data, mll)
    loss.backward()
    grads = {k: (ps[k].grad if ps[k].grad is not None else torch.zeros_like(ps[k])) for k in ps}
    return loss.detach(), grads, mu.detach(), varn.detach()


def ard_predictive(P64, x, D, pd):
    """(mu, Sigma) of q(f) over the B (pd + 1) outputs, no likelihood noise (``rect_predictive`` of tests/test_gpu_rect_predict.py)"""
    Z, V, m = P64["inducing_points"], P64["inducing_directions"], P64["variational_mean"]
    L_S = torch.tril(P64["chol_variational_covar"])
    c = P64["constant"].reshape(())
    ell, s, _ = ard_constrained(P64)
    p = V.shape[0] // Z.shape[0]
    K_ZZ = s * ard_kernel(Z, V, p, Z, V, p, ell)
    L = O.psd_safe_cholesky(K_ZZ + O.KZZ_JITTER * torch.eye(K_ZZ.shape[0], dtype=K_ZZ.dtype))
    K_ZX = s * ard_kernel(Z, V, p, x, D, pd, ell)
    K_XX = s * ard_kernel(x, D, pd, x, D, pd, ell) + O.KXX_JITTER * torch.eye(x.shape[0] * (pd + 1), dtype=x.dtype)
    A = torch.linalg.solve_triangular(L, K_ZX, upper=False)
    W = L_S.t() @ A
    return A.t() @ m + c, K_XX + W.t() @ W - A.t() @ A


def ard_lengthscales(d, dtype=torch.float64):
    """ell_k = 0.4 sqrt(d) (0.5 + k / (d - 1)): a 3x spread across the dimensions, so every d_ell[k] is distinct"""
    return 0.4 * math.sqrt(d) * (0.5 + torch.arange(d, dtype=dtype) / max(d - 1, 1))
