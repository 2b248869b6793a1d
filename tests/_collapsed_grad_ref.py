"""The float64 yardstick of the collapsed bound's gradients: the collapsed loss

    l_c(theta) = loss(m*(theta), L_S*(theta); theta)

as a differentiable function of the raw parameters -- ``_collapsed_ref.whitened``'s construction without the ``detach``, then
``_collapsed_ref.optimum`` and ``_collapsed_ref.loss`` -- with its gradients by autograd, and the closed forms the HIP path computes, as
plain functions.  RBF, ARD and Matern-5/2 through tests/_ard_yardstick.py and tests/_matern_yardstick.py.

Closed forms (envelope theorem: at the optimum only the expected log-likelihood term depends on theta).  With K~ = s K_ZZ + 1e-3 I = L L^T,
K = s K_ZX, A = L^-1 K, r = y - c, kappa = num_data / (R noise), w = 1 / (2 R noise), alpha = L^-T m, Q = L^-T (S - I) L^-1,
rho = r - K^T alpha:

    K-bar   = 2 w (Q K - alpha rho^T)
    N       = 2 w [(S - I) G - m m^T / kappa]  =  (I - S - kappa G - m m^T) / num_data     (symmetric at the optimum)
    K~-bar  = -1/2 L^-T N L^-1  =  (Q + alpha alpha^T + kappa L^-T G L^-1) / (2 num_data)
    dg-bar  = w       c-bar = -2 w sum rho       d l_c / d noise = -(E + V) / (2 R noise^2) + 1 / noise"""
import torch

import dsvgp_oracle as O
import _collapsed_ref as R
from _ard_yardstick import ard_kernel
from _matern_yardstick import radial_kernel, radial_prior_diag

GRAD_NAMES = ("raw_lengthscale", "raw_outputscale", "raw_noise", "constant", "inducing_points", "inducing_directions")


def kernel_matrices(P, x, D, kernel="rbf"):
    """(K~ = s K_ZZ + 1e-3 I, K = s K_ZX [M', B (pd + 1)], prior diagonal [B (pd + 1)] without jitter, noise): ``_collapsed_ref.whitened``'s
    routes, differentiable in the float64 parameters ``P``"""
    Z, V = P["inducing_points"], P["inducing_directions"]
    M, B = Z.shape[0], x.shape[0]
    p = V.shape[0] // M
    pd = 0 if D is None or D.numel() == 0 else D.shape[0] // B
    D = x.new_zeros(0, x.shape[1]) if pd == 0 else D
    ell, s, noise, family = R._pieces(P, kernel)
    plain = kernel == "rbf" and P["raw_lengthscale"].numel() == 1
    if plain:
        K_ZZ = s * O.kernel_matrix(Z, Z, V, V, ell[0])
    else:
        K_ZZ = s * radial_kernel(Z, V, p, Z, V, p, ell, family)
    Kt = K_ZZ + O.KZZ_JITTER * torch.eye(K_ZZ.shape[0], dtype=torch.float64)
    if plain and pd == p:
        K = s * O.kernel_matrix(Z, x, V, D, ell[0])
    elif plain:
        K = s * ard_kernel(Z, V, p, x, D, pd, ell)
    else:
        K = s * radial_kernel(Z, V, p, x, D, pd, ell, family)
    dg = s * radial_prior_diag(D, B, pd, ell, family)
    return Kt, K, dg, noise


def statistics_from(Kt, K, r, dg, noise):
    """the sufficient statistics as differentiable functions of the matrices (``_collapsed_ref.statistics``'s dict, without absG)"""
    L = O.psd_safe_cholesky(Kt)
    A = torch.linalg.solve_triangular(L, K, upper=False)
    return {"G": A @ A.t(), "b": A @ r, "yy": (r * r).sum(), "dg": dg.sum(), "R": float(r.numel()), "noise": noise}


def collapsed_loss_from(Kt, K, y, c, dg, noise, num_data, optimum=None):
    """l_c from the matrices; ``optimum`` = (m, L_S) evaluates the loss at that fixed q(u) instead (the envelope's right-hand side)"""
    stats = statistics_from(Kt, K, y - c, dg, noise)
    m, L_S = R.optimum(stats, num_data=num_data)[:2] if optimum is None else optimum
    return R.loss(stats, m, L_S, num_data=num_data), stats, m, L_S


def _leaves(P, names=GRAD_NAMES):
    Q = {k: v.detach().double().clone() for k, v in P.items()}
    for k in names:
        Q[k].requires_grad_(True)
    return Q


def collapsed_loss_and_grads(P, x, y, D, num_data, kernel="rbf", at_fixed_optimum=False):
    """(loss, {name: gradient}, m*, L_S*) in float64 by autograd through L, A, the statistics, ``optimum`` and ``loss``.
    ``at_fixed_optimum``: the gradient of ``_collapsed_ref.loss`` at the DETACHED optimum instead -- equal, by the envelope theorem."""
    Q = _leaves(P)
    x, y = x.double(), y.double()
    D = None if D is None else D.double()
    Kt, K, dg, noise = kernel_matrices(Q, x, D, kernel)
    c = Q["constant"].reshape(())
    fixed = None
    if at_fixed_optimum:
        with torch.no_grad():
            fixed = R.optimum(statistics_from(Kt, K, y - c, dg, noise), num_data=num_data)[:2]
    loss, _, m, L_S = collapsed_loss_from(Kt, K, y, c, dg, noise, num_data, optimum=fixed)
    grads = torch.autograd.grad(loss, [Q[k] for k in GRAD_NAMES], allow_unused=True)
    grads = {k: (torch.zeros_like(Q[k]) if g is None else g) for k, g in zip(GRAD_NAMES, grads)}
    return loss.detach(), grads, m.detach(), L_S.detach()


def collapsed_loss_and_grads_union(P, sets, num_data, kernel="rbf"):
    """``collapsed_loss_and_grads`` for the union of several data sets ``(x, y, D)`` with their own numbers of directions: the columns of
    K, the targets and the prior diagonals side by side"""
    Q = _leaves(P)
    Ks, ys, dgs = [], [], []
    for x, y, D in sets:
        Kt, K, dg, noise = kernel_matrices(Q, x.double(), None if D is None else D.double(), kernel)
        Ks.append(K), ys.append(y.double()), dgs.append(dg)
    loss, _, m, L_S = collapsed_loss_from(Kt, torch.cat(Ks, dim=1), torch.cat(ys), Q["constant"].reshape(()), torch.cat(dgs), noise, num_data)
    grads = torch.autograd.grad(loss, [Q[k] for k in GRAD_NAMES], allow_unused=True)
    grads = {k: (torch.zeros_like(Q[k]) if g is None else g) for k, g in zip(GRAD_NAMES, grads)}
    return loss.detach(), grads, m.detach(), L_S.detach()


def matrix_adjoints_autograd(P, x, y, D, num_data, kernel="rbf"):
    """autograd gradients of l_c with respect to the intermediate leaves: dict of Kbar [M', B'], Ktbar [M', M'] (symmetric: the factor's
    backward returns the symmetrised gradient), cbar, dgbar [B'], dnoise"""
    with torch.no_grad():
        Kt, K, dg, noise = kernel_matrices({k: v.double() for k, v in P.items()}, x.double(), None if D is None else D.double(), kernel)
    c = P["constant"].double().reshape(())
    leaves = [t.clone().requires_grad_(True) for t in (Kt, K, c, dg, noise)]
    loss = collapsed_loss_from(leaves[0], leaves[1], y.double(), leaves[2], leaves[3], leaves[4], num_data)[0]
    g = torch.autograd.grad(loss, leaves)
    return {"Ktbar": 0.5 * (g[0] + g[0].t()), "Kbar": g[1], "cbar": g[2], "dgbar": g[3], "dnoise": g[4], "loss": loss.detach()}


def closed_forms(P, x, y, D, num_data, kernel="rbf"):
    """the closed forms of the module docstring in float64, as a dict (plus the pieces the per-chunk form needs: Q, alpha, w, K, r)"""
    with torch.no_grad():
        Kt, K, dg, noise = kernel_matrices({k: v.double() for k, v in P.items()}, x.double(), None if D is None else D.double(), kernel)
        r = y.double() - P["constant"].double().reshape(())
        stats = statistics_from(Kt, K, r, dg, noise)
        m, L_S = R.optimum(stats, num_data=num_data)[:2]
        n, Rr, G = m.shape[0], stats["R"], stats["G"]
        eye = torch.eye(n, dtype=torch.float64)
        L = O.psd_safe_cholesky(Kt)
        Linv = torch.linalg.solve_triangular(L, eye, upper=False)
        S = L_S @ L_S.t()
        kappa, w = num_data / (Rr * noise), 1.0 / (2.0 * Rr * noise)
        alpha = Linv.t() @ m
        Q = Linv.t() @ (S - eye) @ Linv
        rho = r - K.t() @ alpha
        N_product = 2.0 * w * ((S - eye) @ G - torch.outer(m, m) / kappa)
        N_free = (eye - S - kappa * G - torch.outer(m, m)) / num_data
        A = Linv @ K
        E = ((r - A.t() @ m) ** 2).sum()
        V = stats["dg"] + Rr * O.KXX_JITTER + (S * G).sum() - torch.trace(G) + Rr * noise
        return {"Kbar": kbar_chunk(Q, alpha, w, K, r), "Ktbar": (Q + torch.outer(alpha, alpha) + kappa * Linv.t() @ G @ Linv) / (2.0 * num_data),
                "Ktbar_from_N": -0.5 * Linv.t() @ N_product @ Linv, "N_product": N_product, "N_free": N_free,
                "cbar": -2.0 * w * rho.sum(), "dgbar": w * torch.ones_like(dg), "dnoise": -(E + V) / (2.0 * Rr * noise ** 2) + 1.0 / noise,
                "Q": Q, "alpha": alpha, "w": w, "K": K, "r": r, "loss": R.loss(stats, m, L_S, num_data=num_data)}


def kbar_chunk(Q, alpha, w, K, r):
    """K-bar of the columns ``K`` [M', B'] with their residual row ``r``: what one per-chunk call computes, from the GLOBAL Q, alpha, w"""
    rho = r - K.t() @ alpha
    return 2.0 * w * (Q @ K - torch.outer(alpha, rho))
