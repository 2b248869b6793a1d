"""The float64 CPU reference of the closed-form optimal q(u) (Titsias 2009) and of the ELBO evaluated from one-pass statistics, written on
the oracle's pieces (``kernel_matrix``, ``psd_safe_cholesky``, ``constrained``, ``kl_whitened``) and, for ARD / Matern-5/2 and for data with
another number of directions than the model, on the yardstick kernels of tests/_ard_yardstick.py and tests/_matern_yardstick.py.

With A = L^-1 K_ZX (L = chol(K_ZZ + 1e-3 I)), r = y - c, R rows, tau = num_data / R and kappa = tau / noise:

    G = A A^T,  b = A r,  yy = r^T r,  dg = sum of the prior diagonal
    B = I + kappa G,   S* = B^-1,   m* = kappa B^-1 b,   natural_vec = kappa b,   natural_mat = -B / 2
    sum |r - A^T m|^2 = yy - 2 m^T b + m^T G m
    sum varn          = dg + R 1e-4 + <S, G> - tr G + R noise
    sum ll            = -1/2 [(sum |.|^2 + sum varn) / noise + R log noise + R log 2 pi]
    loss(m, L_S)      = -(sum ll / R - KL(m, L_S) / num_data)

which is ``O.elbo_forward`` on all R rows as one batch (tests/test_collapsed_host.py holds the two against each other)."""
import math

import torch

import dsvgp_oracle as O
from _ard_yardstick import ard_constrained, ard_kernel
from _matern_yardstick import matern52_family, radial_kernel, radial_prior_diag, rbf_family


def _pieces(params, kernel):
    """(ell [d], s, noise, family): a scalar lengthscale is d equal ones for the yardstick kernels"""
    d = params["inducing_points"].shape[1]
    ell, s, noise = ard_constrained(params)
    ell = ell.expand(d) if ell.numel() == 1 else ell
    return ell, s, noise, (matern52_family if kernel == "matern52" else rbf_family)


def whitened(params, x, D, kernel="rbf"):
    """(A [M', B (pd + 1)], prior diagonal [B (pd + 1)] without jitter, noise) in float64.  ``D`` None or empty: values only."""
    P = {k: v.detach().double() for k, v in params.items()}
    x = x.double()
    Z, V = P["inducing_points"], P["inducing_directions"]
    M, B = Z.shape[0], x.shape[0]
    p = V.shape[0] // M
    pd = 0 if D is None or D.numel() == 0 else D.shape[0] // B
    D = x.new_zeros(0, x.shape[1]) if pd == 0 else D.double()
    ell, s, noise, family = _pieces(P, kernel)
    plain = kernel == "rbf" and P["raw_lengthscale"].numel() == 1
    if plain:
        K_ZZ = s * O.kernel_matrix(Z, Z, V, V, ell[0])
    else:
        K_ZZ = s * radial_kernel(Z, V, p, Z, V, p, ell, family)
    L = O.psd_safe_cholesky(K_ZZ + O.KZZ_JITTER * torch.eye(K_ZZ.shape[0], dtype=torch.float64))
    if plain and pd == p:
        K_ZX = s * O.kernel_matrix(Z, x, V, D, ell[0])
    elif plain:
        K_ZX = s * ard_kernel(Z, V, p, x, D, pd, ell)
    else:
        K_ZX = s * radial_kernel(Z, V, p, x, D, pd, ell, family)
    A = torch.linalg.solve_triangular(L, K_ZX, upper=False)
    dg = s * radial_prior_diag(D, B, pd, ell, family)
    return A, dg, noise


def statistics(params, x, y, D, kernel="rbf"):
    """the sufficient statistics of one data set as a dict: G, b, yy, dg, R, noise (and absG = |A| |A|^T, the scale of G's rounding)"""
    A, dg, noise = whitened(params, x, D, kernel)
    r = y.double() - params["constant"].double().reshape(())
    return {"G": A @ A.t(), "b": A @ r, "yy": (r * r).sum(), "dg": dg.sum(), "R": float(r.numel()), "noise": noise,
            "absG": A.abs() @ A.abs().t()}


def merge(*stats):
    """statistics of the union of data sets (same model)"""
    out = dict(stats[0])
    for s in stats[1:]:
        for k in ("G", "b", "yy", "dg", "R", "absG"):
            out[k] = out[k] + s[k]
    return out


def _B(stats, noise, num_data):
    kappa = num_data / (stats["R"] * noise)
    n = stats["G"].shape[0]
    return torch.eye(n, dtype=torch.float64) + kappa * stats["G"], kappa


def cond_B(stats, noise=None, num_data=None):
    noise = stats["noise"] if noise is None else noise
    B, _ = _B(stats, noise, stats["R"] if num_data is None else num_data)
    ev = torch.linalg.eigvalsh(B)
    return (ev[-1] / ev[0]).item()


def optimum(stats, noise=None, num_data=None):
    """(m*, L_S*, natural_vec, natural_mat) in float64.  L_S* = chol(B^-1) comes from the factor of the flipped matrix: with the exchange
    matrix J, J B J = Lt Lt^T gives chol(B^-1) = J Lt^-T J, lower triangular with a positive diagonal -- no second factorisation."""
    noise = stats["noise"] if noise is None else noise
    num_data = stats["R"] if num_data is None else num_data
    B, kappa = _B(stats, noise, num_data)
    n = B.shape[0]
    Lt = torch.linalg.cholesky(B.flip(0, 1))
    Linv = torch.linalg.solve_triangular(Lt, torch.eye(n, dtype=torch.float64), upper=False)
    L_S = Linv.t().flip(0, 1)
    m = kappa * (L_S @ (L_S.t() @ stats["b"]))
    return m, L_S, kappa * stats["b"], -0.5 * B


def terms(stats, m, L_S, noise=None, num_data=None):
    """dict of loss, ll, kl, residual, varn for any (m, L_S)"""
    noise = stats["noise"] if noise is None else noise
    R = stats["R"]
    num_data = R if num_data is None else num_data
    m, L_S = m.double(), torch.tril(L_S.double())
    G, b = stats["G"], stats["b"]
    res = stats["yy"] - 2.0 * (m @ b) + m @ (G @ m)
    W = L_S.t() @ G @ L_S
    varn = stats["dg"] + R * O.KXX_JITTER + torch.trace(W) - torch.trace(G) + R * noise
    ll = -0.5 * ((res + varn) / noise + R * torch.log(noise) + R * math.log(2 * math.pi))
    kl = O.kl_whitened(m, L_S)
    return {"loss": -(ll / R - kl / num_data), "ll": ll, "kl": kl, "residual": res, "varn": varn}


def loss(stats, m, L_S, noise=None, num_data=None):
    return terms(stats, m, L_S, noise, num_data)["loss"]


# ------------------------------------------------------------------ the shared cases of the host and GPU tests
#      name  N    d   M  p  pd  raw_noise  num_data / R  kernel
CASES = {"a": (150, 3, 24, 2, 2, -2.0, 1.0, "rbf"),         # M' = 72: crosses one 64-tile; B' = 450 ragged
         "b": (203, 4, 43, 2, 2, -3.0, 2.5, "rbf"),         # M' = 129: one row past two tiles
         "c": (97, 5, 13, 4, 4, -4.0, 0.7, "rbf"),          # M' = 65, q = 5
         "d": (97, 5, 13, 4, 0, -4.0, 0.7, "rbf"),          # rectangular, values only
         "e": (97, 5, 13, 4, 5, -4.0, 0.7, "rbf"),          # rectangular, pd = d
         "f": (40, 100, 6, 2, 2, -3.0, 2.5, "rbf"),         # wide route (d >= 93)
         "g": (150, 3, 24, 2, 2, -2.0, 1.0, "ard"),         # case a with ARD lengthscales
         "h": (150, 3, 24, 2, 2, -2.0, 1.0, "matern52")}    # case a with Matern-5/2
HELD_OUT = 64


def problem(name):
    """(params fp32 at q(u) = (0, I), x [N, d], y [N (pd + 1)], D [N pd, d] or None, num_data, held-out points, their p directions, kernel);
    constant = 0.3, raw_lengthscale = -0.5 (ARD: -0.5 + a spread of +-0.2), unit data directions.  Deterministic in ``name``."""
    N, d, M, p, pd, raw_noise, ratio, kernel = CASES[name]
    g = torch.Generator().manual_seed(1000 + 7 * N + d)        # (cases c, d, e: the same points, inducing set and held-out set)
    X = torch.rand(N + M + HELD_OUT, d, generator=g)
    if d > 20:                                                  # (wide inputs: a cube of side 2 / sqrt(d), so that K_ZX is not ~0 at this lengthscale)
        X = X * (2.0 / math.sqrt(d))
    Z, x, xt = X[:M].clone(), X[M:M + N].contiguous(), X[M + N:].contiguous()
    V = torch.eye(d)[:p].repeat(M, 1) + 0.1 * torch.randn(M * p, d, generator=g)
    P = O.init_params(Z, V, torch.float32)
    P["constant"] = torch.tensor([0.3])
    P["raw_noise"] = torch.tensor([raw_noise])
    P["raw_lengthscale"] = torch.tensor([[-0.5]])
    if kernel == "ard":
        P["raw_lengthscale"] = (-0.5 + 0.2 * torch.linspace(-1.0, 1.0, d)).reshape(1, d)
    F = O.testfun(x)
    D = None
    y = F[:, 0].contiguous()
    if pd:
        D = O.normalize_rows(torch.randn(N * pd, d, generator=g)).contiguous()
        dirs = torch.einsum("nad,nd->na", D.reshape(N, pd, d), F[:, 1:])
        y = torch.cat([F[:, :1], dirs], dim=1).reshape(-1).contiguous()
    Dt = O.normalize_rows(torch.randn(HELD_OUT * p, d, generator=g)).contiguous()
    return P, x, y, D, ratio * N * (pd + 1), xt, Dt, kernel
