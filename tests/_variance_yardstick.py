"""Float64 yardstick of the posterior-variance predictor and of the acquisitions built on it (csrc/predict_variance.hip,
ElboEngine.variance_predictor): the Q-form of include/dsvgp.h restated in torch,

    K~ = s K_ZZ + j I = L L^T,  Q = L^-T (S - I) L^-1,  k(x) = s K_Z'x,  v = Q k,
    sigma^2 = s + 1e-4 + k . v = s + 1e-4 + s sum_i k_i beta_i,   grad sigma^2 = 2 s sum_i k_i (beta_i r_i / ell + g_i / ell^2)

with a_i = v[i(p+1)], g_i = sum_s v[i(p+1)+1+s] v^_is, r_i = (z_i - x) / ell, k_i = exp(-|r_i|^2 / 2), beta_i = a_i - r_i . g_i / ell,
the posterior mean in the same form with alpha = L^-T m, and the three acquisitions with their gradients in closed form.
tests/test_variance_host.py pins all of it to the oracle and to autograd; tests/test_gpu_variance.py holds the kernels to it."""
import functools
import math

import torch

import dsvgp_oracle as O

f64 = torch.float64
KINDS = ("lcb_var", "lcb", "ei")
MIN_VAR = 1e-6


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _raw(v):
    return math.log(math.expm1(v))          # softplus^-1


@functools.lru_cache(maxsize=None)
def problem(d, M, p, B, seed=1, small_variance=False):
    """(P fp32, P64, x fp64 [B, d]): random inducing points in the unit cube, random directions (any p, also p > d), a perturbed
    q(u); lengthscale 0.4 sqrt(d) for d > 30 (otherwise the kernel between random points is numerically zero).  ``small_variance``:
    L_S = 0.05 I and the test points placed ON inducing points (cyclically), so that sigma^2 << s.  Once per shape, shared, never
    changed."""
    g = torch.Generator().manual_seed(seed)
    Z = torch.rand(M, d, generator=g)
    V = torch.randn(M * p, d, generator=g)
    P = O.init_params(Z, V, torch.float32, mean_init_std=0.2, generator=g)
    Mp = M * (p + 1)
    P["chol_variational_covar"] = (0.05 * torch.eye(Mp) if small_variance
                                   else torch.eye(Mp) + 0.05 * torch.randn(Mp, Mp, generator=g))      # (above the diagonal: masked)
    P["constant"] = torch.tensor([0.1])
    P["raw_outputscale"] = torch.tensor(0.2)
    P["raw_lengthscale"] = torch.tensor([[_raw(0.4 * math.sqrt(d))]]) if d > 30 else torch.tensor([[0.3]])
    P["raw_noise"] = torch.tensor([-0.5])
    x = Z[torch.arange(B) % M].clone() if small_variance else torch.rand(B, d, generator=g)
    return P, {k: v.double() for k, v in P.items()}, x.double()


def expanded(P, shared):
    """oracle-style parameters of a shared-directions model with the direction set tiled (O.shared_expand); its q(u) covariance does
    not reach the predictive: a unit factor stands in and ``factor(no_middle=True)`` ignores it"""
    if not shared:
        return P
    M = P["inducing_points"].shape[0]
    V, iv = O.shared_expand(P["inducing_directions"], P["variational_mean"], M)
    out = dict(P)
    out["inducing_directions"], out["variational_mean"] = V, iv
    out["chol_variational_covar"] = torch.eye(iv.shape[0], dtype=iv.dtype)
    return out


def factor(P64, no_middle=False):
    """(L, Q, alpha, ell, s, c, M, d, p) in float64; ``no_middle``: S = 0 (shared directions), Q = -K~^-1"""
    Z, V, m = P64["inducing_points"], P64["inducing_directions"], P64["variational_mean"]
    ell, s, _ = O.constrained(P64)
    M, d = Z.shape
    p = V.shape[0] // M
    Mp = M * (p + 1)
    I = torch.eye(Mp, dtype=f64)
    L = O.psd_safe_cholesky(s * O.kernel_matrix(Z, Z, V, V, ell) + O.KZZ_JITTER * I)
    Linv = torch.linalg.solve_triangular(L, I, upper=False)
    L_S = torch.tril(P64["chol_variational_covar"])
    Q = Linv.t() @ ((-I) if no_middle else (L_S @ L_S.t() - I)) @ Linv
    return L, 0.5 * (Q + Q.t()), Linv.t() @ m, ell, s, P64["constant"].reshape(()), M, d, p


def cross(P64, x):
    """k(x) = s K_Z'x [M (p + 1), B]: value columns only (the data side carries no directions)"""
    Z, V = P64["inducing_points"], P64["inducing_directions"]
    ell, s, _ = O.constrained(P64)
    M, d = Z.shape
    p = V.shape[0] // M
    r = (Z[:, None] - x[None]) / ell                                                          # [M, B, d]
    k = torch.exp(-0.5 * (r * r).sum(-1))                                                     # [M, B]
    rows = [k[:, None]]
    if p:
        rows.append(-torch.einsum("ibk,iak->iab", r, O.normalize_rows(V).view(M, p, d)) * k[:, None] / ell)
    return s * torch.cat(rows, dim=1).reshape(M * (p + 1), x.shape[0])


def _weighted_sums(P64, x, w, ell, s, M, d, p):
    """(s sum_i k_i beta_i [B], s sum_i k_i (beta_i r_i / ell + g_i / ell^2) [B, d]) for per-point weights w [M (p + 1), B]"""
    Z, V = P64["inducing_points"], P64["inducing_directions"]
    w = w.reshape(M, p + 1, -1)
    a = w[:, 0].t()                                                                           # [B, M]
    g = (torch.einsum("iab,iak->bik", w[:, 1:], O.normalize_rows(V).view(M, p, d)) if p
         else torch.zeros(w.shape[2], M, d, dtype=f64))                                       # [B, M, d]
    r = (Z[None] - x[:, None]) / ell                                                          # [B, M, d]
    k = torch.exp(-0.5 * (r * r).sum(-1))                                                     # [B, M]
    beta = a - (r * g).sum(-1) / ell
    val = s * (k * beta).sum(1)
    grad = s * (((k * beta)[..., None] * r).sum(1) / ell + (k[..., None] * g).sum(1) / ell ** 2)
    return val, grad


def moments(P64, x, no_middle=False):
    """(mu [B], grad mu [B, d], sigma^2 [B], grad sigma^2 [B, d]) of q(f) at x, float64, closed forms"""
    L, Q, alpha, ell, s, c, M, d, p = factor(P64, no_middle)
    B = x.shape[0]
    mu, gmu = _weighted_sums(P64, x, alpha[:, None].expand(-1, B), ell, s, M, d, p)
    kv, gkv = _weighted_sums(P64, x, Q @ cross(P64, x), ell, s, M, d, p)
    return c + mu, gmu, s + O.KXX_JITTER + kv, 2.0 * gkv


def variance(P64, x, no_middle=False):
    """sigma^2 [B] as the quadratic form itself: s + 1e-4 + k . Q k (differentiable in x)"""
    _, Q, _, _, s, _, _, _, _ = factor(P64, no_middle)
    k = cross(P64, x)
    return s + O.KXX_JITTER + (k * (Q @ k)).sum(0)


def acquisition(mu, gmu, var, gvar, kind, beta=2.0, best=None, maximize=False):
    """(a [B], grad a [B, d]) of the three kinds, smaller is better; ``maximize`` mirrors the model (mu -> -mu, best -> -best)"""
    sg = -1.0 if maximize else 1.0
    m, gm = sg * mu, sg * gmu
    if kind == "lcb_var":
        return m - beta * var, gm - beta * gvar
    clamped = ~(var > MIN_VAR)
    sd = torch.sqrt(torch.where(clamped, torch.full_like(var, MIN_VAR), var))
    gsd = torch.where(clamped[:, None], torch.zeros_like(gvar), gvar / (2.0 * sd[:, None]))
    if kind == "lcb":
        return m - beta * sd, gm - beta * gsd
    if kind != "ei":
        raise ValueError(kind)
    imp = sg * best - m
    z = imp / sd
    Phi = 0.5 * torch.erfc(-z / math.sqrt(2.0))
    phi = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return -(imp * Phi + sd * phi), Phi[:, None] * gm - phi[:, None] * gsd


def acquisition_at(P64, x, kind, beta=2.0, best=None, maximize=False, no_middle=False):
    return acquisition(*moments(P64, x, no_middle), kind, beta, best, maximize)


def ei_best(P64, x, maximize=False, no_middle=False):
    """an incumbent for which |z| <= 3 on every point of x: the midpoint of the range of mu -/+ 3 sigma intervals' intersection
    when it is not empty, checked by the caller"""
    mu, _, var, _ = moments(P64, x, no_middle)
    m = -mu if maximize else mu
    sd = var.clamp_min(MIN_VAR).sqrt()
    lo, hi = (m - 3.0 * sd).max(), (m + 3.0 * sd).min()
    best = 0.5 * (lo + hi)
    return float(-best if maximize else best)
