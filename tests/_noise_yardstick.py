"""The float64 yardstick of two likelihood noises, independent of the HIP code: function-value rows of an
interleaved batch (row j with j % (pd + 1) == 0) are observed under n_f = softplus(raw_noise) + 1e-4, derivative rows under
n_g = softplus(raw_derivative_noise) + 1e-4.

The step is ``matern_forward`` of tests/_matern_yardstick.py itself -- imported, not edited -- run with its noise replaced by the per-row
vector built from the two raw parameters (every use of the noise there broadcasts).  The family is a parameter: ``rbf_family`` or
``matern52_family``.  ``predictive`` is ``matern_predictive`` plus the per-row noise on the diagonal.

The weighted statistics and their closed-form optimum are written out directly here: with omega_r = n_f / n_r,
    G = sum omega a a^T, b = sum omega a r, yy = sum omega r^2, dg = sum omega (dg_r + 1e-4) - R 1e-4
and the ELBO of the whole data is, for any q(u) = N(m, L_S L_S^T),
    sum ll = -1/2 [ (yy - 2 m.b + m.G m + dg + R 1e-4 + tr(S G) - tr G) / n_f + R + R log n_f - R_g log rho + R log 2 pi ],  rho = n_f / n_g,
whose maximiser is S = (I + kappa G)^-1, m = kappa S b, kappa = num_data / (R n_f)."""
import contextlib
import math

import torch
import torch.nn.functional as F

import dsvgp_oracle as O
import _matern_yardstick as Y
from _matern_yardstick import matern52_family, rbf_family          # noqa: F401  (the families a caller names)

DNOISE = "raw_derivative_noise"
NAMES = tuple(O.PARAM_NAMES) + (DNOISE,)


def raw_of(noise):
    """the raw parameter whose constrained value is ``noise``"""
    return math.log(math.expm1(noise - O.NOISE_FLOOR))


def class_noises(P):
    return (F.softplus(P["raw_noise"]).reshape(()) + O.NOISE_FLOOR, F.softplus(P[DNOISE]).reshape(()) + O.NOISE_FLOOR)


def row_noise(P, B, pd):
    """[B (pd + 1)]: n_f on the value rows, n_g on the derivative rows; differentiable in both raw parameters"""
    n_f, n_g = class_noises(P)
    return torch.cat([n_f.reshape(1), n_g.reshape(1).expand(pd)]).repeat(B)


@contextlib.contextmanager
def _per_row_noise(noise_rows):
    """``matern_forward`` takes (ell, s, noise) from ``_matern_yardstick._ell``: the same with the per-row vector for the noise"""
    ell_of = Y._ell

    def per_row(P, d):
        ell, s, _ = ell_of(P, d)
        return ell, s, noise_rows
    Y._ell = per_row
    try:
        yield
    finally:
        Y._ell = ell_of


def forward(P, x, y, D, pd, num_data, mll, family=rbf_family):
    """(loss, mu, varn) of one minibatch objective under the two noises; differentiable"""
    with _per_row_noise(row_noise(P, x.shape[0], pd)):
        return Y.matern_forward(P, x, y, D, pd, num_data, mll, family)


def step(P, x, y, D, pd, num_data, mll, family=rbf_family):
    """(loss, grads over NAMES, mu, varn) in float64, gradients by autograd"""
    ps = {k: v.detach().double().clone().requires_grad_(True) for k, v in P.items()}
    loss, mu, varn = forward(ps, x.double(), y.double(), None if D is None else D.double(), pd, num_data, mll, family)
    loss.backward()
    grads = {k: (ps[k].grad if ps[k].grad is not None else torch.zeros_like(ps[k])) for k in ps}
    return loss.detach(), grads, mu.detach(), varn.detach()


def predictive(P, x, D, pd, family=rbf_family):
    """(mu, Sigma with the per-row likelihood noise on its diagonal, the same without it) in float64"""
    P64 = {k: v.detach().double() for k, v in P.items()}
    mu, Sigma = Y.matern_predictive(P64, x.double(), None if D is None else D.double(), pd, family)
    return mu, Sigma + torch.diag(row_noise(P64, x.shape[0], pd)), Sigma


# ------------------------------------------------------------------ weighted statistics, written out directly
def whitened(P, x, y, D, pd, family=rbf_family, noises=None):
    """(A [M', R], r [R], prior diagonal s dg_r [R], n_f, n_g) in float64.  ``noises``: (n_f, n_g) as given instead of the constrained
    raw parameters -- the C entry takes them from the float32 ``hyp``, so rho carries float32 rounding by its specification"""
    P = {k: v.detach().double() for k, v in P.items()}
    x, y = x.double(), y.double()
    D = None if D is None else D.double()
    Z, V = P["inducing_points"], P["inducing_directions"]
    ell, s, _ = Y._ell(P, Z.shape[1])
    p = V.shape[0] // Z.shape[0]
    K_ZZ = s * Y.radial_kernel(Z, V, p, Z, V, p, ell, family)
    L = torch.linalg.cholesky(K_ZZ + O.KZZ_JITTER * torch.eye(K_ZZ.shape[0], dtype=torch.float64))
    A = torch.linalg.solve_triangular(L, s * Y.radial_kernel(Z, V, p, x, D, pd, ell, family), upper=False)
    n_f, n_g = class_noises(P) if noises is None else (torch.as_tensor(v, dtype=torch.float64).reshape(()) for v in noises)
    return A, y - P["constant"].reshape(()), s * Y.radial_prior_diag(D, x.shape[0], pd, ell, family), n_f, n_g


def statistics(P, x, y, D, pd, family=rbf_family, noises=None):
    """dict: G, b, yy, dg (as the state word [0] holds it: sum omega dg_r + 1e-4 sum (omega - 1)), R, R_g, n_f, n_g, absG"""
    A, r, dg, n_f, n_g = whitened(P, x, y, D, pd, family, noises)
    B = x.shape[0]
    w = torch.cat([torch.ones(1, dtype=torch.float64), (n_f / n_g).reshape(1).expand(pd)]).repeat(B)
    Aw = A * w
    return {"G": Aw @ A.t(), "b": Aw @ r, "yy": (w * r * r).sum(), "dg": (w * dg).sum() + O.KXX_JITTER * (w - 1.0).sum(),
            "R": float(r.numel()), "R_g": float(B * pd), "n_f": n_f, "n_g": n_g, "absG": Aw.abs() @ A.abs().t()}


def kappa(stats, num_data):
    return num_data / (stats["R"] * stats["n_f"])


def cond_B(stats, num_data):
    n = stats["G"].shape[0]
    return torch.linalg.cond(torch.eye(n, dtype=torch.float64) + kappa(stats, num_data) * stats["G"]).item()


def optimum(stats, num_data):
    """(m*, L_S*): S = (I + kappa G)^-1, m = kappa S b"""
    n = stats["G"].shape[0]
    S = torch.linalg.inv(torch.eye(n, dtype=torch.float64) + kappa(stats, num_data) * stats["G"])
    S = 0.5 * (S + S.t())
    return kappa(stats, num_data) * (S @ stats["b"]), torch.linalg.cholesky(S)


def statistics_loss(stats, m, L_S, num_data, correction=True):
    """the full-data loss from the statistics alone; ``correction=False`` leaves out the (R_g / 2) log rho of the log-noise term (what
    the single-noise formula gives on the weighted statistics)"""
    m, L_S = m.double(), torch.tril(L_S.double())
    S = L_S @ L_S.t()
    R, n_f = stats["R"], stats["n_f"]
    quad = (stats["yy"] - 2.0 * m @ stats["b"] + m @ stats["G"] @ m + stats["dg"] + R * O.KXX_JITTER + (S * stats["G"]).sum()
            - torch.trace(stats["G"]))
    ll = -0.5 * (quad / n_f + R + R * torch.log(n_f) + R * math.log(2 * math.pi))
    if correction:
        ll = ll + 0.5 * stats["R_g"] * torch.log(n_f / stats["n_g"])
    return -(ll / R - O.kl_whitened(m, L_S) / num_data)


# ------------------------------------------------------------------ the shared problems of the host and GPU tests
def problem(d, M, p, pd, B, ard=False, seed=None, raw=(-2.0, 0.5)):
    """(params fp32 with raw_noise, raw_derivative_noise = ``raw``, x [B, d], y [B (pd + 1)], D [B pd, d] or None, num_data):
    ``test_gpu_step.make_problem``'s model with generic unit data directions.  Deterministic in its arguments."""
    from test_gpu_step import make_problem
    N = M + B + 20
    P, x, _, _, nd = make_problem(N, d, M, p, B, seed=(7 + 13 * d + M + 5 * pd + B) if seed is None else seed)
    if ard:
        P["raw_lengthscale"] = (P["raw_lengthscale"].reshape(()) + 0.2 * torch.linspace(-1.0, 1.0, d)).reshape(1, d)
    P["raw_noise"] = torch.tensor([raw[0]])
    P[DNOISE] = torch.tensor([raw[1]])
    g = torch.Generator().manual_seed(23 + pd + d)
    Fx = O.testfun(x)
    if pd == 0:
        return P, x, Fx[:, 0].contiguous(), None, nd
    D = O.normalize_rows(torch.randn(B * pd, d, generator=g)).contiguous()
    dirs = torch.einsum("nad,nd->na", D.reshape(B, pd, d), Fx[:, 1:])
    return P, x, torch.cat([Fx[:, :1], dirs], dim=1).reshape(-1).contiguous(), D, nd
