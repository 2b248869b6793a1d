"""The float64 CPU reference of training with missing observations, independent of the HIP code: a NaN target is an
observation that does not exist, so its column of K_ZX, its target and its prior-diagonal entry are DELETED and everything else is the
plain objective on what is left.

K~ = s K_ZZ + 1e-3 I, K = s K_ZX and the prior diagonal come from ``_collapsed_grad_ref.kernel_matrices`` -- the oracle's
``kernel_matrix`` for the scalar RBF model at pd = p, tests/_ard_yardstick.py / tests/_matern_yardstick.py (``radial_kernel``) otherwise,
as tests/_collapsed_ref.py builds them -- differentiable in the float64 raw parameters.  The Cholesky factor is ``torch.linalg.cholesky``
itself: a case whose K~ needs a jitter step fails here instead of being compared.

    step(...)       the minibatch loss -(sum_present ll / n - KL / num_data) (ELBO and PLL; n = 0: KL / num_data), its autograd gradients,
                    mu and varn of the present rows
    collapsed(...)  the collapsed statistics of the present rows, the optimum, the ELBO terms there and the collapsed loss's gradients"""
import math

import torch

import dsvgp_oracle as O
import _collapsed_ref as R
import _collapsed_grad_ref as RG


def present_mask(y):
    return ~torch.isnan(y)


def _leaves(P, names):
    Q = {k: v.detach().double().clone() for k, v in P.items()}
    for k in names:
        Q[k].requires_grad_(True)
    return Q


def _deleted(Q, x, y, D, kernel, keep):
    """(K~, K [M', n], y [n], prior diagonal [n], noise) with the missing columns / entries deleted"""
    keep = present_mask(y) if keep is None else keep
    Kt, K, dg, noise = RG.kernel_matrices(Q, x.double(), None if D is None else D.double(), kernel)
    return Kt, K[:, keep], y.double()[keep], dg[keep], noise, keep


def step_forward(Q, x, y, D, num_data, mll, kernel="rbf", keep=None):
    """(loss, mu [n], varn [n], keep) of the present rows; differentiable in the float64 parameters ``Q``"""
    Kt, K, yk, dg, noise, keep = _deleted(Q, x, y, D, kernel, keep)
    m, L_S = Q["variational_mean"], torch.tril(Q["chol_variational_covar"])
    kl = O.kl_whitened(m, L_S)
    n = int(keep.sum())
    L = torch.linalg.cholesky(Kt)
    A = torch.linalg.solve_triangular(L, K, upper=False)
    mu = A.t() @ m + Q["constant"].reshape(())
    SA = L_S @ (L_S.t() @ A) - A
    varn = (dg + O.KXX_JITTER + (A * SA).sum(0) + noise).clamp_min(O.MIN_VARIANCE)
    if n == 0:
        return kl / num_data, mu, varn, keep
    if mll == "ELBO":
        ll = -0.5 * (((yk - mu) ** 2 + varn) / noise + torch.log(noise) + math.log(2 * math.pi))
    elif mll == "PLL":
        tot = (varn + noise).clamp_min(1e-8)
        ll = -0.5 * ((yk - mu) ** 2 / tot + torch.log(tot) + math.log(2 * math.pi))
    else:
        raise ValueError(mll)
    return -(ll.sum() / n - kl / num_data), mu, varn, keep


def step(P, x, y, D, num_data, mll, kernel="rbf", keep=None):
    """(loss, {name: gradient} over O.PARAM_NAMES, mu [n], varn [n], keep [B'] bool) in float64, gradients by autograd.
    ``keep`` (default: the entries of y that are not NaN) names the present rows; what stands in the others is never read."""
    Q = _leaves(P, O.PARAM_NAMES)
    loss, mu, varn, keep = step_forward(Q, x, y, D, num_data, mll, kernel, keep)
    grads = torch.autograd.grad(loss, [Q[k] for k in O.PARAM_NAMES], allow_unused=True)
    grads = {k: (torch.zeros_like(Q[k]) if g is None else g) for k, g in zip(O.PARAM_NAMES, grads)}
    return loss.detach(), grads, mu.detach(), varn.detach(), keep


def collapsed(P, x, y, D, num_data=None, kernel="rbf", keep=None):
    """dict of the collapsed quantities of the present rows in float64: ``stats`` (G, b, yy, dg, R, noise), ``m`` / ``L_S`` (the optimum),
    ``terms`` (``_collapsed_ref.terms`` there), ``loss`` and ``grads`` (autograd through the optimum, over ``_collapsed_grad_ref.GRAD_NAMES``).
    ``num_data`` None: R, the present count."""
    Q = _leaves(P, RG.GRAD_NAMES)
    Kt, K, yk, dg, noise, keep = _deleted(Q, x, y, D, kernel, keep)
    nd = float(keep.sum()) if num_data is None else num_data
    L = torch.linalg.cholesky(Kt)
    A = torch.linalg.solve_triangular(L, K, upper=False)
    r = yk - Q["constant"].reshape(())
    stats = {"G": A @ A.t(), "b": A @ r, "yy": (r * r).sum(), "dg": dg.sum(), "R": float(r.numel()), "noise": noise}
    m, L_S = R.optimum(stats, num_data=nd)[:2]
    loss = R.loss(stats, m, L_S, num_data=nd)
    grads = torch.autograd.grad(loss, [Q[k] for k in RG.GRAD_NAMES], allow_unused=True)
    grads = {k: (torch.zeros_like(Q[k]) if g is None else g) for k, g in zip(RG.GRAD_NAMES, grads)}
    det = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in stats.items()}
    det["absG"] = (A.abs() @ A.abs().t()).detach()
    return {"stats": det, "m": m.detach(), "L_S": L_S.detach(), "terms": {k: v.detach() for k, v in R.terms(det, m.detach(), L_S.detach(), num_data=nd).items()},
            "loss": loss.detach(), "grads": grads, "keep": keep, "num_data": nd}


# ------------------------------------------------------------------ the shared cases of the host and GPU tests
def _raw(v):
    return math.log(math.expm1(v))          # softplus^-1


#        name      N    d    M  p  pd   B  kernel
CASES = {"m72":   (300, 3, 24, 2, 2, 37, "rbf"),          # M' = 72: crosses one 64-tile; B' = 111 ragged
         "m129":  (300, 3, 43, 2, 2, 37, "rbf"),          # M' = 129: one row past two tiles
         "wide":  (200, 100, 8, 2, 2, 37, "rbf"),         # d = 100: the wide assembly
         "ard":   (300, 3, 24, 2, 2, 37, "ard"),
         "matern": (300, 3, 24, 2, 2, 37, "matern52"),
         "rect":  (300, 3, 24, 2, 3, 37, "rbf")}          # pd != p: the rectangular step, B' = 148


def problem(name):
    """(params fp32, x [B, d], y [B (pd + 1)] all present, D [B pd, d], num_data, kernel): ``test_gpu_step.make_problem``'s model with generic
    unit data directions.  Deterministic in ``name``."""
    from test_gpu_step import make_problem
    N, d, M, p, pd, B, kernel = CASES[name]
    P, x, _, _, nd = make_problem(N, d, M, p, B, seed=5 + N + d + M + pd)
    if d > 30:                              # (otherwise the kernel between random points is numerically zero)
        P["raw_lengthscale"] = torch.tensor([[_raw(0.4 * math.sqrt(d))]])
    if kernel == "ard":
        P["raw_lengthscale"] = (P["raw_lengthscale"].reshape(()) + 0.2 * torch.linspace(-1.0, 1.0, d)).reshape(1, d)
    g = torch.Generator().manual_seed(23 + pd + d)
    D = O.normalize_rows(torch.randn(B * pd, d, generator=g)).contiguous()
    F = O.testfun(x)
    dirs = torch.einsum("nad,nd->na", D.reshape(B, pd, d), F[:, 1:])
    y = torch.cat([F[:, :1], dirs], dim=1).reshape(-1).contiguous()
    return P, x, y, D, nd, kernel


def random_pattern(y, pd, frac=0.3, seed=0):
    """y with about ``frac`` of its entries NaN (seeded CPU generator); by construction point 0 has every row missing and point 1 only
    its value"""
    g = torch.Generator().manual_seed(seed)
    q = pd + 1
    miss = torch.rand(y.shape[0], generator=g) < frac
    miss[0:q] = True
    miss[q:2 * q] = False
    miss[q] = True
    out = y.clone()
    out[miss] = float("nan")
    return out


def derivatives_missing(y, pd):
    """y with every derivative row NaN"""
    out = y.clone().reshape(-1, pd + 1)
    out[:, 1:] = float("nan")
    return out.reshape(-1)
