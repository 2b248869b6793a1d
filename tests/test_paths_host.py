"""CPU: the mathematics and the surface of the pathwise posterior sampler (ElboEngine.sample_paths / SamplePaths, csrc/paths.hip).

The yardstick ``path_reference`` is float64 and built from the oracle's kernel (through ``rect_kernel`` of test_gpu_rect_predict.py) and
the feature map, written as  c + Phi_X w + K_XZ' nu  -- NOT as the closed form the kernels evaluate:
    nu_s = L^-T [m + L_S eps_s - L^-1 (Phi_Z' w_s + sqrt(j) eta_s)],   K~ = s K_ZZ + j I = L L^T,
    phi_j(x) = sqrt(2 s / F) cos(omega_j . x / ell + b_j)
with the value row and all d derivative rows of every point (data directions eye(d) tiled).  The tests pin it to the oracle's
predictive mean, to the closed form, to the exact-moment identity  Cov f = s K_XX - A^T A + W^T W  and to the predictive covariance
at growing F.  tests/test_gpu_paths.py imports it."""
import functools
import inspect
import math
import os
import re

import pytest
import torch

import dsvgp_oracle as O
from test_gpu_rect_predict import rect_kernel, rect_predictive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = torch.float64


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ------------------------------------------------------------------ the yardstick
def make_draws(d, Mp, F, n, seed=7, zero=False):
    """omega, then phase, then w, eps, eta from one seeded generator (float64)"""
    g = torch.Generator().manual_seed(seed)
    dr = {"omega": torch.randn(F, d, generator=g, dtype=f64), "phase": 2 * math.pi * torch.rand(F, generator=g, dtype=f64),
          "w": torch.randn(n, F, generator=g, dtype=f64), "eps": torch.randn(n, Mp, generator=g, dtype=f64),
          "eta": torch.randn(n, Mp, generator=g, dtype=f64)}
    if zero:
        for k in ("w", "eps", "eta"):
            dr[k].zero_()
    return dr


def features(pts, dirs, q, omega, phase, ell, s):
    """Phi [N (q + 1), F], interleaved like the kernel: phi_j at the point, then -sqrt(2 s / F) sin(.) (omega_j . v^) / ell per direction"""
    N, d = pts.shape
    F = omega.shape[0]
    amp = torch.sqrt(2 * s / F)
    arg = pts @ omega.t() / ell + phase
    Phi = torch.empty(N, q + 1, F, dtype=f64)
    Phi[:, 0] = amp * torch.cos(arg)
    if q:
        Vn = O.normalize_rows(dirs).reshape(N, q, d)
        Phi[:, 1:] = -amp * torch.sin(arg)[:, None, :] * (Vn @ omega.t()) / ell
    return Phi.reshape(N * (q + 1), F)


def path_factor(P64):
    """(L, j, ell, s, c, M, d, p): the oracle's own factor of K~ = s K_ZZ + j I and the TOTAL diagonal j it carries"""
    Z, V = P64["inducing_points"], P64["inducing_directions"]
    ell, s, _ = O.constrained(P64)
    M, d = Z.shape
    p = V.shape[0] // M
    K = s * O.kernel_matrix(Z, Z, V, V, ell)
    L = O.psd_safe_cholesky(K + O.KZZ_JITTER * torch.eye(K.shape[0], dtype=f64))
    j = (L @ L.t() - K).diagonal().mean()
    return L, j, ell, s, P64["constant"].reshape(()), M, d, p


def path_nu(P64, draws):
    """nu [n, M'] in float64"""
    L, j, ell, s, c, M, d, p = path_factor(P64)
    Z, V = P64["inducing_points"], P64["inducing_directions"]
    m, L_S = P64["variational_mean"], torch.tril(P64["chol_variational_covar"])
    PhiZ = features(Z, V, p, draws["omega"], draws["phase"], ell, s)
    X = torch.linalg.solve_triangular(L, PhiZ @ draws["w"].t() + torch.sqrt(j) * draws["eta"].t(), upper=False)
    T = m[:, None] + L_S @ draws["eps"].t() - X
    return torch.linalg.solve_triangular(L.t(), T, upper=True).t().contiguous()


def path_reference(P64, x, draws):
    """(values [n, B], gradients [n, B, d]) of the paths as  c + Phi_X w + K_XZ' nu  with data directions eye(d) tiled; the gradient
    rows carry no constant"""
    L, j, ell, s, c, M, d, p = path_factor(P64)
    Z, V = P64["inducing_points"], P64["inducing_directions"]
    B = x.shape[0]
    E = torch.eye(d, dtype=f64).repeat(B, 1)
    nu = path_nu(P64, draws)
    PhiX = features(x, E, d, draws["omega"], draws["phase"], ell, s)
    K_XZ = s * rect_kernel(x, E, d, Z, V, p, ell)
    out = (PhiX @ draws["w"].t() + K_XZ @ nu.t()).t().reshape(-1, B, d + 1)
    return c + out[:, :, 0], out[:, :, 1:].contiguous()


def closed_form(P64, x, draws):
    """the closed form the kernels evaluate (value and gradient), float64"""
    L, j, ell, s, c, M, d, p = path_factor(P64)
    Z, V = P64["inducing_points"], P64["inducing_directions"]
    F = draws["omega"].shape[0]
    nu = path_nu(P64, draws).view(-1, M, p + 1)
    a = nu[:, :, 0]                                                                          # [n, M]
    Vn = O.normalize_rows(V).view(M, p, d) if p else torch.zeros(M, 0, d, dtype=f64)
    g = torch.einsum("sia,iak->sik", nu[:, :, 1:], Vn)                                       # [n, M, d]
    r = (Z[None] - x[:, None]) / ell                                                         # [B, M, d]
    k = torch.exp(-0.5 * (r * r).sum(-1))                                                    # [B, M]
    beta = a[:, None] - torch.einsum("bik,sik->sbi", r, g) / ell                             # [n, B, M]
    arg = x @ draws["omega"].t() / ell + draws["phase"]                                      # [B, F]
    amp = torch.sqrt(2 * s / F)
    val = c + amp * torch.cos(arg) @ draws["w"].t() + s * torch.einsum("bi,sbi->bs", k, beta)
    grad = (-amp * torch.einsum("bj,sj,jk->sbk", torch.sin(arg), draws["w"], draws["omega"]) / ell
            + s * (torch.einsum("bi,sbi,bik->sbk", k, beta, r) / ell + torch.einsum("bi,sik->sbk", k, g) / ell ** 2))
    return val.t().contiguous(), grad


def path_covariance(P64, x, Gxx, Gxz, Gzz):
    """Cov of f over the B (d + 1) outputs with w, eps, eta integrated out, from the prior's second moments G.. = E Phi. w w^T Phi.^T:
    f - c = Phi_X w + A^T [m + L_S eps - L^-1 (Phi_Z' w + sqrt(j) eta)],  A = L^-1 K_ZX'"""
    L, j, ell, s, c, M, d, p = path_factor(P64)
    Z, V = P64["inducing_points"], P64["inducing_directions"]
    L_S = torch.tril(P64["chol_variational_covar"])
    E = torch.eye(d, dtype=f64).repeat(x.shape[0], 1)
    A = torch.linalg.solve_triangular(L, s * rect_kernel(Z, V, p, x, E, d, ell), upper=False)
    T = torch.linalg.solve_triangular(L.t(), A, upper=True)                                  # L^-T A
    W = L_S.t() @ A
    return Gxx - Gxz @ T - T.t() @ Gxz.t() + T.t() @ Gzz @ T + W.t() @ W + j * T.t() @ T


def linear_map_covariance(P64, x, omega, phase):
    """J J^T of the linear map (w, eps, eta) -> f with omega, phase fixed"""
    L, j, ell, s, c, M, d, p = path_factor(P64)
    Z, V = P64["inducing_points"], P64["inducing_directions"]
    L_S = torch.tril(P64["chol_variational_covar"])
    E = torch.eye(d, dtype=f64).repeat(x.shape[0], 1)
    A = torch.linalg.solve_triangular(L, s * rect_kernel(Z, V, p, x, E, d, ell), upper=False)
    T = torch.linalg.solve_triangular(L.t(), A, upper=True)
    PhiX, PhiZ = features(x, E, d, omega, phase, ell, s), features(Z, V, p, omega, phase, ell, s)
    J = torch.cat([PhiX - T.t() @ PhiZ, A.t() @ L_S, -torch.sqrt(j) * T.t()], dim=1)
    return J @ J.t()


@functools.lru_cache(maxsize=None)
def problem(d, M, p, B, N=600):
    """(P fp32, P64, x fp64) of make_problem(N, d, M, p, B, seed=1): once per shape, shared, never changed"""
    from test_gpu_step import make_problem
    P, x, _, _, _ = make_problem(N, d, M, p, B, seed=1)
    return P, {k: v.double() for k, v in P.items()}, x.double()


TABLE = [(3, 12, 2, 20), (5, 40, 2, 32)]        # the two problems the covariance figures were measured on


# ------------------------------------------------------------------ (a) zero draws: the predictive mean
@pytest.mark.parametrize("d,M,p,B", TABLE)
def test_zero_draws_give_the_predictive_mean(d, M, p, B):
    _, P64, x = problem(d, M, p, B)
    draws = make_draws(d, M * (p + 1), 64, 2, zero=True)
    val, grad = path_reference(P64, x, draws)
    mu0, _ = O.predictive(P64, x, torch.eye(d, dtype=f64)[:p].repeat(B, 1), data_outputs="values")      # pd = 0
    mud, _, _ = rect_predictive(P64, x, torch.eye(d, dtype=f64).repeat(B, 1), d)                          # pd = d
    mud = mud.view(B, d + 1)
    c = P64["constant"].reshape(())
    errs = dict(values0=relmax(val[0], mu0), values=relmax(val[1], mud[:, 0]), gradient=relmax(grad[0], mud[:, 1:] - c))
    print("[paths] zero draws d=%d M=%d: %s" % (d, M, errs))
    assert max(errs.values()) <= 1e-12, errs


# ------------------------------------------------------------------ (b) the closed form of the kernels
@pytest.mark.parametrize("d,M,p,B", TABLE + [(5, 19, 5, 7), (4, 9, 0, 6)])
def test_closed_form_equals_the_yardstick(d, M, p, B):
    _, P64, x = problem(d, M, p, B)
    draws = make_draws(d, M * (p + 1), 256, 3)
    val, grad = path_reference(P64, x, draws)
    val_c, grad_c = closed_form(P64, x, draws)
    errs = dict(values=relmax(val_c, val), gradient=relmax(grad_c, grad))
    print("[paths] closed form d=%d M=%d p=%d: %s" % (d, M, p, errs))
    assert val.shape == (3, B) and grad.shape == (3, B, d)
    assert max(errs.values()) <= 1e-11, errs


# ------------------------------------------------------------------ (c) exact prior moments: the model's q(f)
@pytest.mark.parametrize("d,M,p,B", TABLE)
def test_exact_prior_moments_give_the_predictive_covariance(d, M, p, B):
    _, P64, x = problem(d, M, p, B)
    L, j, ell, s, c, _, _, _ = path_factor(P64)
    Z, V = P64["inducing_points"], P64["inducing_directions"]
    E = torch.eye(d, dtype=f64).repeat(B, 1)
    Gxx, Gxz, Gzz = s * rect_kernel(x, E, d, x, E, d, ell), s * rect_kernel(x, E, d, Z, V, p, ell), s * O.kernel_matrix(Z, Z, V, V, ell)
    cov = path_covariance(P64, x, Gxx, Gxz, Gzz)
    _, Sigma, _ = rect_predictive(P64, x, E, d)
    ref = Sigma - O.KXX_JITTER * torch.eye(Sigma.shape[0], dtype=f64)
    err = relmax(cov, ref)
    print("[paths] exact-moment identity d=%d M=%d: %.2e" % (d, M, err))
    assert err <= 1e-11, err


# ------------------------------------------------------------------ (d) the covariance of the linear map at growing F
@pytest.mark.parametrize("d,M,p,B", TABLE)
def test_linear_map_covariance_approaches_the_predictive(d, M, p, B):
    """Relative max-norm error of J J^T against the predictive covariance without its 1e-4 I, data directions eye(d) tiled.  The
    oracle's kernel takes equal direction counts on both sides, so at pd = d != p the reference is its rectangular restatement
    (rect_predictive, pinned to O.predictive_joint where that is defined); the rows of the directions eye(d)[:p] are held to
    O.predictive_joint itself as well.  Measured with make_draws' seed 7 (omega, then phase): d = 3 2.27e-2 / 8.4e-3 / 2.2e-3,
    d = 5 1.21e-1 / 2.5e-2 / 4.7e-3 at F = 256 / 4096 / 65536."""
    _, P64, x = problem(d, M, p, B)
    E = torch.eye(d, dtype=f64).repeat(B, 1)
    _, Sigma, _ = rect_predictive(P64, x, E, d)
    ref = Sigma - O.KXX_JITTER * torch.eye(Sigma.shape[0], dtype=f64)
    _, Sig_p = O.predictive_joint(P64, x, torch.eye(d, dtype=f64)[:p].repeat(B, 1))
    ref_p = Sig_p - O.KXX_JITTER * torch.eye(Sig_p.shape[0], dtype=f64)
    idx = (torch.arange(B)[:, None] * (d + 1) + torch.arange(p + 1)[None]).reshape(-1)
    errs = {}
    for F in (256, 4096, 65536):
        dr = make_draws(d, 1, F, 1)
        cov = linear_map_covariance(P64, x, dr["omega"], dr["phase"])
        errs[F] = relmax(cov, ref)
        err_p = relmax(cov[idx][:, idx], ref_p)
        print("[paths] covariance of the linear map d=%d M=%d F=%d: %.3e (rows of eye(d)[:p] vs O.predictive_joint: %.3e), bound %.3e"
              % (d, M, F, errs[F], err_p, 4 / math.sqrt(F)))
        assert errs[F] <= 4 / math.sqrt(F), (F, errs[F])
        assert err_p <= 4 / math.sqrt(F), (F, err_p)
    assert errs[65536] < errs[256], errs


def test_linear_map_covariance_is_the_moment_form():
    """J J^T equals the moment form at the features' own second moments (ties (c) to (d))"""
    d, M, p, B = TABLE[0]
    _, P64, x = problem(d, M, p, B)
    L, j, ell, s, c, _, _, _ = path_factor(P64)
    dr = make_draws(d, 1, 128, 1)
    E = torch.eye(d, dtype=f64).repeat(B, 1)
    PhiX = features(x, E, d, dr["omega"], dr["phase"], ell, s)
    PhiZ = features(P64["inducing_points"], P64["inducing_directions"], p, dr["omega"], dr["phase"], ell, s)
    err = relmax(linear_map_covariance(P64, x, dr["omega"], dr["phase"]), path_covariance(P64, x, PhiX @ PhiX.t(), PhiX @ PhiZ.t(), PhiZ @ PhiZ.t()))
    assert err <= 1e-11, err


# ------------------------------------------------------------------ (e) the surface
NEW = {"dsvgp_paths_weights_bytes": 4, "dsvgp_paths_workspace_bytes": 6, "dsvgp_paths_prepare": 16, "dsvgp_paths_eval": 11}


def test_library_exports_declares_and_binds_the_new_entries(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n, nargs in NEW.items():
        assert hasattr(dsvgp._lib.lib, n), "missing export: " + n
        assert n in dsvgp._lib.SIGNATURES, "missing binding: " + n
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, hdr, flags=re.S)
        assert decl, "not declared in include/dsvgp.h: " + n
        assert len(decl.group(1).split(",")) == len(dsvgp._lib.SIGNATURES[n][1]) == nargs, n
    build = open(os.path.join(os.path.dirname(dsvgp._lib.__file__), "build_ext.py")).read()
    assert '"paths.hip"' in build                           # the source list of the library


def test_size_helpers_are_host_functions_and_refuse_with_zero(dsvgp):
    wb, ws = dsvgp._ops.paths_weights_bytes, dsvgp._ops.paths_workspace_bytes
    assert 0 < wb(12, 3, 64, 1) < wb(12, 3, 64, 2) < wb(24, 3, 64, 2) < wb(24, 3, 128, 2) < wb(24, 40, 128, 2)
    assert wb(12, 3, 64, 1) % 16 == 0
    for bad in ((0, 3, 64, 1), (12, 0, 64, 1), (12, 3, 0, 1), (12, 3, 64, 0), (-1, 3, 64, 1)):
        assert wb(*bad) == 0 and ws(*bad, 8, 1) == 0, bad
    assert ws(12, 40, 64, 2, 0, 1) == 0
    assert ws(12, 3, 64, 2, 100, 1) == 0 and ws(12, 32, 64, 2, 100, 1) == 0          # fused route: registers and LDS only
    assert 0 < ws(12, 33, 64, 2, 100, 0) < ws(12, 33, 64, 2, 100, 1) < ws(12, 33, 64, 2, 200, 1) < ws(24, 33, 64, 2, 200, 1)
    assert ws(500, 200, 2048, 1, 2000000, 1) == 0                                   # B x F passes 2^31 entries: refused
    # nothing of size B x B: linear in B at the rover-like shape
    one, two = ws(512, 200, 2048, 8, 2500, 1), ws(512, 200, 2048, 8, 5000, 1)
    assert two < 2 * one + 4096 and two < (1 << 30)


def _params(M, d, p, dtype):
    Mp = M * (p + 1)
    return {"inducing_points": torch.zeros(M, d, dtype=dtype), "inducing_directions": torch.ones(M * p, d, dtype=dtype),
            "variational_mean": torch.zeros(Mp, dtype=dtype), "chol_variational_covar": torch.eye(Mp, dtype=dtype)}


def test_engines_refuse_before_touching_a_device(dsvgp):
    from dsvgp_amd._step64 import ElboEngine64
    eng64 = ElboEngine64(torch.device("cpu"))       # (construction allocates nothing; the refusal comes before any device work)
    with pytest.raises(NotImplementedError, match="float64"):
        eng64.sample_paths(_params(4, 3, 2, torch.float64), 2)
    eng = dsvgp.ElboEngine(torch.device("cpu"))
    eng.whitening = "ciq"
    with pytest.raises(NotImplementedError, match="msMINRES"):
        eng.sample_paths(_params(4, 3, 2, torch.float32), 2)


def test_model_and_harness_carry_the_new_entry_points(dsvgp):
    from dsvgp_amd import directional_vi, shared_directional_vi
    from dsvgp_amd.gp_shim import ApproximateGP
    sig = ["self", "params", "num_samples", "num_features", "generator", "base_samples"]
    assert list(inspect.signature(dsvgp.ElboEngine.sample_paths).parameters) == sig
    assert list(inspect.signature(ApproximateGP.sample_paths).parameters) == ["self"] + sig[2:]
    assert inspect.signature(dsvgp.ElboEngine.sample_paths).parameters["num_features"].default == 2048
    assert list(inspect.signature(directional_vi.eval_paths).parameters) == ["dataset_or_tensor", "paths", "minibatch_size", "gradients"]
    assert dsvgp.eval_paths is directional_vi.eval_paths and shared_directional_vi.eval_paths is directional_vi.eval_paths
    for name in ("values", "values_and_gradients", "__call__"):
        assert callable(getattr(dsvgp.SamplePaths, name))
