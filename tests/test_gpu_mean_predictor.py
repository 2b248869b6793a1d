"""Posterior-mean predictor (ElboEngine.mean_predictor / MeanPredictor, csrc/predict_mean.hip): the predictive mean and its
gradient of a frozen model from alpha = L^-T m, without K_ZX or a solve per batch.

The yardstick is ``mean_reference`` below, a compact float64 restatement of the closed form; the CPU tests pin it to the
reference-text strategy vectors (tests/golden/strategy_*.npz) and to autograd through the oracle's predictive.  The GPU tests hold
the HIP path (fused kernel for d <= 32, GEMM-composed path beyond) to the float64 oracle at the project's predictive-mean tolerance
(2e-4 of the max magnitude, tests/test_gpu_step.py); the measured errors are printed as [parity] lines."""
import functools
import math
import os

import pytest
import torch

import dsvgp_oracle as O
from _golden import STRATEGY, strategy_problem

gpu = pytest.mark.gpu
TOL = 2e-4


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _report(tag, errs):
    print("[parity] %s: %s" % (tag, ", ".join("%s %.2e" % (k, v) for k, v in errs.items())))


def mean_reference(P64, x, D, pd, values_only=False):      # P64: oracle-style params in float64
    Z, V, m = P64["inducing_points"], P64["inducing_directions"], P64["variational_mean"]
    ell, s, _ = O.constrained(P64); M, d = Z.shape; p = V.shape[0] // M
    K = s * O.kernel_matrix(Z, Z, V, V, ell) + O.KZZ_JITTER * torch.eye(M * (p + 1), dtype=torch.float64)
    L = O.psd_safe_cholesky(K)
    al = torch.linalg.solve_triangular(L.t(), m[:, None], upper=True)[:, 0].view(M, p + 1)
    g = (al[:, 1:, None] * O.normalize_rows(V).view(M, p, d)).sum(1) if p else torch.zeros(M, d, dtype=torch.float64)
    r = (Z[None] - x[:, None]) / ell; k = torch.exp(-0.5 * (r * r).sum(-1)); beta = al[:, 0][None] - (r * g[None]).sum(-1) / ell
    c = P64["constant"].reshape(())
    mu = c + s * (k * beta).sum(1)
    grad = s * (((k * beta)[..., None] * r).sum(1) / ell + (k[..., None] * g[None]).sum(1) / ell ** 2)
    if values_only or pd == 0: return mu, grad
    out = torch.cat([mu[:, None], (O.normalize_rows(D).view(-1, pd, d) * grad[:, None]).sum(-1) + c], 1).reshape(-1)
    return out, grad


def _expanded(P, shared):
    """oracle-style parameters of a strategy vector with the shared direction set tiled (O.shared_expand); q(u)'s covariance does
    not reach the mean, a unit factor stands in"""
    if not shared:
        return P
    M = P["inducing_points"].shape[0]
    V, iv = O.shared_expand(P["inducing_directions"], P["variational_mean"], M)
    Q = dict(P)
    Q["inducing_directions"], Q["variational_mean"] = V, iv
    Q["chol_variational_covar"] = torch.eye(iv.shape[0], dtype=iv.dtype)
    return Q


def _raw(v):
    return math.log(math.expm1(v))          # softplus^-1


# ------------------------------------------------------------------ CPU 1: the yardstick against the reference-text vectors
@pytest.mark.parametrize("path", STRATEGY, ids=[os.path.basename(p) for p in STRATEGY])
def test_reference_formula_matches_strategy_vectors_and_autograd(path):
    P, x, D, fl, mean_ref, _ = strategy_problem(path)
    P = _expanded(P, fl["shared"])
    B = x.shape[0]
    values = fl["outputs"] == "values"
    pd = D.shape[0] // B
    mu, grad = mean_reference(P, x, D, pd, values_only=values)
    xg = x.clone().requires_grad_(True)
    q = 1 if values else pd + 1
    total = O.predictive(P, xg, D, data_outputs=fl["outputs"])[0][::q].sum()
    (g_auto,) = torch.autograd.grad(total, xg)
    errs = dict(mean=relmax(mu, mean_ref), gradient=relmax(grad, g_auto))
    _report("closed form vs strategy vector " + os.path.basename(path), errs)
    assert mu.shape == mean_ref.shape
    assert errs["mean"] <= 1e-12 and errs["gradient"] <= 1e-12, errs


# ------------------------------------------------------------------ CPU 2: the size helpers (pure host functions)
def test_size_helpers_are_host_functions_and_bound_the_workspace(dsvgp):
    ops = dsvgp._ops
    assert 0 < ops.mean_weights_bytes(100, 5) < ops.mean_weights_bytes(200, 5) < ops.mean_weights_bytes(200, 50)
    # the fused kernel (d <= 32) keeps everything in registers and LDS; beyond, [B, 2M] intermediates
    assert ops.mean_workspace_bytes(100, 5, 64, 2) == 0
    w = ops.mean_workspace_bytes
    assert 0 < w(100, 200, 64, 2) < w(200, 200, 64, 2) < w(200, 400, 64, 2) < w(200, 400, 128, 2) <= w(200, 400, 128, 4)
    for M, d, B, pd in ((500, 20, 4096, 5), (512, 200, 2048, 3)):
        bound = 4 * (4 * B * M + 8 * (B + M) * (d + 16) + 4096)
        assert w(M, d, B, pd) < bound, (M, d, B, pd, w(M, d, B, pd), bound)      # nothing of size M' x B'
    assert ops.mean_weights_bytes(0, 5) == 0 and w(0, 5, 1, 0) == 0 and w(5, 0, 1, 0) == 0 and w(5, 5, 0, 0) == 0


# ------------------------------------------------------------------ GPU 3: reference-text means
@gpu
@pytest.mark.parametrize("path", STRATEGY, ids=[os.path.basename(p) for p in STRATEGY])
def test_mean_matches_reference_strategy_vectors(dsvgp, gpu_device, path):
    P, x, D, fl, mean_ref, _ = strategy_problem(path, torch.float32)
    eng = dsvgp.ElboEngine(gpu_device)
    eng.data_outputs, eng.shared_directions = fl["outputs"], fl["shared"]
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    mu = eng.mean_predictor(Pg).mean(x.to(gpu_device), D.to(gpu_device))
    errs = dict(mean=relmax(mu, mean_ref))
    _report("mean predictor vs strategy vector " + os.path.basename(path), errs)
    assert mu.shape == mean_ref.shape and errs["mean"] < TOL, errs


# ------------------------------------------------------------------ GPU 4 / 5: shapes where tiling can go wrong, wide inputs
NARROW = [(300, 3, 33, 3, 70), (300, 5, 19, 0, 67), (900, 28, 17, 5, 77), (400, 32, 21, 5, 37), (400, 33, 21, 5, 37),
          (3000, 5, 200, 2, 512), (6000, 20, 130, 5, 4099), (300, 100, 9, 95, 5)]
WIDE = [(400, 92, 21, 3, 37), (400, 93, 21, 3, 37), (400, 120, 24, 3, 40), (400, 200, 24, 3, 40), (300, 4035, 6, 2, 9)]


@functools.lru_cache(maxsize=None)
def _case(N, d, M, p, B):
    """(params fp32, x, D, oracle mean fp64, closed-form gradient fp64, constant): computed once per shape, shared, never changed"""
    from test_gpu_step import make_problem
    P, x, _, D, _ = make_problem(N, d, M, p, B, seed=1)
    if d > 30:          # (lengthscale of tests/test_gpu_wide_inputs.py: otherwise the kernel between random points is numerically zero)
        P["raw_lengthscale"] = torch.tensor([[_raw(0.4 * math.sqrt(d))]])
    P64 = {k: v.double() for k, v in P.items()}
    mu_ref, _ = O.predictive(P64, x.double(), D.double())
    _, grad_ref = mean_reference(P64, x.double(), D.double(), p)
    return P, x, D, mu_ref, grad_ref, float(P["constant"].reshape(()))


def _check_case(dsvgp, dev, N, d, M, p, B):
    P, x, D, mu_ref, grad_ref, c = _case(N, d, M, p, B)
    eng = dsvgp.ElboEngine(dev)
    pred = eng.mean_predictor({k: v.to(dev) for k, v in P.items()})
    mu = pred.mean(x.to(dev), D.to(dev))
    val, grad = pred.value_and_gradient(x.to(dev))
    span = (mu_ref - c).abs().max().item()
    errs = {"mean": relmax(mu, mu_ref), "gradient": relmax(grad, grad_ref), "values": relmax(val, mu_ref[::p + 1]),
            "max|mu_ref - c|": span}
    _report("mean predictor N=%d d=%d M=%d p=%d B=%d" % (N, d, M, p, B), errs)
    assert span >= 0.05                                                  # the reference is not trivial
    assert mu.shape == (B * (p + 1),) and grad.shape == (B, d)
    assert errs["mean"] < TOL and errs["gradient"] < TOL and errs["values"] < TOL, errs


@gpu
@pytest.mark.parametrize("N,d,M,p,B", NARROW)
def test_mean_and_gradient_match_fp64(dsvgp, gpu_device, N, d, M, p, B):
    """ragged tiles, p = 0, the fused / composed boundary (d = 32 | 33), the C2 size, several workgroups with a ragged last tile,
    q = 96"""
    _check_case(dsvgp, gpu_device, N, d, M, p, B)


@gpu
@pytest.mark.parametrize("N,d,M,p,B", WIDE)
def test_mean_and_gradient_match_fp64_at_wide_inputs(dsvgp, gpu_device, N, d, M, p, B):
    _check_case(dsvgp, gpu_device, N, d, M, p, B)


# ------------------------------------------------------------------ GPU 6: directions at the data
@gpu
def test_directions_are_normalised_and_independent_of_the_models_p(dsvgp, gpu_device):
    from test_gpu_step import make_problem
    dev = gpu_device
    N, d, M, p, B = 600, 5, 40, 2, 128
    P, x, _, D, _ = make_problem(N, d, M, p, B, seed=1)
    P64 = {k: v.double() for k, v in P.items()}
    c = P64["constant"].reshape(())
    pred = dsvgp.ElboEngine(dev).mean_predictor({k: v.to(dev) for k, v in P.items()})
    xg = x.to(dev)
    # (a) rows of D scaled by factors in [0.1, 10]: the same means (the oracle normalises too)
    g = torch.Generator().manual_seed(3)
    Ds = D * (0.1 * 100.0 ** torch.rand(D.shape[0], 1, generator=g))
    mu_ref, _ = O.predictive(P64, x.double(), Ds.double())
    mu_unit, mu_scaled = pred.mean(xg, D.to(dev)), pred.mean(xg, Ds.to(dev))
    errs = {"unit rows": relmax(mu_unit, mu_ref), "scaled rows": relmax(mu_scaled, mu_ref)}
    # (b) pd = d with eye(d) tiled: the derivative rows minus c are the gradient
    E = torch.eye(d).repeat(B, 1)
    mu_full = pred.mean(xg, E.to(dev))
    val, grad = pred.value_and_gradient(xg)
    ref_full, grad_ref = mean_reference(P64, x.double(), E.double(), d)
    rows = mu_full.reshape(B, d + 1)[:, 1:].double().cpu() - c
    errs.update({"pd = d rows": relmax(mu_full, ref_full), "rows - c vs closed-form gradient": relmax(rows, grad_ref),
                 "gradient": relmax(grad, grad_ref), "rows - c vs gradient": relmax(rows, grad)})
    _report("directions d=5 p=2", errs)
    assert max(errs.values()) < TOL, errs
    # (c) D = None: exactly the value rows of the pd = 2 call
    assert torch.equal(pred.mean(xg), mu_unit[::p + 1])
    assert torch.equal(val, mu_unit[::p + 1])


# ------------------------------------------------------------------ GPU 7: reproducibility
@gpu
def test_two_identical_calls_are_bitwise_equal(dsvgp, gpu_device):
    N, d, M, p, B = 3000, 5, 200, 2, 512          # the C2 size
    P, x, D, *_ = _case(N, d, M, p, B)
    dev = gpu_device
    pred = dsvgp.ElboEngine(dev).mean_predictor({k: v.to(dev) for k, v in P.items()})
    xg, Dg = x.to(dev), D.to(dev)
    m1, m2 = pred.mean(xg, Dg), pred.mean(xg, Dg)
    (v1, g1), (v2, g2) = pred.value_and_gradient(xg), pred.value_and_gradient(xg)
    assert torch.equal(m1, m2) and torch.equal(v1, v2) and torch.equal(g1, g2)


@gpu
def test_composed_path_is_bitwise_reproducible_too(dsvgp, gpu_device):
    P, x, D, *_ = _case(400, 200, 24, 3, 40)
    dev = gpu_device
    pred = dsvgp.ElboEngine(dev).mean_predictor({k: v.to(dev) for k, v in P.items()})
    xg, Dg = x.to(dev), D.to(dev)
    m1, m2 = pred.mean(xg, Dg), pred.mean(xg, Dg)
    (v1, g1), (v2, g2) = pred.value_and_gradient(xg), pred.value_and_gradient(xg)
    assert torch.equal(m1, m2) and torch.equal(v1, v2) and torch.equal(g1, g2)


# ------------------------------------------------------------------ GPU 8: natural parameters
@gpu
def test_natural_parameters(dsvgp, gpu_device):
    from test_ngd import make_ngd_problem
    dev = gpu_device
    P, x, _, D, _ = make_ngd_problem(600, 5, 40, 2, 128)
    P64 = {k: v.double() for k, v in P.items()}
    m, LS = O.natural_to_mu_chol(P64["natural_vec"], P64["natural_mat"])
    Pc = {k: v for k, v in P64.items() if not k.startswith("natural_")}
    Pc["variational_mean"], Pc["chol_variational_covar"] = m, LS
    mu_ref, _ = O.predictive(Pc, x.double(), D.double())
    mu = dsvgp.ElboEngine(dev).mean_predictor({k: v.to(dev) for k, v in P.items()}).mean(x.to(dev), D.to(dev))
    errs = dict(mean=relmax(mu, mu_ref))
    _report("mean predictor, natural parameters", errs)
    assert errs["mean"] < TOL, errs


# ------------------------------------------------------------------ GPU 9: model level
@gpu
def test_model_posterior_mean_eval_mean_and_cache_invalidation(dsvgp, gpu_device, capsys):
    from torch.utils.data import TensorDataset
    torch.manual_seed(0)
    n, dim, n_test = 600, 2, 300          # the size of tests/test_gpu_step.py's drop-in run, one epoch
    train_x, test_x = torch.rand(n, dim), torch.rand(n_test, dim)
    train_y, test_y = O.testfun(train_x), O.testfun(test_x)
    model, likelihood = dsvgp.train_gp(TensorDataset(train_x, train_y), num_inducing=20, num_directions=2, minibatch_size=200,
                                       minibatch_dim=2, num_epochs=1, inducing_data_initialization=False, tqdm=False,
                                       verbose=False, seed=0)
    capsys.readouterr()
    model.eval()
    likelihood.eval()
    dev = gpu_device
    xg = test_x.to(dev)
    D = torch.eye(dim, device=dev)[:2].repeat(n_test, 1)
    with torch.no_grad():
        mu_old = likelihood(model(xg, derivative_directions=D)).mean
    mu = model.posterior_mean(xg, derivative_directions=D)
    dst = TensorDataset(test_x, test_y)
    means = dsvgp.eval_mean(dst, model, num_directions=2, minibatch_size=128, minibatch_dim=2)
    means_old, _ = dsvgp.eval_gp(dst, model, likelihood, num_directions=2, minibatch_size=128, minibatch_dim=2)
    capsys.readouterr()
    grad = model.posterior_mean_gradient(xg)
    c = model.mean_module.constant.detach().reshape(())
    errs = {"posterior_mean vs model(x).mean": relmax(mu, mu_old), "eval_mean vs eval_gp": relmax(means, means_old),
            "gradient vs derivative rows - c": relmax(grad, mu.reshape(n_test, 3)[:, 1:] - c)}
    _report("model level", errs)
    assert means.shape == (n_test * 3,) and not means.is_cuda and means.dim() == 1
    assert max(errs.values()) < TOL, errs
    # eval mode: the predictor is cached; an in-place parameter change invalidates it
    assert model._mean_predictor() is model._mean_predictor()
    with torch.no_grad():
        model.variational_strategy._variational_distribution.variational_mean.add_(0.1)
    mu2 = model.posterior_mean(xg, derivative_directions=D)
    fresh = model.engine.mean_predictor(model._param_dict(None)).mean(xg, D)
    assert not torch.equal(mu2, mu)
    assert torch.equal(mu2, fresh)


# ------------------------------------------------------------------ GPU 10: refusals
@gpu
def test_refusals(dsvgp, gpu_device):
    from test_gpu_step import make_problem
    dev = gpu_device
    P, x, _, D, _ = make_problem(300, 3, 12, 2, 20, seed=1)
    Pg = {k: v.to(dev) for k, v in P.items()}
    eng = dsvgp.ElboEngine(dev)
    eng.whitening = "ciq"
    with pytest.raises(NotImplementedError, match="msMINRES"):
        eng.mean_predictor(Pg)
    pred = dsvgp.ElboEngine(dev).mean_predictor(Pg)
    with pytest.raises(dsvgp._lib.DsvgpError):
        pred.mean(x, D.to(dev))                      # x on the CPU
    with pytest.raises(dsvgp._lib.DsvgpError):
        pred.value_and_gradient(x)
    eng64 = dsvgp.ElboEngine64(dev)
    if hasattr(eng64, "mean_predictor"):
        with pytest.raises(NotImplementedError):
            eng64.mean_predictor({k: v.double() for k, v in Pg.items()})
    # the C entry points refuse empty problems like their neighbours
    ops, lib = dsvgp._ops, dsvgp._lib.lib
    ctx = ops.Context.get(dev)
    w = pred.weights
    out = torch.empty(8, device=dev)
    import ctypes as C
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert lib.dsvgp_mean_predict(ctx.h, vp(w), 12, 3, vp(Pg["inducing_points"]), 0, None, 0, vp(out), None, None) == -1
    assert lib.dsvgp_mean_predict(ctx.h, vp(w), 0, 3, vp(Pg["inducing_points"]), 2, None, 0, vp(out), None, None) == -1
    assert lib.dsvgp_mean_predict(ctx.h, vp(w), 12, 0, vp(Pg["inducing_points"]), 2, None, 0, vp(out), None, None) == -1
