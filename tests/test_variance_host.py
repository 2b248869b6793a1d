"""CPU: the float64 yardstick of the posterior-variance predictor (tests/_variance_yardstick.py) against the oracle and autograd, the
acquisition closed forms against autograd of torch expressions, and the host surface of the feature: exports, header declarations,
ctypes bindings, the size / route / chunk helpers (pure host functions) and the refusals that are raised before any device work."""
import math
import os
import re

import pytest
import torch

import dsvgp_oracle as O
import _variance_yardstick as Y
from _variance_yardstick import relmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = torch.float64

#          d   M  p   B
SHAPES = [(3, 24, 2, 50), (5, 64, 2, 70), (4, 9, 0, 6), (3, 8, 3, 10), (6, 10, 2, 12)]
IDS = ["d%d-M%d-p%d-B%d" % s for s in SHAPES]


def _oracle_dirs(d, p, B):
    return torch.eye(d, dtype=f64)[:p].repeat(B, 1)           # (data directions: not read with data_outputs = "values")


# ------------------------------------------------------------------ the Q-form against the oracle's predictive
@pytest.mark.parametrize("d,M,p,B", SHAPES, ids=IDS)
def test_q_form_equals_the_oracle_variance_and_mean(d, M, p, B):
    _, P64, x = Y.problem(d, M, p, B)
    mu_ref, var_ref = O.predictive(P64, x, _oracle_dirs(d, p, B), data_outputs="values")
    mu, _, var, _ = Y.moments(P64, x)
    errs = dict(closed_form=relmax(var, var_ref), quadratic_form=relmax(Y.variance(P64, x), var_ref), mean=relmax(mu, mu_ref))
    print("[variance] yardstick vs oracle d=%d M=%d p=%d: %s" % (d, M, p, errs))
    assert max(errs.values()) <= 1e-11, errs


@pytest.mark.parametrize("d,M,p,B", SHAPES, ids=IDS)
def test_gradients_equal_autograd_through_the_oracle(d, M, p, B):
    _, P64, x = Y.problem(d, M, p, B)
    xg = x.clone().requires_grad_(True)
    mu_o, var_o = O.predictive(P64, xg, _oracle_dirs(d, p, B), data_outputs="values")
    (gvar_auto,) = torch.autograd.grad(var_o.sum(), xg, retain_graph=True)
    (gmu_auto,) = torch.autograd.grad(mu_o.sum(), xg)
    _, gmu, _, gvar = Y.moments(P64, x)
    errs = dict(variance_gradient=relmax(gvar, gvar_auto), mean_gradient=relmax(gmu, gmu_auto))
    print("[variance] yardstick gradients vs oracle autograd d=%d M=%d p=%d: %s" % (d, M, p, errs))
    assert max(errs.values()) <= 1e-9, errs


def test_shared_directions_take_the_zero_middle_term():
    """S = 0: sigma^2 = s + 1e-4 - k . K~^-1 k"""
    d, M, p, B = 4, 12, 2, 9
    _, P64, x = Y.problem(d, M, p, B)
    L, _, _, _, s, _, _, _, _ = Y.factor(P64, no_middle=True)
    k = Y.cross(P64, x)
    A = torch.linalg.solve_triangular(L, k, upper=False)
    ref = s + O.KXX_JITTER - (A * A).sum(0)
    mu, _, var, _ = Y.moments(P64, x, no_middle=True)
    assert relmax(var, ref) <= 1e-11 and relmax(Y.variance(P64, x, no_middle=True), ref) <= 1e-11
    assert (var < s + O.KXX_JITTER).all()


def test_small_variance_case_keeps_the_floor():
    """L_S = 0.05 I at the inducing points: sigma^2 << s, and the float64 yardstick stays above 1e-4 - 2e-4 s"""
    for d, M, p, B in ((3, 40, 2, 50), (5, 30, 0, 40)):
        _, P64, x = Y.problem(d, M, p, B, small_variance=True)
        s = O.constrained(P64)[1].item()
        _, _, var, _ = Y.moments(P64, x)
        _, var_ref = O.predictive(P64, x, _oracle_dirs(d, p, B), data_outputs="values")
        # (sigma^2 is what is left of s after a cancellation: both float64 routes round terms of size s, so the agreement is
        #  measured against s, not against the small result)
        err = (var - var_ref).abs().max().item() / s
        print("[variance] small variance d=%d: min sigma^2 %.3e, s %.3f, err / s %.2e" % (d, var.min().item(), s, err))
        assert err <= 1e-11
        assert var.max().item() < 0.2 * s and var.min().item() >= 1e-4 - 2e-4 * s


# ------------------------------------------------------------------ the acquisition closed forms against autograd
def _acq_autograd(mu, gmu, var, gvar, kind, beta, best, maximize):
    mu_t, var_t = mu.clone().requires_grad_(True), var.clone().requires_grad_(True)
    sg = -1.0 if maximize else 1.0
    m = sg * mu_t
    if kind == "lcb_var":
        a = m - beta * var_t
    else:
        sd = var_t.clamp_min(Y.MIN_VAR).sqrt()
        if kind == "lcb":
            a = m - beta * sd
        else:
            N = torch.distributions.Normal(torch.zeros((), dtype=f64), torch.ones((), dtype=f64))
            z = (sg * best - m) / sd
            a = -((sg * best - m) * torch.special.ndtr(z) + sd * N.log_prob(z).exp())
    da_dmu, da_dvar = torch.autograd.grad(a.sum(), (mu_t, var_t), allow_unused=True)
    return a.detach(), da_dmu[:, None] * gmu + da_dvar[:, None] * gvar


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("kind", Y.KINDS)
def test_acquisition_closed_forms_equal_autograd(kind, maximize):
    g = torch.Generator().manual_seed(5)
    B, d = 40, 4
    mu = torch.randn(B, generator=g, dtype=f64)
    gmu, gvar = torch.randn(B, d, generator=g, dtype=f64), torch.randn(B, d, generator=g, dtype=f64)
    var = 0.05 + torch.rand(B, generator=g, dtype=f64)
    var[:3] = torch.tensor([1e-7, 0.0, -1e-5], dtype=f64)            # clamped: sigma = 1e-3, grad sigma = 0
    a, ga = Y.acquisition(mu, gmu, var, gvar, kind, beta=1.7, best=0.3, maximize=maximize)
    a_ref, ga_ref = _acq_autograd(mu, gmu, var, gvar, kind, 1.7, 0.3, maximize)
    errs = dict(value=relmax(a, a_ref), gradient=relmax(ga, ga_ref))
    assert max(errs.values()) <= 1e-12, errs
    # mirrored model: the maximiser's acquisition of (mu, best) is the minimiser's of (-mu, -best)
    a_m, ga_m = Y.acquisition(-mu, -gmu, var, gvar, kind, beta=1.7, best=-0.3, maximize=not maximize)
    assert torch.equal(a_m, a) and torch.equal(ga_m, ga)


def test_ei_best_keeps_z_within_three():
    _, P64, x = Y.problem(3, 24, 2, 50)
    for maximize in (False, True):
        best = Y.ei_best(P64, x, maximize)
        mu, _, var, _ = Y.moments(P64, x)
        z = ((-best if maximize else best) - (-mu if maximize else mu)) / var.sqrt()
        assert z.abs().max().item() <= 3.0


# ------------------------------------------------------------------ the host surface
ENTRIES = ("dsvgp_var_route", "dsvgp_var_chunk", "dsvgp_var_weights_bytes", "dsvgp_var_workspace_bytes", "dsvgp_var_prepare",
           "dsvgp_var_predict", "dsvgp_acq_eval", "dsvgp_acq_descend_workspace_bytes", "dsvgp_acq_descend")


def test_exports_header_and_bindings(dsvgp):
    for name in ("VariancePredictor", "acquisition_candidates", "PathDescent"):
        assert hasattr(dsvgp, name), name
    assert dsvgp.shared_directional_vi.acquisition_candidates is dsvgp.directional_vi.acquisition_candidates
    for name in ("variance_predictor",):
        assert callable(getattr(dsvgp.ElboEngine, name))
    for name in ("variance", "variance_and_gradient", "acquisition", "descend"):
        assert callable(getattr(dsvgp.VariancePredictor, name))
    for name in ("posterior_variance", "posterior_variance_gradient", "acquisition", "acquisition_step"):
        assert callable(getattr(dsvgp.GPModel, name)), name
    with open(os.path.join(ROOT, "include", "dsvgp.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert re.search(r"^(int|size_t) %s\(" % name, header, re.M), name
        assert hasattr(dsvgp._lib.lib, name) and getattr(dsvgp._lib.lib, name).argtypes is not None, name


def test_route_and_chunk_rule(dsvgp):
    ops = dsvgp._ops
    # chunk = min(64, floor(12288 / ((p + 1) pad4(d)))) rounded down to a multiple of 8; fused iff d <= 32 and chunk >= 8
    for d, p in ((3, 2), (5, 0), (20, 5), (32, 32), (4, 95), (32, 95), (32, 47), (32, 48), (33, 2), (40, 3), (200, 0)):
        D = (d + 3) & ~3
        chunk = (min(64, 12288 // ((p + 1) * D)) & ~7) if d <= 32 else 0
        assert ops.var_chunk(d, p) == chunk, (d, p)
        assert ops.var_route(d, p) == ("fused" if chunk >= 8 else "composed"), (d, p)
        assert chunk * (p + 1) * D * 4 <= 48 * 1024
    assert ops.var_route(32, 32) == "fused" and ops.var_route(4, 95) == "fused"
    assert ops.var_route(32, 95) == "composed" and ops.var_route(33, 2) == "composed"
    for d, p in ((0, 2), (3, -1), (3, 96)):
        assert ops.var_route(d, p) is None and ops.var_chunk(d, p) == 0


def test_size_helpers_are_host_functions(dsvgp):
    ops = dsvgp._ops
    pad4 = lambda v: (v + 3) & ~3
    wb, ws, dw = ops.var_weights_bytes, ops.var_workspace_bytes, ops.acq_descend_workspace_bytes
    assert wb(100, 5, 2) == 4 * (8 + 8 + 100 * 8 + 200 * 8)
    assert 0 < wb(100, 5, 0) < wb(100, 5, 2) < wb(200, 5, 2) < wb(200, 50, 2)
    for args in ((0, 5, 2), (5, 0, 2), (5, 5, -1), (5, 5, 96)):
        assert wb(*args) == 0
    # fused route, as documented: the x pack, K_ZX and V; the same with and without the gradient
    for M, d, p, B in ((70, 3, 2, 70), (500, 20, 5, 4096), (9, 32, 32, 65)):
        Mp = M * (p + 1)
        want = 4 * (B * (pad4(d) + 4) + pad4(B) + 2 * Mp * pad4(B))
        assert ws(M, d, p, B, 0) == want and ws(M, d, p, B, 1) == want, (M, d, p, B)
    # composed route: the gradient adds G [B, M'] and the kernel backward's workspace
    for M, d, p, B in ((40, 33, 2, 70), (17, 40, 3, 129), (24, 200, 3, 40)):
        Mp = M * (p + 1)
        base = 4 * (B * (pad4(d) + 4) + pad4(B) + 2 * Mp * pad4(B) + -(-Mp // 256) * pad4(B))
        assert ws(M, d, p, B, 0) == base
        bwd = ops.kernel_bwd_rect_workspace_bytes(B, 0, M, p, d)
        assert bwd > 0 and ws(M, d, p, B, 1) == base + 4 * (B * pad4(Mp) + 4) + (bwd + 15) // 16 * 16
    # monotone in B; 0 for refused arguments and for an intermediate past 2^31 entries
    for M, d, p in ((70, 3, 2), (40, 33, 2)):
        for g in (0, 1):
            sizes = [ws(M, d, p, B, g) for B in (1, 2, 63, 64, 65, 1000, 4096)]
            assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
        sizes = [dw(M, d, p, B) for B in (1, 9, 64, 65, 512)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > ws(M, d, p, 1, 1)
    for args in ((0, 3, 2, 5), (5, 0, 2, 5), (5, 3, -1, 5), (5, 3, 96, 5), (5, 3, 2, 0)):
        assert ws(*args, 1) == 0 and ws(*args, 0) == 0 and dw(*args) == 0
    assert ws(3000, 3, 0, 1 << 20, 0) == 0                      # M' B = 3000 x 2^20 passes 2^31 entries: split the batch


# ------------------------------------------------------------------ refusals raised before any device work (a CPU-device engine)
def test_refusals_before_device_work(dsvgp):
    P, _, _ = Y.problem(3, 6, 2, 4)
    eng = dsvgp.ElboEngine(torch.device("cpu"))
    ard = dict(P, raw_lengthscale=torch.zeros(1, 3))
    with pytest.raises(ValueError, match="ARD"):
        eng.variance_predictor(ard)
    eng.kernel = "matern52"
    with pytest.raises(ValueError, match="Matern"):
        eng.variance_predictor(P)
    eng.kernel = "rbf"
    eng.whitening = "ciq"
    with pytest.raises(NotImplementedError, match="msMINRES"):
        eng.variance_predictor(P)
    eng64 = dsvgp._step64.ElboEngine64(torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="float64"):
        eng64.variance_predictor({k: v.double() for k, v in P.items()})
    # the existing refusal messages stand
    with pytest.raises(ValueError, match="mean_predictor is not built for ARD"):
        dsvgp.ElboEngine(torch.device("cpu")).mean_predictor(ard)
    pred = dsvgp.VariancePredictor.__new__(dsvgp.VariancePredictor)
    with pytest.raises(ValueError, match="kind"):
        dsvgp.VariancePredictor._scalars(pred, "ucb", None, None)
    with pytest.raises(ValueError, match="best"):
        dsvgp.VariancePredictor._scalars(pred, "ei", None, None)
