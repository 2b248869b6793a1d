"""Posterior-variance predictor (ElboEngine.variance_predictor / VariancePredictor, csrc/predict_variance.hip): the variance of the
function value with its gradient, the confidence-bound / expected-improvement acquisitions on it and their on-device descent, held
to the float64 yardstick of tests/_variance_yardstick.py (pinned to the oracle in tests/test_variance_host.py) at the project's
predictive tolerance: 2e-4 of the largest entry (``TOL`` of tests/test_gpu_mean_predictor.py).  The shapes are the smallest at which
the kernels can go wrong (chunk and tile remainders, an exact fit, p = d, the chunk-sizing rule, the composed route); the measured
errors are printed as [parity] lines."""
import functools

import pytest
import torch

import dsvgp_oracle as O
import _variance_yardstick as Y
from _variance_yardstick import relmax

gpu = pytest.mark.gpu
TOL = 2e-4
f64 = torch.float64

#          d   M   p   B
FUSED = [(3, 70, 2, 70), (5, 64, 0, 64), (20, 65, 5, 130), (32, 9, 32, 65)]
CHUNK_RULE = [(4, 3, 95, 5)]                       # whichever route the helper reports
COMPOSED = [(33, 40, 2, 70), (40, 17, 3, 129)]
ALL = FUSED + CHUNK_RULE + COMPOSED
IDS = ["d%d-M%d-p%d-B%d" % s for s in ALL]
DESCENT = [(3, 40, 2, 9), (33, 20, 1, 5)]
DESCENT_IDS = ["d%d-M%d-p%d-B%d" % s for s in DESCENT]


def _report(tag, errs):
    print("[parity] %s: %s" % (tag, ", ".join("%s %.2e" % (k, v) for k, v in errs.items())))


@functools.lru_cache(maxsize=None)
def _case(d, M, p, B, small_variance=False):
    """(P fp32, P64, x fp64, (mu, grad mu, sigma^2, grad sigma^2) fp64): once per shape, shared, never changed"""
    P, P64, x = Y.problem(d, M, p, B, small_variance=small_variance)
    return P, P64, x, Y.moments(P64, x)


@functools.lru_cache(maxsize=None)
def _predictor(dsvgp, dev, d, M, p, B, small_variance=False):
    P, _, x, _ = _case(d, M, p, B, small_variance)
    pred = dsvgp.ElboEngine(dev).variance_predictor({k: v.to(dev) for k, v in P.items()})
    return pred, x.float().to(dev)


# ------------------------------------------------------------------ sigma^2 and its gradient, both routes
@gpu
@pytest.mark.parametrize("d,M,p,B", ALL, ids=IDS)
def test_variance_and_gradient(dsvgp, gpu_device, d, M, p, B):
    _, _, _, (_, _, var_ref, gvar_ref) = _case(d, M, p, B)
    pred, xg = _predictor(dsvgp, gpu_device, d, M, p, B)
    if (d, M, p, B) in FUSED:
        assert pred.route == "fused"
    elif (d, M, p, B) in COMPOSED:
        assert pred.route == "composed"
    assert pred.route == dsvgp._ops.var_route(d, p)
    var, gvar = pred.variance_and_gradient(xg)
    var_only = pred.variance(xg)                                       # grad_out = NULL
    var1, gvar1 = pred.variance_and_gradient(xg[:1])                   # B = 1
    var1_only = pred.variance(xg[:1])
    errs = dict(variance=relmax(var, var_ref), gradient=relmax(gvar, gvar_ref), variance_B1=relmax(var1, var_ref[:1]),
                gradient_B1=relmax(gvar1, gvar_ref[:1]))
    _report("variance d=%d M=%d p=%d B=%d (%s)" % (d, M, p, B, pred.route), errs)
    assert var.shape == (B,) and gvar.shape == (B, d) and var1.shape == (1,) and gvar1.shape == (1, d)
    assert torch.equal(var_only, var) and torch.equal(var1_only, var1)
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ the three acquisitions with their gradients
@gpu
@pytest.mark.parametrize("d,M,p,B", ALL, ids=IDS)
def test_acquisitions(dsvgp, gpu_device, d, M, p, B):
    _, P64, x, mom = _case(d, M, p, B)
    pred, xg = _predictor(dsvgp, gpu_device, d, M, p, B)
    errs = {}
    for maximize in (False, True):
        best = Y.ei_best(P64, x, maximize)
        sg = -1.0 if maximize else 1.0
        z = (sg * best - sg * mom[0]) / mom[2].sqrt()
        assert z.abs().max().item() <= 3.0, "the incumbent must keep |z| <= 3 on every test point"
        for kind in Y.KINDS:
            a_ref, ga_ref = Y.acquisition(*mom, kind, beta=2.0, best=best, maximize=maximize)
            a, ga = pred.acquisition(xg, kind, beta=2.0, best=best, maximize=maximize, gradients=True)
            a_only = pred.acquisition(xg, kind, beta=torch.tensor(2.0, device=gpu_device), best=best, maximize=maximize)
            tag = kind + ("_max" if maximize else "")
            errs[tag] = relmax(a, a_ref)
            errs[tag + "_grad"] = relmax(ga, ga_ref)
            errs[tag + "_values_only"] = relmax(a_only, a_ref)
            assert a.shape == (B,) and ga.shape == (B, d) and a_only.shape == (B,)
    _report("acquisitions d=%d M=%d p=%d B=%d" % (d, M, p, B), errs)
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ sigma^2 << s
@gpu
def test_small_variance(dsvgp, gpu_device):
    d, M, p, B = 3, 40, 2, 50
    _, P64, _, (_, _, var_ref, gvar_ref) = _case(d, M, p, B, True)
    pred, xg = _predictor(dsvgp, gpu_device, d, M, p, B, True)
    s = O.constrained(P64)[1].item()
    var, gvar = pred.variance_and_gradient(xg)
    errs = dict(variance=relmax(var, var_ref), gradient=relmax(gvar, gvar_ref))
    _report("small variance: min sigma^2 %.3e (yardstick %.3e), s %.3f" % (var.min().item(), var_ref.min().item(), s), errs)
    assert var_ref.max().item() < 0.2 * s
    assert var.min().item() >= 1e-4 - 2e-4 * s
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ what users get today
@gpu
@pytest.mark.parametrize("d,M,p,B", [FUSED[0], COMPOSED[0]], ids=[IDS[0], IDS[5]])
def test_agrees_with_predict(dsvgp, gpu_device, d, M, p, B):
    P, _, _, _ = _case(d, M, p, B)
    pred, xg = _predictor(dsvgp, gpu_device, d, M, p, B)
    _, varn = dsvgp.ElboEngine(gpu_device).predict({k: v.to(gpu_device) for k, v in P.items()}, xg, None)
    errs = dict(variance_with_noise=relmax(pred.variance(xg, with_noise=True), varn))
    _report("variance(with_noise) vs predict d=%d" % d, errs)
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ natural parameters, shared directions
@gpu
def test_natural_parameters(dsvgp, gpu_device):
    d, M, p, B = 5, 30, 2, 40
    P, P64, x, (mu_ref, gmu_ref, var_ref, gvar_ref) = _case(d, M, p, B)
    L_S = torch.tril(P64["chol_variational_covar"])
    Sinv = torch.cholesky_inverse(L_S)
    Pn = {k: v for k, v in P.items() if k not in ("variational_mean", "chol_variational_covar")}
    Pn["natural_vec"] = (Sinv @ P64["variational_mean"]).float()
    Pn["natural_mat"] = (-0.5 * Sinv).float()
    # (the yardstick on the moments these float32 natural parameters define)
    m, LS = O.natural_to_mu_chol(Pn["natural_vec"].double(), Pn["natural_mat"].double())
    Pc = dict(P64, variational_mean=m, chol_variational_covar=LS)
    mu_ref, gmu_ref, var_ref, gvar_ref = Y.moments(Pc, x)
    pred = dsvgp.ElboEngine(gpu_device).variance_predictor({k: v.to(gpu_device) for k, v in Pn.items()})
    xg = x.float().to(gpu_device)
    var, gvar = pred.variance_and_gradient(xg)
    a, ga = pred.acquisition(xg, "lcb", beta=2.0, gradients=True)
    a_ref, ga_ref = Y.acquisition(mu_ref, gmu_ref, var_ref, gvar_ref, "lcb", beta=2.0)
    errs = dict(variance=relmax(var, var_ref), gradient=relmax(gvar, gvar_ref), lcb=relmax(a, a_ref), lcb_grad=relmax(ga, ga_ref))
    _report("natural parameters", errs)
    assert max(errs.values()) < TOL, errs


@gpu
def test_shared_directions(dsvgp, gpu_device):
    d, M, p, B = 4, 25, 2, 33
    g = torch.Generator().manual_seed(3)
    P, _, x = Y.problem(d, M, 0, B)
    Ps = dict(P)
    Ps["inducing_directions"] = torch.randn(p, d, generator=g)
    Ps["variational_mean"] = 0.2 * torch.randn(M + p, generator=g)
    Ps["chol_variational_covar"] = torch.eye(M + p)
    P64 = Y.expanded({k: v.double() for k, v in Ps.items()}, True)
    mu_ref, gmu_ref, var_ref, gvar_ref = Y.moments(P64, x, no_middle=True)
    eng = dsvgp.ElboEngine(gpu_device)
    eng.shared_directions = True
    pred = eng.variance_predictor({k: v.to(gpu_device) for k, v in Ps.items()})
    xg = x.float().to(gpu_device)
    var, gvar = pred.variance_and_gradient(xg)
    a, ga = pred.acquisition(xg, "lcb_var", beta=1.5, gradients=True)
    a_ref, ga_ref = Y.acquisition(mu_ref, gmu_ref, var_ref, gvar_ref, "lcb_var", beta=1.5)
    errs = dict(variance=relmax(var, var_ref), gradient=relmax(gvar, gvar_ref), lcb_var=relmax(a, a_ref), lcb_var_grad=relmax(ga, ga_ref))
    _report("shared directions (S = 0)", errs)
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ determinism
@gpu
@pytest.mark.parametrize("d,M,p,B", [FUSED[2], COMPOSED[1]], ids=[IDS[2], IDS[6]])
def test_two_identical_calls_are_bitwise_equal(dsvgp, gpu_device, d, M, p, B):
    pred, xg = _predictor(dsvgp, gpu_device, d, M, p, B)
    lower, upper = torch.zeros(d, device=gpu_device), torch.ones(d, device=gpu_device)
    for _ in range(2):
        (v1, g1), (v2, g2) = pred.variance_and_gradient(xg), pred.variance_and_gradient(xg)
        assert torch.equal(v1, v2) and torch.equal(g1, g2)
        for kind in Y.KINDS:
            (a1, ga1), (a2, ga2) = (pred.acquisition(xg, kind, best=0.2, gradients=True) for _ in range(2))
            assert torch.equal(a1, a2) and torch.equal(ga1, ga2)
            r1, r2 = (pred.descend(xg[:7], lower, upper, kind, best=0.2, iterations=3) for _ in range(2))
            assert all(torch.equal(s, t) for s, t in zip(r1, r2))


# ------------------------------------------------------------------ the descent
@gpu
@pytest.mark.parametrize("maximize", [False, True], ids=["min", "max"])
@pytest.mark.parametrize("kind", Y.KINDS)
@pytest.mark.parametrize("d,M,p,B", DESCENT, ids=DESCENT_IDS)
def test_descent(dsvgp, gpu_device, d, M, p, B, kind, maximize):
    dev = gpu_device
    _, P64, x, _ = _case(d, M, p, B)
    pred, xg = _predictor(dsvgp, dev, d, M, p, B)
    x0 = 1.2 * xg - 0.1                                              # some starts lie outside the box: clamped
    lower, upper = torch.zeros(d, device=dev), torch.ones(d, device=dev)
    best = Y.ei_best(P64, x, maximize)
    kw = dict(kind=kind, beta=2.0, best=best, maximize=maximize)
    fresh = lambda pts: pred.acquisition(pts, gradients=True, **kw)
    # iterations = 0: the clamped start with its value
    start = pred.descend(x0, lower, upper, iterations=0, **kw)
    assert torch.equal(start.x, x0.clamp(0.0, 1.0)) and not torch.equal(start.x, x0)
    a0, g0 = fresh(start.x)
    assert torch.equal(start.values, a0) and torch.equal(start.gradients, g0)
    assert (start.accepted == 0).all() and (start.steps > 0).all()
    # one iteration at a time: inside the box, never worse
    states = [start]
    for _ in range(6):
        states.append(pred.descend(None, lower, upper, iterations=1, state=states[-1], **kw))
    for prev, cur in zip(states, states[1:]):
        assert (cur.x >= lower).all() and (cur.x <= upper).all()
        assert (cur.values <= prev.values).all()
        assert ((cur.accepted - prev.accepted) >= 0).all() and ((cur.accepted - prev.accepted) <= 1).all()
    # 6 iterations = 3 + 3 with state = 6 x 1, bitwise
    full = pred.descend(x0, lower, upper, iterations=6, **kw)
    half = pred.descend(None, lower, upper, iterations=3, state=pred.descend(x0, lower, upper, iterations=3, **kw), **kw)
    assert all(torch.equal(s, t) for s, t in zip(full, half))
    assert all(torch.equal(s, t) for s, t in zip(full, states[-1]))
    assert full.x.shape == (B, d) and full.values.shape == (B,) and full.gradients.shape == (B, d)
    assert int(full.accepted.sum()) > 0 and (full.values < start.values).any()
    # the returned values are the acquisition at the returned points, and that is the yardstick's
    a, ga = fresh(full.x)
    assert torch.equal(full.values, a) and torch.equal(full.gradients, ga)
    a_ref, ga_ref = Y.acquisition_at(P64, full.x.double().cpu(), kind, 2.0, best, maximize)
    errs = dict(value=relmax(a, a_ref), gradient=relmax(ga, ga_ref))
    _report("descent d=%d %s%s: accepted %d of %d" % (d, kind, " max" if maximize else "", int(full.accepted.sum()), 6 * B), errs)
    assert max(errs.values()) < TOL, errs
    assert torch.equal(x0, 1.2 * xg - 0.1)                           # the starts are not modified


# ------------------------------------------------------------------ candidates -> refined step, engine and model level
@gpu
@pytest.mark.parametrize("kind", Y.KINDS)
def test_acquisition_candidates(dsvgp, gpu_device, kind):
    d, M, p, B = 3, 40, 2, 9
    _, P64, x, _ = _case(d, M, p, B)
    pred, _ = _predictor(dsvgp, gpu_device, d, M, p, B)
    cand = torch.rand(200, d, generator=torch.Generator().manual_seed(11))
    lower, upper = torch.zeros(d), torch.ones(d)
    best = Y.ei_best(P64, x)
    x_next, a_next, a_cand = dsvgp.acquisition_candidates(pred, cand, lower, upper, kind, beta=2.0, best=best, num_starts=8, iterations=10)
    a_all = pred.acquisition(cand.to(gpu_device), kind, beta=2.0, best=best)
    a_ref, _ = Y.acquisition_at(P64, x_next.double().cpu()[None], kind, 2.0, best)
    scale = Y.acquisition_at(P64, cand.double(), kind, 2.0, best)[0].abs().max().item()
    err = abs(a_next.item() - a_ref.item()) / scale
    _report("acquisition_candidates %s: %.5f -> %.5f" % (kind, a_cand.item(), a_next.item()), dict(value=err))
    assert x_next.shape == (d,) and a_next.dim() == 0 and (x_next >= 0).all() and (x_next <= 1).all()
    assert a_cand.item() == a_all.min().item() and a_next.item() <= a_cand.item()
    assert err < TOL


@gpu
def test_model_level(dsvgp, gpu_device, capsys):
    from torch.utils.data import TensorDataset
    torch.manual_seed(0)
    n, dim = 600, 2
    train_x = torch.rand(n, dim)
    model, likelihood = dsvgp.train_gp(TensorDataset(train_x, O.testfun(train_x)), num_inducing=20, num_directions=2, minibatch_size=200,
                                       minibatch_dim=2, num_epochs=1, inducing_data_initialization=False, tqdm=False, verbose=False,
                                       seed=0)
    capsys.readouterr()
    model.eval()
    likelihood.eval()
    dev = gpu_device
    xg = torch.rand(150, dim, generator=torch.Generator().manual_seed(2)).to(dev)
    P64 = {k: v.detach().double().cpu() for k, v in model._param_dict(None).items()}
    mu_ref, gmu_ref, var_ref, gvar_ref = Y.moments(P64, xg.double().cpu())
    with torch.no_grad():
        varn_old = model.posterior(xg, likelihood=likelihood).variance
    a_ref, _ = Y.acquisition(mu_ref, gmu_ref, var_ref, gvar_ref, "lcb", beta=2.0)
    errs = {"posterior_variance": relmax(model.posterior_variance(xg), var_ref),
            "posterior_variance_gradient": relmax(model.posterior_variance_gradient(xg), gvar_ref),
            "posterior_variance(likelihood) vs posterior().variance": relmax(model.posterior_variance(xg, likelihood), varn_old),
            "acquisition": relmax(model.acquisition(xg, "lcb", beta=2.0), a_ref)}
    _report("model level", errs)
    assert max(errs.values()) < TOL, errs
    lower, upper = torch.zeros(dim, device=dev), torch.ones(dim, device=dev)
    x_next, a_next, a_cand = model.acquisition_step(xg, lower, upper, "lcb", beta=2.0, num_starts=4, iterations=10)
    a_y, _ = Y.acquisition_at(P64, x_next.double().cpu()[None], "lcb", 2.0)
    assert a_next.item() <= a_cand.item() and abs(a_next.item() - a_y.item()) / a_ref.abs().max().item() < TOL
    # eval mode: the predictor is cached; an in-place parameter change invalidates it
    assert model._variance_predictor() is model._variance_predictor()
    var_old = model.posterior_variance(xg)
    with torch.no_grad():
        model.variational_strategy._variational_distribution.chol_variational_covar.mul_(1.5)
    var_new = model.posterior_variance(xg)
    assert not torch.equal(var_new, var_old)
    assert torch.equal(var_new, model.engine.variance_predictor(model._param_dict(None)).variance(xg))


# ------------------------------------------------------------------ refusals on the device
@gpu
def test_refusals(dsvgp, gpu_device):
    dev = gpu_device
    P, _, x, _ = _case(3, 40, 2, 9)
    Pg = {k: v.to(dev) for k, v in P.items()}
    with pytest.raises(ValueError, match="ARD"):
        dsvgp.ElboEngine(dev).variance_predictor(dict(Pg, raw_lengthscale=torch.zeros(1, 3, device=dev)))
    eng = dsvgp.ElboEngine(dev)
    eng.kernel = "matern52"
    with pytest.raises(ValueError, match="Matern"):
        eng.variance_predictor(Pg)
    eng = dsvgp.ElboEngine(dev)
    eng.whitening = "ciq"
    with pytest.raises(NotImplementedError, match="msMINRES"):
        eng.variance_predictor(Pg)
    with pytest.raises(NotImplementedError, match="float64"):
        dsvgp.ElboEngine64(dev).variance_predictor({k: v.double() for k, v in Pg.items()})
    pred, xg = _predictor(dsvgp, dev, 3, 40, 2, 9)
    lower, upper = torch.zeros(3, device=dev), torch.ones(3, device=dev)
    for call in (lambda: pred.variance(x.float()), lambda: pred.variance_and_gradient(x.float()), lambda: pred.acquisition(x.float(), "lcb"),
                 lambda: pred.descend(x.float(), lower, upper, "lcb"), lambda: pred.descend(xg, lower.cpu(), upper, "lcb")):
        with pytest.raises(dsvgp._lib.DsvgpError):
            call()
    with pytest.raises(ValueError, match="best"):
        pred.acquisition(xg, "ei")
    with pytest.raises(ValueError, match="kind"):
        pred.acquisition(xg, "ucb")
    # the C entries refuse empty problems and unknown kinds like their neighbours
    import ctypes as C
    lib, ctx = dsvgp._lib.lib, dsvgp._ops.Context.get(dev)
    vp = lambda t: C.c_void_p(t.data_ptr())
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    out = torch.empty(16, device=dev)
    args = lambda M, d, p, B: (ctx.h, vp(pred.weights), vp(pred.Q), 120, vp(pred.packZ[0]), vp(pred.packZ[1]), vp(pred.hyp), M, d, p, vp(xg), B,
                               vp(out), None, vp(ws))
    for bad in ((0, 3, 2, 9), (40, 0, 2, 9), (40, 3, -1, 9), (40, 3, 96, 9), (40, 3, 2, 0)):
        assert lib.dsvgp_var_predict(*args(*bad)) == -1, bad
    assert lib.dsvgp_acq_eval(ctx.h, 3, 0, vp(out), vp(out), vp(out), None, vp(out), None, 4, 3, vp(out), None) == -1
