"""Two likelihood noises on the GPU (csrc/noise_classes.hip) against the float64 yardstick of tests/_noise_yardstick.py at
n_f != n_g (raw values -2.0 and 0.5), at the tolerances of tests/test_gpu_rect_train.py: the two-class likelihood entry, the per-output step
of every kernel family, the predictions, the weighted collapsed statistics with their solve / evaluate / refit, the harness and the
refusals.  Every reference is computed once per case and shared."""
import functools
import math
import types

import pytest
import torch

import dsvgp_oracle as O
import _noise_yardstick as NY
from _matern_yardstick import matern52_family, rbf_family
from test_gpu_rect_train import GRAD_TOL, LOSS_TOL, MU_TOL, VAR_TOL

pytestmark = pytest.mark.gpu
DN = NY.DNOISE
GUARD = 64


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _report(tag, errs):
    print("[parity] %s: %s" % (tag, ", ".join("%s %.2e" % (k, v) for k, v in errs.items())))


# ------------------------------------------------------------------ 1. the entry against the per-row formulas in float64
HYP = (0.7, 1.3, 0.2, 0.9)                  # ell, s, n_f, n_g
#              ncols    p
ENTRY_SHAPES = [(21, 2), (40, 0), (288, 95), (655, 4), (256 * 512 + 300, 4)]       # the last: a second grid-stride round of the 512 workgroups


@functools.lru_cache(maxsize=None)
def _entry_inputs(ncols, p, hyp=HYP):
    """(mu, var, y) float32 with a residual of non-zero mean (well-conditioned sums) and two rows whose var + noise is below the clamp"""
    g = torch.Generator().manual_seed(11 + ncols + p)
    mu = torch.randn(ncols, generator=g)
    y = mu + 0.8 + 0.6 * torch.randn(ncols, generator=g)
    var = 0.1 + torch.rand(ncols, generator=g)
    q = p + 1
    clamp_rows = [2 * q] + ([2 * q + 1] if p > 0 else [])                          # a value row and a derivative row
    for j in clamp_rows:
        var[j] = -(hyp[2] if j % q == 0 else hyp[3])
    return mu, var, y, tuple(clamp_rows)


@functools.lru_cache(maxsize=None)
def _entry_reference(ncols, p, mll_type, rows, hyp=HYP):
    """float64, gradients by autograd: (mu_bar, var_bar, varn, scalars[6])"""
    mu, var, y, _ = _entry_inputs(ncols, p, hyp)
    mu, var, y = (t.double().requires_grad_(True) for t in (mu, var, y))
    ell, s = hyp[0], hyp[1]
    n_f, n_g = (torch.tensor(float(torch.tensor(v, dtype=torch.float32)), dtype=torch.float64, requires_grad=True) for v in hyp[2:])
    isf = (torch.arange(ncols) % (p + 1)) == 0
    noise = torch.where(isf, n_f, n_g)
    vn = (var + noise).clamp_min(1e-6)
    r = y - mu
    if mll_type == 0:
        ll = -0.5 * ((r * r + vn) / noise + torch.log(noise) + math.log(2 * math.pi))
    else:
        tot = (vn + noise).clamp_min(1e-8)
        ll = -0.5 * (r * r / tot + torch.log(tot) + math.log(2 * math.pi))
    loss = -ll.sum() / rows
    mb, vb, d_f, d_g = torch.autograd.grad(loss, [mu, var, n_f, n_g])
    dg = torch.where(isf, torch.ones(()).double(), torch.tensor(1.0 / (ell * ell)).double())
    scal = torch.stack([ll.sum().detach(), d_f, mb.sum(), (vb * dg).sum(), (vb[~isf] * (-2.0 * s / ell ** 3)).sum(), d_g])
    return mb, vb, vn.detach(), scal


def _run_entry(dsvgp, dev, ncols, p, mll_type, rows, hyp=HYP, classes=True):
    """the outputs inside guard bands: (mu_bar, var_bar, varn, scalars, the four whole buffers)"""
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    mu, var, y, _ = _entry_inputs(ncols, p, HYP)
    bufs = [torch.full((ncols + 2 * GUARD,), 7.5, device=dev) for _ in range(3)] + [torch.full((8 + 2 * GUARD,), 7.5, device=dev)]
    outs = [b[GUARD:b.numel() - GUARD] for b in bufs]
    h = torch.tensor(hyp, device=dev)
    if classes:
        ops.likelihood_terms_classes(ctx, mu.to(dev), var.to(dev), y.to(dev), p, h, mll_type, rows, *outs,
                                     ops.likelihood_terms_classes_workspace(dev))
    else:
        ops.likelihood_terms(ctx, mu.to(dev), var.to(dev), y.to(dev), p, h, mll_type, rows, *outs)
    torch.cuda.synchronize()
    return outs + [bufs]


@pytest.mark.parametrize("mll_type", [0, 1])
@pytest.mark.parametrize("ncols,p", ENTRY_SHAPES)
def test_entry_matches_the_per_row_formulas(dsvgp, gpu_device, ncols, p, mll_type):
    rows = float(ncols + 5)                                                        # (global_rows need not be the local count)
    mb, vb, vn, scal, bufs = _run_entry(dsvgp, gpu_device, ncols, p, mll_type, rows)
    r_mb, r_vb, r_vn, r_scal = _entry_reference(ncols, p, mll_type, rows)
    errs = {"mu_bar": relmax(mb, r_mb), "var_bar": relmax(vb, r_vb), "varn": relmax(vn, r_vn)}
    for c in range(6):
        if r_scal[c].item() != 0.0:
            errs["scal%d" % c] = abs(scal[c].item() - r_scal[c].item()) / abs(r_scal[c].item())
    _report("classes entry (%d, %d) mll %d" % (ncols, p, mll_type), errs)
    assert errs["mu_bar"] <= 1e-6 and errs["var_bar"] <= 1e-6 and errs["varn"] <= 1e-6, errs
    assert all(v <= 1e-5 for k, v in errs.items() if k.startswith("scal")), errs
    assert scal[6].item() == 0.0 and scal[7].item() == 0.0
    if p == 0:                                                                     # all rows are value rows
        assert scal[5].item() == 0.0 and scal[4].item() == 0.0 and r_scal[5].item() == 0.0
    # the clamp: var + noise < 1e-6 on one row of each class -- no variance gradient there, the floor comes out
    for j in _entry_inputs(ncols, p)[3]:
        assert vb[j].item() == 0.0 and vn[j].item() == torch.tensor(1e-6, dtype=torch.float32).item() and mb[j].item() != 0.0
    # guard bands
    for b in bufs:
        assert bool((b[:GUARD] == 7.5).all()) and bool((b[-GUARD:] == 7.5).all())
    # two calls: bitwise equal
    again = _run_entry(dsvgp, gpu_device, ncols, p, mll_type, rows)
    assert all(torch.equal(u, v) for u, v in zip((mb, vb, vn, scal), again[:4]))


def test_entry_empty_batch_and_refusals(dsvgp, gpu_device):
    dev = gpu_device
    ops, lib = dsvgp._ops, dsvgp._lib.lib
    ctx = ops.Context.get(dev)
    n, p = 21, 2
    t = [torch.full((n,), 3.0, device=dev) for _ in range(6)]
    scal, hyp, ws = torch.full((8,), 9.0, device=dev), torch.tensor(HYP, device=dev), ops.likelihood_terms_classes_workspace(dev)
    P_ = lambda v: v.data_ptr()
    call = lambda ncols, mll, rows, ws_ptr, sc=scal: lib.dsvgp_likelihood_terms_classes(ctx.h, P_(t[0]), P_(t[1]), P_(t[2]), ncols, p, P_(hyp), mll, rows,
                                                                                          P_(t[3]), P_(t[4]), P_(t[5]), P_(sc), ws_ptr)
    assert call(0, 0, 8.0, P_(ws)) == 0                                            # no launch: the scalars are cleared, nothing else is touched
    torch.cuda.synchronize()
    assert bool((scal == 0).all()) and all(bool((v == 3.0).all()) for v in t)
    assert call(-1, 0, 8.0, P_(ws)) == -1 and call(n, 2, 8.0, P_(ws)) == -1 and call(n, 0, 0.0, P_(ws)) == -1 and call(n, 0, 8.0, None) == -1
    assert call(n, 0, 8.0, P_(ws) + 4) == -3                                       # DSVGP_EALIGN
    assert lib.dsvgp_likelihood_terms_classes(ctx.h, P_(t[0]), P_(t[1]), P_(t[2]), n, -1, P_(hyp), 0, 8.0, P_(t[3]), P_(t[4]), P_(t[5]), P_(scal),
                                              P_(ws)) == -1
    with pytest.raises(ValueError):
        ops.likelihood_terms_classes(ctx, t[0], t[1], t[2], p, hyp, 0, 8.0, t[3], t[4], t[5], scal, ws[:64])
    torch.cuda.synchronize()
    assert all(bool((v == 3.0).all()) for v in t)


# ------------------------------------------------------------------ 2. equal noises against the single-noise entry
@pytest.mark.parametrize("mll_type", [0, 1])
@pytest.mark.parametrize("ncols,p", [(21, 2), (288, 95), (655, 4)])
def test_equal_noises_are_the_single_noise_entry(dsvgp, gpu_device, ncols, p, mll_type):
    hyp = (HYP[0], HYP[1], HYP[2], HYP[2])
    rows = float(ncols)
    a = _run_entry(dsvgp, gpu_device, ncols, p, mll_type, rows, hyp=hyp)
    b = _run_entry(dsvgp, gpu_device, ncols, p, mll_type, rows, hyp=hyp, classes=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])       # element-wise, the same operations
    sa, sb = a[3].double().cpu(), b[3].double().cpu()
    errs = {"scal%d" % c: abs(sa[c] - sb[c]).item() / abs(sb[c]).item() for c in (0, 2, 3, 4)}
    errs["scal1 + scal5"] = abs(sa[1] + sa[5] - sb[1]).item() / abs(sb[1]).item()
    _report("classes entry at equal noises vs likelihood_terms (%d, %d) mll %d" % (ncols, p, mll_type), errs)
    assert all(errs["scal%d" % c] <= 1e-6 for c in (0, 2, 3, 4)) and errs["scal1 + scal5"] <= 1e-5, errs
    assert sa[1].item() != 0.0 and sa[5].item() != 0.0


# ------------------------------------------------------------------ 3. the step against the yardstick
#          name        d   M  p  pd   B  kernel      ard
STEPS = {"rbf":       (5, 24, 2, 2, 96, "rbf", False),
         "ard":       (4, 16, 2, 2, 48, "rbf", True),
         "matern":    (3, 12, 1, 1, 40, "matern52", False),
         "matern_ard": (3, 12, 1, 1, 40, "matern52", True),
         "pd4":       (5, 24, 2, 4, 96, "rbf", False),
         "pd0":       (5, 24, 2, 0, 96, "rbf", False)}


@functools.lru_cache(maxsize=None)
def _step_case(name):
    d, M, p, pd, B, kernel, ard = STEPS[name]
    P, x, y, D, nd = NY.problem(d, M, p, pd, B, ard=ard)
    if kernel == "matern52" and not ard:
        P["raw_lengthscale"] = P["raw_lengthscale"].reshape(1, 1)
    return P, x, y, D, nd, kernel, p, pd


@functools.lru_cache(maxsize=None)
def _step_reference(name, mll):
    P, x, y, D, nd, kernel, p, pd = _step_case(name)
    return NY.step(P, x, y, D, pd, nd, mll, matern52_family if kernel == "matern52" else rbf_family)


def _engine(dsvgp, dev, kernel="rbf"):
    eng = dsvgp.ElboEngine(dev)
    eng.kernel = kernel
    return eng


def _to(P, dev):
    return {k: v.to(dev) for k, v in P.items()}


@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
@pytest.mark.parametrize("name", sorted(STEPS))
def test_step_matches_the_yardstick(dsvgp, gpu_device, name, mll):
    dev = gpu_device
    P, x, y, D, nd, kernel, p, pd = _step_case(name)
    eng = _engine(dsvgp, dev, kernel)
    loss, grads, mu, varn = eng.loss_and_grads(_to(P, dev), x.to(dev), y.to(dev), None if D is None else D.to(dev), nd, mll)
    torch.cuda.synchronize()
    l_ref, g_ref, mu_ref, var_ref = _step_reference(name, mll)
    assert eng.c_step_used is False and sorted(grads) == sorted(NY.NAMES) and grads[DN].shape == P[DN].shape
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref), "varn": relmax(varn, var_ref)}
    for k in NY.NAMES:
        if pd == 0 and k == DN:
            continue
        errs[k] = relmax(grads[k].reshape(-1), g_ref[k].reshape(-1))
    _report("two-noise step %s %s" % (name, mll), errs)
    assert errs["loss"] < LOSS_TOL and errs["mu"] < MU_TOL and errs["varn"] < VAR_TOL, errs
    assert all(errs[k] < GRAD_TOL for k in NY.NAMES if k in errs), errs
    if pd == 0:
        assert grads[DN].item() == 0.0 and g_ref[DN].item() == 0.0                 # no derivative row: exactly zero
    else:
        assert grads[DN].abs().item() > 0 and grads["raw_noise"].abs().item() > 0


@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
def test_without_the_key_the_engine_returns_the_bits_it_returned_before(dsvgp, gpu_device, mll):
    dev = gpu_device
    P, x, y, D, nd, kernel, p, pd = _step_case("rbf")
    Pg, xg, yg, Dg = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)
    P1 = {k: v for k, v in Pg.items() if k != DN}
    never, given = _engine(dsvgp, dev), _engine(dsvgp, dev)
    given.loss_and_grads(Pg, xg, yg, Dg, nd, mll)
    for fast in (False, None):
        a = never.loss_and_grads(P1, xg, yg, Dg, nd, mll, fast=fast)
        b = given.loss_and_grads(P1, xg, yg, Dg, nd, mll, fast=fast)
        torch.cuda.synchronize()
        assert sorted(a[1]) == sorted(b[1]) == sorted(O.PARAM_NAMES) and never.c_step_used == given.c_step_used
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
        assert all(torch.equal(a[1][k], b[1][k]) for k in O.PARAM_NAMES)


# ------------------------------------------------------------------ 4. predictions
def _model(dsvgp, dev, P):
    """(GPModel, GaussianLikelihood(derivative_noise=True)) on the device holding the parameters ``P``, in eval mode"""
    dvi = dsvgp.directional_vi
    model = dvi.GPModel(P["inducing_points"].clone(), P["inducing_directions"].clone(), P["inducing_points"].shape[1]).to(dev)
    lik = dsvgp.gp_shim.GaussianLikelihood(derivative_noise=True).to(dev)
    model.variational_strategy._maybe_init()
    vd = model.variational_strategy._variational_distribution
    with torch.no_grad():
        vd.variational_mean.copy_(P["variational_mean"])
        vd.chol_variational_covar.copy_(P["chol_variational_covar"])
        model.mean_module.constant.copy_(P["constant"])
        model.covar_module.raw_outputscale.copy_(P["raw_outputscale"])
        model.covar_module.base_kernel.raw_lengthscale.copy_(P["raw_lengthscale"].reshape(model.covar_module.base_kernel.raw_lengthscale.shape))
        lik.noise_covar.raw_noise.copy_(P["raw_noise"])
        lik.noise_covar.raw_derivative_noise.copy_(P[DN])
    model.eval()
    lik.eval()
    return model, lik


@pytest.mark.parametrize("name", ["rbf", "pd4", "pd0", "ard", "matern"])
def test_predictions_carry_the_class_noise(dsvgp, gpu_device, name):
    dev = gpu_device
    P, x, y, D, nd, kernel, p, pd = _step_case(name)
    B, q = x.shape[0], pd + 1
    eng = _engine(dsvgp, dev, kernel)
    Pg, xg, Dg = _to(P, dev), x.to(dev), None if D is None else D.to(dev)
    mu_ref, S_noise, S_f = NY.predictive(P, x, D, pd, matern52_family if kernel == "matern52" else rbf_family)
    n_f, n_g = (v.item() for v in NY.class_noises({k: v.double() for k, v in P.items()}))
    mu, varn = eng.predict(Pg, xg, Dg)
    mu_j, Sigma = eng.predict_joint(Pg, xg, Dg)
    torch.cuda.synchronize()
    errs = {"mu": relmax(mu, mu_ref), "predict": relmax(varn, S_noise.diagonal()), "joint diagonal": relmax(Sigma.diagonal(), S_noise.diagonal()),
            "joint": relmax(Sigma, S_noise)}
    # the noise itself, against the same engine without the key (single noise n_f on every row)
    P1 = {k: v for k, v in Pg.items() if k != DN}
    _, var1 = eng.predict(P1, xg, Dg)
    delta = (varn - var1).reshape(B, q).cpu().double()
    assert bool((delta[:, 0] == 0).all())
    if pd:
        errs["n_g - n_f"] = (delta[:, 1:] - (n_g - n_f)).abs().max().item() / (n_g - n_f)
    if name in ("rbf", "pd4", "pd0"):                                              # (predict_blocks: the scalar RBF model)
        _, blocks = eng.predict_blocks(Pg, xg, Dg)
        torch.cuda.synchronize()
        want = torch.stack([S_noise[b * q:(b + 1) * q, b * q:(b + 1) * q] for b in range(B)])
        errs["blocks diagonal"] = relmax(blocks.diagonal(dim1=1, dim2=2), want.diagonal(dim1=1, dim2=2))
        errs["blocks"] = relmax(blocks, want)
    _report("two-noise predictions %s" % name, errs)
    assert errs["mu"] < MU_TOL and all(v < VAR_TOL for k, v in errs.items() if k != "mu"), errs


@pytest.mark.parametrize("name", ["rbf", "pd4", "pd0"])
def test_posterior_without_a_likelihood_is_q_f(dsvgp, gpu_device, name):
    dev = gpu_device
    P, x, y, D, nd, kernel, p, pd = _step_case(name)
    B, q = x.shape[0], pd + 1
    model, lik = _model(dsvgp, dev, P)
    xg, Dg = x.to(dev), None if D is None else D.to(dev)
    n_f, n_g = lik.noise.item(), lik.derivative_noise.item()
    rows = torch.tensor([n_f] + [n_g] * pd, dtype=torch.float64).repeat(B)
    with torch.no_grad():
        with_lik, without = model.posterior(xg, Dg, lik), model.posterior(xg, Dg)
        errs = {"variance": relmax(without.variance, with_lik.variance.double().cpu() - rows),
                "covariance diagonal": relmax(without.covariance_matrix.diagonal(), with_lik.covariance_matrix.diagonal().double().cpu() - rows),
                "blocks diagonal": relmax(without.point_covariances.diagonal(dim1=1, dim2=2).reshape(-1),
                                          with_lik.point_covariances.diagonal(dim1=1, dim2=2).reshape(-1).double().cpu() - rows)}
        roots, logdet = with_lik.point_roots
    torch.cuda.synchronize()
    _, S_noise, S_f = NY.predictive(P, x, D, pd)
    errs_ref = {"q(f) variance": relmax(without.variance, S_f.diagonal()), "variance": relmax(with_lik.variance, S_noise.diagonal())}
    want = torch.stack([S_noise[b * q:(b + 1) * q, b * q:(b + 1) * q] for b in range(B)])
    errs_ref["block roots"] = relmax(roots @ roots.transpose(1, 2), want)
    _report("posterior(likelihood=None) against the noisy one minus the class noise, %s" % name, errs)
    _report("posterior against the yardstick, %s" % name, errs_ref)
    assert all(v <= 1e-6 for v in errs.values()), errs
    assert all(v < VAR_TOL for v in errs_ref.values()), errs_ref


# ------------------------------------------------------------------ 5. the weighted collapsed statistics
COLLAPSED = (3, 10, 2, 240)                 # d, M, p, N
CUTS = (96, 192)                            # chunks of 96 / 96 / 48 points


@functools.lru_cache(maxsize=None)
def _collapsed_case(pd_name):
    d, M, p, N = COLLAPSED
    pd = d if pd_name == "all" else int(pd_name)
    P, x, y, D, nd = NY.problem(d, M, p, pd, N)
    stats = NY.statistics(P, x, y, D, pd)
    m_opt, L_opt = NY.optimum(stats, nd)
    return P, x, y, D, nd, pd, stats, m_opt, L_opt


def _accumulate(dsvgp, dev, P, x, y, D, pd, cuts=CUTS):
    acc = _engine(dsvgp, dev).collapsed_accumulator(_to(P, dev))
    xg, yg, Dg = x.to(dev), y.to(dev), D.to(dev)
    q = pd + 1
    bounds = [0] + list(cuts) + [x.shape[0]]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        acc.add(xg[lo:hi], yg[lo * q:hi * q], Dg[lo * pd:hi * pd])
    return acc


@pytest.mark.parametrize("pd_name", ["2", "all"])
def test_collapsed_statistics_solve_and_evaluate(dsvgp, gpu_device, pd_name):
    dev = gpu_device
    P, x, y, D, nd, pd, stats, m_opt, L_opt = _collapsed_case(pd_name)
    assert NY.cond_B(stats, nd) < 1e4
    acc = _accumulate(dsvgp, dev, P, x, y, D, pd)
    G, b, yy, dg, R = (t.cpu() for t in acc.statistics())
    assert R.item() == stats["R"] == y.numel() and acc._state[2].item() == x.shape[0]
    # the entry reads both noises from the float32 hyp (rho = hyp[2] / hyp[3] in float64): the statistics are compared at THOSE noises --
    # which are the float64 ones to float32 rounding -- and everything from the solve on against the float64 noises' own statistics
    dev_noises = tuple(acc._hyp[2:4].double().cpu().tolist())
    assert abs(dev_noises[0] - stats["n_f"].item()) <= 2e-7 * stats["n_f"].item() and abs(dev_noises[1] - stats["n_g"].item()) <= 2e-7 * stats["n_g"].item()
    exact, stats = stats, NY.statistics(P, x, y, D, pd, noises=dev_noises)
    errs = {"G": relmax(torch.tril(G), torch.tril(stats["G"])), "b": relmax(b, stats["b"]), "yy": abs(yy.item() - stats["yy"].item()) / stats["yy"].item(),
            "dg": abs(dg.item() - stats["dg"].item()) / abs(stats["dg"].item())}
    _report("weighted statistics pd = %s" % pd_name, errs)
    assert errs["G"] < 1e-2 and errs["b"] < 1e-2 and errs["yy"] < 1e-10 and errs["dg"] < 2e-5, errs
    stats = exact
    # solve against the yardstick's loss at ITS optimum; evaluate at the solve's optimum and at (0, I)
    want = NY.statistics_loss(stats, m_opt, L_opt, nd).item()
    res = acc.solve(nd)
    n = acc.Mp
    at_opt = acc.evaluate(res.variational_mean, res.chol_variational_covar, nd)
    zero = acc.evaluate(torch.zeros(n, device=dev), torch.eye(n, device=dev), nd)
    want_zero = NY.statistics_loss(stats, torch.zeros(n), torch.eye(n), nd).item()
    direct_zero = NY.step(dict(P, variational_mean=torch.zeros(n), chol_variational_covar=torch.eye(n)), x, y, D, pd, nd, "ELBO")[0].item()
    assert abs(want_zero - direct_zero) <= 1e-12 * abs(direct_zero)
    e = {"solve": abs(res.loss - want) / abs(want), "evaluate(m*, L_S*) vs solve": abs(at_opt.loss - res.loss) / abs(res.loss),
         "evaluate(0, I)": abs(zero.loss - want_zero) / abs(want_zero), "m*": relmax(res.variational_mean, m_opt)}
    t = res.terms
    _report("weighted solve / evaluate pd = %s (loss %.6f, log-noise shift %.6f)"
            % (pd_name, res.loss, stats["R_g"] * math.log(stats["n_f"].item() / stats["n_g"].item()) / (2 * stats["R"])), e)
    assert e["solve"] <= LOSS_TOL and e["evaluate(m*, L_S*) vs solve"] <= LOSS_TOL and e["evaluate(0, I)"] <= LOSS_TOL, e
    assert abs(t["loss"] + (t["log_likelihood"] / t["rows"] - t["kl"] / nd)) <= 1e-12 * abs(t["loss"])
    with pytest.raises(ValueError, match="derivative noise.*begin_backward"):
        acc.begin_backward(res)


@pytest.mark.parametrize("pd_name", ["2", "all"])
def test_equal_noises_give_the_unweighted_state(dsvgp, gpu_device, pd_name):
    dev = gpu_device
    P, x, y, D, nd, pd = _collapsed_case(pd_name)[:6]
    Pe = dict(P)
    Pe[DN] = P["raw_noise"].clone()                                               # rho = 1
    a = _accumulate(dsvgp, dev, Pe, x, y, D, pd)
    b = _accumulate(dsvgp, dev, {k: v for k, v in P.items() if k != DN}, x, y, D, pd)
    assert a._classes and not b._classes
    n = a.Mp
    Ta, Tb = (torch.tril(t._state[8:].view(n + 1, n + 1)).cpu() for t in (a, b))
    errs = {"T": relmax(Ta, Tb), "diag": abs(a._state[0].item() - b._state[0].item()) / abs(b._state[0].item())}
    _report("weighted state at rho = 1 vs dsvgp_collapsed_accumulate pd = %s" % pd_name, errs)
    assert errs["T"] <= 1e-12 and errs["diag"] <= 1e-12 and a._state[1].item() == b._state[1].item(), errs
    ra, rb = a.solve(nd), b.solve(nd)
    assert abs(ra.loss - rb.loss) <= 1e-12 * abs(rb.loss)                          # (log rho = 0: no shift)


@pytest.mark.parametrize("pd_name", ["2", "all"])
def test_fit_variational_leaves_no_variational_gradient(dsvgp, gpu_device, pd_name):
    dev = gpu_device
    dvi = dsvgp.directional_vi
    d, M, p, N = COLLAPSED
    P, x, y, D, nd, pd = _collapsed_case(pd_name)[:6]
    X = x.to(dev)
    Y = O.testfun(x).to(dev)
    model, lik = _model(dsvgp, dev, P)
    columns = dvi._collapsed_columns(N, d, pd, 96, 5)
    chunks = list(dvi._collapsed_chunks(X, Y, pd, 96, columns))
    assert [c[0].shape[0] for c in chunks] == [96, 96, 48]
    xs, ys, Ds = torch.cat([c[0] for c in chunks]), torch.cat([c[1] for c in chunks]), torch.cat([c[2] for c in chunks])

    def variational_grads():
        out = model.engine.loss_and_grads(model._param_dict(lik), xs, ys, Ds, float((d + 1) * N), "ELBO")
        torch.cuda.synchronize()
        return out[0].item(), out[1]["variational_mean"].abs().max().item(), torch.tril(out[1]["chol_variational_covar"]).abs().max().item()
    vd = model.variational_strategy._variational_distribution
    with torch.no_grad():
        vd.variational_mean.zero_()
        vd.chol_variational_covar.copy_(torch.eye(M * (p + 1)))
    l0, gm0, gl0 = variational_grads()
    res = dvi.fit_variational(model, lik, (X, Y), minibatch_size=96, data_directions="all" if pd_name == "all" else pd, seed=5)
    l1, gm1, gl1 = variational_grads()
    errs = {"variational_mean": gm1 / gm0, "chol_variational_covar": gl1 / gl0, "loss vs solve": abs(l1 - res.loss) / abs(res.loss)}
    _report("gradients after fit_variational over their size at (0, I), pd = %s (loss %.5f -> %.5f)" % (pd_name, l0, l1), errs)
    assert errs["variational_mean"] < GRAD_TOL and errs["chol_variational_covar"] < GRAD_TOL and errs["loss vs solve"] < LOSS_TOL, errs
    assert l1 < l0
    with pytest.raises(ValueError, match="derivative noise.*collapsed backward"):
        dvi.collapsed_loss_and_grads(model, lik, (X, Y), minibatch_size=96)


# ------------------------------------------------------------------ 6. the harness
def _noisy_dataset(n=600, d=2, sd_value=0.02, sd_gradient=0.5, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g)
    Y = O.testfun(X).clone()
    Y[:, 0] += sd_value * torch.randn(n, generator=g)
    Y[:, 1:] += sd_gradient * torch.randn(n, d, generator=g)
    return torch.utils.data.TensorDataset(X, Y)


def test_train_gp_learns_a_larger_derivative_noise(dsvgp, gpu_device):
    """d = 2, N = 600, value noise of standard deviation 0.02, gradient noise 0.5, 20 epochs of 6 steps.  The same optimisation on the
    float64 yardstick (torch Adam on tests/_noise_yardstick.py's ``forward``, its own permutations) ends at (n_f, n_g) = (0.453, 1.276) with
    a last-epoch mean loss of 6.058; with one noise it ends at n = 1.272 and 6.138 -- both assertions hold there with room to spare."""
    dvi = dsvgp.directional_vi
    train = _noisy_dataset()
    kw = dict(num_inducing=16, num_directions=2, minibatch_size=100, minibatch_dim=2, num_epochs=20, seed=0, verbose=False)

    def run(**extra):
        torch.manual_seed(0)
        history = []
        model, lik = dvi.train_gp(train, **kw, loss_history=history, **extra)
        last = torch.stack(history[-6:]).mean().item()
        assert len(history) == 120 and math.isfinite(last)
        return model, lik, last
    _, lik2, last2 = run(derivative_noise=True)
    _, lik1, last1 = run()
    assert lik2.has_derivative_noise and not lik1.has_derivative_noise
    n_f, n_g = lik2.noise.item(), lik2.derivative_noise.item()
    print("[noise classes] train_gp: two noises n_f %.4f n_g %.4f last-epoch loss %.4f; one noise n %.4f loss %.4f"
          % (n_f, n_g, last2, lik1.noise.item(), last1))
    assert n_g > n_f
    assert last2 < last1


# ------------------------------------------------------------------ 7. refusals on a GPU engine, and the model-level ones
def test_refusals_on_the_gpu(dsvgp, gpu_device):
    dev = gpu_device
    dvi = dsvgp.directional_vi
    P, x, y, D, nd, kernel, p, pd = _step_case("rbf")
    Pg, xg, yg, Dg = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)

    def engine(**attrs):
        eng = _engine(dsvgp, dev)
        for k, v in attrs.items():
            setattr(eng, k, v)
        return eng
    with pytest.raises(ValueError, match=r"derivative noise.*fast=True"):
        engine().loss_and_grads(Pg, xg, yg, Dg, nd, fast=True)
    for attrs, what in ((dict(capture_mode=True), "capture_mode"), (dict(deterministic=True), "deterministic"),
                        (dict(collective=types.SimpleNamespace(world=2, rank=0)), "world = 2"), (dict(whitening="ciq"), "CIQ"),
                        (dict(shared_directions=True), "shared"), (dict(data_outputs="values"), "values"),
                        (dict(missing_targets=True), "missing_targets")):
        with pytest.raises(ValueError, match=r"derivative noise.*%s" % what):
            engine(**attrs).loss_and_grads(Pg, xg, yg, Dg, nd)
        if what not in ("capture_mode", "deterministic"):
            with pytest.raises(ValueError, match=r"derivative noise.*%s" % what):
                engine(**attrs).predict(Pg, xg, Dg)
            with pytest.raises(ValueError, match=r"derivative noise.*%s" % what):
                engine(**attrs).collapsed_accumulator(Pg)
    P64 = {k: v.double() for k, v in Pg.items()}
    with pytest.raises(ValueError, match=r"derivative noise.*float"):
        dsvgp._step64.ElboEngine64(dev).loss_and_grads(P64, xg.double(), yg.double(), Dg.double(), nd)
    # the model level
    train = _noisy_dataset(n=60)
    for mod, args in ((dsvgp.dfree_directional_vi, ()), (dsvgp.shared_directional_vi, ()), (dsvgp.grad_svgp, (2,)), (dsvgp.traditional_vi, (2,))):
        with pytest.raises(ValueError, match="derivative_noise"):
            mod.train_gp(train, *args, derivative_noise=True)
    loop = dvi.setup_training(train, 8, 2, 30, 2, 1, seed=0, use_ngd=True)
    with pytest.raises(ValueError, match="derivative noise.*natural"):
        loop.set_derivative_noise()
    loop = dvi.setup_training(train, 8, 2, 30, 2, 1, seed=0)
    loop.graph = True
    with pytest.raises(ValueError, match="derivative noise.*graph"):
        loop.set_derivative_noise()
    loop.graph = None
    loop.set_missing_targets()
    with pytest.raises(ValueError, match="derivative noise.*missing_targets"):
        loop.set_derivative_noise()
    assert not loop.likelihood.has_derivative_noise
