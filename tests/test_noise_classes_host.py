"""Two likelihood noises, host side: the float64 yardstick of tests/_noise_yardstick.py against the committed
yardsticks at equal noises, its weighted statistics against its own direct objective, the closed-form optimum, the C ABI's declarations and
bindings, the refusals (checked on a CPU-device engine: every refusal comes before any device work), the likelihood's parameter and the
harness keywords."""
import inspect
import os
import re
import types

import pytest
import torch

import dsvgp_oracle as O
import _noise_yardstick as NY
from _matern_yardstick import matern52_family, matern_elbo, rbf_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dsvgp_likelihood_terms_classes_workspace_bytes", "dsvgp_likelihood_terms_classes", "dsvgp_collapsed_accumulate_classes")
#          d  M   p  pd  N
SHAPES = [(3, 10, 2, 2, 60), (2, 8, 1, 3, 40)]
FAMILIES = {"rbf": rbf_family, "matern52": matern52_family}


def relmax(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _problem(shape, raw):
    d, M, p, pd, N = shape
    return NY.problem(d, M, p, pd, N, raw=raw) + (pd,)


@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES)
def test_equal_noises_reproduce_the_single_noise_yardstick(shape, family, mll):
    P, x, y, D, nd, pd = _problem(shape, (-0.5, -0.5))
    loss, grads, mu, varn = NY.step(P, x, y, D, pd, nd, mll, FAMILIES[family])
    P1 = {k: v.double() for k, v in P.items() if k != NY.DNOISE}
    l_ref, g_ref, mu_ref, var_ref = matern_elbo(P1, x.double(), y.double(), D.double(), pd, nd, mll, FAMILIES[family])
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref), "varn": relmax(varn, var_ref)}
    for k in O.PARAM_NAMES:
        if k != "raw_noise":
            errs[k] = relmax(grads[k].reshape(-1), g_ref[k].reshape(-1))
    errs["noise sum"] = relmax(grads["raw_noise"] + grads[NY.DNOISE], g_ref["raw_noise"])
    print("[parity] two-noise yardstick at equal noises vs matern_forward %s %s %s: %s" % (shape, family, mll, errs))
    assert max(errs.values()) <= 1e-12, errs
    assert grads["raw_noise"].abs().item() > 0 and grads[NY.DNOISE].abs().item() > 0


@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
def test_equal_noises_reproduce_the_oracle(mll):
    """the oracle's ``elbo_forward`` is the scalar RBF model with pd = p: the first shape"""
    P, x, y, D, nd, pd = _problem(SHAPES[0], (-0.5, -0.5))
    loss, grads, mu, varn = NY.step(P, x, y, D, pd, nd, mll, rbf_family)
    P1 = {k: v.double() for k, v in P.items() if k != NY.DNOISE}
    l_ref, g_ref, mu_ref, var_ref = O.elbo_loss_and_grads(P1, x.double(), y.double(), D.double(), nd, mll)
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref), "varn": relmax(varn, var_ref)}
    for k in O.PARAM_NAMES:
        if k != "raw_noise":
            errs[k] = relmax(grads[k].reshape(-1), g_ref[k].reshape(-1))
    errs["noise sum"] = relmax(grads["raw_noise"] + grads[NY.DNOISE], g_ref["raw_noise"])
    print("[parity] two-noise yardstick at equal noises vs the oracle %s: %s" % (mll, errs))
    assert max(errs.values()) <= 1e-12, errs


def test_value_only_data_give_no_derivative_noise_gradient():
    P, x, y, D, nd = NY.problem(3, 10, 2, 0, 30)
    loss, grads, mu, varn = NY.step(P, x, y, D, 0, nd, "ELBO")
    assert grads[NY.DNOISE].item() == 0.0 and grads["raw_noise"].abs().item() > 0


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES)
def test_weighted_statistics_and_their_optimum(shape, family):
    raw = (NY.raw_of(0.05), NY.raw_of(0.8))
    P, x, y, D, nd, pd = _problem(shape, raw)
    P["raw_noise"], P[NY.DNOISE] = (torch.tensor([v], dtype=torch.float64) for v in raw)          # (not rounded to float32)
    fam = FAMILIES[family]
    stats = NY.statistics(P, x, y, D, pd, fam)
    assert abs(stats["n_f"].item() - 0.05) < 1e-12 and abs(stats["n_g"].item() - 0.8) < 1e-12
    assert NY.cond_B(stats, nd) < 1e4
    n = stats["G"].shape[0]

    def direct(m, L_S):
        Q = dict(P, variational_mean=m, chol_variational_covar=L_S)
        return NY.step(Q, x, y, D, pd, nd, "ELBO", fam)

    # the statistics-form loss equals the direct one at a generic q(u), at (0, I) and at the optimum; without the log correction it does not
    g = torch.Generator().manual_seed(17)
    m_any = 0.3 * torch.randn(n, generator=g, dtype=torch.float64)
    L_any = torch.tril(torch.eye(n, dtype=torch.float64) + 0.05 * torch.randn(n, n, generator=g, dtype=torch.float64))
    m_opt, L_opt = NY.optimum(stats, nd)
    for tag, m, L_S in (("generic", m_any, L_any), ("(0, I)", torch.zeros(n, dtype=torch.float64), torch.eye(n, dtype=torch.float64)),
                        ("optimum", m_opt, L_opt)):
        want = direct(m, L_S)[0].item()
        got = NY.statistics_loss(stats, m, L_S, nd).item()
        bare = NY.statistics_loss(stats, m, L_S, nd, correction=False).item()
        print("[parity] statistics-form loss %s %s %s: %.3e (uncorrected %.3e)" % (shape, family, tag, abs(got - want) / abs(want),
                                                                                 abs(bare - want) / abs(want)))
        assert abs(got - want) <= 1e-12 * abs(want)
        assert abs(bare - want) > 1e-3 * abs(want)
        shift = stats["R_g"] * torch.log(stats["n_f"] / stats["n_g"]).item() / (2.0 * stats["R"])
        assert abs((bare - got) - shift) <= 1e-12 * abs(want)
    # the gradient of the direct objective with respect to (m, L_S) vanishes at the weighted closed-form optimum
    g0 = direct(torch.zeros(n, dtype=torch.float64), torch.eye(n, dtype=torch.float64))[1]
    g1 = direct(m_opt, L_opt)[1]
    for k in ("variational_mean", "chol_variational_covar"):
        ratio = g1[k].abs().max().item() / g0[k].abs().max().item()              # (above the diagonal both are exactly 0)
        print("[parity] gradient at the weighted optimum over its size at (0, I), %s %s %s: %.2e" % (shape, family, k, ratio))
        assert ratio <= 1e-10, (k, ratio)
    assert direct(m_opt, L_opt)[0].item() < direct(m_any, L_any)[0].item()


def test_new_symbols_are_declared_and_bound(dsvgp):
    with open(os.path.join(ROOT, "include", "dsvgp.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
        assert name in dsvgp._lib.SIGNATURES and hasattr(dsvgp._lib.lib, name), name
    for name in ("likelihood_terms_classes", "likelihood_terms_classes_workspace", "collapsed_accumulate_classes_"):
        assert callable(getattr(dsvgp._ops, name)), name
    lib = dsvgp._lib.lib
    assert lib.dsvgp_likelihood_terms_classes_workspace_bytes() >= 512 * 4 * 6        # (a fixed size: it takes no argument to refuse)
    assert lib.dsvgp_collapsed_state_bytes(0) == 0 and lib.dsvgp_collapsed_workspace_bytes(0) == 0
    # null pointers, negative sizes, a bad objective, rows that are no multiple of pd + 1: DSVGP_EINVAL (-1), before anything is touched
    assert lib.dsvgp_likelihood_terms_classes(None, None, None, None, 8, 2, None, 0, 8.0, None, None, None, None, None) == -1
    assert lib.dsvgp_collapsed_accumulate_classes(None, None, 4, None, 8, 8, 1, None, None, None, None) == -1
    with open(os.path.join(ROOT, "gp-derivatives-variational-inference_amd", "csrc", "noise_classes.hip")) as f:
        src = f.read()
    assert "atomicAdd" not in src and "Bp % (pd + 1)" in src


def test_parameter_names_and_the_likelihood(dsvgp):
    step = dsvgp._step
    assert step.PARAM_NAMES[-1] == "raw_noise" and step.NGD_PARAM_NAMES[-1] == "raw_noise"
    assert step.DERIVATIVE_NOISE == "raw_derivative_noise" not in step.PARAM_NAMES + step.NGD_PARAM_NAMES
    shim = dsvgp.gp_shim
    plain, two = shim.GaussianLikelihood(), shim.GaussianLikelihood(derivative_noise=True)
    assert list(plain.state_dict()) == ["noise_covar.raw_noise"] and not plain.has_derivative_noise
    assert sorted(set(two.state_dict()) - set(plain.state_dict())) == ["noise_covar.raw_derivative_noise"] and len(two.state_dict()) == 2
    raw = two.noise_covar.raw_derivative_noise
    assert tuple(raw.shape) == (1,) and raw.dtype == torch.float32 and torch.equal(raw.detach(), plain.noise_covar.raw_noise.detach())
    assert abs(two.derivative_noise.item() - (torch.nn.functional.softplus(torch.zeros(())) + 1e-4).item()) < 1e-7
    with pytest.raises(AttributeError):
        plain.derivative_noise
    dvi = dsvgp.directional_vi
    Z, V = torch.rand(4, 3), torch.eye(3)[:2].repeat(4, 1)
    model = dvi.GPModel(Z, V, 3)
    assert model._param_names() == step.PARAM_NAMES == model._param_names(plain) and len(model._param_list(plain)) == len(step.PARAM_NAMES)
    assert model._param_names(two) == step.PARAM_NAMES + ("raw_derivative_noise",)
    assert model._param_list(two)[-1] is raw and "raw_derivative_noise" in model._param_dict(two)
    assert "raw_derivative_noise" not in model._param_dict(plain) and "raw_derivative_noise" not in model._param_dict(None)


def test_pinned_signatures_and_harness_keywords(dsvgp):
    dvi = dsvgp.directional_vi
    sig = lambda fn: list(inspect.signature(fn).parameters)
    assert sig(dvi.setup_training)[-1] == "ard_num_dims" and sig(dvi.train_gp)[-1] == "args" and sig(dvi.train_collapsed)[-1] == "missing_targets"
    assert sig(dvi.GPModel.__init__) == ["self", "inducing_points", "inducing_directions", "dim", "learn_inducing_locations", "ard_num_dims",
                                         "kwargs"]
    for fn in (dvi.setup_training, dvi.train_collapsed, dvi.collapsed_loss_and_grads, dvi.fit_variational, dvi.TrainLoop.refit_variational,
               dvi.GPModel.__init__):
        assert "derivative_noise" not in inspect.signature(fn).parameters
    assert "derivative_noise" in inspect.getsource(dvi.train_gp) and sig(dvi.TrainLoop.set_derivative_noise) == ["self"]
    # the loop's switch: refusals on its switches alone, then the parameter in the likelihood's optimiser group
    Z, V = torch.rand(4, 3), torch.eye(3)[:2].repeat(4, 1)

    def loop(model, **kw):
        lik = dsvgp.gp_shim.GaussianLikelihood()
        opt = types.SimpleNamespace(param_groups=[{"params": []}, {"params": list(lik.parameters())}])
        base = dict(model=model, likelihood=lik, dfree=False, full_gradient=False, dp=None, X=torch.rand(2, 3), graph=None,
                    hyperparameter_optimizer=opt)
        base.update(kw)
        return types.SimpleNamespace(**base)
    ok = loop(dvi.GPModel(Z, V, 3))
    ok.likelihood.noise_covar.raw_noise.data.fill_(-1.5)
    dvi._enable_derivative_noise(ok)
    raw = ok.likelihood.noise_covar.raw_derivative_noise
    assert ok.likelihood.has_derivative_noise and raw.item() == -1.5 and ok.hyperparameter_optimizer.param_groups[-1]["params"][-1] is raw
    dvi._enable_derivative_noise(ok)
    assert len(ok.hyperparameter_optimizer.param_groups[-1]["params"]) == 2                      # (registered once)
    for bad in (loop(dvi.GPModel(Z, V, 3), dfree=True), loop(dvi.GPModel(Z, V, 3), dp=object()), loop(dvi.GPModel(Z, V, 3), X=torch.rand(2, 3).double()),
                loop(dvi.GPModel(Z, V, 3), graph=True), loop(dvi.GPModel(Z, V, 3, missing_targets=True)),
                loop(dvi.GPModel(Z, V, 3, variational_distribution="NGD")),
                loop(dvi.GPModel(Z, V, 3, variational_distribution="NGD", variational_strategy="CIQ"))):
        with pytest.raises(ValueError, match="derivative noise"):
            dvi._enable_derivative_noise(bad)
        assert not bad.likelihood.has_derivative_noise
    # the other harnesses refuse the keyword by name, before they look at anything else
    X = torch.rand(6, 3)
    for mod, args in ((dsvgp.dfree_directional_vi, ()), (dsvgp.shared_directional_vi, ()), (dsvgp.grad_svgp, (3,)), (dsvgp.traditional_vi, (3,))):
        with pytest.raises(ValueError, match="derivative_noise"):
            mod.train_gp(torch.utils.data.TensorDataset(X, torch.rand(6, 4)), *args, derivative_noise=True)
    with pytest.raises(ValueError, match="derivative_noise"):
        dvi.train_gp(torch.utils.data.TensorDataset(X, torch.rand(6, 4)), derivative_noise=True, missing_targets=True)
    two = dsvgp.gp_shim.GaussianLikelihood(derivative_noise=True)
    with pytest.raises(ValueError, match="derivative noise.*collapsed backward"):
        dvi.collapsed_loss_and_grads(dvi.GPModel(Z, V, 3), two, (X, torch.rand(6, 4)))


def _cpu_problem():
    return NY.problem(3, 10, 2, 2, 12)


def test_refusals_name_the_derivative_noise_before_any_device_work(dsvgp):
    P, x, y, D, nd = _cpu_problem()

    def engine(**attrs):
        eng = dsvgp.ElboEngine(torch.device("cpu"))
        for k, v in attrs.items():
            setattr(eng, k, v)
        return eng

    with pytest.raises(ValueError, match=r"derivative noise.*fast=True"):
        engine().loss_and_grads(P, x, y, D, nd, fast=True)
    switches = ((dict(capture_mode=True), "capture_mode"), (dict(deterministic=True), "deterministic"),
                (dict(collective=types.SimpleNamespace(world=2, rank=0)), "world = 2"), (dict(whitening="ciq"), "CIQ"),
                (dict(shared_directions=True), "shared"), (dict(data_outputs="values"), "values"),
                (dict(missing_targets=True), "missing_targets"))
    for attrs, what in switches:
        for mll in ("ELBO", "PLL"):
            with pytest.raises(ValueError, match=r"derivative noise.*%s" % what):
                engine(**attrs).loss_and_grads(P, x, y, D, nd, mll)
    nat = {k: v for k, v in P.items() if k not in ("variational_mean", "chol_variational_covar")}
    nat["natural_vec"], nat["natural_mat"] = P["variational_mean"], -0.5 * torch.eye(P["variational_mean"].shape[0])
    with pytest.raises(ValueError, match=r"derivative noise.*natural"):
        engine().loss_and_grads(nat, x, y, D, nd)
    P64 = {k: v.double() for k, v in P.items()}
    with pytest.raises(ValueError, match=r"derivative noise.*float"):
        engine().loss_and_grads(P64, x.double(), y.double(), D.double(), nd)
    with pytest.raises(ValueError, match=r"derivative noise.*float64"):
        engine().loss_and_grads(P, x.double(), y, D, nd)
    with pytest.raises(ValueError, match=r"derivative noise.*float64"):
        engine().loss_and_grads(dict(P64, raw_derivative_noise=P["raw_derivative_noise"]), x.double(), y.double(), D.double(), nd)
    eng64 = dsvgp._step64.ElboEngine64(torch.device("cpu"))
    for call in (lambda: eng64.loss_and_grads(P64, x.double(), y.double(), D.double(), nd), lambda: eng64.predict(P64, x.double(), D.double()),
                 lambda: eng64.predict_joint(P64, x.double(), D.double())):
        with pytest.raises(ValueError, match=r"derivative noise.*float"):
            call()
    # ARD and Matern-5/2 models: the same refusals, the derivative noise named first
    Pa = dict(P, raw_lengthscale=P["raw_lengthscale"].reshape(1, 1).expand(1, 3).contiguous())
    with pytest.raises(ValueError, match=r"derivative noise.*fast=True"):
        engine().loss_and_grads(Pa, x, y, D, nd, fast=True)
    with pytest.raises(ValueError, match=r"derivative noise.*deterministic"):
        engine(kernel="matern52", deterministic=True).loss_and_grads(P, x, y, D, nd)
    # the predictions and the accumulator: the switches that are not about training
    for attrs, what in switches:
        if what in ("capture_mode", "deterministic"):
            continue
        for entry in ("predict", "predict_joint", "predict_blocks"):
            with pytest.raises(ValueError, match=r"derivative noise.*%s" % what):
                getattr(engine(**attrs), entry)(P, x, D)
        with pytest.raises(ValueError, match=r"derivative noise.*%s" % what):
            engine(**attrs).collapsed_accumulator(P)
    # the collapsed backward pass
    acc = dsvgp._step.CollapsedAccumulator.__new__(dsvgp._step.CollapsedAccumulator)
    acc._classes = True
    with pytest.raises(ValueError, match=r"derivative noise.*begin_backward"):
        acc.begin_backward(None)
    # without the key nothing above is looked at: the default engine goes on to the device work (and fails there, on a CPU tensor)
    P1 = {k: v for k, v in P.items() if k != "raw_derivative_noise"}
    with pytest.raises(Exception) as info:
        engine().loss_and_grads(P1, x, y, D, nd, fast=False)
    assert "derivative noise" not in str(info.value)
