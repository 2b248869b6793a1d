"""Missing observations, host side: the float64 reference of tests/_missing_ref.py against the existing yardsticks on
all-present data, its invariance to what stands in the deleted entries, the C ABI's declarations and bindings, the ``missing_targets``
switch with its refusals (checked on a CPU-device engine: every refusal comes before any device work) and the harness keywords.
Every case of the GPU tests (tests/test_gpu_missing.py) is run through the reference here first: finite, Cholesky without a jitter step."""
import inspect
import os
import re
import types

import pytest
import torch

import dsvgp_oracle as O
import _missing_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dsvgp_likelihood_terms_masked_workspace_bytes", "dsvgp_likelihood_terms_masked", "dsvgp_collapsed_accumulate_masked",
               "dsvgp_collapsed_grad_chunk_masked_bytes", "dsvgp_collapsed_grad_chunk_masked")


def relmax(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _yardstick(name, mll):
    """the committed float64 step of the case's kernel on its all-present data"""
    P, x, y, D, nd, kernel = MR.problem(name)
    pd = MR.CASES[name][4]
    P64, x, y, D = {k: v.double() for k, v in P.items()}, x.double(), y.double(), D.double()
    if kernel == "matern52":
        from _matern_yardstick import matern_elbo
        return matern_elbo(P64, x, y, D, pd, nd, mll)
    if kernel == "ard":
        from _ard_yardstick import ard_elbo
        return ard_elbo(P64, x, y, D, pd, nd, mll)
    if pd != MR.CASES[name][3]:
        from test_gpu_rect_train import rect_elbo
        return rect_elbo(P64, x, y, D, pd, nd, mll)
    return O.elbo_loss_and_grads(P64, x, y, D, nd, mll)


@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
@pytest.mark.parametrize("name", ["m72", "ard", "matern", "rect"])
def test_reference_equals_the_yardstick_on_all_present_data(name, mll):
    P, x, y, D, nd, kernel = MR.problem(name)
    loss, grads, mu, varn, keep = MR.step(P, x, y, D, nd, mll, kernel)
    l_ref, g_ref, mu_ref, var_ref = _yardstick(name, mll)
    assert bool(keep.all())
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref), "varn": relmax(varn, var_ref)}
    for k in O.PARAM_NAMES:
        errs[k] = relmax(grads[k].reshape(-1), g_ref[k].reshape(-1))
    print("[parity] missing reference vs yardstick %s %s: %s" % (name, mll, errs))
    assert max(errs.values()) <= 1e-12, errs


@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
def test_reference_never_reads_the_deleted_entries(mll):
    P, x, y, D, nd, kernel = MR.problem("m72")
    pd = MR.CASES["m72"][4]
    y_nan = MR.random_pattern(y, pd)
    keep = MR.present_mask(y_nan)
    assert 0.2 < 1.0 - keep.double().mean().item() < 0.4
    a = MR.step(P, x, y_nan, D, nd, mll, kernel)
    for filler in (0.0, 7.5, float("inf")):
        y_fill = y_nan.clone()
        y_fill[~keep] = filler
        b = MR.step(P, x, y_fill, D, nd, mll, kernel, keep=keep)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
        assert all(torch.equal(a[1][k], b[1][k]) for k in O.PARAM_NAMES)
    ca = MR.collapsed(P, x, y_nan, D, nd, kernel)
    y_fill = y_nan.clone()
    y_fill[~keep] = -3.0
    cb = MR.collapsed(P, x, y_fill, D, nd, kernel, keep=keep)
    assert torch.equal(ca["loss"], cb["loss"]) and torch.equal(ca["m"], cb["m"]) and ca["stats"]["R"] == float(keep.sum())


def test_reference_with_nothing_present_is_the_kl_term():
    P, x, y, D, nd, kernel = MR.problem("m72")
    loss, grads, _, _, keep = MR.step(P, x, torch.full_like(y, float("nan")), D, nd, "ELBO", kernel)
    kl = O.kl_whitened(P["variational_mean"].double(), torch.tril(P["chol_variational_covar"].double()))
    assert int(keep.sum()) == 0 and loss.item() == (kl / nd).item()
    assert all(grads[k].abs().max().item() == 0.0 for k in O.PARAM_NAMES if k not in ("variational_mean", "chol_variational_covar"))


@pytest.mark.parametrize("name", sorted(MR.CASES))
def test_every_gpu_case_has_a_finite_reference_without_a_jitter_step(name):
    """``torch.linalg.cholesky`` inside the reference raises where K~ (or I + kappa G) would need jitter"""
    P, x, y, D, nd, kernel = MR.problem(name)
    pd = MR.CASES[name][4]
    patterns = [MR.random_pattern(y, pd), y]
    if name == "m72":
        patterns.append(MR.derivatives_missing(y, pd))
    for yy in patterns:
        for mll in ("ELBO", "PLL"):
            loss, grads, mu, varn, _ = MR.step(P, x, yy, D, nd, mll, kernel)
            assert all(bool(torch.isfinite(t).all()) for t in [loss, mu, varn] + list(grads.values()))
            assert varn.min().item() > 2 * O.MIN_VARIANCE                      # (no clamp in play)
    c = MR.collapsed(P, x, MR.random_pattern(y, pd), D, nd, kernel)
    assert all(bool(torch.isfinite(t).all()) for t in [c["loss"], c["m"], c["L_S"]] + list(c["grads"].values()))


def test_new_symbols_are_declared_and_bound(dsvgp):
    with open(os.path.join(ROOT, "include", "dsvgp.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
        assert name in dsvgp._lib.SIGNATURES and hasattr(dsvgp._lib.lib, name), name
    for name in ("likelihood_terms_masked", "likelihood_terms_masked_workspace", "collapsed_accumulate_masked_",
                 "collapsed_grad_chunk_masked", "collapsed_grad_chunk_masked_bytes"):
        assert callable(getattr(dsvgp._ops, name)), name
    lib = dsvgp._lib.lib
    assert lib.dsvgp_likelihood_terms_masked_workspace_bytes() >= 512 * 4 * 6
    assert lib.dsvgp_collapsed_grad_chunk_masked_bytes(72, 111) >= lib.dsvgp_collapsed_grad_chunk_bytes(72, 111) + 4 * 111
    assert lib.dsvgp_collapsed_grad_chunk_masked_bytes(0, 111) == 0 and lib.dsvgp_collapsed_grad_chunk_masked_bytes(72, 0) == 0
    # null pointers and negative sizes: DSVGP_EINVAL (-1), before anything is touched
    assert lib.dsvgp_likelihood_terms_masked(None, None, None, None, 8, 2, None, 0, None, None, None, None, None, None) == -1
    assert lib.dsvgp_collapsed_accumulate_masked(None, None, 4, None, 8, 8, 1, None, None, None) == -1
    assert lib.dsvgp_collapsed_grad_chunk_masked(None, 4, 8, None, 8, None, None, None, 4, None, None, None, 8, None, None, None) == -1


def test_switch_exists_and_defaults_to_off(dsvgp):
    eng = dsvgp.ElboEngine(torch.device("cpu"))
    assert eng.missing_targets is False
    dvi = dsvgp.directional_vi
    Z, V = torch.rand(4, 3), torch.eye(3)[:2].repeat(4, 1)
    assert dvi.GPModel(Z, V, 3).missing_targets is False and dvi.GPModel(Z, V, 3).engine.missing_targets is False
    model = dvi.GPModel(Z, V, 3, missing_targets=True)
    assert model.missing_targets is True and model.engine.missing_targets is True
    model.missing_targets = False
    assert model.engine.missing_targets is False                                 # (carried on every access, as ``kernel`` is)


def test_harness_keywords_are_accepted(dsvgp):
    dvi = dsvgp.directional_vi
    params = inspect.signature(dvi.train_collapsed).parameters
    assert list(params)[-1] == "missing_targets" and params["missing_targets"].default is False
    assert "missing_targets" in inspect.getsource(dvi.train_gp) and list(inspect.signature(dvi.train_gp).parameters)[-1] == "args"
    assert list(inspect.signature(dvi.TrainLoop.set_missing_targets).parameters) == ["self"]
    # the pinned signatures stay as they are (setup_training's last parameter is held by tests/test_abi_ard.py, test_abi_matern.py and
    # test_kmeans_host.py: the loop it returns takes the switch)
    for fn in (dvi.setup_training, dvi.collapsed_loss_and_grads, dvi.fit_variational, dvi.TrainLoop.refit_variational):
        assert "missing_targets" not in inspect.signature(fn).parameters
    # the loop's switch: refusals on switches alone, then the model's attribute and num_data times the present fraction of Y
    Z, V = torch.rand(4, 3), torch.eye(3)[:2].repeat(4, 1)
    Yl = torch.tensor([[1.0, float("nan"), 2.0, 3.0], [0.5, 1.0, float("nan"), float("nan")]])

    def loop(model, **kw):
        base = dict(model=model, dfree=False, full_gradient=False, dp=None, X=torch.rand(2, 3), Y=Yl, mll=types.SimpleNamespace(num_data=8))
        base.update(kw)
        return types.SimpleNamespace(**base)
    ok = loop(dvi.GPModel(Z, V, 3))
    dvi._enable_missing_targets(ok)
    assert ok.model.missing_targets is True and ok.model.engine.missing_targets is True and ok.mll.num_data == 8 * 5 / 8
    dvi._enable_missing_targets(ok)
    assert ok.mll.num_data == 5.0                                                # (scaled once)
    for bad in (loop(dvi.GPModel(Z, V, 3), dfree=True), loop(dvi.GPModel(Z, V, 3), dp=object()), loop(dvi.GPModel(Z, V, 3), X=torch.rand(2, 3).double()),
                loop(dvi.GPModel(Z, V, 3, variational_distribution="NGD")),
                loop(dvi.GPModel(Z, V, 3, variational_distribution="NGD", variational_strategy="CIQ"))):
        with pytest.raises(ValueError, match="missing_targets"):
            dvi._enable_missing_targets(bad)
        assert bad.model.missing_targets is False and bad.mll.num_data == 8
    Y = torch.tensor([[1.0, float("nan")], [float("nan"), float("nan")]])
    assert dvi._present_num_data(8, Y) == 2.0


def _cpu_problem():
    P, x, y, D, nd, _ = MR.problem("m72")
    return P, x, MR.random_pattern(y, 2), D, nd


def test_refusals_name_the_switch_before_any_device_work(dsvgp):
    P, x, y, D, nd = _cpu_problem()

    def engine(**attrs):
        eng = dsvgp.ElboEngine(torch.device("cpu"))
        eng.missing_targets = True
        for k, v in attrs.items():
            setattr(eng, k, v)
        return eng

    with pytest.raises(ValueError, match=r"missing_targets.*fast=True"):
        engine().loss_and_grads(P, x, y, D, nd, fast=True)
    for attrs, what in ((dict(capture_mode=True), "capture_mode"), (dict(deterministic=True), "deterministic"),
                        (dict(collective=types.SimpleNamespace(world=2, rank=0)), "world = 2"), (dict(whitening="ciq"), "CIQ"),
                        (dict(shared_directions=True), "shared"), (dict(data_outputs="values"), "values")):
        for mll in ("ELBO", "PLL"):
            with pytest.raises(ValueError, match=r"missing_targets.*%s" % what):
                engine(**attrs).loss_and_grads(P, x, y, D, nd, mll)
    nat = {k: v for k, v in P.items() if k not in ("variational_mean", "chol_variational_covar")}
    nat["natural_vec"], nat["natural_mat"] = P["variational_mean"], -0.5 * torch.eye(P["variational_mean"].shape[0])
    with pytest.raises(ValueError, match=r"missing_targets.*natural"):
        engine().loss_and_grads(nat, x, y, D, nd)
    with pytest.raises(ValueError, match=r"missing_targets.*float64"):
        engine().loss_and_grads({k: v.double() for k, v in P.items()}, x.double(), y.double(), D.double(), nd)
    with pytest.raises(ValueError, match=r"missing_targets.*float64"):
        engine().loss_and_grads(P, x.double(), y, D, nd)
    eng64 = dsvgp._step64.ElboEngine64(torch.device("cpu"))
    eng64.missing_targets = True
    with pytest.raises(ValueError, match=r"missing_targets.*float64"):
        eng64.loss_and_grads({k: v.double() for k, v in P.items()}, x.double(), y.double(), D.double(), nd)
    # ARD and Matern-5/2 models: the same refusals, the switch named first
    Pa = dict(P, raw_lengthscale=P["raw_lengthscale"].reshape(1, 1).expand(1, 3).contiguous())
    with pytest.raises(ValueError, match=r"missing_targets.*fast=True"):
        engine().loss_and_grads(Pa, x, y, D, nd, fast=True)
    with pytest.raises(ValueError, match=r"missing_targets.*deterministic"):
        engine(kernel="matern52", deterministic=True).loss_and_grads(P, x, y, D, nd)
    # the accumulator reads the switch when it is made
    for attrs, what in ((dict(whitening="ciq"), "CIQ"), (dict(shared_directions=True), "shared"), (dict(data_outputs="values"), "values"),
                        (dict(collective=types.SimpleNamespace(world=2, rank=0)), "world = 2")):
        with pytest.raises(ValueError, match=r"missing_targets.*%s" % what):
            engine(**attrs).collapsed_accumulator(P)
