"""Closed-form optimal q(u) on the GPU (csrc/collapsed.hip, ``ElboEngine.collapsed_accumulator``, ``fit_variational``) against the float64
reference of tests/_collapsed_ref.py and the oracle's objective.

Cases (tests/_collapsed_ref.py: CASES) sit where the kernels can go wrong, not at workload size: M' = 72 / 129 / 65 (one row past a
64-tile, past two), ragged B', rectangular data (values only, pd = d), the wide route (d = 100), ARD and Matern-5/2.  Every case first
asserts cond(B) < 1e4 on the reference.

Bounds.  Errors in function space and gradients at the optimum are held against a MEASURED floor -- the same engine call against the same
oracle when both are handed the reference's optimum cast to float32 -- times 4 (the fp32 assembly error enters the optimum once more
through G and once through b).  Gradients at the optimum are also at most 1e-2 of those at (0, I): an fp32 Gram error of about 2^-20
times cond(B) < 1e4.  Chunked statistics agree to 1e-10 of |A| |A|^T (float64 reassociation over <= 1e3 terms; the assembly route does
not depend on the chunking).  The natural pair maps back within 4 x 2^-24 x cond(B).  The step's loss agrees with the float64 value
within the project's step-loss tolerance 2e-5 (tests/test_gpu_rect_train.py: LOSS_TOL)."""
import ctypes as C
import math

import pytest
import torch

import dsvgp_oracle as O
import _collapsed_ref as R
from _matern_yardstick import matern52_family, matern_forward, matern_predictive, rbf_family

pytestmark = pytest.mark.gpu
NAMES = sorted(R.CASES)
LOSS_TOL = 2e-5
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()                                              # (engines and accumulators: freed with the module, not at interpreter exit)


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _engine(dsvgp, dev, kernel):
    eng = dsvgp.ElboEngine(dev)
    eng.kernel = "matern52" if kernel == "matern52" else "rbf"
    return eng


def _ref(name):
    """(problem, reference statistics, cond(B), reference optimum) -- once per case, shared, never changed"""
    key = ("ref", name)
    if key not in _cache:
        prob = R.problem(name)
        P, x, y, D, nd, _, _, kernel = prob
        stats = R.statistics(P, x, y, D, kernel)
        _cache[key] = (prob, stats, R.cond_B(stats, num_data=nd), R.optimum(stats, num_data=nd))
    return _cache[key]


def _gpu(dsvgp, dev, name):
    """(engine, device parameters, accumulator holding the whole case, its solve result) -- once per case"""
    key = ("gpu", name)
    if key not in _cache:
        (P, x, y, D, nd, _, _, kernel), _, cond, _ = _ref(name)
        assert cond < 1e4, cond
        eng = _engine(dsvgp, dev, kernel)
        Pg = {k: v.to(dev) for k, v in P.items()}
        acc = eng.collapsed_accumulator(Pg)
        acc.add(x.to(dev), y.to(dev), None if D is None else D.to(dev))
        _cache[key] = (eng, Pg, acc, acc.solve(nd))
    return _cache[key]


def _with_q(P, m, L_S, dev=None, dtype=torch.float32):
    Q = dict(P)
    Q["variational_mean"], Q["chol_variational_covar"] = m.to(dtype), L_S.to(dtype)
    return {k: v.to(dev) for k, v in Q.items()} if dev is not None else Q


def _family(kernel):
    return matern52_family if kernel == "matern52" else rbf_family


def _oracle_predict(P, m, L_S, xt, Dt, kernel):
    """(mean, variance with noise) in float64 at the held-out points with the model's own p directions"""
    Q = {k: v.double() for k, v in _with_q(P, m, L_S, dtype=torch.float64).items()}
    p = Q["inducing_directions"].shape[0] // Q["inducing_points"].shape[0]
    noise = torch.nn.functional.softplus(Q["raw_noise"]).reshape(()) + O.NOISE_FLOOR
    if kernel == "rbf":
        mu, var = O.predictive(Q, xt.double(), Dt.double())
    else:
        mu, Sigma = matern_predictive(Q, xt.double(), Dt.double(), p, family=_family(kernel))
        var = Sigma.diagonal()
    return mu, var + noise


def _oracle_loss(P, m, L_S, x, y, D, nd, kernel):
    Q = {k: v.double() for k, v in _with_q(P, m, L_S, dtype=torch.float64).items()}
    B = x.shape[0]
    pd = 0 if D is None else D.shape[0] // B
    p = Q["inducing_directions"].shape[0] // Q["inducing_points"].shape[0]
    if kernel == "rbf" and pd == p:
        return O.elbo_forward(Q, x.double(), y.double(), D.double(), nd)[0].item()
    Dd = x.new_zeros(0, x.shape[1]).double() if D is None else D.double()
    return matern_forward(Q, x.double(), y.double(), Dd, pd, nd, "ELBO", family=_family(kernel))[0].item()


def _step(eng, Pq, x, y, D, nd, dev):
    Dg = None if D is None else D.to(dev)
    if Dg is None:
        Dg = torch.zeros(0, x.shape[1], device=dev)
    loss, grads, _, _ = eng.loss_and_grads(Pq, x.to(dev), y.to(dev), Dg, nd)
    return loss.item(), grads["variational_mean"].abs().max().item(), torch.tril(grads["chol_variational_covar"]).abs().max().item()


# ------------------------------------------------------------------ 1. statistics and optimum in function space
@pytest.mark.parametrize("name", NAMES)
def test_optimum_in_function_space(dsvgp, gpu_device, name):
    dev = gpu_device
    (P, x, y, D, nd, xt, Dt, kernel), _, cond, (m_ref, L_ref, _, _) = _ref(name)
    eng, Pg, acc, res = _gpu(dsvgp, dev, name)
    assert acc.rows == y.numel() and res.terms["rows"] == y.numel()
    xg, Dg = xt.to(dev), Dt.to(dev)
    m32, L32 = m_ref.float(), L_ref.float()
    mu_f, var_f = eng.predict(_with_q(P, m32, L32, dev), xg, Dg)                       # the floor of the existing path
    mu_o, var_o = _oracle_predict(P, m32, L32, xt, Dt, kernel)
    floor = (relmax(mu_f, mu_o), relmax(var_f, var_o))
    mu_n, var_n = eng.predict(_with_q(Pg, res.variational_mean, res.chol_variational_covar), xg, Dg)
    mu_r, var_r = _oracle_predict(P, m_ref, L_ref, xt, Dt, kernel)
    new = (relmax(mu_n, mu_r), relmax(var_n, var_r))
    msg = "case %s: cond(B) %.2e; mean error %.3e (floor %.3e), variance error %.3e (floor %.3e)" % (name, cond, new[0], floor[0], new[1], floor[1])
    print("[collapsed] " + msg)
    assert new[0] <= 4 * floor[0] and new[1] <= 4 * floor[1], msg


# ------------------------------------------------------------------ 2. stationarity under the engine's own objective
@pytest.mark.parametrize("name", NAMES)
def test_optimum_is_stationary_for_the_step(dsvgp, gpu_device, name):
    dev = gpu_device
    (P, x, y, D, nd, _, _, kernel), _, cond, (m_ref, L_ref, _, _) = _ref(name)
    eng, Pg, acc, res = _gpu(dsvgp, dev, name)
    n = m_ref.shape[0]
    _, gm0, gl0 = _step(eng, _with_q(P, torch.zeros(n), torch.eye(n), dev), x, y, D, nd, dev)
    _, gmf, glf = _step(eng, _with_q(P, m_ref.float(), L_ref.float(), dev), x, y, D, nd, dev)
    loss, gm, gl = _step(eng, _with_q(Pg, res.variational_mean, res.chol_variational_covar), x, y, D, nd, dev)
    msg = ("case %s: |dm| %.3e (floor %.3e, at (0, I) %.3e), |dL_S| %.3e (floor %.3e, at (0, I) %.3e); loss %.9f, result.loss %.9f"
           % (name, gm, gmf, gm0, gl, glf, gl0, loss, res.loss))
    print("[collapsed] " + msg)
    assert gm <= 4 * gmf and gl <= 4 * glf, msg
    assert gm <= 1e-2 * gm0 and gl <= 1e-2 * gl0, msg
    assert abs(loss - res.loss) <= LOSS_TOL * abs(res.loss), msg
    g = torch.Generator().manual_seed(3)
    for _ in range(3):                                          # random perturbations raise evaluate's loss
        dm = 1e-2 * torch.randn(n, generator=g).to(dev)
        dL = 1e-2 * torch.tril(torch.randn(n, n, generator=g)).to(dev)
        up = acc.evaluate(res.variational_mean + dm, res.chol_variational_covar + dL, nd).loss
        assert up > res.loss, (up, res.loss)
    at = acc.evaluate(res.variational_mean, res.chol_variational_covar, nd)
    assert abs(at.loss - res.loss) <= 1e-6 * abs(res.loss), (at.loss, res.loss)          # (float32 rounding of the optimum: second order)


# ------------------------------------------------------------------ 3. evaluate against loss_and_grads
@pytest.mark.parametrize("name", NAMES)
def test_evaluate_against_the_step(dsvgp, gpu_device, name):
    dev = gpu_device
    (P, x, y, D, nd, _, _, kernel), _, _, _ = _ref(name)
    eng, Pg, acc, res = _gpu(dsvgp, dev, name)
    n = acc.Mp
    g = torch.Generator().manual_seed(17)
    for _ in range(3):
        m = 0.3 * torch.randn(n, generator=g)
        L_S = torch.tril(torch.eye(n) + 0.05 * torch.randn(n, n, generator=g))
        ref = _oracle_loss(P, m, L_S, x, y, D, nd, kernel)
        got = acc.evaluate(m.to(dev), L_S.to(dev), nd)
        step_loss, _, _ = _step(eng, _with_q(P, m, L_S, dev), x, y, D, nd, dev)
        e_eval, e_step = abs(got.loss - ref) / abs(ref), abs(step_loss - ref) / abs(ref)
        print("[collapsed] case %s: evaluate error %.3e, loss_and_grads error %.3e" % (name, e_eval, e_step))
        assert e_eval <= max(4 * e_step, 1e-6), (e_eval, e_step)
        t = got.terms
        assert abs(t["loss"] + (t["log_likelihood"] / t["rows"] - t["kl"] / nd)) <= 1e-12 * abs(t["loss"])


# ------------------------------------------------------------------ 4. chunking
def _stats_close(a, b, stats):
    Ga, ba, yya, dga, Ra = a
    Gb, bb, yyb, dgb, Rb = b
    scale = stats["absG"].max().item()
    assert (torch.tril(Ga) - torch.tril(Gb)).abs().max().item() <= 1e-10 * scale
    assert (ba - bb).abs().max().item() <= 1e-10 * max(ba.abs().max().item(), scale)
    assert abs(yya.item() - yyb.item()) <= 1e-10 * abs(yyb.item())
    assert abs(dga.item() - dgb.item()) <= 1e-10 * abs(dgb.item()) and Ra.item() == Rb.item()


@pytest.mark.parametrize("name", ["a", "h"])
def test_chunking_does_not_change_the_statistics(dsvgp, gpu_device, name):
    dev = gpu_device
    (P, x, y, D, nd, _, _, kernel), stats, _, _ = _ref(name)
    eng, Pg, acc, _ = _gpu(dsvgp, dev, name)
    whole = acc.statistics()
    xg, yg, Dg = x.to(dev), y.to(dev), D.to(dev)
    pd = D.shape[0] // x.shape[0]
    q = pd + 1

    def three(a):
        for lo, hi in ((0, 50), (50, 51), (51, x.shape[0])):
            a.add(xg[lo:hi], yg[lo * q:hi * q], Dg[lo * pd:hi * pd])
        return a
    split = three(eng.collapsed_accumulator(Pg))
    assert split.rows == acc.rows
    _stats_close(split.statistics(), whole, stats)
    small = eng.collapsed_accumulator(Pg, workspace_budget=37 * acc.row_bytes(pd))
    assert small.chunk_rows(pd) == 37
    small.add(xg, yg, Dg)
    _stats_close(small.statistics(), whole, stats)
    split.reset()
    assert split.rows == 0 and split.statistics()[0].abs().max().item() == 0.0
    with pytest.raises(ValueError, match="empty"):
        split.solve()
    _stats_close(three(split).statistics(), whole, stats)
    # against the reference itself: float32 assembly, so the project's kernel tolerance (2e-5 of max) times the conditioning of L is
    # the scale; here only a sanity bound -- the function-space test holds the statistics to the measured floor
    assert relmax(torch.tril(whole[0]), torch.tril(stats["G"])) < 1e-2 and relmax(whole[1], stats["b"]) < 1e-2


def test_mixed_direction_counts_accumulate_to_the_union(dsvgp, gpu_device):
    """case d (values only) then case e (pd = d) on the same points: the statistics are the sum of the two, and the optimum is the
    reference optimum of the union in function space (4 x the floor of the existing path)"""
    dev = gpu_device
    (Pd, xd, yd, _, _, xt, Dt, kernel), sd, _, _ = _ref("d")
    (Pe, xe, ye, De, _, _, _, _), se, _, _ = _ref("e")
    assert torch.equal(xd, xe) and all(torch.equal(Pd[k], Pe[k]) for k in Pd)
    eng, Pg, acc_d, _ = _gpu(dsvgp, dev, "d")
    _, _, acc_e, _ = _gpu(dsvgp, dev, "e")
    mixed = eng.collapsed_accumulator(Pg)
    mixed.add(xd.to(dev), yd.to(dev), None).add(xe.to(dev), ye.to(dev), De.to(dev))
    union = R.merge(sd, se)
    assert mixed.rows == union["R"]
    summed = tuple(a + b for a, b in zip(acc_d.statistics(), acc_e.statistics()))
    _stats_close(mixed.statistics(), summed, union)
    nd = 1.3 * union["R"]
    assert R.cond_B(union, num_data=nd) < 1e4
    m_ref, L_ref, _, _ = R.optimum(union, num_data=nd)
    res = mixed.solve(nd)
    xg, Dg = xt.to(dev), Dt.to(dev)
    mu_f, var_f = eng.predict(_with_q(Pd, m_ref.float(), L_ref.float(), dev), xg, Dg)
    mu_o, var_o = _oracle_predict(Pd, m_ref.float(), L_ref.float(), xt, Dt, kernel)
    mu_n, var_n = eng.predict(_with_q(Pg, res.variational_mean, res.chol_variational_covar), xg, Dg)
    mu_r, var_r = _oracle_predict(Pd, m_ref, L_ref, xt, Dt, kernel)
    new, floor = (relmax(mu_n, mu_r), relmax(var_n, var_r)), (relmax(mu_f, mu_o), relmax(var_f, var_o))
    print("[collapsed] union of d and e: mean error %.3e (floor %.3e), variance error %.3e (floor %.3e)" % (new[0], floor[0], new[1], floor[1]))
    assert new[0] <= 4 * floor[0] and new[1] <= 4 * floor[1], (new, floor)


# ------------------------------------------------------------------ 5. natural parameters, 6. outputs
@pytest.mark.parametrize("name", NAMES)
def test_natural_pair_and_output_structure(dsvgp, gpu_device, name):
    dev = gpu_device
    (P, x, y, D, nd, _, _, kernel), _, cond, _ = _ref(name)
    eng, Pg, acc, res = _gpu(dsvgp, dev, name)
    m, L_S, nv, nm = res.variational_mean, res.chol_variational_covar, res.natural_vec, res.natural_mat
    assert all(t.dtype == torch.float32 for t in (m, L_S, nv, nm)) and isinstance(res.loss, float)
    assert torch.triu(L_S, 1).abs().max().item() == 0.0 and (L_S.diagonal() > 0).all()
    assert torch.equal(nm, nm.t())
    mu, chol = O.natural_to_mu_chol(nv.double().cpu(), nm.double().cpu())
    bound = 4 * 2.0 ** -24 * cond
    errs = (relmax(mu, m), relmax(chol, L_S))
    print("[collapsed] case %s: natural pair -> (m, L_S) errors %.3e, %.3e (bound %.3e)" % (name, errs[0], errs[1], bound))
    assert errs[0] <= bound and errs[1] <= bound, (errs, bound)
    if kernel != "rbf":
        return                                                  # (ARD / Matern-5/2 steps take the Cholesky parameterisation only)
    Pn = {k: v for k, v in Pg.items() if k not in ("variational_mean", "chol_variational_covar")}
    Pn["natural_vec"], Pn["natural_mat"] = nv, nm
    Dg = torch.zeros(0, x.shape[1], device=dev) if D is None else D.to(dev)
    ngd_loss = eng.loss_and_grads(Pn, x.to(dev), y.to(dev), Dg, nd)[0].item()
    ref = _oracle_loss(P, m.cpu(), L_S.cpu(), x, y, D, nd, kernel)
    step_loss, _, _ = _step(eng, _with_q(Pg, m, L_S), x, y, D, nd, dev)
    e_step = abs(step_loss - ref) / abs(ref)
    assert abs(ngd_loss - res.loss) <= max(4 * e_step, 1e-6) * abs(res.loss), (ngd_loss, res.loss, e_step)


# ------------------------------------------------------------------ 7. C entries
def test_c_entries_refuse_and_report(dsvgp, gpu_device):
    dev = gpu_device
    lib, ops = dsvgp._lib.lib, dsvgp._ops
    ctx = ops.Context.get(dev)
    Mp, Bp = 5, 7
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    state = torch.full((int(lib.dsvgp_collapsed_state_bytes(Mp)) // 8,), 7.0, dtype=torch.float64, device=dev)
    A64 = torch.full((Mp + 1, Bp), 3.0, dtype=torch.float64, device=dev)
    y, diag, c = torch.ones(Bp, device=dev), torch.ones(Bp, device=dev), torch.zeros(1, device=dev)
    hyp = torch.tensor([1.0, 1.0, 0.1, 0.0], device=dev)
    ws = ops.collapsed_workspace(Mp, dev)
    m, LS = torch.full((Mp,), 9.0, device=dev), torch.full((Mp, Mp), 9.0, device=dev)
    nv, nm = torch.full((Mp,), 9.0, device=dev), torch.full((Mp, Mp), 9.0, device=dev)
    scal = torch.full((8,), 9.0, dtype=torch.float64, device=dev)
    info = torch.full((1,), 9, dtype=torch.int32, device=dev)
    EINVAL = -1
    acc = lambda **k: lib.dsvgp_collapsed_accumulate(k.get("ctx", ctx.h), k.get("state", p(state)), k.get("Mp", Mp), k.get("A", p(A64)),
                                                     k.get("lda", Bp), k.get("Bp", Bp), k.get("y", p(y)), p(c), k.get("diag", p(diag)))
    sol = lambda **k: lib.dsvgp_collapsed_solve(ctx.h, k.get("state", p(state)), k.get("Mp", Mp), k.get("hyp", p(hyp)), k.get("nd", 10.0),
                                                p(m), p(LS), k.get("ldls", Mp), p(nv), p(nm), k.get("ldnm", Mp), p(scal), p(info),
                                                k.get("ws", p(ws)))
    ev = lambda **k: lib.dsvgp_collapsed_evaluate(ctx.h, k.get("state", p(state)), k.get("Mp", Mp), k.get("m", p(m)), p(LS), k.get("ldls", Mp),
                                                  p(hyp), k.get("nd", 10.0), k.get("scal", p(scal)), p(ws))
    for rc in (acc(state=null), acc(A=null), acc(y=null), acc(diag=null), acc(Mp=0), acc(lda=Bp - 1), acc(Bp=-1), acc(ctx=null),
               sol(state=null), sol(hyp=null), sol(ws=null), sol(Mp=0), sol(Mp=-2), sol(nd=0.0), sol(nd=-1.0), sol(ldls=Mp - 1),
               sol(ldnm=Mp - 1), ev(state=null), ev(m=null), ev(scal=null), ev(Mp=0), ev(nd=0.0), ev(ldls=Mp - 1),
               lib.dsvgp_collapsed_reset(ctx.h, null, Mp), lib.dsvgp_collapsed_reset(ctx.h, p(state), 0)):
        assert rc == EINVAL, rc
    assert acc(Bp=0) == 0
    torch.cuda.synchronize()
    assert (state == 7.0).all() and (A64 == 3.0).all() and (scal == 9.0).all() and info.item() == 9
    assert all((t == 9.0).all() for t in (m, LS, nv, nm))
    # an empty state is an error of solve (info = -2, NaN outputs), reported without a host read and without a fault
    assert lib.dsvgp_collapsed_reset(ctx.h, p(state), Mp) == 0
    assert sol() == 0
    assert info.item() == -2 and torch.isnan(m).all() and torch.isnan(LS).all() and torch.isnan(scal[:5]).all()
    # optional outputs may be null
    A64.copy_(torch.randn(Mp + 1, Bp, dtype=torch.float64, generator=torch.Generator().manual_seed(0)))
    assert acc() == 0
    assert lib.dsvgp_collapsed_solve(ctx.h, p(state), Mp, p(hyp), 10.0, null, null, 0, null, null, 0, null, null, p(ws)) == 0
    assert lib.dsvgp_collapsed_solve(ctx.h, p(state), Mp, p(hyp), 10.0, null, null, 0, null, null, 0, p(scal), p(info), p(ws)) == 0
    assert info.item() == 0 and torch.isfinite(scal).all() and scal[5].item() == Bp
    # a NaN in y: info = -1 and NaN outputs
    y[3] = float("nan")
    assert acc() == 0 and sol() == 0
    assert info.item() == -1 and torch.isnan(m).all() and torch.isnan(nm).all() and torch.isnan(scal[0])


def test_a_nan_target_raises_from_the_python_layer(dsvgp, gpu_device):
    dev = gpu_device
    (P, x, y, D, nd, _, _, kernel), _, _, _ = _ref("c")
    eng, Pg, _, _ = _gpu(dsvgp, dev, "c")
    acc = eng.collapsed_accumulator(Pg)
    bad = y.clone()
    bad[11] = float("nan")
    acc.add(x.to(dev), bad.to(dev), D.to(dev))
    with pytest.raises((ValueError, dsvgp.NotPSDError), match="not finite"):
        acc.solve(nd)
    with pytest.raises(ValueError, match="interleaved"):
        acc.add(x.to(dev), y[:-1].to(dev), D.to(dev))
    with pytest.raises(ValueError, match="num_data must be positive"):
        acc.solve(0.0)


# ------------------------------------------------------------------ 8. harness
def _harness_data(dev):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("train_quality", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                "tools", "train_quality.py"))
    tq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tq)
    X, Y = tq.make_data("sin", 600 + 256, 3, dev, seed=0)
    Y = Y.float()
    return (X[:600].contiguous(), Y[:600].contiguous()), (X[600:].contiguous(), Y[600:].contiguous())


def test_fit_variational_and_the_optimal_start(dsvgp, gpu_device):
    dev = gpu_device
    (X, Y), (Xt, Yt) = _harness_data(dev)
    dvi = dsvgp.directional_vi
    train = torch.utils.data.TensorDataset(X, Y)
    test = torch.utils.data.TensorDataset(Xt, Yt)
    kw = dict(num_inducing=32, num_directions=2, minibatch_size=200, minibatch_dim=2, num_epochs=1, seed=4)
    loop = dvi.setup_training(train, **kw)
    model, likelihood = loop.model, loop.likelihood
    nd = 4 * 600
    acc = model.engine.collapsed_accumulator(model._param_dict(likelihood))
    E = torch.eye(3, device=dev)[:2].repeat(600, 1)
    acc.add(X, Y[:, [0, 1, 2]].reshape(-1).contiguous(), E)
    n = acc.Mp
    prior = acc.evaluate(torch.zeros(n, device=dev), torch.eye(n, device=dev), nd).loss
    res = model.fit_variational(likelihood, (X, Y), minibatch_size=256, seed=4)
    vd = model.variational_strategy._variational_distribution
    assert torch.equal(vd.variational_mean.data, res.variational_mean) and torch.equal(vd.chol_variational_covar.data, res.chol_variational_covar)
    fitted = acc.evaluate(vd.variational_mean.data, vd.chol_variational_covar.data, nd).loss
    print("[collapsed] harness: full-data loss %.5f at (0, I) -> %.5f after fit_variational (its own %.5f)" % (prior, fitted, res.loss))
    assert fitted < prior
    means, _ = dvi.eval_gp(test, model, likelihood, num_directions=2, minibatch_size=128, minibatch_dim=2)
    mse = ((means[::3] - Yt[:, 0].cpu()) ** 2).mean().item()
    const = ((Yt[:, 0].cpu() - Y[:, 0].mean().item()) ** 2).mean().item()
    print("[collapsed] harness: test MSE %.5f after one fit_variational, constant predictor %.5f" % (mse, const))
    assert mse < const

    def first_loss(**extra):
        torch.manual_seed(0)                                    # (q(u)'s start draws 1e-3 randn from the global generator)
        lp = dvi.setup_training(train, **kw, **extra)
        start = [q.detach().clone() for q in lp.model.variational_parameters()]
        perm = lp.epoch_permutation()
        out = [lp.step(perm[s:s + 200])[0].item() for s in range(0, 600, 200)]
        lp.finish()
        return out, lp, start
    default, _, start_default = first_loss()
    again, _, start_again = first_loss(variational_initialization=None)
    # the default start through the untouched path: the same bits in q(u); the step's sums meet in atomics, so its loss to fp32 rounding
    assert all(torch.equal(a, b) for a, b in zip(start_default, start_again))
    assert abs(default[0] - again[0]) <= 1e-6 * abs(default[0])
    optimal, lp, _ = first_loss(variational_initialization="optimal")
    print("[collapsed] harness: first loss %.5f (default start) -> %.5f (optimal start)" % (default[0], optimal[0]))
    assert optimal[0] < default[0] and all(math.isfinite(v) for v in optimal)
    model2, _ = dvi.train_gp(train, **kw, variational_initialization="optimal", max_steps=3, verbose=False)
    assert torch.isfinite(model2.variational_strategy._variational_distribution.variational_mean).all()
    # refit on the loop: the two tensors' optimiser moments (and step counts) start again from zero
    states = [lp.variational_optimizer.state[q] for q in lp.model.variational_parameters()]
    assert len(states) == 2 and all(st["step"] == 3 and st["exp_avg"].abs().max().item() > 0 for st in states)
    lp.refit_variational(seed=4)
    assert all(st["step"] == 0 and st["exp_avg"].abs().max().item() == 0.0 and st["exp_avg_sq"].abs().max().item() == 0.0 for st in states)
    assert math.isfinite(lp.step(lp.epoch_permutation()[:200])[0].item())
