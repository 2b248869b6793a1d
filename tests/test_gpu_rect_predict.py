"""Predictions with any number of data directions: the rectangular kernel assembly (``dsvgp_kernel_fwd_rect``,
csrc/assemble_wide.hip) and ``ElboEngine.predict`` / ``predict_joint`` / ``ApproximateGP.posterior`` / ``eval_values`` on top of it.

The yardstick is built here in float64 from the oracle (``rect_kernel``, ``rect_predictive``); the CPU test pins it to
``O.predictive`` / ``O.predictive_joint`` where those are defined (pd = 0 through the derivative-free variant, pd = p).  The GPU
tests hold the HIP path to it at the tolerances of the square kernel (tests/test_gpu_ops.py, tests/test_gpu_wide_inputs.py: 2e-5)
and of the predictive tests (tests/test_gpu_step.py: mean / variance 2e-4, covariance 5e-4, diagonal 1e-4); measured errors are
printed as [parity] lines."""
import ctypes as C
import functools
import math

import pytest
import torch

import dsvgp_oracle as O

gpu = pytest.mark.gpu
KTOL, TOL, CTOL, DTOL = 2e-5, 2e-4, 5e-4, 1e-4

#        d    M   p  pd    B    N
SHAPES = [(5, 40, 2, 0, 128, 600),        # value columns
          (5, 40, 2, 5, 67, 600),         # pd > p, ragged B
          (3, 33, 3, 1, 70, 300),         # pd < p
          (5, 19, 0, 5, 67, 300),         # plain SVGP with gradient rows
          (20, 64, 5, 20, 33, 900),       # full gradient at the C4 width
          (120, 24, 3, 0, 40, 400),       # wide inputs: several K chunks
          (200, 24, 3, 7, 40, 400),
          (100, 9, 95, 2, 5, 300),        # q = 96 on the inducing side
          (100, 9, 2, 95, 5, 300)]        # q = 96 on the data side
IDS = ["d%d-M%d-p%d-pd%d-B%d" % s[:5] for s in SHAPES]


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _report(tag, errs):
    print("[parity] %s: %s" % (tag, ", ".join("%s %.2e" % (k, v) for k, v in errs.items())))


def _raw(v):
    return math.log(math.expm1(v))          # softplus^-1


# ------------------------------------------------------------------ the yardstick
from _conditioning import rect_kernel        # (the padded square kernel; shared with the per-block conditioning tests)


def rect_predictive(P64, x, D, pd):
    """(mu, Sigma, prior) of q(f) over the B (pd + 1) outputs, no likelihood noise; prior = diag(s K_XX + 1e-4 I)"""
    Z, V, m = P64["inducing_points"], P64["inducing_directions"], P64["variational_mean"]
    L_S = torch.tril(P64["chol_variational_covar"])
    c = P64["constant"].reshape(())
    ell, s, _ = O.constrained(P64)
    M = Z.shape[0]
    p = V.shape[0] // M
    K_ZZ = s * O.kernel_matrix(Z, Z, V, V, ell)
    L = O.psd_safe_cholesky(K_ZZ + O.KZZ_JITTER * torch.eye(K_ZZ.shape[0], dtype=K_ZZ.dtype))
    K_ZX = s * rect_kernel(Z, V, p, x, D, pd, ell)
    K_XX = s * rect_kernel(x, D, pd, x, D, pd, ell) + O.KXX_JITTER * torch.eye(x.shape[0] * (pd + 1), dtype=x.dtype)
    A = torch.linalg.solve_triangular(L, K_ZX, upper=False)
    W = L_S.t() @ A
    return A.t() @ m + c, K_XX + W.t() @ W - A.t() @ A, K_XX.diagonal().clone()


@functools.lru_cache(maxsize=None)
def _case(d, M, p, pd, B, N):
    """(params fp32, x, data directions [B pd, d], mu / Sigma / prior fp64, noise, constant): once per shape, shared, never changed"""
    from test_gpu_step import make_problem
    P, x, _, _, _ = make_problem(N, d, M, p, B, seed=1)
    if d > 30:          # (tests/test_gpu_mean_predictor.py: otherwise the kernel between random points is numerically zero)
        P["raw_lengthscale"] = torch.tensor([[_raw(0.4 * math.sqrt(d))]])
    D = torch.randn(B * pd, d, generator=torch.Generator().manual_seed(5))
    P64 = {k: v.double() for k, v in P.items()}
    mu, Sigma, prior = rect_predictive(P64, x.double(), D.double(), pd)
    return P, x, D, mu, Sigma, prior, float(O.constrained(P64)[2]), float(P["constant"].reshape(()))


def _nontrivial(mu, Sigma, prior, c):
    """a kernel that returns the prior cannot pass: the yardstick moves the mean by >= 0.05 and the variance by >= 4 %"""
    span, shrink = (mu - c).abs().max().item(), (Sigma.diagonal() / prior - 1).abs().max().item()
    assert span >= 0.05 and shrink >= 0.04, (span, shrink)
    return {"max|mu - c|": span, "max|var/prior - 1|": shrink}


# ------------------------------------------------------------------ CPU: the yardstick against the oracle
def test_yardstick_equals_the_oracle_where_the_oracle_is_defined():
    from test_gpu_step import make_problem
    P, x, _, D, _ = make_problem(600, 5, 40, 2, 128, seed=1)
    P64, x, D = {k: v.double() for k, v in P.items()}, x.double(), D.double()
    mu0, Sig0, _ = rect_predictive(P64, x, D[:0], 0)
    mu_v, var_v = O.predictive(P64, x, D, data_outputs="values")
    mu_jv, Sig_v = O.predictive_joint(P64, x, D, data_outputs="values")
    mu2, Sig2, _ = rect_predictive(P64, x, D, 2)
    mu_j, Sig_j = O.predictive_joint(P64, x, D)
    errs = {"pd=0 mean": relmax(mu0, mu_v), "pd=0 variance": relmax(Sig0.diagonal(), var_v), "pd=0 joint mean": relmax(mu0, mu_jv),
            "pd=0 covariance": relmax(Sig0, Sig_v), "pd=p mean": relmax(mu2, mu_j), "pd=p covariance": relmax(Sig2, Sig_j)}
    _report("yardstick vs oracle", errs)
    assert mu0.shape == (128,) and Sig2.shape == (384, 384)
    assert max(errs.values()) <= 1e-12, errs


# ------------------------------------------------------------------ GPU 1: the kernel entry
def _packs(dsvgp, dev, P, x, D, p, pd):
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    ell, s, noise = O.constrained({k: v.double() for k, v in P.items()})
    hyp = torch.tensor([float(ell), float(s), float(noise), 0.0], dtype=torch.float32, device=dev)
    Z = P["inducing_points"].to(dev).contiguous()
    center = ops.column_mean(ctx, Z)
    pz = ops.pack_points(ctx, Z, P["inducing_directions"].to(dev).contiguous() if p else None, p, hyp, center)
    px = ops.pack_points(ctx, x.to(dev).contiguous(), D.to(dev).contiguous() if pd else None, pd, hyp, center)
    return ops, ctx, hyp, pz, px, float(ell), float(s)


@gpu
@pytest.mark.parametrize("d,M,p,pd,B,N", SHAPES, ids=IDS)
def test_kernel_fwd_rect_matches_fp64(dsvgp, gpu_device, d, M, p, pd, B, N):
    P, x, D, *_ = _case(d, M, p, pd, B, N)
    ops, ctx, hyp, pz, px, ell, s = _packs(dsvgp, gpu_device, P, x, D, p, pd)
    K = ops.kernel_fwd_rect(ctx, pz, M, p, px, B, pd, d, hyp)
    ref = s * rect_kernel(P["inducing_points"].double(), P["inducing_directions"].double(), p, x.double(), D.double(), pd, ell)
    # the transposed block through the same entry, into a view with a padded, unaligned leading dimension
    buf = torch.zeros(B * (pd + 1), M * (p + 1) + 3, device=gpu_device)
    Kt = ops.kernel_fwd_rect(ctx, px, B, pd, pz, M, p, d, hyp, out=buf[:, 1:M * (p + 1) + 1])
    errs = {"K_ZX": relmax(K, ref), "K_XZ": relmax(Kt, ref.t()), "max|K|": ref.abs().max().item()}
    _report("kernel_fwd_rect d=%d p1=%d p2=%d %dx%d" % (d, p, pd, M, B), errs)
    assert K.shape == (M * (p + 1), B * (pd + 1)) and K.dtype == torch.float32
    assert errs["K_ZX"] < KTOL and errs["K_XZ"] < KTOL, errs
    assert bool((buf[:, 0] == 0).all()) and bool((buf[:, M * (p + 1) + 1:] == 0).all())      # nothing outside the view


@gpu
@pytest.mark.parametrize("d,M,p,B,N", [(5, 40, 2, 128, 600), (200, 24, 3, 40, 400)])
def test_kernel_fwd_rect_at_equal_counts_is_as_accurate_as_the_square_kernel(dsvgp, gpu_device, d, M, p, B, N):
    """same expansion, same operand packs: at p1 == p2 the error against float64 may be at most twice that of dsvgp_kernel_fwd"""
    from test_gpu_step import make_problem
    P, x, _, _, _ = make_problem(N, d, M, p, B, seed=1)
    if d > 30:
        P["raw_lengthscale"] = torch.tensor([[_raw(0.4 * math.sqrt(d))]])
    D = torch.randn(B * p, d, generator=torch.Generator().manual_seed(5))
    ops, ctx, hyp, pz, px, ell, s = _packs(dsvgp, gpu_device, P, x, D, p, p)
    ref = s * O.kernel_matrix(P["inducing_points"].double(), x.double(), P["inducing_directions"].double(), D.double(), ell)
    e_rect = relmax(ops.kernel_fwd_rect(ctx, pz, M, p, px, B, p, d, hyp), ref)
    e_sq = relmax(ops.kernel_fwd(ctx, pz, M, px, B, d, p, hyp), ref)
    _report("equal counts d=%d p=%d %dx%d" % (d, p, M, B), {"kernel_fwd_rect": e_rect, "kernel_fwd": e_sq})
    assert e_rect < KTOL and e_rect <= 2 * e_sq, (e_rect, e_sq)


# ------------------------------------------------------------------ GPU 2: predict / predict_joint against the yardstick
@gpu
@pytest.mark.parametrize("d,M,p,pd,B,N", SHAPES, ids=IDS)
def test_predict_and_predict_joint_match_fp64(dsvgp, gpu_device, d, M, p, pd, B, N):
    P, x, D, mu_ref, Sig_ref, prior, noise, c = _case(d, M, p, pd, B, N)
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    Dg = D.to(dev) if pd else None
    mu, varn = eng.predict(Pg, x.to(dev), Dg)
    mu_j, Sigma = eng.predict_joint(Pg, x.to(dev), Dg)
    n = B * (pd + 1)
    errs = _nontrivial(mu_ref, Sig_ref, prior, c)
    errs.update({"mean": relmax(mu, mu_ref), "variance": relmax(varn, Sig_ref.diagonal() + noise), "joint mean": relmax(mu_j, mu_ref),
                 "covariance": relmax(Sigma, Sig_ref + noise * torch.eye(n, dtype=torch.float64)),
                 "diagonal vs variance": relmax(Sigma.diagonal(), varn)})
    _report("predict d=%d M=%d p=%d pd=%d B=%d" % (d, M, p, pd, B), errs)
    assert mu.shape == varn.shape == mu_j.shape == (n,) and Sigma.shape == (n, n)
    assert errs["mean"] < TOL and errs["variance"] < TOL and errs["joint mean"] < TOL, errs
    assert errs["covariance"] < CTOL and errs["diagonal vs variance"] < DTOL, errs


# ------------------------------------------------------------------ GPU 3: the value rows two ways
@gpu
def test_value_predictions_equal_the_value_rows_of_the_square_path(dsvgp, gpu_device):
    from test_gpu_step import make_problem
    dev = gpu_device
    P, x, _, D, _ = make_problem(600, 5, 40, 2, 128, seed=1)
    eng = dsvgp.ElboEngine(dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    mu0, var0 = eng.predict(Pg, x.to(dev), None)
    mu2, var2 = eng.predict(Pg, x.to(dev), D.to(dev))
    errs = {"mean": relmax(mu0, mu2[::3]), "variance": relmax(var0, var2[::3])}
    _report("predict(x, None) vs predict(x, D_p)[::p+1]", errs)
    assert mu0.shape == (128,) and max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ GPU 5: reproducibility
@gpu
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[6]], ids=[IDS[0], IDS[6]])
def test_two_identical_calls_are_bitwise_equal(dsvgp, gpu_device, shape):
    d, M, p, pd, B, N = shape
    P, x, D, *_ = _case(*shape)
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    xg, Dg = x.to(dev), (D.to(dev) if pd else None)
    (m1, v1), (m2, v2) = eng.predict(Pg, xg, Dg), eng.predict(Pg, xg, Dg)
    (j1, S1), (j2, S2) = eng.predict_joint(Pg, xg, Dg), eng.predict_joint(Pg, xg, Dg)
    assert torch.equal(m1, m2) and torch.equal(v1, v2) and torch.equal(j1, j2) and torch.equal(S1, S2)


# ------------------------------------------------------------------ GPU 6: natural parameters, shared directions
@gpu
def test_natural_parameters(dsvgp, gpu_device):
    from test_ngd import make_ngd_problem
    dev = gpu_device
    P, x, _, _, _ = make_ngd_problem(600, 5, 40, 2, 128)
    P64 = {k: v.double() for k, v in P.items()}
    m, LS = O.natural_to_mu_chol(P64["natural_vec"], P64["natural_mat"])
    Pc = {k: v for k, v in P64.items() if not k.startswith("natural_")}
    Pc["variational_mean"], Pc["chol_variational_covar"] = m, LS
    mu_ref, Sig_ref, _ = rect_predictive(Pc, x.double(), x.double()[:0], 0)
    noise = float(O.constrained(P64)[2])
    eng = dsvgp.ElboEngine(dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    mu, varn = eng.predict(Pg, x.to(dev), None)
    _, Sigma = eng.predict_joint(Pg, x.to(dev), None)
    errs = {"mean": relmax(mu, mu_ref), "variance": relmax(varn, Sig_ref.diagonal() + noise),
            "covariance": relmax(Sigma, Sig_ref + noise * torch.eye(128, dtype=torch.float64))}
    _report("natural parameters, pd = 0", errs)
    assert mu.shape == (128,) and max(errs.values()) < TOL, errs


@gpu
def test_shared_directions(dsvgp, gpu_device):
    from test_gpu_step import make_problem
    dev = gpu_device
    N, d, M, p, B = 600, 5, 40, 2, 128
    P, x, _, _, _ = make_problem(N, d, M, p, B, seed=1)
    g = torch.Generator().manual_seed(4)
    P["inducing_directions"] = torch.eye(d)[:p] + 0.2 * torch.randn(p, d, generator=g)        # ONE shared set
    P["variational_mean"] = 0.3 * torch.randn(M + p, generator=g)
    P["chol_variational_covar"] = torch.eye(M + p) + 0.05 * torch.randn(M + p, M + p, generator=g)
    P64 = {k: v.double() for k, v in P.items()}
    V, iv = O.shared_expand(P64["inducing_directions"], P64["variational_mean"], M)
    Q = dict(P64)
    Q["inducing_directions"], Q["variational_mean"] = V, iv
    Q["chol_variational_covar"] = torch.eye(iv.shape[0], dtype=torch.float64)      # zero middle term: S - I = 0
    mu_ref, Sig_ref, _ = rect_predictive(Q, x.double(), x.double()[:0], 0)
    noise = float(O.constrained(P64)[2])
    eng = dsvgp.ElboEngine(dev)
    eng.shared_directions = True
    Pg = {k: v.to(dev) for k, v in P.items()}
    mu, varn = eng.predict(Pg, x.to(dev), None)
    _, Sigma = eng.predict_joint(Pg, x.to(dev), None)
    errs = {"mean": relmax(mu, mu_ref), "variance": relmax(varn, Sig_ref.diagonal() + noise),
            "covariance": relmax(Sigma, Sig_ref + noise * torch.eye(B, dtype=torch.float64))}
    _report("shared directions, pd = 0", errs)
    assert mu.shape == (B,) and max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ GPU 4 / 7: model level
@pytest.fixture(scope="module")
def trained(dsvgp, gpu_device):
    """the 600-point, d = 2, p = 2 drop-in run of tests/test_gpu_mean_predictor.py, one epoch"""
    from torch.utils.data import TensorDataset
    torch.manual_seed(0)
    n, dim, n_test = 600, 2, 300
    train_x, test_x = torch.rand(n, dim), torch.rand(n_test, dim)
    train_y, test_y = O.testfun(train_x), O.testfun(test_x)
    model, likelihood = dsvgp.train_gp(TensorDataset(train_x, train_y), num_inducing=20, num_directions=2, minibatch_size=200,
                                       minibatch_dim=2, num_epochs=1, inducing_data_initialization=False, tqdm=False,
                                       verbose=False, seed=0)
    model.eval()
    likelihood.eval()
    return model, likelihood, test_x, test_y


@gpu
def test_posterior_with_the_models_count_is_the_models_distribution(trained, gpu_device):
    model, likelihood, test_x, _ = trained
    xg = test_x[:100].to(gpu_device)
    D = torch.eye(2, device=gpu_device).repeat(100, 1)
    with torch.no_grad():
        old, new = likelihood(model(xg, derivative_directions=D)), model.posterior(xg, D, likelihood)
        assert torch.equal(new.mean, old.mean) and torch.equal(new.variance, old.variance)
        assert torch.equal(new.covariance_matrix, old.covariance_matrix)
        old_f, new_f = model(xg, derivative_directions=D), model.posterior(xg, D)
        assert torch.equal(new_f.mean, old_f.mean) and torch.equal(new_f.variance, old_f.variance)
    assert new.mean.shape == (300,) and torch.equal(new.value_variance, old.variance[::3])
    with pytest.raises(AssertionError):                  # the call keeps the reference's assertion on a count mismatch (DGVS.py:106)
        model(xg, derivative_directions=D[:100])


@gpu
def test_model_posterior_eval_values_samples_and_cache_invalidation(dsvgp, trained, gpu_device, capsys):
    from torch.utils.data import TensorDataset
    model, likelihood, test_x, test_y = trained
    dev = gpu_device
    n_test, dim = test_x.shape
    dst = TensorDataset(test_x, test_y)
    means, variances = dsvgp.eval_values(dst, model, likelihood, minibatch_size=128)
    means_old, vars_old = dsvgp.eval_gp(dst, model, likelihood, num_directions=2, minibatch_size=128, minibatch_dim=2)
    capsys.readouterr()
    errs = {"eval_values mean": relmax(means, means_old[::3]), "eval_values variance": relmax(variances, vars_old[::3])}
    assert means.shape == variances.shape == (n_test,) and not means.is_cuda and not variances.is_cuda
    xg = test_x[:64].to(dev)
    B = xg.shape[0]
    post = model.posterior(xg, likelihood=likelihood)
    draws = post.sample(torch.Size([4]))
    assert draws.shape == (4, B) and torch.isfinite(draws).all()
    errs["sample at zero base samples vs mean"] = relmax(post.sample(torch.Size([4]), base_samples=torch.zeros(4, B, device=dev)),
                                                         post.mean.expand(4, B))
    lo, hi = post.confidence_region()
    assert bool((lo < post.mean).all()) and bool((post.mean < hi).all()) and torch.equal(post.value_variance, post.variance)
    # q(f) itself: the likelihood noise is gone from the diagonal
    noise = likelihood.noise.detach().reshape(())
    errs["variance with noise - noise vs q(f)"] = relmax(post.variance - noise, model.posterior(xg).variance)
    # values and the full gradient of a model trained with p = 2 = d here, and with pd = 1 != p
    full = model.posterior(xg, torch.eye(dim, device=dev).repeat(B, 1), likelihood)
    one = model.posterior(xg, torch.eye(dim, device=dev)[:1].repeat(B, 1), likelihood)
    assert full.variance.shape == (B * (dim + 1),) and one.variance.shape == (B * 2,) and one.covariance_matrix.shape == (B * 2, B * 2)
    errs["pd = 1 rows vs pd = d rows"] = relmax(one.variance, full.variance.reshape(B, 3)[:, :2].reshape(-1))
    errs["value_variance at pd = 1"] = relmax(one.value_variance, post.variance)
    _report("model level", errs)
    assert max(errs.values()) < TOL, errs
    # eval mode keeps the factor; an in-place parameter change is seen by the next call
    vm = model.variational_strategy._variational_distribution.variational_mean
    with torch.no_grad():
        vm.add_(0.1)
    try:
        moved = model.posterior(xg, likelihood=likelihood).mean
        assert not torch.equal(moved, post.mean)
    finally:
        with torch.no_grad():
            vm.sub_(0.1)


# ------------------------------------------------------------------ GPU 8: refusals
@gpu
def test_refusals(dsvgp, gpu_device):
    from test_gpu_step import make_problem
    from test_ngd import make_ngd_problem
    dev = gpu_device
    P, x, _, D, _ = make_problem(300, 3, 12, 2, 20, seed=1)
    Pg = {k: v.to(dev) for k, v in P.items()}
    xg = x.to(dev)
    D3 = torch.randn(20 * 3, 3, device=dev)
    Pn, xn, _, _, _ = make_ngd_problem(300, 3, 12, 2, 20)
    eng = dsvgp.ElboEngine(dev)
    eng.whitening = "ciq"
    for call in (eng.predict, eng.predict_joint):
        with pytest.raises(ValueError, match="CIQ"):
            call({k: v.to(dev) for k, v in Pn.items()}, xn.to(dev), None)
    eng = dsvgp.ElboEngine(dev)
    eng.data_outputs = "values"
    for call in (eng.predict, eng.predict_joint):
        with pytest.raises(ValueError, match="derivative-free"):
            call(Pg, xg, D3)
    assert eng.predict(Pg, xg, D.to(dev))[0].shape == (20,)          # the model's own count: the derivative-free path as before
    with pytest.raises(ValueError, match="derivative directions"):
        dsvgp.ElboEngine(dev).predict(Pg, xg, D3[:-1])
    # the C entry: empty problems, d = 0, q > 96, a leading dimension that is too small, a misaligned pack
    ops, lib = dsvgp._ops, dsvgp._lib.lib
    ctx = ops.Context.get(dev)
    hyp = torch.tensor([0.9, 1.7, 0.1, 0.0], device=dev)
    pz = ops.pack_points(ctx, Pg["inducing_points"], Pg["inducing_directions"], 2, hyp)
    px = ops.pack_points(ctx, xg, None, 0, hyp)
    out = torch.empty(36, 20, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr())

    def entry(n1=12, p1=2, n2=20, p2=0, d=3, ld=20, P1=pz[0].data_ptr()):
        return lib.dsvgp_kernel_fwd_rect(ctx.h, C.c_void_p(P1), vp(pz[1]), n1, p1, vp(px[0]), vp(px[1]), n2, p2, d, vp(hyp), vp(out), ld)

    assert entry() == 0
    assert entry(n1=0) == -1 and entry(n2=0) == -1 and entry(d=0) == -1 and entry(p1=96) == -1 and entry(p2=96) == -1
    assert entry(p1=-1) == -1 and entry(ld=19) == -1 and entry(P1=pz[0].data_ptr() + 4) == -1
    torch.cuda.synchronize()
