"""Hessian-vector products of the paths and of the posterior mean on the GPU (dsvgp_paths_hvp, csrc/paths.hip; SamplePaths.hvp /
hessians, MeanPredictor.hvp / hessian, ApproximateGP.posterior_mean_hvp / posterior_mean_hessian).

The yardstick is ``hvp_reference`` of tests/test_paths_hvp_host.py: float64 autograd on the CPU through ``closed_form`` of
tests/test_paths_host.py (the returned gradient contracted with v and differentiated with respect to x); for the mean the same form
with zero draws.  Both HIP routes (fused kernel for d <= 32, GEMM-composed beyond) are held to it at the 2e-4 relative max-norm of
tests/test_gpu_paths.py and tests/test_gpu_mean_predictor.py; measured errors are printed as [parity] lines."""
import ctypes as C
import functools
import math

import pytest
import torch

import dsvgp_oracle as O
from test_paths_host import make_draws, path_nu, relmax
from test_paths_hvp_host import hvp_reference, unit_hessians

gpu = pytest.mark.gpu
TOL = 2e-4
f64 = torch.float64

#          d    M  p    B    F  n
SHAPES = [(3, 12, 2, 70, 64, 3),          # fused route; ragged last workgroup
          (5, 40, 2, 130, 100, 5),        # fused route; ragged feature chunk
          (20, 70, 5, 33, 128, 9),        # fused route; two inducing chunks; a partial last sample group (5 + 4)
          (32, 16, 0, 65, 96, 2),         # fused route; p = 0; the last fused width (one sample per group)
          (5, 19, 5, 67, 1, 1),           # fused route; F = 1, n = 1
          (33, 16, 3, 40, 128, 4),        # composed route
          (200, 24, 3, 40, 160, 3)]       # composed route
IDS = ["d%d-M%d-p%d-B%d-F%d-n%d" % s for s in SHAPES]
FUSED = [s for s in SHAPES if s[0] <= 32]
COMPOSED = [s for s in SHAPES if s[0] > 32]
ids = lambda shapes: [IDS[SHAPES.index(s)] for s in shapes]


def _report(tag, errs):
    print("[parity] %s: %s" % (tag, ", ".join("%s %.2e" % (k, v) for k, v in errs.items())))


def _raw(v):
    return math.log(math.expm1(v))          # softplus^-1


def _vectors(B, d):
    return torch.randn(B, d, generator=torch.Generator().manual_seed(11), dtype=f64)


@functools.lru_cache(maxsize=None)
def _problem(d, M, p, B):
    from test_gpu_step import make_problem
    P, x, _, _, _ = make_problem(600, d, M, p, B, seed=1)
    if d > 30:          # (tests/test_gpu_mean_predictor.py: otherwise the kernel between random points is numerically zero)
        P["raw_lengthscale"] = torch.tensor([[_raw(0.4 * math.sqrt(d))]])
    return P, {k: t.double() for k, t in P.items()}, x


@functools.lru_cache(maxsize=None)
def _case(d, M, p, B, F, n):
    """(params fp32, x fp32, v fp32, draws fp64, nu fp64 [n, M'], Hv fp64 [n, B, d]): once per shape, shared, never changed"""
    P, P64, x = _problem(d, M, p, B)
    draws = make_draws(d, M * (p + 1), F, n)
    v = _vectors(B, d).float()
    return P, x, v, draws, path_nu(P64, draws), hvp_reference(P64, x.double(), v.double(), draws)


@functools.lru_cache(maxsize=None)
def _mean_case(d, M, p, B):
    """(params fp32, x fp32, v fp32, Hv of the mean fp64 [B, d], Hessian of the mean fp64 [B, d, d]): the yardstick at zero draws"""
    P, P64, x = _problem(d, M, p, B)
    zero = make_draws(d, M * (p + 1), 1, 1, zero=True)
    v = _vectors(B, d).float()
    H = unit_hessians(lambda e: hvp_reference(P64, x.double(), e, zero)[0], B, d)
    return P, x, v, hvp_reference(P64, x.double(), v.double(), zero)[0], H


def _prepare(dsvgp, dev, P, nu, draws, p, sl=None):
    """dsvgp_paths_prepare on float64 nu from the CPU; ``sl``: a slice of the samples"""
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    Pg = {k: t.to(dev) for k, t in P.items()}
    hyp = ops.hyp_forward(ctx, Pg["raw_lengthscale"], Pg["raw_outputscale"], Pg["raw_noise"])
    Z, V = Pg["inducing_points"].contiguous(), Pg["inducing_directions"].contiguous()
    center = ops.column_mean(ctx, Z)
    sl = sl or slice(None)
    w = ops.paths_prepare(ctx, nu[sl].contiguous().to(dev), draws["w"][sl].contiguous().to(dev), draws["omega"].to(dev),
                          draws["phase"].to(dev), Z, V if p else None, p, hyp, Pg["constant"], center)
    return ctx, w


def _hvp(dsvgp, dev, ctx, w, M, d, F, n, x, v, hv=None):
    ops = dsvgp._ops
    need = ops.paths_hvp_workspace_bytes(M, d, F, n, x.shape[0])
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    return ops.paths_hvp(ctx, w, M, d, F, n, x, v, hv, ws)


# ------------------------------------------------------------------ 1: the C entry and the engine against the yardstick
@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", SHAPES, ids=IDS)
def test_entry_matches_the_float64_yardstick(dsvgp, gpu_device, d, M, p, B, F, n):
    dev = gpu_device
    P, x, v, draws, nu, ref = _case(d, M, p, B, F, n)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    hv = _hvp(dsvgp, dev, ctx, w, M, d, F, n, x.to(dev), v.to(dev))
    errs = {"Hv": relmax(hv, ref), "max|Hv|": ref.abs().max().item()}
    _report("paths hvp entry " + IDS[SHAPES.index((d, M, p, B, F, n))], errs)
    assert hv.shape == (n, B, d) and errs["max|Hv|"] >= 0.05                     # the reference is not trivial
    assert errs["Hv"] < TOL, errs


@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", SHAPES, ids=IDS)
def test_engine_sample_paths_hvp(dsvgp, gpu_device, d, M, p, B, F, n):
    """nu from the engine's own factor and solves (ElboEngine.sample_paths) against the yardstick with the oracle's factor;
    ``values_and_gradients`` on the same object returns the same bits before and after"""
    dev = gpu_device
    P, x, v, draws, _, ref = _case(d, M, p, B, F, n)
    paths = dsvgp.ElboEngine(dev).sample_paths({k: t.to(dev) for k, t in P.items()}, n, F, base_samples=draws)
    xg, vg = x.to(dev), v.to(dev)
    val0, grad0 = paths.values_and_gradients(xg)
    hv = paths.hvp(xg, vg)
    val1, grad1 = paths.values_and_gradients(xg)
    errs = {"Hv": relmax(hv, ref)}
    _report("SamplePaths.hvp " + IDS[SHAPES.index((d, M, p, B, F, n))], errs)
    assert hv.shape == (n, B, d) and errs["Hv"] < TOL, errs
    assert torch.equal(val0, val1) and torch.equal(grad0, grad1)


# ------------------------------------------------------------------ 2: the posterior mean
MEAN = [(5, 40, 2, 130), (33, 16, 3, 40)]          # one fused shape, one composed shape


@gpu
@pytest.mark.parametrize("d,M,p,B", MEAN, ids=["fused", "composed"])
def test_mean_predictor_hvp_and_hessian(dsvgp, gpu_device, d, M, p, B):
    dev = gpu_device
    P, x, v, ref, H_ref = _mean_case(d, M, p, B)
    Pg = {k: t.to(dev) for k, t in P.items()}
    pred = dsvgp.ElboEngine(dev).mean_predictor(Pg)
    xg = x.to(dev)
    mu0, g0 = pred.value_and_gradient(xg)
    hv, H = pred.hvp(xg, v.to(dev)), pred.hessian(xg)
    mu1, g1 = pred.value_and_gradient(xg)
    errs = {"Hv": relmax(hv, ref), "Hessian": relmax(H, H_ref), "max|H|": H_ref.abs().max().item()}
    _report("MeanPredictor.hvp / hessian d=%d" % d, errs)
    assert hv.shape == (B, d) and H.shape == (B, d, d) and errs["max|H|"] >= 0.05
    assert errs["Hv"] < TOL and errs["Hessian"] < TOL, errs
    assert torch.equal(H, H.transpose(1, 2))
    assert torch.equal(mu0, mu1) and torch.equal(g0, g1)                         # ``mean`` / ``value_and_gradient`` are untouched


@gpu
@pytest.mark.parametrize("d,M,p,B", MEAN, ids=["fused", "composed"])
def test_model_posterior_mean_hvp_and_hessian(dsvgp, gpu_device, d, M, p, B):
    dev = gpu_device
    P, x, v, ref, H_ref = _mean_case(d, M, p, B)
    model = dsvgp.GPModel(P["inducing_points"].clone(), P["inducing_directions"].clone(), d)
    vd = model.variational_strategy._variational_distribution
    with torch.no_grad():
        vd.variational_mean.copy_(P["variational_mean"])
        vd.chol_variational_covar.copy_(P["chol_variational_covar"])
        model.mean_module.constant.copy_(P["constant"].reshape(model.mean_module.constant.shape))
        model.covar_module.raw_outputscale.copy_(P["raw_outputscale"].reshape(()))
        model.covar_module.base_kernel.raw_lengthscale.copy_(P["raw_lengthscale"].reshape(1, 1))
    model = model.to(dev).eval()
    xg = x.to(dev)
    hv, H = model.posterior_mean_hvp(xg, v.to(dev)), model.posterior_mean_hessian(xg)
    errs = {"Hv": relmax(hv, ref), "Hessian": relmax(H, H_ref)}
    _report("model.posterior_mean_hvp / posterior_mean_hessian d=%d" % d, errs)
    assert hv.shape == (B, d) and H.shape == (B, d, d)
    assert max(errs.values()) < TOL, errs


@gpu
def test_mean_hvp_with_natural_parameters_and_shared_directions(dsvgp, gpu_device):
    from test_gpu_step import make_problem
    from test_ngd import make_ngd_problem
    dev = gpu_device
    # natural parameters
    P, x, _, _, _ = make_ngd_problem(600, 5, 40, 2, 64)
    P64 = {k: t.double() for k, t in P.items()}
    m, LS = O.natural_to_mu_chol(P64["natural_vec"], P64["natural_mat"])
    Pc = {k: t for k, t in P64.items() if not k.startswith("natural_")}
    Pc["variational_mean"], Pc["chol_variational_covar"] = m, LS
    zero = make_draws(5, 120, 1, 1, zero=True)
    v = _vectors(64, 5)
    ref = hvp_reference(Pc, x.double(), v, zero)[0]
    hv = dsvgp.ElboEngine(dev).mean_predictor({k: t.to(dev) for k, t in P.items()}).hvp(x.to(dev), v.float().to(dev))
    errs = {"natural": relmax(hv, ref)}
    # shared directions (tests/test_gpu_paths.py)
    d, M, p, B = 5, 40, 2, 64
    P, x, _, _, _ = make_problem(600, d, M, p, B, seed=1)
    g = torch.Generator().manual_seed(4)
    P["inducing_directions"] = torch.eye(d)[:p] + 0.2 * torch.randn(p, d, generator=g)
    P["variational_mean"] = 0.3 * torch.randn(M + p, generator=g)
    P["chol_variational_covar"] = torch.eye(M + p) + 0.05 * torch.randn(M + p, M + p, generator=g)
    P64 = {k: t.double() for k, t in P.items()}
    V, iv = O.shared_expand(P64["inducing_directions"], P64["variational_mean"], M)
    Q = dict(P64)
    Q["inducing_directions"], Q["variational_mean"] = V, iv
    Q["chol_variational_covar"] = torch.eye(iv.shape[0], dtype=f64)
    ref = hvp_reference(Q, x.double(), v, make_draws(d, iv.shape[0], 1, 1, zero=True))[0]
    eng = dsvgp.ElboEngine(dev)
    eng.shared_directions = True
    hv = eng.mean_predictor({k: t.to(dev) for k, t in P.items()}).hvp(x.to(dev), v.float().to(dev))
    errs["shared"] = relmax(hv, ref)
    _report("MeanPredictor.hvp, natural parameters / shared directions", errs)
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ 3: Hessians from products
@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", [SHAPES[1], SHAPES[5]], ids=["fused", "composed"])
def test_hessians_are_symmetric_and_their_rows_are_single_products(dsvgp, gpu_device, d, M, p, B, F, n):
    dev = gpu_device
    P, x, _, draws, nu, _ = _case(d, M, p, B, F, n)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    paths = dsvgp.SamplePaths(dev, w, M, d, F, n, torch.zeros((), device=dev))
    xg = x.to(dev)
    H = paths.hessians(xg)
    assert H.shape == (n, B, d, d) and torch.equal(H, H.transpose(2, 3))
    scale = H.abs().max().item()
    worst = 0.0
    for k in range(d):
        e = torch.zeros(B, d, device=dev)
        e[:, k] = 1.0
        worst = max(worst, (paths.hvp(xg, e) - H[:, :, k, :]).abs().max().item() / scale)
    _report("rows of hessians vs single products d=%d" % d, {"worst row": worst, "max|H|": scale})
    assert scale >= 0.05 and worst < TOL, worst
    paths.workspace_budget = 4 * n * B * d * d - 1
    with pytest.raises(ValueError, match=str(4 * n * B * d * d)):
        paths.hessians(xg)


# ------------------------------------------------------------------ 4: a product is a function of its sample, point and vector
@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", FUSED, ids=ids(FUSED))
def test_fused_route_is_independent_of_the_batch_and_linear_in_v(dsvgp, gpu_device, d, M, p, B, F, n):
    dev = gpu_device
    P, x, v, draws, nu, _ = _case(d, M, p, B, F, n)
    xg, vg = x.to(dev), v.to(dev)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    hv = _hvp(dsvgp, dev, ctx, w, M, d, F, n, xg, vg)
    r0, r1 = 10, min(50, B)
    rows = _hvp(dsvgp, dev, ctx, w, M, d, F, n, xg[r0:r1].contiguous(), vg[r0:r1].contiguous())
    assert torch.equal(rows, hv[:, r0:r1])
    if n >= 2:
        sl = slice(1, min(3, n))
        _, w_sub = _prepare(dsvgp, dev, P, nu, draws, p, sl)
        assert torch.equal(_hvp(dsvgp, dev, ctx, w_sub, M, d, F, sl.stop - sl.start, xg, vg), hv[sl])
    assert torch.equal(_hvp(dsvgp, dev, ctx, w, M, d, F, n, xg, 2 * vg), 2 * hv)
    assert bool((_hvp(dsvgp, dev, ctx, w, M, d, F, n, xg, torch.zeros_like(vg)) == 0).all())


@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", COMPOSED, ids=ids(COMPOSED))
def test_composed_route_in_batches_sample_subsets_and_scaled_v(dsvgp, gpu_device, d, M, p, B, F, n):
    """the GEMM tiles see other neighbours in another batch: the differences are reported and held to the yardstick tolerance"""
    dev = gpu_device
    P, x, v, draws, nu, ref = _case(d, M, p, B, F, n)
    xg, vg = x.to(dev), v.to(dev)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    hv = _hvp(dsvgp, dev, ctx, w, M, d, F, n, xg, vg)
    rows = _hvp(dsvgp, dev, ctx, w, M, d, F, n, xg[10:].contiguous(), vg[10:].contiguous())
    _, w_sub = _prepare(dsvgp, dev, P, nu, draws, p, slice(1, 3))
    sub = _hvp(dsvgp, dev, ctx, w_sub, M, d, F, 2, xg, vg)
    twice = _hvp(dsvgp, dev, ctx, w, M, d, F, n, xg, 2 * vg)
    zero = _hvp(dsvgp, dev, ctx, w, M, d, F, n, xg, torch.zeros_like(vg))
    scale = ref.abs().max().item()
    errs = {"rows 10:": (rows - hv[:, 10:]).abs().max().item() / scale, "samples 1:3": (sub - hv[1:3]).abs().max().item() / scale,
            "2 v": (twice - 2 * hv).abs().max().item() / scale, "v = 0": zero.abs().max().item() / scale}
    _report("composed hvp, batches, subsets and scaled v d=%d" % d, errs)
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ 5: reproducibility and guards
@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", [SHAPES[2], SHAPES[6]], ids=["fused", "composed"])
def test_bitwise_reproducible_and_guard_bands_untouched(dsvgp, gpu_device, d, M, p, B, F, n):
    dev = gpu_device
    P, x, v, draws, nu, _ = _case(d, M, p, B, F, n)
    xg, vg = x.to(dev), v.to(dev)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    h1 = _hvp(dsvgp, dev, ctx, w, M, d, F, n, xg, vg)
    h2 = _hvp(dsvgp, dev, ctx, w, M, d, F, n, xg, vg)
    assert torch.equal(h1, h2) and torch.isfinite(h1).all()
    G = 256                                                                      # guard floats on either side (a multiple of 4)
    buf = torch.full((n * B * d + 2 * G,), float("nan"), device=dev)
    hh = buf[G:G + n * B * d].view(n, B, d)
    _hvp(dsvgp, dev, ctx, w, M, d, F, n, xg, vg, hh)
    assert torch.equal(hh, h1)
    assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n * B * d:]).all()


# ------------------------------------------------------------------ 6: refusals
@gpu
def test_refusals(dsvgp, gpu_device):
    dev = gpu_device
    d, M, p, B, F, n = SHAPES[0]
    P, x, v, draws, nu, _ = _case(d, M, p, B, F, n)
    Pg = {k: t.to(dev) for k, t in P.items()}
    eng = dsvgp.ElboEngine(dev)
    paths = eng.sample_paths(Pg, n, F, base_samples=draws)
    pred = eng.mean_predictor(Pg)
    xg, vg = x.to(dev), v.to(dev)
    for obj in (paths, pred):
        with pytest.raises(dsvgp._lib.DsvgpError):
            obj.hvp(x, v)                                # both on the CPU
        with pytest.raises(dsvgp._lib.DsvgpError):
            obj.hvp(xg, v)                               # v on the CPU
        with pytest.raises(ValueError):
            obj.hvp(xg, vg[:-1])                         # v is not [B, d]
        with pytest.raises(ValueError):
            obj.hvp(xg, vg[:, :-1])
    with pytest.raises(dsvgp._lib.DsvgpError):
        paths.hessians(x)
    with pytest.raises(dsvgp._lib.DsvgpError):
        pred.hessian(x)
    # the C entry: DSVGP_EINVAL for M, d, F, n or B < 1, a null required pointer, a misaligned weights, an intermediate past 2^31
    lib = dsvgp._lib.lib
    ctx = dsvgp._ops.Context.get(dev)
    vp = lambda t: C.c_void_p(t.data_ptr())
    w = paths.weights
    out = torch.empty(n * B * d, device=dev)
    null = C.c_void_p(0)
    ev = lambda M_, d_, F_, n_, B_, wp=None, xp=None, vv=None, op=None: lib.dsvgp_paths_hvp(
        ctx.h, vp(w) if wp is None else wp, M_, d_, F_, n_, vp(xg) if xp is None else xp, vp(vg) if vv is None else vv, B_,
        vp(out) if op is None else op, None)
    assert ev(M, d, F, n, B) == 0
    for bad in ((0, d, F, n, B), (M, 0, F, n, B), (M, d, 0, n, B), (M, d, F, 0, B), (M, d, F, n, 0)):
        assert ev(*bad) == -1, bad
    assert ev(M, d, F, n, B, wp=null) == -1 and ev(M, d, F, n, B, xp=null) == -1
    assert ev(M, d, F, n, B, vv=null) == -1 and ev(M, d, F, n, B, op=null) == -1
    assert ev(M, d, F, n, B, wp=C.c_void_p(w.data_ptr() + 4)) == -1                  # misaligned weights
    assert lib.dsvgp_paths_hvp(ctx.h, vp(w), 500, 200, 2048, 1, vp(xg), vp(vg), 2000000, vp(out), vp(out)) == -1   # B x F entries pass 2^31
    assert lib.dsvgp_paths_hvp(ctx.h, vp(w), M, 40, F, n, vp(xg), vp(vg), B, vp(out), None) == -1                  # composed route without a workspace
    torch.cuda.synchronize(dev)
