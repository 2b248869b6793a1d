"""Pathwise posterior samples on the GPU (dsvgp_paths_prepare / dsvgp_paths_eval, csrc/paths.hip; ElboEngine.sample_paths, SamplePaths,
ApproximateGP.sample_paths, eval_paths): draws of the posterior function with exact gradients.

The yardstick is ``path_reference`` of tests/test_paths_host.py (float64, c + Phi_X w + K_XZ' nu from the oracle's kernel), pinned there
to the oracle's predictive.  The HIP routes (fused kernel for d <= 32, GEMM-composed beyond) are held to it at the mean predictor's
tolerance (tests/test_gpu_mean_predictor.py: 2e-4, relative in max-norm over the whole output); measured errors are printed as
[parity] lines."""
import ctypes as C
import functools
import math

import pytest
import torch

import dsvgp_oracle as O
from test_paths_host import make_draws, path_nu, path_reference, relmax

gpu = pytest.mark.gpu
TOL = 2e-4
f64 = torch.float64

#          d    M  p    B    F  n
SHAPES = [(3, 12, 2, 70, 64, 3),          # the smallest; B crosses one 64-point tile
          (5, 40, 2, 130, 100, 5),        # ragged F
          (20, 70, 5, 33, 128, 9),        # M crosses the 64-point LDS chunk, D = 20; n = 9 crosses the group of 6 samples
          (32, 16, 0, 65, 96, 2),         # p = 0, last fused width
          (33, 16, 3, 40, 128, 4),        # first composed width
          (200, 24, 3, 40, 160, 3),       # rover width
          (5, 19, 5, 67, 1, 1)]           # F = n = 1, p = d
IDS = ["d%d-M%d-p%d-B%d-F%d-n%d" % s for s in SHAPES]
FUSED = [s for s in SHAPES if s[0] <= 32]
COMPOSED = [s for s in SHAPES if s[0] > 32]


def _report(tag, errs):
    print("[parity] %s: %s" % (tag, ", ".join("%s %.2e" % (k, v) for k, v in errs.items())))


def _raw(v):
    return math.log(math.expm1(v))          # softplus^-1


@functools.lru_cache(maxsize=None)
def _case(d, M, p, B, F, n):
    """(params fp32, x fp32, draws fp64, nu fp64 [n, M'], values fp64 [n, B], gradients fp64 [n, B, d]): once per shape, shared, never
    changed"""
    from test_gpu_step import make_problem
    P, x, _, _, _ = make_problem(600, d, M, p, B, seed=1)
    if d > 30:          # (tests/test_gpu_mean_predictor.py: otherwise the kernel between random points is numerically zero)
        P["raw_lengthscale"] = torch.tensor([[_raw(0.4 * math.sqrt(d))]])
    P64 = {k: v.double() for k, v in P.items()}
    draws = make_draws(d, M * (p + 1), F, n)
    val, grad = path_reference(P64, x.double(), draws)
    return P, x, draws, path_nu(P64, draws), val, grad


def _prepare(dsvgp, dev, P, nu, draws, p, sl=None):
    """the C entry on float64 nu from the CPU; ``sl``: a slice of the samples"""
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    hyp = ops.hyp_forward(ctx, Pg["raw_lengthscale"], Pg["raw_outputscale"], Pg["raw_noise"])
    Z, V = Pg["inducing_points"].contiguous(), Pg["inducing_directions"].contiguous()
    center = ops.column_mean(ctx, Z)
    sl = sl or slice(None)
    w = ops.paths_prepare(ctx, nu[sl].contiguous().to(dev), draws["w"][sl].contiguous().to(dev), draws["omega"].to(dev),
                          draws["phase"].to(dev), Z, V if p else None, p, hyp, Pg["constant"], center)
    return ctx, w


def _eval(dsvgp, dev, ctx, w, M, d, F, n, x, want_grad=True):
    ops = dsvgp._ops
    B = x.shape[0]
    need = ops.paths_workspace_bytes(M, d, F, n, B, want_grad)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    grads = torch.empty(n, B, d, device=dev) if want_grad else None
    vals = ops.paths_eval(ctx, w, M, d, F, n, x, None, grads, ws)
    return vals, grads


# ------------------------------------------------------------------ 1: the C entry against the yardstick
@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", SHAPES, ids=IDS)
def test_entry_matches_the_float64_yardstick(dsvgp, gpu_device, d, M, p, B, F, n):
    dev = gpu_device
    P, x, draws, nu, val_ref, grad_ref = _case(d, M, p, B, F, n)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    vals, grads = _eval(dsvgp, dev, ctx, w, M, d, F, n, x.to(dev))
    c = float(P["constant"].reshape(()))
    errs = {"values": relmax(vals, val_ref), "gradients": relmax(grads, grad_ref), "max|f - c|": (val_ref - c).abs().max().item(),
            "max|nu|": nu.abs().max().item()}
    _report("paths entry " + IDS[SHAPES.index((d, M, p, B, F, n))], errs)
    assert errs["max|f - c|"] >= 0.05                                            # the reference is not trivial
    assert vals.shape == (n, B) and grads.shape == (n, B, d)
    assert errs["values"] < TOL and errs["gradients"] < TOL, errs


# ------------------------------------------------------------------ 2: all draws zero: the posterior mean
@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", SHAPES, ids=IDS)
def test_zero_draws_give_the_mean_predictor(dsvgp, gpu_device, d, M, p, B, F, n):
    dev = gpu_device
    P, x, *_ = _case(d, M, p, B, F, n)
    Pg = {k: v.to(dev) for k, v in P.items()}
    eng = dsvgp.ElboEngine(dev)
    paths = eng.sample_paths(Pg, n, F, base_samples=make_draws(d, M * (p + 1), F, n, zero=True))
    vals, grads = paths.values_and_gradients(x.to(dev))
    mu, gmu = eng.mean_predictor(Pg).value_and_gradient(x.to(dev))
    errs = {"values": relmax(vals, mu[None].expand(n, B)), "gradients": relmax(grads, gmu[None].expand(n, B, d))}
    _report("paths at zero draws vs mean predictor " + IDS[SHAPES.index((d, M, p, B, F, n))], errs)
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ 3: a path is a function: batches and sample subsets
@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", FUSED, ids=[IDS[SHAPES.index(s)] for s in FUSED])
def test_fused_route_is_independent_of_the_batch_and_of_the_other_samples(dsvgp, gpu_device, d, M, p, B, F, n):
    dev = gpu_device
    P, x, draws, nu, *_ = _case(d, M, p, B, F, n)
    xg = x.to(dev)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    vals, grads = _eval(dsvgp, dev, ctx, w, M, d, F, n, xg)
    r0, r1 = 10, min(50, B)
    v_rows, g_rows = _eval(dsvgp, dev, ctx, w, M, d, F, n, xg[r0:r1].contiguous())
    assert torch.equal(v_rows, vals[:, r0:r1]) and torch.equal(g_rows, grads[:, r0:r1])
    if n >= 2:
        sl = slice(1, min(3, n))
        ns = sl.stop - sl.start
        _, w_sub = _prepare(dsvgp, dev, P, nu, draws, p, sl)
        v_sub, g_sub = _eval(dsvgp, dev, ctx, w_sub, M, d, F, ns, xg)
        assert torch.equal(v_sub, vals[sl]) and torch.equal(g_sub, grads[sl])


@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", COMPOSED, ids=[IDS[SHAPES.index(s)] for s in COMPOSED])
def test_composed_route_in_batches_and_sample_subsets(dsvgp, gpu_device, d, M, p, B, F, n):
    """the GEMM tiles see other neighbours in another batch: the difference is reported and, where it is not zero, held to the
    yardstick tolerance"""
    dev = gpu_device
    P, x, draws, nu, val_ref, grad_ref = _case(d, M, p, B, F, n)
    xg = x.to(dev)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    vals, grads = _eval(dsvgp, dev, ctx, w, M, d, F, n, xg)
    v_rows, g_rows = _eval(dsvgp, dev, ctx, w, M, d, F, n, xg[10:].contiguous())
    _, w_sub = _prepare(dsvgp, dev, P, nu, draws, p, slice(1, 3))
    v_sub, g_sub = _eval(dsvgp, dev, ctx, w_sub, M, d, F, 2, xg)
    vs, gs = val_ref.abs().max(), grad_ref.abs().max()
    errs = {"rows 10: values": ((v_rows - vals[:, 10:]).abs().max().cpu() / vs).item(),
            "rows 10: gradients": ((g_rows - grads[:, 10:]).abs().max().cpu() / gs).item(),
            "samples 1:3 values": ((v_sub - vals[1:3]).abs().max().cpu() / vs).item(),
            "samples 1:3 gradients": ((g_sub - grads[1:3]).abs().max().cpu() / gs).item()}
    _report("composed route, batches and subsets d=%d" % d, errs)
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ 4: reproducibility and guards
@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", [SHAPES[2], SHAPES[5]], ids=["fused", "composed"])
def test_bitwise_reproducible_guard_bands_untouched_and_values_alone(dsvgp, gpu_device, d, M, p, B, F, n):
    dev = gpu_device
    ops = dsvgp._ops
    P, x, draws, nu, *_ = _case(d, M, p, B, F, n)
    xg = x.to(dev)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    v1, g1 = _eval(dsvgp, dev, ctx, w, M, d, F, n, xg)
    v2, g2 = _eval(dsvgp, dev, ctx, w, M, d, F, n, xg)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    v3, _ = _eval(dsvgp, dev, ctx, w, M, d, F, n, xg, want_grad=False)
    assert torch.equal(v3, v1)                                                   # grads = NULL: the same values bits
    G = 256                                                                      # guard floats on either side (a multiple of 4)
    vbuf = torch.full((n * B + 2 * G,), float("nan"), device=dev)
    gbuf = torch.full((n * B * d + 2 * G,), float("nan"), device=dev)
    vv, gg = vbuf[G:G + n * B].view(n, B), gbuf[G:G + n * B * d].view(n, B, d)
    need = ops.paths_workspace_bytes(M, d, F, n, B, True)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    ops.paths_eval(ctx, w, M, d, F, n, xg, vv, gg, ws)
    assert torch.equal(vv, v1) and torch.equal(gg, g1)
    for buf, m in ((vbuf, n * B), (gbuf, n * B * d)):
        assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + m:]).all()
        assert not torch.isnan(buf[G:G + m]).any()


# ------------------------------------------------------------------ 5: engine and model
ENGINE = [SHAPES[1], SHAPES[3], SHAPES[5]]          # fused, the p = 0 model, composed


@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", ENGINE, ids=[IDS[SHAPES.index(s)] for s in ENGINE])
def test_engine_sample_paths_with_cpu_base_samples(dsvgp, gpu_device, d, M, p, B, F, n):
    """nu from the engine's own factor and solves (ElboEngine.sample_paths) against the yardstick with the oracle's factor"""
    dev = gpu_device
    P, x, draws, _, val_ref, grad_ref = _case(d, M, p, B, F, n)
    eng = dsvgp.ElboEngine(dev)
    paths = eng.sample_paths({k: v.to(dev) for k, v in P.items()}, n, F, base_samples={k: v.float() if k == "eps" else v for k, v in draws.items()})
    xg = x.to(dev)
    vals, grads = paths.values_and_gradients(xg)
    assert paths.num_samples == n and paths.num_features == F
    assert torch.equal(paths.values(xg), vals)
    # __call__(x, D): value row, then c + w^ . grad f for every direction, recombined here in float64
    pd = 2
    D = torch.randn(B * pd, d, generator=torch.Generator().manual_seed(5))
    out = paths(xg, D.to(dev))
    c = P["constant"].double().reshape(())
    rows = torch.einsum("nbk,bak->nba", grads.double().cpu(), O.normalize_rows(D.double()).view(B, pd, d)) + c
    recombined = torch.cat([vals.double().cpu()[..., None], rows], dim=2).reshape(n, B * (pd + 1))
    ref = torch.cat([val_ref[..., None], torch.einsum("nbk,bak->nba", grad_ref, O.normalize_rows(D.double()).view(B, pd, d)) + c], dim=2)
    errs = {"values": relmax(vals, val_ref), "gradients": relmax(grads, grad_ref), "__call__ vs recombined": relmax(out, recombined),
            "__call__ vs yardstick": relmax(out, ref.reshape(n, -1))}
    _report("engine sample_paths " + IDS[SHAPES.index((d, M, p, B, F, n))], errs)
    assert out.shape == (n, B * (pd + 1)) and torch.equal(paths(xg), vals)
    assert max(errs.values()) < TOL, errs


@gpu
def test_engine_natural_parameters_and_shared_directions(dsvgp, gpu_device):
    from test_gpu_step import make_problem
    from test_ngd import make_ngd_problem
    dev = gpu_device
    F, n = 64, 3
    # natural parameters
    P, x, _, _, _ = make_ngd_problem(600, 5, 40, 2, 64)
    P64 = {k: v.double() for k, v in P.items()}
    m, LS = O.natural_to_mu_chol(P64["natural_vec"], P64["natural_mat"])
    Pc = {k: v for k, v in P64.items() if not k.startswith("natural_")}
    Pc["variational_mean"], Pc["chol_variational_covar"] = m, LS
    draws = make_draws(5, 120, F, n)
    val_ref, grad_ref = path_reference(Pc, x.double(), draws)
    vals, grads = dsvgp.ElboEngine(dev).sample_paths({k: v.to(dev) for k, v in P.items()}, n, F, base_samples=draws).values_and_gradients(x.to(dev))
    errs = {"natural values": relmax(vals, val_ref), "natural gradients": relmax(grads, grad_ref)}
    # shared directions (tests/test_gpu_rect_predict.py): q(u)'s covariance does not reach the predictive, a unit factor stands in
    d, M, p, B = 5, 40, 2, 64
    P, x, _, _, _ = make_problem(600, d, M, p, B, seed=1)
    g = torch.Generator().manual_seed(4)
    P["inducing_directions"] = torch.eye(d)[:p] + 0.2 * torch.randn(p, d, generator=g)
    P["variational_mean"] = 0.3 * torch.randn(M + p, generator=g)
    P["chol_variational_covar"] = torch.eye(M + p) + 0.05 * torch.randn(M + p, M + p, generator=g)
    P64 = {k: v.double() for k, v in P.items()}
    V, iv = O.shared_expand(P64["inducing_directions"], P64["variational_mean"], M)
    Q = dict(P64)
    Q["inducing_directions"], Q["variational_mean"] = V, iv
    Q["chol_variational_covar"] = torch.eye(iv.shape[0], dtype=f64)
    val_ref, grad_ref = path_reference(Q, x.double(), draws)
    eng = dsvgp.ElboEngine(dev)
    eng.shared_directions = True
    vals, grads = eng.sample_paths({k: v.to(dev) for k, v in P.items()}, n, F, base_samples=draws).values_and_gradients(x.to(dev))
    errs.update({"shared values": relmax(vals, val_ref), "shared gradients": relmax(grads, grad_ref)})
    _report("engine sample_paths, natural parameters / shared directions", errs)
    assert max(errs.values()) < TOL, errs


@gpu
def test_model_sample_paths_and_eval_paths(dsvgp, gpu_device, capsys):
    from torch.utils.data import TensorDataset
    torch.manual_seed(0)
    dev = gpu_device
    n_tr, dim = 600, 2                    # the size of tests/test_gpu_mean_predictor.py's drop-in run, one epoch
    train_x, test_x = torch.rand(n_tr, dim), torch.rand(50, dim)
    train_y, test_y = O.testfun(train_x), O.testfun(test_x)
    model, _ = dsvgp.train_gp(TensorDataset(train_x, train_y), num_inducing=20, num_directions=2, minibatch_size=200, minibatch_dim=2,
                              num_epochs=1, inducing_data_initialization=False, tqdm=False, verbose=False, seed=0)
    capsys.readouterr()
    model.eval()
    n, F = 4, 64
    draws = make_draws(dim, 60, F, n)
    paths = model.sample_paths(n, num_features=F, base_samples=draws)
    assert isinstance(paths, dsvgp.SamplePaths) and model.sample_paths(n, num_features=F, base_samples=draws) is not paths
    xg = test_x.to(dev)
    vals, grads = paths.values_and_gradients(xg)
    P64 = {k: v.detach().double().cpu() for k, v in model._param_dict(None).items()}
    val_ref, grad_ref = path_reference(P64, test_x.double(), draws)
    errs = {"values": relmax(vals, val_ref), "gradients": relmax(grads, grad_ref)}
    _report("model.sample_paths", errs)
    assert max(errs.values()) < TOL, errs
    # minibatches of 16 on 50 points: the same functions, the same bits (fused route)
    v16, g16 = dsvgp.eval_paths(TensorDataset(test_x, test_y), paths, 16, gradients=True)
    assert v16.is_cuda and torch.equal(v16, vals) and torch.equal(g16, grads)
    assert torch.equal(dsvgp.eval_paths(xg, paths, 16), vals)
    # drawn on the device: another generator state, another function; the same state, the same function
    gen = torch.Generator(device=dev).manual_seed(3)
    a = model.sample_paths(2, num_features=F, generator=gen).values(xg)
    b = model.sample_paths(2, num_features=F, generator=gen).values(xg)
    gen.manual_seed(3)
    a2 = model.sample_paths(2, num_features=F, generator=gen).values(xg)
    assert torch.equal(a, a2) and not torch.equal(a, b) and torch.isfinite(a).all()


# ------------------------------------------------------------------ 6: memory
@gpu
def test_peak_memory_is_the_outputs_plus_the_reported_workspace(dsvgp, gpu_device):
    dev = gpu_device
    ops = dsvgp._ops
    M, d, p, B, n, F = 500, 20, 5, 4096, 16, 512
    g = torch.Generator().manual_seed(2)
    ctx = ops.Context.get(dev)
    Z = torch.rand(M, d, generator=g).to(dev)
    V = torch.randn(M * p, d, generator=g).to(dev)
    raw = torch.tensor([[0.5]], device=dev)
    hyp = ops.hyp_forward(ctx, raw, torch.tensor(0.2, device=dev), torch.tensor([-0.5], device=dev))
    w = ops.paths_prepare(ctx, 0.1 * torch.randn(n, M * (p + 1), generator=g, dtype=f64).to(dev),
                          torch.randn(n, F, generator=g, dtype=f64).to(dev), torch.randn(F, d, generator=g, dtype=f64).to(dev),
                          torch.rand(F, generator=g, dtype=f64).to(dev), Z, V, p, hyp, torch.tensor([0.1], device=dev),
                          ops.column_mean(ctx, Z))
    paths = dsvgp.SamplePaths(dev, w, M, d, F, n, torch.tensor(0.1, device=dev))
    x = torch.rand(B, d, generator=g).to(dev)
    torch.cuda.synchronize(dev)
    # the measurement must not depend on which modules ran before: a free cached block up to 1 MiB larger than an output is handed out
    # whole by the caching allocator and counted in full, and such blocks come and go with every GPU test module that runs earlier
    torch.cuda.empty_cache()
    # ... and emptying the cache does not return the free pieces of segments that tensors kept alive by earlier modules still sit in: a free
    # piece less than 1 MiB larger than the gradient output is handed out whole as well (seen: 6475776 > 5506048 bytes).  The call allocates
    # from a pool of its own, which starts without free pieces; the statistics are the device's and count it like any other allocation.
    pool = torch.cuda.MemPool()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    with torch.cuda.use_mem_pool(pool):
        vals, grads = paths.values_and_gradients(x)
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    outputs = 4 * (n * B + n * B * d)
    allowed = outputs + ops.paths_workspace_bytes(M, d, F, n, B, True) + 2 * 512      # (the allocator rounds each of the two outputs up to 512 bytes)
    print("[memory] peak %d bytes, outputs %d, workspace %d, B^2 floats %d" % (peak, outputs, allowed - outputs - 1024, 4 * B * B))
    assert torch.isfinite(vals).all() and torch.isfinite(grads).all()
    assert peak <= allowed, (peak, allowed)
    assert peak < 4 * B * B                                                          # nothing of size B x B
    del vals, grads                                                                  # (before the pool they live in)
    del pool


# ------------------------------------------------------------------ 7: refusals
@gpu
def test_refusals(dsvgp, gpu_device):
    dev = gpu_device
    d, M, p, B, F, n = SHAPES[0]
    P, x, draws, nu, *_ = _case(d, M, p, B, F, n)
    Pg = {k: v.to(dev) for k, v in P.items()}
    eng = dsvgp.ElboEngine(dev)
    eng.whitening = "ciq"
    with pytest.raises(NotImplementedError, match="msMINRES"):
        eng.sample_paths(Pg, 2)
    with pytest.raises(NotImplementedError, match="float64"):
        dsvgp.ElboEngine64(dev).sample_paths({k: v.double() for k, v in Pg.items()}, 2)
    paths = dsvgp.ElboEngine(dev).sample_paths(Pg, n, F, base_samples=draws)
    with pytest.raises(dsvgp._lib.DsvgpError):
        paths.values(x)                              # x on the CPU
    with pytest.raises(dsvgp._lib.DsvgpError):
        paths.values_and_gradients(x)
    with pytest.raises(ValueError, match="base_samples"):
        dsvgp.ElboEngine(dev).sample_paths(Pg, n, F, base_samples={k: v for k, v in draws.items() if k != "eta"})
    # the C entry: DSVGP_EINVAL for M, d, F, n or B < 1, a null required pointer, a misaligned weights, an intermediate past 2^31
    lib = dsvgp._lib.lib
    ctx = dsvgp._ops.Context.get(dev)
    vp = lambda t: C.c_void_p(t.data_ptr())
    w, xg = paths.weights, x.to(dev)
    out = torch.empty(n * B, device=dev)
    ev = lambda M_, d_, F_, n_, B_, wp=None, xp=None, op=None: lib.dsvgp_paths_eval(
        ctx.h, vp(w) if wp is None else wp, M_, d_, F_, n_, vp(xg) if xp is None else xp, B_, vp(out) if op is None else op, None, None)
    assert ev(M, d, F, n, B) == 0
    for bad in ((0, d, F, n, B), (M, 0, F, n, B), (M, d, 0, n, B), (M, d, F, 0, B), (M, d, F, n, 0)):
        assert ev(*bad) == -1, bad
    null = C.c_void_p(0)
    assert ev(M, d, F, n, B, wp=null) == -1 and ev(M, d, F, n, B, xp=null) == -1 and ev(M, d, F, n, B, op=null) == -1
    assert ev(M, d, F, n, B, wp=C.c_void_p(w.data_ptr() + 4)) == -1                  # misaligned weights
    assert lib.dsvgp_paths_eval(ctx.h, vp(w), 500, 200, 2048, 1, vp(xg), 2000000, vp(out), None, vp(out)) == -1    # B x F entries pass 2^31
    assert lib.dsvgp_paths_eval(ctx.h, vp(w), M, 40, F, n, vp(xg), B, vp(out), None, None) == -1                   # composed route without a workspace
    torch.cuda.synchronize(dev)
