"""Sample paths at their own points on the GPU: dsvgp_paths_eval_own and dsvgp_paths_descend (csrc/paths.hip), SamplePaths.values_at /
values_and_gradients_at / descend, directional_vi.thompson_candidates and ApproximateGP.thompson_step.

The yardstick is ``own_reference`` of tests/test_paths_own_host.py: ``path_reference(P64, x[s], draws)[.][s]`` per sample, float64 on
the CPU; both HIP routes (fused kernel for d <= 32, GEMM-composed beyond) are held to it at the paths' own 2e-4 relative max-norm.  The
descent is held to the float64 restatement of its rule ONE STEP AT A TIME, each step judged from the kernel's own state, so that no
error accumulates.  Measured errors are printed as [parity] lines."""
import ctypes as C
import functools

import pytest
import torch

from test_gpu_paths_hvp import _prepare
from test_paths_host import closed_form, make_draws, path_nu, relmax
from test_paths_own_host import DESCENT, DESCENT_IDS, descend_trial, descent_case, own_points, own_problem, own_reference

gpu = pytest.mark.gpu
TOL = 2e-4
f64 = torch.float64

#          d    M  p    B    F  n
SHAPES = [(3, 12, 2, 70, 64, 3),          # fused route; ragged second point tile, M < one chunk
          (5, 40, 2, 130, 100, 5),        # fused route; ragged feature chunk
          (20, 70, 5, 33, 128, 4),        # fused route; two inducing chunks
          (32, 16, 0, 65, 96, 2),         # fused route; p = 0; the last fused width
          (5, 19, 5, 67, 1, 1),           # fused route; F = 1, n = 1
          (33, 16, 3, 40, 128, 4),        # composed route; the first composed width
          (200, 24, 3, 40, 160, 3)]       # composed route; rover-like d
IDS = ["d%d-M%d-p%d-B%d-F%d-n%d" % s for s in SHAPES]
FUSED = [s for s in SHAPES if s[0] <= 32]
COMPOSED = [s for s in SHAPES if s[0] > 32]
ids = lambda shapes: [IDS[SHAPES.index(s)] for s in shapes]


def _report(tag, errs):
    print("[parity] %s: %s" % (tag, ", ".join("%s %.2e" % (k, v) for k, v in errs.items())))


@functools.lru_cache(maxsize=None)
def _case(d, M, p, B, F, n):
    """(params fp32, x fp32 [B, d], own points fp32 [n, B, d], draws fp64, nu fp64, values fp64 [n, B], gradients fp64 [n, B, d]):
    once per shape, shared, never changed"""
    P, P64, x = own_problem(d, M, p, B)
    draws = make_draws(d, M * (p + 1), F, n)
    xs = own_points(x, n)
    val, grad = own_reference(P64, xs, draws)
    return P, x.float(), xs.float(), draws, path_nu(P64, draws), val, grad


def _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xs, want_grad=True, values=None, grads=None):
    ops = dsvgp._ops
    B = xs.shape[1]
    need = ops.paths_own_workspace_bytes(M, d, F, n, B, want_grad)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    if want_grad and grads is None:
        grads = torch.empty(n, B, d, device=dev)
    values = ops.paths_eval_own(ctx, w, M, d, F, n, xs, values, grads if want_grad else None, ws)
    return values, grads


def _paths(dsvgp, dev, d, M, p, F, n, P, nu, draws):
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    return dsvgp.SamplePaths(dev, w, M, d, F, n, torch.zeros((), device=dev))


# ------------------------------------------------------------------ 1: the C entry and the engine against the yardstick
@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", SHAPES, ids=IDS)
def test_entry_matches_the_float64_yardstick(dsvgp, gpu_device, d, M, p, B, F, n):
    dev = gpu_device
    P, x, xs, draws, nu, ref_v, ref_g = _case(d, M, p, B, F, n)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    xg = xs.to(dev)
    val, grad = _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xg)
    errs = {"values": relmax(val, ref_v), "gradient": relmax(grad, ref_g), "max|f|": ref_v.abs().max().item(),
            "max|grad|": ref_g.abs().max().item()}
    _report("paths own entry " + IDS[SHAPES.index((d, M, p, B, F, n))], errs)
    assert val.shape == (n, B) and grad.shape == (n, B, d)
    assert errs["max|f|"] >= 0.05 and errs["max|grad|"] >= 0.05                  # the reference is not trivial
    assert errs["values"] < TOL and errs["gradient"] < TOL, errs
    alone, _ = _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xg, want_grad=False)    # grads = NULL: the same values bits
    assert torch.equal(alone, val)
    # all x[s] equal: the shared-point entry's result
    xb = x.to(dev)
    need = dsvgp._ops.paths_workspace_bytes(M, d, F, n, B, True)
    g_sh = torch.empty(n, B, d, device=dev)
    v_sh = dsvgp._ops.paths_eval(ctx, w, M, d, F, n, xb, None, g_sh, torch.empty(need, dtype=torch.uint8, device=dev) if need else None)
    v_eq, g_eq = _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xb[None].expand(n, B, d).contiguous())
    scale_v, scale_g = v_sh.abs().max().item(), g_sh.abs().max().item()
    same = {"values": (v_eq - v_sh).abs().max().item() / scale_v, "gradient": (g_eq - g_sh).abs().max().item() / scale_g}
    _report("own points all equal vs the shared-point entry (bitwise equal: %s)" % (torch.equal(v_eq, v_sh) and torch.equal(g_eq, g_sh)), same)
    assert max(same.values()) < TOL, same


@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", SHAPES, ids=IDS)
def test_engine_sample_paths_at_their_own_points(dsvgp, gpu_device, d, M, p, B, F, n):
    """nu from the engine's own factor and solves; ``values_at`` returns the values bits of ``values_and_gradients_at``; a workspace
    budget that cuts the points into blocks (d > 32) stays within the tolerance"""
    dev = gpu_device
    P, x, xs, draws, _, ref_v, ref_g = _case(d, M, p, B, F, n)
    paths = dsvgp.ElboEngine(dev).sample_paths({k: t.to(dev) for k, t in P.items()}, n, F, base_samples=draws)
    xg = xs.to(dev)
    val, grad = paths.values_and_gradients_at(xg)
    errs = {"values": relmax(val, ref_v), "gradient": relmax(grad, ref_g)}
    assert val.shape == (n, B) and grad.shape == (n, B, d)
    assert torch.equal(paths.values_at(xg), val)
    if d > 32:
        paths.workspace_budget = dsvgp._ops.paths_own_workspace_bytes(M, d, F, n, B, True) // 3
        v2, g2 = paths.values_and_gradients_at(xg)
        errs["values, blocks"], errs["gradient, blocks"] = relmax(v2, ref_v), relmax(g2, ref_g)
    _report("SamplePaths.values_and_gradients_at " + IDS[SHAPES.index((d, M, p, B, F, n))], errs)
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ 2: a result is a function of its sample and its point
@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", FUSED, ids=ids(FUSED))
def test_fused_route_is_independent_of_the_batch_the_other_samples_and_the_order(dsvgp, gpu_device, d, M, p, B, F, n):
    dev = gpu_device
    P, x, xs, draws, nu, _, _ = _case(d, M, p, B, F, n)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    xg = xs.to(dev)
    val, grad = _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xg)
    r0, r1 = 10, min(50, B)
    v, g = _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xg[:, r0:r1].contiguous())
    assert torch.equal(v, val[:, r0:r1]) and torch.equal(g, grad[:, r0:r1])
    if n >= 2:
        sl = slice(1, min(3, n))
        _, w_sub = _prepare(dsvgp, dev, P, nu, draws, p, sl)
        v, g = _eval_own(dsvgp, dev, ctx, w_sub, M, d, F, sl.stop - sl.start, xg[sl].contiguous())
        assert torch.equal(v, val[sl]) and torch.equal(g, grad[sl])
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5)).to(dev)
    v, g = _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xg[:, perm].contiguous())
    assert torch.equal(v, val[:, perm]) and torch.equal(g, grad[:, perm])


@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", COMPOSED, ids=ids(COMPOSED))
def test_composed_route_in_batches_sample_subsets_and_permuted(dsvgp, gpu_device, d, M, p, B, F, n):
    """the GEMM tiles see other neighbours in another batch: the differences are reported and held to the yardstick tolerance"""
    dev = gpu_device
    P, x, xs, draws, nu, ref_v, ref_g = _case(d, M, p, B, F, n)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    xg = xs.to(dev)
    val, grad = _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xg)
    sv, sg = ref_v.abs().max().item(), ref_g.abs().max().item()
    v1, g1 = _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xg[:, 10:].contiguous())
    _, w_sub = _prepare(dsvgp, dev, P, nu, draws, p, slice(1, 3))
    v2, g2 = _eval_own(dsvgp, dev, ctx, w_sub, M, d, F, 2, xg[1:3].contiguous())
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5)).to(dev)
    v3, g3 = _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xg[:, perm].contiguous())
    errs = {"rows 10: f": (v1 - val[:, 10:]).abs().max().item() / sv, "rows 10: g": (g1 - grad[:, 10:]).abs().max().item() / sg,
            "samples 1:3 f": (v2 - val[1:3]).abs().max().item() / sv, "samples 1:3 g": (g2 - grad[1:3]).abs().max().item() / sg,
            "permuted f": (v3 - val[:, perm]).abs().max().item() / sv, "permuted g": (g3 - grad[:, perm]).abs().max().item() / sg}
    _report("composed own points, batches, subsets and permutation d=%d" % d, errs)
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ 3: reproducibility and guards
def _guarded(shape, dev, dtype=torch.float32, G=256):
    numel = 1
    for s in shape:
        numel *= s
    fill = float("nan") if dtype.is_floating_point else -7
    buf = torch.full((numel + 2 * G,), fill, dtype=dtype, device=dev)
    untouched = lambda: bool((torch.isnan(buf[:G]).all() and torch.isnan(buf[G + numel:]).all()) if dtype.is_floating_point
                             else ((buf[:G] == -7).all() and (buf[G + numel:] == -7).all()))
    return buf[G:G + numel].view(*shape), untouched


@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", [SHAPES[2], SHAPES[6]], ids=["fused", "composed"])
def test_bitwise_reproducible_and_guard_bands_untouched(dsvgp, gpu_device, d, M, p, B, F, n):
    dev = gpu_device
    ops = dsvgp._ops
    P, x, xs, draws, nu, _, _ = _case(d, M, p, B, F, n)
    ctx, w = _prepare(dsvgp, dev, P, nu, draws, p)
    xg = xs.to(dev)
    v1, g1 = _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xg)
    v2, g2 = _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xg)
    assert torch.equal(v1, v2) and torch.equal(g1, g2) and torch.isfinite(v1).all() and torch.isfinite(g1).all()
    vv, v_ok = _guarded((n, B), dev)
    gg, g_ok = _guarded((n, B, d), dev)
    _eval_own(dsvgp, dev, ctx, w, M, d, F, n, xg, values=vv, grads=gg)
    assert torch.equal(vv, v1) and torch.equal(gg, g1) and v_ok() and g_ok()
    # the descent: every output inside its own guard band, two identical calls bitwise equal
    lo, hi = (t.to(dev) for t in (xs.amin(dim=(0, 1)) - 0.1, xs.amax(dim=(0, 1)) + 0.1))
    ws = torch.empty(ops.paths_descend_workspace_bytes(M, d, F, n, B), dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        bufs = [_guarded((n, B, d), dev), _guarded((n, B), dev), _guarded((n, B, d), dev), _guarded((n, B), dev),
                _guarded((n, B), dev, torch.int32)]
        xx, fv, gv, st, ac = (b[0] for b in bufs)
        xx.copy_(xg)
        ops.paths_descend(ctx, w, M, d, F, n, xx, lo, hi, 3, -1.0, False, False, fv, gv, st, ac, ws)
        assert all(b[1]() for b in bufs)
        assert all(bool(torch.isfinite(t).all()) for t in (xx, fv, gv, st))
        runs.append([t.clone() for t in (xx, fv, gv, st, ac)])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    # SamplePaths.descend leaves its starts alone
    paths = dsvgp.SamplePaths(dev, w, M, d, F, n, torch.zeros((), device=dev))
    keep = xg.clone()
    res = paths.descend(xg, lo, hi, iterations=3)
    assert torch.equal(xg, keep) and res.x.data_ptr() != xg.data_ptr()
    assert all(torch.equal(a, b) for a, b in zip(res, runs[0]))                  # (initial_step=None is the entry's 0.25 ell)


# ------------------------------------------------------------------ 4: the descent, one step at a time
def _descent_setup(dsvgp, dev, shape):
    d, M, p, B, F, n = shape
    P, P64, x0, lower, upper, draws, step0 = descent_case(*shape)
    paths = _paths(dsvgp, dev, d, M, p, F, n, P, path_nu(P64, draws), draws)
    return paths, P64, draws, x0.float().to(dev), lower.float().to(dev), upper.float().to(dev), step0


@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", DESCENT, ids=DESCENT_IDS)
def test_descent_single_step_consistency(dsvgp, gpu_device, d, M, p, B, F, n):
    """T = 4 as four resumed calls of one iteration.  From every returned state the float64 restatement takes one step (its f and g
    recomputed in float64 at the kernel's x, the kernel's step length): accepted iterates, values and gradients within TOL; rejected
    pairs bit-unchanged with the step halved exactly; the decision equals the sign of the float64 Armijo margin except where
    |margin| <= 1e-3 max|f(x0)| = 5 TOL (a difference of two values each good to TOL) -- those are left out and counted, at most 10 %
    per shape (the restatement alone: 3.8 % at d = 3, 1.1 % at d = 5, 0 elsewhere: tests/test_paths_own_host.py)."""
    dev = gpu_device
    paths, P64, draws, x0, lo, hi, step0 = _descent_setup(dsvgp, dev, (d, M, p, B, F, n))
    lo64, hi64 = lo.double().cpu(), hi.double().cpu()
    states = [paths.descend(x0, lo, hi, iterations=0, initial_step=step0)]
    for _ in range(4):
        states.append(paths.descend(None, lo, hi, iterations=1, initial_step=step0, state=states[-1]))
    start = states[0]
    assert torch.equal(start.x, torch.minimum(torch.maximum(x0, lo), hi)) and int(start.accepted.abs().sum()) == 0
    f_start, g_start = own_reference(P64, start.x.double().cpu(), draws, closed_form)
    scale = f_start.abs().max().item()
    errs = {"start f": relmax(start.values, f_start), "start g": relmax(start.gradients, g_start),
            "start eta |g|": relmax(start.steps * start.gradients.norm(dim=-1), torch.full((n, B), step0, dtype=f64))}
    left_out = wrong = total = 0
    for t in range(4):
        a, b = states[t], states[t + 1]
        xa = a.x.double().cpu()
        fa, ga = own_reference(P64, xa, draws, closed_form)
        y, fy, gy, margin = descend_trial(P64, xa, fa, ga, a.steps.double().cpu(), lo64, hi64, draws, False)
        took = (b.accepted - a.accepted).cpu()
        assert bool(((took == 0) | (took == 1)).all())
        took = took.bool()
        rej = (~took).to(dev)
        assert torch.equal(b.x[rej], a.x[rej]) and torch.equal(b.values[rej], a.values[rej]) and torch.equal(b.gradients[rej], a.gradients[rej])
        assert torch.equal(b.steps[rej], 0.5 * a.steps[rej]) and torch.equal(b.steps[~rej], 2.0 * a.steps[~rej])
        if bool(took.any()):
            errs["step %d x" % (t + 1)] = relmax(b.x.cpu()[took], y[took])
            errs["step %d f" % (t + 1)] = relmax(b.values.cpu()[took], fy[took])
            errs["step %d g" % (t + 1)] = relmax(b.gradients.cpu()[took], gy[took])
        clear = margin.abs() > 1e-3 * scale
        left_out += int((~clear).sum())
        wrong += int((took != (margin >= 0))[clear].sum())
        total += margin.numel()
        assert bool((b.x >= lo).all()) and bool((b.x <= hi).all())
    errs["share left out"] = left_out / total
    _report("descent, one step at a time " + DESCENT_IDS[DESCENT.index((d, M, p, B, F, n))], errs)
    assert wrong == 0, wrong
    assert left_out / total <= 0.10, (left_out, total)
    assert max(v for k, v in errs.items() if k != "share left out") < TOL, errs
    last = states[-1]
    at = paths.values_at(last.x)
    if d <= 32:
        once = paths.descend(x0, lo, hi, iterations=4, initial_step=step0)
        assert all(torch.equal(u, v) for u, v in zip(once, last))                # four one-iteration calls = one call of four
        assert torch.equal(last.values, at)
    else:
        assert relmax(last.values, at) < TOL


# ------------------------------------------------------------------ 5: the descent, outcome
@gpu
@pytest.mark.parametrize("d,M,p,B,F,n", DESCENT, ids=DESCENT_IDS)
def test_descent_outcome(dsvgp, gpu_device, d, M, p, B, F, n):
    """every pair ends strictly better than it started (the restatement alone gains at least 0.168 on a scale of 1.2 at d = 3 and more
    elsewhere: TOL-sized errors cannot flip this), inside the box exactly; clamps active and a degenerate box"""
    dev = gpu_device
    paths, P64, draws, x0, lo, hi, step0 = _descent_setup(dsvgp, dev, (d, M, p, B, F, n))
    start = paths.descend(x0, lo, hi, iterations=0, initial_step=step0)
    f_start, g_start = own_reference(P64, start.x.double().cpu(), draws)
    assert torch.equal(start.x, torch.minimum(torch.maximum(x0, lo), hi))
    assert relmax(start.values, f_start) < TOL and relmax(start.gradients, g_start) < TOL
    down = paths.descend(x0, lo, hi, iterations=4, initial_step=step0)
    up = paths.descend(x0, lo, hi, iterations=4, initial_step=step0, maximize=True)
    print("[descent] d=%d: least gain down %.3e, up %.3e on a scale of %.3e; accepted %d / %d of %d"
          % (d, (start.values - down.values).min().item(), (up.values - start.values).min().item(), f_start.abs().max().item(),
             int(down.accepted.sum()), int(up.accepted.sum()), 4 * n * B))
    assert bool((down.values < start.values).all()) and bool((up.values > start.values).all())
    for res in (down, up):
        assert bool((res.x >= lo).all()) and bool((res.x <= hi).all())
        assert all(bool(torch.isfinite(t).all()) for t in res[:4]) and int(res.accepted.min()) >= 0 and int(res.accepted.max()) <= 4
        # (the gradient's error is absolute -- it follows the size of the summed terms, not of their sum, which shrinks towards a
        #  stationary point -- so it is measured on the scale of the gradients at the start, the paths' own scale at these points)
        f_end, g_end = own_reference(P64, res.x.double().cpu(), draws)
        g_err = (res.gradients.double().cpu() - g_end).abs().max().item() / g_start.abs().max().item()
        assert relmax(res.values, f_end) < TOL and g_err < TOL, (relmax(res.values, f_end), g_err)
    # a tight box around one start: every start is clamped onto it and the clamps stay active
    c = x0[0, 0]
    tl, th = c - 0.02, c + 0.02
    t0 = paths.descend(x0, tl, th, iterations=0, initial_step=step0)
    t4 = paths.descend(x0, tl, th, iterations=4, initial_step=step0)
    assert bool((t4.x >= tl).all()) and bool((t4.x <= th).all()) and bool(((t4.x == tl) | (t4.x == th)).any())
    assert bool((t4.values <= t0.values).all()) and all(bool(torch.isfinite(t).all()) for t in t4[:4])
    # lower = upper: the trial is the point itself
    deg = paths.descend(x0, c, c, iterations=5, initial_step=step0)
    assert torch.equal(deg.x, c.expand(n, B, d)) and bool((deg.accepted == 5).all())
    assert all(bool(torch.isfinite(t).all()) for t in deg[:4])


# ------------------------------------------------------------------ 6: a Thompson step with refinement
@gpu
def test_thompson_candidates_and_model_thompson_step(dsvgp, gpu_device):
    dev = gpu_device
    d, M, p, N, F, n = 5, 40, 2, 130, 100, 5
    P, P64, x = own_problem(d, M, p, N)
    lo, hi = x.min(dim=0).values.float().to(dev) - 0.1, x.max(dim=0).values.float().to(dev) + 0.1
    cand = x.float().to(dev)
    draws = make_draws(d, M * (p + 1), F, n)

    def check(tag, paths, out, draws):
        x_next, f_next, f_best = out
        assert x_next.shape == (n, d) and f_next.shape == (n,) and f_best.shape == (n,)
        assert bool((x_next >= lo).all()) and bool((x_next <= hi).all())
        assert torch.equal(f_best, paths.values(cand).min(dim=1).values)
        assert bool((f_next <= f_best).all())
        ref = own_reference(P64, x_next.double().cpu()[:, None, :], draws)[0][:, 0]
        errs = {"f_next": relmax(f_next, ref), "least gain": (f_best - f_next).min().item()}
        _report(tag, errs)
        assert errs["f_next"] < TOL, errs

    paths = dsvgp.ElboEngine(dev).sample_paths({k: t.to(dev) for k, t in P.items()}, n, F, base_samples=draws)
    check("thompson_candidates", paths, dsvgp.thompson_candidates(paths, cand, lo, hi, num_starts=4, iterations=4), draws)
    up = dsvgp.thompson_candidates(paths, cand, lo, hi, num_starts=4, iterations=4, maximize=True)
    assert torch.equal(up[2], paths.values(cand).max(dim=1).values) and bool((up[1] >= up[2]).all())
    # the model: sample_paths with a generator, then the same; the draws are those of a generator with the same seed
    model = dsvgp.GPModel(P["inducing_points"].clone(), P["inducing_directions"].clone(), d)
    vd = model.variational_strategy._variational_distribution
    with torch.no_grad():
        vd.variational_mean.copy_(P["variational_mean"])
        vd.chol_variational_covar.copy_(P["chol_variational_covar"])
        model.mean_module.constant.copy_(P["constant"].reshape(model.mean_module.constant.shape))
        model.covar_module.raw_outputscale.copy_(P["raw_outputscale"].reshape(()))
        model.covar_module.base_kernel.raw_lengthscale.copy_(P["raw_lengthscale"].reshape(1, 1))
    model = model.to(dev).eval()
    gen = lambda: torch.Generator(device=dev).manual_seed(23)
    out = model.thompson_step(cand, lo, hi, n, num_starts=4, iterations=4, num_features=F, generator=gen())
    mpaths = model.sample_paths(n, num_features=F, generator=gen())
    again = dsvgp.thompson_candidates(mpaths, cand, lo, hi, num_starts=4, iterations=4)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    g = gen()
    rn = lambda *shape: torch.randn(*shape, dtype=f64, device=dev, generator=g)
    Mp = M * (p + 1)
    mdraws = {"omega": rn(F, d), "phase": 2.0 * torch.pi * torch.rand(F, dtype=f64, device=dev, generator=g), "w": rn(n, F),
              "eps": rn(n, Mp), "eta": rn(n, Mp)}
    check("model.thompson_step", mpaths, out, {k: t.cpu() for k, t in mdraws.items()})


# ------------------------------------------------------------------ 7: refusals
@gpu
def test_refusals(dsvgp, gpu_device):
    dev = gpu_device
    d, M, p, B, F, n = SHAPES[0]
    P, x, xs, draws, nu, _, _ = _case(d, M, p, B, F, n)
    paths = dsvgp.ElboEngine(dev).sample_paths({k: t.to(dev) for k, t in P.items()}, n, F, base_samples=draws)
    xg = xs.to(dev)
    lo, hi = xg.amin(dim=(0, 1)), xg.amax(dim=(0, 1))
    for call in (paths.values_at, paths.values_and_gradients_at, lambda t: paths.descend(t, lo, hi)):
        with pytest.raises(dsvgp._lib.DsvgpError):
            call(xs)                                     # on the CPU
        for bad in (xg[0], xg[:-1], xg[:, :, :-1], xg.reshape(n, B * d)):
            with pytest.raises(ValueError):
                call(bad)                                # not [n, B, d]
    with pytest.raises(dsvgp._lib.DsvgpError):
        paths.descend(xg, lo.cpu(), hi)
    with pytest.raises(dsvgp._lib.DsvgpError):
        paths.descend(xg, lo, hi.cpu())
    for blo, bhi in ((lo[:-1], hi), (lo, hi[None]), (lo, torch.cat([hi, hi]))):
        with pytest.raises(ValueError):
            paths.descend(xg, blo, bhi)                  # lower / upper not [d]
    with pytest.raises(ValueError):
        paths.descend(xg, lo, hi, iterations=-1)
    # the C entries: DSVGP_EINVAL for M, d, F, n or B < 1, a null required pointer, a misaligned weights, n > 65535, an intermediate
    # past 2^31 entries, a composed call without a workspace, iterations < 0
    lib = dsvgp._lib.lib
    ctx = dsvgp._ops.Context.get(dev)
    vp = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    w = paths.weights
    val, grad = torch.empty(n, B, device=dev), torch.empty(n, B, d, device=dev)
    ev = lambda M_, d_, F_, n_, B_, wp=None, xp=None, op=None, ws=None: lib.dsvgp_paths_eval_own(
        ctx.h, vp(w) if wp is None else wp, M_, d_, F_, n_, vp(xg) if xp is None else xp, B_, vp(val) if op is None else op, vp(grad), ws)
    assert ev(M, d, F, n, B) == 0
    for bad in ((0, d, F, n, B), (M, 0, F, n, B), (M, d, 0, n, B), (M, d, F, 0, B), (M, d, F, n, 0), (M, d, F, 65536, 1)):
        assert ev(*bad) == -1, bad
    assert ev(M, d, F, n, B, wp=null) == -1 and ev(M, d, F, n, B, xp=null) == -1 and ev(M, d, F, n, B, op=null) == -1
    assert ev(M, d, F, n, B, wp=C.c_void_p(w.data_ptr() + 4)) == -1                  # misaligned weights
    assert ev(500, 200, 2048, 64, 40000, ws=vp(grad)) == -1                          # n B x F entries pass 2^31
    assert ev(M, 40, F, n, B) == -1                                                  # composed route without a workspace
    st, ac = torch.empty(n, B, device=dev), torch.empty(n, B, dtype=torch.int32, device=dev)
    xx = xg.clone()
    ws = torch.empty(dsvgp._ops.paths_descend_workspace_bytes(M, d, F, n, B), dtype=torch.uint8, device=dev)
    ptrs = {"w": vp(w), "x": vp(xx), "lo": vp(lo), "hi": vp(hi), "val": vp(val), "grad": vp(grad), "st": vp(st), "ac": vp(ac), "ws": vp(ws)}

    def de(M_=M, d_=d, F_=F, n_=n, B_=B, it=1, **over):
        q = dict(ptrs, **over)
        return lib.dsvgp_paths_descend(ctx.h, q["w"], M_, d_, F_, n_, q["x"], B_, q["lo"], q["hi"], it, C.c_float(0.1), 0, 0, q["val"],
                                       q["grad"], q["st"], q["ac"], q["ws"])

    assert de() == 0 and de(it=0) == 0
    assert de(it=-1) == -1
    for k in ptrs:
        assert de(**{k: null}) == -1, k
    for kw in (dict(M_=0), dict(d_=0), dict(F_=0), dict(n_=0), dict(B_=0), dict(n_=65536, B_=1)):
        assert de(**kw) == -1, kw
    assert de(w=C.c_void_p(w.data_ptr() + 4)) == -1 and de(ws=C.c_void_p(ws.data_ptr() + 4)) == -1
    assert de(M_=500, d_=200, F_=2048, n_=64, B_=40000) == -1
    torch.cuda.synchronize(dev)
