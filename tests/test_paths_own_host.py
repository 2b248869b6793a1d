"""CPU: the surface and the float64 restatement of the own-point evaluation of the sample paths and of the descent built on it
(dsvgp_paths_eval_own / dsvgp_paths_descend, csrc/paths.hip; SamplePaths.values_at / values_and_gradients_at / descend,
directional_vi.thompson_candidates, ApproximateGP.thompson_step).

The own-point yardstick is ``path_reference(P64, x[s], draws)[.][s]`` of tests/test_paths_host.py per sample.  ``descend_reference``
restates the descent rule of include/dsvgp.h in float64 on ``closed_form``: clamp, evaluate, eta = step0 / max(|g|, tiny), then per
iteration one trial y = clamp(x - sigma eta g), accepted iff sigma f_y <= sigma f + c1 sigma g.(y - x), eta doubled or halved.
tests/test_gpu_paths_own.py imports the helpers and holds the kernels to them one step at a time."""
import functools
import inspect
import math
import os
import re

import pytest
import torch

import dsvgp_oracle as O
from test_paths_host import closed_form, make_draws, path_reference, problem, relmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = torch.float64
C1, GROW, SHRINK, ETA_MAX, TINY = 1e-4, 2.0, 0.5, 1e30, 1e-30          # csrc/paths_plan.h

#            d    M  p   B    F  n
DESCENT = [(3, 12, 2, 20, 64, 3), (5, 40, 2, 32, 100, 5), (20, 70, 5, 33, 128, 4), (32, 16, 0, 20, 96, 2), (33, 16, 3, 20, 128, 4),
           (200, 24, 3, 12, 160, 3)]
DESCENT_IDS = ["d%d-M%d-p%d-B%d-F%d-n%d" % s for s in DESCENT]


def _raw(v):
    return math.log(math.expm1(v))          # softplus^-1


@functools.lru_cache(maxsize=None)
def own_problem(d, M, p, B):
    """(P fp32, P64, x fp64 [B, d]) of test_paths_host.problem with the lengthscale 0.4 sqrt(d) for d > 30 (tests/test_gpu_paths_hvp.py:
    otherwise the kernel between random points is numerically zero); once per shape, shared, never changed"""
    P, P64, x = problem(d, M, p, B)
    if d > 30:
        P = dict(P)
        P["raw_lengthscale"] = torch.tensor([[_raw(0.4 * math.sqrt(d))]])
        P64 = {k: t.double() for k, t in P.items()}
    return P, P64, x


def own_points(x, n):
    """x[s] = x + 0.05 randn(n, B, d): the first use of a generator seeded with 3, float64"""
    B, d = x.shape
    return x[None] + 0.05 * torch.randn(n, B, d, generator=torch.Generator().manual_seed(3), dtype=f64)


def own_reference(P64, xs, draws, form=path_reference):
    """(values [n, B], gradients [n, B, d]) of sample s at its own points xs[s], float64: ``form(P64, xs[s], draws)[.][s]`` per sample"""
    vals, grads = [], []
    for s in range(xs.shape[0]):
        v, g = form(P64, xs[s].contiguous(), draws)
        vals.append(v[s])
        grads.append(g[s])
    return torch.stack(vals), torch.stack(grads)


def descend_box(x):
    """[min_b x - 0.1, max_b x + 0.1] per coordinate"""
    return x.min(dim=0).values - 0.1, x.max(dim=0).values + 0.1


def descend_start(P64, x0, lower, upper, draws, initial_step, maximize):
    """the start state (x, f, g, eta, accepted) of the rule, float64"""
    x = torch.minimum(torch.maximum(x0, lower), upper)
    f, g = own_reference(P64, x, draws, closed_form)
    step0 = initial_step if initial_step is not None and initial_step > 0 else 0.25 * O.constrained(P64)[0].item()
    eta = step0 / g.norm(dim=-1).clamp_min(TINY)
    return x, f, g, eta, torch.zeros(f.shape, dtype=torch.int64)


def descend_trial(P64, x, f, g, eta, lower, upper, draws, maximize):
    """one trial from a state: (y, f_y, g_y, margin) with margin = sigma f + c1 sigma g.(y - x) - sigma f_y, accepted iff >= 0"""
    sg = -1.0 if maximize else 1.0
    y = torch.minimum(torch.maximum(x - sg * eta[..., None] * g, lower), upper)
    fy, gy = own_reference(P64, y, draws, closed_form)
    margin = sg * f + C1 * sg * (g * (y - x)).sum(-1) - sg * fy
    return y, fy, gy, margin


def descend_reference(P64, x0, lower, upper, draws, T, initial_step, maximize, trace=None):
    """float64 restatement of dsvgp_paths_descend: (x, f, g, eta, accepted) after T iterations; ``trace``: a list that receives
    (margin, f) of every iteration"""
    x, f, g, eta, acc = descend_start(P64, x0, lower, upper, draws, initial_step, maximize)
    for _ in range(T):
        y, fy, gy, margin = descend_trial(P64, x, f, g, eta, lower, upper, draws, maximize)
        take = margin >= 0                                          # (a NaN margin compares false: rejected)
        x = torch.where(take[..., None], y, x)
        g = torch.where(take[..., None], gy, g)
        f = torch.where(take, fy, f)
        eta = torch.where(take, (GROW * eta).clamp_max(ETA_MAX), SHRINK * eta)
        acc = acc + take.long()
        if trace is not None:
            trace.append((margin, f.clone()))
    return x, f, g, eta, acc


@functools.lru_cache(maxsize=None)
def descent_case(d, M, p, B, F, n):
    """(P fp32, P64, x0 fp64 [n, B, d], lower, upper fp64 [d], draws, initial_step = 0.25 ell): once per shape, shared, never changed"""
    P, P64, x = own_problem(d, M, p, B)
    draws = make_draws(d, M * (p + 1), F, n)
    lower, upper = descend_box(x)
    return P, P64, own_points(x, n), lower, upper, draws, 0.25 * O.constrained(P64)[0].item()


# ------------------------------------------------------------------ the surface
NEW = {"dsvgp_paths_own_workspace_bytes": 6, "dsvgp_paths_eval_own": 11, "dsvgp_paths_descend_workspace_bytes": 5, "dsvgp_paths_descend": 19}


def test_library_exports_declares_and_binds_the_new_entries(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n, nargs in NEW.items():
        assert hasattr(dsvgp._lib.lib, n), "missing export: " + n
        assert n in dsvgp._lib.SIGNATURES, "missing binding: " + n
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, hdr, flags=re.S)
        assert decl, "not declared in include/dsvgp.h: " + n
        assert len(decl.group(1).split(",")) == len(dsvgp._lib.SIGNATURES[n][1]) == nargs, n
    plan = open(os.path.join(os.path.dirname(dsvgp._lib.__file__), "csrc", "paths_plan.h")).read()
    for name, value in (("PP_DESCEND_C1", "1e-4f"), ("PP_DESCEND_GROW", "2.f"), ("PP_DESCEND_SHRINK", "0.5f")):
        assert re.search(r"constexpr float %s = %s;" % (name, re.escape(value)), plan), name


def test_size_helpers_are_host_functions_and_refuse_with_zero(dsvgp):
    own, desc = dsvgp._ops.paths_own_workspace_bytes, dsvgp._ops.paths_descend_workspace_bytes
    assert own(12, 3, 64, 2, 100, 1) == 0 and own(12, 32, 64, 2, 100, 1) == 0          # fused route: registers and LDS only
    # (the descent keeps the trial point, its value and its gradient in the workspace on both routes)
    assert desc(12, 3, 64, 2, 100) == 4 * (2 * 2 * 100 * 3 + 2 * 100) and desc(12, 32, 64, 2, 100) > 0
    for bad in ((0, 3, 64, 1, 8), (12, 0, 64, 1, 8), (12, 3, 0, 1, 8), (12, 3, 64, 0, 8), (12, 3, 64, 1, 0), (-1, 3, 64, 1, 8),
                (0, 40, 64, 1, 8), (12, 40, 64, 1, 0), (12, 40, 64, 65536, 8)):
        assert own(*bad, 1) == 0 and own(*bad, 0) == 0 and desc(*bad) == 0, bad
    assert own(500, 200, 2048, 64, 40000, 1) == 0 and desc(500, 200, 2048, 64, 40000) == 0      # n B x F passes 2^31 entries: refused
    assert desc(12, 3, 64, 65535, 65535) == 0                                                   # n B passes 2^31
    assert 0 < own(12, 33, 64, 2, 100, 0) < own(12, 33, 64, 2, 100, 1) < own(12, 33, 64, 2, 200, 1)          # B
    assert own(12, 33, 64, 2, 200, 1) < own(12, 33, 64, 3, 200, 1) < own(24, 33, 64, 3, 200, 1)              # n, M
    assert own(12, 33, 64, 2, 100, 1) < desc(12, 33, 64, 2, 100) < desc(12, 33, 64, 2, 200) < desc(12, 33, 64, 3, 200) < desc(24, 33, 64, 3, 200)
    assert own(12, 33, 64, 2, 100, 1) % 16 == 0 and desc(12, 33, 64, 2, 100) % 16 == 0
    # nothing of size B x B: linear in B at the rover-like shape
    for fn in (lambda B: own(512, 200, 2048, 5, B, 1), lambda B: desc(512, 200, 2048, 5, B)):
        one, two = fn(2500), fn(5000)
        assert 0 < one < two <= 2 * one + 4096, (one, two)


def test_model_and_harness_carry_the_new_entry_points(dsvgp):
    from dsvgp_amd import directional_vi, shared_directional_vi
    from dsvgp_amd.gp_shim import ApproximateGP
    sp = dsvgp.SamplePaths
    assert list(inspect.signature(sp.values_at).parameters) == ["self", "x"]
    assert list(inspect.signature(sp.values_and_gradients_at).parameters) == ["self", "x"]
    sig = inspect.signature(sp.descend)
    assert list(sig.parameters) == ["self", "x0", "lower", "upper", "iterations", "initial_step", "maximize", "state"]
    assert [sig.parameters[k].default for k in ("iterations", "initial_step", "maximize", "state")] == [20, None, False, None]
    assert dsvgp.PathDescent._fields == ("x", "values", "gradients", "steps", "accepted")
    sig = inspect.signature(directional_vi.thompson_candidates)
    assert list(sig.parameters) == ["paths", "candidates", "lower", "upper", "num_starts", "iterations", "maximize"]
    assert [sig.parameters[k].default for k in ("num_starts", "iterations", "maximize")] == [8, 20, False]
    assert dsvgp.thompson_candidates is directional_vi.thompson_candidates
    assert shared_directional_vi.thompson_candidates is directional_vi.thompson_candidates
    sig = inspect.signature(ApproximateGP.thompson_step)
    assert list(sig.parameters) == ["self", "candidates", "lower", "upper", "num_samples", "num_starts", "iterations", "num_features",
                                    "maximize", "generator"]
    assert [sig.parameters[k].default for k in ("num_starts", "iterations", "num_features", "maximize", "generator")] == [8, 20, 2048, False, None]


def test_thompson_step_refuses_before_touching_a_device(dsvgp):
    """float64 and CIQ-whitened models refuse where ``sample_paths`` refuses: before any device work"""
    from dsvgp_amd._step64 import ElboEngine64
    from dsvgp_amd.gp_shim import ApproximateGP

    class Model:
        training = False
        variational_strategy = object()
        _param_dict = lambda self, _: {"inducing_points": torch.zeros(4, 3), "inducing_directions": torch.ones(8, 3),
                                       "variational_mean": torch.zeros(12), "chol_variational_covar": torch.eye(12)}
        sample_paths = ApproximateGP.sample_paths
        thompson_step = ApproximateGP.thompson_step

    cand, lo, hi = torch.zeros(5, 3), torch.zeros(3), torch.ones(3)
    m = Model()
    m.engine = ElboEngine64(torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="float64"):
        m.thompson_step(cand, lo, hi, 2)
    m.engine = dsvgp.ElboEngine(torch.device("cpu"))
    m.engine.whitening = "ciq"
    with pytest.raises(NotImplementedError, match="msMINRES"):
        m.thompson_step(cand, lo, hi, 2)


def test_own_point_methods_refuse_cpu_tensors_and_wrong_shapes(dsvgp):
    paths = dsvgp.SamplePaths(torch.device("cpu"), torch.zeros(8), 4, 3, 8, 2, torch.zeros(()))
    x = torch.zeros(2, 5, 3)
    for call in (lambda: paths.values_at(x), lambda: paths.values_and_gradients_at(x),
                 lambda: paths.descend(x, torch.zeros(3), torch.ones(3))):
        with pytest.raises(dsvgp._lib.DsvgpError):
            call()


# ------------------------------------------------------------------ the restatement
def test_own_reference_is_the_shared_reference_at_equal_points():
    d, M, p, B, F, n = 5, 19, 5, 7, 32, 3
    _, P64, x = own_problem(d, M, p, B)
    draws = make_draws(d, M * (p + 1), F, n)
    v, g = path_reference(P64, x, draws)
    vo, go = own_reference(P64, x[None].expand(n, B, d), draws)
    assert torch.equal(vo, v) and torch.equal(go, g)
    vc, gc = own_reference(P64, own_points(x, n), draws, closed_form)
    vr, gr = own_reference(P64, own_points(x, n), draws)
    assert relmax(vc, vr) <= 1e-11 and relmax(gc, gr) <= 1e-11


@pytest.mark.parametrize("d,M,p,B,F,n", DESCENT, ids=DESCENT_IDS)
def test_descend_reference_is_monotone_in_the_box_and_decisive(d, M, p, B, F, n):
    """The reference-only conditions the GPU test relies on, at its exact inputs (T = 4, initial_step = 0.25 ell): values never get
    worse; iterates stay in the box; T = 0 is the clamped start; EVERY pair ends strictly better than it started, by far more than
    the kernels' 2e-4 error; the share of decisions with |Armijo margin| <= 1e-3 max|f(x0)| -- those the GPU test cannot hold the
    kernel to, the margin being a difference of two values each good to 2e-4 -- is at most 10 %."""
    _, P64, x0, lower, upper, draws, step0 = descent_case(d, M, p, B, F, n)
    x_s, f_s, g_s, eta_s, acc_s = descend_reference(P64, x0, lower, upper, draws, 0, step0, False)
    assert torch.equal(x_s, torch.minimum(torch.maximum(x0, lower), upper)) and int(acc_s.sum()) == 0
    fr, gr = own_reference(P64, x_s, draws)
    assert relmax(f_s, fr) <= 1e-11 and relmax(g_s, gr) <= 1e-11
    assert torch.allclose(eta_s * g_s.norm(dim=-1), torch.full_like(eta_s, step0), rtol=1e-12)
    for maximize in (False, True):
        sg = -1.0 if maximize else 1.0
        trace = []
        x, f, g, eta, acc = descend_reference(P64, x0, lower, upper, draws, 4, step0, maximize, trace)
        prev = sg * f_s
        for margin, ft in trace:
            assert bool((sg * ft <= prev).all())
            prev = sg * ft
        assert bool((x >= lower).all()) and bool((x <= upper).all())
        assert bool(torch.isfinite(x).all() and torch.isfinite(f).all() and torch.isfinite(g).all() and torch.isfinite(eta).all())
        assert int(acc.max()) <= 4 and int(acc.min()) >= 0
        gain = (sg * f_s - sg * f)
        scale = f_s.abs().max().item()
        margins = torch.stack([m for m, _ in trace])
        share = (margins.abs() <= 1e-3 * scale).double().mean().item()
        print("[descent reference] d=%d %s: least gain %.3e on a scale of %.3e, accepted %d of %d, undecidable share %.3f"
              % (d, "max" if maximize else "min", gain.min().item(), scale, int(acc.sum()), 4 * acc.numel(), share))
        assert gain.min().item() > 50 * 2e-4 * scale, gain.min().item()
        assert share <= 0.10, share


def test_descend_reference_with_active_and_degenerate_boxes():
    d, M, p, B, F, n = DESCENT[1]
    _, P64, x0, _, _, draws, step0 = descent_case(d, M, p, B, F, n)
    base = own_problem(d, M, p, B)[2]
    lo, hi = base.min(dim=0).values + 0.3, base.max(dim=0).values - 0.3        # a box the starts stick out of: clamps are active
    trace = []
    x, f, g, eta, acc = descend_reference(P64, x0, lo, hi, draws, 4, step0, False, trace)
    assert bool((x >= lo).all()) and bool((x <= hi).all())
    assert bool(((x == lo) | (x == hi)).any())
    f0 = descend_reference(P64, x0, lo, hi, draws, 0, step0, False)[1]
    assert bool((f <= f0).all())
    # lower = upper: every trial is the point itself, accepted with a zero margin
    pt = x0[:, 0].mean(dim=0)
    x, f, g, eta, acc = descend_reference(P64, x0, pt, pt, draws, 3, step0, False)
    assert torch.equal(x, pt.expand_as(x)) and bool((acc == 3).all()) and bool(torch.isfinite(eta).all())
