"""CPU: the mathematics and the surface of the Hessian-vector products of the paths and of the posterior mean (dsvgp_paths_hvp,
SamplePaths.hvp / hessians, MeanPredictor.hvp / hessian, ApproximateGP.posterior_mean_hvp / posterior_mean_hessian; csrc/paths.hip).

The yardstick ``hvp_reference`` is float64 autograd through ``closed_form`` of tests/test_paths_host.py (pinned there to
``path_reference`` at 1e-11): the returned gradient is contracted with v and differentiated with respect to x.  ``hvp_formula`` restates
the expression the kernels evaluate,
    grad^2 f_s(x) v = (s / ell^2) [ sum_i ((k_i beta_is (r_i.v) + k_i (G'_is.v)) r_i + k_i (r_i.v) G'_is)
                                    + sum_j wq_js (-4 pi^2 cos 2 pi theta_j)(Om_j.v) Om_j - (sum_i k_i beta_is) v ]
in float64.  tests/test_gpu_paths_hvp.py imports both."""
import inspect
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

import dsvgp_oracle as O
from test_paths_host import closed_form, make_draws, path_factor, path_nu, problem, relmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = torch.float64
TABLE = [(3, 12, 2, 20), (5, 40, 2, 32)]


# ------------------------------------------------------------------ the yardstick and the restated formula
def hvp_reference(P64, x, v, draws):
    """[n, B, d] float64: d/dx of (grad f_s(x) . v) by autograd through ``closed_form`` (every point depends on its own row of x alone)"""
    xr = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        _, grad = closed_form(P64, xr, draws)
        out = [torch.autograd.grad((grad[s] * v).sum(), xr, retain_graph=True)[0] for s in range(grad.shape[0])]
    return torch.stack(out)


def hvp_formula(P64, x, v, draws):
    """[n, B, d] float64: the expression above, term by term"""
    L, j, ell, s, c, M, d, p = path_factor(P64)
    Z, V = P64["inducing_points"], P64["inducing_directions"]
    F = draws["omega"].shape[0]
    nu = path_nu(P64, draws).view(-1, M, p + 1)
    a = nu[:, :, 0]                                                                          # [n, M]
    Vn = O.normalize_rows(V).view(M, p, d) if p else torch.zeros(M, 0, d, dtype=f64)
    Gp = torch.einsum("sia,iak->sik", nu[:, :, 1:], Vn) / ell                                # G' [n, M, d]
    r = (Z[None] - x[:, None]) / ell                                                         # [B, M, d]
    k = torch.exp(-0.5 * (r * r).sum(-1))                                                    # [B, M]
    beta = a[:, None] - torch.einsum("bik,sik->sbi", r, Gp)                                  # [n, B, M]
    rv = torch.einsum("bik,bk->bi", r, v)                                                    # r_i . v
    gv = torch.einsum("sik,bk->sbi", Gp, v)                                                  # G'_is . v
    Om = draws["omega"] / (2 * math.pi)
    theta = x @ Om.t() / ell + draws["phase"] / (2 * math.pi)                                # revolutions
    wq = torch.sqrt(2 / (s * F)) * draws["w"]                                                # [n, F]
    T = -4 * math.pi ** 2 * torch.cos(2 * math.pi * theta) * (v @ Om.t())                    # [B, F]
    acc = (torch.einsum("sbi,bik->sbk", k * beta * rv + k * gv, r) + torch.einsum("bi,sik->sbk", k * rv, Gp)
           + torch.einsum("sj,bj,jk->sbk", wq, T, Om))
    sigma = (k * beta).sum(-1)                                                               # [n, B]
    return (s / ell ** 2) * (acc - sigma[..., None] * v[None])


def unit_hessians(fn, B, d):
    """[.., B, d, d] with column k = fn(e_k tiled over the points)"""
    cols = [fn(torch.eye(d, dtype=f64)[k].repeat(B, 1)) for k in range(d)]
    return torch.stack(cols, dim=-1)


def _v(B, d, seed=11):
    return torch.randn(B, d, generator=torch.Generator().manual_seed(seed), dtype=f64)


# ------------------------------------------------------------------ (a) the formula
@pytest.mark.parametrize("d,M,p,B", TABLE)
def test_formula_equals_the_autograd_yardstick(d, M, p, B):
    _, P64, x = problem(d, M, p, B)
    draws = make_draws(d, M * (p + 1), 256, 3)
    v = _v(B, d)
    ref, got = hvp_reference(P64, x, v, draws), hvp_formula(P64, x, v, draws)
    err = relmax(got, ref)
    print("[paths hvp] formula vs autograd d=%d M=%d: %.2e, max|Hv| %.3g" % (d, M, err, ref.abs().max().item()))
    assert ref.shape == (3, B, d) and ref.abs().max() > 0.05
    assert err <= 1e-11, err


@pytest.mark.parametrize("d,M,p,B", TABLE)
def test_hessian_from_unit_vectors_is_symmetric(d, M, p, B):
    _, P64, x = problem(d, M, p, B)
    draws = make_draws(d, M * (p + 1), 256, 3)
    H = unit_hessians(lambda e: hvp_formula(P64, x, e, draws), B, d)
    err = relmax(H, H.transpose(-1, -2))
    print("[paths hvp] asymmetry of the assembled Hessian d=%d M=%d: %.2e" % (d, M, err))
    assert H.shape == (3, B, d, d)
    assert err <= 1e-12, err


@pytest.mark.parametrize("d,M,p,B", TABLE)
def test_zero_draws_give_the_hessian_of_the_predictive_mean(d, M, p, B):
    _, P64, x = problem(d, M, p, B)
    draws = make_draws(d, M * (p + 1), 64, 2, zero=True)
    H = unit_hessians(lambda e: hvp_formula(P64, x, e, draws), B, d)
    xr = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        mu, _ = O.predictive(P64, xr, torch.eye(d, dtype=f64)[:p].repeat(B, 1), data_outputs="values")      # pd = 0
        g, = torch.autograd.grad(mu.sum(), xr, create_graph=True)
        ref = torch.stack([torch.autograd.grad(g[:, k].sum(), xr, retain_graph=True)[0] for k in range(d)], dim=-1)
    errs = dict(sample0=relmax(H[0], ref), sample1=relmax(H[1], ref))
    print("[paths hvp] zero draws vs Hessian of O.predictive's mean d=%d M=%d: %s" % (d, M, errs))
    assert ref.abs().max() > 0.05
    assert max(errs.values()) <= 1e-11, errs


# ------------------------------------------------------------------ (b) the surface
NEW = {"dsvgp_paths_hvp_workspace_bytes": 5, "dsvgp_paths_hvp": 11}


def test_library_exports_declares_and_binds_the_new_entries(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n, nargs in NEW.items():
        assert hasattr(dsvgp._lib.lib, n), "missing export: " + n
        assert n in dsvgp._lib.SIGNATURES, "missing binding: " + n
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, hdr, flags=re.S)
        assert decl, "not declared in include/dsvgp.h: " + n
        assert len(decl.group(1).split(",")) == len(dsvgp._lib.SIGNATURES[n][1]) == nargs, n
    assert callable(dsvgp._ops.paths_hvp) and callable(dsvgp._ops.paths_hvp_workspace_bytes)


def test_workspace_helper_is_a_host_function_and_refuses_with_zero(dsvgp):
    ws = dsvgp._ops.paths_hvp_workspace_bytes
    for bad in ((0, 40, 64, 1, 8), (12, 0, 64, 1, 8), (12, 40, 0, 1, 8), (12, 40, 64, 0, 8), (12, 40, 64, 1, 0), (-1, 40, 64, 1, 8)):
        assert ws(*bad) == 0, bad
    assert ws(12, 3, 64, 2, 100) == 0 and ws(12, 32, 64, 2, 100) == 0                # fused route: registers and LDS only
    assert 0 < ws(12, 33, 64, 2, 100) < ws(12, 33, 64, 2, 200) < ws(24, 33, 64, 2, 200) < ws(24, 33, 128, 2, 200)
    assert ws(12, 33, 64, 2, 100) % 16 == 0
    assert ws(500, 200, 2048, 1, 2000000) == 0                                       # B x F passes 2^31 entries: refused
    # nothing of size B x B: linear in B at the rover-like shape, and the group part under 512 MiB
    one, two = ws(512, 200, 2048, 8, 2500), ws(512, 200, 2048, 8, 5000)
    assert two < 2 * one + 4096 and two < (1 << 30)


def test_host_check_of_the_plan_builds_and_passes(tmp_path):
    """tools/paths_hvp_check.cpp on csrc/paths_plan.h: the sample-group table and the LDS plan stay within 64 KiB for every D, every
    (sample, point, i) and (sample, point, j) is visited once, every offset is in bounds"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tools/paths_hvp_check.cpp")
    exe = str(tmp_path / "paths_hvp_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "gp-derivatives-variational-inference_amd", "csrc"),
                           os.path.join(ROOT, "tools", "paths_hvp_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    plan = re.findall(r"plan D +(\d+): NS (\d+), LDS +(\d+) bytes", out.stdout)
    assert [int(D) for D, _, _ in plan] == list(range(4, 33, 4))
    assert all(1 <= int(ns) <= 8 and int(lds) <= 65536 for _, ns, lds in plan), plan
    assert "every (sample, point, i) and (sample, point, j) visited exactly once, every offset in bounds" in out.stdout
    assert "FAILED" not in out.stdout


def test_model_and_predictors_carry_the_new_methods(dsvgp):
    from dsvgp_amd.gp_shim import ApproximateGP
    params = lambda f: list(inspect.signature(f).parameters)
    assert params(dsvgp.SamplePaths.hvp) == ["self", "x", "v"] and params(dsvgp.SamplePaths.hessians) == ["self", "x"]
    assert params(dsvgp.MeanPredictor.hvp) == ["self", "x", "v"] and params(dsvgp.MeanPredictor.hessian) == ["self", "x"]
    assert params(ApproximateGP.posterior_mean_hvp) == ["self", "x", "v"]
    assert params(ApproximateGP.posterior_mean_hessian) == ["self", "x"]
    assert params(dsvgp._ops.paths_hvp) == ["ctx", "weights", "M", "d", "F", "n", "x", "v", "hv", "workspace"]
    assert params(dsvgp._ops.paths_hvp_workspace_bytes) == ["M", "d", "F", "n", "B"]


def test_cpu_tensors_and_wrong_shapes_are_refused_before_any_device_work(dsvgp):
    paths = dsvgp.SamplePaths(torch.device("cpu"), torch.zeros(8), 4, 3, 2, 2, torch.zeros(()))
    x = torch.zeros(5, 3)
    with pytest.raises(dsvgp._lib.DsvgpError):
        paths.hvp(x, torch.zeros(5, 3))
    with pytest.raises(dsvgp._lib.DsvgpError):
        paths.hessians(x)
