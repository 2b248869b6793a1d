"""CPU: the surface of the per-point covariance roots (csrc/block_roots.hip) -- the three exports, their declarations and bindings, the
argument checks of ``_ops.blocks_factor`` / ``blocks_draw`` / ``blocks_logpdf`` (which raise before any device work), the Python layers
on top -- the yardstick of tests/test_gpu_block_roots.py against closed forms and against itself, and the host check of the kernels'
index arithmetic (tools/block_roots_check.cpp).  Nothing here touches a GPU."""
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

from test_gpu_block_roots import (BS, QS, U, bound_reconstruction, closed_form_1d, synthetic, synthetic_yardstick, yardstick,
                                  yardstick_density)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = torch.float32, torch.float64


def test_library_exports_declares_and_binds_the_three_entries(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    # ctx, blocks, B, q, jitter, roots, logdet, info, status | ctx, roots, mu, eps, B, q, n, out | ctx, roots, logdet, mu, y, B, q, z, logp
    for n, nargs in (("dsvgp_blocks_factor", 9), ("dsvgp_blocks_draw", 8), ("dsvgp_blocks_logpdf", 9)):
        assert hasattr(dsvgp._lib.lib, n), "missing export: " + n
        assert n in dsvgp._lib.SIGNATURES, "missing binding: " + n
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, hdr, flags=re.S)
        assert decl, "not declared in include/dsvgp.h: " + n
        assert len(decl.group(1).split(",")) == len(dsvgp._lib.SIGNATURES[n][1]) == nargs
    import ctypes as C
    assert dsvgp._lib.SIGNATURES["dsvgp_blocks_factor"][1][4] is C.c_double            # the jitter
    assert "block_roots.hip" in open(os.path.join(ROOT, "gp-derivatives-variational-inference_amd", "build_ext.py")).read()


def test_python_layers_carry_the_new_entry_points(dsvgp):
    from dsvgp_amd import directional_vi, shared_directional_vi
    from dsvgp_amd._step64 import ElboEngine64
    from dsvgp_amd.gp_shim import ApproximateGP, PredictiveDistribution
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(dsvgp._ops.blocks_factor) == ["ctx", "blocks", "jitter"]
    assert sig(dsvgp._ops.blocks_draw) == ["ctx", "roots", "mu", "eps"]
    assert sig(dsvgp._ops.blocks_logpdf) == ["ctx", "roots", "logdet", "mu", "y", "want_z"]
    assert sig(dsvgp.ElboEngine.block_roots) == ["self", "blocks"]
    assert sig(dsvgp.ElboEngine.block_draw) == ["self", "mu", "roots", "eps"]
    assert sig(dsvgp.ElboEngine.block_log_prob) == ["self", "mu", "roots", "logdet", "y"]
    assert isinstance(PredictiveDistribution.point_roots, property)
    for name in ("rsample_points", "sample_points"):
        assert sig(getattr(PredictiveDistribution, name)) == ["self", "sample_shape", "base_samples"]
        assert inspect.signature(getattr(PredictiveDistribution, name)).parameters["sample_shape"].default == torch.Size()
        assert "independent between points" in getattr(PredictiveDistribution, name).__doc__.lower()
        assert "``sample``" in getattr(PredictiveDistribution, name).__doc__
    assert sig(PredictiveDistribution.point_log_prob) == sig(PredictiveDistribution.point_whitened_residuals) == ["self", "y"]
    assert sig(ApproximateGP.sample_gradients) == ["self", "x", "num_samples", "likelihood", "base_samples"]
    assert sig(ApproximateGP.gradient_log_prob) == ["self", "x", "y", "likelihood"]
    assert sig(ApproximateGP.posterior_gradient) == ["self", "x", "likelihood"]           # (as it was)
    assert sig(directional_vi.eval_gradient_nll) == ["test_dataset", "model", "likelihood", "minibatch_size"]
    assert inspect.signature(directional_vi.eval_gradient_nll).parameters["minibatch_size"].default == 1
    assert dsvgp.eval_gradient_nll is directional_vi.eval_gradient_nll is shared_directional_vi.eval_gradient_nll
    assert directional_vi.GradientNLL._fields == ("nll", "whitened", "value_nll")
    # the float64 engine keeps refusing the blocks themselves
    with pytest.raises(NotImplementedError, match="float64"):
        ElboEngine64(torch.device("cpu")).predict_blocks({}, torch.zeros(2, 3, dtype=f64), None)


def test_ops_refuse_bad_arguments_before_any_device_work(dsvgp):
    ops = dsvgp._ops
    B, q = 4, 3
    blocks = torch.eye(q).repeat(B, 1, 1)
    roots, logdet = blocks.double(), torch.zeros(B, dtype=f64)
    mu, y, eps = torch.zeros(B * q), torch.zeros(B * q), torch.zeros(2, B * q)
    # wrong dtype
    with pytest.raises(TypeError):
        ops.blocks_factor(None, blocks.double())
    with pytest.raises(TypeError):
        ops.blocks_draw(None, roots.float(), mu, eps)
    with pytest.raises(TypeError):
        ops.blocks_draw(None, roots, mu.double(), eps)
    with pytest.raises(TypeError):
        ops.blocks_logpdf(None, roots, logdet.float(), mu, y)
    with pytest.raises(TypeError):
        ops.blocks_logpdf(None, roots, logdet, mu, y.double())
    # not contiguous
    with pytest.raises(ValueError, match="contiguous"):
        ops.blocks_factor(None, torch.eye(q).repeat(B, 1, 2)[:, :, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        ops.blocks_draw(None, roots, mu, torch.zeros(B * q, 2).t())
    with pytest.raises(ValueError, match="contiguous"):
        ops.blocks_logpdf(None, roots, logdet, torch.zeros(2 * B * q)[::2], y)
    # q = 97: the existing message
    for call in (lambda: ops.blocks_factor(None, torch.zeros(2, 97, 97)),
                 lambda: ops.blocks_draw(None, torch.zeros(2, 97, 97, dtype=f64), torch.zeros(194), torch.zeros(1, 194)),
                 lambda: ops.blocks_logpdf(None, torch.zeros(2, 97, 97, dtype=f64), torch.zeros(2, dtype=f64), torch.zeros(194), torch.zeros(194))):
        with pytest.raises(ValueError, match="at most 95 derivative directions per data point"):
            call()
    # shapes
    with pytest.raises(ValueError, match="B, q, q"):
        ops.blocks_factor(None, torch.zeros(4, 3, 2))
    with pytest.raises(ValueError, match="y has 11 entries"):
        ops.blocks_logpdf(None, roots, logdet, mu, torch.zeros(B * q - 1))
    with pytest.raises(ValueError, match="mu has"):
        ops.blocks_draw(None, roots, torch.zeros(B * q + 1), eps)
    with pytest.raises(ValueError, match="eps has"):
        ops.blocks_draw(None, roots, mu, torch.zeros(2, B * q + 3))
    with pytest.raises(ValueError, match="logdet"):
        ops.blocks_logpdf(None, roots, torch.zeros(B + 1, dtype=f64), mu, y)
    # well-formed arguments on the CPU: no fallback
    for call in (lambda: ops.blocks_factor(None, blocks), lambda: ops.blocks_draw(None, roots, mu, eps),
                 lambda: ops.blocks_logpdf(None, roots, logdet, mu, y)):
        with pytest.raises(dsvgp._lib.DsvgpError, match="no CPU fallback"):
            call()
    # the engine: float32 blocks only
    eng = dsvgp.ElboEngine(torch.device("cpu"))
    with pytest.raises(TypeError, match="float32"):
        eng.block_roots(blocks.double())


def test_yardstick_density_at_q1_is_the_closed_form():
    g = torch.Generator().manual_seed(2)
    v = torch.rand(50, 1, 1, generator=g) + 0.1
    mu, y = torch.randn(50, generator=g), torch.randn(50, generator=g)
    _, L, logdet, kappa = yardstick(v)
    z, logp = yardstick_density(L, mu, y)
    cf = closed_form_1d(mu, v, y)
    assert torch.equal(kappa, torch.ones(50, dtype=f64))
    assert float((logp - cf).abs().max()) <= 8 * U * float(cf.abs().max().clamp_min(1.0))
    assert float((z[:, 0] - (y.double() - mu.double()) / v.double().reshape(-1).sqrt()).abs().max()) <= 4 * U * float(z.abs().max())
    assert float((logdet - v.double().reshape(-1).log()).abs().max()) <= 8 * U * float(logdet.abs().max().clamp_min(1.0))


@pytest.mark.parametrize("q", QS)
def test_synthetic_blocks_keep_the_bounds_meaningful_on_the_yardstick_alone(q):
    """the condition number stays below 1e3; the yardstick's own factor keeps bound 1; its z agrees with an LU solve within bound 4;
    its log-determinant agrees with a second evaluation (the sum of the logs of the eigenvalues) within bound 2 in every block where
    that bound is above what rounding alone moves: a root stored in double carries a relative u on every diagonal entry and every
    logarithm is rounded, so an evaluation of 2 sum log L_ii is uncertain by floor = 2 u (q + sum |log L_ii|) to first order, and two
    evaluations may differ by twice that.  Bound 2, q^2 u kappa, is below 2 floor at q = 1 always (kappa = 1: the bound is
    u = 1.1e-16, less than one rounding of the root) and in some well-conditioned blocks at q = 2 and 3; the count is printed."""
    for B in BS:
        blocks, mu, y = synthetic(B, q)
        A, L, logdet, kappa, z, logp = synthetic_yardstick(B, q)
        assert blocks.dtype == f32 and torch.equal(blocks, blocks.transpose(1, 2))
        assert float(kappa.max()) <= 1e3
        rec = ((L @ L.transpose(1, 2) - A).abs() / bound_reconstruction(L, q)).max().item()
        assert rec <= 1.0
        second = torch.linalg.eigvalsh(A).log().sum(-1)
        bound2 = q * q * U * kappa
        floor = 2.0 * U * (q + L.diagonal(dim1=1, dim2=2).log().abs().sum(-1))
        above = bound2 >= 2.0 * floor
        r2 = ((logdet - second).abs() / bound2)
        print("[parity] yardstick q %d B %d: kappa <= %.1f, reconstruction / bound %.2e, logdet vs eigenvalues / bound %.2e, "
              "bound 2 above twice the rounding floor in %d of %d blocks" % (q, B, float(kappa.max()), rec, float(r2.max()), int(above.sum()), B))
        assert bool((r2[above] <= 1.0).all())
        z2 = torch.linalg.solve(L, (y.double() - mu.double()).reshape(B, q, 1)).squeeze(-1)
        zb = 2.0 ** -23 * z.abs() + (q * 2.0 ** -52 * kappa * z.abs().max(-1).values).unsqueeze(-1)
        assert float(((z - z2).abs() / zb).max()) <= 1.0
        assert bool(torch.isfinite(logp).all())


def test_host_check_of_the_index_arithmetic_builds_and_passes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tools/block_roots_check.cpp")
    exe = str(tmp_path / "block_roots_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "gp-derivatives-variational-inference_amd", "csrc"),
                           os.path.join(ROOT, "tools", "block_roots_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "every element, row and draw item owned exactly once, every offset in bounds" in out.stdout and "FAILED" not in out.stdout
