"""CPU: the surface of the per-point predictive covariance blocks (``dsvgp_predictive_blocks``, csrc/predict_blocks.hip) and of what is
built on it -- the two exports, their declaration and binding, ``_ops.predictive_blocks``, ``ElboEngine.predict_blocks``,
``PredictiveDistribution.point_covariances``, ``ApproximateGP.posterior_gradient``, ``eval_gradients``, the float64 engine's refusal --
and the yardstick of tests/test_gpu_blocks.py against the oracle.  Nothing here touches a GPU."""
import inspect
import os
import re

import pytest
import torch

import dsvgp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_declares_and_binds_both_entries(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    # ctx, A, lda, W, ldw, Mp, B, pd, PX, d, hyp, with_noise, blocks, workspace, workspace_bytes | Mp, B, pd
    for n, nargs in (("dsvgp_predictive_blocks", 15), ("dsvgp_predictive_blocks_workspace_bytes", 3)):
        assert hasattr(dsvgp._lib.lib, n), "missing export: " + n
        assert n in dsvgp._lib.SIGNATURES, "missing binding: " + n
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, hdr, flags=re.S)
        assert decl, "not declared in include/dsvgp.h: " + n
        assert len(decl.group(1).split(",")) == len(dsvgp._lib.SIGNATURES[n][1]) == nargs
    import ctypes as C
    assert dsvgp._lib.SIGNATURES["dsvgp_predictive_blocks_workspace_bytes"][0] is C.c_size_t
    assert "predict_blocks.hip" in open(os.path.join(ROOT, "gp-derivatives-variational-inference_amd", "build_ext.py")).read()


def test_python_layers_carry_the_new_entry_points(dsvgp):
    from dsvgp_amd import directional_vi, shared_directional_vi
    from dsvgp_amd.gp_shim import ApproximateGP, PredictiveDistribution
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(dsvgp._ops.predictive_blocks) == ["ctx", "A", "W", "pd", "packX", "d", "hyp", "with_noise", "out"]
    assert inspect.signature(dsvgp._ops.predictive_blocks).parameters["out"].default is None
    assert sig(dsvgp.ElboEngine.predict_blocks) == ["self", "params", "x", "D", "cache"]
    assert inspect.signature(dsvgp.ElboEngine.predict_blocks).parameters["cache"].default is False
    assert isinstance(PredictiveDistribution.point_covariances, property)
    assert sig(ApproximateGP.posterior_gradient) == ["self", "x", "likelihood"]
    assert inspect.signature(ApproximateGP.posterior_gradient).parameters["likelihood"].default is None
    assert sig(directional_vi.eval_gradients) == ["test_dataset", "model", "likelihood", "minibatch_size"]
    assert dsvgp.eval_gradients is directional_vi.eval_gradients and shared_directional_vi.eval_gradients is directional_vi.eval_gradients
    from dsvgp_amd.gp_shim import PosteriorGradient
    assert PosteriorGradient._fields == ("value_mean", "value_variance", "gradient_mean", "gradient_covariance",
                                         "value_gradient_covariance")


def test_workspace_helper_is_a_pure_host_function(dsvgp):
    ws = dsvgp._lib.lib.dsvgp_predictive_blocks_workspace_bytes
    assert ws(3000, 4096, 20) > 0
    assert ws(3000, 4096, 20) % (4096 * 21 * 21 * 4) == 0              # whole [B, q, q] float slabs, one per row slice
    assert ws(3000, 4096, 96) == 0 and ws(3000, 4096, -1) == 0 and ws(0, 4096, 5) == 0 and ws(3000, 0, 5) == 0
    assert ws(1200, 9, 5) >= 2 * 9 * 36 * 4                            # one strip, 1200 rows: more than one slice
    assert ws(27, 5, 95) == 5 * 96 * 96 * 4


def test_fp64_engine_refuses_before_any_device_work(dsvgp):
    from dsvgp_amd._step64 import ElboEngine64
    eng = ElboEngine64(torch.device("cpu"))        # (construction allocates nothing)
    P = {"inducing_points": torch.zeros(4, 3, dtype=torch.float64), "inducing_directions": torch.ones(8, 3, dtype=torch.float64)}
    x = torch.zeros(7, 3, dtype=torch.float64)
    for D in (None, torch.ones(14, 3, dtype=torch.float64), torch.ones(21, 3, dtype=torch.float64)):
        with pytest.raises(NotImplementedError, match="float64"):
            eng.predict_blocks(P, x, D)
    # the refusals that existing tests pin are as they were
    with pytest.raises(ValueError, match="float64"):
        eng.predict(P, x, None)


def test_float32_engine_refuses_ciq_at_another_count_on_the_shapes_alone(dsvgp):
    eng = dsvgp.ElboEngine(torch.device("cpu"))
    eng.whitening = "ciq"
    P = {"inducing_points": torch.zeros(4, 3), "inducing_directions": torch.ones(8, 3)}
    with pytest.raises(ValueError, match="CIQ"):
        eng._rect_pd(P, torch.zeros(7, 3), torch.ones(21, 3))


def test_yardstick_blocks_are_the_oracles_diagonal_blocks():
    """the blocks the GPU tests compare with are the diagonal blocks of ``rect_predictive``'s Sigma; where the oracle defines the
    joint covariance (pd = p, and pd = 0 through the derivative-free variant) its diagonal blocks are the same numbers"""
    from test_gpu_blocks import diag_blocks
    from test_gpu_rect_predict import rect_predictive, relmax
    from test_gpu_step import make_problem
    P, x, _, D, _ = make_problem(600, 5, 40, 2, 128, seed=1)
    P64, x, D = {k: v.double() for k, v in P.items()}, x.double(), D.double()
    _, Sig2, _ = rect_predictive(P64, x, D, 2)
    _, Sig0, _ = rect_predictive(P64, x, D[:0], 0)
    _, Sig_j = O.predictive_joint(P64, x, D)
    _, Sig_v = O.predictive_joint(P64, x, D, data_outputs="values")
    b2, b0 = diag_blocks(Sig2, 128, 3), diag_blocks(Sig0, 128, 1)
    errs = {"pd=p": relmax(b2, diag_blocks(Sig_j, 128, 3)), "pd=0": relmax(b0, diag_blocks(Sig_v, 128, 1))}
    print("[parity] yardstick blocks vs oracle: %s" % errs)
    assert b2.shape == (128, 3, 3) and b0.shape == (128, 1, 1)
    assert torch.equal(b2[7], Sig2[21:24, 21:24]) and torch.equal(b0[:, 0, 0], Sig0.diagonal())
    assert max(errs.values()) <= 1e-12, errs
