"""CPU: the surface of the rectangular kernel assembly (``dsvgp_kernel_fwd_rect``, csrc/assemble_wide.hip) and of what is built on it
-- the export, its declaration and binding, ``ApproximateGP.posterior``, ``eval_values`` and the float64 engine's refusal.  Nothing here
touches a GPU."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_declares_and_binds_the_rectangular_entry(dsvgp):
    n = "dsvgp_kernel_fwd_rect"
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    assert hasattr(dsvgp._lib.lib, n), "missing export: " + n
    assert n in dsvgp._lib.SIGNATURES, "missing binding: " + n
    decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, hdr, flags=re.S)
    assert decl, "not declared in include/dsvgp.h: " + n
    # one argument per binding slot: ctx, P1, self1, n1, p1, P2, self2, n2, p2, d, hyp, out, ld
    assert len(decl.group(1).split(",")) == len(dsvgp._lib.SIGNATURES[n][1]) == 13
    assert list(inspect.signature(dsvgp._ops.kernel_fwd_rect).parameters) == ["ctx", "pack1", "n1", "p1", "pack2", "n2", "p2", "d", "hyp",
                                                                             "out"]


def test_model_and_harness_carry_the_new_entry_points(dsvgp):
    from dsvgp_amd import directional_vi, shared_directional_vi
    from dsvgp_amd.gp_shim import ApproximateGP
    assert list(inspect.signature(ApproximateGP.posterior).parameters) == ["self", "x", "derivative_directions", "likelihood"]
    assert list(inspect.signature(directional_vi.eval_values).parameters) == ["test_dataset", "model", "likelihood", "minibatch_size"]
    assert dsvgp.eval_values is directional_vi.eval_values and shared_directional_vi.eval_values is directional_vi.eval_values


def _params(M, d, p, dtype):
    return {"inducing_points": torch.zeros(M, d, dtype=dtype), "inducing_directions": torch.ones(M * p, d, dtype=dtype)}


def test_direction_counts_are_read_from_the_shapes(dsvgp):
    count = dsvgp.ElboEngine._direction_counts
    x = torch.zeros(7, 3)
    assert count(_params(4, 3, 2, torch.float32), x, None) == (2, 0)
    assert count(_params(4, 3, 2, torch.float32), x, torch.zeros(0, 3)) == (2, 0)
    assert count(_params(4, 3, 0, torch.float32), x, torch.zeros(21, 3)) == (0, 3)
    assert count({"inducing_points": torch.zeros(4, 3), "inducing_directions": torch.zeros(2, 3)}, x, torch.zeros(14, 3), True) == (2, 2)
    with pytest.raises(ValueError, match="derivative directions"):
        count(_params(4, 3, 2, torch.float32), x, torch.zeros(15, 3))
    with pytest.raises(ValueError, match="derivative directions"):
        count(_params(4, 3, 2, torch.float32), x, torch.zeros(14, 2))


def test_fp64_engine_refuses_a_direction_count_other_than_the_models(dsvgp):
    from dsvgp_amd._step64 import ElboEngine64
    eng = ElboEngine64(torch.device("cpu"))        # (construction allocates nothing; the refusal comes before any device work)
    P = _params(4, 3, 2, torch.float64)
    x = torch.zeros(7, 3, dtype=torch.float64)
    for D in (None, torch.ones(7 * 3, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="float64"):
            eng.predict(P, x, D)
        with pytest.raises(ValueError, match="float64"):
            eng.predict_joint(P, x, D)


def test_float32_engine_names_the_reason_of_its_refusals(dsvgp):
    P, x = _params(4, 3, 2, torch.float32), torch.zeros(7, 3)
    eng = dsvgp.ElboEngine(torch.device("cpu"))
    assert eng._rect_pd(P, x, torch.ones(14, 3)) is None and eng._rect_pd(P, x, None) == 0 and eng._rect_pd(P, x, torch.ones(21, 3)) == 3
    eng.data_outputs = "values"
    assert eng._rect_pd(P, x, None) == 0
    with pytest.raises(ValueError, match="derivative-free"):
        eng._rect_pd(P, x, torch.ones(21, 3))
    eng.data_outputs, eng.whitening = "all", "ciq"
    with pytest.raises(ValueError, match="CIQ"):
        eng._rect_pd(P, x, None)
    eng.whitening = "cholesky"
    with pytest.raises(ValueError, match="at most 95"):
        eng._rect_pd(P, x, torch.ones(7 * 96, 3))
