"""CPU: the surface of the rectangular kernel backward (``dsvgp_kernel_bwd_rect``, csrc/assemble_wide.hip) and of the training step
built on it -- the exports, their declarations and bindings, the workspace arithmetic, the engines' refusals (raised on the shapes
alone, before any device work), the harness signatures and the model attribute.  Nothing here touches a GPU."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_declares_and_binds_the_backward_entries(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    for n, nargs in (("dsvgp_kernel_bwd_rect_workspace_bytes", 5), ("dsvgp_kernel_bwd_rect", 19)):
        assert hasattr(dsvgp._lib.lib, n), "missing export: " + n
        assert n in dsvgp._lib.SIGNATURES, "missing binding: " + n
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, hdr, flags=re.S)
        assert decl, "not declared in include/dsvgp.h: " + n
        assert len(decl.group(1).split(",")) == len(dsvgp._lib.SIGNATURES[n][1]) == nargs, n
    assert list(inspect.signature(dsvgp._ops.kernel_bwd_rect).parameters) == ["ctx", "G", "pack1", "n1", "p1", "pack2", "n2", "p2", "d", "hyp",
                                                                             "d_x1", "d_v1", "d_hyp", "workspace"]
    assert list(inspect.signature(dsvgp._ops.kernel_bwd_rect_workspace_bytes).parameters) == ["n1", "p1", "n2", "p2", "d"]


def test_workspace_bytes(dsvgp):
    ws = dsvgp._ops.kernel_bwd_rect_workspace_bytes
    for bad in ((0, 2, 10, 0, 3), (-1, 2, 10, 0, 3), (10, 2, 0, 0, 3), (10, 2, -5, 0, 3), (10, 2, 10, 0, 0), (10, 96, 10, 0, 3),
                (10, 2, 10, 96, 3), (10, -1, 10, 0, 3)):
        assert ws(*bad) == 0, bad
    for n1, p1, n2, p2, d in ((40, 2, 130, 0, 3), (100, 0, 50, 3, 5), (3, 95, 100, 0, 9), (30, 1, 5, 95, 9), (9, 3, 30, 0, 200),
                              (500, 5, 4096, 0, 20), (1, 0, 1, 0, 1)):
        n1q, n2q = n1 * (p1 + 1), n2 * (p2 + 1)
        NP = (dsvgp._ops.packed_width(d) + 15) // 16 * 16
        assert ws(n1, p1, n2, p2, d) >= 4 * (n1q * n2q + n1q * NP), (n1, p1, n2, p2, d)


def _params(M, d, p, dtype=torch.float32, shared=False):
    return {"inducing_points": torch.zeros(M, d, dtype=dtype), "inducing_directions": torch.ones(p if shared else M * p, d, dtype=dtype)}


class _World:
    rank, world = 0, 2


def test_engine_refusals_come_before_any_device_work(dsvgp):
    """on CPU tensors and a CPU device: whatever touched the device would raise something else"""
    from dsvgp_amd._step64 import ElboEngine64
    P, x = _params(4, 3, 2), torch.zeros(7, 3)
    y0, y3, D3 = torch.zeros(7), torch.zeros(7 * 4), torch.ones(21, 3)

    def engine(**kw):
        eng = dsvgp.ElboEngine(torch.device("cpu"))
        for k, v in kw.items():
            setattr(eng, k, v)
        return eng

    for y, D in ((y0, None), (y3, D3)):
        with pytest.raises(ValueError, match="CIQ"):
            engine(whitening="ciq").loss_and_grads(P, x, y, D, 100.0)
        with pytest.raises(ValueError, match="shared"):
            engine(shared_directions=True).loss_and_grads(_params(4, 3, 2, shared=True), x, y, D, 100.0)
        with pytest.raises(ValueError, match="world = 2"):
            engine(collective=_World()).loss_and_grads(P, x, y, D, 100.0)
        with pytest.raises(ValueError, match="capture_mode"):
            engine(capture_mode=True).loss_and_grads(P, x, y, D, 100.0)
        with pytest.raises(ValueError, match="float64"):
            ElboEngine64(torch.device("cpu")).loss_and_grads(_params(4, 3, 2, torch.float64), x.double(), y.double(),
                                                             None if D is None else D.double(), 100.0)
    # the target vector: B (pd + 1) entries, the existing text with that number
    with pytest.raises(ValueError, match=r"length B\*\(p\+1\)=7$"):
        engine().loss_and_grads(P, x, y3, None, 100.0)
    with pytest.raises(ValueError, match=r"length B\*\(p\+1\)=28$"):
        engine().loss_and_grads(P, x, y0, D3, 100.0)
    with pytest.raises(ValueError, match="at most 95"):
        engine().loss_and_grads(P, x, torch.zeros(7 * 97), torch.ones(7 * 96, 3), 100.0)
    with pytest.raises(ValueError, match="derivative directions"):
        engine().loss_and_grads(P, x, y0, torch.ones(15, 3), 100.0)
    # which step a call selects: the model's own count and the derivative-free engine are not the rectangular step
    eng = engine()
    assert eng._train_rect_pd(P, x, torch.ones(14, 3)) is None and eng._train_rect_pd(P, x, None) == 0 and eng._train_rect_pd(P, x, D3) == 3
    assert eng._train_pd is None
    assert engine(data_outputs="values")._train_rect_pd(P, x, None) is None


def test_harness_signatures_and_model_attribute(dsvgp):
    from dsvgp_amd import directional_vi
    from dsvgp_amd.gp_shim import ApproximateGP
    for fn in (dsvgp.train_gp, directional_vi.train_gp, directional_vi.setup_training):
        params = inspect.signature(fn).parameters
        assert params["data_directions"].default is None and params["data_directions"].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD
        if "args" in params:
            assert list(params)[-1] == "args" and list(params)[-2] == "data_directions"
    assert list(inspect.signature(dsvgp.train_gp).parameters)[-1] == "args"
    with pytest.raises(AssertionError):
        dsvgp.train_gp(None, num_directions=2, minibatch_dim=1, data_directions=0)      # reference directional_vi.py:130, keyword or not
    Z, V = torch.rand(6, 3), torch.eye(3)[:2].repeat(6, 1)
    assert dsvgp.GPModel(Z, V, 3).data_directions is None
    assert ApproximateGP(torch.nn.Identity()).data_directions is None
