"""CPU: the surface of the ARD entries (csrc/assemble_ard.hip) -- the exports, their declarations and bindings, the workspace
arithmetic, the wrappers' signatures and the kernel module's parameter shapes.  Nothing here touches a GPU."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = (("dsvgp_hyp_forward_ard", 7), ("dsvgp_hyp_backward_ard", 10), ("dsvgp_pack_points_ard", 11), ("dsvgp_kernel_diag_ard", 7),
           ("dsvgp_kernel_diag_ard_bwd", 11), ("dsvgp_kernel_bwd_ard_workspace_bytes", 5), ("dsvgp_kernel_bwd_ard_slabs", 5),
           ("dsvgp_kernel_bwd_ard", 22))


def test_library_exports_declares_and_binds_the_ard_entries(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    for n, nargs in ENTRIES:
        assert hasattr(dsvgp._lib.lib, n), "missing export: " + n
        assert n in dsvgp._lib.SIGNATURES, "missing binding: " + n
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, hdr, flags=re.S)
        assert decl, "not declared in include/dsvgp.h: " + n
        assert len(decl.group(1).split(",")) == len(dsvgp._lib.SIGNATURES[n][1]) == nargs, n
    ops = dsvgp._ops
    assert list(inspect.signature(ops.kernel_bwd_ard).parameters) == ["ctx", "G", "pack1", "n1", "p1", "pack2", "n2", "p2", "d", "ell", "hyp",
                                                                      "symmetric", "d_x1", "d_v1", "d_ell", "d_hyp", "workspace"]
    assert list(inspect.signature(ops.kernel_bwd_ard_workspace_bytes).parameters) == ["n1", "p1", "n2", "p2", "d"]
    assert list(inspect.signature(ops.pack_points_ard).parameters) == ["ctx", "x", "v", "p", "ell", "center"]
    assert list(inspect.signature(ops.kernel_diag_ard).parameters) == ["ctx", "pack", "n", "p", "d", "hyp"]
    assert list(inspect.signature(ops.hyp_forward_ard).parameters) == ["ctx", "raw_l", "raw_s", "raw_n"]
    src = open(os.path.join(ROOT, "gp-derivatives-variational-inference_amd", "build_ext.py")).read()
    assert '"assemble_ard.hip"' in src


def test_workspace_bytes_and_slab_count(dsvgp):
    ws, slabs, rect = dsvgp._ops.kernel_bwd_ard_workspace_bytes, dsvgp._ops.kernel_bwd_ard_slabs, dsvgp._ops.kernel_bwd_rect_workspace_bytes
    for bad in ((0, 2, 10, 0, 3), (-1, 2, 10, 0, 3), (10, 2, 0, 0, 3), (10, 2, -5, 0, 3), (10, 2, 10, 0, 0), (10, 96, 10, 0, 3),
                (10, 2, 10, 96, 3), (10, -1, 10, 0, 3)):
        assert ws(*bad) == 0 and slabs(*bad) == 0, bad
    for n1, p1, n2, p2, d in ((37, 2, 41, 3, 5), (20, 5, 45, 5, 20), (11, 2, 23, 1, 200), (9, 0, 30, 2, 7), (12, 3, 30, 0, 6),
                              (24, 2, 24, 2, 5), (500, 5, 4096, 0, 20), (1, 0, 1, 0, 1)):
        # the rectangular backward's workspace, then the column sums [n2 q2] and the per-point rows [(n1 + n2), d]
        assert ws(n1, p1, n2, p2, d) >= rect(n1, p1, n2, p2, d) + 4 * (n2 * (p2 + 1) + (n1 + n2) * d), (n1, p1, n2, p2, d)
        assert slabs(n1, p1, n2, p2, d) >= 1
    assert slabs(37, 2, 41, 3, 5) == 1 and slabs(37, 2, 130, 3, 5) > 1      # (the split shape of tests/test_gpu_ard.py)


def test_kernel_module_parameter_shapes_and_setter(dsvgp):
    from dsvgp_amd.RBFKernelDirectionalGrad import RBFKernelDirectionalGrad
    k0 = RBFKernelDirectionalGrad()
    assert k0.ard_num_dims is None and k0.raw_lengthscale.shape == (1, 1) and list(k0.state_dict()) == ["raw_lengthscale"]
    k = RBFKernelDirectionalGrad(ard_num_dims=4)
    assert k.raw_lengthscale.shape == (1, 4) and k.lengthscale.shape == (1, 4) and list(k.state_dict()) == ["raw_lengthscale"]
    k.lengthscale = 0.7
    assert torch.allclose(k.lengthscale, torch.full((1, 4), 0.7))
    k.lengthscale = torch.tensor([0.1, 0.2, 0.3, 0.4])
    assert torch.allclose(k.lengthscale, torch.tensor([[0.1, 0.2, 0.3, 0.4]]))
    with pytest.raises(RuntimeError):
        k.lengthscale = torch.tensor([0.1, 0.2, 0.3])
    k2 = RBFKernelDirectionalGrad(ard_num_dims=4)
    k2.load_state_dict(k.state_dict())
    assert torch.equal(k2.raw_lengthscale, k.raw_lengthscale)
    with pytest.raises(ValueError):
        RBFKernelDirectionalGrad(ard_num_dims=0)
    with pytest.raises(ValueError, match="ARD lengthscales"):       # float64 inputs: refused before any device work
        k.forward(torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.float64), v1=torch.ones(3, 4, dtype=torch.float64),
                  v2=torch.ones(3, 4, dtype=torch.float64))


class _World:
    rank, world = 0, 2


def test_engine_refusals_come_before_any_device_work(dsvgp):
    """on CPU tensors and a CPU device: whatever touched the device would raise something else"""
    from dsvgp_amd._step64 import ElboEngine64
    M, d, p, B = 4, 3, 2, 7
    P = {"inducing_points": torch.zeros(M, d), "inducing_directions": torch.ones(M * p, d), "raw_lengthscale": torch.zeros(1, d)}
    x, y, D = torch.zeros(B, d), torch.zeros(B * 3), torch.ones(B * 2, d)
    word = "ARD lengthscales"

    def engine(**kw):
        eng = dsvgp.ElboEngine(torch.device("cpu"))
        for k, v in kw.items():
            setattr(eng, k, v)
        return eng

    for kw in (dict(whitening="ciq"), dict(shared_directions=True), dict(data_outputs="values"), dict(collective=_World()),
               dict(capture_mode=True), dict(deterministic=True)):
        with pytest.raises(ValueError, match=word):
            engine(**kw).loss_and_grads(P, x, y, D, 100.0)
        if "deterministic" not in kw:
            for call in ("predict", "predict_joint"):
                with pytest.raises(ValueError, match=word):
                    getattr(engine(**kw), call)(P, x, D)
    with pytest.raises(ValueError, match=word):
        engine().loss_and_grads(P, x, y, D, 100.0, fast=True)
    with pytest.raises(ValueError, match=word):
        engine().loss_and_grads(dict(P, natural_vec=torch.zeros(M * 3), natural_mat=torch.zeros(M * 3, M * 3)), x, y, D, 100.0)
    P64 = {k: v.double() for k, v in P.items()}
    for eng in (engine(), ElboEngine64(torch.device("cpu"))):
        with pytest.raises(ValueError, match=word):
            eng.loss_and_grads(P64, x.double(), y.double(), D.double(), 100.0)
        with pytest.raises(ValueError, match=word):
            eng.predict(P64, x.double(), D.double())
    eng = engine()
    for call in (lambda: eng.mean_predictor(P), lambda: eng.predict_blocks(P, x, D), lambda: eng.sample_paths(P, 2), lambda: eng.prior_moments(P),
                 lambda: eng.whiten_legacy(P)):
        with pytest.raises(ValueError, match=word):
            call()
    with pytest.raises(ValueError, match="one entry per input dimension"):
        engine().predict(dict(P, raw_lengthscale=torch.zeros(1, 2)), x, D)
    with pytest.raises(ValueError, match=r"length B\*\(p\+1\)=21$"):
        engine().loss_and_grads(P, x, torch.zeros(22), D, 100.0)
    with pytest.raises(ValueError, match="derivative directions"):
        engine().loss_and_grads(P, x, y, torch.ones(15, d), 100.0)
    assert engine()._is_ard(P) and not engine()._is_ard(dict(P, raw_lengthscale=torch.zeros(1, 1))) and not engine()._is_ard({})


def test_harness_signatures(dsvgp):
    from dsvgp_amd import directional_vi
    params = inspect.signature(directional_vi.setup_training).parameters
    assert list(params)[-1] == "ard_num_dims" and params["ard_num_dims"].default is None
    params = inspect.signature(dsvgp.GPModel.__init__).parameters
    assert params["ard_num_dims"].default is None and list(params)[-2] == "ard_num_dims"          # (then **kwargs)
    assert "ard_num_dims" not in inspect.signature(dsvgp.train_gp).parameters                       # read from **args, like seed / max_steps
    Z, V = torch.rand(6, 3), torch.eye(3)[:2].repeat(6, 1)
    assert dsvgp.GPModel(Z, V, 3).covar_module.base_kernel.raw_lengthscale.shape == (1, 1)
    model = dsvgp.GPModel(Z, V, 3, ard_num_dims=3)
    assert model.covar_module.base_kernel.raw_lengthscale.shape == (1, 3)
    assert [k for k in model.state_dict() if "lengthscale" in k] == ["covar_module.base_kernel.raw_lengthscale"]
    with pytest.raises(ValueError, match="input dimension"):
        dsvgp.GPModel(Z, V, 3, ard_num_dims=2)
    for kw in (dict(use_ngd=True), dict(use_ciq=True), dict(dfree=True), dict(shared=True)):
        with pytest.raises(ValueError, match="ARD lengthscales"):
            directional_vi.setup_training(None, num_inducing=4, ard_num_dims=3, **kw)
    with pytest.raises(ValueError, match="ARD lengthscales"):
        directional_vi.setup_training(None, num_inducing=4, ard_num_dims=3, tensors=(torch.rand(8, 3).double(), torch.rand(8, 4).double()))
