"""CPU: the surface of the Matern-5/2 entries (csrc/assemble_matern.hip) -- the exports, their declarations and bindings, the workspace
and LDS arithmetic, the wrappers' and the harness' signatures, the kernel module's parameters and every refusal.  Nothing here touches a GPU."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = (("dsvgp_kernel_fwd_matern52", 15), ("dsvgp_kernel_fwd_matern52_lds_bytes", 2), ("dsvgp_kernel_bwd_matern52_workspace_bytes", 5),
           ("dsvgp_kernel_bwd_matern52", 22), ("dsvgp_kernel_diag_matern52", 7), ("dsvgp_kernel_diag_matern52_bwd", 11))
WORD = "Matern"


def test_library_exports_declares_and_binds_the_matern_entries(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    for n, nargs in ENTRIES:
        assert hasattr(dsvgp._lib.lib, n), "missing export: " + n
        assert n in dsvgp._lib.SIGNATURES, "missing binding: " + n
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, hdr, flags=re.S)
        assert decl, "not declared in include/dsvgp.h: " + n
        assert len(decl.group(1).split(",")) == len(dsvgp._lib.SIGNATURES[n][1]) == nargs, n
    sig = dsvgp._lib.SIGNATURES
    assert sig["dsvgp_kernel_bwd_matern52"] == sig["dsvgp_kernel_bwd_ard"]                 # the ARD backward's argument list
    assert sig["dsvgp_kernel_diag_matern52"] == sig["dsvgp_kernel_diag_ard"]
    assert sig["dsvgp_kernel_diag_matern52_bwd"] == sig["dsvgp_kernel_diag_ard_bwd"]
    ops = dsvgp._ops
    assert list(inspect.signature(ops.kernel_bwd_matern52).parameters) == list(inspect.signature(ops.kernel_bwd_ard).parameters)
    assert list(inspect.signature(ops.kernel_bwd_matern52_workspace_bytes).parameters) == ["n1", "p1", "n2", "p2", "d"]
    assert list(inspect.signature(ops.kernel_fwd_matern52).parameters) == ["ctx", "pack1", "n1", "p1", "pack2", "n2", "p2", "d", "hyp",
                                                                         "jitter", "out", "dtype"]
    assert list(inspect.signature(ops.kernel_diag_matern52).parameters) == list(inspect.signature(ops.kernel_diag_ard).parameters)
    assert list(inspect.signature(ops.kernel_diag_matern52_bwd).parameters) == list(inspect.signature(ops.kernel_diag_ard_bwd).parameters)
    src = open(os.path.join(ROOT, "gp-derivatives-variational-inference_amd", "build_ext.py")).read()
    assert '"assemble_matern.hip"' in src
    # existing entries keep their argument counts
    assert len(sig["dsvgp_kernel_bwd_ard"][1]) == 22 and len(sig["dsvgp_kernel_fwd_rect"][1]) == 13 and len(sig["dsvgp_kernel_bwd_rect"][1]) == 19


def test_workspace_bytes_are_the_ard_backwards_rounded_to_16(dsvgp):
    """pure host arithmetic: 0 for refused shapes, a multiple of 16, and the ARD helper's value (the launches after the Tbar tiles and the
    workspace layout are the ARD backward's) -- which is a multiple of 4 only -- rounded up to the next multiple of 16"""
    ws, ard = dsvgp._ops.kernel_bwd_matern52_workspace_bytes, dsvgp._ops.kernel_bwd_ard_workspace_bytes
    for bad in ((0, 2, 10, 0, 3), (-1, 2, 10, 0, 3), (10, 2, 0, 0, 3), (10, 2, -5, 0, 3), (10, 2, 10, 0, 0), (10, 96, 10, 0, 3),
                (10, 2, 10, 96, 3), (10, -1, 10, 0, 3)):
        assert ws(*bad) == 0, bad
    for shape in ((37, 2, 41, 3, 5), (20, 5, 45, 5, 20), (11, 2, 23, 1, 200), (9, 0, 30, 2, 7), (12, 3, 30, 0, 6), (24, 2, 24, 2, 5),
                  (500, 5, 4096, 0, 20), (1, 0, 1, 0, 1)):
        assert ws(*shape) % 16 == 0 and 0 < ard(*shape) <= ws(*shape) < ard(*shape) + 16, shape


def test_forward_lds_stays_inside_a_workgroup_for_every_direction_count(dsvgp):
    """the forward keeps three pair values per point pair: its dynamic LDS over all q1, q2 <= 96, in a host computation.  The Tbar launch
    adds no array to the RBF launch's (at most 117372 bytes, csrc/assemble_wide.hip).  The worst case is pinned: 47424 bytes at 2 x 1, the
    RBF forward's bytes there plus two more pair arrays of Rr x Rc = 24 x 96 floats."""
    lds = dsvgp._lib.lib.dsvgp_kernel_fwd_matern52_lds_bytes
    worst = max((int(lds(p1, p2)), p1 + 1, p2 + 1) for p1 in range(96) for p2 in range(96))
    print("[parity] Matern forward LDS: at most %d bytes, at q1 x q2 = %d x %d" % worst)
    assert worst == (47424, 2, 1)
    assert lds(96, 0) == 0 and lds(0, 96) == 0 and lds(-1, 0) == 0


def test_kernel_module_parameter_shapes_and_setter(dsvgp):
    from dsvgp_amd.Matern52KernelDirectionalGrad import Matern52KernelDirectionalGrad
    from dsvgp_amd.RBFKernelDirectionalGrad import RBFKernelDirectionalGrad
    assert dsvgp.Matern52KernelDirectionalGrad is Matern52KernelDirectionalGrad
    k0 = Matern52KernelDirectionalGrad()
    assert k0.ard_num_dims is None and k0.raw_lengthscale.shape == (1, 1) and list(k0.state_dict()) == ["raw_lengthscale"]
    k = Matern52KernelDirectionalGrad(ard_num_dims=4)
    assert k.raw_lengthscale.shape == (1, 4) and k.lengthscale.shape == (1, 4) and list(k.state_dict()) == list(RBFKernelDirectionalGrad(4).state_dict())
    k.lengthscale = 0.7
    assert torch.allclose(k.lengthscale, torch.full((1, 4), 0.7))
    k.lengthscale = torch.tensor([0.1, 0.2, 0.3, 0.4])
    assert torch.allclose(k.lengthscale, torch.tensor([[0.1, 0.2, 0.3, 0.4]]))
    assert torch.allclose(k.lengthscale, torch.nn.functional.softplus(k.raw_lengthscale))
    with pytest.raises(RuntimeError):
        k.lengthscale = torch.tensor([0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        Matern52KernelDirectionalGrad(ard_num_dims=0)
    assert list(inspect.signature(k.forward).parameters) == list(inspect.signature(RBFKernelDirectionalGrad().forward).parameters)
    z64 = torch.zeros(3, 4, dtype=torch.float64)
    for kern in (k, k0):
        with pytest.raises(ValueError, match=WORD):                     # float64 inputs: refused before any device work
            kern.forward(z64, z64, v1=torch.ones(3, 4, dtype=torch.float64), v2=torch.ones(3, 4, dtype=torch.float64))
    k.set_num_directions(3)
    assert k.num_outputs_per_input(None, None) == 4


class _World:
    rank, world = 0, 2


def test_engine_refusals_come_before_any_device_work(dsvgp):
    """on CPU tensors and a CPU device: whatever touched the device would raise something else"""
    from dsvgp_amd._step64 import ElboEngine64
    M, d, p, B = 4, 3, 2, 7
    x, y, D = torch.zeros(B, d), torch.zeros(B * 3), torch.ones(B * 2, d)
    for rl in (torch.zeros(1, d), torch.zeros(1, 1)):                   # Matern-ARD and the scalar lengthscale
        P = {"inducing_points": torch.zeros(M, d), "inducing_directions": torch.ones(M * p, d), "raw_lengthscale": rl}

        def engine(cls=dsvgp.ElboEngine, **kw):
            eng = cls(torch.device("cpu"))
            eng.kernel = "matern52"
            for k, v in kw.items():
                setattr(eng, k, v)
            return eng

        for kw in (dict(whitening="ciq"), dict(shared_directions=True), dict(data_outputs="values"), dict(collective=_World()),
                   dict(capture_mode=True), dict(deterministic=True)):
            with pytest.raises(ValueError, match=WORD):
                engine(**kw).loss_and_grads(P, x, y, D, 100.0)
            if "deterministic" not in kw:
                for call in ("predict", "predict_joint"):
                    with pytest.raises(ValueError, match=WORD):
                        getattr(engine(**kw), call)(P, x, D)
        with pytest.raises(ValueError, match=WORD):
            engine().loss_and_grads(P, x, y, D, 100.0, fast=True)
        Pn = dict(P, natural_vec=torch.zeros(M * 3), natural_mat=torch.zeros(M * 3, M * 3))
        for call in (lambda: engine().loss_and_grads(Pn, x, y, D, 100.0), lambda: engine().predict(Pn, x, D)):
            with pytest.raises(ValueError, match=WORD):
                call()
        P64 = {k: v.double() for k, v in P.items()}
        for eng in (engine(), engine(ElboEngine64)):
            with pytest.raises(ValueError, match=WORD):
                eng.loss_and_grads(P64, x.double(), y.double(), D.double(), 100.0)
            with pytest.raises(ValueError, match=WORD):
                eng.predict(P64, x.double(), D.double())
        eng = engine()
        for call in (lambda: eng.mean_predictor(P), lambda: eng.predict_blocks(P, x, D), lambda: eng.sample_paths(P, 2),
                     lambda: eng.prior_moments(P), lambda: eng.whiten_legacy(P), lambda: eng.value_variances(P)):
            with pytest.raises(ValueError, match=WORD):
                call()
        with pytest.raises(ValueError, match=r"length B\*\(p\+1\)=21$"):
            engine().loss_and_grads(P, x, torch.zeros(22), D, 100.0)
        with pytest.raises(ValueError, match="derivative directions"):
            engine().loss_and_grads(P, x, y, torch.ones(15, d), 100.0)
    with pytest.raises(ValueError, match="1 entry or one per input dimension"):
        engine().predict(dict(P, raw_lengthscale=torch.zeros(1, 2)), x, D)
    eng = dsvgp.ElboEngine(torch.device("cpu"))
    assert eng.kernel == "rbf"
    eng.kernel = "matern32"
    with pytest.raises(ValueError, match="'rbf' or 'matern52'"):
        eng.predict(P, x, D)
    # with kernel == "rbf" the ARD messages stay as they are
    P = dict(P, raw_lengthscale=torch.zeros(1, d))
    with pytest.raises(ValueError, match="ARD lengthscales"):
        dsvgp.ElboEngine(torch.device("cpu")).loss_and_grads(P, x, y, D, 100.0, fast=True)


def test_harness_signatures_and_state_dict_keys(dsvgp):
    from dsvgp_amd import directional_vi
    from dsvgp_amd.Matern52KernelDirectionalGrad import Matern52KernelDirectionalGrad
    params = inspect.signature(directional_vi.setup_training).parameters
    assert list(params)[-1] == "ard_num_dims" and params["ard_num_dims"].default is None
    assert list(params)[-2] == "kernel" and params["kernel"].default == "rbf"
    params = inspect.signature(dsvgp.GPModel.__init__).parameters
    assert list(params) == ["self", "inducing_points", "inducing_directions", "dim", "learn_inducing_locations", "ard_num_dims", "kwargs"]
    assert "kernel" not in inspect.signature(dsvgp.train_gp).parameters                          # read from **args, like ard_num_dims
    Z, V = torch.rand(6, 3), torch.eye(3)[:2].repeat(6, 1)
    rbf, mat, mat_ard = dsvgp.GPModel(Z, V, 3), dsvgp.GPModel(Z, V, 3, kernel="matern52"), dsvgp.GPModel(Z, V, 3, ard_num_dims=3, kernel="matern52")
    assert type(dsvgp.GPModel(Z, V, 3, kernel="rbf").covar_module.base_kernel) is type(rbf.covar_module.base_kernel)
    assert isinstance(mat.covar_module.base_kernel, Matern52KernelDirectionalGrad)
    assert mat.covar_module.base_kernel.raw_lengthscale.shape == (1, 1) and mat_ard.covar_module.base_kernel.raw_lengthscale.shape == (1, 3)
    sd_rbf, sd_mat = rbf.state_dict(), mat.state_dict()
    assert list(sd_rbf) == list(sd_mat) and all(sd_rbf[k].shape == sd_mat[k].shape for k in sd_rbf)
    assert list(dsvgp.GPModel(Z, V, 3, ard_num_dims=3).state_dict()) == list(mat_ard.state_dict())
    rbf.load_state_dict(sd_mat)                          # same keys and shapes: nothing in the state dict records the kernel
    with pytest.raises(ValueError, match="'rbf' or 'matern52'"):
        dsvgp.GPModel(Z, V, 3, kernel="matern32")
    for kw in (dict(variational_strategy="CIQ", variational_distribution="NGD"), dict(variational_distribution="NGD")):
        with pytest.raises(ValueError, match=WORD):
            dsvgp.GPModel(Z, V, 3, kernel="matern52", **kw)
    for kw in (dict(use_ngd=True), dict(use_ciq=True), dict(dfree=True), dict(shared=True)):
        with pytest.raises(ValueError, match=WORD):
            directional_vi.setup_training(None, num_inducing=4, kernel="matern52", **kw)
    with pytest.raises(ValueError, match=WORD):
        directional_vi.setup_training(None, num_inducing=4, kernel="matern52", tensors=(torch.rand(8, 3).double(), torch.rand(8, 4).double()))
    with pytest.raises(ValueError, match="'rbf' or 'matern52'"):
        directional_vi.setup_training(None, num_inducing=4, kernel="exp")
    with pytest.raises(ValueError, match="ARD lengthscales"):                                     # rbf: the existing message
        directional_vi.setup_training(None, num_inducing=4, ard_num_dims=3, use_ngd=True)
