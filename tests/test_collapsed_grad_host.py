"""Gradients of the collapsed bound, CPU part: the closed forms of tests/_collapsed_grad_ref.py against float64 autograd through the factor,
the whitened operand, the statistics, the optimum and the loss; the envelope identity; the surface of the new C entries and the
Python-level argument errors that need no device.

Bounds (float64): closed forms against autograd 1e-10 of the largest entry (observed <= 6e-13); asymmetry of N and the two forms of N
1e-12 of its largest entry; the envelope 1e-9 of each gradient's largest entry."""
import functools
import inspect
import os
import re

import pytest
import torch

import _collapsed_ref as R
import _collapsed_grad_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CASES = ["a", "d", "e", "g", "h"]      # RBF square, values only, pd = d, ARD, Matern-5/2


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@functools.lru_cache(maxsize=None)
def _case(name):
    P, x, y, D, nd, _, _, kernel = R.problem(name)
    return P, x, y, D, nd, kernel, GR.closed_forms(P, x, y, D, nd, kernel), GR.matrix_adjoints_autograd(P, x, y, D, nd, kernel)


@pytest.mark.parametrize("name", HOST_CASES)
def test_closed_forms_against_autograd(name):
    _, _, _, _, _, _, cf, ag = _case(name)
    errs = {k: rel(cf[k], ag[k]) for k in ("Kbar", "Ktbar", "dgbar")}
    errs["Ktbar_from_N"] = rel(cf["Ktbar_from_N"], ag["Ktbar"])
    scale = max(abs(ag["cbar"].item()), abs(ag["dnoise"].item()))
    errs["cbar"] = abs(cf["cbar"].item() - ag["cbar"].item()) / scale
    errs["dnoise"] = abs(cf["dnoise"].item() - ag["dnoise"].item()) / scale
    errs["loss"] = abs(cf["loss"].item() - ag["loss"].item()) / abs(ag["loss"].item())
    print("[collapsed-grad] case %s: " % name + ", ".join("%s %.2e" % kv for kv in sorted(errs.items())))
    assert all(v <= 1e-10 for v in errs.values()), errs


@pytest.mark.parametrize("name", HOST_CASES)
def test_n_is_symmetric_and_needs_no_product(name):
    cf = _case(name)[6]
    N, Nf = cf["N_product"], cf["N_free"]
    scale = N.abs().max().item()
    asym, diff = (N - N.t()).abs().max().item() / scale, (N - Nf).abs().max().item() / scale
    print("[collapsed-grad] case %s: asymmetry of N %.2e, product-free form %.2e" % (name, asym, diff))
    assert asym <= 1e-12 and diff <= 1e-12


@pytest.mark.parametrize("name", HOST_CASES)
def test_envelope(name):
    P, x, y, D, nd, kernel = _case(name)[:6]
    loss, g, m, L_S = GR.collapsed_loss_and_grads(P, x, y, D, nd, kernel)
    loss_f, g_f, _, _ = GR.collapsed_loss_and_grads(P, x, y, D, nd, kernel, at_fixed_optimum=True)
    assert abs(loss.item() - loss_f.item()) <= 1e-12 * abs(loss.item())
    errs = {k: rel(g_f[k], g[k]) for k in GR.GRAD_NAMES}
    print("[collapsed-grad] case %s: envelope " % name + ", ".join("%s %.2e" % kv for kv in errs.items()))
    assert all(v <= 1e-9 for v in errs.values()), errs
    assert all(g[k].abs().max().item() > 0 for k in GR.GRAD_NAMES)


def test_two_chunks_merged_equal_one_chunk():
    P, x, y, D, nd, kernel, cf, _ = _case("a")
    q = D.shape[0] // x.shape[0] + 1
    cut = 61
    Pd = {k: v.double() for k, v in P.items()}
    parts, csum = [], 0.0
    for lo, hi in ((0, cut), (cut, x.shape[0])):
        _, K, _, _ = GR.kernel_matrices(Pd, x[lo:hi].double(), D[lo * (q - 1):hi * (q - 1)].double(), kernel)
        r = y[lo * q:hi * q].double() - Pd["constant"].reshape(())
        parts.append(GR.kbar_chunk(cf["Q"], cf["alpha"], cf["w"], K, r))
        csum = csum + (-2.0 * cf["w"] * (r - K.t() @ cf["alpha"]).sum())
    assert rel(torch.cat(parts, dim=1), cf["Kbar"]) <= 1e-12
    assert abs(csum.item() - cf["cbar"].item()) <= 1e-12 * abs(cf["cbar"].item())
    # ... and the merged statistics give the same optimum, hence the same K~-bar
    whole = R.statistics(P, x, y, D, kernel)
    merged = R.merge(R.statistics(P, x[:cut], y[:cut * q], D[:cut * (q - 1)], kernel), R.statistics(P, x[cut:], y[cut * q:], D[cut * (q - 1):], kernel))
    for a, b in zip(R.optimum(whole, num_data=nd)[:2], R.optimum(merged, num_data=nd)[:2]):
        assert rel(a, b) <= 1e-10


# ------------------------------------------------------------------ the surface of the new entries
ENTRIES = (("dsvgp_collapsed_grad_workspace_bytes", 1), ("dsvgp_collapsed_grad_chunk_bytes", 2), ("dsvgp_collapsed_grad_prepare", 17),
           ("dsvgp_collapsed_grad_chunk", 16))


def test_library_exports_declares_and_binds_the_entries(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    for n, nargs in ENTRIES:
        assert hasattr(dsvgp._lib.lib, n), "missing export: " + n
        assert n in dsvgp._lib.SIGNATURES, "missing binding: " + n
        decl = re.search(r"^(?:size_t|int)\s+%s\s*\((.*?)\)\s*;" % n, hdr, flags=re.S | re.M)      # (the prototype, not the prose above it)
        assert decl, "not declared in include/dsvgp.h: " + n
        assert len(decl.group(1).split(",")) == len(dsvgp._lib.SIGNATURES[n][1]) == nargs, n
    ops = dsvgp._ops
    assert list(inspect.signature(ops.collapsed_grad_chunk).parameters) == ["ctx", "Mp", "Kzx", "y", "constant", "Q", "alpha", "adj", "K_bar",
                                                                            "diag_bar", "rho_sum", "workspace"]
    assert list(inspect.signature(ops.collapsed_grad_prepare).parameters) == ["ctx", "state", "Mp", "m", "LS", "inverse", "hyp", "num_data",
                                                                              "workspace"]
    acc = dsvgp.CollapsedAccumulator
    assert list(inspect.signature(acc.begin_backward).parameters) == ["self", "result"]
    assert list(inspect.signature(acc.add_backward).parameters) == ["self", "x", "y", "D"]
    assert list(inspect.signature(acc.finish_backward).parameters) == ["self"]
    assert dsvgp.COLLAPSED_GRAD_NAMES == GR.GRAD_NAMES
    params = inspect.signature(dsvgp.collapsed_loss_and_grads).parameters
    assert list(params) == ["model", "likelihood", "dataset_or_tensors", "minibatch_size", "data_directions", "num_data", "seed",
                            "workspace_budget", "write_variational"]
    assert params["minibatch_size"].default == 4096 and params["workspace_budget"].default == 1 << 30 and params["write_variational"].default is True
    assert list(inspect.signature(dsvgp.GPModel.collapsed_loss_and_grads).parameters)[1:] == list(params)[1:]
    params = inspect.signature(dsvgp.train_collapsed).parameters
    assert list(params)[:7] == ["train_dataset", "num_inducing", "num_directions", "num_iterations", "learning_rate_hypers", "minibatch_size",
                                "data_directions"]
    assert params["num_iterations"].default == 50 and params["learning_rate_hypers"].default == 0.01 and params["minibatch_size"].default == 4096
    for k in ("kernel", "ard_num_dims", "inducing_data_initialization", "seed", "fixed_inducing_locations", "verbose"):
        assert k in params, k
    assert "num_iterations" not in inspect.signature(dsvgp.train_gp).parameters         # (train_gp's signature is untouched)


def test_size_helpers(dsvgp):
    lib = dsvgp._lib.lib
    ws, ch = lib.dsvgp_collapsed_grad_workspace_bytes, lib.dsvgp_collapsed_grad_chunk_bytes
    for bad in (0, -3, 8193):
        assert ws(bad) == 0 and ch(bad, 100) == 0, bad
    assert ch(72, 0) == 0 and ch(72, -5) == 0
    assert ws(72) >= 8 * 4 * 72 * 72 and ws(129) > ws(72)
    sizes = [ch(129, b) for b in (1, 2, 63, 64, 65, 450, 4096, 24576)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)       # monotone in B'
    assert ch(129, 450) == 8 * 450 * (1 + 1) and ch(300, 450) == 8 * 450 * (2 + 1)                      # one slab per 256 rows, then rho
    assert dsvgp._ops.collapsed_grad_chunk_bytes(72, 450) == ch(72, 450) and dsvgp._ops.collapsed_grad_workspace_bytes(0) == 0


# ------------------------------------------------------------------ Python-level argument errors: no device is touched before them
def _cpu_accumulator(dsvgp):
    M, d, p = 4, 3, 2
    Mp = M * (p + 1)
    eng = dsvgp.ElboEngine(torch.device("cpu"))
    z = lambda *s: torch.zeros(*s)
    return dsvgp.CollapsedAccumulator(eng, z(4), (z(Mp, 8), z(Mp), z(M * p)), z(Mp, Mp).double(), (M, d, p, Mp), z(16 * Mp * Mp).to(torch.uint8), z(d),
                                      z(1), None, False, 1 << 20)


def test_backward_argument_errors_come_before_any_device_work(dsvgp):
    acc = _cpu_accumulator(dsvgp)
    x, y, D = torch.zeros(7, 3), torch.zeros(21), torch.ones(14, 3)
    with pytest.raises(ValueError, match="begin_backward"):
        acc.add_backward(x, y, D)
    with pytest.raises(ValueError, match="begin_backward"):
        acc.finish_backward()
    with pytest.raises(TypeError, match="CollapsedResult"):
        acc.begin_backward((None, None))
    res = dsvgp.CollapsedResult(torch.zeros(12), torch.eye(12), None, None, dict(loss=1.0, rows=21.0), 21.0)
    with pytest.raises(ValueError, match="solve"):
        acc.begin_backward(res)                                 # no solve yet
    acc._rows, acc._solved = 21, (50.0, 21)
    with pytest.raises(ValueError, match=r"num_data = 21.0 .* num_data = 50.0"):
        acc.begin_backward(res)                                 # a result of another num_data
    acc._solved = (21.0, 21)
    with pytest.raises(TypeError, match="on the GPU"):
        acc.begin_backward(res)                                 # CPU tensors
    acc._bwd = {"rows": 0, "points": 0}
    with pytest.raises(ValueError, match=r"x must be \[B, 3\]"):
        acc.add_backward(torch.zeros(7, 4), y, D)
    with pytest.raises(ValueError, match="interleaved"):
        acc.add_backward(x, y[:-1], D)
    with pytest.raises(ValueError, match="derivative directions"):
        acc.add_backward(x, y, torch.ones(15, 3))
    with pytest.raises(ValueError, match="at most 95"):
        acc.add_backward(torch.zeros(1, 3), torch.zeros(97), torch.ones(96, 3))
    with pytest.raises(TypeError, match="on the GPU"):
        acc.add_backward(x, y, D)
    for moved in (lambda: acc.add(x, y, D), lambda: acc.solve()):
        with pytest.raises(ValueError, match="between begin_backward and finish_backward"):
            moved()
    acc._bwd["rows"] = 9
    with pytest.raises(ValueError, match=r"seen 9 rows.*R = 21"):
        acc.finish_backward()
    assert acc.row_bytes(2, backward=True) < acc.row_bytes(2) and acc.chunk_rows(2, backward=True) >= acc.chunk_rows(2)
