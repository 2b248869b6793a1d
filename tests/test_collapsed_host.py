"""Closed-form optimal q(u): the float64 reference of tests/_collapsed_ref.py against the oracle's objective (``elbo_loss_and_grads`` on all
rows as one batch), and the refusals of the engine and the harness that need no device.

Bounds: at the optimum the gradient with respect to ``variational_mean`` and ``tril chol_variational_covar`` is at most 1e-10 of its size
at (0, I) (float64 round-off times cond(B) < 1e4); the loss from the statistics equals ``elbo_forward`` to 1e-12 relative; gpytorch's
``natural_to_mu_chol`` returns (m*, L_S*) from the natural pair to 1e-10."""
import functools

import pytest
import torch

import dsvgp_oracle as O
import _collapsed_ref as R

HOST_CASES = ["a", "b", "c"]                # (N, d, M, p) = (150, 3, 24, 2), (203, 4, 43, 2), (97, 5, 13, 4); num_data / R = 1, 2.5, 0.7


@functools.lru_cache(maxsize=None)
def _case(name):
    P, x, y, D, nd, _, _, kernel = R.problem(name)
    P64 = {k: v.double() for k, v in P.items()}
    stats = R.statistics(P, x, y, D, kernel)
    return P64, x.double(), y.double(), D.double(), nd, stats


def _grads(P64, x, y, D, nd, m, L_S):
    Q = dict(P64, variational_mean=m.clone(), chol_variational_covar=L_S.clone())
    loss, g, _, _ = O.elbo_loss_and_grads(Q, x, y, D, nd)
    return loss, g["variational_mean"].abs().max().item(), torch.tril(g["chol_variational_covar"]).abs().max().item()


@pytest.mark.parametrize("name", HOST_CASES)
def test_the_optimum_is_stationary_for_the_oracle(name):
    P64, x, y, D, nd, stats = _case(name)
    assert nd != stats["R"] or name == "a"                      # (num_data != R is part of the cases)
    cond = R.cond_B(stats, num_data=nd)
    assert cond < 1e4, cond
    m, L_S, _, _ = R.optimum(stats, num_data=nd)
    assert torch.equal(L_S, torch.tril(L_S)) and (L_S.diagonal() > 0).all()
    assert (L_S @ L_S.t() - torch.linalg.inv(-2.0 * R.optimum(stats, num_data=nd)[3])).abs().max() < 1e-12
    n = m.shape[0]
    _, gm0, gl0 = _grads(P64, x, y, D, nd, torch.zeros(n, dtype=torch.float64), torch.eye(n, dtype=torch.float64))
    loss, gm, gl = _grads(P64, x, y, D, nd, m, L_S)
    print("[collapsed] case %s: cond(B) %.2e, |dm| %.2e -> %.2e, |dL_S| %.2e -> %.2e" % (name, cond, gm0, gm, gl0, gl))
    assert gm <= 1e-10 * gm0 and gl <= 1e-10 * gl0, (gm, gm0, gl, gl0)
    assert abs(R.loss(stats, m, L_S, num_data=nd).item() - loss.item()) <= 1e-12 * abs(loss.item())
    g = torch.Generator().manual_seed(5)
    for _ in range(3):                                          # random perturbations of the optimum always raise the loss
        dm = 1e-3 * torch.randn(n, generator=g, dtype=torch.float64)
        dL = 1e-3 * torch.tril(torch.randn(n, n, generator=g, dtype=torch.float64))
        assert R.loss(stats, m + dm, L_S + dL, num_data=nd) > R.loss(stats, m, L_S, num_data=nd)


@pytest.mark.parametrize("name", HOST_CASES)
def test_the_statistic_loss_is_the_oracles_objective(name):
    P64, x, y, D, nd, stats = _case(name)
    n = stats["b"].shape[0]
    g = torch.Generator().manual_seed(11)
    for _ in range(3):
        m = 0.3 * torch.randn(n, generator=g, dtype=torch.float64)
        L_S = torch.eye(n, dtype=torch.float64) + 0.05 * torch.randn(n, n, generator=g, dtype=torch.float64)   # (above the diagonal: masked)
        Q = dict(P64, variational_mean=m, chol_variational_covar=L_S)
        ref, _, _ = O.elbo_forward(Q, x, y, D, nd)
        got = R.loss(stats, m, L_S, num_data=nd)
        assert abs(got.item() - ref.item()) <= 1e-12 * abs(ref.item()), (got.item(), ref.item())


@pytest.mark.parametrize("name", HOST_CASES)
def test_the_natural_pair_is_the_same_distribution(name):
    _, _, _, _, nd, stats = _case(name)
    m, L_S, nat_vec, nat_mat = R.optimum(stats, num_data=nd)
    mu, chol = O.natural_to_mu_chol(nat_vec, nat_mat)
    assert (mu - m).abs().max() <= 1e-10 * m.abs().max() and (chol - L_S).abs().max() <= 1e-10 * L_S.abs().max()


def test_merged_statistics_are_those_of_the_union():
    P, x, y, D, nd, _, _, kernel = R.problem("c")
    whole = R.statistics(P, x, y, D, kernel)
    q = D.shape[0] // x.shape[0] + 1
    parts = R.merge(R.statistics(P, x[:50], y[:50 * q], D[:50 * (q - 1)], kernel), R.statistics(P, x[50:], y[50 * q:], D[50 * (q - 1):], kernel))
    assert (parts["G"] - whole["G"]).abs().max() <= 1e-10 * whole["absG"].max() and parts["R"] == whole["R"]


# ------------------------------------------------------------------ refusals that need no device
def _params():
    P = R.problem("c")[0]
    return P


def test_engine_refusals(dsvgp):
    P = _params()
    with pytest.raises(NotImplementedError, match="float32 model mode only"):
        dsvgp.ElboEngine64("cuda").collapsed_accumulator({k: v.double() for k, v in P.items()})
    eng = dsvgp.ElboEngine("cuda")
    eng.whitening = "ciq"
    with pytest.raises(ValueError, match="CIQ whitening"):
        eng.collapsed_accumulator(P)
    eng = dsvgp.ElboEngine("cuda")
    eng.shared_directions = True
    with pytest.raises(ValueError, match="shared-directions"):
        eng.collapsed_accumulator(P)
    eng = dsvgp.ElboEngine("cuda")

    class Stub:
        rank, world = 0, 2
    eng.collective = Stub()
    with pytest.raises(ValueError, match="world = 2"):
        eng.collapsed_accumulator(P)
    eng = dsvgp.ElboEngine("cuda")
    with pytest.raises(ValueError, match="float32 models"):
        eng.collapsed_accumulator({k: v.double() for k, v in P.items()})


def test_variational_initialization_value_is_checked_before_any_device_work(dsvgp):
    with pytest.raises(ValueError, match="variational_initialization must be None or 'optimal'"):
        dsvgp.setup_training(None, variational_initialization="best")
    with pytest.raises(ValueError, match="variational_initialization must be None or 'optimal'"):
        dsvgp.train_gp(None, variational_initialization=True, verbose=False)


def test_size_helpers_refuse_what_the_entries_refuse(dsvgp):
    lib = dsvgp._lib.lib
    assert lib.dsvgp_collapsed_state_bytes(0) == 0 and lib.dsvgp_collapsed_state_bytes(-3) == 0
    assert lib.dsvgp_collapsed_state_bytes(5) == 8 * (8 + 36)
    assert lib.dsvgp_collapsed_workspace_bytes(0) == 0 and lib.dsvgp_collapsed_workspace_bytes(8193) == 0
    assert lib.dsvgp_collapsed_workspace_bytes(72) > 8 * 3 * 72 * 72
