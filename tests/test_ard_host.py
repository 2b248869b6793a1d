"""CPU: the float64 ARD yardstick (tests/_ard_yardstick.py) pinned to what it must equal -- the scalar-lengthscale yardstick at equal
lengthscales, and directional derivatives of the ARD RBF function taken by autograd."""
import math

import pytest
import torch

import dsvgp_oracle as O
from _ard_yardstick import ard_elbo, ard_kernel
from test_gpu_rect_predict import rect_kernel
from test_gpu_rect_train import rect_elbo, relmax


@pytest.mark.parametrize("n1,p1,n2,p2,d", [(5, 2, 7, 3, 4), (4, 0, 6, 2, 3), (6, 3, 5, 0, 5), (4, 2, 4, 2, 3)])
def test_equal_lengthscales_give_the_scalar_kernel(n1, p1, n2, p2, d):
    g = torch.Generator().manual_seed(3 + n1 + d)
    x1, x2 = torch.rand(n1, d, generator=g, dtype=torch.float64), torch.rand(n2, d, generator=g, dtype=torch.float64)
    v1, v2 = torch.randn(n1 * p1, d, generator=g, dtype=torch.float64), torch.randn(n2 * p2, d, generator=g, dtype=torch.float64)
    ell = 0.7
    K = ard_kernel(x1, v1, p1, x2, v2, p2, torch.full((d,), ell, dtype=torch.float64))
    assert K.shape == (n1 * (p1 + 1), n2 * (p2 + 1))
    assert relmax(K, rect_kernel(x1, v1, p1, x2, v2, p2, torch.tensor(ell, dtype=torch.float64))) <= 1e-12


@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
@pytest.mark.parametrize("pd", [0, 2, 3])
def test_equal_lengthscales_give_the_scalar_objective(mll, pd):
    from test_gpu_step import make_problem
    N, d, M, p, B = 400, 3, 16, 2, 96
    P, x, _, _, nd = make_problem(N, d, M, p, B, seed=11)
    g = torch.Generator().manual_seed(5 + pd)
    y = torch.randn(B * (pd + 1), generator=g, dtype=torch.float64)
    D = torch.randn(B * pd, d, generator=g, dtype=torch.float64)
    P64 = {k: v.double() for k, v in P.items()}
    ref = rect_elbo(P64, x.double(), y, D, pd, nd, mll)
    Pard = dict(P64, raw_lengthscale=P64["raw_lengthscale"].reshape(1, 1).expand(1, d).contiguous())
    mine = ard_elbo(Pard, x.double(), y, D, pd, nd, mll)
    assert abs(mine[0].item() - ref[0].item()) <= 1e-12 * abs(ref[0].item())
    assert relmax(mine[2], ref[2]) <= 1e-12 and relmax(mine[3], ref[3]) <= 1e-12
    for k in O.PARAM_NAMES:
        a = mine[1][k].sum().reshape(1) if k == "raw_lengthscale" else mine[1][k]      # the scalar's gradient is the sum over dimensions
        assert relmax(a, ref[1][k].reshape(a.shape)) <= 1e-12, k


def test_every_block_is_a_directional_derivative_of_the_ard_rbf():
    n, d, p = 3, 3, 2
    g = torch.Generator().manual_seed(0)
    x, z = torch.rand(n, d, generator=g, dtype=torch.float64), torch.rand(n, d, generator=g, dtype=torch.float64)
    vx, vz = torch.randn(n * p, d, generator=g, dtype=torch.float64), torch.randn(n * p, d, generator=g, dtype=torch.float64)
    ell = torch.tensor([0.3, 0.8, 1.7], dtype=torch.float64)
    K = ard_kernel(x, vx, p, z, vz, p, ell).reshape(n, p + 1, n, p + 1)
    ux, uz = O.normalize_rows(vx).reshape(n, p, d), O.normalize_rows(vz).reshape(n, p, d)
    worst = 0.0
    for i in range(n):
        for j in range(n):
            xi, zj = x[i].clone().requires_grad_(True), z[j].clone().requires_grad_(True)
            k = torch.exp(-0.5 * (((xi - zj) / ell) ** 2).sum())
            gx, gz = torch.autograd.grad(k, (xi, zj), create_graph=True)
            want = torch.zeros(p + 1, p + 1, dtype=torch.float64)
            want[0, 0] = k.detach()
            for b in range(p):
                want[0, 1 + b] = (gz @ uz[j, b]).detach()
            for a in range(p):
                da = gx @ ux[i, a]
                want[1 + a, 0] = da.detach()
                hz, = torch.autograd.grad(da, zj, retain_graph=True)
                for b in range(p):
                    want[1 + a, 1 + b] = hz @ uz[j, b]
            worst = max(worst, (K[i, :, j, :] - want).abs().max().item())
    print("[parity] ard_kernel vs autograd of the ARD RBF: %.2e" % worst)
    assert worst <= 1e-12 * max(1.0, K.abs().max().item())
    assert math.isfinite(worst)
