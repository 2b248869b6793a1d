"""The patterns of gemm32_gram_kernel (csrc/gemm32.hip, csrc/gram_walk.h): diagonal tiles deal their 36 live MFMA tiles 9 per wave (DIAG),
off-diagonal tiles of a last tile row with 5 or 6 live MFMA rows deal them 12 per wave (ROWS3), every other tile runs the 4 x 4 quadrants
(FULL), and the workgroups get equal COST of the (tile, stage) sequence.  DSVGP_G32_GRAM_LIVE=0, read at every launch, is the kernel without
them: FULL everywhere, equal stage counts.

Every call goes through _ops.gemm under DSVGP_G32_GRAM=2, where a product the kernel does not take is an error: a call that returns ran it.
Each case runs with the patterns on (the default) and off.

Reference: tril(P P[:N]^T) in float64 on the GPU, P ~ randn seeded by the shape.  Elementwise bound, as in test_gpu_gemm32_gram.py:
(K + S + 2) 2^-24 |alpha| (|P| |P[:N]|^T), S = ceil(K / 32) -- K roundings of the fmaf chains over all partials of an element, at most one
partial per stage of a tile, each added by one atomic (one rounding), 2 for alpha and the first-order remainder.  It carries over because
every live MFMA tile of a tile has exactly one owning wave over a unit's whole stage range (tools/gram_walk_live_check.cpp shows it for
the tables): an element still receives one partial per unit.

Shapes (the kernel's floor is M, N, K >= 512): the smallest at which each path can go wrong -- see the cases.
"""
import os
from contextlib import contextmanager

import pytest
import torch

pytestmark = pytest.mark.gpu


@contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_CACHE = {}


def _operands(dev, M, N, K):
    """P, the float64 reference tril(P P[:N]^T) and |P| |P[:N]|^T: computed once per shape on the GPU, shared, never written"""
    key = (str(dev), M, N, K)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(M + N + K)
        P = torch.randn(M, K, generator=g).to(dev)
        Pd = P.double()
        _CACHE[key] = (P, torch.tril(Pd @ Pd[:N].t()), Pd.abs() @ Pd[:N].abs().t())
    return _CACHE[key]


def _run(dsvgp, dev, live, P, M, N, K, alpha, ldc, kchunks):
    ops, L = dsvgp._ops, dsvgp._lib
    ctx = ops.Context.get(dev)
    full = torch.full((M, ldc), float("nan"), device=dev)
    C = full[:, :N]
    with env(DSVGP_G32_GRAM=2, DSVGP_G32_GRAM_LIVE=None if live else 0, DSVGP_G32_GRAM_KCHUNKS=kchunks):
        ops.gemm(ctx, L.TRANS_B | L.OUT_LOWER, P, P[:N], C, alpha=alpha, M=M, N=N, K=K)
    torch.cuda.synchronize()
    return C, full


def _check(dsvgp, dev, name, M, N, K, alpha=1.0, ldc=None, kchunks=None):
    ldc = ldc or N + 8                                       # ldc > N always: the columns past N must stay NaN
    P, ref, absprod = _operands(dev, M, N, K)
    S = (K + 31) // 32
    bound = (K + S + 2) * 2.0 ** -24 * abs(alpha) * absprod
    low = torch.ones(M, N, device=dev).tril().bool()
    out = {}
    for live in (True, False):
        C, full = _run(dsvgp, dev, live, P, M, N, K, alpha, ldc, kchunks)
        worst = ((C.double() - alpha * ref).abs() / bound)[low].max().item()
        print("[gemm32 gram live] %s M=%d N=%d K=%d patterns %s: error / bound %.3f" % (name, M, N, K, "on" if live else "off", worst))
        assert worst <= 1.0, (live, worst)
        assert not torch.isnan(C).any(), live
        assert (C.triu(1) == 0).all(), live                  # the strict upper triangle is exactly 0
        assert torch.isnan(full[:, N:]).all(), live          # nothing outside [:M, :N] is written
        out[live] = full
    assert torch.equal(torch.isnan(out[True]), torch.isnan(out[False]))
    assert torch.equal(out[True] == 0, out[False] == 0)


def test_two_diagonal_tiles(dsvgp, gpu_device):
    """two full diagonal tiles (DIAG) and one FULL tile, 17 stages: a unit is one or two stages of one pattern"""
    _check(dsvgp, gpu_device, "diag", 512, 512, 544)


@pytest.mark.parametrize("r", [1, 33, 89, 97, 160, 185, 200, 256])
def test_ragged_last_tile_row(dsvgp, gpu_device, r):
    """R = 1 .. 8 live MFMA rows in the last tile row (r = 160, 185: ROWS3 with 5 and 6 rows, 185 the flagship's; the others keep FULL),
    the extra row M = N + 1, a corner tile that is diagonal and ragged, a K tail stage of 20"""
    _check(dsvgp, gpu_device, "ragged r=%d" % r, 512 + r, 511 + r, 532)


def test_cost_ranges_cross_unequal_tiles(dsvgp, gpu_device):
    """6 tiles of three weights x 512 stages: cost ranges start and end mid-tile and cross tiles of unequal weight"""
    _check(dsvgp, gpu_device, "long K", 697, 696, 16384)


def test_alpha_and_strided_output(dsvgp, gpu_device):
    """epilogue scaling and a strided output under DIAG and ROWS3"""
    _check(dsvgp, gpu_device, "alpha ldc", 697, 696, 1300, alpha=-1.0, ldc=704)


def test_flagship_walk_in_chunks(dsvgp, gpu_device):
    """the 78-tile weighted walk in three K chunks (the one-chunk walk is test_gpu_gemm32_gram.py::test_flagship_walk)"""
    _check(dsvgp, gpu_device, "78 tiles, 3 chunks", 3001, 3000, 1024, kchunks=3)


def test_in_the_step(dsvgp, gpu_device):
    """the one-call ELBO step of test_gpu_gemm32_gram.py::test_in_the_step (M' = 600, B' = 1536, its Gram product on the 256 x 256 kernel) with
    the patterns on against the same step with them off: two orders of the same fp32 atomics, at that test's tolerances; twice on one plan"""
    import dsvgp_oracle as O
    from test_gpu_step import make_problem, relmax
    N, d, M, p, B = 3000, 5, 200, 2, 512
    P, x, y, D, nd = make_problem(N, d, M, p, B, seed=N + d + 1)
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    xd, yd, Dd = x.to(gpu_device), y.to(gpu_device), D.to(gpu_device)
    with env(DSVGP_G32_GRAM=1, DSVGP_G32_GRAM_LIVE=0):
        ref = dsvgp.ElboEngine(gpu_device)
        l0, g0, mu0, _ = ref.loss_and_grads(Pg, xd, yd, Dd, nd)
        torch.cuda.synchronize()
        assert ref.c_step_used
    with env(DSVGP_G32_GRAM=1, DSVGP_G32_GRAM_LIVE=None):
        eng = dsvgp.ElboEngine(gpu_device)
        for call in range(2):                                # the second call runs on the same plan / workspace
            l1, g1, mu1, _ = eng.loss_and_grads(Pg, xd, yd, Dd, nd)
            torch.cuda.synchronize()
            assert eng.c_step_used
            errs = {k: relmax(g1[k], g0[k]) for k in O.PARAM_NAMES if g0[k].numel()}
            print("[gemm32 gram live] step call %d: loss %.3e mean %.3e grads %s" % (call, abs(l1.item() - l0.item()) / abs(l0.item()),
                                                                                     relmax(mu1, mu0), ", ".join("%s %.1e" % kv for kv in errs.items())))
            assert abs(l1.item() - l0.item()) < 4e-6 * abs(l0.item()), (call, l1.item(), l0.item())
            assert relmax(mu1, mu0) < 4e-6, (call, relmax(mu1, mu0))
            for k, e in errs.items():
                assert e < 5e-5, (call, k, e)
            assert g1["chol_variational_covar"].triu(1).abs().max().item() == 0.0
