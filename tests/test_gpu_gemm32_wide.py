"""The 256 x 192 fp32 dense kernel of csrc/gemm32.hip (gemm32_wide_kernel) against the 128 x 128 LDS-DMA kernel it stands in for.

DSVGP_G32_WIDE is read at every launch: 1 sends every product the wide kernel can take to it (K whole), 2 does the same and makes
a product it cannot take an error -- a call that returns under 2 therefore ran the wide kernel --, -1 runs the 128 x 128 kernel with
K whole on the same products, 0 is the 128 x 128 kernel's own launch.  At these sizes that launch splits K over workgroups that
meet in atomics (no fixed order, other chains), so the bit-for-bit reference of the wide kernel is -1: the same kernel as 0,
gemm32_dma_kernel<32, true, false, 32>, over the same K range as the wide one.  0 is compared at the fp32 chain bound below.

Error bound against float64: both kernels add the K products of an output element in one fmaf chain (one rounding per term) and
scale by alpha once, so |C - alpha A B| <= (K + 1) 2^-24 |alpha| (|A| |B|) elementwise to first order; the test allows (K + 2) 2^-24.
"""
import os
from contextlib import contextmanager

import pytest
import torch

pytestmark = pytest.mark.gpu


@contextmanager
def wide_mode(value):
    old = os.environ.get("DSVGP_G32_WIDE")
    os.environ["DSVGP_G32_WIDE"] = str(value)
    try:
        yield
    finally:
        if old is None:
            del os.environ["DSVGP_G32_WIDE"]
        else:
            os.environ["DSVGP_G32_WIDE"] = old


def _operands(dev, M, N, K, lda, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.zeros(M, lda)
    A[:, :K] = torch.randn(M, K, generator=g)               # zero-padded up to lda (DSVGP_GEMM_K_PADDED)
    B = torch.randn(K, N, generator=g)
    return A.to(dev), B.to(dev)


def _run(dsvgp, dev, mode, A, B, M, N, K, alpha=1.0, ldc=None, flags=None):
    ops, L = dsvgp._ops, dsvgp._lib
    ctx = ops.Context.get(dev)
    C = torch.full((M, ldc or N), float("nan"), device=dev)[:, :N]
    with wide_mode(mode):
        ops.gemm(ctx, L.K_PADDED if flags is None else flags, A, B, C, alpha=alpha, M=M, N=N, K=K)
    torch.cuda.synchronize()
    return C


def _check(dsvgp, dev, name, M, N, K, lda, alpha=1.0, ldc=None):
    A, B = _operands(dev, M, N, K, lda, seed=M + N + K)
    wide = _run(dsvgp, dev, 1, A, B, M, N, K, alpha, ldc)
    strict = _run(dsvgp, dev, 2, A, B, M, N, K, alpha, ldc)         # returns only if the wide kernel took the product
    old_whole = _run(dsvgp, dev, -1, A, B, M, N, K, alpha, ldc)
    old = _run(dsvgp, dev, 0, A, B, M, N, K, alpha, ldc)
    ref = alpha * (A[:, :K].double() @ B.double())
    bound = (K + 2) * 2.0 ** -24 * abs(alpha) * (A[:, :K].double().abs() @ B.double().abs())
    worst = lambda C: ((C.double() - ref).abs() / bound).max().item()
    print("[gemm32 wide] %s M=%d N=%d K=%d: error / bound  wide %.3f  128x128 K whole %.3f  128x128 (its own launch) %.3f; bits equal %s"
          % (name, M, N, K, worst(wide), worst(old_whole), worst(old), torch.equal(wide, old_whole)))
    assert torch.equal(wide, old_whole)
    assert torch.equal(strict, wide)
    assert worst(wide) <= 1.0
    assert worst(wide) <= worst(old_whole)
    assert worst(old) <= 1.0
    if ldc:                                                 # the padding of a strided output is not written
        assert torch.isnan(wide.as_strided((M, ldc - N), (ldc, 1), wide.storage_offset() + N)).all()


def test_exact_tiles(dsvgp, gpu_device):
    """whole tiles (2 x 3), whole stages"""
    _check(dsvgp, gpu_device, "exact", 512, 576, 512, 512)


def test_ragged(dsvgp, gpu_device):
    """88 valid rows in the last tile row, 124 valid columns in the last tile column, a one-element K tail stage"""
    _check(dsvgp, gpu_device, "ragged", 600, 700, 545, 548)


def test_alpha_and_strided_output(dsvgp, gpu_device):
    """epilogue scaling; ldc > N"""
    _check(dsvgp, gpu_device, "alpha", 600, 700, 545, 548, alpha=-1.0)
    _check(dsvgp, gpu_device, "alpha ldc", 600, 700, 545, 548, alpha=-1.0, ldc=708)


def test_tall(dsvgp, gpu_device):
    """twelve tile rows, one band of eight tile columns: the tile walk of the flagship's K_ZX-bar product"""
    _check(dsvgp, gpu_device, "tall", 3000, 1536, 3001, 3004)


def test_fallback(dsvgp, gpu_device):
    """products the wide kernel does not take stay on the old path under 1 (and are refused under 2)"""
    L = dsvgp._lib
    dev = gpu_device
    # M = 300: below the fp32 MFMA kernels' smallest product
    M, N, K = 300, 700, 545
    A, B = _operands(dev, M, N, K, 548, seed=5)
    ref = A[:, :K].double() @ B.double()
    bound = (K + 2) * 2.0 ** -24 * (A[:, :K].double().abs() @ B.double().abs())
    C = _run(dsvgp, dev, 1, A, B, M, N, K)
    assert ((C.double() - ref).abs() / bound).max().item() <= 1.0
    # a lower-triangular output (the Gram product's form)
    M = N = 640
    K = 1024
    g = torch.Generator().manual_seed(6)
    P = torch.randn(M, K, generator=g).to(dev)
    ref = torch.tril(P.double() @ P.double().t())
    bound = (K + 2) * 2.0 ** -24 * (P.double().abs() @ P.double().abs().t())
    for mode in (1, 0):
        C = _run(dsvgp, dev, mode, P, P, M, N, K, flags=L.TRANS_B | L.OUT_LOWER)
        assert ((C.double() - ref).abs() / bound).max().item() <= 1.0
    with pytest.raises(L.DsvgpError):
        _run(dsvgp, dev, 2, P, P, M, N, K, flags=L.TRANS_B | L.OUT_LOWER)
