"""The 256 x 256 stream-K kernel of csrc/gemm32.hip (gemm32_gram_kernel) against the split-K launch of the 128 x 128 kernel it stands in for.

DSVGP_G32_GRAM is read at every launch: 1 sends every lower-triangular product of two k-contiguous operands the kernel can take to it,
2 does the same and makes a lower-triangular product it cannot take an error -- a call that returns under 2 therefore ran the new
kernel --, 0 is the 128 x 128 kernel's own launch.  Both launches meet in fp32 atomics, in no fixed order: there is no bitwise reference.

Error bound against float64, elementwise: (K + S + 2) 2^-24 |alpha| (|P| |P[:N]|^T) with S = ceil(K / 32).  One fmaf chain per partial sum:
K roundings over all partials of an element; at most one partial per stage of a tile, each added by one atomic (one rounding): at most S
more; the scaling by alpha and the first-order remainder take the 2.  Derived, not tuned; the old launch is held to the same bound.

Not covered: a product under the deterministic slab -- the slab is set by the step's deterministic mode, not through _ops.gemm, and no
fp32 product of that mode has this form; the launcher's `!g.slab` gate is read from the code.
"""
import os
from contextlib import contextmanager

import pytest
import torch

pytestmark = pytest.mark.gpu

C_ZEROED, UPPER_UNDEF = 1 << 21, 1 << 22      # internal flags of csrc/common.h (the one-call step sets them): dsvgp_gemm passes them on


@contextmanager
def gram_mode(value):
    old = os.environ.get("DSVGP_G32_GRAM")
    os.environ["DSVGP_G32_GRAM"] = str(value)
    try:
        yield
    finally:
        if old is None:
            del os.environ["DSVGP_G32_GRAM"]
        else:
            os.environ["DSVGP_G32_GRAM"] = old


_CACHE = {}


def _operands(dev, M, N, K):
    """P, the float64 reference tril(P P[:N]^T) and |P| |P[:N]|^T: computed once per shape, shared, never written"""
    key = (str(dev), M, N, K)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(M + N + K)
        P = torch.randn(M, K, generator=g).to(dev)
        Pd = P.double()
        _CACHE[key] = (P, torch.tril(Pd @ Pd[:N].t()), Pd.abs() @ Pd[:N].abs().t())
    return _CACHE[key]


def _run(dsvgp, dev, mode, P, M, N, K, alpha=1.0, ldc=None, extra=0, fill=float("nan"), trans_b=True, B=None):
    ops, L = dsvgp._ops, dsvgp._lib
    ctx = ops.Context.get(dev)
    full = torch.full((M, ldc or N), fill, device=dev)
    C = full[:, :N]
    flags = (L.TRANS_B if trans_b else 0) | L.OUT_LOWER | extra
    with gram_mode(mode):
        ops.gemm(ctx, flags, P, P[:N] if B is None else B, C, alpha=alpha, M=M, N=N, K=K)
    torch.cuda.synchronize()
    return C, full


def _check(dsvgp, dev, name, M, N, K, alpha=1.0, ldc=None, extra=0, fill=float("nan"), lower_only=False):
    P, ref, absprod = _operands(dev, M, N, K)
    S = (K + 31) // 32
    bound = (K + S + 2) * 2.0 ** -24 * abs(alpha) * absprod
    new, new_full = _run(dsvgp, dev, 1, P, M, N, K, alpha, ldc, extra, fill)
    strict, _ = _run(dsvgp, dev, 2, P, M, N, K, alpha, ldc, extra, fill)         # returns only if the new kernel took the product
    old, old_full = _run(dsvgp, dev, 0, P, M, N, K, alpha, ldc, extra, fill)
    low = torch.ones(M, N, device=dev).tril().bool()
    worst = lambda C: ((C.double() - alpha * ref).abs() / bound)[low].max().item()
    print("[gemm32 gram] %s M=%d N=%d K=%d: error / bound  stream-K %.3f  (under 2: %.3f)  128x128 split-K %.3f"
          % (name, M, N, K, worst(new), worst(strict), worst(old)))
    assert worst(new) <= 1.0
    assert worst(strict) <= 1.0
    assert worst(old) <= 1.0
    if not lower_only:
        for C in (new, strict, old):
            assert not torch.isnan(C).any()
            assert (C.triu(1) == 0).all()                    # the strict upper triangle is exactly 0
        # the same NaN and zero pattern as the old launch, over the whole buffer: nothing outside [:M, :N] is written
        assert torch.equal(torch.isnan(new_full), torch.isnan(old_full))
        assert torch.equal(new_full == 0, old_full == 0)
        if ldc:
            assert torch.isnan(new_full[:, N:]).all()
    else:
        assert not torch.isnan(new[low]).any()


def test_few_stages(dsvgp, gpu_device):
    """3 tiles x 16 stages = 48 stages for one workgroup per CU: most workgroups get no range, every stage of a tile is its own partial"""
    _check(dsvgp, gpu_device, "few stages", 512, 512, 512)


def test_ragged_one_stage_each(dsvgp, gpu_device):
    """6 tiles, ragged last tile row and column (89 / 88 valid), 41 stages with a 20-element K tail stage, at most one stage per workgroup"""
    _check(dsvgp, gpu_device, "ragged", 601, 600, 1300)


def test_ranges_cross_tile_boundaries(dsvgp, gpu_device):
    """6 x 512 stages: ranges of about 12 stages that start and end mid-tile and cross tile boundaries"""
    _check(dsvgp, gpu_device, "long K", 601, 600, 16384)


def test_flagship_walk(dsvgp, gpu_device):
    """the flagship's 78-tile walk, 32 stages per tile, ranges of 9-10 stages crossing boundaries, the extra row b^T in the ragged last tile row"""
    _check(dsvgp, gpu_device, "78 tiles", 3001, 3000, 1024)


def test_alpha_and_strided_output(dsvgp, gpu_device):
    """epilogue scaling; ldc > N"""
    _check(dsvgp, gpu_device, "alpha ldc", 601, 600, 1300, alpha=-1.0, ldc=608)


def test_c_zeroed(dsvgp, gpu_device):
    """the launcher makes no clear: the caller's zeros are what the units accumulate onto"""
    _check(dsvgp, gpu_device, "C_ZEROED", 640, 640, 1024, extra=C_ZEROED, fill=0.0)


def test_upper_undef(dsvgp, gpu_device):
    """nobody reads the strict upper triangle: only the lower one is compared"""
    _check(dsvgp, gpu_device, "UPPER_UNDEF", 640, 640, 1024, extra=UPPER_UNDEF, lower_only=True)


def test_fallback(dsvgp, gpu_device):
    """products the kernel does not take stay on the old path under 1 (and are refused under 2)"""
    L = dsvgp._lib
    dev = gpu_device
    # M = 300: below the fp32 MFMA kernels' smallest product
    M, N, K = 300, 300, 1024
    P, ref, absprod = _operands(dev, M, N, K)
    bound = (K + (K + 31) // 32 + 2) * 2.0 ** -24 * absprod
    C, _ = _run(dsvgp, dev, 1, P, M, N, K)
    assert ((C.double() - ref).abs() / bound).max().item() <= 1.0
    with pytest.raises(L.DsvgpError):
        _run(dsvgp, dev, 2, P, M, N, K)
    # an m-contiguous right operand: OUT_LOWER without TRANS_B
    M = N = 640
    P, ref, absprod = _operands(dev, M, N, K)
    bound = (K + (K + 31) // 32 + 2) * 2.0 ** -24 * absprod
    Bt = P[:N].t().contiguous()                              # [K, N]
    C, _ = _run(dsvgp, dev, 1, P, M, N, K, trans_b=False, B=Bt)
    assert ((C.double() - ref).abs() / bound).max().item() <= 1.0
    assert (C.triu(1) == 0).all()
    with pytest.raises(L.DsvgpError):
        _run(dsvgp, dev, 2, P, M, N, K, trans_b=False, B=Bt)


def test_in_the_step(dsvgp, gpu_device):
    """the one-call ELBO step at M' = 600, B' = 1536 with its Gram product on the new kernel against the same step on the old launch:
    two orders of the same fp32 atomics (the tolerances of test_one_call_step_equals_the_piecewise_step); twice on the same plan"""
    import dsvgp_oracle as O
    from test_gpu_step import make_problem, relmax
    N, d, M, p, B = 3000, 5, 200, 2, 512
    P, x, y, D, nd = make_problem(N, d, M, p, B, seed=N + d + 1)
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    xd, yd, Dd = x.to(gpu_device), y.to(gpu_device), D.to(gpu_device)
    with gram_mode(0):
        ref = dsvgp.ElboEngine(gpu_device)
        l0, g0, mu0, _ = ref.loss_and_grads(Pg, xd, yd, Dd, nd)
        torch.cuda.synchronize()
        assert ref.c_step_used
    with gram_mode(1):
        eng = dsvgp.ElboEngine(gpu_device)
        for call in range(2):                                # the second call runs on the same plan / workspace
            l1, g1, mu1, _ = eng.loss_and_grads(Pg, xd, yd, Dd, nd)
            torch.cuda.synchronize()
            assert eng.c_step_used
            errs = {k: relmax(g1[k], g0[k]) for k in O.PARAM_NAMES if g0[k].numel()}
            print("[gemm32 gram] step call %d: loss %.3e mean %.3e grads %s" % (call, abs(l1.item() - l0.item()) / abs(l0.item()),
                                                                                relmax(mu1, mu0), ", ".join("%s %.1e" % kv for kv in errs.items())))
            assert abs(l1.item() - l0.item()) < 4e-6 * abs(l0.item()), (call, l1.item(), l0.item())
            assert relmax(mu1, mu0) < 4e-6, (call, relmax(mu1, mu0))
            for k, e in errs.items():
                assert e < 5e-5, (call, k, e)
            assert g1["chol_variational_covar"].triu(1).abs().max().item() == 0.0
