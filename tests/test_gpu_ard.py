"""ARD lengthscales on the GPU: the entries of csrc/assemble_ard.hip (pack, prior diagonal, kernel backward), the kernel module's
``ard_num_dims``, the engine's step and predictions on ``raw_lengthscale`` [1, d] and the harness keyword, against the float64 yardstick
of tests/_ard_yardstick.py.

Inputs: X ~ U[0, 1]^d, ell_k = 0.4 sqrt(d) (0.5 + k / (d - 1)) (a 3x spread: every d_ell[k] is distinct, nothing compares zeros), generic
directions.  Tolerances are the project's for the same quantities: kernel forward 2e-5 of max (KTOL, tests/test_gpu_rect_predict.py),
kernel backward 2e-4 (KBWD_TOL, tests/test_gpu_rect_train.py), step loss 2e-5, mean and variance 2e-4, gradients 2e-3 (``_check_step`` of
tests/test_gpu_rect_train.py), predictions TOL / CTOL of tests/test_gpu_rect_predict.py; each is a max-norm relative to the quantity's largest entry, d_ell held as
one vector.  Measured errors are printed as [parity] lines."""
import functools
import math

import pytest
import torch

import dsvgp_oracle as O
from _ard_yardstick import ard_elbo, ard_kernel, ard_lengthscales, ard_predictive
from test_gpu_rect_train import _check_step, _raw, _report, relmax

gpu = pytest.mark.gpu
KTOL, KBWD_TOL = 2e-5, 2e-4
S = 1.3

#        n1  p1  n2  p2   d
SHAPES = [(37, 2, 41, 3, 5),        # 111 x 164: several tiles, ragged last ones, d not a multiple of 4
          (37, 2, 130, 3, 5),       # the first shape with n2 grown until the contraction splits: 520 columns, 3 slabs
          (20, 5, 45, 5, 20),       # the C4 micro-block
          (11, 2, 23, 1, 200),      # wide: several K chunks
          (9, 0, 30, 2, 7),         # p1 = 0: null vnorm1 / d_v1
          (12, 3, 30, 0, 6)]        # value-only data
SYM = (24, 2, 24, 2, 5)             # symmetric, same pack, symmetric G
IDS = ["%dx%d-%dx%d-d%d" % s for s in SHAPES]
SPLIT = SHAPES[1]


@functools.lru_cache(maxsize=None)
def _case(n1, p1, n2, p2, d, symmetric=False, equal=False):
    """(x1, v1, x2, v2, ell fp64, G fp64, K fp64, autograd gradients of sum(G * S K) w.r.t. x1, v1, ell, S): once per shape, shared"""
    g = torch.Generator().manual_seed(n1 + 31 * n2 + 7 * p1 + 3 * p2 + d)
    x1, v1 = torch.rand(n1, d, generator=g), torch.randn(n1 * p1, d, generator=g)
    x2, v2 = torch.rand(n2, d, generator=g), torch.randn(n2 * p2, d, generator=g)
    G = torch.randn(n1 * (p1 + 1), n2 * (p2 + 1), generator=g, dtype=torch.float64)
    if symmetric:
        x2, v2, G = x1, v1, G + G.t()
    ell = torch.full((d,), 0.4 * math.sqrt(d), dtype=torch.float64) if equal else ard_lengthscales(d)
    x1r, v1r = x1.double().requires_grad_(True), v1.double().requires_grad_(True)
    ellr, sr = ell.clone().requires_grad_(True), torch.tensor(S, dtype=torch.float64, requires_grad=True)
    K = ard_kernel(x1r, v1r, p1, x1r, v1r, p1, ellr) if symmetric else ard_kernel(x1r, v1r, p1, x2.double(), v2.double(), p2, ellr)
    (sr * K * G).sum().backward()
    gv = v1r.grad if p1 else torch.zeros(0, d, dtype=torch.float64)
    return x1, v1, x2, v2, ell, G, K.detach(), (x1r.grad, gv, ellr.grad, sr.grad.item())


def _packs(dsvgp, dev, x1, v1, p1, x2, v2, p2, ell):
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    hyp = torch.tensor([1.0, S, 0.1, 0.0], dtype=torch.float32, device=dev)
    elld = ell.float().to(dev)
    x1d = x1.to(dev).contiguous()
    center = ops.column_mean(ctx, x1d)
    pk1 = ops.pack_points_ard(ctx, x1d, v1.to(dev).contiguous() if p1 else None, p1, elld, center)
    pk2 = ops.pack_points_ard(ctx, x2.to(dev).contiguous(), v2.to(dev).contiguous() if p2 else None, p2, elld, center)
    return ops, ctx, hyp, elld, pk1, pk2


def _outputs(n1, p1, d, dev):
    return (torch.zeros(n1, d, device=dev), torch.zeros(max(n1 * p1, 1), d, device=dev), torch.zeros(d, device=dev),
            torch.zeros(4, device=dev))


def test_one_shape_splits_the_contraction(dsvgp):
    slabs = dsvgp._ops.kernel_bwd_ard_slabs
    assert slabs(*SHAPES[0]) == 1 and slabs(*SYM) == 1          # one slab: the plain case
    assert slabs(*SPLIT) == 3 and slabs(*SHAPES[2]) == 2        # 520 and 270 columns: pieces of at least 256


@gpu
def test_hyp_forward_and_backward_ard(dsvgp, gpu_device):
    dev = gpu_device
    ops, ctx = dsvgp._ops, dsvgp._ops.Context.get(dev)
    d = 300                                                     # more than one workgroup
    g = torch.Generator().manual_seed(1)
    rl, rs, rn = torch.randn(1, d, generator=g), torch.tensor([0.3]), torch.tensor([-1.2])
    ell, hyp = ops.hyp_forward_ard(ctx, rl.to(dev), rs.to(dev), rn.to(dev))
    sp = torch.nn.functional.softplus
    assert relmax(ell, sp(rl.double()).reshape(-1)) < 1e-6
    assert hyp[0].item() == 1.0 and hyp[3].item() == 0.0
    assert abs(hyp[1].item() - sp(rs.double()).item()) < 1e-6 and abs(hyp[2].item() - sp(rn.double()).item() - 1e-4) < 1e-6
    d_ell, dh = torch.randn(d, generator=g), torch.tensor([123.0, 0.7, -0.4, 0.0])
    drl, drs, drn = torch.ones(1, d, device=dev), torch.ones(1, device=dev), torch.ones(1, device=dev)
    ops.hyp_backward_ard(ctx, rl.to(dev), rs.to(dev), rn.to(dev), d_ell.to(dev), dh.to(dev), drl, drs, drn)
    assert relmax(drl.reshape(-1) - 1, d_ell.double() * torch.sigmoid(rl.double()).reshape(-1)) < 1e-5       # += ; d_hyp[0] is not read
    assert abs(drs.item() - 1 - 0.7 * torch.sigmoid(rs.double()).item()) < 1e-6
    assert abs(drn.item() - 1 + 0.4 * torch.sigmoid(rn.double()).item()) < 1e-6


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_matches_the_yardstick(dsvgp, gpu_device, shape):
    n1, p1, n2, p2, d = shape
    x1, v1, x2, v2, ell, _, K, _ = _case(*shape)
    ops, ctx, hyp, elld, pk1, pk2 = _packs(dsvgp, gpu_device, x1, v1, p1, x2, v2, p2, ell)
    out = ops.kernel_fwd_rect(ctx, pk1, n1, p1, pk2, n2, p2, d, hyp)
    errs = {"rect": relmax(out, S * K)}
    if p1 == p2:
        errs["wide"] = relmax(ops.kernel_fwd_wide(ctx, pk1, n1, pk2, n2, d, p1, hyp, jitter=0.0, dtype=torch.float32), S * K)
    _report("ARD forward d=%d p1=%d p2=%d %dx%d" % (d, p1, p2, n1, n2), errs)
    assert max(errs.values()) < KTOL, errs


@gpu
def test_symmetric_forward_is_exact_on_the_diagonal_blocks(dsvgp, gpu_device):
    """K_ZZ through the wide forward (double output, jitter): r == 0 stays exact, so the diagonal is s + jitter, s |v~|^2 + jitter"""
    n, p, _, _, d = SYM
    x, v, _, _, ell, _, K, _ = _case(*SYM, symmetric=True)
    ops, ctx, hyp, elld, pk, _ = _packs(dsvgp, gpu_device, x, v, p, x, v, p, ell)
    out = ops.kernel_fwd_wide(ctx, pk, n, pk, n, d, p, hyp, jitter=1e-3, dtype=torch.float64)
    ref = S * K + 1e-3 * torch.eye(K.shape[0], dtype=torch.float64)
    diag = ops.kernel_diag_ard(ctx, pk, n, p, d, hyp)
    errs = {"K_ZZ": relmax(out, ref), "diag": relmax(diag, S * K.diagonal()),
            "diag of K_ZZ vs kernel_diag_ard": relmax(out.diagonal() - 1e-3, diag)}
    _report("ARD symmetric forward", errs)
    assert max(errs.values()) < KTOL, errs
    exact = (torch.tensor(S, dtype=torch.float32) + torch.tensor(1e-3, dtype=torch.float32)).double()      # the fp32 sum, widened
    assert torch.equal(out.diagonal()[::p + 1].cpu(), exact.expand(n))


@gpu
@pytest.mark.parametrize("n,p,d", [(41, 3, 5), (23, 1, 200), (30, 0, 6)])
def test_kernel_diag_ard_and_its_backward(dsvgp, gpu_device, n, p, d):
    dev = gpu_device
    g = torch.Generator().manual_seed(n + d)
    x, v, gbar = torch.rand(n, d, generator=g), torch.randn(n * p, d, generator=g), torch.randn(n * (p + 1), generator=g, dtype=torch.float64)
    ell = ard_lengthscales(d)
    ellr, sr = ell.clone().requires_grad_(True), torch.tensor(S, dtype=torch.float64, requires_grad=True)
    ref = sr * ard_kernel(x.double(), v.double(), p, x.double(), v.double(), p, ellr).diagonal()
    (ref * gbar).sum().backward()
    ops, ctx, hyp, elld, pk, _ = _packs(dsvgp, dev, x, v, p, x, v, p, ell)
    out = ops.kernel_diag_ard(ctx, pk, n, p, d, hyp)
    d_ell, d_hyp = torch.zeros(d, device=dev), torch.zeros(4, device=dev)
    ops.kernel_diag_ard_bwd(ctx, pk, n, p, d, elld, hyp, out, gbar.float().to(dev), d_ell, d_hyp)
    errs = {"diag": relmax(out, ref.detach()), "d_s": abs(d_hyp[1].item() - sr.grad.item()) / max(1.0, abs(sr.grad.item()))}
    if p:
        errs["d_ell"] = relmax(d_ell, ellr.grad)
    else:
        assert d_ell.abs().max().item() == 0.0
    _report("kernel_diag_ard n=%d p=%d d=%d" % (n, p, d), errs)
    assert errs["diag"] < KTOL and errs["d_s"] < KBWD_TOL and errs.get("d_ell", 0.0) < KBWD_TOL, errs
    again_l, again_h = torch.zeros(d, device=dev), torch.zeros(4, device=dev)
    ops.kernel_diag_ard_bwd(ctx, pk, n, p, d, elld, hyp, out, gbar.float().to(dev), again_l, again_h)
    assert torch.equal(again_l, d_ell) and torch.equal(again_h, d_hyp) and d_hyp[0].item() == 0.0


def _check_bwd(tag, outs, refs, p1):
    dx, dv, dl, dh = outs
    gx, gv, gl, gs = refs
    errs = {"d_x1": relmax(dx, gx), "d_ell": relmax(dl, gl), "d_s": abs(dh[1].item() - gs) / max(1.0, abs(gs))}
    if p1 > 0:
        errs["d_v1"] = relmax(dv[:gv.shape[0]], gv)
    _report(tag, errs)
    assert dh[0].item() == 0.0 and dh[2].item() == 0.0 and dh[3].item() == 0.0       # the scalar lengthscale slot is not written
    for k, e in errs.items():
        assert e < KBWD_TOL, (tag, k, e)


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernel_bwd_ard_matches_autograd(dsvgp, gpu_device, shape):
    dev = gpu_device
    n1, p1, n2, p2, d = shape
    x1, v1, x2, v2, ell, G, _, refs = _case(*shape)
    ops, ctx, hyp, elld, pk1, pk2 = _packs(dsvgp, dev, x1, v1, p1, x2, v2, p2, ell)
    for Gd, up in ((G.to(dev), "double"), (G.float().to(dev), "float")):
        outs = _outputs(n1, p1, d, dev)
        ops.kernel_bwd_ard(ctx, Gd, pk1, n1, p1, pk2, n2, p2, d, elld, hyp, False, *outs)
        _check_bwd("kernel_bwd_ard d=%d p1=%d p2=%d %dx%d %s upstream" % (d, p1, p2, n1, n2, up), outs, refs, p1)


@gpu
def test_kernel_bwd_ard_symmetric_matches_autograd_of_the_symmetric_kernel(dsvgp, gpu_device):
    dev = gpu_device
    n, p, _, _, d = SYM
    x, v, _, _, ell, G, _, refs = _case(*SYM, symmetric=True)
    ops, ctx, hyp, elld, pk, _ = _packs(dsvgp, dev, x, v, p, x, v, p, ell)
    for Gd, up in ((G.to(dev), "double"), (G.float().to(dev), "float")):
        outs = _outputs(n, p, d, dev)
        ops.kernel_bwd_ard(ctx, Gd, pk, n, p, pk, n, p, d, elld, hyp, True, *outs)
        _check_bwd("kernel_bwd_ard symmetric %s upstream" % up, outs, refs, p)


@gpu
@pytest.mark.parametrize("shape", [SHAPES[0], SPLIT, SHAPES[3]], ids=[IDS[0], IDS[1], IDS[3]])
def test_kernel_bwd_ard_accumulates_takes_a_strided_upstream_and_is_reproducible(dsvgp, gpu_device, shape):
    dev = gpu_device
    n1, p1, n2, p2, d = shape
    x1, v1, x2, v2, ell, G, _, _ = _case(*shape)
    ops, ctx, hyp, elld, pk1, pk2 = _packs(dsvgp, dev, x1, v1, p1, x2, v2, p2, ell)
    Gf = G.float().to(dev)

    def run(Gd, out=None, with_ell=True):
        out = out or _outputs(n1, p1, d, dev)
        ops.kernel_bwd_ard(ctx, Gd, pk1, n1, p1, pk2, n2, p2, d, elld, hyp, False, out[0], out[1], out[2] if with_ell else None, out[3])
        return out

    a, b = run(Gf), run(Gf)
    assert all(torch.equal(u, v) for u, v in zip(a, b))                     # two identical calls on zeroed outputs
    assert a[0].abs().max().item() > 0 and a[2].abs().min().item() > 0 and a[3][1].abs().item() > 0
    twice = run(Gf, run(Gf))                                               # += : a second call into the same outputs doubles them
    assert all(torch.equal(t, 2 * u) for t, u in zip(twice, a))
    wide = torch.full((Gf.shape[0], Gf.shape[1] + 5), float("nan"), device=dev)      # a view with ldg > n2 q2; nothing outside it is read
    wide[:, 2:2 + Gf.shape[1]] = Gf
    c = run(wide[:, 2:2 + Gf.shape[1]])
    assert all(torch.equal(u, v) for u, v in zip(a, c))
    G64 = torch.full((Gf.shape[0], Gf.shape[1] + 3), float("nan"), device=dev, dtype=torch.float64)
    G64[:, 1:1 + Gf.shape[1]] = G.to(dev)
    e, f = run(G.to(dev)), run(G64[:, 1:1 + Gf.shape[1]])
    assert all(torch.equal(u, v) for u, v in zip(e, f))
    n = run(Gf, with_ell=False)                                            # d_ell = NULL: the other outputs bitwise unchanged
    assert torch.equal(n[0], a[0]) and torch.equal(n[1], a[1]) and torch.equal(n[3], a[3]) and n[2].abs().max().item() == 0.0


@gpu
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3], SHAPES[0]], ids=[IDS[2], IDS[3], IDS[0]])
def test_equal_lengthscales_agree_with_the_scalar_path(dsvgp, gpu_device, shape):
    """a cross-check against the existing code (the yardstick stays the float64 one): ell_k = ell"""
    dev = gpu_device
    n1, p1, n2, p2, d = shape
    x1, v1, x2, v2, ell, G, K, refs = _case(*shape, equal=True)
    ops, ctx, hyp, elld, pk1, pk2 = _packs(dsvgp, dev, x1, v1, p1, x2, v2, p2, ell)
    hyp_s = torch.tensor([ell[0].item(), S, 0.1, 0.0], dtype=torch.float32, device=dev)
    center = ops.column_mean(ctx, x1.to(dev).contiguous())
    sk1 = ops.pack_points(ctx, x1.to(dev).contiguous(), v1.to(dev).contiguous(), p1, hyp_s, center)
    sk2 = ops.pack_points(ctx, x2.to(dev).contiguous(), v2.to(dev).contiguous(), p2, hyp_s, center)
    f_ard = ops.kernel_fwd_rect(ctx, pk1, n1, p1, pk2, n2, p2, d, hyp)
    f_sc = ops.kernel_fwd_rect(ctx, sk1, n1, p1, sk2, n2, p2, d, hyp_s)
    Gd = G.float().to(dev)
    outs = _outputs(n1, p1, d, dev)
    ops.kernel_bwd_ard(ctx, Gd, pk1, n1, p1, pk2, n2, p2, d, elld, hyp, False, *outs)
    dx, dv, dh = torch.zeros(n1, d, device=dev), torch.zeros(n1 * p1, d, device=dev), torch.zeros(4, device=dev)
    ops.kernel_bwd_rect(ctx, Gd, sk1, n1, p1, sk2, n2, p2, d, hyp_s, dx, dv, dh)
    errs = {"forward": relmax(f_ard, f_sc), "d_x1": relmax(outs[0], dx), "d_v1": relmax(outs[1][:n1 * p1], dv),
            "sum d_ell": abs(outs[2].double().sum().item() - dh[0].item()) / max(1.0, abs(dh[0].item())),
            "d_s": abs(outs[3][1].item() - dh[1].item()) / max(1.0, abs(dh[1].item()))}
    _report("ARD at equal lengthscales vs the scalar path d=%d" % d, errs)
    assert errs.pop("forward") < 2 * KTOL
    assert max(errs.values()) < KBWD_TOL, errs
    _check_bwd("ARD at equal lengthscales vs the yardstick d=%d" % d, outs, refs, p1)


@gpu
@pytest.mark.parametrize("n1,n2,p,d", [(13, 17, 2, 5), (7, 9, 1, 120)])
def test_kernel_module_with_ard_reaches_all_five_inputs(dsvgp, gpu_device, n1, n2, p, d):
    from dsvgp_amd.RBFKernelDirectionalGrad import RBFKernelDirectionalGrad
    dev = gpu_device
    g = torch.Generator().manual_seed(n1 + d)
    x1, x2 = torch.rand(n1, d, generator=g), torch.rand(n2, d, generator=g)
    v1, v2 = torch.randn(n1 * p, d, generator=g), torch.randn(n2 * p, d, generator=g)
    G = torch.randn(n1 * (p + 1), n2 * (p + 1), generator=g, dtype=torch.float64)
    ell = ard_lengthscales(d)
    ins64 = [t.double().requires_grad_(True) for t in (x1, x2, v1, v2, ell)]
    K64 = ard_kernel(ins64[0], ins64[2], p, ins64[1], ins64[3], p, ins64[4])
    ref = torch.autograd.grad((K64 * G).sum(), ins64)
    kern = RBFKernelDirectionalGrad(ard_num_dims=d).to(dev)
    kern.lengthscale = ell.float()
    assert kern.lengthscale.shape == (1, d) and relmax(kern.lengthscale.reshape(-1), ell) < 1e-6
    ins = [t.to(dev).requires_grad_(True) for t in (x1, x2, v1, v2)]
    K = kern(ins[0], ins[1], v1=ins[2], v2=ins[3])
    got = torch.autograd.grad((K * G.float().to(dev)).sum(), ins + [kern.raw_lengthscale])
    sig = torch.sigmoid(kern.raw_lengthscale.detach().double().cpu()).reshape(-1)
    errs = {"K": relmax(K.detach(), K64.detach())}
    for name, a, b in zip(("d_x1", "d_x2", "d_v1", "d_v2"), got, ref):
        errs[name] = relmax(a, b)
    errs["d_raw_lengthscale"] = relmax(got[4].reshape(-1), ref[4] * sig)
    _report("RBFKernelDirectionalGrad(ard_num_dims=%d)" % d, errs)
    assert got[4].shape == (1, d)
    assert errs.pop("K") < KTOL and max(errs.values()) < KBWD_TOL, errs
    xs, vs = x1.to(dev), v1.to(dev)
    diag = kern(xs, xs, diag=True, v1=vs, v2=vs)
    Kd = ard_kernel(x1.double(), v1.double(), p, x1.double(), v1.double(), p, ell).diagonal()
    assert relmax(diag, Kd) < KTOL
    with pytest.raises(ValueError, match="ARD lengthscales"):
        kern(xs.double(), xs.double(), v1=vs.double(), v2=vs.double())


# ------------------------------------------------------------------ the engine: step and predictions against the yardstick
TOL, CTOL = 2e-4, 5e-4              # mean / variance and covariance of a prediction (tests/test_gpu_rect_predict.py)
#          N    d    M  p pd   B
STEPS = [(400, 3, 16, 2, 2, 96),
         (400, 3, 16, 2, 0, 96),
         (300, 20, 10, 5, 1, 48),
         (300, 120, 8, 2, 1, 32)]           # wide inputs: several K chunks
STEP_IDS = ["N%d-d%d-M%d-p%d-pd%d-B%d" % s for s in STEPS]


@functools.lru_cache(maxsize=None)
def _problem(N, d, M, p, pd, B):
    """(params fp32 with raw_lengthscale [1, d], x, y [B (pd + 1)], data directions [B pd, d], num_data): once per shape, shared"""
    from test_gpu_step import make_problem
    P, x, _, _, nd = make_problem(N, d, M, p, B, seed=N + d + pd)
    P["raw_lengthscale"] = torch.tensor([[_raw(v) for v in ard_lengthscales(d).tolist()]], dtype=torch.float32)
    g = torch.Generator().manual_seed(17 + pd)
    cols = sorted((torch.randperm(d, generator=g)[:pd] + 1).tolist())
    y = O.testfun(x)[:, [0] + cols].reshape(-1).contiguous()
    D = (torch.eye(d)[[c - 1 for c in cols]] + 0.1 * torch.randn(pd, d, generator=g)).repeat(B, 1)        # generic, not one-hot
    return P, x, y, D, nd


@functools.lru_cache(maxsize=None)
def _reference(shape, mll):
    P, x, y, D, nd = _problem(*shape)
    return ard_elbo({k: v.double() for k, v in P.items()}, x.double(), y.double(), D.double(), shape[4], nd, mll)


@gpu
@pytest.mark.parametrize("shape", STEPS, ids=STEP_IDS)
@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
def test_step_matches_the_yardstick(dsvgp, gpu_device, shape, mll):
    N, d, M, p, pd, B = shape
    P, x, y, D, nd = _problem(*shape)
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    out = eng.loss_and_grads(Pg, x.to(dev), y.to(dev), D.to(dev) if pd else None, nd, mll)
    torch.cuda.synchronize()
    assert eng.c_step_used is False and eng._train_pd is None and eng._ard is False
    assert out[2].shape == (B * (pd + 1),) and out[1]["raw_lengthscale"].shape == (1, d)
    _check_step("ARD step N=%d d=%d M=%d p=%d pd=%d B=%d %s" % (N, d, M, p, pd, B, mll), out, _reference(shape, mll), p, False)
    with pytest.raises(ValueError, match=r"B\*\(p\+1\)=%d$" % (B * (pd + 1))):
        eng.loss_and_grads(Pg, x.to(dev), torch.zeros(B * (pd + 1) + 1, device=dev), D.to(dev) if pd else None, nd, mll)


@gpu
@pytest.mark.parametrize("shape", [STEPS[0], STEPS[3]], ids=[STEP_IDS[0], STEP_IDS[3]])
def test_predict_and_predict_joint_match_the_yardstick(dsvgp, gpu_device, shape):
    N, d, M, p, pd, B = shape
    P, x, _, D, _ = _problem(*shape)
    P64 = {k: v.double() for k, v in P.items()}
    mu_ref, Sig_ref = ard_predictive(P64, x.double(), D.double(), pd)
    noise = (torch.nn.functional.softplus(P64["raw_noise"]).reshape(()) + O.NOISE_FLOOR).item()
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    Dg = D.to(dev) if pd else None
    mu, varn = eng.predict(Pg, x.to(dev), Dg)
    mu_c, varn_c = eng.predict(Pg, x.to(dev), Dg, cache=True)
    mu_h, varn_h = eng.predict(Pg, x.to(dev), Dg, cache=True)             # the evaluation cache: the factor and the lengthscales kept
    mu_j, Sigma = eng.predict_joint(Pg, x.to(dev), Dg)
    n = B * (pd + 1)
    errs = {"mean": relmax(mu, mu_ref), "variance": relmax(varn, Sig_ref.diagonal() + noise), "joint mean": relmax(mu_j, mu_ref),
            "covariance": relmax(Sigma, Sig_ref + noise * torch.eye(n, dtype=torch.float64)),
            "diagonal vs variance": relmax(Sigma.diagonal(), varn), "cached mean": relmax(mu_h, mu_ref),
            "cached variance": relmax(varn_h, Sig_ref.diagonal() + noise)}
    _report("ARD predict d=%d M=%d p=%d pd=%d B=%d" % (d, M, p, pd, B), errs)
    assert mu.shape == varn.shape == mu_j.shape == (n,) and Sigma.shape == (n, n) and eng._ard is False
    assert torch.equal(mu_c, mu) and torch.equal(varn_c, varn)
    assert errs.pop("covariance") < CTOL and max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ model and harness
@gpu
def test_harness_learns_which_dimension_matters(dsvgp, gpu_device):
    """f(x) = sin(6 x_0) with its gradient on U[0, 1]^2: d = 2, N = 400, M = 16, p = 2, full-gradient data, 30 epochs of 4 minibatches of
    100 (120 Adam steps, learning rate 0.05).  The float64 yardstick (``ard_forward``) under torch.optim.Adam on the CPU with this schedule:
    mean loss of the first 10 steps 5.019, of the last 10 steps 1.236; lengthscales (0.353, 1.647), ratio 4.66 (after 200 steps: 0.443,
    ratio 6.38).  Asked here: the loss falls and the irrelevant dimension relaxes."""
    from torch.utils.data import TensorDataset
    from dsvgp_amd import directional_vi
    torch.manual_seed(0)
    n, dim = 400, 2
    X = torch.rand(n, dim)
    Y = torch.stack([torch.sin(6 * X[:, 0]), 6 * torch.cos(6 * X[:, 0]), torch.zeros(n)], 1)
    kw = dict(num_inducing=16, num_directions=2, minibatch_size=100, minibatch_dim=2, num_epochs=30, learning_rate_hypers=0.05, seed=0,
              ard_num_dims=2)
    loop = directional_vi.setup_training(TensorDataset(X, Y), **kw)
    assert loop.model.covar_module.base_kernel.raw_lengthscale.shape == (1, 2)
    losses = []
    for _ in range(30):
        perm = loop.epoch_permutation()
        for start in range(0, n, 100):
            loss, output, y_batch = loop.step(perm[start:start + 100])
            assert loop.model.engine.c_step_used is False
            losses.append(loss.item())
    loop.finish()
    ell = loop.model.covar_module.base_kernel.lengthscale.detach().cpu()
    first, last = sum(losses[:10]) / 10, sum(losses[-10:]) / 10
    print("[parity] ARD harness: mean loss of the first 10 steps %.4f, of the last 10 %.4f, lengthscales (%.4f, %.4f), ratio %.3f"
          % (first, last, ell[0, 0].item(), ell[0, 1].item(), (ell[0, 1] / ell[0, 0]).item()))
    assert ell.shape == (1, 2) and all(math.isfinite(l) for l in losses)
    assert last < first
    assert ell[0, 1].item() > ell[0, 0].item()
    # train_gp itself takes the keyword; the state round-trips; eval_gp runs
    model, likelihood = dsvgp.train_gp(TensorDataset(X, Y), tqdm=False, verbose=False, max_steps=3, **kw)
    assert model.covar_module.base_kernel.lengthscale.shape == (1, 2)
    state = model.state_dict()
    key = [k for k in state if k.endswith("raw_lengthscale")]
    assert len(key) == 1 and state[key[0]].shape == (1, 2)
    fresh = directional_vi.setup_training(TensorDataset(X, Y), **kw).model
    assert not torch.equal(fresh.covar_module.base_kernel.raw_lengthscale, model.covar_module.base_kernel.raw_lengthscale)
    fresh.load_state_dict(state)
    assert torch.equal(fresh.covar_module.base_kernel.raw_lengthscale, model.covar_module.base_kernel.raw_lengthscale)
    scalar = directional_vi.setup_training(TensorDataset(X, Y), **dict(kw, ard_num_dims=None)).model
    assert scalar.covar_module.base_kernel.raw_lengthscale.shape == (1, 1)
    with pytest.raises(RuntimeError):
        scalar.load_state_dict(state)                                      # a scalar-lengthscale model does not take the [1, 2] entry
    assert dsvgp.GPModel(torch.rand(16, 2), torch.eye(2).repeat(16, 1), 2, ard_num_dims=2).covar_module.base_kernel.ard_num_dims == 2
    test = TensorDataset(torch.rand(50, 2), torch.zeros(50, 3))
    means, variances = dsvgp.eval_gp(test, loop.model, loop.likelihood, num_directions=2, minibatch_size=25, minibatch_dim=2)
    assert means.shape == variances.shape == (150,) and bool(torch.isfinite(means).all()) and bool((variances > 0).all())


# ------------------------------------------------------------------ refusals
@gpu
def test_what_is_not_built_for_ard_raises_and_the_scalar_model_is_untouched(dsvgp, gpu_device):
    from dsvgp_amd._step64 import ElboEngine64
    dev = gpu_device
    shape = STEPS[0]
    N, d, M, p, pd, B = shape
    P, x, y, D, nd = _problem(*shape)
    Pg = {k: v.to(dev) for k, v in P.items()}
    xg, yg, Dg = x.to(dev), y.to(dev), D.to(dev)
    word = "ARD lengthscales"
    with pytest.raises(ValueError, match=word):                            # the Gram fast path
        dsvgp.ElboEngine(dev).loss_and_grads(Pg, xg, yg, Dg, nd, "ELBO", fast=True)

    class _World:
        rank, world = 0, 2

    for attr, val in (("whitening", "ciq"), ("shared_directions", True), ("capture_mode", True), ("deterministic", True),
                      ("data_outputs", "values"), ("collective", _World())):
        eng = dsvgp.ElboEngine(dev)
        setattr(eng, attr, val)
        with pytest.raises(ValueError, match=word):
            eng.loss_and_grads(Pg, xg, yg, Dg, nd)
        if attr != "deterministic":
            with pytest.raises(ValueError, match=word):
                eng.predict(Pg, xg, Dg)
    from test_ngd import make_ngd_problem
    Pn = {k: v.to(dev) for k, v in make_ngd_problem(N, d, M, p, B)[0].items()}
    Pn["raw_lengthscale"] = Pg["raw_lengthscale"]
    with pytest.raises(ValueError, match=word):
        dsvgp.ElboEngine(dev).loss_and_grads(Pn, xg, yg, Dg, nd)
    P64 = {k: v.double() for k, v in Pg.items()}
    with pytest.raises(ValueError, match=word):
        ElboEngine64(dev).loss_and_grads(P64, xg.double(), yg.double(), Dg.double(), nd)
    with pytest.raises(ValueError, match=word):
        ElboEngine64(dev).predict(P64, xg.double(), Dg.double())
    eng = dsvgp.ElboEngine(dev)
    for call in (lambda: eng.mean_predictor(Pg), lambda: eng.predict_blocks(Pg, xg, Dg), lambda: eng.sample_paths(Pg, 2, num_features=16),
                 lambda: eng.prior_moments(Pg), lambda: eng.whiten_legacy(Pg)):
        with pytest.raises(ValueError, match=word):
            call()
    with pytest.raises(ValueError, match="one entry per input dimension"):
        eng.predict(dict(Pg, raw_lengthscale=Pg["raw_lengthscale"][:, :2].contiguous()), xg, Dg)
    # a one-element raw_lengthscale still takes the one-call step
    from test_gpu_step import make_problem
    Ps, xs, ys, Ds, nds = make_problem(400, 5, 24, 2, 96, seed=3)
    eng = dsvgp.ElboEngine(dev)
    eng.loss_and_grads({k: v.to(dev) for k, v in Ps.items()}, xs.to(dev), ys.to(dev), Ds.to(dev), nds)
    assert Ps["raw_lengthscale"].numel() == 1 and eng.c_step_used is True


@gpu
def test_c_entry_refusals(dsvgp, gpu_device):
    """dsvgp_kernel_bwd_ard: a leading dimension that is too small, a misaligned pack, p = 96, null pointers, d = 0, symmetric on unequal
    sides; the optional pointers; empty problems return 0; refused calls touch nothing"""
    import ctypes as C
    dev = gpu_device
    ops, lib = dsvgp._ops, dsvgp._lib.lib
    ctx = ops.Context.get(dev)
    n1, p1, n2, p2, d = 12, 2, 20, 0, 3
    g = torch.Generator().manual_seed(5)
    hyp = torch.tensor([1.0, 1.7, 0.1, 0.0], device=dev)
    ell = torch.tensor([0.5, 0.9, 1.4], device=dev)
    pz = ops.pack_points_ard(ctx, torch.rand(n1, d, generator=g).to(dev), torch.randn(n1 * p1, d, generator=g).to(dev), p1, ell)
    px = ops.pack_points_ard(ctx, torch.rand(n2, d, generator=g).to(dev), None, p2, ell)
    G = torch.zeros(n1 * (p1 + 1), n2, device=dev)
    dx, dv, dl, dh = torch.zeros(n1, d, device=dev), torch.zeros(n1 * p1, d, device=dev), torch.zeros(d, device=dev), torch.zeros(4, device=dev)
    ws = torch.empty(ops.kernel_bwd_ard_workspace_bytes(n1, p1, n2, p2, d), dtype=torch.uint8, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def entry(n1=n1, p1=p1, n2=n2, p2=p2, d=d, ldg=n2, P1=pz[0].data_ptr(), vn=pz[2], dv_=dv, dl_=dl, ws_=ws, ell_=ell, sym=0, dx_=dx):
        return lib.dsvgp_kernel_bwd_ard(ctx.h, vp(G), ldg, 0, C.c_void_p(P1), vp(pz[1]), vp(vn), n1, p1, vp(px[0]), vp(px[1]), n2, p2, d,
                                        vp(ell_), vp(hyp), sym, vp(dx_), vp(dv_), vp(dl_), vp(dh), vp(ws_))

    assert entry() == 0
    assert entry(dl_=None) == 0 and entry(dv_=None, vn=None) == 0            # the optional outputs
    assert entry(ldg=n2 - 1) == -1 and entry(P1=pz[0].data_ptr() + 4) == -1 and entry(p1=96) == -1 and entry(p2=96) == -1
    assert entry(p1=-1) == -1 and entry(d=0) == -1 and entry(vn=None) == -1 and entry(ws_=None) == -1 and entry(ell_=None) == -1
    assert entry(dx_=None) == -1 and entry(sym=1) == -1                      # symmetric needs n1 == n2 and p1 == p2
    assert entry(n1=0) == 0 and entry(n2=0) == 0 and entry(n1=-1) == -1
    assert lib.dsvgp_pack_points_ard(ctx.h, vp(dx), None, n1, d, 0, None, None, vp(pz[0]), vp(pz[1]), None) == -1          # no ell
    assert lib.dsvgp_pack_points_ard(ctx.h, vp(dx), None, n1, d, 96, vp(ell), None, vp(pz[0]), vp(pz[1]), None) == -1
    assert lib.dsvgp_kernel_diag_ard(ctx.h, None, n1, p1, d, vp(hyp), vp(dh)) == -1
    assert lib.dsvgp_hyp_forward_ard(ctx.h, vp(ell), 0, vp(hyp), vp(hyp), vp(dl), vp(dh)) == -1
    torch.cuda.synchronize()
    assert all(t.abs().max().item() == 0.0 for t in (dx, dv, dl, dh))        # (G = 0, and the refused calls touched nothing)
