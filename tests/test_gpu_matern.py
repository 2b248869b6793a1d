"""Matern-5/2 with directional derivatives on the GPU: the entries of csrc/assemble_matern.hip (forward, prior diagonal, kernel backward),
``Matern52KernelDirectionalGrad``, the engine with ``kernel = "matern52"`` (step and predictions) and the harness keyword, against the
float64 yardstick of tests/_matern_yardstick.py.

Inputs are the ARD tests': X ~ U[0, 1]^d, ell_k = 0.4 sqrt(d) (0.5 + k / (d - 1)), generic directions, S = 1.3.  Tolerances are the
project's for the same quantities: kernel forward 2e-5 of max (KTOL), kernel backward 2e-4 (KBWD_TOL, d_ell held as one vector), the step
``_check_step`` of tests/test_gpu_rect_train.py (loss 2e-5, mean / variance 2e-4, gradients 2e-3), predictions TOL / CTOL of
tests/test_gpu_rect_predict.py; each a max-norm relative to the quantity's largest entry.  Measured errors are printed as [parity] lines."""
import functools
import math

import pytest
import torch

import dsvgp_oracle as O
from _ard_yardstick import ard_lengthscales
from _matern_yardstick import matern_elbo, matern_kernel, matern_predictive
from test_gpu_ard import SHAPES, IDS, STEPS, STEP_IDS, SYM, _outputs, _packs, _problem
from test_gpu_rect_train import _check_step, _report, relmax

gpu = pytest.mark.gpu
KTOL, KBWD_TOL = 2e-5, 2e-4
TOL, CTOL = 2e-4, 5e-4
S = 1.3
ONE = (33, 0, 300, 0, 5)            # 1 x 1 micro-blocks: the forward's separate path; several column tiles
FWD_SHAPES = SHAPES + [ONE]
FWD_IDS = IDS + ["%dx%d-%dx%d-d%d" % ONE]
DUP = (37, 2, 41, 3, 5)             # three rows of x2 copied from x1 (other directions), three more at distance 1e-3 ell


@functools.lru_cache(maxsize=None)
def _case(n1, p1, n2, p2, d, symmetric=False, duplicates=False):
    """(x1, v1, x2, v2, ell fp64, G fp64, K fp64, autograd gradients of sum(G * S K) w.r.t. x1, v1, ell, S): once per shape, shared"""
    g = torch.Generator().manual_seed(n1 + 31 * n2 + 7 * p1 + 3 * p2 + d)
    x1, v1 = torch.rand(n1, d, generator=g), torch.randn(n1 * p1, d, generator=g)
    x2, v2 = torch.rand(n2, d, generator=g), torch.randn(n2 * p2, d, generator=g)
    G = torch.randn(n1 * (p1 + 1), n2 * (p2 + 1), generator=g, dtype=torch.float64)
    ell = ard_lengthscales(d)
    if symmetric:
        x2, v2, G = x1, v1, G + G.t()
    if duplicates:
        x2 = x2.clone()
        x2[[3, 17, 40]] = x1[[5, 0, 36]]                                       # exact copies, off the diagonal
        u = torch.randn(3, d, generator=g)
        x2[[8, 20, 33]] = x1[[7, 11, 30]] + (1e-3 * ell.float() * u / u.norm(dim=1, keepdim=True))      # distance 1e-3 in units of ell
    x1r, v1r = x1.double().requires_grad_(True), v1.double().requires_grad_(True)
    ellr, sr = ell.clone().requires_grad_(True), torch.tensor(S, dtype=torch.float64, requires_grad=True)
    K = matern_kernel(x1r, v1r, p1, x1r, v1r, p1, ellr) if symmetric else matern_kernel(x1r, v1r, p1, x2.double(), v2.double(), p2, ellr)
    (sr * K * G).sum().backward()
    gv = v1r.grad if p1 else torch.zeros(0, d, dtype=torch.float64)
    return x1, v1, x2, v2, ell, G, K.detach(), (x1r.grad, gv, ellr.grad, sr.grad.item())


# ------------------------------------------------------------------ forward
@gpu
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=FWD_IDS)
def test_forward_matches_the_yardstick(dsvgp, gpu_device, shape):
    n1, p1, n2, p2, d = shape
    x1, v1, x2, v2, ell, _, K, _ = _case(*shape)
    ops, ctx, hyp, elld, pk1, pk2 = _packs(dsvgp, gpu_device, x1, v1, p1, x2, v2, p2, ell)
    out = ops.kernel_fwd_matern52(ctx, pk1, n1, p1, pk2, n2, p2, d, hyp)
    errs = {"float": relmax(out, S * K)}
    again = ops.kernel_fwd_matern52(ctx, pk1, n1, p1, pk2, n2, p2, d, hyp)
    assert torch.equal(out, again)
    if p1 == p2:                        # double output with jitter on the global diagonal (the K_ZZ form of the call)
        o64 = ops.kernel_fwd_matern52(ctx, pk1, n1, p1, pk2, n2, p2, d, hyp, jitter=1e-3, dtype=torch.float64)
        ref = S * K
        ref = ref + 1e-3 * torch.eye(ref.shape[0], ref.shape[1], dtype=torch.float64)
        errs["double + jitter"] = relmax(o64, ref)
        off = ~torch.eye(ref.shape[0], ref.shape[1], dtype=torch.bool)
        assert torch.equal(o64.cpu()[off], out.double().cpu()[off])             # the same fp32 values, widened
    # a padded output (ld > n2 q2): nothing outside the view is written
    wide = torch.full((out.shape[0], out.shape[1] + 5), float("nan"), device=gpu_device)
    ops.kernel_fwd_matern52(ctx, pk1, n1, p1, pk2, n2, p2, d, hyp, out=wide[:, 2:2 + out.shape[1]])
    assert torch.equal(wide[:, 2:2 + out.shape[1]], out) and bool(torch.isnan(wide[:, :2]).all()) and bool(torch.isnan(wide[:, -3:]).all())
    _report("Matern forward d=%d p1=%d p2=%d %dx%d" % (d, p1, p2, n1, n2), errs)
    assert max(errs.values()) < KTOL, errs


@gpu
def test_kzz_is_exact_on_its_diagonal_and_symmetric(dsvgp, gpu_device):
    """K_ZZ (double output, jitter 1e-3): r == 0 stays exact, so the value diagonal is s + jitter bit for bit and the derivative diagonal
    the prior diagonal (5/3) s |v~|^2.  The output is exactly symmetric, as the RBF wide forward's is on the same pack (asserted for both:
    T[i, j] and T[j, i] are the same fma chain over k, and the transform is symmetric in (u, w) up to the sign both entries share)."""
    n, p, _, _, d = SYM
    x, v, _, _, ell, _, K, _ = _case(*SYM, symmetric=True)
    ops, ctx, hyp, elld, pk, _ = _packs(dsvgp, gpu_device, x, v, p, x, v, p, ell)
    out = ops.kernel_fwd_matern52(ctx, pk, n, p, pk, n, p, d, hyp, jitter=1e-3, dtype=torch.float64)
    ref = S * K + 1e-3 * torch.eye(K.shape[0], dtype=torch.float64)
    diag = ops.kernel_diag_matern52(ctx, pk, n, p, d, hyp)
    errs = {"K_ZZ": relmax(out, ref), "diag": relmax(diag, S * K.diagonal()), "diag of K_ZZ vs kernel_diag_matern52": relmax(out.diagonal() - 1e-3, diag)}
    _report("Matern symmetric forward", errs)
    assert max(errs.values()) < KTOL, errs
    exact = (torch.tensor(S, dtype=torch.float32) + torch.tensor(1e-3, dtype=torch.float32)).double()      # the fp32 sum, widened
    assert torch.equal(out.diagonal()[::p + 1].cpu(), exact.expand(n))
    rbf = ops.kernel_fwd_wide(ctx, pk, n, pk, n, d, p, hyp, jitter=1e-3, dtype=torch.float64)
    sym_rbf, sym_mat = torch.equal(rbf, rbf.t()), torch.equal(out, out.t())
    print("[parity] exactly symmetric K_ZZ: RBF wide forward %s, Matern forward %s" % (sym_rbf, sym_mat))
    assert sym_mat or not sym_rbf


@gpu
@pytest.mark.parametrize("n,p,d", [(41, 3, 5), (23, 1, 200), (30, 0, 6)])
def test_kernel_diag_matern52_and_its_backward(dsvgp, gpu_device, n, p, d):
    dev = gpu_device
    g = torch.Generator().manual_seed(n + d)
    x, v, gbar = torch.rand(n, d, generator=g), torch.randn(n * p, d, generator=g), torch.randn(n * (p + 1), generator=g, dtype=torch.float64)
    ell = ard_lengthscales(d)
    ellr, sr = ell.clone().requires_grad_(True), torch.tensor(S, dtype=torch.float64, requires_grad=True)
    ref = sr * matern_kernel(x.double(), v.double(), p, x.double(), v.double(), p, ellr).diagonal()
    (ref * gbar).sum().backward()
    ops, ctx, hyp, elld, pk, _ = _packs(dsvgp, dev, x, v, p, x, v, p, ell)
    out = ops.kernel_diag_matern52(ctx, pk, n, p, d, hyp)
    d_ell, d_hyp = torch.zeros(d, device=dev), torch.zeros(4, device=dev)
    ops.kernel_diag_matern52_bwd(ctx, pk, n, p, d, elld, hyp, out, gbar.float().to(dev), d_ell, d_hyp)
    errs = {"diag": relmax(out, ref.detach()), "d_s": abs(d_hyp[1].item() - sr.grad.item()) / max(1.0, abs(sr.grad.item()))}
    if p:
        errs["d_ell"] = relmax(d_ell, ellr.grad)
    else:
        assert d_ell.abs().max().item() == 0.0
    _report("kernel_diag_matern52 n=%d p=%d d=%d" % (n, p, d), errs)
    assert errs["diag"] < KTOL and errs["d_s"] < KBWD_TOL and errs.get("d_ell", 0.0) < KBWD_TOL, errs
    again_l, again_h = torch.zeros(d, device=dev), torch.zeros(4, device=dev)
    ops.kernel_diag_matern52_bwd(ctx, pk, n, p, d, elld, hyp, out, gbar.float().to(dev), again_l, again_h)
    assert torch.equal(again_l, d_ell) and torch.equal(again_h, d_hyp) and d_hyp[0].item() == 0.0


# ------------------------------------------------------------------ backward
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
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=FWD_IDS)
def test_kernel_bwd_matern52_matches_autograd(dsvgp, gpu_device, shape):
    dev = gpu_device
    n1, p1, n2, p2, d = shape
    x1, v1, x2, v2, ell, G, _, refs = _case(*shape)
    ops, ctx, hyp, elld, pk1, pk2 = _packs(dsvgp, dev, x1, v1, p1, x2, v2, p2, ell)
    for Gd, up in ((G.to(dev), "double"), (G.float().to(dev), "float")):
        outs = _outputs(n1, p1, d, dev)
        ops.kernel_bwd_matern52(ctx, Gd, pk1, n1, p1, pk2, n2, p2, d, elld, hyp, False, *outs)
        _check_bwd("kernel_bwd_matern52 d=%d p1=%d p2=%d %dx%d %s upstream" % (d, p1, p2, n1, n2, up), outs, refs, p1)


@gpu
def test_kernel_bwd_matern52_symmetric_matches_autograd_of_the_symmetric_kernel(dsvgp, gpu_device):
    """K_ZZ-bar: every diagonal micro-block has nn = 0, where the f3 term must vanish and not turn into 0 * inf"""
    dev = gpu_device
    n, p, _, _, d = SYM
    x, v, _, _, ell, G, _, refs = _case(*SYM, symmetric=True)
    ops, ctx, hyp, elld, pk, _ = _packs(dsvgp, dev, x, v, p, x, v, p, ell)
    for Gd, up in ((G.to(dev), "double"), (G.float().to(dev), "float")):
        outs = _outputs(n, p, d, dev)
        ops.kernel_bwd_matern52(ctx, Gd, pk, n, p, pk, n, p, d, elld, hyp, True, *outs)
        assert all(bool(torch.isfinite(t).all()) for t in outs)
        _check_bwd("kernel_bwd_matern52 symmetric %s upstream" % up, outs, refs, p)


@gpu
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[3]], ids=[IDS[0], IDS[1], IDS[3]])
def test_kernel_bwd_matern52_accumulates_is_reproducible_and_stays_inside_its_buffers(dsvgp, gpu_device, shape):
    dev = gpu_device
    n1, p1, n2, p2, d = shape
    x1, v1, x2, v2, ell, G, _, _ = _case(*shape)
    ops, ctx, hyp, elld, pk1, pk2 = _packs(dsvgp, dev, x1, v1, p1, x2, v2, p2, ell)
    Gf = G.float().to(dev)

    def run(Gd, out=None, with_ell=True, workspace=None):
        out = out or _outputs(n1, p1, d, dev)
        ops.kernel_bwd_matern52(ctx, Gd, pk1, n1, p1, pk2, n2, p2, d, elld, hyp, False, out[0], out[1], out[2] if with_ell else None, out[3],
                                workspace)
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
    n = run(Gf, with_ell=False)                                            # d_ell = NULL: the other outputs bitwise unchanged
    assert torch.equal(n[0], a[0]) and torch.equal(n[1], a[1]) and torch.equal(n[3], a[3]) and n[2].abs().max().item() == 0.0
    # NaN guard bands around the outputs and the workspace stay untouched
    band = 64
    nbytes = ops.kernel_bwd_matern52_workspace_bytes(n1, p1, n2, p2, d)
    wsbuf = torch.full((nbytes // 4 + 2 * band,), float("nan"), device=dev)
    ws = wsbuf[band:band + nbytes // 4].view(torch.uint8)
    sizes = (n1 * d, max(n1 * p1, 1) * d, d, 4)
    bufs = [torch.full((sz + 2 * band,), float("nan"), device=dev) for sz in sizes]
    for buf, sz in zip(bufs, sizes):
        buf[band:band + sz] = 0.0
    guarded = (bufs[0][band:band + sizes[0]].view(n1, d), bufs[1][band:band + sizes[1]].view(-1, d), bufs[2][band:band + d], bufs[3][band:band + 4])
    e = run(Gf, out=guarded, workspace=ws)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a, e))
    for buf, sz in zip(bufs + [wsbuf], sizes + (nbytes // 4,)):
        assert bool(torch.isnan(buf[:band]).all()) and bool(torch.isnan(buf[band + sz:]).all())


@gpu
def test_exact_duplicates_off_the_diagonal_are_finite_and_match_the_yardstick(dsvgp, gpu_device):
    """three rows of x2 copied from x1 with other directions: nn == 0 exactly off the diagonal (the packs share the centre and the
    k-ordered self terms), those blocks are s [[1, 0], [0, (5/3) v~_a . v~_b]]; three more pairs at distance 1e-3 (in units of ell) are
    measured and asserted finite only: there nn is what cancellation leaves of the fp32 self terms"""
    dev = gpu_device
    n1, p1, n2, p2, d = DUP
    x1, v1, x2, v2, ell, G, K, refs = _case(*DUP, duplicates=True)
    ops, ctx, hyp, elld, pk1, pk2 = _packs(dsvgp, dev, x1, v1, p1, x2, v2, p2, ell)
    out = ops.kernel_fwd_matern52(ctx, pk1, n1, p1, pk2, n2, p2, d, hyp)
    assert bool(torch.isfinite(out).all())
    Kb, ob = (S * K).reshape(n1, p1 + 1, n2, p2 + 1), out.double().cpu().reshape(n1, p1 + 1, n2, p2 + 1)
    scale = (S * K).abs().max().item()
    exact = max((ob[i, :, j, :] - Kb[i, :, j, :]).abs().max().item() for i, j in ((5, 3), (0, 17), (36, 40))) / scale
    near = max((ob[i, :, j, :] - Kb[i, :, j, :]).abs().max().item() for i, j in ((7, 8), (11, 20), (30, 33))) / scale
    for i, j in ((5, 3), (0, 17), (36, 40)):
        assert ob[i, 0, j, 0].item() == torch.tensor(S, dtype=torch.float32).item()          # nn == 0: s f0 = s exactly
        assert ob[i, 0, j, 1:].abs().max().item() == 0.0 and ob[i, 1:, j, 0].abs().max().item() == 0.0
    outs = _outputs(n1, p1, d, dev)
    ops.kernel_bwd_matern52(ctx, G.float().to(dev), pk1, n1, p1, pk2, n2, p2, d, elld, hyp, False, *outs)
    assert all(bool(torch.isfinite(t).all()) for t in outs)
    # the duplicate rows' own gradients (G restricted to the duplicate pairs' blocks): finite and the yardstick's
    mask = torch.zeros(n1, p1 + 1, n2, p2 + 1, dtype=torch.float64)
    for i, j in ((5, 3), (0, 17), (36, 40)):
        mask[i, :, j, :] = 1.0
    Gm = G * mask.reshape(G.shape)
    x1r, v1r = x1.double().requires_grad_(True), v1.double().requires_grad_(True)
    ellr, sr = ell.clone().requires_grad_(True), torch.tensor(S, dtype=torch.float64, requires_grad=True)
    (sr * matern_kernel(x1r, v1r, p1, x2.double(), v2.double(), p2, ellr) * Gm).sum().backward()
    outs_m = _outputs(n1, p1, d, dev)
    ops.kernel_bwd_matern52(ctx, Gm.float().to(dev), pk1, n1, p1, pk2, n2, p2, d, elld, hyp, False, *outs_m)
    assert all(bool(torch.isfinite(t).all()) for t in outs_m)
    _report("Matern duplicates: forward blocks", {"exact duplicates": exact, "near duplicates (1e-3 ell, reported)": near,
                                                  "whole matrix": relmax(out, S * K)})
    assert exact < KTOL
    _check_bwd("kernel_bwd_matern52 on the exact-duplicate blocks alone", outs_m, (x1r.grad, v1r.grad, ellr.grad, sr.grad.item()), p1)
    errs = {"d_x1": relmax(outs[0], refs[0]), "d_v1": relmax(outs[1], refs[1]), "d_ell": relmax(outs[2], refs[2]),
            "d_s": abs(outs[3][1].item() - refs[3]) / max(1.0, abs(refs[3]))}
    _report("kernel_bwd_matern52 with exact and near duplicates, whole upstream (reported)", errs)


# ------------------------------------------------------------------ the kernel module
@gpu
@pytest.mark.parametrize("n1,n2,p,d,ard", [(13, 17, 2, 5, True), (13, 17, 2, 5, False), (7, 9, 1, 120, True)])
def test_kernel_module_reaches_all_five_inputs(dsvgp, gpu_device, n1, n2, p, d, ard):
    dev = gpu_device
    g = torch.Generator().manual_seed(n1 + d)
    x1, x2 = torch.rand(n1, d, generator=g), torch.rand(n2, d, generator=g)
    v1, v2 = torch.randn(n1 * p, d, generator=g), torch.randn(n2 * p, d, generator=g)
    G = torch.randn(n1 * (p + 1), n2 * (p + 1), generator=g, dtype=torch.float64)
    ell = ard_lengthscales(d) if ard else torch.tensor([0.4 * math.sqrt(d)], dtype=torch.float64)
    ins64 = [t.double().requires_grad_(True) for t in (x1, x2, v1, v2, ell)]
    K64 = matern_kernel(ins64[0], ins64[2], p, ins64[1], ins64[3], p, ins64[4].expand(d))
    ref = torch.autograd.grad((K64 * G).sum(), ins64)
    kern = dsvgp.Matern52KernelDirectionalGrad(ard_num_dims=d if ard else None).to(dev)
    kern.lengthscale = ell.float()
    assert kern.lengthscale.shape == (1, ell.numel()) and relmax(kern.lengthscale.reshape(-1), ell) < 1e-6
    ins = [t.to(dev).requires_grad_(True) for t in (x1, x2, v1, v2)]
    K = kern(ins[0], ins[1], v1=ins[2], v2=ins[3])
    (K * G.float().to(dev)).sum().backward()
    got = [t.grad for t in ins] + [kern.raw_lengthscale.grad]
    sig = torch.sigmoid(kern.raw_lengthscale.detach().double().cpu()).reshape(-1)
    errs = {"K": relmax(K.detach(), K64.detach())}
    for name, a, b in zip(("d_x1", "d_x2", "d_v1", "d_v2"), got, ref):
        errs[name] = relmax(a, b)
    errs["d_raw_lengthscale"] = relmax(got[4].reshape(-1), ref[4] * sig)
    _report("Matern52KernelDirectionalGrad(ard_num_dims=%s) d=%d" % (d if ard else None, d), errs)
    assert got[4].shape == (1, ell.numel()) and kern.n_dir1 == p and kern.num_outputs_per_input(None, None) == p + 1
    assert errs.pop("K") < KTOL and max(errs.values()) < KBWD_TOL, errs
    xs, vs = x1.to(dev), v1.to(dev)
    diag = kern(xs, xs, diag=True, v1=vs, v2=vs)
    Kd = matern_kernel(x1.double(), v1.double(), p, x1.double(), v1.double(), p, ell.expand(d)).diagonal()
    assert relmax(diag, Kd) < KTOL
    with pytest.raises(RuntimeError, match="diag=True"):
        kern(xs, x2[:n1].to(dev), diag=True, v1=vs, v2=vs)
    with pytest.raises(ValueError, match="Matern"):
        kern(xs.double(), xs.double(), v1=vs.double(), v2=vs.double())


# ------------------------------------------------------------------ the engine: step and predictions against the yardstick
@functools.lru_cache(maxsize=None)
def _reference(shape, mll):
    P, x, y, D, nd = _problem(*shape)
    return matern_elbo({k: v.double() for k, v in P.items()}, x.double(), y.double(), D.double(), shape[4], nd, mll)


def _engine(dsvgp, dev, kernel="matern52"):
    eng = dsvgp.ElboEngine(dev)
    eng.kernel = kernel
    return eng


@gpu
@pytest.mark.parametrize("shape", STEPS, ids=STEP_IDS)
@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
def test_step_matches_the_yardstick(dsvgp, gpu_device, shape, mll):
    N, d, M, p, pd, B = shape
    P, x, y, D, nd = _problem(*shape)
    dev = gpu_device
    eng = _engine(dsvgp, dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    out = eng.loss_and_grads(Pg, x.to(dev), y.to(dev), D.to(dev) if pd else None, nd, mll)
    torch.cuda.synchronize()
    assert eng.c_step_used is False and eng._train_pd is None and eng._ard is False and eng._matern is False
    assert out[2].shape == (B * (pd + 1),) and out[1]["raw_lengthscale"].shape == (1, d)
    _check_step("Matern step N=%d d=%d M=%d p=%d pd=%d B=%d %s" % (N, d, M, p, pd, B, mll), out, _reference(shape, mll), p, False)
    loss0, grads0 = out[0].clone(), {k: v.clone() for k, v in out[1].items()}      # (the engine hands out its own buffers)
    again = eng.loss_and_grads(Pg, x.to(dev), y.to(dev), D.to(dev) if pd else None, nd, mll)
    assert torch.equal(again[0], loss0) and all(torch.equal(again[1][k], grads0[k]) for k in grads0)
    with pytest.raises(ValueError, match=r"B\*\(p\+1\)=%d$" % (B * (pd + 1))):
        eng.loss_and_grads(Pg, x.to(dev), torch.zeros(B * (pd + 1) + 1, device=dev), D.to(dev) if pd else None, nd, mll)


@gpu
@pytest.mark.parametrize("shape", [STEPS[0], STEPS[1], STEPS[3]], ids=[STEP_IDS[0], STEP_IDS[1], STEP_IDS[3]])
def test_predict_and_predict_joint_match_the_yardstick(dsvgp, gpu_device, shape):
    N, d, M, p, pd, B = shape
    P, x, _, D, _ = _problem(*shape)
    P64 = {k: v.double() for k, v in P.items()}
    mu_ref, Sig_ref = matern_predictive(P64, x.double(), D.double(), pd)
    noise = (torch.nn.functional.softplus(P64["raw_noise"]).reshape(()) + O.NOISE_FLOOR).item()
    dev = gpu_device
    eng = _engine(dsvgp, dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    Dg = D.to(dev) if pd else None
    mu, varn = eng.predict(Pg, x.to(dev), Dg)
    mu_c, varn_c = eng.predict(Pg, x.to(dev), Dg, cache=True)
    mu_h, varn_h = eng.predict(Pg, x.to(dev), Dg, cache=True)             # the evaluation cache: the factor and the lengthscales kept
    assert eng._eval_cache is not None and eng._eval_cache[0][0] == "matern52"
    mu_j, Sigma = eng.predict_joint(Pg, x.to(dev), Dg)
    n = B * (pd + 1)
    errs = {"mean": relmax(mu, mu_ref), "variance": relmax(varn, Sig_ref.diagonal() + noise), "joint mean": relmax(mu_j, mu_ref),
            "covariance": relmax(Sigma, Sig_ref + noise * torch.eye(n, dtype=torch.float64)),
            "diagonal vs variance": relmax(Sigma.diagonal(), varn), "cached mean": relmax(mu_h, mu_ref),
            "cached variance": relmax(varn_h, Sig_ref.diagonal() + noise)}
    _report("Matern predict d=%d M=%d p=%d pd=%d B=%d" % (d, M, p, pd, B), errs)
    assert mu.shape == varn.shape == mu_j.shape == (n,) and Sigma.shape == (n, n) and eng._ard is False and eng._matern is False
    assert torch.equal(mu_c, mu) and torch.equal(varn_c, varn) and torch.equal(mu_h, mu) and torch.equal(varn_h, varn)
    assert errs.pop("covariance") < CTOL and max(errs.values()) < TOL, errs


@gpu
@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
def test_a_scalar_lengthscale_is_d_equal_ard_lengthscales(dsvgp, gpu_device, mll):
    """bitwise in the loss, the predictions and every gradient but the lengthscale's, which is the sum of the ARD one"""
    shape = STEPS[0]
    N, d, M, p, pd, B = shape
    P, x, y, D, nd = _problem(*shape)
    dev = gpu_device
    Pv = {k: v.to(dev) for k, v in P.items()}
    Pv["raw_lengthscale"] = torch.full((1, d), 0.3, device=dev)
    Ps = dict(Pv, raw_lengthscale=torch.full((1, 1), 0.3, device=dev))
    xg, yg, Dg = x.to(dev), y.to(dev), D.to(dev)
    a = _engine(dsvgp, dev).loss_and_grads(Ps, xg, yg, Dg, nd, mll)
    b = _engine(dsvgp, dev).loss_and_grads(Pv, xg, yg, Dg, nd, mll)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    for k in a[1]:
        if k != "raw_lengthscale":
            assert torch.equal(a[1][k], b[1][k]), k
    gs, gv = a[1]["raw_lengthscale"], b[1]["raw_lengthscale"]
    assert gs.shape == (1, 1) and gv.shape == (1, d)
    rel = abs(gs.item() - gv.double().sum().item()) / abs(gv.double().sum().item())
    print("[parity] scalar-lengthscale gradient vs the sum of the ARD one (%s): %.2e" % (mll, rel))
    assert rel < 1e-6
    ref = matern_elbo({k: v.double().cpu() for k, v in Ps.items()}, x.double(), y.double(), D.double(), pd, nd, mll)
    _check_step("Matern scalar-lengthscale step %s" % mll, a, ref, p, False)
    eng_s, eng_v = _engine(dsvgp, dev), _engine(dsvgp, dev)
    for cache in (False, True, True):
        ps, pv = eng_s.predict(Ps, xg, Dg, cache=cache), eng_v.predict(Pv, xg, Dg, cache=cache)
        assert torch.equal(ps[0], pv[0]) and torch.equal(ps[1], pv[1])
    js, jv = eng_s.predict_joint(Ps, xg, Dg), eng_v.predict_joint(Pv, xg, Dg)
    assert torch.equal(js[0], jv[0]) and torch.equal(js[1], jv[1])


@gpu
def test_the_rbf_engine_is_untouched_and_the_switch_leaves_no_state(dsvgp, gpu_device):
    from test_gpu_step import make_problem
    dev = gpu_device
    Ps, xs, ys, Ds, nds = make_problem(400, 5, 24, 2, 96, seed=3)
    Pg = {k: v.to(dev) for k, v in Ps.items()}
    xg, yg, Dg = xs.to(dev), ys.to(dev), Ds.to(dev)

    def keep(out):                      # (the engine hands out its own buffers: copies)
        return tuple({k: v.clone() for k, v in t.items()} if isinstance(t, dict) else t.clone() for t in out)

    def rbf_run(eng):
        assert eng.kernel == "rbf"
        step = keep(eng.loss_and_grads(Pg, xg, yg, Dg, nds))
        general = keep(eng.loss_and_grads(Pg, xg, yg, Dg, nds, "PLL"))
        pred = keep(eng.predict(Pg, xg, Dg, cache=True))
        pred2 = keep(eng.predict(Pg, xg, Dg, cache=True))
        joint = keep(eng.predict_joint(Pg, xg, Dg))
        return step, general, pred, pred2, joint

    def same(a, b):
        for u, v in zip(a, b):
            assert torch.equal(u[0], v[0])
            if isinstance(u[1], dict):
                assert all(torch.equal(u[1][k], v[1][k]) for k in u[1]) and torch.equal(u[2], v[2]) and torch.equal(u[3], v[3])
            else:
                assert torch.equal(u[1], v[1])

    fresh = rbf_run(dsvgp.ElboEngine(dev))
    eng = dsvgp.ElboEngine(dev)
    first = rbf_run(eng)
    eng.kernel = "matern52"
    m1 = keep(eng.loss_and_grads(Pg, xg, yg, Dg, nds))
    mp = keep(eng.predict(Pg, xg, Dg, cache=True))
    assert not torch.equal(m1[0], first[0][0]) and not torch.equal(mp[0], first[2][0])       # (another kernel, and no stale cache hit)
    eng.kernel = "rbf"
    back = rbf_run(eng)
    same(fresh, first)
    same(fresh, back)
    eng.kernel = "matern52"
    mp2 = eng.predict(Pg, xg, Dg, cache=True)
    m2 = eng.loss_and_grads(Pg, xg, yg, Dg, nds)
    assert torch.equal(mp2[0], mp[0]) and torch.equal(mp2[1], mp[1]) and torch.equal(m2[0], m1[0])
    assert all(torch.equal(m2[1][k], m1[1][k]) for k in m1[1])


# ------------------------------------------------------------------ model and harness
@gpu
def test_harness_trains_evaluates_and_round_trips(dsvgp, gpu_device):
    """f(x) = sin(6 x_0) with its gradient on U[0, 1]^2 (the ARD harness test's set): d = 2, N = 400, M = 16, p = 2, 10 epochs of 4
    minibatches of 100, learning rate 0.05, fixed seed.  Nothing in the state dict records the kernel: a Matern model's state loads into
    an RBF model (same keys and shapes) -- whoever stores a model stores its kernel name next to it."""
    from torch.utils.data import TensorDataset
    from dsvgp_amd import directional_vi
    torch.manual_seed(0)
    n, dim = 400, 2
    X = torch.rand(n, dim)
    Y = torch.stack([torch.sin(6 * X[:, 0]), 6 * torch.cos(6 * X[:, 0]), torch.zeros(n)], 1)
    kw = dict(num_inducing=16, num_directions=2, minibatch_size=100, minibatch_dim=2, num_epochs=10, learning_rate_hypers=0.05, seed=0,
              kernel="matern52", ard_num_dims=2)
    losses = []
    loop = directional_vi.setup_training(TensorDataset(X, Y), **kw)
    assert isinstance(loop.model.covar_module.base_kernel, dsvgp.Matern52KernelDirectionalGrad) and loop.model.engine.kernel == "matern52"
    for _ in range(10):
        perm = loop.epoch_permutation()
        for start in range(0, n, 100):
            loss, output, y_batch = loop.step(perm[start:start + 100])
            assert loop.model.engine.c_step_used is False
            losses.append(loss.item())
    loop.finish()
    first, last = sum(losses[:4]) / 4, sum(losses[-4:]) / 4
    ell = loop.model.covar_module.base_kernel.lengthscale.detach().cpu()
    print("[parity] Matern harness: mean loss of the first epoch %.4f, of the last %.4f, lengthscales (%.4f, %.4f)"
          % (first, last, ell[0, 0].item(), ell[0, 1].item()))
    assert all(math.isfinite(l) for l in losses) and last < first and losses[-1] < losses[0]
    # train_gp itself takes the keyword (through **args); eval_gp runs; the state round-trips bitwise
    model, likelihood = dsvgp.train_gp(TensorDataset(X, Y), tqdm=False, verbose=False, max_steps=3, **kw)
    assert isinstance(model.covar_module.base_kernel, dsvgp.Matern52KernelDirectionalGrad)
    assert model.covar_module.base_kernel.lengthscale.shape == (1, 2)
    test = TensorDataset(torch.rand(50, 2), torch.zeros(50, 3))
    means, variances = dsvgp.eval_gp(test, loop.model, loop.likelihood, num_directions=2, minibatch_size=25, minibatch_dim=2)
    assert means.shape == variances.shape == (150,) and bool(torch.isfinite(means).all()) and bool((variances > 0).all())
    state = {k: v.clone() for k, v in loop.model.state_dict().items()}
    fresh = directional_vi.setup_training(TensorDataset(X, Y), **kw)
    fresh.model.load_state_dict(state)
    fresh.likelihood.load_state_dict(loop.likelihood.state_dict())
    m2, v2 = dsvgp.eval_gp(test, fresh.model, fresh.likelihood, num_directions=2, minibatch_size=25, minibatch_dim=2)
    assert torch.equal(m2, means) and torch.equal(v2, variances)
    rbf = directional_vi.setup_training(TensorDataset(X, Y), **dict(kw, kernel="rbf"))
    assert list(rbf.model.state_dict()) == list(state) and rbf.model.engine.kernel == "rbf"
    rbf.model.load_state_dict(state)                                         # succeeds: the state dict does not say which kernel
    rbf.likelihood.load_state_dict(loop.likelihood.state_dict())
    m3, _ = dsvgp.eval_gp(test, rbf.model, rbf.likelihood, num_directions=2, minibatch_size=25, minibatch_dim=2)
    assert not torch.equal(m3, means)                                        # ... and the same numbers mean another model under RBF
    # a scalar-lengthscale Matern model through the harness
    sc = directional_vi.setup_training(TensorDataset(X, Y), **dict(kw, ard_num_dims=None))
    assert sc.model.covar_module.base_kernel.raw_lengthscale.shape == (1, 1)
    l0 = sc.step(torch.arange(100, device=gpu_device))[0].item()
    assert math.isfinite(l0) and sc.model.covar_module.base_kernel.raw_lengthscale.grad.shape == (1, 1)
    sc.finish()


# ------------------------------------------------------------------ refusals
@gpu
def test_what_is_not_built_for_matern_raises(dsvgp, gpu_device):
    from dsvgp_amd._step64 import ElboEngine64
    dev = gpu_device
    shape = STEPS[0]
    N, d, M, p, pd, B = shape
    P, x, y, D, nd = _problem(*shape)
    xg, yg, Dg = x.to(dev), y.to(dev), D.to(dev)
    word = "Matern"

    class _World:
        rank, world = 0, 2

    for rl in (P["raw_lengthscale"], torch.zeros(1, 1)):
        Pg = {k: v.to(dev) for k, v in dict(P, raw_lengthscale=rl).items()}
        with pytest.raises(ValueError, match=word):                            # the Gram fast path
            _engine(dsvgp, dev).loss_and_grads(Pg, xg, yg, Dg, nd, "ELBO", fast=True)
        for attr, val in (("whitening", "ciq"), ("shared_directions", True), ("capture_mode", True), ("deterministic", True),
                          ("data_outputs", "values"), ("collective", _World())):
            eng = _engine(dsvgp, dev)
            setattr(eng, attr, val)
            with pytest.raises(ValueError, match=word):
                eng.loss_and_grads(Pg, xg, yg, Dg, nd)
            if attr != "deterministic":
                for call in (eng.predict, eng.predict_joint):
                    with pytest.raises(ValueError, match=word):
                        call(Pg, xg, Dg)
        from test_ngd import make_ngd_problem
        Pn = {k: v.to(dev) for k, v in make_ngd_problem(N, d, M, p, B)[0].items()}
        Pn["raw_lengthscale"] = Pg["raw_lengthscale"]
        with pytest.raises(ValueError, match=word):
            _engine(dsvgp, dev).loss_and_grads(Pn, xg, yg, Dg, nd)
        P64 = {k: v.double() for k, v in Pg.items()}
        e64 = ElboEngine64(dev)
        e64.kernel = "matern52"
        with pytest.raises(ValueError, match=word):
            e64.loss_and_grads(P64, xg.double(), yg.double(), Dg.double(), nd)
        with pytest.raises(ValueError, match=word):
            e64.predict(P64, xg.double(), Dg.double())
        with pytest.raises(ValueError, match=word):
            _engine(dsvgp, dev).loss_and_grads(P64, xg.double(), yg.double(), Dg.double(), nd)
        eng = _engine(dsvgp, dev)
        for call in (lambda: eng.mean_predictor(Pg), lambda: eng.predict_blocks(Pg, xg, Dg), lambda: eng.sample_paths(Pg, 2, num_features=16),
                     lambda: eng.prior_moments(Pg), lambda: eng.whiten_legacy(Pg), lambda: eng.value_variances(Pg)):
            with pytest.raises(ValueError, match=word):
                call()
    with pytest.raises(ValueError, match="1 entry or one per input dimension"):
        _engine(dsvgp, dev).predict(dict(Pg, raw_lengthscale=torch.zeros(1, 2, device=dev)), xg, Dg)
    # the model: what is built on those entries refuses too
    Z, V = torch.rand(8, d).to(dev), torch.eye(d)[:p].repeat(8, 1).to(dev)
    model = dsvgp.GPModel(Z, V, d, kernel="matern52").to(dev)
    model.eval()
    for call in (lambda: model.posterior_mean(xg), lambda: model.sample_paths(2, num_features=16),
                 lambda: model.thompson_step(xg, torch.zeros(d, device=dev), torch.ones(d, device=dev), 2, num_features=16)):
        with pytest.raises(ValueError, match=word):
            call()


@gpu
def test_c_entry_refusals(dsvgp, gpu_device):
    """dsvgp_kernel_fwd_matern52 refuses what dsvgp_kernel_fwd_rect refuses and touches nothing; dsvgp_kernel_bwd_matern52 has the ARD
    backward's refusals and optional pointers; empty problems return 0"""
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
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    out = torch.zeros(n1 * (p1 + 1), n2, device=dev)

    def fwd(n1=n1, p1=p1, n2=n2, p2=p2, d=d, ld=n2, P1=pz[0].data_ptr(), s1=pz[1], out_=out, hyp_=hyp, dbl=0):
        return lib.dsvgp_kernel_fwd_matern52(ctx.h, C.c_void_p(P1), vp(s1), n1, p1, vp(px[0]), vp(px[1]), n2, p2, d, vp(hyp_), 0.0, vp(out_), ld, dbl)

    assert fwd(ld=n2 - 1) == -1 and fwd(P1=pz[0].data_ptr() + 4) == -1 and fwd(p1=96) == -1 and fwd(p2=96) == -1 and fwd(p1=-1) == -1
    assert fwd(d=0) == -1 and fwd(n1=0) == -1 and fwd(n2=0) == -1 and fwd(s1=None) == -1 and fwd(out_=None) == -1 and fwd(hyp_=None) == -1
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0.0                                     # the refused calls touched nothing
    assert fwd() == 0
    G = torch.zeros(n1 * (p1 + 1), n2, device=dev)
    dx, dv, dl, dh = torch.zeros(n1, d, device=dev), torch.zeros(n1 * p1, d, device=dev), torch.zeros(d, device=dev), torch.zeros(4, device=dev)
    ws = torch.empty(ops.kernel_bwd_matern52_workspace_bytes(n1, p1, n2, p2, d), dtype=torch.uint8, device=dev)

    def entry(n1=n1, p1=p1, n2=n2, p2=p2, d=d, ldg=n2, P1=pz[0].data_ptr(), vn=pz[2], dv_=dv, dl_=dl, ws_=ws, ell_=ell, sym=0, dx_=dx):
        return lib.dsvgp_kernel_bwd_matern52(ctx.h, vp(G), ldg, 0, C.c_void_p(P1), vp(pz[1]), vp(vn), n1, p1, vp(px[0]), vp(px[1]), n2, p2, d,
                                             vp(ell_), vp(hyp), sym, vp(dx_), vp(dv_), vp(dl_), vp(dh), vp(ws_))

    assert entry() == 0
    assert entry(dl_=None) == 0 and entry(dv_=None, vn=None) == 0            # the optional outputs
    assert entry(ldg=n2 - 1) == -1 and entry(P1=pz[0].data_ptr() + 4) == -1 and entry(p1=96) == -1 and entry(p2=96) == -1
    assert entry(p1=-1) == -1 and entry(d=0) == -1 and entry(vn=None) == -1 and entry(ws_=None) == -1 and entry(ell_=None) == -1
    assert entry(dx_=None) == -1 and entry(sym=1) == -1                      # symmetric needs n1 == n2 and p1 == p2
    assert entry(n1=0) == 0 and entry(n2=0) == 0 and entry(n1=-1) == -1
    assert lib.dsvgp_kernel_diag_matern52(ctx.h, None, n1, p1, d, vp(hyp), vp(dh)) == -1
    assert lib.dsvgp_kernel_diag_matern52(ctx.h, vp(pz[0]), n1, 96, d, vp(hyp), vp(dh)) == -1
    assert lib.dsvgp_kernel_diag_matern52_bwd(ctx.h, vp(pz[0]), n1, p1, d, None, vp(hyp), vp(dh), vp(dh), vp(dl), vp(dh)) == -1
    torch.cuda.synchronize()
    assert all(t.abs().max().item() == 0.0 for t in (dx, dv, dl, dh))        # (G = 0, and the refused calls touched nothing)
