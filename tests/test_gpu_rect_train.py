"""Training with any number of data directions: the rectangular kernel backward (``dsvgp_kernel_bwd_rect``, csrc/assemble_wide.hip),
``ElboEngine.loss_and_grads`` with pd != p on top of it, and the ``data_directions`` keyword of the model / harness.

The yardstick is built here in float64: ``rect_kernel`` of tests/test_gpu_rect_predict.py (differentiable torch), the oracle's Cholesky
and the oracle's likelihood / KL terms (``rect_forward``), gradients by autograd (``rect_elbo``).  The CPU tests pin it to
``O.elbo_loss_and_grads`` where that is defined (pd = p; pd = 0 through ``data_outputs="values"``), to 1e-12 relative.  The GPU tests
hold the HIP path to it at the project's tolerances for the same quantities: kernel backward against float64 autograd 2e-4
(tests/test_gpu_wide_inputs.py); step loss 2e-5 relative, mean 2e-4, variance 2e-4, gradients 2e-3
(tests/test_gpu_step.py::test_dfree_step_matches_oracle).  Measured errors are printed as [parity] lines.

Kernel-level inputs: X ~ U[0, 1]^d with the lengthscale 0.4 sqrt(d), as the wide-input tests (the kernel between random points is
~0.6 at every d, so no comparison checks zeros)."""
import ctypes as C
import functools
import math

import pytest
import torch

import dsvgp_oracle as O
from test_gpu_rect_predict import rect_kernel

gpu = pytest.mark.gpu
KBWD_TOL, LOSS_TOL, MU_TOL, VAR_TOL, GRAD_TOL = 2e-4, 2e-5, 2e-4, 2e-4, 2e-3


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _report(tag, errs):
    print("[parity] %s: %s" % (tag, ", ".join("%s %.2e" % (k, v) for k, v in errs.items())))


def _raw(v):
    return math.log(math.expm1(v))          # softplus^-1


# ------------------------------------------------------------------ the yardstick
def rect_forward(P, x, y, D, pd, num_data, mll):
    """(loss, mu, varn) of one minibatch objective when the data carry pd directions per point and the model p: ``O.elbo_forward``
    (reference directional_vi.py:245-246) with K_ZX and diag K_XX of the (p + 1) x (pd + 1) block kernel.  Differentiable."""
    Z, V, m = P["inducing_points"], P["inducing_directions"], P["variational_mean"]
    L_S = torch.tril(P["chol_variational_covar"])
    c = P["constant"].reshape(())
    ell, s, noise = O.constrained(P)
    M, B = Z.shape[0], x.shape[0]
    p = V.shape[0] // M
    K_ZZ = s * O.kernel_matrix(Z, Z, V, V, ell)
    L = O.psd_safe_cholesky(K_ZZ + O.KZZ_JITTER * torch.eye(K_ZZ.shape[0], dtype=K_ZZ.dtype))
    K_ZX = s * rect_kernel(Z, V, p, x, D, pd, ell)
    A = torch.linalg.solve_triangular(L, K_ZX, upper=False)
    mu = A.t() @ m + c
    SA = L_S @ (L_S.t() @ A) - A
    var = s * O.kernel_diag(B, pd, ell).to(x.dtype) + O.KXX_JITTER + (A * SA).sum(0)
    varn = (var + noise).clamp_min(O.MIN_VARIANCE)
    if mll == "ELBO":
        ll = -0.5 * (((y - mu) ** 2 + varn) / noise + torch.log(noise) + math.log(2 * math.pi))
    elif mll == "PLL":
        tot = (varn + noise).clamp_min(1e-8)
        ll = -0.5 * ((y - mu) ** 2 / tot + torch.log(tot) + math.log(2 * math.pi))
    else:
        raise ValueError(mll)
    loss = -(ll.sum() / y.shape[0] - O.kl_whitened(m, L_S) / num_data)
    return loss, mu, varn


def rect_elbo(P64, x, y, D, pd, num_data, mll):
    """(loss, grads, mu, varn) in float64, gradients by autograd"""
    ps = {k: v.detach().clone().requires_grad_(True) for k, v in P64.items()}
    loss, mu, varn = rect_forward(ps, x, y, D, pd, num_data, mll)
    loss.backward()
    grads = {k: (ps[k].grad if ps[k].grad is not None else torch.zeros_like(ps[k])) for k in ps}
    return loss.detach(), grads, mu.detach(), varn.detach()


#          N    d    M  p pd   B
STEPS = [(400, 3, 16, 2, 0, 96),
         (400, 3, 16, 2, 3, 96),
         (300, 5, 12, 0, 2, 64),
         (300, 20, 10, 5, 1, 48),
         (300, 120, 8, 2, 1, 32)]           # wide inputs: several K chunks
STEP_IDS = ["N%d-d%d-M%d-p%d-pd%d-B%d" % s for s in STEPS]


@functools.lru_cache(maxsize=None)
def _problem(N, d, M, p, pd, B):
    """(params fp32, x, y [B (pd + 1)], data directions [B pd, d], num_data): once per shape, shared, never changed"""
    from test_gpu_step import make_problem
    P, x, _, _, nd = make_problem(N, d, M, p, B, seed=N + d + pd)
    if d > 30:          # (otherwise the kernel between random points is numerically zero)
        P["raw_lengthscale"] = torch.tensor([[_raw(0.4 * math.sqrt(d))]])
    g = torch.Generator().manual_seed(17 + pd)
    cols = sorted((torch.randperm(d, generator=g)[:pd] + 1).tolist())
    y = O.testfun(x)[:, [0] + cols].reshape(-1).contiguous()
    D = (torch.eye(d)[[c - 1 for c in cols]] + 0.1 * torch.randn(pd, d, generator=g)).repeat(B, 1)        # generic, not one-hot
    return P, x, y, D, nd


@functools.lru_cache(maxsize=None)
def _reference(shape, mll):
    P, x, y, D, nd = _problem(*shape)
    return rect_elbo({k: v.double() for k, v in P.items()}, x.double(), y.double(), D.double(), shape[4], nd, mll)


# ------------------------------------------------------------------ CPU: the yardstick against the oracle
@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
def test_yardstick_equals_the_oracle_where_the_oracle_is_defined(mll):
    from test_gpu_step import make_problem
    N, d, M, p, B = 400, 3, 16, 2, 96
    P, x, y, D, nd = make_problem(N, d, M, p, B, seed=11)
    P64, x, y, D = {k: v.double() for k, v in P.items()}, x.double(), y.double(), D.double()
    y0 = O.testfun(x)[:, 0].contiguous()
    errs = {}
    for tag, mine, ref in (("pd=p", rect_elbo(P64, x, y, D, p, nd, mll), O.elbo_loss_and_grads(P64, x, y, D, nd, mll)),
                           ("pd=0", rect_elbo(P64, x, y0, D[:0], 0, nd, mll),
                            O.elbo_loss_and_grads(P64, x, y0, D, nd, mll, data_outputs="values"))):
        errs[tag + " loss"] = abs(mine[0].item() - ref[0].item()) / abs(ref[0].item())
        errs[tag + " mu"], errs[tag + " varn"] = relmax(mine[2], ref[2]), relmax(mine[3], ref[3])
        for k in O.PARAM_NAMES:
            errs[tag + " " + k] = relmax(mine[1][k], ref[1][k])
    _report("yardstick vs oracle, %s" % mll, errs)
    assert max(errs.values()) <= 1e-12, errs


# ------------------------------------------------------------------ GPU 1: the kernel entry against float64 autograd
#       n1  p1   n2 p2    d
OPS = [(40, 2, 130, 0, 3),          # ragged row and column tiles at q2 = 1
       (100, 0, 50, 3, 5),          # value-only model side
       (20, 5, 45, 2, 20),          # pd < p
       (20, 2, 45, 5, 20),          # pd > p
       (3, 95, 100, 0, 9),          # q = 96 on the model side (the capped column tile)
       (30, 1, 5, 95, 9),           # q = 96 on the data side
       (11, 2, 23, 4, 120),         # K loop, ragged last chunk
       (9, 3, 30, 0, 200)]
OP_IDS = ["%dx%d-%dx%d-d%d" % o for o in OPS]


@functools.lru_cache(maxsize=None)
def _op_case(n1, p1, n2, p2, d):
    """(x1, v1, x2, v2, ell, s, G fp64, autograd gradients of sum(G * s K) w.r.t. x1, v1, ell, s): once per shape"""
    g = torch.Generator().manual_seed(n1 + 31 * n2 + 7 * p1 + 3 * p2 + d)
    x1, x2 = torch.rand(n1, d, generator=g), torch.rand(n2, d, generator=g)
    v1, v2 = torch.randn(n1 * p1, d, generator=g), torch.randn(n2 * p2, d, generator=g)
    ell, s = 0.4 * math.sqrt(d), 1.3
    G = torch.randn(n1 * (p1 + 1), n2 * (p2 + 1), generator=g, dtype=torch.float64)
    x1r, v1r = x1.double().requires_grad_(True), v1.double().requires_grad_(True)
    ellr = torch.tensor(ell, dtype=torch.float64, requires_grad=True)
    sr = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    (sr * rect_kernel(x1r, v1r, p1, x2.double(), v2.double(), p2, ellr) * G).sum().backward()
    gv = v1r.grad if p1 else torch.zeros(0, d, dtype=torch.float64)
    return x1, v1, x2, v2, ell, s, G, (x1r.grad, gv, ellr.grad.item(), sr.grad.item())


def _op_packs(dsvgp, dev, x1, v1, p1, x2, v2, p2, ell, s):
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    hyp = torch.tensor([ell, s, 0.1, 0.0], dtype=torch.float32, device=dev)
    x1d = x1.to(dev).contiguous()
    center = ops.column_mean(ctx, x1d)
    pk1 = ops.pack_points(ctx, x1d, v1.to(dev).contiguous() if p1 else None, p1, hyp, center)
    pk2 = ops.pack_points(ctx, x2.to(dev).contiguous(), v2.to(dev).contiguous() if p2 else None, p2, hyp, center)
    return ops, ctx, hyp, pk1, pk2


def _outputs(n1, p1, d, dev):
    return torch.zeros(n1, d, device=dev), torch.zeros(max(n1 * p1, 1), d, device=dev), torch.zeros(4, device=dev)


@gpu
@pytest.mark.parametrize("n1,p1,n2,p2,d", OPS, ids=OP_IDS)
def test_kernel_bwd_rect_matches_autograd(dsvgp, gpu_device, n1, p1, n2, p2, d):
    dev = gpu_device
    x1, v1, x2, v2, ell, s, G, (gx, gv, gl, gs) = _op_case(n1, p1, n2, p2, d)
    ops, ctx, hyp, pk1, pk2 = _op_packs(dsvgp, dev, x1, v1, p1, x2, v2, p2, ell, s)
    for Gd, up in ((G.to(dev), "double"), (G.float().to(dev), "float")):
        dx, dv, dh = _outputs(n1, p1, d, dev)
        ops.kernel_bwd_rect(ctx, Gd, pk1, n1, p1, pk2, n2, p2, d, hyp, dx, dv, dh)
        errs = {"d_x1": relmax(dx, gx), "d_l": abs(dh[0].item() - gl) / max(1.0, abs(gl)), "d_s": abs(dh[1].item() - gs) / max(1.0, abs(gs))}
        if p1 > 0:
            errs["d_v1"] = relmax(dv[:n1 * p1], gv)
        _report("kernel_bwd_rect d=%d p1=%d p2=%d %dx%d %s upstream" % (d, p1, p2, n1, n2, up), errs)
        assert dh[2].item() == 0.0 and dh[3].item() == 0.0
        for k, e in errs.items():
            assert e < KBWD_TOL, (up, k, e)


@gpu
@pytest.mark.parametrize("shape", [OPS[0], OPS[3], OPS[6]], ids=[OP_IDS[0], OP_IDS[3], OP_IDS[6]])
def test_kernel_bwd_rect_accumulates_takes_a_strided_upstream_and_is_reproducible(dsvgp, gpu_device, shape):
    dev = gpu_device
    n1, p1, n2, p2, d = shape
    x1, v1, x2, v2, ell, s, G, _ = _op_case(*shape)
    ops, ctx, hyp, pk1, pk2 = _op_packs(dsvgp, dev, x1, v1, p1, x2, v2, p2, ell, s)
    Gf = G.float().to(dev)

    def run(Gd, out=None):
        out = out or _outputs(n1, p1, d, dev)
        ops.kernel_bwd_rect(ctx, Gd, pk1, n1, p1, pk2, n2, p2, d, hyp, *out)
        return out

    a, b = run(Gf), run(Gf)
    assert all(torch.equal(u, v) for u, v in zip(a, b))                     # two identical calls on zeroed outputs
    assert a[0].abs().max().item() > 0 and a[2][:2].abs().min().item() > 0
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


@gpu
@pytest.mark.parametrize("n1,p,n2,d", [(20, 5, 45, 20), (11, 2, 23, 200)])
def test_kernel_bwd_rect_at_equal_counts_is_kernel_bwd_wide(dsvgp, gpu_device, n1, p, n2, d):
    """p1 == p2 > 0: the column-tile cap does not bite, so the two entries plan the same tiles for the one kernel_bwd_tbar_kernel --
    bitwise equal"""
    dev = gpu_device
    x1, v1, x2, v2, ell, s, G, _ = _op_case(n1, p, n2, p, d)
    ops, ctx, hyp, pk1, pk2 = _op_packs(dsvgp, dev, x1, v1, p, x2, v2, p, ell, s)
    for Gd in (G.to(dev), G.float().to(dev)):
        rect, wide = _outputs(n1, p, d, dev), _outputs(n1, p, d, dev)
        ops.kernel_bwd_rect(ctx, Gd, pk1, n1, p, pk2, n2, p, d, hyp, *rect)
        ops.kernel_bwd_wide(ctx, Gd, pk1, n1, pk2, n2, d, p, hyp, False, *wide)
        _report("equal counts d=%d p=%d %dx%d" % (d, p, n1, n2), {k: relmax(u, v) for k, u, v in zip(("d_x1", "d_v1", "d_hyp"), rect, wide)})
        assert all(torch.equal(u, v) for u, v in zip(rect, wide))


@gpu
@pytest.mark.parametrize("n1,p,n2,d", [(20, 5, 45, 20), (11, 2, 23, 200), (9, 0, 30, 200)])
def test_kernel_fwd_rect_at_equal_counts_is_kernel_fwd_wide(dsvgp, gpu_device, n1, p, n2, d):
    """p1 == p2 (the forward has no column cap, so p = 0 too): the same tiles of the one kernel_fwd_tiled_kernel, ragged on both sides, one K
    chunk and several with a ragged last one, 1 x 1 micro-blocks -- equal values (not told apart: a -0 that meets the wide entry's
    zero jitter on the global diagonal)"""
    dev = gpu_device
    x1, v1, x2, v2, ell, s, _, _ = _op_case(n1, p, n2, p, d)
    ops, ctx, hyp, pk1, pk2 = _op_packs(dsvgp, dev, x1, v1, p, x2, v2, p, ell, s)
    rect = ops.kernel_fwd_rect(ctx, pk1, n1, p, pk2, n2, p, d, hyp)
    wide = ops.kernel_fwd_wide(ctx, pk1, n1, pk2, n2, d, p, hyp, jitter=0.0, dtype=torch.float32)
    assert rect.shape == wide.shape == (n1 * (p + 1), n2 * (p + 1)) and rect.abs().max().item() > 0
    assert torch.equal(rect, wide)


# ------------------------------------------------------------------ GPU 2: the step against the yardstick
def _check_step(tag, out, ref, p, fast):
    loss, grads, mu, varn = out
    l_ref, g_ref, mu_ref, var_ref = ref
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref)}
    if fast:
        assert varn.numel() == 0
    else:
        errs["varn"] = relmax(varn, var_ref)
    for k in O.PARAM_NAMES:
        if p == 0 and k == "inducing_directions":
            continue
        errs[k] = relmax(grads[k], g_ref[k])
    _report(tag, errs)
    assert grads["chol_variational_covar"].triu(1).abs().max().item() == 0.0
    assert errs["loss"] < LOSS_TOL and errs["mu"] < MU_TOL and errs.get("varn", 0.0) < VAR_TOL, errs
    for k in O.PARAM_NAMES:
        assert errs.get(k, 0.0) < GRAD_TOL, (k, errs)
    return errs


@gpu
@pytest.mark.parametrize("shape", STEPS, ids=STEP_IDS)
@pytest.mark.parametrize("mll", ["ELBO", "ELBO-general", "PLL"])
def test_step_matches_the_yardstick(dsvgp, gpu_device, shape, mll):
    fast = mll == "ELBO"
    mll = mll.split("-")[0]
    N, d, M, p, pd, B = shape
    P, x, y, D, nd = _problem(*shape)
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    out = eng.loss_and_grads(Pg, x.to(dev), y.to(dev), D.to(dev) if pd else None, nd, mll, fast=fast)
    torch.cuda.synchronize()
    assert eng.c_step_used is False and eng._train_pd is None
    assert out[2].shape == (B * (pd + 1),)
    _check_step("rect step N=%d d=%d M=%d p=%d pd=%d B=%d %s%s" % (N, d, M, p, pd, B, mll, " fast" if fast else ""), out,
                _reference(shape, mll), p, fast)
    with pytest.raises(ValueError, match=r"B\*\(p\+1\)=%d$" % (B * (pd + 1))):
        eng.loss_and_grads(Pg, x.to(dev), torch.zeros(B * (pd + 1) + 1, device=dev), D.to(dev) if pd else None, nd, mll, fast=fast)


@gpu
@pytest.mark.parametrize("mll", ["ELBO", "ELBO-general", "PLL"])
def test_value_only_data_against_the_derivative_free_engine(dsvgp, gpu_device, mll):
    """pd = 0 two ways, same parameters and batch: both held to the yardstick and to each other at the tolerances, not bitwise"""
    from test_gpu_step import make_problem
    fast = mll == "ELBO"
    mll = mll.split("-")[0]
    shape = STEPS[0]
    N, d, M, p, pd, B = shape
    P, x, y, _, nd = _problem(*shape)
    dev = gpu_device
    Pg = {k: v.to(dev) for k, v in P.items()}
    Dp = torch.eye(d)[:p].repeat(B, 1).to(dev)                   # (the derivative-free engine takes the model's count and ignores it)
    rect = dsvgp.ElboEngine(dev).loss_and_grads(Pg, x.to(dev), y.to(dev), None, nd, mll, fast=fast)
    dfree_eng = dsvgp.ElboEngine(dev)
    dfree_eng.data_outputs = "values"
    dfree = dfree_eng.loss_and_grads(Pg, x.to(dev), y.to(dev), Dp, nd, mll, fast=fast)
    ref = _reference(shape, mll)
    _check_step("pd = 0 rectangular %s%s" % (mll, " fast" if fast else ""), rect, ref, p, fast)
    _check_step("pd = 0 derivative-free %s%s" % (mll, " fast" if fast else ""), dfree, ref, p, fast)
    _check_step("pd = 0 rectangular vs derivative-free %s%s" % (mll, " fast" if fast else ""), rect,
                (dfree[0], dfree[1], dfree[2], dfree[3]), p, fast)


@gpu
@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
def test_natural_parameters(dsvgp, gpu_device, mll):
    from test_ngd import make_ngd_problem
    N, d, M, p, B, pd = 400, 3, 16, 2, 96, 3
    P, x, _, _, nd = make_ngd_problem(N, d, M, p, B)
    g = torch.Generator().manual_seed(3)
    y = O.testfun(x)[:, :pd + 1].reshape(-1).contiguous()
    D = (torch.eye(d)[:pd] + 0.1 * torch.randn(pd, d, generator=g)).repeat(B, 1)
    P64 = {k: v.double() for k, v in P.items()}
    l_ref, g_ref, mu_ref, var_ref = O.ngd_loss_and_grads(P64, x.double(), y.double(), D.double(), nd, mll,
                                                         forward=lambda ps, x_, y_, D_, n_, m_, gr, sd: rect_forward(ps, x_, y_, D_, pd, n_, m_))
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    loss, grads, mu, varn = eng.loss_and_grads({k: v.to(dev) for k, v in P.items()}, x.to(dev), y.to(dev), D.to(dev), nd, mll)
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref)}
    if varn.numel():
        errs["varn"] = relmax(varn, var_ref)
    errs.update({k: relmax(grads[k], g_ref[k]) for k in O.NGD_PARAM_NAMES})
    _report("rect step, natural parameters, pd = %d %s" % (pd, mll), errs)
    assert eng.c_step_used is False and set(grads) == set(O.NGD_PARAM_NAMES)
    assert errs["loss"] < LOSS_TOL and errs["mu"] < MU_TOL and errs.get("varn", 0.0) < VAR_TOL, errs
    assert all(errs[k] < GRAD_TOL for k in O.NGD_PARAM_NAMES), errs


@gpu
@pytest.mark.parametrize("mll,fast", [("ELBO", True), ("PLL", False)])
def test_deterministic_steps_are_bitwise_equal(dsvgp, gpu_device, mll, fast):
    shape = STEPS[1]
    P, x, y, D, nd = _problem(*shape)
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    eng.deterministic = True
    Pg = {k: v.to(dev) for k, v in P.items()}
    runs = []
    for _ in range(2):
        loss, grads, mu, varn = eng.loss_and_grads(Pg, x.to(dev), y.to(dev), D.to(dev), nd, mll, fast=fast)
        runs.append([loss.clone(), mu.clone(), varn.clone()] + [grads[k].clone() for k in O.PARAM_NAMES])
    assert all(torch.equal(u, v) for u, v in zip(*runs))
    _check_step("rect step, deterministic %s" % mll, (runs[0][0], dict(zip(O.PARAM_NAMES, runs[0][3:])), runs[0][1], runs[0][2]),
                _reference(shape, mll), shape[3], fast)


# ------------------------------------------------------------------ GPU 3: model and harness
def _harness_run(dsvgp, data_directions, capsys):
    """the 600-point, d = 2 drop-in problem of tests/test_gpu_rect_predict.py with ONE inducing direction, one epoch of 12 minibatches"""
    from torch.utils.data import TensorDataset
    from dsvgp_amd import directional_vi
    torch.manual_seed(0)
    n, dim, n_test = 600, 2, 300
    train_x, test_x = torch.rand(n, dim), torch.rand(n_test, dim)
    train_y, test_y = O.testfun(train_x), O.testfun(test_x)
    kw = dict(num_inducing=20, num_directions=1, minibatch_size=50, minibatch_dim=1, num_epochs=1, learning_rate_hypers=0.01,
              use_ngd=True, learning_rate_ngd=0.1, inducing_data_initialization=False, seed=0, data_directions=data_directions)
    # the loop of train_gp, step by step: every step's loss
    loop = directional_vi.setup_training(TensorDataset(train_x, train_y), **kw)
    assert loop.data_directions == data_directions and loop.model.data_directions == data_directions
    perm = loop.epoch_permutation()
    losses = []
    for start in range(0, n, 50):
        loss, output, y_batch = loop.step(perm[start:start + 50])
        assert y_batch.shape == (50 * (data_directions + 1),) and output.mean.shape == y_batch.shape
        assert loop.model.engine.c_step_used is False
        losses.append(loss.item())
    loop.finish()
    # and train_gp itself (its every-50th-step report reads the value rows with the data's stride)
    model, likelihood = dsvgp.train_gp(TensorDataset(train_x, train_y), tqdm=False, verbose=True, **kw)
    out = capsys.readouterr().out
    report = [l for l in out.splitlines() if l.startswith("Epoch")]
    assert len(report) == 1 and math.isfinite(float(report[0].split("loss: ")[1].split(",")[0])) and math.isfinite(float(report[0].split("nll: ")[1]))
    means, variances = dsvgp.eval_values(TensorDataset(test_x, test_y), model, likelihood, minibatch_size=128)
    mse = ((means - test_y[:, 0]) ** 2).mean().item()
    mse_const = ((test_y[:, 0].mean() - test_y[:, 0]) ** 2).mean().item()
    return losses, mse, mse_const, variances, model, test_x


@gpu
@pytest.mark.parametrize("data_directions", [2, 0])
def test_harness_trains_with_another_number_of_data_directions(dsvgp, gpu_device, capsys, data_directions):
    losses, mse, mse_const, variances, model, test_x = _harness_run(dsvgp, data_directions, capsys)
    print("[parity] harness data_directions=%d: first loss %.4f, epoch mean %.4f, last %.4f, MSE %.4f (constant predictor %.4f)"
          % (data_directions, losses[0], sum(losses) / len(losses), losses[-1], mse, mse_const))
    assert len(losses) == 12 and all(math.isfinite(l) for l in losses)
    assert sum(losses) / len(losses) < losses[0]
    assert mse < mse_const and bool((variances > 0).all())
    # the call takes exactly data_directions per point
    model.train()
    xg = test_x[:10].to(gpu_device)
    with pytest.raises(AssertionError):
        model(xg, derivative_directions=torch.eye(2, device=gpu_device)[:1].repeat(10, 1))          # the model's own count is the wrong one now


@gpu
def test_model_call_keeps_the_reference_assertion_without_data_directions(dsvgp, gpu_device):
    dev = gpu_device
    Z, V = torch.rand(6, 3), torch.eye(3)[:2].repeat(6, 1)
    model = dsvgp.GPModel(Z, V, 3).to(dev)
    x = torch.rand(5, 3, device=dev)
    assert model.data_directions is None
    with pytest.raises(AssertionError):
        model(x, derivative_directions=torch.eye(3, device=dev)[:1].repeat(5, 1))
    with pytest.raises(AssertionError):
        model(x, derivative_directions=torch.eye(3, device=dev).repeat(5, 1))
    assert model(x, derivative_directions=torch.eye(3, device=dev)[:2].repeat(5, 1)).x is x
    model.data_directions = 3
    assert model(x, derivative_directions=torch.eye(3, device=dev).repeat(5, 1)).D.shape == (15, 3)
    with pytest.raises(AssertionError):
        model(x, derivative_directions=torch.eye(3, device=dev)[:2].repeat(5, 1))
    model.data_directions = 0
    assert model(x, derivative_directions=None).D is None and model(x).D is None


# ------------------------------------------------------------------ GPU 4: refusals
@gpu
def test_refusals(dsvgp, gpu_device):
    from torch.utils.data import TensorDataset
    from test_gpu_step import make_problem
    from dsvgp_amd import dfree_directional_vi
    dev = gpu_device
    P, x, _, _, nd = make_problem(300, 3, 12, 2, 20, seed=1)
    Pg = {k: v.to(dev) for k, v in P.items()}
    xg, y0 = x.to(dev), torch.zeros(20, device=dev)
    for attr, val, word in (("whitening", "ciq", "CIQ"), ("shared_directions", True, "shared"), ("capture_mode", True, "capture_mode")):
        eng = dsvgp.ElboEngine(dev)
        setattr(eng, attr, val)
        with pytest.raises(ValueError, match=word):
            eng.loss_and_grads(Pg, xg, y0, None, nd)
    from dsvgp_amd._step64 import ElboEngine64
    with pytest.raises(ValueError, match="float64"):
        ElboEngine64(dev).loss_and_grads({k: v.double() for k, v in Pg.items()}, xg.double(), y0.double(), None, nd)
    # harness: float64 data, the other variants
    data = TensorDataset(torch.rand(40, 2), O.testfun(torch.rand(40, 2)))
    with pytest.raises(ValueError, match="float64"):
        dsvgp.directional_vi.setup_training(None, num_inducing=4, data_directions=2,
                                            tensors=(torch.rand(40, 2, device=dev).double(), torch.rand(40, 3, device=dev).double()))
    with pytest.raises(ValueError, match="dfree"):
        dsvgp.directional_vi.setup_training(data, num_inducing=4, dfree=True, data_directions=0)
    with pytest.raises(ValueError, match=r"\[0, 2\]"):
        dsvgp.directional_vi.setup_training(data, num_inducing=4, data_directions=3)
    # the C entry: a leading dimension that is too small, a misaligned pack, p = 96, null pointers, d = 0; empty problems return 0
    ops, lib = dsvgp._ops, dsvgp._lib.lib
    ctx = ops.Context.get(dev)
    hyp = torch.tensor([0.9, 1.7, 0.1, 0.0], device=dev)
    pz = ops.pack_points(ctx, Pg["inducing_points"], Pg["inducing_directions"], 2, hyp)
    px = ops.pack_points(ctx, xg, None, 0, hyp)
    G = torch.zeros(36, 20, device=dev)
    dx, dv, dh = torch.zeros(12, 3, device=dev), torch.zeros(24, 3, device=dev), torch.zeros(4, device=dev)
    ws = torch.empty(ops.kernel_bwd_rect_workspace_bytes(12, 2, 20, 0, 3), dtype=torch.uint8, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def entry(n1=12, p1=2, n2=20, p2=0, d=3, ldg=20, P1=pz[0].data_ptr(), vn=pz[2], dv_=dv, ws_=ws):
        return lib.dsvgp_kernel_bwd_rect(ctx.h, vp(G), ldg, 0, C.c_void_p(P1), vp(pz[1]), vp(vn), n1, p1, vp(px[0]), vp(px[1]), n2, p2, d,
                                         vp(hyp), vp(dx), vp(dv_), vp(dh), vp(ws_))

    assert entry() == 0
    assert entry(ldg=19) == -1 and entry(P1=pz[0].data_ptr() + 4) == -1 and entry(p1=96) == -1 and entry(p2=96) == -1
    assert entry(p1=-1) == -1 and entry(d=0) == -1 and entry(vn=None) == -1 and entry(dv_=None) == -1 and entry(ws_=None) == -1
    assert entry(n1=0) == 0 and entry(n2=0) == 0 and entry(n1=-1) == -1
    torch.cuda.synchronize()
    assert dx.abs().max().item() == 0.0 and dv.abs().max().item() == 0.0          # (G = 0, and the refused calls touched nothing)
