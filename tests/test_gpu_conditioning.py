"""Every kernel-assembly route of the library across input scale, offset and lengthscale, scored block by block (tests/_conditioning.py):
the isotropic routes (general whole-row, pair KSM 8 / 16, split-row, canon, canon2, wide, rect), ARD, Matern-5/2, the float64 assembly
plain and tiled, then the three on-the-fly predictors and one ELBO step.

Forward: every route x every regime, the four block errors under 4 y + 2e-7 (fp64: 4 y + 1e-13), y the reference's own op sequence in
float32 on centred inputs.  Backward: five regimes, four block-masked upstreams plus the dense one; d_x1 and d_v1 within 2e-4 of that
gradient's own maximum under that mask, d_ell and d_s within 2e-4 sum|G_ij dK_ij / d theta| (the reduction's conditioning scale; fp64
routes: 1e-10, tests/test_gpu_fp64.py's backward tolerance), truth float64 autograd through the oracle.  Measured errors are printed as
[parity] lines next to their yardsticks."""
import functools
import math

import pytest
import torch

import dsvgp_oracle as O
import _conditioning as C
import _variance_yardstick as Y

pytestmark = pytest.mark.gpu
f32, f64 = torch.float32, torch.float64
JITTER = 1e-3
FWD = [(r, g) for r in C.ROUTES for g in C.REGIMES]
SYM = [(r, g) for r in C.SYMMETRIC_ROUTES for g in C.REGIMES]
BWD = [(r, g) for r in C.BWD_ROUTES for g in C.BWD_REGIMES]
_id = lambda rg: "%s-%s" % rg


def _fmt(d):
    return ", ".join("%s %s" % (k, "-" if v is None else "%.2e" % v) for k, v in d.items())


class Route:
    """the packs of one case on the device and its forward / backward entry"""

    def __init__(self, dsvgp, dev, name, c):
        self.ops, self.dev, self.c, self.name = dsvgp._ops, dev, c, name
        ops = self.ops
        self.ctx = ctx = ops.Context.get(dev)
        self.fp64 = c.kind == "rbf64"
        dt = f64 if self.fp64 else f32
        self.dt = dt
        up = lambda t: t.to(dt).to(dev).contiguous()
        x1, x2 = up(c.x1), up(c.x2)
        v1, v2 = (up(c.v1) if c.p1 else None), (up(c.v2) if c.p2 else None)
        self.vec = c.ell.dim() > 0
        self.hyp = torch.tensor([1.0 if self.vec else float(c.ell), C.S, 0.1, 0.0], dtype=dt, device=dev)
        if self.fp64:
            center = x1.mean(0).contiguous()
            self.pk1 = ops.pack_points_f64(ctx, x1, v1, c.p1, self.hyp, center)
            self.pk2 = self.pk1 if c.symmetric else ops.pack_points_f64(ctx, x2, v2, c.p2, self.hyp, center)
        elif self.vec:
            self.ell = up(c.ell)
            center = ops.column_mean(ctx, x1)
            self.pk1 = ops.pack_points_ard(ctx, x1, v1, c.p1, self.ell, center)
            self.pk2 = ops.pack_points_ard(ctx, x2, v2, c.p2, self.ell, center)
        else:
            center = ops.column_mean(ctx, x1)
            self.pk1 = ops.pack_points(ctx, x1, v1, c.p1, self.hyp, center)
            self.pk2 = self.pk1 if c.symmetric else ops.pack_points(ctx, x2, v2, c.p2, self.hyp, center)
        if c.idx is not None:
            self.di = (torch.tensor(c.idx, dtype=torch.int32) + 1).to(dev)            # idx_base = 1

    def forward(self, out=None, jitter=0.0, dtype=None):
        o, c, ctx = self.ops, self.c, self.ctx
        a = (ctx, self.pk1, c.n1, self.pk2, c.n2, c.d, c.p1)
        if self.fp64:
            return o.kernel_fwd_f64(*a, self.hyp, jitter=jitter, out=out)
        if self.name == "canon2":
            return o.kernel_fwd_canon2(*a, self.di, 1, self.hyp, jitter=jitter, out=out, dtype=dtype)
        if self.name == "canon":
            return o.kernel_fwd_canon(*a, self.di, 1, self.hyp, out=out)
        if c.kind == "matern":
            return o.kernel_fwd_matern52(ctx, self.pk1, c.n1, c.p1, self.pk2, c.n2, c.p2, c.d, self.hyp, out=out)
        if self.vec or self.name.startswith("rect"):
            return o.kernel_fwd_rect(ctx, self.pk1, c.n1, c.p1, self.pk2, c.n2, c.p2, c.d, self.hyp, out=out)
        return o.kernel_fwd(*a, self.hyp, jitter=jitter, out=out, dtype=dtype or f32)

    def backward(self, G):
        """-> (d_x1, d_v1, d_ell, d_s) from zeroed accumulators"""
        o, c, ctx, dev = self.ops, self.c, self.ctx, self.dev
        dx = torch.zeros(c.n1, c.d, dtype=self.dt, device=dev)
        dv = torch.zeros(max(c.n1 * c.p1, 1), c.d, dtype=self.dt, device=dev)
        dh = torch.zeros(4, dtype=self.dt, device=dev)
        dl = torch.zeros(c.d, dtype=self.dt, device=dev)
        a = (ctx, G, self.pk1, c.n1, self.pk2, c.n2, c.d, c.p1)
        if self.fp64:
            o.kernel_bwd_f64(*a, self.hyp, False, dx, dv[:c.n1 * c.p1], dh)
        elif self.name == "canon2":
            o.kernel_bwd_canon2(*a, self.di, 1, self.hyp, False, dx, dv, dh)
        elif self.name == "canon":
            o.kernel_bwd_canon(*a, self.di, 1, self.hyp, dx, dv, dh)
        elif c.kind in ("ard", "matern"):
            fn = o.kernel_bwd_ard if c.kind == "ard" else o.kernel_bwd_matern52
            fn(ctx, G, self.pk1, c.n1, c.p1, self.pk2, c.n2, c.p2, c.d, self.ell, self.hyp, False, dx, dv, dl, dh)
            assert dh[0].item() == 0.0
        elif self.name.startswith("rect"):
            o.kernel_bwd_rect(ctx, G, self.pk1, c.n1, c.p1, self.pk2, c.n2, c.p2, c.d, self.hyp, dx, dv, dh)
        else:
            o.kernel_bwd(*a, self.hyp, False, dx, dv, dh)
        assert dh[2].item() == 0.0 and dh[3].item() == 0.0
        return dx, dv[:c.n1 * c.p1], (dl if self.vec else dh[0]).cpu(), dh[1].item()


def _padded(rows, cols, dt, dev):
    """a NaN-filled buffer and its [rows, cols] view one element in: a padded leading dimension, rows not 16-byte aligned"""
    buf = torch.full((rows, cols + 3), float("nan"), dtype=dt, device=dev)
    return buf, buf[:, 1:cols + 1]


def _check_blocks(tag, K, Kref, c, bound, y, exc):
    errs = C.block_errors(K, Kref, c.n1, c.q1, c.n2, c.q2)
    print("[parity] %s: %s | yardstick %s%s" % (tag, _fmt(errs), _fmt(y),
                                                  " | bound 4x the packed restatement's error in " + ", ".join(exc) if exc else ""))
    for k, e in errs.items():
        assert e <= bound[k], (tag, k, e, bound[k])
    return errs


@pytest.mark.parametrize("route,regime", FWD, ids=[_id(x) for x in FWD])
def test_forward_blocks(dsvgp, gpu_device, route, regime):
    c, Kref, y = C.reference(route, regime)
    bound, exc = C.effective_bounds(route, regime)
    r = Route(dsvgp, gpu_device, route, c)
    K = r.forward()
    assert K.dtype == r.dt and bool(torch.isfinite(K).all())
    _check_blocks("fwd %s %s" % (route, regime), K, Kref, c, bound, y, exc)
    buf, view = _padded(K.shape[0], K.shape[1], r.dt, gpu_device)
    r.forward(out=view)
    _check_blocks("fwd %s %s (padded view)" % (route, regime), view, Kref, c, bound, y, exc)
    assert bool(torch.isnan(buf[:, 0]).all()) and bool(torch.isnan(buf[:, -2:]).all())
    if regime in ("near_dup", "clusters"):                   # the clamp at |r|^2 >= 0: no value above s (one rounding of the product)
        val = C.blocks_of(K.double().cpu(), c.n1, c.q1, c.n2, c.q2)["value"]
        assert float(val.max()) <= C.S * (1 + 2.0 ** -22), float(val.max())


@pytest.mark.parametrize("route,regime", SYM, ids=[_id(x) for x in SYM])
def test_forward_symmetric_with_jitter(dsvgp, gpu_device, route, regime):
    """x2 is x1 (one pack), float64 output with jitter: the off-diagonal entries under the block bounds, the diagonal exact"""
    c, Kref, y = C.reference(route, regime, True)
    bound, exc = C.effective_bounds(route, regime, True)
    r = Route(dsvgp, gpu_device, route, c)
    K = r.forward(jitter=JITTER, dtype=f64).cpu()
    assert K.dtype == f64 and bool(torch.isfinite(K).all())
    eye = torch.eye(K.shape[0], dtype=torch.bool)
    # float32 routes: the diagonal is checked on its own below (its float32 sum with the jitter is not a kernel error)
    Koff = K - JITTER * eye.double() if r.fp64 else torch.where(eye, Kref, K)
    _check_blocks("fwd symmetric %s %s" % (route, regime), Koff, Kref, c, bound, y, exc)
    q = c.q1
    dg, dref = K.diagonal(), Kref.diagonal()
    if not r.fp64:
        assert torch.equal(K, K.float().double())           # float32 values, widened
        exact = (torch.tensor(C.S, dtype=f32) + torch.tensor(JITTER, dtype=f32)).double()
        assert torch.equal(dg[::q], exact.expand(c.n1))     # r == 0 exactly on the diagonal: s + jitter, one float32 sum
        # derivative diagonal: s / ell^2 |v^|^2 + jitter.  |v^|^2 is 1 up to the float32 normalisation of the direction; the reference's own
        # normalisation (RBFKernelDirectionalGrad.py:57-58) run in float32 is the yardstick y_n of that, the rule 4 y_n + 2e-7 as everywhere,
        # then one float32 rounding (2^-24) of the sum with the jitter
        v = c.v1.float()
        u = (v.t() / v.norm(dim=1)).t()
        y_n = float(((u * u).sum(1).double() - 1).abs().max())
        lim = (4 * y_n + 2e-7) * dref + 2.0 ** -24 * (dref + JITTER)
        err = (dg - dref - JITTER).abs()
        print("[parity] fwd symmetric %s %s derivative diagonal: worst error / limit %.2f, y_n %.2e" % (route, regime, float((err / lim).max()), y_n))
        assert bool((err <= lim).all())
    for i in (0, c.n1 // 2, c.n1 - 1):                      # cross terms of the diagonal micro-blocks: exactly 0
        blk = K[i * q:(i + 1) * q, i * q:(i + 1) * q]
        assert blk[0, 1:].abs().max().item() == 0.0 and blk[1:, 0].abs().max().item() == 0.0


@pytest.mark.parametrize("route,regime", BWD, ids=[_id(x) for x in BWD])
def test_backward_masked_upstreams(dsvgp, gpu_device, route, regime):
    dev = gpu_device
    c, ref = C.backward_reference(route, regime)
    r = Route(dsvgp, dev, route, c)
    tol = 1e-10 if r.fp64 else C.BWD_TOL
    present = C.blocks_of(ref["dense"]["G"], c.n1, c.q1, c.n2, c.q2)
    for mask in C.MASKS:
        if mask != "dense" and present[mask].numel() == 0:
            continue
        m = ref[mask]
        yard = C.backward_errors(m["yard"], m)
        for gdt in ((f64,) if r.fp64 else (f64, f32)):
            cols = c.n2 * c.q2
            ldp = (cols + 3) // 4 * 4 + 4                    # rows of whole 16-byte pieces (what canon2's DMA path asks for), padded
            buf = torch.zeros(c.n1 * c.q1, ldp, dtype=gdt, device=dev)
            buf[:, :cols] = m["G"].to(gdt).to(dev)
            Gd = buf[:, :cols] if route == "canon2" else m["G"].to(gdt).to(dev).contiguous()
            got = r.backward(Gd)
            errs = C.backward_errors(got, m)
            if route == "canon2":                            # fixed directions: no d_v1 (asserted untouched below)
                errs.pop("d_v1", None)
            tag = "bwd %s %s mask=%s upstream=%s" % (route, regime, mask, str(gdt).split(".")[-1])
            print("[parity] %s: %s | float32 autograd yardstick %s" % (tag, _fmt(errs), _fmt(yard)))
            for k, e in errs.items():
                if e is None:                                # identically zero in truth: exactly zero
                    if k == "d_v1":
                        assert got[1].abs().max().item() == 0.0, tag
                    continue
                assert e <= tol, (tag, k, e)
            if route == "canon2":                            # fixed directions: d_v1 is not written
                assert got[1].abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------ predictors
PRED_REGIMES = ("offset", "scaled_up", "long8")
TOL = 2e-4                                                   # tests/test_gpu_mean_predictor.py, test_gpu_variance.py, test_gpu_paths.py


def _softplus_inverse(v):
    return v + math.log(-math.expm1(-v))


def _in_regime(P, x, regime):
    """the model and the test points in a regime: Z, x and the lengthscale; float32 values, the float64 copy made from them"""
    P = dict(P)
    ell = float(torch.nn.functional.softplus(P["raw_lengthscale"].double()).reshape(()))
    Z, x = P["inducing_points"].double(), x.double()
    if regime == "offset":
        Z, x = Z + 1024, x + 1024
    elif regime == "scaled_up":
        Z, x, ell = Z * 1e3, x * 1e3, 1e3 * ell
    elif regime == "long8":
        ell = 8 * ell
    else:
        raise ValueError(regime)
    P["inducing_points"] = Z.float()
    P["raw_lengthscale"] = torch.tensor([[_softplus_inverse(ell)]], dtype=f32)
    return P, {k: v.double() for k, v in P.items()}, x.float()


@functools.lru_cache(maxsize=None)
def _pred_case(kind, shape, regime):
    """(P fp32, x fp32, (mu, grad mu, sigma^2, grad sigma^2) fp64): once per case, shared.  The truth of all three predictors is ``moments``
    of tests/_variance_yardstick.py, the float64 closed forms that tests/test_variance_host.py pins to the oracle and to autograd (the mean
    and paths files' own yardsticks are the same closed form, ``mean_reference``, and the oracle's predictive)"""
    from test_gpu_step import make_problem
    if kind == "variance":
        d, M, p, B = shape
        P, _, x = Y.problem(d, M, p, B)
    else:
        N, d, M, p, B = shape
        P, x, _, _, _ = make_problem(N, d, M, p, B, seed=1)
        if d > 30:
            P["raw_lengthscale"] = torch.tensor([[_softplus_inverse(0.4 * math.sqrt(d))]])
    P, P64, x = _in_regime(P, x, regime)
    return P, x, Y.moments(P64, x.double())


def _two(tag, val, grad, val_ref, grad_ref):
    errs = {"values": Y.relmax(val, val_ref), "gradients": Y.relmax(grad, grad_ref)}
    print("[parity] %s: %s" % (tag, _fmt(errs)))
    assert errs["values"] < TOL and errs["gradients"] < TOL, (tag, errs)


@pytest.mark.parametrize("regime", PRED_REGIMES)
@pytest.mark.parametrize("shape", [(400, 32, 21, 5, 37), (400, 33, 21, 5, 37)], ids=["fused", "composed"])
def test_mean_predictor(dsvgp, gpu_device, shape, regime):
    P, x, (mu, gmu, _, _) = _pred_case("mean", shape, regime)
    pred = dsvgp.ElboEngine(gpu_device).mean_predictor({k: v.to(gpu_device) for k, v in P.items()})
    _, d, M, p, B = shape                                    # the fused kernel needs no workspace, the composed path [B, 2M] intermediates
    assert (dsvgp._ops.mean_workspace_bytes(M, d, B, 0) == 0) == (d <= 32)
    val, grad = pred.value_and_gradient(x.to(gpu_device))
    c = float(P["constant"].reshape(()))
    assert (mu - c).abs().max().item() >= 0.05              # the reference is not trivial
    _two("mean predictor %s %s" % (shape, regime), val, grad, mu, gmu)


@pytest.mark.parametrize("regime", PRED_REGIMES)
@pytest.mark.parametrize("shape", [(20, 65, 5, 130), (33, 40, 2, 70)], ids=["fused", "composed"])
def test_variance_predictor(dsvgp, gpu_device, shape, regime):
    P, x, (_, _, var, gvar) = _pred_case("variance", shape, regime)
    pred = dsvgp.ElboEngine(gpu_device).variance_predictor({k: v.to(gpu_device) for k, v in P.items()})
    assert pred.route == ("fused" if shape[0] <= 32 else "composed")
    val, grad = pred.variance_and_gradient(x.to(gpu_device))
    _two("variance predictor %s %s" % (shape, regime), val, grad, var, gvar)


@pytest.mark.parametrize("regime", PRED_REGIMES)
@pytest.mark.parametrize("shape,F,n", [((600, 20, 70, 5, 33), 128, 9), ((600, 33, 16, 3, 40), 128, 4)], ids=["fused", "composed"])
def test_paths_at_zero_draws(dsvgp, gpu_device, shape, F, n, regime):
    """all draws zero: every path is the posterior mean"""
    from test_paths_host import make_draws
    _, d, M, p, B = shape
    P, x, (mu, gmu, _, _) = _pred_case("paths", shape, regime)
    assert (dsvgp._ops.paths_workspace_bytes(M, d, F, n, B, True) == 0) == (d <= 32)      # fused: no workspace
    eng = dsvgp.ElboEngine(gpu_device)
    paths = eng.sample_paths({k: v.to(gpu_device) for k, v in P.items()}, n, F, base_samples=make_draws(d, M * (p + 1), F, n, zero=True))
    vals, grads = paths.values_and_gradients(x.to(gpu_device))
    _two("paths at zero draws %s %s" % (shape, regime), vals, grads, mu[None].expand(n, B), gmu[None].expand(n, B, d))


# ------------------------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("fast", [False, True], ids=["general", "fast"])
@pytest.mark.parametrize("regime", ["offset", "scaled_up"])
@pytest.mark.parametrize("N,d,M,p,B", [(400, 5, 20, 2, 100), (500, 20, 24, 5, 48)])
def test_one_step(dsvgp, gpu_device, N, d, M, p, B, regime, fast):
    """ElboEngine against the oracle on the same float32 inputs: loss 2e-5, mean / variance 2e-4 (tests/test_gpu_step.py), gradients against
    the float64 oracle per parameter, each relative to its own maximum, at that file's 3e-4 -- d_raw_lengthscale relative to itself"""
    from test_gpu_step import GRAD_TOL_FP64, make_problem, relmax, run_gpu
    P, x, y, D, nd = make_problem(N, d, M, p, B, seed=N + d)
    P, P64, x = _in_regime(P, x, regime)
    if regime == "scaled_up":
        want = 1e3 * math.log1p(math.exp(0.3))
        assert abs(float(torch.nn.functional.softplus(P["raw_lengthscale"])) - want) < 1e-6 * want
    l_ref, _, mu_ref, var_ref = O.elbo_loss_and_grads(P, x, y, D, nd, "ELBO")
    _, g64, _, _ = O.elbo_loss_and_grads(P64, x.double(), y.double(), D.double(), nd, "ELBO")
    loss, grads, mu, varn, _, _ = run_gpu(dsvgp, gpu_device, P, x, y, D, nd, "ELBO", fast=fast)
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref)}
    if not fast:
        errs["varn"] = relmax(varn, var_ref)
    for k in O.PARAM_NAMES:
        errs[k] = relmax(grads[k], g64[k])
    print("[parity] step N=%d d=%d M=%d p=%d B=%d %s %s: %s" % (N, d, M, p, B, regime, "fast" if fast else "general", _fmt(errs)))
    assert float(g64["raw_lengthscale"].abs().max()) > 0
    assert errs["loss"] < 2e-5 and errs["mu"] < 2e-4 and errs.get("varn", 0.0) < 2e-4, errs
    for k in O.PARAM_NAMES:
        assert errs[k] < GRAD_TOL_FP64, (k, errs[k])
