"""Per-point covariance roots (csrc/block_roots.hip): ``dsvgp_blocks_factor`` / ``dsvgp_blocks_draw`` / ``dsvgp_blocks_logpdf`` and what is
built on them -- ``_ops.blocks_*``, ``ElboEngine.block_roots`` / ``block_draw`` / ``block_log_prob``, ``PredictiveDistribution.point_roots`` /
``sample_points`` / ``point_log_prob`` / ``point_whitened_residuals``, ``ApproximateGP.sample_gradients`` / ``gradient_log_prob`` and
``eval_gradient_nll``.

The yardstick is float64 torch on the CPU applied to the SAME float32-valued blocks widened to double: ``torch.linalg.cholesky``,
``torch.distributions.MultivariateNormal(scale_tril=...)`` for the density, a triangular solve for z.  Synthetic blocks are
R R^T + delta I with R [q, q] standard normal in float64 from a fixed seed, symmetrised and rounded to float32, delta = q / 50:
lambda_max(R R^T) stays below about 6 q, so the condition number kappa stays below about 300; the tests compute kappa from the
yardstick's eigenvalues and assert kappa <= 1e3 themselves.  Every tolerance is derived (u = 2^-53):
  1  |L L^T - block| <= 2 (q + 1) u |L| |L|^T entrywise       the backward error of a Cholesky factorisation, whatever the conditioning
  2  |logdet - yardstick| <= q^2 u kappa; strict upper part exactly 0, positive diagonal, info all zero, status 0
  3  |draw - (mu + L eps)| <= 2^-23 (|mu| + |L| |eps|)          one rounding of an fp64 sum to float
  4  |z - yardstick| <= 2^-23 |z| + q 2^-52 kappa |z|_inf;  |logp - yardstick| <= 2^-22 max(1, |logp|)
(tests/test_abi_block_roots.py checks on the CPU that the yardstick itself keeps 1, 2 and 4 against a second evaluation, and reports
where bound 2 falls below what one rounding of a stored root moves: q = 1, where kappa = 1 and the bound is u.  Measured on an MI355X:
largest error / bound 0.49 (1), 1.00 at q = 1 and <= 0.13 elsewhere (2), 0.50 (3), 0.50 and 0.24 (4).)
"""
import functools
import math

import pytest
import torch
from torch.distributions import MultivariateNormal

import dsvgp_oracle as O
from test_gpu_rect_predict import rect_predictive
from test_gpu_step import make_problem

gpu = pytest.mark.gpu
f32, f64 = torch.float32, torch.float64
U = 2.0 ** -53
QS = [1, 2, 3, 6, 21, 64, 65, 96]          # both sides of every team width (8 / 16 / 32 / 64 lanes), one and two rows per lane, the largest LDS image
BS = [1, 37, 130]                          # ragged against 8, 16 and 32 blocks per workgroup
NS = [1, 5, 65]
QB = [(q, B) for q in QS for B in BS]
QB_IDS = ["q%d-B%d" % qb for qb in QB]
LOG_2PI = math.log(2.0 * math.pi)


def _report(tag, errs):
    print("[parity] %s: %s" % (tag, ", ".join("%s %.2e" % (k, v) for k, v in errs.items())))


# ------------------------------------------------------------------ the yardstick (CPU, float64)
def yardstick(blocks32):
    """(A, L, logdet, kappa) of float32 blocks [B, q, q]: widened to double, torch.linalg.cholesky, 2 sum log diag, lambda_max / lambda_min"""
    A = blocks32.detach().cpu().double()
    L = torch.linalg.cholesky(A)
    logdet = 2.0 * L.diagonal(dim1=1, dim2=2).log().sum(-1)
    ev = torch.linalg.eigvalsh(A)
    return A, L, logdet, ev[:, -1] / ev[:, 0]


def yardstick_density(L, mu, y):
    """(z [B, q], logp [B]) of y under N(mu, L L^T) per block: a triangular solve, MultivariateNormal(scale_tril)"""
    B, q = L.shape[0], L.shape[1]
    mu, y = mu.detach().cpu().double().reshape(B, q), y.detach().cpu().double().reshape(B, q)
    z = torch.linalg.solve_triangular(L, (y - mu).unsqueeze(-1), upper=False).squeeze(-1)
    return z, MultivariateNormal(mu, scale_tril=L).log_prob(y)


def closed_form_1d(mu, var, y):
    mu, var, y = (t.detach().cpu().double().reshape(-1) for t in (mu, var, y))
    return -0.5 * torch.log(2.0 * math.pi * var) - (y - mu) ** 2 / (2.0 * var)


@functools.lru_cache(maxsize=None)
def synthetic(B, q):
    """(blocks f32 [B, q, q], mu f32 [B q], y f32 [B q]) from a fixed seed; once per shape, shared, never changed"""
    g = torch.Generator().manual_seed(7919 * q + B)
    R = torch.randn(B, q, q, dtype=f64, generator=g)
    A = R @ R.transpose(1, 2)
    A = 0.5 * (A + A.transpose(1, 2)) + (q / 50.0) * torch.eye(q, dtype=f64)
    mu = torch.randn(B * q, dtype=f64, generator=g).float()
    y = (mu.double() + math.sqrt(q) * torch.randn(B * q, dtype=f64, generator=g)).float()
    return A.float().contiguous(), mu, y


@functools.lru_cache(maxsize=None)
def synthetic_yardstick(B, q):
    blocks, mu, y = synthetic(B, q)
    A, L, logdet, kappa = yardstick(blocks)
    z, logp = yardstick_density(L, mu, y)
    return A, L, logdet, kappa, z, logp


def bound_reconstruction(L, q):
    return 2.0 * (q + 1) * U * (L.abs() @ L.abs().transpose(1, 2))


def check_density(z_got, logp_got, z_ref, logp_ref, kappa, q):
    """bound 4; returns the largest ratios error / bound"""
    z_got, logp_got = z_got.detach().cpu().double(), logp_got.detach().cpu().double()
    zb = 2.0 ** -23 * z_ref.abs() + (q * 2.0 ** -52 * kappa * z_ref.abs().max(-1).values).unsqueeze(-1)
    lb = 2.0 ** -22 * logp_ref.abs().clamp_min(1.0)
    rz = ((z_got - z_ref).abs() / zb).max().item()
    rl = ((logp_got - logp_ref).abs() / lb).max().item()
    return rz, rl


def _ctx(dsvgp, dev):
    return dsvgp._ops, dsvgp._ops.Context.get(dev)


# ------------------------------------------------------------------ GPU 1, 2: the factor
@gpu
@pytest.mark.parametrize("qb", QB, ids=QB_IDS)
def test_factor_reconstructs_the_block_and_gives_the_log_determinant(dsvgp, gpu_device, qb):
    q, B = qb
    ops, ctx = _ctx(dsvgp, gpu_device)
    blocks, _, _ = synthetic(B, q)
    A, L_ref, logdet_ref, kappa, _, _ = synthetic_yardstick(B, q)
    assert float(kappa.max()) <= 1e3
    roots, logdet, info, status = ops.blocks_factor(ctx, blocks.to(gpu_device))
    torch.cuda.synchronize()
    assert roots.dtype == f64 and roots.shape == (B, q, q) and logdet.dtype == f64 and logdet.shape == (B,)
    assert info.dtype == torch.int32 and info.shape == (B,) and status.shape == (1,)
    L, ld = roots.cpu(), logdet.cpu()
    rec = ((L @ L.transpose(1, 2) - A).abs() / bound_reconstruction(L, q)).max().item()
    ldr = ((ld - logdet_ref).abs() / (q * q * U * kappa)).max().item()
    _report("factor q %d B %d (error / bound)" % (q, B), {"reconstruction": rec, "logdet": ldr, "logdet abs": (ld - logdet_ref).abs().max().item(),
                                                          "kappa": float(kappa.max())})
    assert int(status.item()) == 0 and not bool(info.any())
    assert torch.equal(L, torch.tril(L)) and not bool(torch.signbit(torch.triu(L, 1)).any())     # strict upper part: exactly +0
    assert bool((L.diagonal(dim1=1, dim2=2) > 0).all())
    assert rec <= 1.0
    assert ldr <= 1.0


# ------------------------------------------------------------------ GPU 3: the draw
@gpu
@pytest.mark.parametrize("qb", QB, ids=QB_IDS)
def test_draw_is_mu_plus_root_times_eps_rounded_once(dsvgp, gpu_device, qb):
    q, B = qb
    ops, ctx = _ctx(dsvgp, gpu_device)
    blocks, mu, _ = synthetic(B, q)
    roots, _, _, _ = ops.blocks_factor(ctx, blocks.to(gpu_device))
    L = roots.cpu()
    mud = mu.to(gpu_device)
    errs = {}
    for n in NS:
        eps = torch.randn(n, B * q, generator=torch.Generator().manual_seed(n))
        out = ops.blocks_draw(ctx, roots, mud, eps.to(gpu_device))
        assert out.dtype == f32 and out.shape == (n, B * q)
        e = eps.double().reshape(n, B, q)
        ref = mu.double().reshape(1, B, q) + torch.einsum("bac,nbc->nba", L, e)
        bound = 2.0 ** -23 * (mu.double().abs().reshape(1, B, q) + torch.einsum("bac,nbc->nba", L.abs(), e.abs()))
        errs["n %d" % n] = ((out.cpu().double().reshape(n, B, q) - ref).abs() / bound).max().item()
    _report("draw q %d B %d (error / bound)" % (q, B), errs)
    assert max(errs.values()) <= 1.0, errs
    # unit vectors as base samples: mu plus the columns of L
    eps = torch.eye(q).repeat(1, B)                                                    # row c: e_c at every point
    out = ops.blocks_draw(ctx, roots, mud, eps.to(gpu_device)).cpu().double().reshape(q, B, q)
    ref = mu.double().reshape(1, B, q) + L.permute(2, 0, 1)                            # [c, b, a] = L[b][a][c]
    assert torch.equal(out.float(), ref.float())
    assert ops.blocks_draw(ctx, roots, mud, torch.empty(0, B * q, device=gpu_device)).shape == (0, B * q)


# ------------------------------------------------------------------ GPU 4: the density
@gpu
@pytest.mark.parametrize("qb", QB, ids=QB_IDS)
def test_whitened_residual_and_log_density(dsvgp, gpu_device, qb):
    q, B = qb
    ops, ctx = _ctx(dsvgp, gpu_device)
    blocks, mu, y = synthetic(B, q)
    _, _, _, kappa, z_ref, logp_ref = synthetic_yardstick(B, q)
    roots, logdet, _, _ = ops.blocks_factor(ctx, blocks.to(gpu_device))
    z, logp = ops.blocks_logpdf(ctx, roots, logdet, mu.to(gpu_device), y.to(gpu_device))
    assert z.dtype == f32 and z.shape == (B, q) and logp.dtype == f32 and logp.shape == (B,)
    rz, rl = check_density(z, logp, z_ref, logp_ref, kappa, q)
    _report("density q %d B %d (error / bound)" % (q, B), {"z": rz, "logp": rl})
    assert rz <= 1.0 and rl <= 1.0
    none, logp2 = ops.blocks_logpdf(ctx, roots, logdet, mu.to(gpu_device), y.to(gpu_device), want_z=False)
    assert none is None and torch.equal(logp, logp2)                                   # z = NULL: the same bits


# ------------------------------------------------------------------ GPU 5: reproducibility and isolation
@gpu
@pytest.mark.parametrize("q", [6, 21, 96])
def test_identical_calls_are_bitwise_equal_and_a_block_is_a_function_of_itself(dsvgp, gpu_device, q):
    ops, ctx = _ctx(dsvgp, gpu_device)
    B = 130
    blocks, mu, y = (t.to(gpu_device) for t in synthetic(B, q))
    r1, l1, _, _ = ops.blocks_factor(ctx, blocks)
    r2, l2, _, _ = ops.blocks_factor(ctx, blocks)
    assert torch.equal(r1, r2) and torch.equal(l1, l2)
    eps = torch.randn(5, B * q, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    assert torch.equal(ops.blocks_draw(ctx, r1, mu, eps), ops.blocks_draw(ctx, r1, mu, eps))
    za, pa = ops.blocks_logpdf(ctx, r1, l1, mu, y)
    zb, pb = ops.blocks_logpdf(ctx, r1, l1, mu, y)
    assert torch.equal(za, zb) and torch.equal(pa, pb)
    # a sub-batch: other workgroups, other teams, other neighbours -- the same bits
    rs, ls, _, _ = ops.blocks_factor(ctx, blocks[10:50].contiguous())
    assert torch.equal(rs, r1[10:50]) and torch.equal(ls, l1[10:50])
    zs, ps = ops.blocks_logpdf(ctx, rs, ls, mu[10 * q:50 * q].contiguous(), y[10 * q:50 * q].contiguous())
    assert torch.equal(zs, za[10:50]) and torch.equal(ps, pa[10:50])
    ds = ops.blocks_draw(ctx, rs, mu[10 * q:50 * q].contiguous(), eps[:, 10 * q:50 * q].contiguous())
    assert torch.equal(ds, ops.blocks_draw(ctx, r1, mu, eps)[:, 10 * q:50 * q])


# ------------------------------------------------------------------ GPU 6: a block that is not positive definite
@gpu
def test_a_failed_pivot_is_flagged_and_touches_no_other_block(dsvgp, gpu_device):
    ops, ctx = _ctx(dsvgp, gpu_device)
    B, q = 37, 2
    good, _, _ = synthetic(B, q)
    ref, ref_ld, _, _ = ops.blocks_factor(ctx, good.to(gpu_device))
    singular, indefinite = torch.tensor([[1.0, 1.0], [1.0, 1.0]]), torch.tensor([[1.0, 2.0], [2.0, 1.0]])
    both = good.clone()
    both[17], both[18] = singular, indefinite
    roots, logdet, info, status = ops.blocks_factor(ctx, both.to(gpu_device))
    torch.cuda.synchronize()
    expect = torch.zeros(B, dtype=torch.int32)
    expect[17] = expect[18] = 2
    assert torch.equal(info.cpu(), expect) and int(status.item()) == 2
    assert bool(torch.isnan(roots[17:19]).all()) and bool(torch.isnan(logdet[17:19]).all())
    keep = [b for b in range(B) if b not in (17, 18)]
    assert torch.equal(roots[keep], ref[keep]) and torch.equal(logdet[keep], ref_ld[keep])
    # the engine's ladder: the singular block goes at the first jitter, the indefinite one never
    eng = dsvgp.ElboEngine(gpu_device)
    one = good.clone()
    one[17] = singular
    r, ld = eng.block_roots(one.to(gpu_device))
    assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(ld).all())
    r0, _, _, st0 = ops.blocks_factor(ctx, one.to(gpu_device), eng.chol_jitter)
    assert int(st0.item()) == 0 and torch.equal(r, r0)                                 # the first jitter, chol_jitter 10^0
    with pytest.raises(dsvgp.NotPSDError, match="Matrix not positive definite after repeatedly adding jitter"):
        eng.block_roots(both.to(gpu_device))
    with pytest.raises(TypeError):
        eng.block_roots(good.double().to(gpu_device))
    # the C entry's argument checks
    import ctypes as C
    lib = dsvgp._lib.lib
    g = good.to(gpu_device)
    vp = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    mu = torch.zeros(B * q, device=gpu_device)
    eps = torch.zeros(3, B * q, device=gpu_device)
    out = torch.empty(3, B * q, device=gpu_device)
    z, lp = torch.empty(B, q, device=gpu_device), torch.empty(B, device=gpu_device)

    def factor(blocks=g, B_=B, q_=q, roots_=roots, logdet_=logdet, info_=info, status_=status):
        return lib.dsvgp_blocks_factor(ctx.h, vp(blocks), B_, q_, 0.0, vp(roots_), vp(logdet_), vp(info_), vp(status_))

    def draw(roots_=ref, mu_=mu, eps_=eps, B_=B, q_=q, n=3, out_=out):
        return lib.dsvgp_blocks_draw(ctx.h, vp(roots_), vp(mu_), vp(eps_), B_, q_, n, vp(out_))

    def logpdf(roots_=ref, logdet_=ref_ld, mu_=mu, y_=mu, B_=B, q_=q, z_=z, lp_=lp):
        return lib.dsvgp_blocks_logpdf(ctx.h, vp(roots_), vp(logdet_), vp(mu_), vp(y_), B_, q_, vp(z_), vp(lp_))

    assert factor() == 0 and draw() == 0 and logpdf() == 0 and logpdf(z_=None) == 0
    assert factor(B_=0) == 0 and draw(B_=0) == 0 and draw(n=0) == 0 and logpdf(B_=0) == 0
    assert factor(blocks=None) == -1 and factor(roots_=None) == -1 and factor(logdet_=None) == -1 and factor(info_=None) == -1
    assert factor(status_=None) == -1 and factor(B_=-1) == -1 and factor(q_=0) == -1 and factor(q_=97) == -1
    assert draw(roots_=None) == -1 and draw(mu_=None) == -1 and draw(eps_=None) == -1 and draw(out_=None) == -1
    assert draw(B_=-1) == -1 and draw(n=-1) == -1 and draw(q_=0) == -1 and draw(q_=97) == -1
    assert logpdf(roots_=None) == -1 and logpdf(logdet_=None) == -1 and logpdf(mu_=None) == -1 and logpdf(y_=None) == -1
    assert logpdf(lp_=None) == -1 and logpdf(B_=-1) == -1 and logpdf(q_=0) == -1 and logpdf(q_=97) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------ GPU 7, 8: engine and model layer
def model_from(dsvgp, P, dev, ciq=False):
    """a model and a likelihood that carry the parameters of ``make_problem`` (directional at p > 0, the plain SVGP at p = 0)"""
    Z, V = P["inducing_points"], P["inducing_directions"]
    if V.shape[0]:
        kw = dict(variational_distribution="NGD", variational_strategy="CIQ") if ciq else {}
        model = dsvgp.GPModel(Z.clone(), V.clone(), Z.shape[1], **kw)
    else:
        model = dsvgp.traditional_vi.GPModel(Z.clone())
    likelihood = dsvgp.GaussianLikelihood()
    vd = model.variational_strategy._variational_distribution
    with torch.no_grad():
        for name in ("variational_mean", "chol_variational_covar", "natural_vec", "natural_mat"):
            if name in P:
                getattr(vd, name).copy_(P[name])
        model.mean_module.constant.copy_(P["constant"])
        model.covar_module.raw_outputscale.copy_(P["raw_outputscale"])
        model.covar_module.base_kernel.raw_lengthscale.copy_(P["raw_lengthscale"])
        likelihood.noise_covar.raw_noise.copy_(P["raw_noise"])
    model, likelihood = model.to(dev), likelihood.to(dev)
    model.eval()
    likelihood.eval()
    return model, likelihood


MODEL_CASES = [(12, 3, 2, 3, 20), (12, 3, 0, 3, 20), (10, 5, 2, 0, 33)]              # (M, d, p, pd, B)
MODEL_IDS = ["M%d-d%d-p%d-pd%d-B%d" % c for c in MODEL_CASES]


@functools.lru_cache(maxsize=None)
def model_case(case):
    """(P, x, D [B pd, d], y [B, pd + 1], all-float64 mean and blocks with the likelihood's noise): once per case, shared, never changed"""
    M, d, p, pd, B = case
    P, x, _, _, _ = make_problem(300, d, M, p, B, seed=1)
    D = torch.eye(d)[:pd].repeat(B, 1)
    P64 = {k: v.double() for k, v in P.items()}
    mu, Sigma, _ = rect_predictive(P64, x.double(), D.double(), pd)
    q = pd + 1
    noise = float(O.constrained(P64)[2])
    blocks = torch.stack([Sigma[b * q:(b + 1) * q, b * q:(b + 1) * q] for b in range(B)]) + noise * torch.eye(q, dtype=f64)
    g = torch.Generator().manual_seed(17)
    Lb = torch.linalg.cholesky(blocks)
    y = (mu.reshape(B, q) + torch.einsum("bac,bc->ba", Lb, torch.randn(B, q, dtype=f64, generator=g))).float()
    return P, x, D, y, mu, blocks


@gpu
@pytest.mark.parametrize("case", MODEL_CASES, ids=MODEL_IDS)
def test_model_layer_roots_and_density(dsvgp, gpu_device, case):
    M, d, p, pd, B = case
    q = pd + 1
    P, x, D, y, mu64, blocks64 = model_case(case)
    model, likelihood = model_from(dsvgp, P, gpu_device)
    xg, Dg = x.to(gpu_device), (D.to(gpu_device) if pd else None)
    with torch.no_grad():
        preds = model.posterior(xg, Dg, likelihood)
        roots, logdet = preds.point_roots
        assert preds.point_roots[0] is roots                                           # cached
        blocks, mean = preds.point_covariances, preds.mean
        logp, z = preds.point_log_prob(y.to(gpu_device)), preds.point_whitened_residuals(y.reshape(-1).to(gpu_device))
    assert roots.shape == (B, q, q) and roots.dtype == f64 and logdet.shape == (B,) and logp.shape == (B,) and z.shape == (B, q)
    # the new code alone: the yardstick on the GPU's own float32 mean and blocks
    A, L_ref, logdet_ref, kappa = yardstick(blocks)
    L = roots.cpu()
    rec = ((L @ L.transpose(1, 2) - A).abs() / bound_reconstruction(L, q)).max().item()
    z_ref, logp_ref = yardstick_density(L_ref, mean, y)
    rz, rl = check_density(z, logp, z_ref, logp_ref, kappa, q)
    # the whole chain against float64: first-order bound on the change of the log-density under the blocks' accepted error 5e-4
    z64, logp64 = yardstick_density(torch.linalg.cholesky(blocks64), mu64, y)
    inv2 = 1.0 / torch.linalg.eigvalsh(blocks64)[:, 0]
    first = (q + (z64 * z64).sum(-1)) * inv2 * q * 5e-4 * blocks64.abs().max()
    diff = (logp.cpu().double() - logp64).abs()
    errs = {"reconstruction / bound": rec, "z / bound": rz, "logp / bound": rl, "logp vs float64": diff.max().item(),
            "first-order bound": first.min().item(), "logp vs float64 / bound": (diff / first).max().item()}
    if pd == 0:                                                                        # the closed form on predict's (mu, varn)
        with torch.no_grad():
            old = model.posterior(xg, None, likelihood)
            cf = closed_form_1d(old.mean, old.variance, y)
        errs["closed form / bound"] = ((logp.cpu().double() - cf).abs() / (2.0 ** -22 * cf.abs().clamp_min(1.0))).max().item()
    _report("model layer %s" % (case,), errs)
    assert rec <= 1.0 and rz <= 1.0 and rl <= 1.0, errs
    assert errs["logp vs float64 / bound"] <= 1.0, errs
    assert errs.get("closed form / bound", 0.0) <= 1.0, errs


@gpu
def test_sampling_at_the_model_layer(dsvgp, gpu_device):
    case = MODEL_CASES[0]
    M, d, p, pd, B = case
    q = pd + 1
    P, x, D, _, _, _ = model_case(case)
    model, likelihood = model_from(dsvgp, P, gpu_device)
    xg, Dg = x.to(gpu_device), D.to(gpu_device)
    preds = model.posterior(xg, Dg, likelihood)
    s = preds.sample_points(torch.Size([5]))
    assert s.shape == (5, B * q) and s.dtype == f32 and bool(torch.isfinite(s).all())
    assert preds.sample_points().shape == (B * q,) and preds.rsample_points(torch.Size([2, 3])).shape == (2, 3, B * q)
    assert torch.equal(preds.sample_points(torch.Size([5]), base_samples=torch.zeros(5, B * q)), preds.mean.expand(5, -1))
    # sample_gradients: shapes, posterior_gradient's means at zero base samples, the noise in the reconstructed covariance
    with torch.no_grad():
        pg = model.posterior_gradient(xg, likelihood)
        values, grads = model.sample_gradients(xg, 4, likelihood, base_samples=torch.zeros(4, B * (d + 1)))
    assert values.shape == (4, B) and grads.shape == (4, B, d)
    assert torch.equal(values, pg.value_mean.expand(4, -1)) and torch.equal(grads, pg.gradient_mean.expand(4, -1, -1))
    v, g = model.sample_gradients(xg, 3)
    assert v.shape == (3, B) and g.shape == (3, B, d) and bool(torch.isfinite(g).all())
    unit = torch.eye(d + 1).repeat(1, B)                                               # draw c: mean + column c of every root

    def covariance(lik):
        vv, gg = model.sample_gradients(xg, d + 1, lik, base_samples=unit)
        with torch.no_grad():
            m = model.posterior_gradient(xg, lik)
        cols = torch.cat([vv.unsqueeze(-1), gg], -1).double() - torch.cat([m.value_mean.unsqueeze(-1), m.gradient_mean], -1).double()
        Lr = cols.permute(1, 2, 0)                                                     # [b, a, c]
        return (Lr @ Lr.transpose(1, 2)).cpu()

    noise = float(O.constrained({k: v.double() for k, v in P.items()})[2])
    dn = covariance(likelihood) - covariance(None)
    err = (dn - noise * torch.eye(d + 1, dtype=f64)).abs().max().item()
    # every column is the float32 rounding of mean + L e_c, so an entry of the reconstructed L carries 2^-23 (|mean| + |L|) and one of
    # L L^T 2 q |L| times that, in both covariances; q(f)'s blocks are float32 differences, 2^-23 |Sigma| more
    with torch.no_grad():
        m = model.posterior_gradient(xg, likelihood)
    big_l = covariance(likelihood).diagonal(dim1=1, dim2=2).max().sqrt().item()
    big_m = max(m.value_mean.abs().max().item(), m.gradient_mean.abs().max().item())
    tol = 2.0 ** -23 * (4 * (d + 1) * big_l * (big_m + big_l) + 2 * big_l * big_l)
    print("[parity] noise in the reconstructed covariance: %.3e (tolerance %.3e, noise %.3e)" % (err, tol, noise))
    assert err <= tol, (err, tol)
    # q(f) with two identical direction rows: a singular block, through the ladder, finite samples
    twice = torch.eye(d)[[0, 0]].repeat(B, 1).to(gpu_device)
    qf = model.posterior(xg, twice)
    s = qf.sample_points(torch.Size([5]))
    assert s.shape == (5, B * 3) and bool(torch.isfinite(s).all()) and bool(torch.isfinite(qf.point_roots[0]).all())


# ------------------------------------------------------------------ GPU 9: the harness
def _dataset(d, n=50, seed=23):
    from torch.utils.data import TensorDataset
    X = torch.rand(n, d, generator=torch.Generator().manual_seed(seed))
    return TensorDataset(X, O.testfun(X)), X, O.testfun(X)


@gpu
def test_eval_gradient_nll(dsvgp, gpu_device):
    from dsvgp_amd import directional_vi, shared_directional_vi
    assert dsvgp.eval_gradient_nll is directional_vi.eval_gradient_nll is shared_directional_vi.eval_gradient_nll
    M, d, p, pd, B = MODEL_CASES[0]
    P = model_case(MODEL_CASES[0])[0]
    model, likelihood = model_from(dsvgp, P, gpu_device)
    ds, X, Y = _dataset(d)
    out = dsvgp.eval_gradient_nll(ds, model, likelihood, minibatch_size=16)
    assert out._fields == ("nll", "whitened", "value_nll")
    assert out.nll.shape == (50,) and out.whitened.shape == (50, d + 1) and out.value_nll.shape == (50,) and out.nll.is_cuda
    Xg, Yg = X.to(gpu_device), Y.to(gpu_device)
    with torch.no_grad():
        parts = torch.cat([model.gradient_log_prob(Xg[s:s + 16], Yg[s:s + 16], likelihood) for s in range(0, 50, 16)])
        whole = model.gradient_log_prob(Xg, Yg, likelihood)
        pg = model.posterior_gradient(Xg, likelihood)
    assert torch.equal(out.nll, -parts)
    print("[parity] eval_gradient_nll in batches of 16 vs one call on the whole set: %.3e" % (out.nll + whole).abs().max().item())
    assert torch.equal(out.nll, -whole)
    cf = closed_form_1d(pg.value_mean, pg.value_variance, Y[:, 0])
    r = ((-out.value_nll.cpu().double() - cf).abs() / (2.0 ** -22 * cf.abs().clamp_min(1.0))).max().item()
    print("[parity] value_nll vs the q = 1 closed form (error / bound): %.3e" % r)
    assert r <= 1.0
    assert bool(torch.isfinite(out.whitened).all())
    with pytest.raises(ValueError, match="d \\+ 1"):
        from torch.utils.data import TensorDataset
        dsvgp.eval_gradient_nll(TensorDataset(X, Y[:, :2].contiguous()), model, likelihood, minibatch_size=16)


@gpu
def test_eval_gradient_nll_ciq_is_diagonal_and_float64_is_refused(dsvgp, gpu_device):
    from test_ngd import make_ngd_problem
    d = 3
    Pn, _, _, _, _ = make_ngd_problem(300, d, 12, d, 20)                               # CIQ predicts at pd == p: a model with p = d
    model, likelihood = model_from(dsvgp, Pn, gpu_device, ciq=True)
    ds, X, Y = _dataset(d)
    out = dsvgp.eval_gradient_nll(ds, model, likelihood, minibatch_size=16)
    assert out.nll.shape == (50,) and out.whitened.shape == (50, d + 1) and out.value_nll.shape == (50,)
    with torch.no_grad():
        terms = []
        for s in range(0, 50, 16):
            xb = X[s:s + 16].to(gpu_device)
            post = model.posterior(xb, torch.eye(d, device=gpu_device).repeat(xb.shape[0], 1), likelihood)
            terms.append(closed_form_1d(post.mean, post.variance, Y[s:s + 16]).reshape(-1, d + 1))
    terms = torch.cat(terms)
    ref = -terms.sum(-1)
    r = ((out.nll.cpu().double() - ref).abs() / (2.0 ** -22 * ref.abs().clamp_min(1.0))).max().item()
    r1 = ((out.value_nll.cpu().double() + terms[:, 0]).abs() / (2.0 ** -22 * terms[:, 0].abs().clamp_min(1.0))).max().item()
    print("[parity] CIQ: nll vs the sum of the per-output terms (error / bound) %.3e, value_nll %.3e" % (r, r1))
    assert r <= 1.0 and r1 <= 1.0
    # a float64 model: what predict_blocks raises
    P, _, _, _, _ = make_problem(300, d, 12, 2, 20, seed=1)
    default = torch.get_default_dtype()
    torch.set_default_dtype(f64)
    try:
        m64, l64 = model_from(dsvgp, {k: v.double() for k, v in P.items()}, gpu_device)
    finally:
        torch.set_default_dtype(default)
    with pytest.raises(NotImplementedError, match="float64"):
        dsvgp.eval_gradient_nll(ds, m64, l64, minibatch_size=16)


# ------------------------------------------------------------------ GPU 10: memory
@gpu
def test_point_log_prob_allocates_the_roots_and_nothing_of_the_size_of_the_joint_covariance(dsvgp, gpu_device):
    """d 5, M 16, p 1, pd 5, B 4096 (the shape of test_gpu_blocks' memory test, which holds predict_blocks to 512 MB): one
    point_log_prob call may add the roots B q^2 8 and B q 16 bytes of vectors to that"""
    dev = gpu_device
    d, M, p, pd, B = 5, 16, 1, 5, 4096
    q = pd + 1
    P, x, _, _, _ = make_problem(4200, d, M, p, B, seed=1)
    model, likelihood = model_from(dsvgp, P, dev)
    xg = x.to(dev)
    Dg = torch.randn(B * pd, d, generator=torch.Generator().manual_seed(5)).to(dev)
    yg = torch.randn(B, q, generator=torch.Generator().manual_seed(6)).to(dev)
    with torch.no_grad():
        model.posterior(xg, Dg, likelihood).point_log_prob(yg)                         # warm-up: the engine's buffers exist
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.max_memory_allocated(dev)
        logp = model.posterior(xg, Dg, likelihood).point_log_prob(yg)
        torch.cuda.synchronize()
    raised = torch.cuda.max_memory_allocated(dev) - before
    allowed = B * q * q * 8 + B * q * 16 + 512 * 2 ** 20
    print("[parity] peak raised by %.1f MB (allowed %.1f MB, joint covariance %.1f MB)" % (raised / 2 ** 20, allowed / 2 ** 20, (B * q) ** 2 * 4 / 2 ** 20))
    assert logp.shape == (B,) and bool(torch.isfinite(logp).all())
    assert raised <= allowed
