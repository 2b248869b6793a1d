"""Missing observations on the GPU (csrc/missing.hip, ``ElboEngine.missing_targets``) against the float64
reference of tests/_missing_ref.py, which DELETES the rows whose target is NaN.

Step cases (tests/_missing_ref.py: CASES) are small shapes where the kernels can go wrong: M' = 72 and 129 (crossing a 64-tile), B = 37 with
pd = 2 (ragged B' = 111), d = 3, one d = 100 case, one ARD, one Matern-5/2 and one rectangular (pd != p) case.  Collapsed cases are those
of tests/_collapsed_ref.py (a: M' = 72, b: M' = 129, e: rectangular, f: d = 100, g: ARD, h: Matern-5/2) with the same seeded pattern.
tests/test_missing_host.py runs every case through the reference on the CPU first (finite, no jitter step).

Tolerances are the committed ones for the same quantities: step loss 2e-5 relative, mean / variance 2e-4, gradients 2e-3 of the largest
entry (tests/test_gpu_rect_train.py, test_gpu_ard.py, test_gpu_matern.py); collapsed loss 2e-5 and gradients 2e-3
(tests/test_gpu_collapsed_grad.py); statistics against the reference 1e-2 of the largest entry and across chunkings 1e-10 of |A| |A|^T
(tests/test_gpu_collapsed.py).  The prior-diagonal sum is a float64 sum of float32 entries: 2e-5, the project's kernel tolerance; yy is
a float64 sum of the same float32 numbers on both sides: 1e-10.  Measured errors are printed as [parity] lines."""
import functools
import math

import pytest
import torch

import dsvgp_oracle as O
import _collapsed_ref as R
import _missing_ref as MR
from test_gpu_rect_train import GRAD_TOL, LOSS_TOL, MU_TOL, VAR_TOL

pytestmark = pytest.mark.gpu
STEP_NAMES = sorted(MR.CASES)
COLLAPSED_NAMES = ["a", "b", "e", "f", "g", "h"]
NAN = float("nan")


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _report(tag, errs):
    print("[parity] %s: %s" % (tag, ", ".join("%s %.2e" % (k, v) for k, v in errs.items())))


def _engine(dsvgp, dev, kernel, missing=True):
    eng = dsvgp.ElboEngine(dev)
    eng.kernel = "matern52" if kernel == "matern52" else "rbf"
    eng.missing_targets = missing
    return eng


@functools.lru_cache(maxsize=None)
def _case(name, pattern):
    """(params, x, y with the pattern's NaNs, D, num_data, kernel, pd, p): once per case and pattern, shared, never changed"""
    P, x, y, D, nd, kernel = MR.problem(name)
    p, pd = MR.CASES[name][3], MR.CASES[name][4]
    if pattern == "random":
        y = MR.random_pattern(y, pd)
    elif pattern == "derivatives":
        y = MR.derivatives_missing(y, pd)
    elif pattern == "all":
        y = torch.full_like(y, NAN)
    return P, x, y, D, nd, kernel, pd, p


@functools.lru_cache(maxsize=None)
def _reference(name, pattern, mll):
    P, x, y, D, nd, kernel, _, _ = _case(name, pattern)
    return MR.step(P, x, y, D, nd, mll, kernel)


def _run(dsvgp, dev, name, pattern, mll, missing=True, fast=None):
    P, x, y, D, nd, kernel, pd, p = _case(name, pattern)
    eng = _engine(dsvgp, dev, kernel, missing)
    out = eng.loss_and_grads({k: v.to(dev) for k, v in P.items()}, x.to(dev), y.to(dev), D.to(dev), nd, mll, fast=fast)
    torch.cuda.synchronize()
    return eng, out


def _step_errors(out, ref, p):
    loss, grads, mu, varn = out
    l_ref, g_ref, mu_ref, var_ref, keep = ref
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu.cpu()[keep], mu_ref),
            "varn": relmax(varn.cpu()[keep], var_ref)}
    for k in O.PARAM_NAMES:
        if p == 0 and k == "inducing_directions":
            continue
        errs[k] = relmax(grads[k].reshape(-1), g_ref[k].reshape(-1))
    return errs


def _assert_step(tag, errs, scale=1.0):
    _report(tag, errs)
    assert errs["loss"] < scale * LOSS_TOL and errs["mu"] < scale * MU_TOL and errs["varn"] < scale * VAR_TOL, errs
    for k in O.PARAM_NAMES:
        assert errs.get(k, 0.0) < scale * GRAD_TOL, (k, errs)


# ------------------------------------------------------------------ 1. a random pattern against the reference on deleted columns
@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
@pytest.mark.parametrize("name", STEP_NAMES)
def test_random_pattern_matches_the_reference(dsvgp, gpu_device, name, mll):
    P, x, y, D, nd, kernel, pd, p = _case(name, "random")
    q = pd + 1
    miss = torch.isnan(y)
    assert bool(miss[:q].all()) and bool(miss[q]) and not bool(miss[q + 1:2 * q].any())       # a whole point; a value alone
    assert 0.2 < miss.double().mean().item() < 0.4
    eng, out = _run(dsvgp, gpu_device, name, "random", mll)
    loss, grads, mu, varn = out
    assert eng.c_step_used is False and eng.present_rows.item() == int((~miss).sum())
    assert mu.shape == y.shape and bool(torch.isfinite(mu).all())
    assert bool((varn.cpu()[miss] == 0).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and math.isfinite(loss.item())
    _assert_step("missing step %s %s (%d of %d rows present)" % (name, mll, int((~miss).sum()), y.numel()),
                 _step_errors(out, _reference(name, "random", mll), p))


# ------------------------------------------------------------------ 2. all derivative rows missing against the value-only rectangular step
@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
def test_all_derivatives_missing_against_the_value_only_step(dsvgp, gpu_device, mll):
    dev = gpu_device
    P, x, y, D, nd, kernel, pd, p = _case("m72", "derivatives")
    ref = _reference("m72", "derivatives", mll)
    _, masked = _run(dsvgp, dev, "m72", "derivatives", mll)
    y0 = y.reshape(-1, pd + 1)[:, 0].contiguous()
    plain = _engine(dsvgp, dev, kernel, missing=False).loss_and_grads({k: v.to(dev) for k, v in P.items()}, x.to(dev), y0.to(dev), None, nd,
                                                                      mll, fast=False)
    torch.cuda.synchronize()
    _assert_step("derivatives missing, masked %s" % mll, _step_errors(masked, ref, p))
    ref_plain = ref[:4] + (torch.ones(y0.numel(), dtype=torch.bool),)
    _assert_step("derivatives missing, D = None %s" % mll, _step_errors(plain, ref_plain, p))
    sub = (masked[0], masked[1], masked[2][::pd + 1], masked[3][::pd + 1])
    mutual = _step_errors(sub, (plain[0].cpu().double(), {k: v.cpu().double() for k, v in plain[1].items()}, plain[2].cpu().double(),
                                plain[3].cpu().double(), torch.ones(y0.numel(), dtype=torch.bool)), p)
    _assert_step("derivatives missing, masked vs D = None %s" % mll, mutual, scale=2.0)          # (triangle inequality)


# ------------------------------------------------------------------ 3. nothing missing, switch on
@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
@pytest.mark.parametrize("name", ["m72", "rect", "ard"])
def test_nothing_missing_is_the_per_output_path(dsvgp, gpu_device, name, mll):
    _, on = _run(dsvgp, gpu_device, name, "none", mll)
    eng_off, off = _run(dsvgp, gpu_device, name, "none", mll, missing=False, fast=False)
    assert torch.equal(on[2], off[2]) and torch.equal(on[3], off[3])                             # mu, varn: bitwise
    p = _case(name, "none")[7]
    _assert_step("nothing missing, switch on, %s %s" % (name, mll), _step_errors(on, _reference(name, "none", mll), p))
    errs = {"loss": abs(on[0].item() - off[0].item()) / abs(off[0].item())}
    for k in O.PARAM_NAMES:
        errs[k] = relmax(on[1][k].reshape(-1), off[1][k].reshape(-1))
    _report("nothing missing, on vs off, %s %s" % (name, mll), errs)
    assert errs["loss"] < 2 * LOSS_TOL and all(errs[k] < 2 * GRAD_TOL for k in O.PARAM_NAMES), errs


# ------------------------------------------------------------------ 4. everything missing
@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
@pytest.mark.parametrize("name", ["m72", "ard"])
def test_everything_missing_leaves_the_kl_term(dsvgp, gpu_device, name, mll):
    dev = gpu_device
    P, x, y, D, nd, kernel, pd, p = _case(name, "all")
    eng, (loss, grads, mu, varn) = _run(dsvgp, dev, name, "all", mll)
    ops = dsvgp._ops
    Mp = P["variational_mean"].shape[0]
    kl_buf = torch.zeros(2 * Mp + 1, device=dev)
    dm, dLS = torch.zeros(Mp, device=dev), torch.zeros(Mp, Mp, device=dev)
    ops.kl_terms(ops.Context.get(dev), P["variational_mean"].to(dev), P["chol_variational_covar"].to(dev).contiguous(), nd, kl_buf, dm, dLS)
    torch.cuda.synchronize()
    assert eng.present_rows.item() == 0
    assert loss.item() == (kl_buf[0] * torch.tensor(1.0 / nd, dtype=torch.float32, device=dev)).item()      # KL / num_data, the epilogue's product
    assert bool((varn == 0).all()) and bool(torch.isfinite(mu).all())
    for k in ("inducing_points", "inducing_directions", "constant", "raw_outputscale", "raw_lengthscale", "raw_noise"):
        assert bool((grads[k] == 0).all()), k                                                    # the data side: exactly 0
    assert torch.equal(grads["variational_mean"], dm) and torch.equal(grads["chol_variational_covar"], dLS)      # the KL term's own
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())


# ------------------------------------------------------------------ 7. reproducibility of the masked kernel
@pytest.mark.parametrize("mll_type", [0, 1])
def test_masked_likelihood_terms_are_reproducible_and_exactly_zero_on_missing_rows(dsvgp, gpu_device, mll_type):
    dev = gpu_device
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    g = torch.Generator().manual_seed(4)
    n, p = 256 * 512 + 77, 2                                   # more than one grid-stride round of the 512 workgroups, ragged
    mu, var = torch.randn(n, generator=g).to(dev), (0.1 + torch.rand(n, generator=g)).to(dev)
    y = torch.randn(n, generator=g)
    miss = torch.rand(n, generator=g) < 0.3
    y[miss] = NAN
    y = y.to(dev)
    hyp = torch.tensor([0.7, 1.3, 0.2, 0.0], device=dev)

    def run():
        outs = [torch.full((n,), 9.0, device=dev) for _ in range(3)]
        scal, cnt = torch.full((8,), 9.0, device=dev), torch.full((1,), -1, dtype=torch.int32, device=dev)
        ops.likelihood_terms_masked(ctx, mu, var, y, p, hyp, mll_type, *outs, scal, cnt, ops.likelihood_terms_masked_workspace(dev))
        return outs + [scal, cnt]
    a, b = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    md = miss.to(dev)
    assert a[4].item() == int((~miss).sum()) and all(bool((t[md] == 0).all()) for t in a[:3]) and bool((a[3][5:] == 0).all())
    # against the unmasked entry on the present rows alone (same p-pattern is not kept by a gather: only the sums that do not depend on it)
    keep = (~miss).to(dev)
    k = int(keep.sum())
    mb, scal = [torch.empty(k, device=dev) for _ in range(3)], torch.empty(8, device=dev)
    ops.likelihood_terms(ctx, mu[keep].contiguous(), var[keep].contiguous(), y[keep].contiguous(), p, hyp, mll_type, float(k), mb[0], mb[1], mb[2], scal)
    torch.cuda.synchronize()
    assert relmax(a[0][keep], mb[0]) < 1e-6 and relmax(a[1][keep], mb[1]) < 1e-6 and torch.equal(a[2][keep], mb[2])
    assert abs(a[3][0].item() * k - scal[0].item()) <= 1e-5 * abs(scal[0].item()) and relmax(a[3][1:3], scal[1:3]) < 1e-4
    # an empty batch: no launch, cleared outputs; refusals
    scal0, cnt0 = torch.full((8,), 9.0, device=dev), torch.full((1,), -1, dtype=torch.int32, device=dev)
    lib = dsvgp._lib.lib
    P_ = lambda t: t.data_ptr()
    ws = ops.likelihood_terms_masked_workspace(dev)
    before = [t.clone() for t in a[:3]]
    assert lib.dsvgp_likelihood_terms_masked(ctx.h, P_(mu), P_(var), P_(y), 0, p, P_(hyp), mll_type, P_(a[0]), P_(a[1]), P_(a[2]), P_(scal0),
                                             P_(cnt0), P_(ws)) == 0
    assert cnt0.item() == 0 and bool((scal0 == 0).all()) and all(torch.equal(u, v) for u, v in zip(before, a[:3]))
    assert lib.dsvgp_likelihood_terms_masked(ctx.h, P_(mu), P_(var), P_(y), -1, p, P_(hyp), mll_type, P_(a[0]), P_(a[1]), P_(a[2]), P_(a[3]),
                                             P_(a[4]), P_(ws)) == -1
    assert lib.dsvgp_likelihood_terms_masked(ctx.h, P_(mu), P_(var), P_(y), n, p, P_(hyp), 2, P_(a[0]), P_(a[1]), P_(a[2]), P_(a[3]),
                                             P_(a[4]), P_(ws)) == -1


# ------------------------------------------------------------------ 5. collapsed statistics, solve, evaluate and the backward pass
@functools.lru_cache(maxsize=None)
def _collapsed_case(name):
    P, x, y, D, nd, _, _, kernel = R.problem(name)
    pd = 0 if D is None else D.shape[0] // x.shape[0]
    y = MR.random_pattern(y, pd, seed=3)
    return P, x, y, D, nd, kernel, pd, MR.collapsed(P, x, y, D, nd, kernel)


def _accumulate(dsvgp, dev, name, cuts):
    P, x, y, D, nd, kernel, pd, _ = _collapsed_case(name)
    eng = _engine(dsvgp, dev, kernel)
    Pg = {k: v.to(dev) for k, v in P.items()}
    acc = eng.collapsed_accumulator(Pg)
    xg, yg, Dg = x.to(dev), y.to(dev), D.to(dev)
    q = pd + 1
    bounds = [0] + list(cuts) + [x.shape[0]]
    chunks = [(xg[lo:hi], yg[lo * q:hi * q], Dg[lo * pd:hi * pd] if pd else None) for lo, hi in zip(bounds[:-1], bounds[1:])]
    for c in chunks:
        acc.add(*c)
    return acc, chunks


@pytest.mark.parametrize("name", COLLAPSED_NAMES)
def test_collapsed_matches_the_reference_on_deleted_columns(dsvgp, gpu_device, name):
    dev = gpu_device
    P, x, y, D, nd, kernel, pd, ref = _collapsed_case(name)
    stats = ref["stats"]
    present = int((~torch.isnan(y)).sum())
    assert R.cond_B(stats, num_data=nd) < 1e4
    acc, chunks = _accumulate(dsvgp, dev, name, (x.shape[0] // 3,))
    other, _ = _accumulate(dsvgp, dev, name, (x.shape[0] - 17,))
    G, b, yy, dg, Rr = (t.cpu() for t in acc.statistics())
    G2, b2, yy2, dg2, R2 = (t.cpu() for t in other.statistics())
    assert Rr.item() == present == R2.item() == stats["R"] and acc.rows == y.numel()
    errs = {"G": relmax(torch.tril(G), torch.tril(stats["G"])), "b": relmax(b, stats["b"]), "yy": abs(yy.item() - stats["yy"].item()) / stats["yy"].item(),
            "dg": abs(dg.item() - stats["dg"].item()) / stats["dg"].item()}
    _report("masked statistics %s" % name, errs)
    assert errs["G"] < 1e-2 and errs["b"] < 1e-2 and errs["yy"] < 1e-10 and errs["dg"] < 2e-5, errs
    scale = stats["absG"].max().item()                                                           # where the chunks are cut changes nothing
    assert (torch.tril(G) - torch.tril(G2)).abs().max().item() <= 1e-10 * scale
    assert (b - b2).abs().max().item() <= 1e-10 * max(b2.abs().max().item(), scale)
    assert abs(yy.item() - yy2.item()) <= 1e-10 * abs(yy2.item()) and abs(dg.item() - dg2.item()) <= 1e-10 * abs(dg2.item())
    # solve, and the default num_data = R
    res = acc.solve(nd)
    e_loss = abs(res.loss - ref["loss"].item()) / abs(ref["loss"].item())
    t = res.terms
    print("[parity] masked solve %s: loss %.2e (ll %.6f ref %.6f, kl %.6f ref %.6f)"
          % (name, e_loss, t["log_likelihood"], ref["terms"]["ll"].item(), t["kl"], ref["terms"]["kl"].item()))
    assert e_loss <= LOSS_TOL and t["rows"] == present
    assert abs(t["loss"] + (t["log_likelihood"] / t["rows"] - t["kl"] / nd)) <= 1e-12 * abs(t["loss"])
    assert acc.solve().num_data == float(present)
    res = acc.solve(nd)
    # evaluate at a fixed q(u)
    g = torch.Generator().manual_seed(17)
    n = acc.Mp
    m, L_S = 0.3 * torch.randn(n, generator=g), torch.tril(torch.eye(n) + 0.05 * torch.randn(n, n, generator=g))
    got, want = acc.evaluate(m.to(dev), L_S.to(dev), nd).terms, R.terms(stats, m, L_S, num_data=nd)
    e_eval = {k: abs(got[a] - want[k].item()) / abs(want[k].item()) for k, a in (("loss", "loss"), ("ll", "log_likelihood"), ("kl", "kl"),
                                                                                  ("residual", "residual"), ("varn", "varn"))}
    _report("masked evaluate %s" % name, e_eval)
    assert all(v <= LOSS_TOL for v in e_eval.values()), e_eval
    # the backward pass over the same chunks
    acc.begin_backward(res)
    for c in chunks:
        acc.add_backward(*c)
    loss, grads = acc.finish_backward()
    e_grad = {k: relmax(grads[k].reshape(-1), ref["grads"][k].reshape(-1)) for k in grads if ref["grads"][k].numel()}
    _report("masked collapsed gradients %s" % name, e_grad)
    assert abs(loss - ref["loss"].item()) <= LOSS_TOL * abs(ref["loss"].item())
    assert all(v <= GRAD_TOL for v in e_grad.values()), e_grad


def test_masked_chunk_call_gives_exact_zeros(dsvgp, gpu_device):
    """K_ZX-bar columns, dg-bar and the share of rho_sum of the missing rows: exactly 0, and the call is reproducible"""
    dev = gpu_device
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    g = torch.Generator().manual_seed(9)
    Mp, Bp = 129, 111
    K = torch.randn(Mp, Bp, generator=g)
    y = torch.randn(Bp, generator=g)
    miss = torch.rand(Bp, generator=g) < 0.3
    y[miss] = NAN
    Q = torch.randn(Mp, Mp, generator=g, dtype=torch.float64)
    Q = (0.5 * (Q + Q.t())).to(dev)
    alpha = torch.randn(Mp, generator=g, dtype=torch.float64).to(dev)
    adj = torch.tensor([0.37, 0, 0.37, 0, 0, 0, 0, 0], dtype=torch.float64, device=dev)
    const = torch.tensor([0.3], device=dev)

    def run(masked, Kin, yin):
        Kd, Kb = Kin.to(dev).contiguous(), torch.full((Mp, Bp), 9.0, device=dev)
        dbar, rsum = torch.full((Bp,), 9.0, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
        nbytes = (ops.collapsed_grad_chunk_masked_bytes if masked else ops.collapsed_grad_chunk_bytes)(Mp, Bp)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        (ops.collapsed_grad_chunk_masked if masked else ops.collapsed_grad_chunk)(ctx, Mp, Kd, yin.to(dev), const, Q, alpha, adj, Kb, dbar, rsum, ws)
        torch.cuda.synchronize()
        return Kb.cpu(), dbar.cpu(), rsum.cpu()
    a, b = run(True, K, y), run(True, K, y)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert bool((a[0][:, miss] == 0).all()) and bool((a[1][miss] == 0).all()) and bool(torch.isfinite(a[0]).all())
    keep = ~miss
    Kz, yz = K.clone(), y.clone()                                                                # the sibling on inputs zeroed by hand
    Kz[:, miss] = 0.0
    yz[miss] = 0.3
    d = run(False, Kz, yz)
    assert torch.equal(a[0], d[0]) and torch.equal(a[2], d[2]) and torch.equal(a[1][keep], d[1][keep])


# ------------------------------------------------------------------ 6. the default is untouched
def test_switch_off_still_refuses_a_nan_target(dsvgp, gpu_device):
    dev = gpu_device
    P, x, y, D, nd, kernel, pd, _ = _collapsed_case("a")
    eng = _engine(dsvgp, dev, kernel, missing=False)
    acc = eng.collapsed_accumulator({k: v.to(dev) for k, v in P.items()})
    acc.add(x.to(dev), y.to(dev), D.to(dev))
    with pytest.raises(ValueError, match="not finite"):
        acc.solve(nd)
    name = "m72"
    _, out = _run(dsvgp, dev, name, "random", "ELBO", missing=False, fast=False)
    assert math.isnan(out[0].item())                                                             # (the step itself has no check: NaN in, NaN out)


# ------------------------------------------------------------------ 8. the harness
def _dataset(n, d, frac, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g)
    Y = O.testfun(X).clone()
    miss = torch.rand(n, d, generator=g) < frac
    Y[:, 1:][miss] = NAN                                                                         # gradients only: every value is present
    return torch.utils.data.TensorDataset(X, Y), X, Y


def test_train_gp_with_missing_gradients(dsvgp, gpu_device):
    dvi = dsvgp.directional_vi
    train, X, Y = _dataset(600, 3, 0.3, 0)
    kw = dict(num_inducing=24, num_directions=2, minibatch_size=150, minibatch_dim=2, num_epochs=20, learning_rate_hypers=0.02, seed=0,
              verbose=False)
    loop = dvi.setup_training(train, 24, 2, 150, 2, 20, 0.02, seed=0).set_missing_targets()
    present = float((~torch.isnan(Y)).sum()) / Y.numel()
    assert loop.model.missing_targets and loop.model.engine.missing_targets
    assert abs(loop.mll.num_data - 4 * 600 * present) <= 1e-9 * 4 * 600
    losses = []
    perm = loop.epoch_permutation()
    for step in range(48):
        start = (step % 4) * 150
        loss, _, _ = loop.step(perm[start:start + 150])
        losses.append(loss.item())
    loop.finish()
    assert all(math.isfinite(v) for v in losses)
    first, last = sum(losses[:8]) / 8, sum(losses[-8:]) / 8
    print("[missing] train_gp: loss %.4f -> %.4f over 48 steps" % (first, last))
    assert last < first
    torch.manual_seed(0)
    model, likelihood = dvi.train_gp(train, **kw, max_steps=4, missing_targets=True)
    assert model.missing_targets and all(bool(torch.isfinite(prm).all()) for prm in model.parameters())


def test_train_collapsed_with_missing_gradients(dsvgp, gpu_device):
    dvi = dsvgp.directional_vi
    train, X, Y = _dataset(300, 3, 0.3, 1)
    torch.manual_seed(0)
    model, likelihood = dvi.train_collapsed(train, num_inducing=24, num_directions=2, num_iterations=3, minibatch_size=128, seed=0,
                                            verbose=False, missing_targets=True)
    assert model.missing_targets and all(bool(torch.isfinite(prm).all()) for prm in list(model.parameters()) + list(likelihood.parameters()))
    res = dvi.fit_variational(model, likelihood, (X.to(gpu_device), Y.to(gpu_device)), minibatch_size=128, seed=0)
    assert math.isfinite(res.loss) and res.terms["rows"] < 300 * 3
