"""GPU parity tests of the wide-input assembly (packed width > 96, i.e. d >= 93: csrc/assemble_wide.hip) and of everything above it at
the input widths of the paper's Bayesian-optimisation runs (rover: d = 200; GCN on PubMed: d = 4035).

Inputs: X ~ U[0, 1]^d with the lengthscale 0.4 sqrt(d), so that the kernel between random points is ~0.6 (with the lengthscales of the
narrow tests, ~0.8, every off-diagonal entry at d = 200 would be ~e^-23 and a comparison would check zeros).  Tolerances are the ones
of the narrow tests (test_gpu_ops.py / test_gpu_step.py); the measured errors are printed as [parity] lines."""
import math
import os

import numpy as np
import pytest
import torch

import dsvgp_oracle as O
from _golden import GOLDEN, kernel_error
from test_gpu_step import make_problem

pytestmark = pytest.mark.gpu


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _report(tag, errs):
    print("[parity] %s: %s" % (tag, ", ".join("%s %.2e" % (k, v) for k, v in errs.items())))


def _ell(d):
    return 0.4 * math.sqrt(d)


def _raw(v):
    return math.log(math.expm1(v))          # softplus^-1


def _packs(dsvgp, dev, x1, x2, v1, v2, ell, s):
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    p = v1.shape[0] // x1.shape[0]
    hyp = torch.tensor([ell, s, 0.1, 0.0], dtype=torch.float32, device=dev)
    x1d = x1.float().to(dev).contiguous()
    center = ops.column_mean(ctx, x1d)
    p1 = ops.pack_points(ctx, x1d, v1.float().to(dev).contiguous(), p, hyp, center)
    p2 = ops.pack_points(ctx, x2.float().to(dev).contiguous(), v2.float().to(dev).contiguous(), p, hyp, center)
    return ctx, hyp, p1, p2


def _points(n1, n2, d, p, seed):
    g = torch.Generator().manual_seed(seed)
    x1, x2 = torch.rand(n1, d, generator=g), torch.rand(n2, d, generator=g)
    v1, v2 = torch.randn(n1 * p, d, generator=g), torch.randn(n2 * p, d, generator=g)
    return g, x1, x2, v1, v2


# ------------------------------------------------------------------ 1. forward against fp64
@pytest.mark.parametrize("d", [92, 93, 97, 128, 200, 1000, 4035])
@pytest.mark.parametrize("p", [0, 1, 3, 5, 10])
def test_kernel_fwd_at_wide_inputs_matches_fp64(dsvgp, gpu_device, d, p):
    """d = 92 is the control (the whole-row kernels); from 93 on kernel_fwd runs the wide kernels.  Ragged 37 x 53 points."""
    n1, n2 = 37, 53
    _, x1, x2, v1, v2 = _points(n1, n2, d, p, seed=d * 16 + p)
    ell, s = _ell(d), 1.7
    ctx, hyp, p1, p2 = _packs(dsvgp, gpu_device, x1, x2, v1, v2, ell, s)
    ref = s * O.kernel_matrix(x1.double(), x2.double(), v1.double(), v2.double(), ell)
    errs = {}
    for dt in (torch.float32, torch.float64):
        K = dsvgp._ops.kernel_fwd(ctx, p1, n1, p2, n2, d, p, hyp, dtype=dt)
        assert K.dtype == dt
        errs[str(dt)[6:]] = relmax(K, ref)
        assert errs[str(dt)[6:]] < 2e-5, (dt, errs)
    _report("kernel_fwd d=%d p=%d 37x53 vs fp64" % (d, p), errs)


# ------------------------------------------------------------------ 2. the wide kernels at small d: golden vectors and the whole-row kernels
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_kernel_fwd_wide_matches_reference_golden_vectors(dsvgp, gpu_device, path):
    g = np.load(path)
    t = lambda k: torch.from_numpy(g[k])
    x1, x2, v1, v2 = t("x1"), t("x2"), t("v1"), t("v2")
    n1, d = x1.shape
    n2 = x2.shape[0]
    p = v1.shape[0] // n1
    ctx, hyp, p1, p2 = _packs(dsvgp, gpu_device, x1, x2, v1, v2, float(g["lengthscale"]), 1.0)
    Kw = dsvgp._ops.kernel_fwd_wide(ctx, p1, n1, p2, n2, d, p, hyp)
    K = dsvgp._ops.kernel_fwd(ctx, p1, n1, p2, n2, d, p, hyp)
    e_sub, e_sum = kernel_error(Kw, g)
    e_narrow = relmax(Kw, K)
    _report("kernel_fwd_wide %s" % os.path.basename(path), {"golden": e_sub, "vs kernel_fwd": e_narrow})
    assert e_sub < 2e-6 and (e_sum is None or e_sum < 2e-6)
    assert e_narrow < 2e-6


# ------------------------------------------------------------------ 3. exact diagonal of K_ZZ
@pytest.mark.parametrize("d", [93, 1000])
def test_kernel_fwd_wide_symmetric_double_with_jitter_and_exact_diagonal(dsvgp, gpu_device, d):
    g = torch.Generator().manual_seed(d)
    M, p = 50, 5
    Z, V = torch.rand(M, d, generator=g), torch.randn(M * p, d, generator=g)
    ell, s = _ell(d), 0.6931
    ctx, hyp, pz, _ = _packs(dsvgp, gpu_device, Z, Z, V, V, ell, s)
    K = dsvgp._ops.kernel_fwd(ctx, pz, M, pz, M, d, p, hyp, jitter=1e-3, dtype=torch.float64)
    ref = s * O.kernel_matrix(Z.double(), Z.double(), V.double(), V.double(), ell) + 1e-3 * torch.eye(M * (p + 1), dtype=torch.float64)
    assert relmax(K, ref) < 2e-5
    Kc = K.cpu()
    assert (Kc - Kc.t()).abs().max().item() < 2e-6
    q = p + 1
    for i in (0, 7, M - 1):
        blk = Kc[i * q:(i + 1) * q, i * q:(i + 1) * q]
        assert blk[0, 0].item() == pytest.approx(np.float32(s) + np.float32(1e-3), rel=1e-6)
        assert blk[0, 1:].abs().max().item() == 0.0 and blk[1:, 0].abs().max().item() == 0.0
    assert torch.equal(Kc, Kc.float().double())


# ------------------------------------------------------------------ 4. backward against fp64 autograd
def _bwd_case(dsvgp, dev, n1, n2, d, p, sym, wide_entry=False, seed=0):
    ops = dsvgp._ops
    g, x1, x2, v1, v2 = _points(n1, n2, d, p, seed=seed)
    if sym:
        x2, v2, n2 = x1, v1, n1
    ell, s = _ell(d), 1.3
    q = p + 1
    G = torch.randn(n1 * q, n2 * q, generator=g, dtype=torch.float64)
    if sym:
        G = G + G.t()
    x1r = x1.double().requires_grad_(True)
    v1r = v1.double().requires_grad_(True)
    ellr = torch.tensor(ell, dtype=torch.float64, requires_grad=True)
    sr = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    if sym:
        K = sr * O.kernel_matrix(x1r, x1r, v1r, v1r, ellr)
    else:
        K = sr * O.kernel_matrix(x1r, x2.double(), v1r, v2.double(), ellr)
    (K * G).sum().backward()
    ctx, hyp, p1, p2 = _packs(dsvgp, dev, x1, x2, v1, v2, ell, s)
    out = []
    for Gd in (G.to(dev), G.float().to(dev)):
        dx = torch.zeros(n1, d, device=dev)
        dv = torch.zeros(max(n1 * p, 1), d, device=dev)
        dh = torch.zeros(4, device=dev)
        (ops.kernel_bwd_wide if wide_entry else ops.kernel_bwd)(ctx, Gd.contiguous(), p1, n1, p2, n2, d, p, hyp, sym, dx, dv, dh)
        out.append((dx, dv[:n1 * p], dh))
    return out, (x1r.grad, v1r.grad, ellr.grad.item(), sr.grad.item())


@pytest.mark.parametrize("n1,n2,d,p,sym", [(11, 23, 93, 2, False), (18, 18, 93, 5, True), (20, 45, 200, 5, False), (16, 16, 200, 3, True),
                                           (9, 30, 200, 0, False), (7, 19, 1000, 10, False), (12, 12, 1000, 1, True),
                                           (5, 13, 4035, 10, False), (6, 6, 4035, 10, True)])
def test_kernel_bwd_at_wide_inputs_matches_autograd(dsvgp, gpu_device, n1, n2, d, p, sym):
    res, (gx, gv, gl, gs) = _bwd_case(dsvgp, gpu_device, n1, n2, d, p, sym, seed=n1 + 31 * n2 + d)
    for (dx, dv, dh), up in zip(res, ("double", "float")):
        errs = {"d_x1": relmax(dx, gx), "d_l": abs(dh[0].item() - gl) / max(1.0, abs(gl)), "d_s": abs(dh[1].item() - gs) / max(1.0, abs(gs))}
        if p > 0:
            errs["d_v1"] = relmax(dv, gv)
        _report("kernel_bwd d=%d p=%d %dx%d sym=%d %s upstream" % (d, p, n1, n2, sym, up), errs)
        for k, e in errs.items():
            assert e < 2e-4, (up, k, e)


@pytest.mark.parametrize("n1,n2,d,p,sym", [(11, 23, 5, 2, False), (20, 45, 20, 5, False), (18, 18, 20, 5, True), (50, 95, 10, 10, False),
                                           (9, 9, 3, 3, True), (6, 10, 6, 0, False), (30, 60, 50, 5, False)])
def test_kernel_bwd_wide_at_small_d_equals_kernel_bwd_and_autograd(dsvgp, gpu_device, n1, n2, d, p, sym):
    seed = n1 + 31 * n2 + d
    wide, (gx, gv, gl, gs) = _bwd_case(dsvgp, gpu_device, n1, n2, d, p, sym, wide_entry=True, seed=seed)
    narrow, _ = _bwd_case(dsvgp, gpu_device, n1, n2, d, p, sym, wide_entry=False, seed=seed)
    for (dx, dv, dh), (nx, nv, nh) in zip(wide, narrow):
        assert relmax(dx, gx) < 2e-4 and relmax(dx, nx) < 2e-4
        if p > 0:
            assert relmax(dv, gv) < 2e-4 and relmax(dv, nv) < 2e-4
        assert abs(dh[0].item() - gl) < 2e-4 * max(1.0, abs(gl)) and abs(dh[1].item() - gs) < 2e-4 * max(1.0, abs(gs))
        assert relmax(dh[:2], nh[:2]) < 2e-4


# ------------------------------------------------------------------ 5. the one-call step, and against the piecewise step
def _wide_problem(N, d, M, p, B, seed):
    P, x, y, D, nd = make_problem(N, d, M, p, B, seed=seed)
    P["raw_lengthscale"] = torch.tensor([[_raw(_ell(d))]])
    return P, x, y, D, nd


STEP_CASES = [(2000, 200, 60, 3, 128), (400, 4035, 10, 10, 256)]


@pytest.mark.parametrize("N,d,M,p,B", STEP_CASES)
@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
def test_one_call_step_at_wide_inputs(dsvgp, gpu_device, N, d, M, p, B, mll):
    P, x, y, D, nd = _wide_problem(N, d, M, p, B, seed=N + d)
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    xd, yd, Dd = x.to(gpu_device), y.to(gpu_device), D.to(gpu_device)
    eng = dsvgp.ElboEngine(gpu_device)
    l1, g1, mu1, _ = eng.loss_and_grads(Pg, xd, yd, Dd, nd, mll)
    torch.cuda.synchronize()
    one_call = eng.c_step_used
    ref = dsvgp.ElboEngine(gpu_device)
    ref.c_step = False
    l0, g0, mu0, _ = ref.loss_and_grads(Pg, xd, yd, Dd, nd, mll)
    torch.cuda.synchronize()
    assert not ref.c_step_used
    l_ref, g_ref, mu_ref, _ = O.elbo_loss_and_grads(P, x, y, D, nd, mll)
    errs = {"loss": abs(l1.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu1, mu_ref),
            "loss vs piecewise": abs(l1.item() - l0.item()) / abs(l0.item()), "mu vs piecewise": relmax(mu1, mu0)}
    for k in O.PARAM_NAMES:
        if g_ref[k].numel():
            errs[k] = relmax(g1[k], g_ref[k])
            errs[k + " vs piecewise"] = relmax(g1[k], g0[k])
    _report("step N=%d d=%d M=%d p=%d B=%d %s (one-call: %s)" % (N, d, M, p, B, mll, one_call), errs)
    assert errs["loss"] < 2e-5 and errs["mu"] < 2e-4
    assert errs["loss vs piecewise"] < 4e-6 and errs["mu vs piecewise"] < 4e-6
    for k in O.PARAM_NAMES:
        if g_ref[k].numel():
            assert errs[k] < 2e-3, (k, errs[k])
            assert errs[k + " vs piecewise"] < 5e-5, (k, errs[k + " vs piecewise"])
    assert g1["chol_variational_covar"].triu(1).abs().max().item() == 0.0


# ------------------------------------------------------------------ 7. prediction
def test_predict_and_joint_predictive_at_d200(dsvgp, gpu_device):
    P, x, y, D, nd = _wide_problem(2000, 200, 60, 3, 80, seed=5)
    mu_ref, var_ref = O.predictive(P, x, D)
    _, _, noise = O.constrained(P)
    eng = dsvgp.ElboEngine(gpu_device)
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    xd, Dd = x.to(gpu_device), D.to(gpu_device)
    mu, varn = eng.predict(Pg, xd, Dd)
    e_mu, e_var = relmax(mu, mu_ref), relmax(varn, var_ref + noise)
    mu_j_ref, Sig_ref = O.predictive_joint({k: v.double() for k, v in P.items()}, x.double(), D.double())
    mu_j, Sigma = eng.predict_joint(Pg, xd, Dd)
    n = Sigma.shape[0]
    Sig_ref = Sig_ref + noise.double() * torch.eye(n, dtype=torch.float64)
    e_jmu, e_sig = relmax(mu_j, mu_j_ref), relmax(Sigma, Sig_ref)
    root = eng.covariance_root(Sigma)
    eps = torch.randn(5, n, device=gpu_device)
    draws = eng.draw(mu_j, root, eps)
    R = torch.tril(root)
    e_draw = relmax(draws, mu_j.double().cpu() + eps.double().cpu() @ R.cpu().t())
    _report("predict d=200", {"mu": e_mu, "var": e_var, "joint mu": e_jmu, "joint Sigma": e_sig, "draw": e_draw})
    assert e_mu < 2e-4 and e_var < 2e-4
    assert e_jmu < 5e-4 and e_sig < 5e-4
    assert draws.shape == (5, n) and torch.isfinite(draws).all() and e_draw < 1e-5


# ------------------------------------------------------------------ 8. deterministic mode
def test_deterministic_mode_at_d200_is_bitwise_reproducible(dsvgp, gpu_device):
    P, x, y, D, nd = _wide_problem(2000, 200, 60, 3, 128, seed=8)
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    xd, yd, Dd = x.to(gpu_device), y.to(gpu_device), D.to(gpu_device)
    runs = []
    for _ in range(2):
        eng = dsvgp.ElboEngine(gpu_device)
        eng.deterministic = True
        loss, grads, mu, _ = eng.loss_and_grads(Pg, xd, yd, Dd, nd)
        torch.cuda.synchronize()
        runs.append((loss.clone(), {k: v.clone() for k, v in grads.items()}, mu.clone()))
    (l0, g0, m0), (l1, g1, m1) = runs
    assert torch.equal(l0, l1) and torch.equal(m0, m1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


# ------------------------------------------------------------------ 6. natural-gradient and CIQ steps
def _wide_ngd_problem(N, d, M, p, B, seed):
    from test_ngd import make_ngd_problem
    P, x, y, D, nd = make_ngd_problem(N, d, M, p, B, seed=seed)
    P["raw_lengthscale"] = torch.tensor([[_raw(_ell(d))]])
    return P, x, y, D, nd


def test_natural_step_at_d200_matches_oracle(dsvgp, gpu_device):
    P, x, y, D, nd = _wide_ngd_problem(2000, 200, 60, 3, 128, seed=6)
    l_ref, g_ref, mu_ref, var_ref = O.ngd_loss_and_grads(P, x, y, D, nd)
    eng = dsvgp.ElboEngine(gpu_device)
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    loss, grads, mu, varn = eng.loss_and_grads(Pg, x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd)
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref)}
    for k in O.NGD_PARAM_NAMES:
        if g_ref[k].numel() and g_ref[k].abs().max() > 0:
            errs[k] = relmax(grads[k], g_ref[k])
    _report("natural step d=200 M=60 p=3 B=128", errs)
    assert errs.pop("loss") < 2e-5 and errs.pop("mu") < 2e-4
    for k, e in errs.items():
        assert e < 5e-3, (k, e)


def test_ciq_step_at_d200_matches_oracle(dsvgp, gpu_device):
    P, x, y, D, nd = _wide_ngd_problem(500, 200, 24, 3, 48, seed=7)
    st = {}
    l_ref, g_ref, mu_ref, var_ref = O.ciq_loss_and_grads(P, x, y, D, nd, stats=st)
    eng = dsvgp.ElboEngine(gpu_device, trsm_nb=4096)
    eng.whitening = "ciq"
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    loss, grads, mu, varn = eng.loss_and_grads(Pg, x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd)
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref), "var": relmax(varn, var_ref)}
    for k in O.NGD_PARAM_NAMES:
        if g_ref[k].numel() and g_ref[k].abs().max() > 0:
            errs[k] = relmax(grads[k], g_ref[k])
    _report("CIQ step d=200 M=24 p=3 B=48", errs)
    assert errs.pop("loss") < 1e-3 and errs.pop("mu") < 5e-3 and errs.pop("var") < 5e-3
    for k, e in errs.items():
        assert e < 2e-2, (k, e)


# ------------------------------------------------------------------ 9. the training harnesses at the rover width
# The harnesses start from gpytorch's lengthscale softplus(0) = 0.693; the inputs are scaled so that this is 0.4 sqrt(d) of U[0, 1]^d.
def _rover_data(N, d, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(N, d, generator=g) * (math.log(2.0) / _ell(d))
    return X, O.testfun(X)


def _first_and_last_loss(out):
    first = [float(l.split("loss: ")[1].split(",")[0]) for l in out.splitlines() if l.startswith("Epoch")][0]
    last = [float(l.split("loss: ")[1]) for l in out.splitlines() if l.startswith("Done! loss: ")][-1]
    return first, last


@pytest.mark.parametrize("harness", ["directional_vi", "dfree_directional_vi", "shared_directional_vi", "traditional_vi"])
def test_training_harnesses_at_d200(dsvgp, gpu_device, harness, capsys):
    from torch.utils.data import TensorDataset
    N, d, B = 2000, 200, 512
    X, Y = _rover_data(N + 300, d, seed=9)
    Xtr, Ytr, Xte, Yte = X[:N], Y[:N], X[N:], Y[N:]
    mod = getattr(dsvgp, harness)
    if harness == "traditional_vi":
        model, lik = mod.train_gp(TensorDataset(Xtr, Ytr[:, 0].contiguous()), d, num_inducing=400, minibatch_size=B, num_epochs=2,
                                  tqdm=False, seed=4)
        means, variances = mod.eval_gp(TensorDataset(Xte, Yte[:, 0].contiguous()), model, lik, minibatch_size=100)
        n_out = 300
    else:
        M, p = 100, 3
        ys = Ytr[:, 0].contiguous() if harness == "dfree_directional_vi" else Ytr
        yt = Yte[:, 0].contiguous() if harness == "dfree_directional_vi" else Yte
        model, lik = mod.train_gp(TensorDataset(Xtr, ys), num_inducing=M, num_directions=p, minibatch_size=B, minibatch_dim=p,
                                  num_epochs=2, inducing_data_initialization=harness != "shared_directional_vi", tqdm=False, seed=4)
        means, variances = mod.eval_gp(TensorDataset(Xte, yt), model, lik, num_directions=p, minibatch_size=100, minibatch_dim=p)
        n_out = 300 if harness == "dfree_directional_vi" else 300 * (p + 1)
    first, last = _first_and_last_loss(capsys.readouterr().out)
    _report("%s d=200 N=2000 B=512, 2 epochs" % harness, {"first loss": first, "last loss": last})
    assert math.isfinite(first) and math.isfinite(last) and last < first
    assert means.shape == (n_out,) and variances.shape == (n_out,)
    assert torch.isfinite(means).all() and (variances > 0).all()


def test_directional_vi_at_d200_tracks_the_oracle_trainer(dsvgp, gpu_device):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from train_quality import against_oracle
    N, d = 2000, 200
    X, Y = _rover_data(N, d, seed=10)
    res = against_oracle(dsvgp.directional_vi, X.to(gpu_device).contiguous(), Y.to(gpu_device).contiguous(),
                         dict(d=d, M=100, p=3, B=512), 25, 0.01)
    _report("directional_vi d=200 M=100 p=3 B=512: 25 steps vs the oracle trainer",
            {"max rel diff": res["max_rel_diff"], "at last step": res["rel_diff_at_last_step"]})
    assert res["max_rel_diff"] < 2e-4


# ------------------------------------------------------------------ 10. the GCN geometry and its Thompson draw
def test_gcn_geometry_trains_and_draws_thompson_samples(dsvgp, gpu_device, capsys):
    """gcn_turbo.py: d = model.n_params = 4035, M = 10, p = 10, B = 256; the draw of :233-239 on 1000 candidates."""
    from torch.utils.data import DataLoader, TensorDataset
    N, d, M, p, B = 400, 4035, 10, 10, 256
    X, Y = _rover_data(N, d, seed=11)
    model, lik = dsvgp.directional_vi.train_gp(TensorDataset(X, Y), num_inducing=M, num_directions=p, minibatch_size=B,
                                               minibatch_dim=p, num_epochs=3, tqdm=False, seed=0)
    first, last = _first_and_last_loss(capsys.readouterr().out)
    assert math.isfinite(first) and math.isfinite(last)
    model.eval()
    lik.eval()
    g = torch.Generator().manual_seed(12)
    X_cand = torch.rand(1000, d, generator=g) * (math.log(2.0) / _ell(d))
    n_samples = 3
    samples = torch.empty(n_samples, 0)
    with torch.no_grad():
        for (x_batch,) in DataLoader(TensorDataset(X_cand), batch_size=250, shuffle=False):
            x_batch = x_batch.to(gpu_device)
            D = torch.eye(d)[:model.num_directions].repeat(x_batch.shape[0], 1).to(gpu_device)
            preds = lik(model(x_batch, derivative_directions=D))
            cur = preds.sample(torch.Size([n_samples]))[:, ::model.num_directions + 1]
            samples = torch.hstack([samples, cur.detach().cpu()])
    _report("GCN geometry d=4035 M=10 p=10 B=256, 3 epochs", {"first loss": first, "last loss": last,
                                                                "draw std": samples.std().item()})
    assert samples.shape == (n_samples, 1000) and torch.isfinite(samples).all()
