"""GPU: the float64 model mode's ELBO step as ONE C call (``dsvgp_elbo_step_f64``, csrc/step64.hip; ``ElboEngine64._c_step64``).

Every case asserts ``eng.c_step_used`` where the call is eligible.  Stated tolerances (everything is double precision on both sides;
what remains is summation order and the cond(K_ZZ) amplification through the Cholesky backward): against the float64 oracle those of
``test_gpu_fp64.py::test_fp64_step_matches_fp64_oracle`` -- loss and predictive mean 1e-9, gradients 1e-7 relative in max-norm per
parameter --, against the reference-text vectors at benchmark size ``test_gpu_reftext.py::TOL64``."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import dsvgp_oracle as O
from _poison import poison_
from test_gpu_fp64 import CASES, make_problem64, relmax

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))

pytestmark = pytest.mark.gpu
f64 = torch.float64

SHAPES = CASES + [
    (300, 20, 12, 20, 40),     # p > 16: the tiled assembly (csrc/assemble64_tiled.hip)
    (300, 200, 20, 3, 48),     # wide inputs: packed width > 96
]


def _engine(gpu_device):
    from dsvgp_amd._step64 import ElboEngine64
    return ElboEngine64(gpu_device)


def _to(P, dev):
    return {k: v.to(dev) for k, v in P.items()}


def _check_against(tag, loss, grads, mu, l_ref, g_ref, mu_ref, p):
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref)}
    assert torch.triu(grads["chol_variational_covar"], 1).abs().max().item() == 0.0
    for k in O.PARAM_NAMES:
        if k == "inducing_directions" and p == 0:
            continue
        errs[k] = relmax(grads[k], g_ref[k])
    print("[parity] fp64 one-call step %s: %s" % (tag, ", ".join("%s %.1e" % kv for kv in errs.items())))
    assert errs["loss"] < 1e-9 and errs["mu"] < 1e-9, (tag, errs)
    assert max(errs[k] for k in O.PARAM_NAMES if k in errs) < 1e-7, (tag, errs)


@pytest.mark.parametrize("N,d,M,p,B", SHAPES)
def test_fp64_one_call_step_matches_fp64_oracle(dsvgp, gpu_device, N, d, M, p, B):
    P, x, y, D, nd = make_problem64(N, d, M, p, B, seed=N + d)
    l_ref, g_ref, mu_ref, _ = O.elbo_loss_and_grads(P, x, y, D, nd, "ELBO")
    eng = _engine(gpu_device)
    loss, grads, mu, varn = eng.loss_and_grads(_to(P, gpu_device), x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd, "ELBO")
    torch.cuda.synchronize()
    assert eng.c_step_used and eng.c_step_status == 0          # (fast=None: the fast_min_work rule does not decide any more)
    assert loss.dtype == f64 and all(v.dtype == f64 for v in grads.values()) and varn.numel() == 0
    assert all(grads[k].shape == P[k].shape for k in O.PARAM_NAMES)
    _check_against(str((N, d, M, p, B)), loss, grads, mu, l_ref, g_ref, mu_ref, p)
    # the switch: off -> the Python-orchestrated path, same numbers
    off = _engine(gpu_device)
    off.c_step = False
    loss0, grads0, mu0, _ = off.loss_and_grads(_to(P, gpu_device), x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd, "ELBO", fast=True)
    torch.cuda.synchronize()
    assert not off.c_step_used
    _check_against(str((N, d, M, p, B)) + " (switch off)", loss0, grads0, mu0, l_ref, g_ref, mu_ref, p)


def test_fp64_one_call_step_path_selection(dsvgp, gpu_device):
    """an explicit fast=False keeps the per-output path and its variances; PLL keeps its path; fast=True takes the call"""
    P, x, y, D, nd = make_problem64(*CASES[1], seed=3)
    Pg, xg, yg, Dg = _to(P, gpu_device), x.to(gpu_device), y.to(gpu_device), D.to(gpu_device)
    eng = _engine(gpu_device)
    _, _, _, varn = eng.loss_and_grads(Pg, xg, yg, Dg, nd, "ELBO", fast=False)
    assert not eng.c_step_used and varn.numel() == y.numel()
    eng.loss_and_grads(Pg, xg, yg, Dg, nd, "PLL")
    assert not eng.c_step_used
    eng.loss_and_grads(Pg, xg, yg, Dg, nd, "ELBO", fast=True)
    assert eng.c_step_used
    eng.data_outputs = "values"                                  # derivative-free data: not through the call
    eng.loss_and_grads(Pg, xg, yg[::3].contiguous(), Dg, nd, "ELBO")
    assert not eng.c_step_used


def test_fp64_one_call_step_without_kl_and_with_global_rows(dsvgp, gpu_device):
    """include_kl=False (a data-parallel rank other than the first) and global_rows != B' (a row shard of a larger minibatch)"""
    N, d, M, p, B = CASES[2]
    P, x, y, D, nd = make_problem64(N, d, M, p, B, seed=11)
    Pg, xg, yg, Dg = _to(P, gpu_device), x.to(gpu_device), y.to(gpu_device), D.to(gpu_device)
    eng = _engine(gpu_device)
    # no KL: the oracle's KL / num_data vanishes for num_data -> infinity (it enters nowhere else)
    l_ref, g_ref, mu_ref, _ = O.elbo_loss_and_grads(P, x, y, D, 1e300, "ELBO")
    loss, grads, mu, _ = eng.loss_and_grads(Pg, xg, yg, Dg, nd, "ELBO", include_kl=False)
    torch.cuda.synchronize()
    assert eng.c_step_used
    _check_against("include_kl=False", loss, grads, mu, l_ref, g_ref, mu_ref, p)
    N, d, M, p, B = CASES[5]
    P, x, y, D, nd = make_problem64(N, d, M, p, B, seed=12)
    rows = 3.0 * y.shape[0] + 5.0
    l_ref, g_ref, mu_ref, _ = O.elbo_loss_and_grads(P, x, y, D, nd, "ELBO", global_rows=rows)
    loss, grads, mu, _ = eng.loss_and_grads(_to(P, gpu_device), x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd, "ELBO",
                                            global_rows=rows)
    torch.cuda.synchronize()
    assert eng.c_step_used
    _check_against("global_rows=%g" % rows, loss, grads, mu, l_ref, g_ref, mu_ref, p)


@pytest.mark.parametrize("name", ["c2", "c3", "c4"])
def test_fp64_one_call_step_against_reference_text_at_baseline_size(dsvgp, gpu_device, name):
    """the call (fast=None: the engine's default) against the reference-text vectors at full C2 / C3 / C4 size"""
    from test_gpu_reftext import TOL64, _check, _errors, _load
    g, P, x, y, D, nd = _load(name)
    eng = _engine(gpu_device)
    if name == "c3":
        eng.chol_jitter = 1e-8                     # GradVariationalStrategy: psd_safe_cholesky's default jitter
    Pg = {k: v.double().to(gpu_device) for k, v in P.items()}
    loss, grads, mu, varn = eng.loss_and_grads(Pg, x.double().to(gpu_device), y.double().to(gpu_device), D.double().to(gpu_device), nd, "ELBO")
    torch.cuda.synchronize()
    assert eng.c_step_used
    assert grads["chol_variational_covar"].triu(1).abs().max().item() == 0.0
    errs = _errors(g, loss, grads, mu, varn, skip=("inducing_directions",) if name == "c3" else ())
    _check("%s fp64 one-call step" % name, errs, *TOL64[name])


def test_fp64_one_call_step_reports_a_failed_factorisation(dsvgp, gpu_device):
    """duplicated inducing points and no add_jitter: K_ZZ is singular, the factorisation leaves a non-zero status word (a numerical
    status, nothing faults), and the engine repeats the step through psd_safe_cholesky's jitter ladder on the Python path: the result
    is that path's"""
    N, d, M, p, B = 300, 3, 30, 1, 40
    P, x, y, D, nd = make_problem64(N, d, M, p, B, seed=5)
    for j in (1, 2, 3):
        P["inducing_points"][j] = P["inducing_points"][0]
        P["inducing_directions"][j * p:(j + 1) * p] = P["inducing_directions"][:p]
    Pg, xg, yg, Dg = _to(P, gpu_device), x.to(gpu_device), y.to(gpu_device), D.to(gpu_device)
    out = []
    for c_step in (True, False):
        eng = _engine(gpu_device)
        eng.c_step = c_step
        eng.kzz_jitter = 0.0
        loss, grads, mu, _ = eng.loss_and_grads(Pg, xg, yg, Dg, nd)
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item() and not eng.c_step_used
        if c_step:
            assert eng.c_step_status is not None and eng.c_step_status != 0
        else:
            assert eng.c_step_status is None
        out.append((loss, {k: v.clone() for k, v in grads.items()}, mu.clone()))
    (l1, g1, mu1), (l0, g0, mu0) = out
    errs = {"loss": abs(l1.item() - l0.item()) / abs(l0.item()), "mu": relmax(mu1, mu0)}
    errs.update({k: relmax(g1[k], g0[k]) for k in O.PARAM_NAMES})
    print("[parity] fp64 one-call step, ladder: %s" % ", ".join("%s %.1e" % kv for kv in errs.items()))
    assert errs["loss"] < 1e-9 and errs["mu"] < 1e-9, errs
    assert max(errs[k] for k in O.PARAM_NAMES) < 1e-7, errs


def test_fp64_one_call_step_plans_and_workspace(dsvgp, gpu_device):
    """two steps on one plan and workspace with different minibatches; flag 8 after the workspace was overwritten with NaN bytes; a
    ragged last batch gets its own plan -- every result against the oracle"""
    N, d, M, p, B = 600, 5, 40, 2, 128
    P, x, y, D, nd = make_problem64(N, d, M, p, 2 * B + 37, seed=21)
    Pg = _to(P, gpu_device)
    eng = _engine(gpu_device)
    q = p + 1

    def batch(lo, hi):
        return x[lo:hi].contiguous(), y[lo * q:hi * q].contiguous(), D[lo * p:hi * p].contiguous()

    for lo, hi in ((0, B), (B, 2 * B)):
        xb, yb, Db = batch(lo, hi)
        l_ref, g_ref, mu_ref, _ = O.elbo_loss_and_grads(P, xb, yb, Db, nd, "ELBO")
        held = (xb.to(gpu_device), yb.to(gpu_device), Db.to(gpu_device))      # (kept alive: the plan's io names them below)
        loss, grads, mu, _ = eng.loss_and_grads(Pg, *held, nd)
        torch.cuda.synchronize()
        assert eng.c_step_used and len(eng._plans) == 1
        _check_against("rows %d:%d" % (lo, hi), loss, grads, mu, l_ref, g_ref, mu_ref, p)
    # flag 8: the workspace contents are undefined -- overwrite it and queue the same step again through the plan (its io still names
    # the tensors of the last step: `held`, `grads`, `mu`, alive here)
    (plan,) = eng._plans.values()
    ws = eng._buf["cstep64_ws_%d_%d_%d_%d" % (M, d, p, B)]
    poison_(ws)                                 # (0xFF bytes: NaN as a double -- accumulating onto it, or reading it as padding, shows)
    grads["chol_variational_covar"].fill_(7.0)
    ctx = dsvgp._ops.Context.get(gpu_device)
    plan.run(ctx, ws, 1 | 2 | 8)
    info, hyp = plan.status()
    torch.cuda.synchronize()
    assert info == 0 and abs(hyp[2] - (torch.nn.functional.softplus(P["raw_noise"]).item() + 1e-4)) < 1e-14
    _check_against("flag 8 after a fill", loss, grads, mu, l_ref, g_ref, mu_ref, p)
    # ragged last batch: its own plan (and workspace); then the full shape again on the first plan
    xb, yb, Db = batch(2 * B, 2 * B + 37)
    l_ref, g_ref, mu_ref, _ = O.elbo_loss_and_grads(P, xb, yb, Db, nd, "ELBO")
    loss, grads, mu, _ = eng.loss_and_grads(Pg, xb.to(gpu_device), yb.to(gpu_device), Db.to(gpu_device), nd)
    torch.cuda.synchronize()
    assert eng.c_step_used and len(eng._plans) == 2
    _check_against("ragged 37 rows", loss, grads, mu, l_ref, g_ref, mu_ref, p)
    xb, yb, Db = batch(0, B)
    l_ref, g_ref, mu_ref, _ = O.elbo_loss_and_grads(P, xb, yb, Db, nd, "ELBO")
    loss, grads, mu, _ = eng.loss_and_grads(Pg, xb.to(gpu_device), yb.to(gpu_device), Db.to(gpu_device), nd)
    torch.cuda.synchronize()
    assert eng.c_step_used and len(eng._plans) == 2
    _check_against("rows 0:%d again" % B, loss, grads, mu, l_ref, g_ref, mu_ref, p)


def test_fp64_one_call_step_event_timings(dsvgp, gpu_device):
    """record_events -> flag 4: the plan's HIP events feed event_durations("solve_fwd") (bench.py --fp64 --full's roofline entry)"""
    P, x, y, D, nd = make_problem64(*CASES[1], seed=2)
    eng = _engine(gpu_device)
    eng.record_events = True
    for _ in range(3):
        eng.loss_and_grads(_to(P, gpu_device), x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd)
    torch.cuda.synchronize()
    assert eng.c_step_used
    for name in ("solve_fwd", "assemble_fwd", "assemble_bwd", "gram", "dense"):
        durs = eng.event_durations(name)
        assert len(durs) == 3 and all(0.0 < t < 1.0 for t in durs), (name, durs)


def test_gather_batch_f64_is_bitwise_the_index_select_form(dsvgp, gpu_device):
    ops = dsvgp._ops
    ctx = ops.Context.get(gpu_device)
    g = torch.Generator().manual_seed(0)
    N, d, p, nb = 500, 7, 3, 77
    X = torch.rand(N, d, generator=g, dtype=f64).to(gpu_device)
    Y = torch.randn(N, d + 1, generator=g, dtype=f64).to(gpu_device)
    E = torch.eye(d, dtype=f64, device=gpu_device)
    idx = torch.randperm(N, generator=g)[:nb].to(gpu_device)
    cols = torch.tensor([0, 2, 5, 7], dtype=torch.int32, device=gpu_device)
    xb = torch.empty(nb, d, dtype=f64, device=gpu_device)
    yb = torch.empty(nb * (p + 1), dtype=f64, device=gpu_device)
    Db = torch.empty(nb * p, d, dtype=f64, device=gpu_device)
    ops.gather_batch_f64(ctx, X, Y, idx, cols, p, xb, yb, E, Db)
    torch.cuda.synchronize()
    assert torch.equal(xb, X.index_select(0, idx))
    assert torch.equal(yb, Y.index_select(0, idx).index_select(1, cols.long()).reshape(-1))
    assert torch.equal(Db, E.index_select(0, cols[1:].long() - 1).repeat(nb, 1))
    # without the direction table (derivative-free data: p = 0 outputs beyond the value)
    y0 = torch.empty(nb, dtype=f64, device=gpu_device)
    ops.gather_batch_f64(ctx, X, Y, idx, cols[:1].contiguous(), 0, xb, y0)
    torch.cuda.synchronize()
    assert torch.equal(y0, Y.index_select(0, idx)[:, 0].contiguous())


def _train_distance(dsvgp, gpu_device, c_step, nsteps=25):
    """largest relative loss difference over ``nsteps`` optimisation steps between the float64 training loop (what train_gp drives)
    and the oracle's trainer in float64, from the same initial state on the same minibatches and derivative columns -- the manner of
    tools/train_quality.py::against_oracle"""
    N, d, M, p, B = 600, 5, 40, 2, 128             # scaled-down C2
    lr = 0.01
    prev = torch.get_default_dtype()
    torch.set_default_dtype(f64)
    try:
        g = torch.Generator().manual_seed(0)
        X = torch.rand(N, d, generator=g, dtype=f64)
        Y = O.testfun(X)
        Xg, Yg = X.to(gpu_device), Y.to(gpu_device)
        loop = dsvgp.setup_training(None, num_inducing=M, num_directions=p, minibatch_size=B, minibatch_dim=p, num_epochs=1,
                                    learning_rate_hypers=lr, inducing_data_initialization=True, seed=1, tensors=(Xg, Yg))
        eng = loop.model.engine
        assert type(eng).__name__ == "ElboEngine64"
        eng.c_step = c_step
        P = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in loop.model._param_dict(loop.likelihood).items()}
        assert all(v.dtype == f64 for v in P.values())
        var = [P["variational_mean"], P["chol_variational_covar"]]
        hyp = [v for k, v in P.items() if k not in ("variational_mean", "chol_variational_covar")]
        opt_v, opt_h = torch.optim.Adam(var, lr=lr), torch.optim.Adam(hyp, lr=lr)
        rng = random.Random(1)            # the loop's own column sampler is random.Random(seed): same sequence here
        perm = loop.epoch_permutation()
        rel = []
        for k in range(nsteps):
            s0 = (k * B) % (N - B + 1)
            idx = perm[s0:s0 + B]
            loss, _, _ = loop.step(idx)
            assert eng.c_step_used == c_step
            cols = sorted(rng.sample(range(1, d + 1), p) + [0])
            xb, yb = X[idx.cpu()], Y[idx.cpu()][:, cols].reshape(-1)
            Dd = torch.eye(d, dtype=f64)[np.array(cols[1:]) - 1].repeat(B, 1)
            opt_v.zero_grad(); opt_h.zero_grad()
            l_ref, _, _ = O.elbo_forward(P, xb, yb, Dd, (d + 1) * N)
            l_ref.backward()
            opt_v.step(); opt_h.step()
            rel.append(abs(float(loss.item()) - float(l_ref.detach())) / max(abs(float(l_ref.detach())), 1e-300))
        loop.finish()
        return max(rel)
    finally:
        torch.set_default_dtype(prev)


def test_fp64_training_through_the_one_call_step_tracks_the_oracle_trainer(dsvgp, gpu_device):
    """25 optimisation steps of the float64 training loop beside the oracle's float64 trainer, once through the one-call step and once
    with it switched off (the Python-orchestrated path).  The bound is measured, not chosen: the one-call distance may be at most 10 x
    the Python path's -- Adam's division by sqrt(v) + eps amplifies last-bit differences of the first steps, and the two paths sum in
    different orders.  Both distances are printed (DESIGN.md section 9 records them)."""
    dist_c = _train_distance(dsvgp, gpu_device, True)
    dist_py = _train_distance(dsvgp, gpu_device, False)
    print("[train] fp64 scaled-down C2, 25 steps, max relative loss distance to the oracle trainer: one-call %.3e, Python path %.3e"
          % (dist_c, dist_py))
    assert dist_c <= 10.0 * dist_py, (dist_c, dist_py)
