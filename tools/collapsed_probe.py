#!/usr/bin/env python3
"""Probe of the closed-form optimal q(u) at BASELINE config 4 (N = 1M, d = 20, M = 500, p = 5, chunks of 4096).  GPU box tool; nothing here
is imported by the package.  Writes profiles/collapsed_probe.txt (or --out):

  1. time of one statistics pass (``fit_variational``) beside the time of one training epoch (245 steps), measured in the same run;
  2. time of one chunk of the pass against the sum of its three existing constituents timed alone through ``_ops`` at the same shape:
     rectangular assembly, fp64 forward solve, fp64 lower product onto the statistics.  The chunk may cost at most 1.15 x that sum;
  3. test MSE and full-data loss of: one ``fit_variational`` on a fresh model; one epoch; one epoch followed by a refit
     (data and evaluation of tools/train_quality.py);
  4. the function-space errors of case b of tests/test_gpu_collapsed.py beside their floors.

  python3 tools/collapsed_probe.py [--n-train 1000000] [--n-test 100000] [--out profiles/collapsed_probe.txt]
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("", "tools", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import torch  # noqa: E402


def timed(fn, reps=10, warm=2):
    """median milliseconds of ``fn`` between HIP events, ``warm`` untimed calls first"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def test_mse(dvi, model, lik, Xte, Yte, p, batch=4096):
    means, _ = dvi.eval_gp(torch.utils.data.TensorDataset(Xte, Yte), model, lik, num_directions=p, minibatch_size=batch, minibatch_dim=p)
    return float(((means[::p + 1] - Yte[:, 0].cpu()) ** 2).mean())


def full_loss(model, lik, X, Y, p, budget):
    """full-data loss of the model's current q(u) (and of the optimum for its hyper-parameters) from one pass with the first p
    canonical directions"""
    acc = model.engine.collapsed_accumulator(model._param_dict(lik), workspace_budget=budget)
    d = X.shape[1]
    E = torch.eye(d, device=X.device)[:p]
    for s in range(0, X.shape[0], 4096):
        xb = X[s:s + 4096]
        acc.add(xb, Y[s:s + 4096, :p + 1].reshape(-1).contiguous(), E.repeat(xb.shape[0], 1))
    nd = (d + 1) * X.shape[0]
    vd = model.variational_strategy._variational_distribution
    return acc.evaluate(vd.variational_mean.data, vd.chol_variational_covar.data, nd).loss, acc.solve(nd).loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=1_000_000)
    ap.add_argument("--n-test", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collapsed_probe.txt"))
    args = ap.parse_args()
    import bench
    import dsvgp_amd
    import train_quality as tq
    from dsvgp_amd import _ops, directional_vi as dvi
    from dsvgp_amd._lib import OUT_LOWER, TRANS_B
    cfg = dict(bench.CONFIGS["c4"])
    d, M, p, B, N = cfg["d"], cfg["M"], cfg["p"], cfg["B"], args.n_train
    dev = torch.device("cuda", 0)
    budget = 4 << 30                                             # a chunk of 4096 points stays one chunk (the default 1 GiB cuts it at 2599)
    lines = ["closed-form optimal q(u): probe at config 4 (N = %d, d = %d, M = %d, p = %d, chunks of %d); %s"
             % (N, d, M, p, B, torch.cuda.get_device_name(0))]
    say = lambda s: (lines.append(s), print(s, flush=True))

    Xall, Yall = tq.make_data("welch", N + args.n_test, d, dev, seed=0)
    mu, sig = Yall[:N, 0].mean(), Yall[:N, 0].std(unbiased=True)
    Yall = torch.cat([((Yall[:, :1] - mu) / sig), Yall[:, 1:] / sig], 1).float().contiguous()
    Xtr, Ytr, Xte, Yte = Xall[:N].contiguous(), Yall[:N].contiguous(), Xall[N:].contiguous(), Yall[N:].contiguous()
    setup = lambda: dsvgp_amd.setup_training(None, num_inducing=M, num_directions=p, minibatch_size=B, minibatch_dim=p, num_epochs=1,
                                             learning_rate_hypers=0.01, inducing_data_initialization=True, seed=0, tensors=(Xtr, Ytr))

    # ---- 3a / 1: one fit_variational on a fresh model, timed (the second of two passes: the first one allocates)
    loop = setup()
    model, lik = loop.model, loop.likelihood
    dvi.fit_variational(model, lik, (Xtr[:2 * B], Ytr[:2 * B]), minibatch_size=B, seed=0, workspace_budget=budget)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = dvi.fit_variational(model, lik, (Xtr, Ytr), minibatch_size=B, seed=0, workspace_budget=budget)
    torch.cuda.synchronize()
    t_pass = time.perf_counter() - t0
    mse_fit = test_mse(dvi, model, lik, Xte, Yte, p)
    say("3. fresh model, one fit_variational:   test MSE %.5f, full-data loss %.5f (constant predictor: MSE %.5f)"
        % (mse_fit, res.loss, float((Yte[:, 0] ** 2).mean())))

    # ---- 1 / 3b: one epoch of the training loop from the default start, timed in the same run; then a refit
    loop = setup()
    model, lik = loop.model, loop.likelihood
    torch.cuda.synchronize()                                     # (no warm-up steps: they would move the state; the first step's allocations are timed)
    t0 = time.perf_counter()
    perm = loop.epoch_permutation()
    steps = 0
    for s0 in range(0, N, B):
        loop.step(perm[s0:s0 + B])
        steps += 1
    loop.finish()
    torch.cuda.synchronize()
    t_epoch = time.perf_counter() - t0
    mse_epoch = test_mse(dvi, model, lik, Xte, Yte, p)
    loss_epoch, loss_opt = full_loss(model, lik, Xtr, Ytr, p, budget)
    say("3. one epoch (%d steps):                test MSE %.5f, full-data loss %.5f (optimum for its hyper-parameters: %.5f)"
        % (steps, mse_epoch, loss_epoch, loss_opt))
    res2 = loop.refit_variational(minibatch_size=B, seed=0)
    mse_refit = test_mse(dvi, model, lik, Xte, Yte, p)
    say("3. one epoch, then refit_variational:  test MSE %.5f, full-data loss %.5f" % (mse_refit, res2.loss))
    say("1. one statistics pass (%d chunks of %d, solve included): %.3f s; one training epoch (%d steps, first-step allocations "
        "included): %.3f s -- same run, same box" % ((N + B - 1) // B, B, t_pass, steps, t_epoch))

    # ---- 2: one chunk against its constituents at the same shape
    eng = model.engine
    Pg = model._param_dict(lik)
    acc = eng.collapsed_accumulator(Pg, workspace_budget=budget)
    assert acc.chunk_rows(p) >= B
    xb = Xtr[:B].contiguous()
    yb = Ytr[:B, :p + 1].reshape(-1).contiguous()
    Db = torch.eye(d, device=dev)[:p].repeat(B, 1).contiguous()
    ctx = _ops.Context.get(dev)
    Mp, Bp = acc.Mp, B * (p + 1)
    chunk = timed(lambda: acc.add(xb, yb, Db))
    packX = _ops.pack_points(ctx, xb, Db, p, acc._hyp, acc._center)
    Kzx = torch.empty(Mp, Bp, device=dev)
    A64 = torch.empty(Mp + 1, Bp, dtype=torch.float64, device=dev)
    ws = acc._buf["trsm_ws"]
    T = torch.zeros(Mp + 1, Mp + 1, dtype=torch.float64, device=dev)
    asm = timed(lambda: _ops.kernel_fwd_rect(ctx, acc._packZ, M, p, packX, B, p, d, acc._hyp, out=Kzx))
    slv = timed(lambda: _ops.trsm(ctx, acc._L, Kzx, False, A64[:Mp], None, acc._nb, ws, reuse_inverse=True))
    A64[Mp].zero_()
    prod = timed(lambda: _ops.gemm(ctx, TRANS_B | OUT_LOWER, A64, A64, T, beta=1.0, Cin=T))
    total = asm[0] + slv[0] + prod[0]
    say("2. one chunk (M' = %d, B' = %d): %.3f ms (min %.3f, max %.3f); alone: assembly %.3f + forward solve %.3f + fp64 lower product "
        "%.3f = %.3f ms; ratio %.3f (bound 1.15: %s)" % (Mp, Bp, chunk[0], chunk[1], chunk[2], asm[0], slv[0], prod[0], total,
                                                        chunk[0] / total, "held" if chunk[0] <= 1.15 * total else "NOT held"))

    # ---- 4: case b of the GPU tests
    import test_gpu_collapsed as tg
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        tg.test_optimum_in_function_space(dsvgp_amd, dev, "b")
    tg._cache.clear()
    say("4. " + buf.getvalue().strip())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
