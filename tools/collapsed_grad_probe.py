#!/usr/bin/env python3
"""Probe of the collapsed bound's gradients at BASELINE config 4 (N = 1M, d = 20, M = 500, p = 5, chunks of 4096).  GPU box tool; nothing
here is imported by the package.  Writes profiles/collapsed_grad_probe.txt (or --out):

  1. time of one backward pass (begin_backward, 245 x add_backward, finish_backward) beside one statistics pass (``fit_variational``) and
     one training epoch (245 steps), all measured in the same run;
  2. time of one backward chunk against the sum of its parts timed alone at the same shape -- rectangular assembly, the C call (the
     Q K_ZX product and the three new kernels), the rectangular kernel backward.  The chunk may cost at most 1.15 x that sum;
  3. the two routes to the M'^2 B' product, timed alone: the C call with Q K_ZX (fp64 accumulation over the float operand, one
     product) against forward solve + fp32 dense product + transposed solve;
  4. test MSE after ``train_collapsed`` for --iterations iterations beside "one epoch, then refit_variational" from the same run
     (data and evaluation of tools/train_quality.py).
Timings follow the measuring rules of the project: two warm-up calls, medians of 10 between device events, A / B in alternating order.

  python3 tools/collapsed_grad_probe.py [--n-train 1000000] [--n-test 100000] [--iterations 10] [--out profiles/collapsed_grad_probe.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("", "tools", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import torch  # noqa: E402


def timed_many(fns, reps=10, warm=2):
    """{name: (median, min, max) ms} of every callable between HIP events; the callables alternate inside every repetition"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    out = {k: [] for k in fns}
    for r in range(reps):
        order = list(fns) if r % 2 == 0 else list(fns)[::-1]
        for k in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fns[k]()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def test_mse(dvi, model, lik, Xte, Yte, p, batch=4096):
    means, _ = dvi.eval_gp(torch.utils.data.TensorDataset(Xte, Yte), model, lik, num_directions=p, minibatch_size=batch, minibatch_dim=p)
    return float(((means[::p + 1] - Yte[:, 0].cpu()) ** 2).mean())


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=1_000_000)
    ap.add_argument("--n-test", type=int, default=100_000)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collapsed_grad_probe.txt"))
    args = ap.parse_args()
    import bench
    import dsvgp_amd
    import train_quality as tq
    from dsvgp_amd import _ops, directional_vi as dvi
    cfg = dict(bench.CONFIGS["c4"])
    d, M, p, B, N = cfg["d"], cfg["M"], cfg["p"], cfg["B"], args.n_train
    dev = torch.device("cuda", 0)
    budget = 4 << 30                                             # a chunk of 4096 points stays one chunk in both passes
    lines = ["collapsed-bound gradients: probe at config 4 (N = %d, d = %d, M = %d, p = %d, chunks of %d); %s"
             % (N, d, M, p, B, torch.cuda.get_device_name(0))]
    say = lambda s: (lines.append(s), print(s, flush=True))

    Xall, Yall = tq.make_data("welch", N + args.n_test, d, dev, seed=0)
    mu, sig = Yall[:N, 0].mean(), Yall[:N, 0].std(unbiased=True)
    Yall = torch.cat([((Yall[:, :1] - mu) / sig), Yall[:, 1:] / sig], 1).float().contiguous()
    Xtr, Ytr, Xte, Yte = Xall[:N].contiguous(), Yall[:N].contiguous(), Xall[N:].contiguous(), Yall[N:].contiguous()
    setup = lambda: dsvgp_amd.setup_training(None, num_inducing=M, num_directions=p, minibatch_size=B, minibatch_dim=p, num_epochs=1,
                                             learning_rate_hypers=0.01, inducing_data_initialization=True, seed=0, tensors=(Xtr, Ytr))

    # ---- 1: statistics pass, backward pass, both through collapsed_loss_and_grads' own pieces; then one epoch
    loop = setup()
    model, lik = loop.model, loop.likelihood
    dvi.collapsed_loss_and_grads(model, lik, (Xtr[:2 * B], Ytr[:2 * B]), minibatch_size=B, seed=0, workspace_budget=budget,
                                 write_variational=False)        # (allocations)
    t_stat, _ = wall(lambda: dvi.fit_variational(model, lik, (Xtr, Ytr), minibatch_size=B, seed=0, workspace_budget=budget))
    acc, X, Y, pd = dvi._collapsed_setup(model, lik, (Xtr, Ytr), None, budget, "probe")
    cols = dvi._collapsed_columns(N, d, pd, B, 0)
    for xb, yb, Db in dvi._collapsed_chunks(X, Y, pd, B, cols):
        acc.add(xb, yb, Db)
    res = acc.solve((d + 1) * N)

    def backward():
        acc.begin_backward(res)
        for xb, yb, Db in dvi._collapsed_chunks(X, Y, pd, B, cols):
            acc.add_backward(xb, yb, Db)
        return acc.finish_backward()
    t_bwd, (loss, grads) = wall(backward)
    t_bwd2, _ = wall(backward)
    say("1. one statistics pass (%d chunks of %d, solve included): %.3f s; one backward pass (prepare and the symmetric K_ZZ backward "
        "included): %.3f s, again %.3f s; collapsed loss %.5f" % ((N + B - 1) // B, B, t_stat, t_bwd, t_bwd2, loss))
    del acc
    loop = setup()
    model, lik = loop.model, loop.likelihood

    def epoch():
        perm = loop.epoch_permutation()
        for s0 in range(0, N, B):
            loop.step(perm[s0:s0 + B])
        loop.finish()
    t_epoch, _ = wall(epoch)
    mse_epoch = test_mse(dvi, model, lik, Xte, Yte, p)
    res2 = loop.refit_variational(minibatch_size=B, seed=0)
    mse_refit = test_mse(dvi, model, lik, Xte, Yte, p)
    say("1. one training epoch (245 steps, first-step allocations included): %.3f s -- same run, same box.  backward / statistics %.2f, "
        "backward / epoch %.2f" % (t_epoch, t_bwd2 / t_stat, t_bwd2 / t_epoch))
    say("4. one epoch: test MSE %.5f; one epoch, then refit_variational: test MSE %.5f, full-data loss %.5f" % (mse_epoch, mse_refit, res2.loss))

    # ---- 2 / 3: one backward chunk against its parts, and the two routes to the product
    acc = model.engine.collapsed_accumulator(model._param_dict(lik), workspace_budget=budget)
    xb, yb = Xtr[:B].contiguous(), Ytr[:B, :p + 1].reshape(-1).contiguous()
    Db = torch.eye(d, device=dev)[:p].repeat(B, 1).contiguous()
    acc.add(xb, yb, Db)
    r1 = acc.solve((d + 1) * N)
    acc.begin_backward(r1)
    st = acc._bwd
    ctx = _ops.Context.get(dev)
    Mp, Bp = acc.Mp, B * (p + 1)
    packX = _ops.pack_points(ctx, xb, Db, p, acc._hyp, acc._center)
    Kzx, Kbar = torch.empty(Mp, Bp, device=dev), torch.empty(Mp, Bp, device=dev)
    V32, A64 = torch.empty(Mp, Bp, device=dev), torch.empty(Mp, Bp, dtype=torch.float64, device=dev)
    S32 = torch.randn(Mp, Mp, device=dev)
    cws = torch.empty(_ops.collapsed_grad_chunk_bytes(Mp, Bp) // 8, dtype=torch.float64, device=dev)
    kws = torch.empty(_ops.kernel_bwd_rect_workspace_bytes(M, p, B, p, d), dtype=torch.uint8, device=dev)
    dZ, dV, dh = torch.zeros(M, d, device=dev), torch.zeros(M * p, d, device=dev), torch.zeros(4, device=dev)
    ws = acc._buf["trsm_ws"]
    _ops.kernel_fwd_rect(ctx, acc._packZ, M, p, packX, B, p, d, acc._hyp, out=Kzx)
    t = timed_many({
        "chunk": lambda: acc.add_backward(xb, yb, Db),
        "assembly": lambda: _ops.kernel_fwd_rect(ctx, acc._packZ, M, p, packX, B, p, d, acc._hyp, out=Kzx),
        "c_call": lambda: _ops.collapsed_grad_chunk(ctx, Mp, Kzx, yb, acc._constant, st["Q"], st["alpha"], st["adj"], Kbar, None, st["rho_sum"], cws),
        "kernel_bwd": lambda: _ops.kernel_bwd_rect(ctx, Kbar, acc._packZ, M, p, packX, B, p, d, acc._hyp, dZ, dV, dh, kws),
        "fwd_solve": lambda: _ops.trsm(ctx, acc._L, Kzx, False, A64, V32, acc._nb, ws, reuse_inverse=True),
        "bwd_solve": lambda: _ops.trsm(ctx, acc._L, V32, True, A64, Kbar, acc._nb, ws, reuse_inverse=True),
        "dense32": lambda: _ops.gemm(ctx, 0, S32, V32, Kbar),
    })
    total = t["assembly"][0] + t["c_call"][0] + t["kernel_bwd"][0]
    say("2. one backward chunk (M' = %d, B' = %d): %.3f ms (min %.3f, max %.3f); alone: assembly %.3f + the C call (Q K_ZX product and the "
        "three new kernels; the product has no entry of its own that writes float32 only) %.3f + kernel backward %.3f = %.3f ms; ratio "
        "%.3f (bound 1.15: %s)" % (Mp, Bp, t["chunk"][0], t["chunk"][1], t["chunk"][2], t["assembly"][0], t["c_call"][0],
                                   t["kernel_bwd"][0], total, t["chunk"][0] / total, "held" if t["chunk"][0] <= 1.15 * total else "NOT held"))
    route2 = t["fwd_solve"][0] + t["dense32"][0] + t["bwd_solve"][0]
    say("3. routes to the M'^2 B' product, alone: the whole C call with Q K_ZX (fp64 accumulation over the float operand, one product) "
        "%.3f ms; forward solve %.3f + fp32 dense product %.3f + transposed solve %.3f = %.3f ms before any epilogue"
        % (t["c_call"][0], t["fwd_solve"][0], t["dense32"][0], t["bwd_solve"][0], route2))
    del acc, Kzx, Kbar, V32, A64, S32

    # ---- 4: train_collapsed from the same start as the epoch above
    t_train, (model_c, lik_c) = wall(lambda: dvi.train_collapsed(None, num_inducing=M, num_directions=p, num_iterations=args.iterations,
                                                                learning_rate_hypers=0.01, minibatch_size=B, seed=0, verbose=False,
                                                                tensors=(Xtr, Ytr), workspace_budget=budget))
    mse_c = test_mse(dvi, model_c, lik_c, Xte, Yte, p)
    say("4. train_collapsed, %d iterations at learning rate 0.01 (%.1f s, final fit_variational included): test MSE %.5f"
        % (args.iterations, t_train, mse_c))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
