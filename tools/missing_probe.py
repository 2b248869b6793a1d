#!/usr/bin/env python3
"""Cost of ``missing_targets`` at BASELINE config 4's step shape (d = 20, M = 500, p = 5, B = 4096: M' = 3000, B' = 24576).  GPU box tool;
nothing here is imported by the package.  Writes profiles/missing_probe.txt (or --out):

  1. the masked per-output step (ELBO and PLL) with 0 % and 30 % of the targets NaN against the unmasked ``fast=False`` step on the same
     batch -- both the path that call takes by default and the piecewise path the masked step runs on (``c_step = False``);
  2. one collapsed statistics chunk (``CollapsedAccumulator.add``) and one backward chunk (``add_backward``), masked at 0 % and 30 %
     against unmasked.
Timings: two warm-up calls, then the callables alternate inside every repetition, each between device events; medians of 30.

  python3 tools/missing_probe.py [--reps 30] [--out profiles/missing_probe.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("", "tools", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import torch  # noqa: E402


def timed_many(fns, reps, warm=2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "missing_probe.txt"))
    args = ap.parse_args()
    import bench
    import dsvgp_amd
    import dsvgp_oracle as O
    cfg = bench.CONFIGS["c4"]
    d, M, p, B = cfg["d"], cfg["M"], cfg["p"], cfg["B"]
    dev = torch.device("cuda", 0)
    lines = ["missing_targets: cost at config 4's step shape (d = %d, M = %d, p = %d, B = %d: M' = %d, B' = %d); medians of %d, alternating; %s"
             % (d, M, p, B, M * (p + 1), B * (p + 1), args.reps, torch.cuda.get_device_name(0))]
    say = lambda s: (lines.append(s), print(s, flush=True))

    g = torch.Generator().manual_seed(0)
    X = torch.rand(M + B, d, generator=g)
    F = O.testfun(X[M:])
    V = torch.eye(d)[:p].repeat(M, 1)
    P = O.init_params(X[:M].clone(), V, torch.float32, 0.1, g)
    x = X[M:].contiguous().to(dev)
    y = F[:, :p + 1].reshape(-1).contiguous()
    D = torch.eye(d)[:p].repeat(B, 1).to(dev)
    y30 = y.clone()
    y30[torch.rand(y.shape[0], generator=g) < 0.3] = float("nan")
    y, y30 = y.to(dev), y30.to(dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    nd = (d + 1) * 1_000_000

    def engine(missing, c_step=True):
        eng = dsvgp_amd.ElboEngine(dev)
        eng.missing_targets, eng.c_step = missing, c_step
        return eng
    off, piece, on = engine(False), engine(False, c_step=False), engine(True)
    for mll in ("ELBO", "PLL"):
        t = timed_many({"off": lambda: off.loss_and_grads(Pg, x, y, D, nd, mll, fast=False),
                        "piecewise": lambda: piece.loss_and_grads(Pg, x, y, D, nd, mll, fast=False),
                        "masked0": lambda: on.loss_and_grads(Pg, x, y, D, nd, mll),
                        "masked30": lambda: on.loss_and_grads(Pg, x, y30, D, nd, mll)}, args.reps)
        say("1. %s step, ms (median, min, max): fast=False default path%s %.3f (%.3f, %.3f); piecewise per-output path %.3f (%.3f, %.3f); masked 0 %% "
            "%.3f (%.3f, %.3f); masked 30 %% %.3f (%.3f, %.3f)" % ((mll, " (one-call step)" if off.c_step_used else "") + t["off"] + t["piecewise"]
                                                                    + t["masked0"] + t["masked30"]))
        say("   ratios: masked 0 %% / piecewise %.4f, masked 30 %% / piecewise %.4f; masked 0 %% / default %.4f, masked 30 %% / default %.4f"
            % (t["masked0"][0] / t["piecewise"][0], t["masked30"][0] / t["piecewise"][0], t["masked0"][0] / t["off"][0],
               t["masked30"][0] / t["off"][0]))
    fast = timed_many({"fast": lambda: off.loss_and_grads(Pg, x, y, D, nd, "ELBO")}, args.reps)["fast"]
    say("   for scale: the Gram fast path's ELBO step (not available with missing_targets) %.3f ms" % fast[0])
    del off, piece

    budget = 4 << 30                                            # the chunk of 4096 points stays one chunk in both passes
    accs = {k: engine(k != "off").collapsed_accumulator(Pg, workspace_budget=budget) for k in ("off", "masked0", "masked30")}
    ys = {"off": y, "masked0": y, "masked30": y30}
    t = timed_many({k: (lambda k=k: accs[k].add(x, ys[k], D)) for k in accs}, args.reps)
    say("2. one statistics chunk (add), ms: unmasked %.3f (%.3f, %.3f); masked 0 %% %.3f (%.3f, %.3f); masked 30 %% %.3f (%.3f, %.3f); ratios "
        "%.4f and %.4f" % (t["off"] + t["masked0"] + t["masked30"] + (t["masked0"][0] / t["off"][0], t["masked30"][0] / t["off"][0])))
    for k, acc in accs.items():
        acc.reset()
        acc.add(x, ys[k], D)
        acc.begin_backward(acc.solve(nd))
    t = timed_many({k: (lambda k=k: accs[k].add_backward(x, ys[k], D)) for k in accs}, args.reps)
    say("2. one backward chunk (add_backward), ms: unmasked %.3f (%.3f, %.3f); masked 0 %% %.3f (%.3f, %.3f); masked 30 %% %.3f (%.3f, %.3f); "
        "ratios %.4f and %.4f" % (t["off"] + t["masked0"] + t["masked30"] + (t["masked0"][0] / t["off"][0], t["masked30"][0] / t["off"][0])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
