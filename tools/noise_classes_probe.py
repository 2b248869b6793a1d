#!/usr/bin/env python3
"""Cost of a separate derivative noise (``raw_derivative_noise``; csrc/noise_classes.hip) at BASELINE config 4's step
shape (d = 20, M = 500, p = 5, B = 4096: M' = 3000, B' = 24576) and at a wide-input shape (d = 200, M = 512, p = 2, B = 2048: M' = 1536,
B' = 6144).  GPU box tool; nothing here is imported by the package.  Writes profiles/noise_classes_probe.txt (or --out):

  1. the two-noise per-output step (ELBO and PLL) against the single-noise ``fast=False`` step on the same batch -- both the path that call
     takes by default and the piecewise path the two-noise step runs on (``c_step = False``);
  2. one weighted collapsed statistics chunk (``CollapsedAccumulator.add``) against an unweighted one.
Timings: five warm-up calls, then the callables alternate inside every repetition, each between device events; medians of 30.

  python3 tools/noise_classes_probe.py [--reps 30] [--out profiles/noise_classes_probe.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("", "tools", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import torch  # noqa: E402

SHAPES = (("config 4", 20, 500, 5, 4096), ("wide inputs", 200, 512, 2, 2048))


def timed_many(fns, reps, warm=5):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_classes_probe.txt"))
    args = ap.parse_args()
    import dsvgp_amd
    import dsvgp_oracle as O
    dev = torch.device("cuda", 0)
    lines = ["raw_derivative_noise: cost of the two noise classes; medians of %d, alternating, 5 warm-ups; %s" % (args.reps, torch.cuda.get_device_name(0))]
    say = lambda s: (lines.append(s), print(s, flush=True))
    for name, d, M, p, B in SHAPES:
        say("%s: d = %d, M = %d, p = %d, B = %d (M' = %d, B' = %d)" % (name, d, M, p, B, M * (p + 1), B * (p + 1)))
        g = torch.Generator().manual_seed(0)
        X = torch.rand(M + B, d, generator=g)
        F = O.testfun(X[M:])
        V = torch.eye(d)[:p].repeat(M, 1)
        P = O.init_params(X[:M].clone(), V, torch.float32, 0.1, g)
        if d > 30:                          # (otherwise the kernel between random points is numerically zero)
            P["raw_lengthscale"] = torch.full_like(P["raw_lengthscale"], 0.4 * d ** 0.5)
        x = X[M:].contiguous().to(dev)
        y = F[:, :p + 1].reshape(-1).contiguous().to(dev)
        D = torch.eye(d)[:p].repeat(B, 1).to(dev)
        P1 = {k: v.to(dev) for k, v in P.items()}
        P2 = dict(P1, raw_derivative_noise=torch.tensor([0.5], device=dev))
        nd = (d + 1) * 1_000_000

        def engine(c_step=True):
            eng = dsvgp_amd.ElboEngine(dev)
            eng.c_step = c_step
            return eng
        off, piece, two = engine(), engine(c_step=False), engine()
        for mll in ("ELBO", "PLL"):
            t = timed_many({"off": lambda: off.loss_and_grads(P1, x, y, D, nd, mll, fast=False),
                            "piecewise": lambda: piece.loss_and_grads(P1, x, y, D, nd, mll, fast=False),
                            "two": lambda: two.loss_and_grads(P2, x, y, D, nd, mll)}, args.reps)
            say("  1. %s step, ms (median, min, max): fast=False default path%s %.3f (%.3f, %.3f); piecewise per-output path %.3f (%.3f, %.3f); "
                "two noises %.3f (%.3f, %.3f)" % ((mll, " (one-call step)" if off.c_step_used else "") + t["off"] + t["piecewise"] + t["two"]))
            say("     ratios: two noises / piecewise %.4f, two noises / default %.4f" % (t["two"][0] / t["piecewise"][0], t["two"][0] / t["off"][0]))
        del off, piece
        budget = 4 << 30                                        # the chunk stays one chunk
        accs = {"plain": two.collapsed_accumulator(P1, workspace_budget=budget), "weighted": two.collapsed_accumulator(P2, workspace_budget=budget)}
        t = timed_many({k: (lambda k=k: accs[k].add(x, y, D)) for k in accs}, args.reps)
        say("  2. one statistics chunk (add), ms: unweighted %.3f (%.3f, %.3f); weighted %.3f (%.3f, %.3f); ratio %.4f"
            % (t["plain"] + t["weighted"] + (t["weighted"][0] / t["plain"][0],)))
        del accs, two
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
