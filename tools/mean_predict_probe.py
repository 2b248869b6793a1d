#!/usr/bin/env python3
"""The posterior-mean predictor on the MI355X against the present prediction path, ALTERNATING in one process on the same model:

    new       MeanPredictor.mean(x, D)                       (csrc/predict_mean.hip: fused kernel for d <= 32, GEMM-composed beyond)
    present   ElboEngine.predict(params, x, D, cache=True)   on a cache hit: K_ZX assembly, fp64 panel solve, W = L_S^T A, statistics

    C4eval d 20 M 500 p 5 B 4096 | C2 d 5 M 200 p 2 B 512 | bunny d 3 M 500 p 3 B 65536 | rover_wide d 200 M 512 p 3 B 2048 (composed)

Times: one pair of device events around every call, median over `--reps` (>= 20) calls after `--warmup` calls of each; for the new path
also the mean over `--burst` back-to-back calls between one pair of events (a single call of a few microseconds is at the resolution of
the events).  `build_ms`: host clock around ``mean_predictor(params)`` ending in a device synchronise (factorisation, transposed solve,
packing), median of 5.  Derived from the shapes by this file: the flops the closed form needs (8 B M d, + 2 B pd d for the direction
rows), the flops the present path cannot avoid (2 M'^2 B' for the solve and as many for W), points per second.  The two paths' means are
compared at the timed size.  Prints one JSON object; --out writes it to a file, --summary a text digest."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

f32 = torch.float32
# name: (d, M, p, B)
GEOMS = {"C4eval": (20, 500, 5, 4096), "C2": (5, 200, 2, 512), "bunny": (3, 500, 3, 65536), "rover_wide": (200, 512, 3, 2048)}


def medians(fns, warmup, reps):
    """fns: name -> callable; called in turn (a, b, a, b, ...), every call between its own pair of events"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}


def burst(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def model(dev, d, M, p, B):
    g = torch.Generator().manual_seed(0)
    Mp = M * (p + 1)
    raw = lambda v: math.log(math.expm1(v))
    P = dict(inducing_points=torch.rand(M, d, generator=g),
             inducing_directions=torch.eye(d)[:p].repeat(M, 1) + 0.1 * torch.randn(M * p, d, generator=g),
             variational_mean=0.2 * torch.randn(Mp, generator=g),
             chol_variational_covar=torch.eye(Mp) + 0.05 * torch.randn(Mp, Mp, generator=g) / math.sqrt(Mp),
             constant=torch.tensor([0.1]), raw_outputscale=torch.tensor(0.2),
             raw_lengthscale=torch.tensor([[raw(0.4 * math.sqrt(d))]]), raw_noise=torch.tensor([-0.5]))
    x = torch.rand(B, d, generator=g)
    D = torch.eye(d)[:p].repeat(B, 1)
    return {k: v.to(dev) for k, v in P.items()}, x.to(dev), D.to(dev).contiguous()


def probe(dsvgp, dev, d, M, p, B, warmup, reps, nburst):
    P, x, D = model(dev, d, M, p, B)
    eng = dsvgp.ElboEngine(dev)
    builds = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred = eng.mean_predictor(P)
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t0) * 1e3)
    eng2 = dsvgp.ElboEngine(dev)         # (its own factor buffers: the predictor's build does not disturb this engine's cache)
    mu_old, _ = eng2.predict(P, x, D, cache=True)
    mu_new = pred.mean(x, D)
    fns = {"new": lambda: pred.mean(x, D), "present": lambda: eng2.predict(P, x, D, cache=True)}
    t = medians(fns, warmup, reps)
    t_burst = burst(fns["new"], nburst)
    t_grad = burst(lambda: pred.value_and_gradient(x), nburst)
    Mq, Bq = M * (p + 1), B * (p + 1)
    f_new, f_old = 8.0 * B * M * d + 2.0 * B * p * d, 4.0 * Mq * Mq * Bq
    res = dict(d=d, M=M, p=p, pd=p, B=B, path="fused" if d <= 32 else "composed", new_ms=t["new"], present_ms=t["present"],
               ratio_present_over_new=t["present"] / t["new"], new_burst_ms=t_burst, ratio_present_over_new_burst=t["present"] / t_burst,
               value_and_gradient_burst_ms=t_grad, points_per_s_new=B / (t_burst * 1e-3), points_per_s_present=B / (t["present"] * 1e-3),
               flops_new=f_new, flops_present_at_least=f_old, gflops_new=f_new / (t_burst * 1e-3) / 1e9,
               build_ms=statistics.median(builds[1:]), build_first_ms=builds[0],
               max_rel_diff_of_the_means=float((mu_new - mu_old).abs().max() / mu_old.abs().max()),
               max_abs_mean_minus_constant=float((mu_old - 0.1).abs().max()),
               workspace_bytes=dsvgp._ops.mean_workspace_bytes(M, d, B, p), weights_bytes=dsvgp._ops.mean_weights_bytes(M, d))
    del eng, eng2, pred
    torch.cuda.empty_cache()
    return res


def summary(res):
    lines = ["posterior-mean predictor vs ElboEngine.predict (cache hit), %s; median ms of %d alternating calls, device events"
             % (res["device"], res["reps"]),
             "%-11s %4s %4s %2s %6s %-8s %10s %10s %8s %12s %8s %12s %9s %9s" % (
                 "shape", "d", "M", "p", "B", "path", "present ms", "new ms", "ratio", "new burst ms", "ratio", "points/s new", "build ms",
                 "rel diff")]
    for name, r in res["geometries"].items():
        lines.append("%-11s %4d %4d %2d %6d %-8s %10.3f %10.4f %8.1f %12.4f %8.1f %12.3e %9.2f %9.1e" % (
            name, r["d"], r["M"], r["p"], r["B"], r["path"], r["present_ms"], r["new_ms"], r["ratio_present_over_new"], r["new_burst_ms"],
            r["ratio_present_over_new_burst"], r["points_per_s_new"], r["build_ms"], r["max_rel_diff_of_the_means"]))
    lines.append("new burst ms: mean over %d back-to-back calls between one pair of events; build ms: mean_predictor(params), host clock to a"
                 % res["burst"])
    lines.append("device synchronise, median of 5; rel diff: max |mean_new - mean_present| / max |mean_present| at the timed size")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--burst", type=int, default=100)
    ap.add_argument("--only", default=",".join(GEOMS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--summary", default=None)
    args = ap.parse_args()
    import dsvgp_amd
    assert torch.cuda.is_available(), "mean_predict_probe needs the GPU"
    assert args.reps >= 20, "medians over at least 20 calls"
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, reps=args.reps, burst=args.burst, geometries={})
    for name in args.only.split(","):
        d, M, p, B = GEOMS[name]
        res["geometries"][name] = probe(dsvgp_amd, dev, d, M, p, B, args.warmup, args.reps, args.burst)
        print(json.dumps({name: res["geometries"][name]}), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.summary:
        with open(args.summary, "w") as f:
            f.write(summary(res))
    print(summary(res))


if __name__ == "__main__":
    main()
