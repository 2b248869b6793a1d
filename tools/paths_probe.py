#!/usr/bin/env python3
"""Pathwise posterior samples on the MI355X against what a user of the joint form does for the same request, ALTERNATING in one
process on the same model:

    new       SamplePaths.values(x) / values_and_gradients(x)            (csrc/paths.hip: fused kernel for d <= 32, GEMM-composed beyond)
    present   predict_joint(x) + covariance_root + draw of n samples     (what ``model.posterior(x).sample(torch.Size([n]))`` runs: the
              whole [B, B] covariance and its fp64 Cholesky root), only where B <= --joint-max; beyond it is "not measured"

    C4eval d 20 M 500 p 5 B 4096 n 64 F 2048 | rover d 200 M 512 p 3 B 5000 n 8 F 2048 (composed) | grid d 3 M 500 p 3 B 65536 n 8 F 2048

Times: one pair of device events around every call, median over `--reps` (>= 20) alternating calls after `--warmup` calls of each.
`build_ms`: host clock around ``sample_paths(params, n, F)`` ending in a device synchronise (factorisation, Phi_Z', two solves, packing),
median of 5 after a first call.  The flop rate is against the count 2 B n (F + 2 M)(d + 1).  Prints one JSON object; --out writes it to
a file, --summary a text digest."""
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

# name: (d, M, p, B, n, F)
GEOMS = {"C4eval": (20, 500, 5, 4096, 64, 2048), "rover": (200, 512, 3, 5000, 8, 2048), "grid": (3, 500, 3, 65536, 8, 2048)}


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
    return {k: v.to(dev) for k, v in P.items()}, torch.rand(B, d, generator=g).to(dev)


def probe(dsvgp, dev, d, M, p, B, n, F, warmup, reps, joint_max):
    P, x = model(dev, d, M, p, B)
    eng = dsvgp.ElboEngine(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    builds = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        paths = eng.sample_paths(P, n, F, generator=gen)
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t0) * 1e3)
    fns = {"values": lambda: paths.values(x), "values_and_gradients": lambda: paths.values_and_gradients(x)}
    joint = B <= joint_max
    if joint:
        eng2 = dsvgp.ElboEngine(dev)         # (its own factor buffers)

        def present():
            mu, Sigma = eng2.predict_joint(P, x, None)
            root = eng2.covariance_root(Sigma)
            return eng2.draw(mu, root, torch.randn(n, mu.shape[0], dtype=mu.dtype, device=dev))
        fns["present"] = present
    t = medians(fns, warmup, reps)
    vals, grads = paths.values_and_gradients(x)
    flops = 2.0 * B * n * (F + 2 * M) * (d + 1)
    res = dict(d=d, M=M, p=p, B=B, n=n, F=F, route="fused" if d <= 32 else "composed", values_ms=t["values"],
               values_and_gradients_ms=t["values_and_gradients"], present_values_ms=t.get("present", "not measured"),
               ratio_present_over_values=(t["present"] / t["values"]) if joint else "not measured",
               present_gradients_ms="not measured", flops=flops, tflops=flops / (t["values_and_gradients"] * 1e-3) / 1e12,
               point_samples_per_s=B * n / (t["values_and_gradients"] * 1e-3), build_ms=statistics.median(builds[1:]),
               build_first_ms=builds[0], finite=bool(torch.isfinite(vals).all() and torch.isfinite(grads).all()),
               value_std_over_samples=float(vals.std(dim=0).mean()),
               workspace_bytes=dsvgp._ops.paths_workspace_bytes(M, d, F, n, paths._rows(B, True), True),
               rows_per_call=paths._rows(B, True), weights_bytes=dsvgp._ops.paths_weights_bytes(M, d, F, n))
    del eng, paths
    torch.cuda.empty_cache()
    return res


def summary(res):
    lines = ["pathwise posterior samples vs predict_joint + covariance_root + draw, %s; median ms of %d alternating calls, device events"
             % (res["device"], res["reps"]),
             "%-7s %4s %4s %2s %6s %3s %5s %-8s %10s %12s %12s %8s %8s %13s %9s" % (
                 "shape", "d", "M", "p", "B", "n", "F", "route", "values ms", "val+grad ms", "present ms", "ratio", "TFLOP/s", "pt-samples/s",
                 "build ms")]
    fmt = lambda v, f: (f % v) if not isinstance(v, str) else v
    for name, r in res["geometries"].items():
        lines.append("%-7s %4d %4d %2d %6d %3d %5d %-8s %10.3f %12.3f %12s %8s %8.2f %13.3e %9.2f" % (
            name, r["d"], r["M"], r["p"], r["B"], r["n"], r["F"], r["route"], r["values_ms"], r["values_and_gradients_ms"],
            fmt(r["present_values_ms"], "%.2f"), fmt(r["ratio_present_over_values"], "%.1f"), r["tflops"], r["point_samples_per_s"],
            r["build_ms"]))
    lines.append("present: the joint form on the value rows (B x B covariance, fp64 root, n draws); its gradient form (B (d + 1) squared) is not")
    lines.append("measured at these sizes.  TFLOP/s: 2 B n (F + 2 M)(d + 1) over the val+grad time.  build ms: sample_paths(params, n, F), host")
    lines.append("clock to a device synchronise, median of 5.")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--joint-max", type=int, default=8192, help="largest B at which the joint form is timed")
    ap.add_argument("--only", default=",".join(GEOMS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--summary", default=None)
    args = ap.parse_args()
    import dsvgp_amd
    assert torch.cuda.is_available(), "paths_probe needs the GPU"
    assert args.reps >= 20, "medians over at least 20 calls"
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, reps=args.reps, geometries={})
    for name in args.only.split(","):
        d, M, p, B, n, F = GEOMS[name]
        res["geometries"][name] = probe(dsvgp_amd, dev, d, M, p, B, n, F, args.warmup, args.reps, args.joint_max)
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
