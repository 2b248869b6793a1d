#!/usr/bin/env python3
"""Sample paths at their OWN points on the MI355X against what a caller had to do before, ALTERNATING in one process on the same
``SamplePaths``:

    own        SamplePaths.values_and_gradients_at(x[n, B, d])          (dsvgp_paths_eval_own)
    stacked    SamplePaths.values_and_gradients(x.reshape(n B, d)), then the diagonal blocks: all n paths at all n B points
    descend    SamplePaths.descend(x, lower, upper, iterations=20)      (dsvgp_paths_descend: one C call, no host read)
    loop       the same rule written with torch operations on the stacked evaluation (no host read either)

    turbo  d 20 M 500 p 5 F 2048 n 64 B 64 | rover d 200 M 512 p 3 F 2048 n 5 B 64 (composed) | fill d 20 M 500 p 5 F 2048 n 5 B 5000

Times: one pair of device events around every call, median over `--reps` (>= 20) alternating calls after `--warmup` calls of each.  The
flop count says the own-point form does about n / 4 times less work than the stacked one; the small grid (n ceil(B / 64) workgroups) and
the composed route's 10 + 2 n launches may eat that.  No speed bound is set.  Prints one JSON object; --out writes it to a file,
--summary a text digest (profiles/paths_own_summary.txt)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from paths_probe import medians, model  # noqa: E402

# name: (d, M, p, F, n, B)
GEOMS = {"turbo": (20, 500, 5, 2048, 64, 64), "rover": (200, 512, 3, 2048, 5, 64), "fill": (20, 500, 5, 2048, 5, 5000)}
ITER = 20


def stacked(paths, x):
    """all n paths at all n B points, then the diagonal blocks"""
    n, B, d = x.shape
    v, g = paths.values_and_gradients(x.reshape(n * B, d))
    s = torch.arange(n, device=x.device)
    return v.view(n, n, B)[s, s], g.view(n, n, B, d)[s, s]


def loop_descend(paths, x0, lower, upper, iterations, step0):
    """dsvgp_paths_descend's rule on the stacked evaluation"""
    x = torch.minimum(torch.maximum(x0, lower), upper)
    f, g = stacked(paths, x)
    eta = step0 / g.norm(dim=-1).clamp_min(1e-30)
    for _ in range(iterations):
        y = torch.minimum(torch.maximum(x - eta[..., None] * g, lower), upper)
        fy, gy = stacked(paths, y)
        take = fy <= f + 1e-4 * (g * (y - x)).sum(-1)
        x, g, f = torch.where(take[..., None], y, x), torch.where(take[..., None], gy, g), torch.where(take, fy, f)
        eta = torch.where(take, (2.0 * eta).clamp_max(1e30), 0.5 * eta)
    return x, f


def probe(dsvgp, dev, d, M, p, F, n, B, warmup, reps):
    P, x = model(dev, d, M, p, B)
    eng = dsvgp.ElboEngine(dev)
    paths = eng.sample_paths(P, n, F, generator=torch.Generator(device=dev).manual_seed(1))
    xs = (x[None] + 0.05 * torch.randn(n, B, d, generator=torch.Generator().manual_seed(3)).to(dev)).contiguous()
    lower, upper = torch.zeros(d, device=dev), torch.ones(d, device=dev)
    step0 = 0.25 * 0.4 * math.sqrt(d)
    t = medians({"own": lambda: paths.values_and_gradients_at(xs), "stacked": lambda: stacked(paths, xs)}, warmup, reps)
    t.update(medians({"descend": lambda: paths.descend(xs, lower, upper, iterations=ITER, initial_step=step0),
                      "loop": lambda: loop_descend(paths, xs, lower, upper, ITER, step0)}, warmup, reps))
    v, g = paths.values_and_gradients_at(xs)
    vs, gs = stacked(paths, xs)
    res_d = paths.descend(xs, lower, upper, iterations=ITER, initial_step=step0)
    _, f_loop = loop_descend(paths, xs, lower, upper, ITER, step0)
    start = paths.descend(xs, lower, upper, iterations=0, initial_step=step0)
    flops = 2.0 * n * B * (F + 3 * M) * d
    res = dict(d=d, M=M, p=p, F=F, n=n, B=B, route="fused" if d <= 32 else "composed", own_ms=t["own"], stacked_ms=t["stacked"],
               speedup_eval=t["stacked"] / t["own"], descend_ms=t["descend"], loop_ms=t["loop"], speedup_descend=t["loop"] / t["descend"],
               iterations=ITER, tflops_own=flops / (t["own"] * 1e-3) / 1e12, workgroups=n * ((B + 63) // 64) if d <= 32 else None,
               launches=None if d <= 32 else 10 + 2 * n,
               own_vs_stacked_values=float((v - vs).abs().max() / vs.abs().max()), own_vs_stacked_gradients=float((g - gs).abs().max() / gs.abs().max()),
               mean_gain_descend=float((start.values - res_d.values).mean()), mean_gain_loop=float((start.values - f_loop).mean()),
               accepted_mean=float(res_d.accepted.float().mean()), finite=bool(torch.isfinite(res_d.values).all() and torch.isfinite(g).all()),
               workspace_bytes=dsvgp._ops.paths_descend_workspace_bytes(M, d, F, n, B))
    del eng, paths
    torch.cuda.empty_cache()
    return res


def summary(res):
    lines = ["Sample paths at their own points vs all paths at the stacked points (then the diagonal), %s; median ms of %d alternating calls, device events"
             % (res["device"], res["reps"]),
             "%-6s %4s %4s %2s %5s %3s %5s %-8s %9s %10s %8s %11s %9s %8s %9s" % (
                 "shape", "d", "M", "p", "F", "n", "B", "route", "own ms", "stacked ms", "speedup", "descend ms", "loop ms", "speedup", "TFLOP/s")]
    for name, r in res["geometries"].items():
        lines.append("%-6s %4d %4d %2d %5d %3d %5d %-8s %9.3f %10.3f %8.2f %11.3f %9.3f %8.2f %9.2f" % (
            name, r["d"], r["M"], r["p"], r["F"], r["n"], r["B"], r["route"], r["own_ms"], r["stacked_ms"], r["speedup_eval"],
            r["descend_ms"], r["loop_ms"], r["speedup_descend"], r["tflops_own"]))
    for name in ("turbo", "rover", "fill"):
        if name not in res["geometries"]:
            lines.append("%-6s not measured" % name)
    lines.append("own: values_and_gradients_at.  descend / loop: %d iterations (21 evaluations).  TFLOP/s: 2 n B (F + 3 M) d over the own time." % ITER)
    for name, r in res["geometries"].items():
        lines.append("%-6s %s; own vs stacked max-norm difference: values %.1e, gradients %.1e; mean gain of the descent %.3f (loop %.3f), "
                     "accepted %.1f of %d" % (name, ("%d workgroups" % r["workgroups"]) if r["workgroups"] else ("%d launches per evaluation" % r["launches"]),
                                              r["own_vs_stacked_values"], r["own_vs_stacked_gradients"], r["mean_gain_descend"], r["mean_gain_loop"],
                                              r["accepted_mean"], ITER))
    lines.append("No speed bound is set.")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=",".join(GEOMS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--summary", default=None)
    args = ap.parse_args()
    import dsvgp_amd
    assert torch.cuda.is_available(), "paths_own_probe needs the GPU"
    assert args.reps >= 20, "medians over at least 20 calls"
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, reps=args.reps, geometries={})
    for name in args.only.split(","):
        d, M, p, F, n, B = GEOMS[name]
        res["geometries"][name] = probe(dsvgp_amd, dev, d, M, p, F, n, B, args.warmup, args.reps)
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
