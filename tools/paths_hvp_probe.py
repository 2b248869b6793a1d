#!/usr/bin/env python3
"""Hessian-vector products of the paths on the MI355X against the gradient of the same paths, ALTERNATING in one process on the same
``SamplePaths``:

    hvp                    SamplePaths.hvp(x, v)                 (dsvgp_paths_hvp: fused kernel for d <= 32, GEMM-composed beyond)
    values_and_gradients   SamplePaths.values_and_gradients(x)   (dsvgp_paths_eval)

    C4eval d 20 M 500 p 5 B 4096 n 64 F 2048 | rover d 200 M 512 p 3 B 5000 n 8 F 2048 (composed)

Times: one pair of device events around every call, median over `--reps` (>= 20) alternating calls after `--warmup` calls of each.
The flop rate of the product is against the count 2 B n (F + 4 M) d (per (point, i, sample) 4 d FMAs, per (point, j, sample) d).  No speed
bound is set; about 4/3 of the gradient's time at d <= 32 is arithmetic, not a result.  Prints one JSON object; --out writes it to a
file, --summary a text digest (profiles/paths_hvp_summary.txt)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from paths_probe import medians, model  # noqa: E402

# name: (d, M, p, B, n, F)
GEOMS = {"C4eval": (20, 500, 5, 4096, 64, 2048), "rover": (200, 512, 3, 5000, 8, 2048)}


def probe(dsvgp, dev, d, M, p, B, n, F, warmup, reps):
    P, x = model(dev, d, M, p, B)
    eng = dsvgp.ElboEngine(dev)
    paths = eng.sample_paths(P, n, F, generator=torch.Generator(device=dev).manual_seed(1))
    v = torch.randn(B, d, generator=torch.Generator().manual_seed(2)).to(dev)
    t = medians({"values_and_gradients": lambda: paths.values_and_gradients(x), "hvp": lambda: paths.hvp(x, v)}, warmup, reps)
    hv = paths.hvp(x, v)
    flops = 2.0 * B * n * (F + 4 * M) * d
    rows = paths._hvp_rows(B)
    res = dict(d=d, M=M, p=p, B=B, n=n, F=F, route="fused" if d <= 32 else "composed", hvp_ms=t["hvp"],
               values_and_gradients_ms=t["values_and_gradients"], ratio_hvp_over_gradients=t["hvp"] / t["values_and_gradients"],
               flops=flops, tflops=flops / (t["hvp"] * 1e-3) / 1e12, point_samples_per_s=B * n / (t["hvp"] * 1e-3),
               finite=bool(torch.isfinite(hv).all()), max_abs_hv=float(hv.abs().max()), rows_per_call=rows,
               workspace_bytes=dsvgp._ops.paths_hvp_workspace_bytes(M, d, F, n, rows))
    del eng, paths
    torch.cuda.empty_cache()
    return res


def summary(res):
    lines = ["Hessian-vector products of the paths vs values_and_gradients of the same paths, %s; median ms of %d alternating calls, device events"
             % (res["device"], res["reps"]),
             "%-7s %4s %4s %2s %6s %3s %5s %-8s %10s %12s %8s %8s %13s %12s" % (
                 "shape", "d", "M", "p", "B", "n", "F", "route", "hvp ms", "val+grad ms", "ratio", "TFLOP/s", "pt-samples/s", "workspace MiB")]
    for name, r in res["geometries"].items():
        lines.append("%-7s %4d %4d %2d %6d %3d %5d %-8s %10.3f %12.3f %8.2f %8.2f %13.3e %12.1f" % (
            name, r["d"], r["M"], r["p"], r["B"], r["n"], r["F"], r["route"], r["hvp_ms"], r["values_and_gradients_ms"],
            r["ratio_hvp_over_gradients"], r["tflops"], r["point_samples_per_s"], r["workspace_bytes"] / 1048576.0))
    lines.append("ratio: hvp over values_and_gradients.  TFLOP/s: 2 B n (F + 4 M) d over the hvp time.  No speed bound is set.")
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
    assert torch.cuda.is_available(), "paths_hvp_probe needs the GPU"
    assert args.reps >= 20, "medians over at least 20 calls"
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, reps=args.reps, geometries={})
    for name in args.only.split(","):
        d, M, p, B, n, F = GEOMS[name]
        res["geometries"][name] = probe(dsvgp_amd, dev, d, M, p, B, n, F, args.warmup, args.reps)
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
