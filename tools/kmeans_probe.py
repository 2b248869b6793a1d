#!/usr/bin/env python3
"""One Lloyd iteration on the MI355X against the eager form a caller would write without the kernels, ALTERNATING in one process:

    lloyd      _ops.kmeans_lloyd_(x, Z, 1)      (dsvgp_kmeans_lloyd: assign, inertia, update, closing assign, counts; no host read)
    assign     _ops.kmeans_assign               (dsvgp_kmeans_assign alone)
    update     _ops.kmeans_update_              (dsvgp_kmeans_update alone)
    eager      torch.cdist in row blocks of 65536, argmin, index_add_, divide (one assignment and one update; index_add_ adds through
               floating-point atomics: its result changes from run to run)

    c4     N 1e6 d 20  M 500  (fused assignment)  |  rover  N 1e5 d 200 M 512  (composed assignment)

Times: one pair of device events around every call, median over `--reps` (>= 20) alternating calls after `--warmup` calls of each.  A
Lloyd call holds TWO assignments and one update.  No speed bound is set.  Prints one JSON object; --out writes it, --summary writes a
text digest (profiles/kmeans_probe.txt)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from paths_probe import medians  # noqa: E402

# name: (N, d, M)
GEOMS = {"c4": (1_000_000, 20, 500), "rover": (100_000, 200, 512)}


def eager(x, Z, block=65536):
    labels = torch.empty(x.shape[0], dtype=torch.long, device=x.device)
    for r0 in range(0, x.shape[0], block):
        labels[r0:r0 + block] = torch.cdist(x[r0:r0 + block], Z).argmin(dim=1)
    sums = torch.zeros_like(Z).index_add_(0, labels, x)
    counts = torch.bincount(labels, minlength=Z.shape[0])
    return torch.where(counts[:, None] > 0, sums / counts.clamp_min(1)[:, None], Z), labels


def probe(dsvgp, dev, N, d, M, warmup, reps):
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(N, d, generator=g).to(dev)
    Z0 = x[torch.randperm(N, generator=g)[:M].to(dev)].contiguous()
    ws = torch.empty(max(ops.kmeans_workspace_bytes(N, d, M), 16), dtype=torch.uint8, device=dev)
    labels, dist2 = ops.kmeans_assign(ctx, x, Z0, workspace=ws)
    counts = torch.empty(M, dtype=torch.int32, device=dev)
    inertia, moved = torch.empty(2, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    Zw, lab_w, d2_w = Z0.clone(), labels.clone(), dist2.clone()

    def lloyd():
        Zw.copy_(Z0)
        ops.kmeans_lloyd_(ctx, x, Zw, 1, labels=lab_w, dist2=d2_w, counts=counts, inertia=inertia, moved=moved, workspace=ws)

    def update():
        Zw.copy_(Z0)
        ops.kmeans_update_(ctx, x, labels, Zw, counts=counts)

    t = medians({"lloyd": lloyd, "eager": lambda: eager(x, Z0)}, warmup, reps)
    t.update(medians({"assign": lambda: ops.kmeans_assign(ctx, x, Z0, labels=lab_w, dist2=d2_w, workspace=ws), "update": update}, warmup, reps))
    lloyd()
    Ze, le = eager(x, Z0)
    res = dict(N=N, d=d, M=M, route="fused" if d <= 32 else "composed", lloyd_ms=t["lloyd"], assign_ms=t["assign"], update_ms=t["update"],
               eager_ms=t["eager"], speedup=t["eager"] / t["lloyd"], tflops_assign=2.0 * N * M * d / (t["assign"] * 1e-3) / 1e12,
               labels_differing_from_eager=int((labels.long() != le).sum()), centroid_diff_vs_eager=float((Zw - Ze).abs().max()),
               inertia=[float(v) for v in inertia.tolist()], moved=int(moved[0]), workspace_bytes=ops.kmeans_workspace_bytes(N, d, M))
    del x, ws
    torch.cuda.empty_cache()
    return res


def summary(res):
    lines = ["One Lloyd iteration (two assignments, one update) vs eager torch (cdist in row blocks, argmin, index_add_), %s; median ms of %d "
             "alternating calls, device events" % (res["device"], res["reps"]),
             "%-6s %8s %4s %4s %-8s %9s %10s %10s %9s %8s %14s" % ("shape", "N", "d", "M", "route", "lloyd ms", "assign ms", "update ms",
                                                                  "eager ms", "speedup", "assign TFLOP/s")]
    for name, r in res["geometries"].items():
        lines.append("%-6s %8d %4d %4d %-8s %9.3f %10.3f %10.3f %9.3f %8.2f %14.2f" % (
            name, r["N"], r["d"], r["M"], r["route"], r["lloyd_ms"], r["assign_ms"], r["update_ms"], r["eager_ms"], r["speedup"],
            r["tflops_assign"]))
    for name in GEOMS:
        if name not in res["geometries"]:
            lines.append("%-6s not measured" % name)
    for name, r in res["geometries"].items():
        lines.append("%-6s labels differing from eager's %d of %d, centroids after the update differ by %.1e; inertia %.4f -> %.4f, moved %d; "
                     "workspace %d bytes" % (name, r["labels_differing_from_eager"], r["N"], r["centroid_diff_vs_eager"], r["inertia"][0],
                                             r["inertia"][1], r["moved"], r["workspace_bytes"]))
    lines.append("speedup: eager (ONE assignment + update) over lloyd (TWO assignments + update + inertia + counts).  TFLOP/s: 2 N M d over the "
                 "assignment.  No speed bound is set.")
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
    assert torch.cuda.is_available(), "kmeans_probe needs the GPU"
    assert args.reps >= 20, "medians over at least 20 calls"
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, reps=args.reps, geometries={})
    for name in args.only.split(","):
        N, d, M = GEOMS[name]
        res["geometries"][name] = probe(dsvgp_amd, dev, N, d, M, args.warmup, args.reps)
        print(json.dumps({name: res["geometries"][name]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.summary:
        with open(args.summary, "w") as f:
            f.write(summary(res))
    print(summary(res))


if __name__ == "__main__":
    main()
