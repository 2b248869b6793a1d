#!/usr/bin/env python3
"""What the Matern-5/2 kernel costs: a training step and a cached prediction of a Matern-ARD model (``ElboEngine.kernel = "matern52"``,
raw_lengthscale [1, d]) against the RBF-ARD model ON THE SAME PATH (ARD packs, piecewise per-output), ALTERNATING in one process on the
same parameters and batch; and the two pairs of tile kernels by themselves (forward K_ZX, kernel backward of K_ZX).

    step PLL / step ELBO    ElboEngine.loss_and_grads (fast=None: the per-output ARD path for both)
    predict                 ElboEngine.predict, cache=True: the factor is kept, K_ZX + solve + statistics per call
    fwd tile / bwd          kernel_fwd_matern52 vs kernel_fwd_rect, kernel_bwd_matern52 vs kernel_bwd_ard on the [M (p+1), B (p+1)] K_ZX
                            (the backward's launches after the Tbar tiles are the same kernels on both sides)

    C4 d 20 M 500 p 5 B 4096 | d200 d 200 M 512 p 2 B 2048

Times: one pair of device events around every call, median over `--reps` (>= 30) alternating calls after `--warmup` calls of each.  Prints
one JSON object; --out writes it to a file, --summary a text digest."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mean_predict_probe import medians, model  # noqa: E402

# name: (d, M, p, B)
GEOMS = {"C4": (20, 500, 5, 4096), "d200": (200, 512, 2, 2048)}


def probe(dsvgp, dev, d, M, p, B, warmup, reps):
    P, x, D = model(dev, d, M, p, B)
    P = dict(P, raw_lengthscale=P["raw_lengthscale"].reshape(1, 1).expand(1, d).contiguous())
    g = torch.Generator().manual_seed(1)
    y = torch.randn(B * (p + 1), generator=g).to(dev)
    nd = 100.0 * B
    rbf, mat = dsvgp.ElboEngine(dev), dsvgp.ElboEngine(dev)
    mat.kernel = "matern52"
    res = dict(d=d, M=M, p=p, B=B)
    for mll in ("PLL", "ELBO"):
        rbf.loss_and_grads(P, x, y, D, nd, mll)
        mat.loss_and_grads(P, x, y, D, nd, mll)
        assert not rbf.c_step_used and not mat.c_step_used
        t = medians({"rbf": lambda: rbf.loss_and_grads(P, x, y, D, nd, mll), "matern": lambda: mat.loss_and_grads(P, x, y, D, nd, mll)},
                    warmup, reps)
        res["step_%s_rbf_ms" % mll], res["step_%s_matern_ms" % mll] = t["rbf"], t["matern"]
        res["step_%s_ratio" % mll] = t["matern"] / t["rbf"]
    t = medians({"rbf": lambda: rbf.predict(P, x, D, cache=True), "matern": lambda: mat.predict(P, x, D, cache=True)}, warmup, reps)
    res["predict_rbf_ms"], res["predict_matern_ms"], res["predict_ratio"] = t["rbf"], t["matern"], t["matern"] / t["rbf"]
    # the tile kernels by themselves, on K_ZX
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    ell, hyp = ops.hyp_forward_ard(ctx, P["raw_lengthscale"], P["raw_outputscale"], P["raw_noise"])
    center = ops.column_mean(ctx, P["inducing_points"])
    pz = ops.pack_points_ard(ctx, P["inducing_points"], P["inducing_directions"].contiguous(), p, ell, center)
    px = ops.pack_points_ard(ctx, x, D, p, ell, center)
    out = torch.empty(M * (p + 1), B * (p + 1), device=dev)
    G = torch.randn(M * (p + 1), B * (p + 1), generator=g).to(dev)
    dZ, dV, dl, dh = torch.zeros(M, d, device=dev), torch.zeros(M * p, d, device=dev), torch.zeros(d, device=dev), torch.zeros(4, device=dev)
    ws = torch.empty(ops.kernel_bwd_matern52_workspace_bytes(M, p, B, p, d), dtype=torch.uint8, device=dev)
    t = medians({"rbf": lambda: ops.kernel_fwd_rect(ctx, pz, M, p, px, B, p, d, hyp, out=out),
                 "matern": lambda: ops.kernel_fwd_matern52(ctx, pz, M, p, px, B, p, d, hyp, out=out)}, warmup, reps)
    res["fwd_tile_rbf_ms"], res["fwd_tile_matern_ms"], res["fwd_tile_ratio"] = t["rbf"], t["matern"], t["matern"] / t["rbf"]
    t = medians({"rbf": lambda: ops.kernel_bwd_ard(ctx, G, pz, M, p, px, B, p, d, ell, hyp, False, dZ, dV, dl, dh, ws),
                 "matern": lambda: ops.kernel_bwd_matern52(ctx, G, pz, M, p, px, B, p, d, ell, hyp, False, dZ, dV, dl, dh, ws)}, warmup, reps)
    res["bwd_rbf_ms"], res["bwd_matern_ms"], res["bwd_ratio"] = t["rbf"], t["matern"], t["matern"] / t["rbf"]
    del rbf, mat
    torch.cuda.empty_cache()
    return res


def summary(res):
    lines = ["Matern-5/2 ARD vs RBF ARD on the piecewise per-output path, %s; median ms of %d alternating calls, device events"
             % (res["device"], res["reps"]),
             "%-5s %3s %4s %2s %5s | %8s %8s %6s | %8s %8s %6s | %8s %8s %6s | %8s %8s %6s | %8s %8s %6s" % (
                 "", "d", "M", "p", "B", "PLL rbf", "matern", "ratio", "ELBO rbf", "matern", "ratio", "pred rbf", "matern", "ratio",
                 "fwd rbf", "matern", "ratio", "bwd rbf", "matern", "ratio")]
    for name, r in res["geometries"].items():
        lines.append("%-5s %3d %4d %2d %5d | %8.3f %8.3f %6.3f | %8.3f %8.3f %6.3f | %8.3f %8.3f %6.3f | %8.3f %8.3f %6.3f | %8.3f %8.3f %6.3f" % (
            name, r["d"], r["M"], r["p"], r["B"], r["step_PLL_rbf_ms"], r["step_PLL_matern_ms"], r["step_PLL_ratio"],
            r["step_ELBO_rbf_ms"], r["step_ELBO_matern_ms"], r["step_ELBO_ratio"], r["predict_rbf_ms"], r["predict_matern_ms"],
            r["predict_ratio"], r["fwd_tile_rbf_ms"], r["fwd_tile_matern_ms"], r["fwd_tile_ratio"], r["bwd_rbf_ms"], r["bwd_matern_ms"],
            r["bwd_ratio"]))
    lines.append("step: loss_and_grads on raw_lengthscale [1, d] (the ARD path for both kernels).  predict: cache=True.")
    lines.append("fwd: the K_ZX forward tile kernel alone.  bwd: the whole kernel backward of K_ZX (Tbar tiles, contraction, ARD reductions); the")
    lines.append("Matern Tbar kernel recomputes its radial factors per task and keeps exp(-a) per pair in LDS (no per-pair array added).")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", default=",".join(GEOMS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--summary", default=None)
    args = ap.parse_args()
    import dsvgp_amd
    assert torch.cuda.is_available(), "matern_probe needs the GPU"
    assert args.reps >= 30, "medians over at least 30 calls"
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, reps=args.reps, geometries={})
    for name in args.only.split(","):
        d, M, p, B = GEOMS[name]
        res["geometries"][name] = probe(dsvgp_amd, dev, d, M, p, B, args.warmup, args.reps)
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
