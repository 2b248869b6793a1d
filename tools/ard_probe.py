#!/usr/bin/env python3
"""What ARD lengthscales cost: a training step and a prediction of a model with raw_lengthscale [1, d] against the scalar-lengthscale
model ON THE SAME PATH (piecewise per-output: the one-call steps switched off for the scalar model), ALTERNATING in one process on the
same parameters and batch.  The ARD model carries d equal lengthscales, so both compute the same numbers (the agreement is printed).

    step PLL / step ELBO (per-output, fast=False)    ElboEngine.loss_and_grads
        ard       raw_lengthscale [1, d]: ARD packs, wide / rectangular forward, dsvgp_kernel_bwd_ard twice, the diagonal's backward
        scalar    raw_lengthscale [1, 1], c_step = False: dsvgp_kernel_fwd / dsvgp_kernel_bwd (canonical-direction kernels where stated)
        onecall   the scalar model as it trains by default (the one-call per-output step), for scale
    predict (cache=True: the factor is kept, K_ZX + solve + statistics per call)    ElboEngine.predict

    C4 d 20 M 500 p 5 B 4096 | d200 d 200 M 512 p 2 B 2048

Times: one pair of device events around every call, median over `--reps` (>= 20) calls after `--warmup` calls of each.  Prints one JSON
object; --out writes it to a file, --summary a text digest."""
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
    Pard = dict(P, raw_lengthscale=P["raw_lengthscale"].reshape(1, 1).expand(1, d).contiguous())
    g = torch.Generator().manual_seed(1)
    y = torch.randn(B * (p + 1), generator=g).to(dev)
    nd = 100.0 * B
    ard, sc, one = dsvgp.ElboEngine(dev), dsvgp.ElboEngine(dev), dsvgp.ElboEngine(dev)
    sc.c_step = False
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    res = dict(d=d, M=M, p=p, B=B)
    for mll in ("PLL", "ELBO"):
        ra = ard.loss_and_grads(Pard, x, y, D, nd, mll)
        rs = sc.loss_and_grads(P, x, y, D, nd, mll, fast=False)
        one.loss_and_grads(P, x, y, D, nd, mll, fast=False)
        assert not ard.c_step_used and not sc.c_step_used
        res["step_%s_onecall_used" % mll] = bool(one.c_step_used)
        res["step_%s_rel_diff_loss" % mll] = abs(float(ra[0]) - float(rs[0])) / abs(float(rs[0]))
        res["step_%s_rel_diff_dZ" % mll] = rel(ra[1]["inducing_points"], rs[1]["inducing_points"])
        res["step_%s_rel_diff_sum_d_raw_ell" % mll] = abs(float(ra[1]["raw_lengthscale"].sum()) - float(rs[1]["raw_lengthscale"].sum())) / \
            abs(float(rs[1]["raw_lengthscale"].sum()))
        t = medians({"ard": lambda: ard.loss_and_grads(Pard, x, y, D, nd, mll),
                     "scalar": lambda: sc.loss_and_grads(P, x, y, D, nd, mll, fast=False),
                     "onecall": lambda: one.loss_and_grads(P, x, y, D, nd, mll, fast=False)}, warmup, reps)
        for k, v in t.items():
            res["step_%s_%s_ms" % (mll, k)] = v
        res["step_%s_ratio" % mll] = t["ard"] / t["scalar"]
    ma, va = ard.predict(Pard, x, D, cache=True)
    ms, vs = sc.predict(P, x, D, cache=True)
    res["predict_rel_diff_mean"], res["predict_rel_diff_variance"] = rel(ma, ms), rel(va, vs)
    t = medians({"ard": lambda: ard.predict(Pard, x, D, cache=True), "scalar": lambda: sc.predict(P, x, D, cache=True)}, warmup, reps)
    res["predict_ard_ms"], res["predict_scalar_ms"], res["predict_ratio"] = t["ard"], t["scalar"], t["ard"] / t["scalar"]
    del ard, sc, one
    torch.cuda.empty_cache()
    return res


def summary(res):
    lines = ["ARD lengthscales (d equal ones) vs the scalar model on the piecewise per-output path, %s; median ms of %d alternating calls, "
             "device events" % (res["device"], res["reps"]),
             "%-5s %3s %4s %2s %5s | %8s %8s %6s %8s | %8s %8s %6s %8s | %8s %8s %6s" % (
                 "", "d", "M", "p", "B", "PLL ard", "scalar", "ratio", "onecall", "ELBO ard", "scalar", "ratio", "onecall", "pred ard",
                 "scalar", "ratio")]
    for name, r in res["geometries"].items():
        lines.append("%-5s %3d %4d %2d %5d | %8.3f %8.3f %6.3f %8.3f | %8.3f %8.3f %6.3f %8.3f | %8.3f %8.3f %6.3f" % (
            name, r["d"], r["M"], r["p"], r["B"], r["step_PLL_ard_ms"], r["step_PLL_scalar_ms"], r["step_PLL_ratio"],
            r["step_PLL_onecall_ms"], r["step_ELBO_ard_ms"], r["step_ELBO_scalar_ms"], r["step_ELBO_ratio"], r["step_ELBO_onecall_ms"],
            r["predict_ard_ms"], r["predict_scalar_ms"], r["predict_ratio"]))
        lines.append("      the two models agree to: loss %.1e, Z-bar %.1e, sum of d raw_lengthscale %.1e (PLL step); mean %.1e, variance %.1e "
                     "(predict); onecall took the one-call step: %s" % (
                         r["step_PLL_rel_diff_loss"], r["step_PLL_rel_diff_dZ"], r["step_PLL_rel_diff_sum_d_raw_ell"],
                         r["predict_rel_diff_mean"], r["predict_rel_diff_variance"], r["step_PLL_onecall_used"]))
    lines.append("step: loss_and_grads, per-output (fast=False); scalar: c_step = False; onecall: the scalar model's default per-output step.")
    lines.append("predict: cache=True, K_ZX assembly + solve + statistics per call.")
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
    assert torch.cuda.is_available(), "ard_probe needs the GPU"
    assert args.reps >= 20, "medians over at least 20 calls"
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
