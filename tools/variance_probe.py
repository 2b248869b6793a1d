#!/usr/bin/env python3
"""The posterior-variance predictor on the MI355X against the present prediction path, ALTERNATING in one process on the same model:

    values     VariancePredictor.variance(x)                   (csrc/predict_variance.hip: K_ZX, V = Q K_ZX in fp64, one contraction)
    present    ElboEngine.predict(params, x, None, cache=True)  on a cache hit: K_ZX, fp64 panel solve, W = L_S^T A, statistics
    gradient   VariancePredictor.variance_and_gradient(x)
    alt_grad   what the present code offers for the gradient: `present` plus a SECOND solve of B columns (L^-T, fp64) and the kernel
               backward of its transposed result (the (S - I) product in between is left out: in favour of the alternative)

    C4eval d 20 M 500 p 5 B 4096 | C2 d 5 M 200 p 2 B 512 | wide d 200 M 512 p 3 B 2048 (composed route)

Times: one pair of device events around every call, median over `--reps` (>= 20) calls after `--warmup` calls of each, the four callables
in turn.  `descend_ms_per_iteration`: one C call of 10 iterations continued from a state, between one pair of events, divided by 10, at 64
and 512 starts ("lcb").  `build_ms`: host clock around ``variance_predictor(params)`` ending in a device synchronise (factorisation, the
two M'-column solves for Q, the mean's solve, packing), median of 5.  Prints one JSON object; --out writes it, --summary a text digest."""
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

from mean_predict_probe import medians, model  # noqa: E402

f32, f64 = torch.float32, torch.float64
# name: (d, M, p, B)
GEOMS = {"C4eval": (20, 500, 5, 4096), "C2": (5, 200, 2, 512), "wide": (200, 512, 3, 2048)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def probe(dsvgp, dev, d, M, p, B, warmup, reps):
    ops = dsvgp._ops
    P, x, _ = model(dev, d, M, p, B)
    Mp = M * (p + 1)
    eng = dsvgp.ElboEngine(dev)
    builds = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred = eng.variance_predictor(P)
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t0) * 1e3)
    eng2 = dsvgp.ElboEngine(dev)         # (its own factor buffers: the predictor's build does not disturb this engine's cache)
    _, varn_old = eng2.predict(P, x, None, cache=True)
    var_new = pred.variance(x, with_noise=True)
    # the alternative for the gradient, on the cached factor of eng2
    ctx = ops.Context.get(dev)
    _, hyp, packZ, L = eng2._eval_cache[:4]
    packX = ops.pack_points(ctx, x, None, 0, hyp, eng2.center)
    rhs = torch.randn(Mp, B, dtype=f64, device=dev)
    sol = torch.empty(Mp, B, dtype=f32, device=dev)
    G = torch.empty(B, Mp, dtype=f32, device=dev)
    gx, dh = torch.zeros(B, d, dtype=f32, device=dev), torch.zeros(4, dtype=f32, device=dev)
    bws = torch.empty(ops.kernel_bwd_rect_workspace_bytes(B, 0, M, p, d), dtype=torch.uint8, device=dev)

    def alt_grad():
        eng2.predict(P, x, None, cache=True)
        ops.trsm(ctx, L, rhs, True, None, sol, eng2.trsm_nb, eng2._inverse_ws, reuse_inverse=True)
        ops.transpose_f32(ctx, sol, G)
        gx.zero_()
        ops.kernel_bwd_rect(ctx, G, packX, B, 0, packZ, M, p, d, hyp, gx, None, dh, bws)

    fns = {"values": lambda: pred.variance(x), "present": lambda: eng2.predict(P, x, None, cache=True),
           "gradient": lambda: pred.variance_and_gradient(x), "alt_grad": alt_grad}
    t = medians(fns, warmup, reps)
    lower, upper = torch.zeros(d, device=dev), torch.ones(d, device=dev)
    descend = {}
    for n in (64, 512):
        st = pred.descend(x[:n], lower, upper, "lcb", iterations=2)
        pred.descend(None, lower, upper, "lcb", iterations=10, state=st)
        ts = [timed(lambda: pred.descend(None, lower, upper, "lcb", iterations=10, state=st)) / 10 for _ in range(5)]
        descend[str(n)] = statistics.median(ts)
    res = dict(d=d, M=M, p=p, B=B, route=pred.route, values_ms=t["values"], present_ms=t["present"], gradient_ms=t["gradient"],
               alt_grad_ms=t["alt_grad"], ratio_present_over_values=t["present"] / t["values"],
               ratio_alt_over_gradient=t["alt_grad"] / t["gradient"], descend_ms_per_iteration=descend,
               flops_q_product=2.0 * Mp * Mp * B, tflops_values=2.0 * Mp * Mp * B / (t["values"] * 1e-3) / 1e12,
               build_ms=statistics.median(builds[1:]), build_first_ms=builds[0],
               max_rel_diff_of_the_variances=float((var_new - varn_old).abs().max() / varn_old.abs().max()),
               workspace_bytes=ops.var_workspace_bytes(M, d, p, B, 1), q_bytes=8 * Mp * Mp)
    del eng, eng2, pred
    torch.cuda.empty_cache()
    return res


def summary(res):
    lines = ["posterior-variance predictor vs ElboEngine.predict (cache hit), %s; median ms of %d alternating calls, device events"
             % (res["device"], res["reps"]),
             "%-7s %4s %4s %2s %5s %-8s %10s %10s %6s %11s %11s %6s %10s %10s %9s %9s" % (
                 "shape", "d", "M", "p", "B", "route", "present ms", "values ms", "ratio", "gradient ms", "alt grad ms", "ratio",
                 "desc64 ms", "desc512 ms", "build ms", "rel diff")]
    for name, r in res["geometries"].items():
        lines.append("%-7s %4d %4d %2d %5d %-8s %10.3f %10.3f %6.2f %11.3f %11.3f %6.2f %10.3f %10.3f %9.2f %9.1e" % (
            name, r["d"], r["M"], r["p"], r["B"], r["route"], r["present_ms"], r["values_ms"], r["ratio_present_over_values"],
            r["gradient_ms"], r["alt_grad_ms"], r["ratio_alt_over_gradient"], r["descend_ms_per_iteration"]["64"],
            r["descend_ms_per_iteration"]["512"], r["build_ms"], r["max_rel_diff_of_the_variances"]))
    lines.append("alt grad: predict + a second L^-T solve of B columns + transpose + kernel backward (what the present code offers for the")
    lines.append("gradient); desc: ms per descent iteration (mean + variance + acquisition + step) at 64 / 512 starts; build: variance_predictor(params),")
    lines.append("host clock to a device synchronise, median of 5; rel diff: max |variance(with_noise) - predict| / max |predict| at the timed size")
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
    assert torch.cuda.is_available(), "variance_probe needs the GPU"
    assert args.reps >= 20, "medians over at least 20 calls"
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, reps=args.reps, geometries={})
    for name in args.only.split(","):
        d, M, p, B = GEOMS[name]
        res["geometries"][name] = probe(dsvgp_amd, dev, d, M, p, B, args.warmup, args.reps)
        print(json.dumps({name: res["geometries"][name]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    text = summary(res)
    if args.summary:
        with open(args.summary, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
