#!/usr/bin/env python3
"""Predictions of the function values only (pd = 0, K_ZX from csrc/assemble_wide.hip) against predictions with the model's own
direction count (pd = p), ALTERNATING in one process on the same model (one engine per path), on a hit of the evaluation cache:

    full     ElboEngine.predict(params, x, D_p, cache=True)     B (p + 1) columns: assembly, fp64 solve, W = L_S^T A, statistics
    values   ElboEngine.predict(params, x, None, cache=True)    B columns

    C4eval d 20 M 500 p 5 B 4096 | BOblock d 200 M 512 p 2 B 2048

and, at B = 1024 of both shapes, ``predict_joint`` followed by ``covariance_root`` (what one joint sample pays before its draw).

Times: one pair of device events around every call, median over `--reps` (>= 20) calls after `--warmup` calls of each.  Derived from
the shapes by this file: the columns each path carries and the arithmetic expectation of their ratio (1 / (p + 1) for the solve and
W, 1 / (p + 1)^3 for the root) -- an expectation, not a result.  The value rows of the two paths are compared at the timed size.
Prints one JSON object; --out writes it to a file, --summary a text digest."""
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
GEOMS = {"C4eval": (20, 500, 5, 4096), "BOblock": (200, 512, 2, 2048)}
JOINT_B = 1024


def probe(dsvgp, dev, d, M, p, B, warmup, reps):
    P, x, D = model(dev, d, M, p, B)
    # one engine per path: an engine keeps its K_ZX / A / W buffers while their shape repeats, as a caller that stays with one pd
    # sees it; alternating the two shapes on ONE engine would re-allocate them in every call
    eng, eng0 = dsvgp.ElboEngine(dev), dsvgp.ElboEngine(dev)
    mu_full, var_full = eng.predict(P, x, D, cache=True)
    mu_val, var_val = eng0.predict(P, x, None, cache=True)
    t = medians({"full": lambda: eng.predict(P, x, D, cache=True), "values": lambda: eng0.predict(P, x, None, cache=True)}, warmup, reps)
    xj, Dj = x[:JOINT_B].contiguous(), D[:JOINT_B * p].contiguous()

    def joint(e, Dq):
        mu, Sigma = e.predict_joint(P, xj, Dq, cache=True)
        return e.covariance_root(Sigma)

    tj = medians({"full": lambda: joint(eng, Dj), "values": lambda: joint(eng0, None)}, max(2, warmup // 2), reps)
    q = p + 1
    res = dict(d=d, M=M, p=p, B=B, columns_full=B * q, columns_values=B, predict_full_ms=t["full"], predict_values_ms=t["values"],
               predict_ratio_values_over_full=t["values"] / t["full"], expected_solve_and_W_ratio=1.0 / q,
               joint_B=JOINT_B, joint_root_full_ms=tj["full"], joint_root_values_ms=tj["values"],
               joint_root_ratio_values_over_full=tj["values"] / tj["full"], expected_root_ratio=1.0 / q ** 3,
               max_rel_diff_of_the_value_means=float((mu_val - mu_full[::q]).abs().max() / mu_full.abs().max()),
               max_rel_diff_of_the_value_variances=float((var_val - var_full[::q]).abs().max() / var_full[::q].abs().max()))
    del eng, eng0
    torch.cuda.empty_cache()
    return res


def summary(res):
    lines = ["predict at pd = 0 (values) vs pd = p (full), evaluation-cache hit, %s; median ms of %d alternating calls, device events"
             % (res["device"], res["reps"]),
             "%-8s %4s %4s %2s %5s %9s %10s %7s %9s | %6s %13s %15s %7s %9s %9s %9s" % (
                 "shape", "d", "M", "p", "B", "full ms", "values ms", "ratio", "1/(p+1)", "B", "joint full ms", "joint values ms", "ratio",
                 "1/(p+1)^3", "d mean", "d var")]
    for name, r in res["geometries"].items():
        lines.append("%-8s %4d %4d %2d %5d %9.3f %10.3f %7.3f %9.3f | %6d %13.3f %15.3f %7.3f %9.4f %9.1e %9.1e" % (
            name, r["d"], r["M"], r["p"], r["B"], r["predict_full_ms"], r["predict_values_ms"], r["predict_ratio_values_over_full"],
            r["expected_solve_and_W_ratio"], r["joint_B"], r["joint_root_full_ms"], r["joint_root_values_ms"],
            r["joint_root_ratio_values_over_full"], r["expected_root_ratio"], r["max_rel_diff_of_the_value_means"],
            r["max_rel_diff_of_the_value_variances"]))
    lines.append("joint: predict_joint + covariance_root at B = %d; 1/(p+1), 1/(p+1)^3: the arithmetic expectation for the solve / W and" % JOINT_B)
    lines.append("for the root alone, not a measurement; d mean / d var: max relative difference of the value rows of the two paths")
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
    assert torch.cuda.is_available(), "rect_predict_probe needs the GPU"
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
