#!/usr/bin/env python3
"""Per-point predictive covariance blocks (csrc/predict_blocks.hip), one process, per shape:

    launches   dsvgp_predictive_blocks alone, on the A and W that predict_blocks left in the engine's buffers
    blocks     ElboEngine.predict_blocks(params, x, D, cache=True)   K_ZX, fp64 solve, W, statistics + the blocks
    predict    ElboEngine.predict(params, x, D, cache=True)          the same without the blocks: what they add to a variance call
    joint      ElboEngine.predict_joint(params, x, D, cache=True)    where B'^2 floats fit (<= 2^15 outputs): K_XX + two Gram products

    C4eval d 20 M 500 p 5 B 4096 at pd = 0, 5, 20 (pd = 20: 86 016 outputs, the joint is not formed) | C2 d 5 M 200 p 2 B 512 pd 5 |
    rover_wide d 200 M 512 p 3 B 2048 at pd = 0, 3

Times: one pair of device events around every call, median over `--reps` (>= 20) ALTERNATING calls after `--warmup` calls of each, on
a hit of the evaluation cache, one engine per path (tools/rect_predict_probe.py).  Derived from the shapes by this file: the bytes the
two launches move, the flops the MFMA instructions issue (every live 16 x 16 tile pair, dead elements included) and the flops the
lower parts of the blocks need, and from them the least time the hardware could take -- the larger of bytes / 8 TB/s and issued
flops / 157.3 TF -- and which of the two bounds the shape.  Prints one JSON object; --out writes it to a file, --summary a digest."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mean_predict_probe import medians, model  # noqa: E402

# name: (d, M, p, B, pd)
GEOMS = {"C4eval_pd0": (20, 500, 5, 4096, 0), "C4eval_pd5": (20, 500, 5, 4096, 5), "C4eval_pd20": (20, 500, 5, 4096, 20),
         "C2_pd5": (5, 200, 2, 512, 5), "rover_wide_pd0": (200, 512, 3, 2048, 0), "rover_wide_pd3": (200, 512, 3, 2048, 3)}
JOINT_MAX_OUTPUTS = 1 << 15
HBM_BYTES_PER_S, FP32_FLOPS_PER_S = 8.0e12, 157.3e12


def plan(Mp, B, pd):
    """csrc/pred_blocks_plan.h in Python: strip, tiles, live tile pairs, groups, slices"""
    q = pd + 1
    G = 96 // q
    Tc = G * q
    ntile = (Tc + 15) // 16
    pairs = sum(1 for ti in range(ntile) for tj in range(ti + 1) if ti == tj or (tj * 16 + 15) // q == (ti * 16) // q)
    ngroups = (B + G - 1) // G
    ns = max(1, min((1024 + ngroups - 1) // ngroups, (Mp + 127) // 128, 32))
    rps = ((Mp + ns - 1) // ns + 31) // 32 * 32
    return dict(q=q, G=G, Tc=Tc, pairs=pairs, ngroups=ngroups, rps=rps, nslices=(Mp + rps - 1) // rps)


def work(Mp, B, pd, d):
    """bytes and flops of the two launches from the shapes alone"""
    w = plan(Mp, B, pd)
    q, ns = w["q"], w["nslices"]
    DP = ((d + 3) & ~3) + 4
    chunks = sum((min(w["rps"], Mp - s * w["rps"]) + 31) // 32 for s in range(ns))          # 32-row chunks over all slices of a group
    gram_bytes = 8 * Mp * B * q + 4 * ns * B * q * (q + 1) // 2
    finish_bytes = 4 * ns * B * q * q + 4 * B * q * q + (4 * B * pd * DP if pd >= 2 else 0)
    issued = w["ngroups"] * chunks * w["pairs"] * 2 * 8 * (16 * 16 * 4 * 2)                  # W and A term, 8 k-steps of 4 per chunk
    needed = 2 * 2 * Mp * B * q * (q + 1) // 2 + 2 * d * B * pd * (pd - 1) // 2
    t_bytes, t_flops = (gram_bytes + finish_bytes) / HBM_BYTES_PER_S, issued / FP32_FLOPS_PER_S
    w.update(bytes=gram_bytes + finish_bytes, issued_flops=issued, needed_flops=needed, least_ms=1e3 * max(t_bytes, t_flops),
             bound="HBM" if t_bytes >= t_flops else "MFMA issue")
    return w


def probe(dsvgp, dev, d, M, p, B, pd, warmup, reps):
    ops = dsvgp._ops
    P, x, _ = model(dev, d, M, p, B)
    D = torch.randn(B * pd, d, generator=torch.Generator().manual_seed(5)).to(dev) if pd else None
    Mp, q = M * (p + 1), pd + 1
    res = dict(d=d, M=M, p=p, B=B, pd=pd, outputs=B * q, **work(Mp, B, pd, d))
    eng_b, eng_p = dsvgp.ElboEngine(dev), dsvgp.ElboEngine(dev)
    mu, blocks = eng_b.predict_blocks(P, x, D, cache=True)
    _, varn = eng_p.predict(P, x, D, cache=True)
    res["max_rel_diff_of_the_diagonals_and_predict"] = float((blocks.diagonal(dim1=1, dim2=2).reshape(-1) - varn).abs().max() / varn.abs().max())
    fns = {"blocks": lambda: eng_b.predict_blocks(P, x, D, cache=True), "predict": lambda: eng_p.predict(P, x, D, cache=True)}
    joint = B * q <= JOINT_MAX_OUTPUTS
    if joint:
        eng_j = dsvgp.ElboEngine(dev)
        _, Sigma = eng_j.predict_joint(P, x, D, cache=True)
        i = torch.arange(B, device=dev)
        res["max_rel_diff_of_the_blocks_and_the_joint"] = float((blocks - Sigma.reshape(B, q, B, q)[i, :, i, :]).abs().max() / blocks.abs().max())
        del Sigma
        fns["joint"] = lambda: eng_j.predict_joint(P, x, D, cache=True)
    # the launches alone, on the operands the engine holds
    ctx = ops.Context.get(dev)
    hyp = ops.hyp_forward(ctx, P["raw_lengthscale"], P["raw_outputscale"], P["raw_noise"])
    px = ops.pack_points(ctx, x, D, pd, hyp, eng_b.center) if pd else None
    A32, W = eng_b._buf["A32"], eng_b._buf["W"]
    out = torch.empty(B, q, q, device=dev)
    fns["launches"] = lambda: ops.predictive_blocks(ctx, A32, W, pd, px, d, hyp, True, out=out)
    t = medians(fns, warmup, reps)
    res["bitwise_equal_to_the_engine_call"] = bool(torch.equal(out, blocks))
    res.update(launches_ms=t["launches"], blocks_ms=t["blocks"], predict_ms=t["predict"], added_ms=t["blocks"] - t["predict"],
               joint_ms=t.get("joint"), share_of_least=res["least_ms"] / t["launches"])
    del eng_b, eng_p, fns
    torch.cuda.empty_cache()
    return res


def summary(res):
    lines = ["per-point covariance blocks, evaluation-cache hit, %s; median ms of %d alternating calls, device events" % (res["device"], res["reps"]),
             "%-15s %4s %4s %2s %5s %3s %6s %2s %4s %3s | %8s %8s %6s %-10s | %9s %10s %8s %9s" % (
                 "shape", "d", "M", "p", "B", "pd", "groups", "sl", "rows", "prs", "launches", "least ms", "share", "bound", "blocks ms",
                 "predict ms", "added ms", "joint ms")]
    for name, r in res["geometries"].items():
        lines.append("%-15s %4d %4d %2d %5d %3d %6d %2d %4d %3d | %8.3f %8.3f %6.2f %-10s | %9.3f %10.3f %8.3f %9s" % (
            name, r["d"], r["M"], r["p"], r["B"], r["pd"], r["ngroups"], r["nslices"], r["rps"], r["pairs"], r["launches_ms"], r["least_ms"],
            r["share_of_least"], r["bound"], r["blocks_ms"], r["predict_ms"], r["added_ms"],
            "%.3f" % r["joint_ms"] if r["joint_ms"] is not None else "not formed"))
    lines += ["launches: dsvgp_predictive_blocks alone (Gram launch + finish launch); least ms: the larger of bytes / 8 TB/s and issued MFMA",
              "flops / 157.3 TF, both from the shapes (tools/blocks_probe.py: work); share = least / launches; bound: which of the two is larger;",
              "sl / rows: row slices and rows per slice; prs: live 16 x 16 tile pairs per strip (of 21); blocks / predict / joint: the engine calls;",
              "added = blocks - predict, what the blocks add to a variance call.  The joint is not formed above %d outputs." % JOINT_MAX_OUTPUTS]
    for name, r in res["geometries"].items():
        lines.append("%-15s bytes %.3e  issued flops %.3e  needed flops %.3e  diagonals vs predict %.1e%s  launches == engine call bitwise: %s" % (
            name, r["bytes"], r["issued_flops"], r["needed_flops"], r["max_rel_diff_of_the_diagonals_and_predict"],
            "  blocks vs joint %.1e" % r["max_rel_diff_of_the_blocks_and_the_joint"] if "max_rel_diff_of_the_blocks_and_the_joint" in r else "",
            r["bitwise_equal_to_the_engine_call"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=",".join(GEOMS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--summary", default=os.path.join(ROOT, "profiles", "pred_blocks_summary.txt"))
    ap.add_argument("--dry", action="store_true", help="print the work derived from the shapes and stop (no GPU)")
    args = ap.parse_args()
    if args.dry:
        for name in args.only.split(","):
            d, M, p, B, pd = GEOMS[name]
            print(name, json.dumps(work(M * (p + 1), B, pd, d)))
        return
    import dsvgp_amd
    assert torch.cuda.is_available(), "blocks_probe needs the GPU"
    assert args.reps >= 20, "medians over at least 20 calls"
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, reps=args.reps, geometries={})
    for name in args.only.split(","):
        d, M, p, B, pd = GEOMS[name]
        res["geometries"][name] = probe(dsvgp_amd, dev, d, M, p, B, pd, args.warmup, args.reps)
        print(json.dumps({name: res["geometries"][name]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    with open(args.summary, "w") as f:
        f.write(summary(res))
    print(summary(res))


if __name__ == "__main__":
    main()
