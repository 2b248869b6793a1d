#!/usr/bin/env python3
"""Training on function values only (pd = 0) two ways, ALTERNATING in one process on the same parameters and batch:

  kernel backward of K_ZX-bar [M', B]
    rect     _ops.kernel_bwd_rect on the [M', B] upstream as it is                                  (csrc/assemble_wide.hip)
    full     the upstream scattered into a zero-filled [M', B (p + 1)] matrix, then _ops.kernel_bwd  (what _kernel_bwd_zx does for the
             derivative-free engine)
  kernel forward of K_ZX [M', B]
    rect     _ops.kernel_fwd_rect                                    full     _ops.kernel_fwd [M', B (p + 1)] + the strided copy-out
  whole step (ELBO fast path, piecewise)
    rect     ElboEngine.loss_and_grads(params, x, y, None, ...)       dfree    the derivative-free engine (data_outputs = "values")

    C4 d 20 M 500 p 5 B 4096 | C2 d 5 M 200 p 2 B 512

Times: one pair of device events around every call, median over `--reps` (>= 20) calls after `--warmup` calls of each.  Derived from
the shapes by this file: the K_ZX assembly traffic each way, 4 M' B bytes against 4 M' B (p + 1), i.e. the expectation 1 / (p + 1) for
the two assembly kernels -- arithmetic, not a result.  Prints one JSON object; --out writes it to a file, --summary a text digest."""
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
GEOMS = {"C4": (20, 500, 5, 4096), "C2": (5, 200, 2, 512)}


def probe(dsvgp, dev, d, M, p, B, warmup, reps):
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    P, x, D = model(dev, d, M, p, B)
    q, Mp = p + 1, M * (p + 1)
    g = torch.Generator().manual_seed(1)
    y = torch.randn(B, generator=g).to(dev)
    hyp = ops.hyp_forward(ctx, P["raw_lengthscale"], P["raw_outputscale"], P["raw_noise"])
    Z = P["inducing_points"].contiguous()
    center = ops.column_mean(ctx, Z)
    pz = ops.pack_points(ctx, Z, P["inducing_directions"].contiguous(), p, hyp, center)
    px0 = ops.pack_points(ctx, x, None, 0, hyp, center)
    pxp = ops.pack_points(ctx, x, D, p, hyp, center)
    G = torch.randn(Mp, B, generator=g).to(dev)
    full = torch.empty(Mp, B * q, device=dev)
    K0, Kfull, Kcopy = torch.empty(Mp, B, device=dev), torch.empty(Mp, B * q, device=dev), torch.empty(Mp, B, device=dev)
    ws_r = torch.empty(ops.kernel_bwd_rect_workspace_bytes(M, p, B, 0, d), dtype=torch.uint8, device=dev)
    ws_f = torch.empty(int(dsvgp._lib.lib.dsvgp_kernel_bwd_workspace_bytes(M, B, d, p)), dtype=torch.uint8, device=dev)
    out = [(torch.zeros(M, d, device=dev), torch.zeros(M * p, d, device=dev), torch.zeros(4, device=dev)) for _ in range(2)]

    def bwd_rect():
        ops.kernel_bwd_rect(ctx, G, pz, M, p, px0, B, 0, d, hyp, *out[0], ws_r)

    def bwd_full():
        full.zero_()
        full[:, ::q] = G
        ops.kernel_bwd(ctx, full, pz, M, pxp, B, d, p, hyp, False, *out[1], ws_f)

    def fwd_full():
        ops.kernel_fwd(ctx, pz, M, pxp, B, d, p, hyp, out=Kfull)
        Kcopy.copy_(Kfull[:, ::q])

    tb = medians({"rect": bwd_rect, "full": bwd_full}, warmup, reps)
    tf = medians({"rect": lambda: ops.kernel_fwd_rect(ctx, pz, M, p, px0, B, 0, d, hyp, out=K0), "full": fwd_full}, warmup, reps)
    for o in out:
        for t in o:
            t.zero_()
    bwd_rect()
    bwd_full()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    eng, eng0 = dsvgp.ElboEngine(dev), dsvgp.ElboEngine(dev)
    eng0.data_outputs = "values"
    nd = 100.0 * B
    r1 = eng.loss_and_grads(P, x, y, None, nd)
    r0 = eng0.loss_and_grads(P, x, y, D, nd)
    ts = medians({"rect": lambda: eng.loss_and_grads(P, x, y, None, nd), "dfree": lambda: eng0.loss_and_grads(P, x, y, D, nd)}, warmup, reps)
    res = dict(d=d, M=M, p=p, B=B, kzx_bytes_rect=4 * Mp * B, kzx_bytes_full=4 * Mp * B * q, expected_assembly_ratio=1.0 / q,
               bwd_rect_ms=tb["rect"], bwd_full_ms=tb["full"], bwd_ratio=tb["rect"] / tb["full"],
               fwd_rect_ms=tf["rect"], fwd_full_ms=tf["full"], fwd_ratio=tf["rect"] / tf["full"],
               step_rect_ms=ts["rect"], step_dfree_ms=ts["dfree"], step_ratio=ts["rect"] / ts["dfree"],
               max_rel_diff_d_x1=rel(out[0][0], out[1][0]), max_rel_diff_d_v1=rel(out[0][1], out[1][1]),
               max_rel_diff_d_hyp=rel(out[0][2][:2], out[1][2][:2]), rel_diff_loss=abs(float(r1[0]) - float(r0[0])) / abs(float(r0[0])),
               max_rel_diff_step_dZ=rel(r1[1]["inducing_points"], r0[1]["inducing_points"]), rect_step_used_the_one_call_step=bool(eng.c_step_used))
    del eng, eng0
    torch.cuda.empty_cache()
    return res


def summary(res):
    lines = ["training on values only (pd = 0): rectangular kernels / step vs the derivative-free path, %s; median ms of %d alternating calls, "
             "device events" % (res["device"], res["reps"]),
             "%-4s %3s %4s %2s %5s | %9s %9s %6s | %9s %9s %6s | %9s %9s %6s | %7s" % (
                 "", "d", "M", "p", "B", "bwd rect", "bwd full", "ratio", "fwd rect", "fwd full", "ratio", "step rect", "step dfree", "ratio",
                 "1/(p+1)")]
    for name, r in res["geometries"].items():
        lines.append("%-4s %3d %4d %2d %5d | %9.4f %9.4f %6.3f | %9.4f %9.4f %6.3f | %9.3f %9.3f %6.3f | %7.3f" % (
            name, r["d"], r["M"], r["p"], r["B"], r["bwd_rect_ms"], r["bwd_full_ms"], r["bwd_ratio"], r["fwd_rect_ms"], r["fwd_full_ms"],
            r["fwd_ratio"], r["step_rect_ms"], r["step_dfree_ms"], r["step_ratio"], r["expected_assembly_ratio"]))
        lines.append("     the two ways agree to: d_x1 %.1e, d_v1 %.1e, d_hyp %.1e (kernel backward); loss %.1e, Z-bar %.1e (step)" % (
            r["max_rel_diff_d_x1"], r["max_rel_diff_d_v1"], r["max_rel_diff_d_hyp"], r["rel_diff_loss"], r["max_rel_diff_step_dZ"]))
    lines.append("bwd full: zero fill + strided scatter + dsvgp_kernel_bwd; fwd full: dsvgp_kernel_fwd + strided copy-out; step: loss_and_grads,")
    lines.append("ELBO fast path, both piecewise.  1/(p+1): the arithmetic expectation for the K_ZX assembly traffic each way, not a measurement.")
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
    assert torch.cuda.is_available(), "rect_train_probe needs the GPU"
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
