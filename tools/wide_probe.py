#!/usr/bin/env python3
"""Wide-input assembly (packed width > 96, csrc/assemble_wide.hip) on the MI355X: the K_ZX forward / backward rate at the stress geometry
W3 and the one-call step at the paper's wide geometries, next to the float64 model mode's step.

    W1   rover (experiments/rover/run_exp.py): d = 200, M(p+1) = 400 (M = 100, p = 3; and the Vanilla run M = 400, p = 0), B = 512
    W2   GCN on PubMed (experiments/GNN_bo/gcn_turbo.py): d = 4035, M = 10, p = 10, B = 256
    W3   stress geometry (not a reference configuration): d = 1024, M = 500, p = 5, B = 4096

Flop counts: forward 2 n1q n2q K4 (T = P1 P2^T over the packed width; the micro-block transform is not counted), backward twice that
(T again, then Tbar . P2).  Peak: 157.3 TF fp32 MFMA.  Times: device events around `--reps` calls after `--warmup` calls.
Prints one JSON object; --out also writes it to a file."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402

PEAK_TF = 157.3
GEOMS = {"W1": (2000, 200, 100, 3, 512), "W1v": (2000, 200, 400, 0, 512), "W2": (400, 4035, 10, 10, 256),
         "W3": (6000, 1024, 500, 5, 4096)}


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def assembly_rate(dsvgp, dev, d, M, p, B, warmup, reps):
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    q = p + 1
    g = torch.Generator(device=dev).manual_seed(0)
    ell = 0.4 * math.sqrt(d)
    hyp = torch.tensor([ell, 1.0, 0.1, 0.0], device=dev)
    Z, V = torch.rand(M, d, device=dev, generator=g), torch.randn(M * p, d, device=dev, generator=g)
    X, D = torch.rand(B, d, device=dev, generator=g), torch.randn(B * p, d, device=dev, generator=g)
    center = ops.column_mean(ctx, Z)
    pz, px = ops.pack_points(ctx, Z, V, p, hyp, center), ops.pack_points(ctx, X, D, p, hyp, center)
    n1q, n2q, K4 = M * q, B * q, (d + 3) // 4 * 4
    out = torch.empty(n1q, n2q, device=dev)
    t_fwd = timed(lambda: ops.kernel_fwd(ctx, pz, M, px, B, d, p, hyp, out=out), warmup, reps)
    G = torch.randn(n1q, n2q, device=dev, generator=g)
    dx, dv, dh = torch.zeros(M, d, device=dev), torch.zeros(max(M * p, 1), d, device=dev), torch.zeros(4, device=dev)
    ws = ops.kernel_bwd(ctx, G, pz, M, px, B, d, p, hyp, False, dx, dv, dh)
    t_bwd = timed(lambda: ops.kernel_bwd(ctx, G, pz, M, px, B, d, p, hyp, False, dx, dv, dh, workspace=ws), warmup, reps)
    f_fwd = 2.0 * n1q * n2q * K4
    res = dict(n1q=n1q, n2q=n2q, K4=K4, fwd_ms=t_fwd, fwd_tflops=f_fwd / t_fwd / 1e9, fwd_frac_of_peak=f_fwd / t_fwd / 1e9 / PEAK_TF,
               bwd_ms=t_bwd, bwd_tflops=2 * f_fwd / t_bwd / 1e9, bwd_frac_of_peak=2 * f_fwd / t_bwd / 1e9 / PEAK_TF,
               bwd_workspace_mb=ws.numel() / 2 ** 20, note="bwd_ms includes the points launch (slab sums -> d_x1, d_v1, d_hyp)")
    del out, G, ws
    torch.cuda.empty_cache()
    return res


def step_time(dsvgp, dev, N, d, M, p, B, fp64, warmup, reps):
    from test_gpu_step import make_problem
    P, x, y, D, nd = make_problem(N, d, M, p, B, seed=1)
    P["raw_lengthscale"] = torch.tensor([[math.log(math.expm1(0.4 * math.sqrt(d)))]])
    dt = torch.float64 if fp64 else torch.float32
    if fp64:
        from dsvgp_amd._step64 import ElboEngine64
        eng = ElboEngine64(dev)
    else:
        eng = dsvgp.ElboEngine(dev)
    Pg = {k: v.to(dev, dt) for k, v in P.items()}
    xd, yd, Dd = x.to(dev, dt), y.to(dev, dt), D.to(dev, dt)
    try:
        ms = timed(lambda: eng.loss_and_grads(Pg, xd, yd, Dd, nd), warmup, reps)
    except Exception as e:     # (reported, not hidden: the float64 mode may not take a geometry)
        return dict(error="%s: %s" % (type(e).__name__, e))
    res = dict(ms_per_step=ms)
    if not fp64:
        res["one_call"] = bool(getattr(eng, "c_step_used", False))
    del eng
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="rate,steps", help="rate: K_ZX at W3; steps: the step at W1 / W1v / W2 / W3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dsvgp_amd
    assert torch.cuda.is_available(), "wide_probe needs the GPU"
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), peak_fp32_mfma_tf=PEAK_TF, geometries={k: dict(zip("N d M p B".split(), v))
                                                                                              for k, v in GEOMS.items()})
    if "rate" in args.only:
        N, d, M, p, B = GEOMS["W3"]
        res["W3_assembly"] = assembly_rate(dsvgp_amd, dev, d, M, p, B, args.warmup, args.reps)
        print(json.dumps({"W3_assembly": res["W3_assembly"]}), flush=True)
    if "steps" in args.only:
        res["steps"] = {}
        for name, (N, d, M, p, B) in GEOMS.items():
            r = dict(fp32=step_time(dsvgp_amd, dev, N, d, M, p, B, False, args.warmup, args.reps),
                     fp64_model_mode=step_time(dsvgp_amd, dev, N, d, M, p, B, True, args.warmup, args.reps))
            res["steps"][name] = r
            print(json.dumps({name: r}), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
