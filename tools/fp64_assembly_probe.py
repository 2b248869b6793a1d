#!/usr/bin/env python3
"""The float64 kernel assembly by itself on the MI355X: K_ZX forward and backward on the register path (csrc/assemble64.hip: fp64 GEMM,
in-place transform, GEMM, points -- p <= 16 only) and on the tiled path (csrc/assemble64_tiled.hip, any p <= 95), ALTERNATING in one
process on the same packs.

    C4 d 20 M 500 p 5 B 4096 | C2 d 5 M 200 p 2 B 512 | C3 d 10 M 300 p 10 B 512 | C5 d 50 M 1024 p 5 B 512       both paths
    welch d = p = 20 M 100 B 512 | stellarator d = p = 45 M 50 B 256 | q96 d = p = 95 M 20 B 128 | rover_wide d 200 p 30 M 100 B 512
                                                                                                                   tiled path only

Times: one pair of device events around every call, median over `--reps` (>= 20) calls after `--warmup` calls.
Derived from the shapes, by this file: the bytes the algorithm needs (forward: 8 per output entry + the packs; backward: 8 per
upstream entry + the packs) over the time as a share of the 8 TB/s HBM roof, the MFMA flops (forward 2 n1q n2q K4; backward that again
+ 2 n1q n2q DP for Tbar [P2 | indicator]) over the time as a share of the 78.6 TF fp64 MFMA peak, and which of the two bounds is the
longer one for the shape.  Prints one JSON object; --out writes it to a file, --summary a ten-line text digest.

--deterministic adds the tiled backward under ``dsvgp_set_deterministic`` to the alternation, in both forms the launcher has: one dP1
slab per sweep group added in sweep order (a scratch of ``dsvgp_deterministic_f64_scratch_bytes``), and one workgroup owning a tile row
over the whole column range (what a scratch too small for two slabs selects)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_TBS = 8.0
PEAK_FP64_TF = 78.6
f64 = torch.float64
# name: (d, M, p, B, both paths)
GEOMS = {"C4": (20, 500, 5, 4096, True), "C2": (5, 200, 2, 512, True), "C3": (10, 300, 10, 512, True), "C5": (50, 1024, 5, 512, True),
         "welch": (20, 100, 20, 512, False), "stellarator": (45, 50, 45, 256, False), "q96": (95, 20, 95, 128, False),
         "rover_wide": (200, 100, 30, 512, False)}


def medians(fns, warmup, reps):
    """fns: name -> callable; called in turn (a, b, a, b, ...), every call between its own pair of events"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}


def shares(ms, nbytes, flops):
    t = ms * 1e-3
    t_hbm, t_mfma = nbytes / (HBM_TBS * 1e12), flops / (PEAK_FP64_TF * 1e12)
    return dict(ms=ms, gb_per_s=nbytes / t / 1e9, share_of_hbm_roof=t_hbm / t, tflops=flops / t / 1e12, share_of_mfma_peak=t_mfma / t,
                bound="hbm" if t_hbm >= t_mfma else "mfma", share_of_bound=max(t_hbm, t_mfma) / t)


def probe(dsvgp, dev, d, M, p, B, both, warmup, reps, deterministic=False):
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    q = p + 1
    g = torch.Generator(device=dev).manual_seed(0)
    hyp = torch.tensor([0.4 * d ** 0.5, 1.0, 0.1, 0.0], dtype=f64, device=dev)
    Z, V = torch.rand(M, d, dtype=f64, device=dev, generator=g), torch.randn(M * p, d, dtype=f64, device=dev, generator=g)
    X, D = torch.rand(B, d, dtype=f64, device=dev, generator=g), torch.randn(B * p, d, dtype=f64, device=dev, generator=g)
    center = Z.mean(0).contiguous()
    pz, px = ops.pack_points_f64(ctx, Z, V, p, hyp, center), ops.pack_points_f64(ctx, X, D, p, hyp, center)
    n1q, n2q, K4 = M * q, B * q, (d + 3) // 4 * 4
    DP = K4 + 4
    pack_bytes = 8 * (n1q + n2q) * (DP + 1)
    nbytes = 8 * n1q * n2q + pack_bytes
    f_fwd, f_bwd = 2.0 * n1q * n2q * K4, 2.0 * n1q * n2q * K4 + 2.0 * n1q * n2q * DP
    out_t, out_o = torch.empty(n1q, n2q, dtype=f64, device=dev), None
    G = torch.randn(n1q, n2q, dtype=f64, device=dev, generator=g)
    dx, dv, dh = (torch.zeros(M, d, dtype=f64, device=dev), torch.zeros(max(M * p, 1), d, dtype=f64, device=dev),
                  torch.zeros(4, dtype=f64, device=dev))
    ws = ops.kernel_bwd_f64_tiled(ctx, G, pz, M, px, B, d, p, hyp, False, dx, dv, dh)
    fwd = {"tiled": lambda: ops.kernel_fwd_f64_tiled(ctx, pz, M, px, B, d, p, hyp, out=out_t)}
    bwd = {"tiled": lambda: ops.kernel_bwd_f64_tiled(ctx, G, pz, M, px, B, d, p, hyp, False, dx, dv, dh, workspace=ws)}
    if both:
        assert p <= ops.F64_REGISTER_P          # kernel_fwd_f64 / kernel_bwd_f64 are the register path there
        out_o, scratch = torch.empty(n1q, n2q, dtype=f64, device=dev), torch.empty(n1q, n2q, dtype=f64, device=dev)
        fwd["register"] = lambda: ops.kernel_fwd_f64(ctx, pz, M, px, B, d, p, hyp, out=out_o)
        bwd["register"] = lambda: ops.kernel_bwd_f64(ctx, G, pz, M, px, B, d, p, hyp, False, dx, dv, dh, scratch)
    if deterministic:
        full = torch.empty(int(dsvgp._lib.lib.dsvgp_deterministic_f64_scratch_bytes(M, d, p, B)), dtype=torch.uint8, device=dev)
        one_slab = torch.empty(8 * n1q * DP, dtype=torch.uint8, device=dev)        # < two slabs: one sweep group per tile row

        def under(scratch):
            def run():
                ctx.set_deterministic(scratch)
                try:
                    ops.kernel_bwd_f64_tiled(ctx, G, pz, M, px, B, d, p, hyp, False, dx, dv, dh, workspace=ws)
                finally:
                    ctx.set_deterministic(None)
            return run
        bwd["tiled_det_slabs"], bwd["tiled_det_owner"] = under(full), under(one_slab)
    tf, tb = medians(fwd, warmup, reps), medians(bwd, warmup, reps)
    res = dict(d=d, M=M, p=p, B=B, n1q=n1q, n2q=n2q, K4=K4, out_mb=8 * n1q * n2q / 1e6, needed_bytes=nbytes,
               fwd_flops=f_fwd, bwd_flops=f_bwd, fwd={k: shares(v, nbytes, f_fwd) for k, v in tf.items()},
               bwd={k: shares(v, nbytes, f_bwd) for k, v in tb.items()})
    if both:
        res["fwd_max_rel_diff"] = float((out_t - out_o).abs().max() / out_o.abs().max())
        res["fwd_tiled_over_register"] = tf["tiled"] / tf["register"]
        res["bwd_tiled_over_register"] = tb["tiled"] / tb["register"]
    else:
        res["register_path"] = "not measured: it does not take p > 16"
    del out_t, out_o, G, ws
    torch.cuda.empty_cache()
    return res


def summary(res):
    lines = ["fp64 kernel assembly, K_ZX, median ms of %d calls (register path | tiled path), share of the longer bound in brackets"
             % res["reps"]]
    for name, r in res["geometries"].items():
        def cell(part, path):
            c = r[part].get(path)
            return "%8.3f [%.2f %s]" % (c["ms"], c["share_of_bound"], c["bound"]) if c else "   not taken    "
        lines.append("%-12s d %3d p %2d M %4d B %4d  fwd %s | %s   bwd %s | %s" % (
            name, r["d"], r["p"], r["M"], r["B"], cell("fwd", "register"), cell("fwd", "tiled"), cell("bwd", "register"), cell("bwd", "tiled")))
    for name, r in res["geometries"].items():
        if "tiled_det_slabs" in r["bwd"]:
            lines.append("%-12s bwd tiled, ms: atomics %.3f | deterministic, slab per sweep group %.3f | deterministic, one workgroup per tile row %.3f"
                         % (name, r["bwd"]["tiled"]["ms"], r["bwd"]["tiled_det_slabs"]["ms"], r["bwd"]["tiled_det_owner"]["ms"]))
    lines.append("bounds: bytes needed / 8 TB/s HBM, MFMA flops / 78.6 TF fp64; backward times include the memset of dP1 and the points launch")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=",".join(GEOMS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--summary", default=None)
    ap.add_argument("--deterministic", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dsvgp_amd
    assert torch.cuda.is_available(), "fp64_assembly_probe needs the GPU"
    assert args.reps >= 20, "medians over at least 20 calls"
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), hbm_roof_tb_s=HBM_TBS, fp64_mfma_peak_tf=PEAK_FP64_TF, warmup=args.warmup,
               reps=args.reps, geometries={})
    for name in args.only.split(","):
        d, M, p, B, both = GEOMS[name]
        res["geometries"][name] = probe(dsvgp_amd, dev, d, M, p, B, both, args.warmup, args.reps, args.deterministic)
        print(json.dumps({name: res["geometries"][name]}), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.summary:
        with open(args.summary, "w") as f:
            f.write(summary(res))


if __name__ == "__main__":
    main()
