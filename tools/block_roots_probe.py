#!/usr/bin/env python3
"""Per-point covariance roots (csrc/block_roots.hip) against what a user of the parent commit has to do with the [B, q, q] blocks, one
process, per shape (B, q) = (4096, 6), (4096, 21), (65536, 4), (4096, 96), n = 64 draws:

    factor   _ops.blocks_factor(blocks)                       | torch.linalg.cholesky(blocks.double())  (+ 2 sum log diag)
    logpdf   _ops.blocks_logpdf(roots, logdet, mu, y)         | torch.linalg.solve_triangular(L, y - mu) in float64,
                                                                -|z|^2 / 2 - logdet / 2 - q log(2 pi) / 2
    draw     _ops.blocks_draw(roots, mu, eps)  [64, B q]      | mu + batched matmul L eps in float64, cast to float32

Blocks: R R^T + (q / 50) I, R standard normal (the blocks of tests/test_gpu_block_roots.py).  Times: one pair of device events around
every call, the median over `--reps` (>= 20) ALTERNATING calls (ours, torch, ours, ...) after `--warmup` (5) calls of each
(tools/mean_predict_probe.py: medians).  No speed bound is attached to these numbers.  Prints one JSON object; --out writes it to a
file, --summary a digest (profiles/block_roots_summary.txt)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mean_predict_probe import medians  # noqa: E402

SHAPES = [(4096, 6), (4096, 21), (65536, 4), (4096, 96)]
N_DRAWS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--summary")
    args = ap.parse_args()
    import dsvgp_amd
    ops = dsvgp_amd._ops
    dev = torch.device("cuda", 0)
    ctx = ops.Context.get(dev)
    f64 = torch.float64
    result = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": max(20, args.reps), "n_draws": N_DRAWS, "shapes": {}}
    for B, q in SHAPES:
        g = torch.Generator(device=dev).manual_seed(q)
        R = torch.randn(B, q, q, dtype=f64, device=dev, generator=g)
        blocks = (R @ R.transpose(1, 2) + (q / 50.0) * torch.eye(q, dtype=f64, device=dev)).float().contiguous()
        mu = torch.randn(B * q, device=dev, generator=g)
        y = mu + torch.randn(B * q, device=dev, generator=g)
        eps = torch.randn(N_DRAWS, B * q, device=dev, generator=g)
        roots, logdet, _, status = ops.blocks_factor(ctx, blocks)
        assert int(status.item()) == 0
        L = torch.linalg.cholesky(blocks.double())
        ld = 2.0 * L.diagonal(dim1=1, dim2=2).log().sum(-1)

        def t_factor():
            Lt = torch.linalg.cholesky(blocks.double())
            return Lt, 2.0 * Lt.diagonal(dim1=1, dim2=2).log().sum(-1)

        def t_logpdf():
            z = torch.linalg.solve_triangular(L, (y.double() - mu.double()).reshape(B, q, 1), upper=False).squeeze(-1)
            return z.float(), (-0.5 * (z * z).sum(-1) - 0.5 * ld - 0.5 * q * math.log(2.0 * math.pi)).float()

        def t_draw():
            e = eps.double().reshape(N_DRAWS, B, q).permute(1, 2, 0)                       # [B, q, n]
            return (mu.double().reshape(B, q, 1) + L @ e).permute(2, 0, 1).reshape(N_DRAWS, B * q).float()

        ms = medians({"factor": lambda: ops.blocks_factor(ctx, blocks), "factor_torch": t_factor,
                      "logpdf": lambda: ops.blocks_logpdf(ctx, roots, logdet, mu, y), "logpdf_torch": t_logpdf,
                      "draw": lambda: ops.blocks_draw(ctx, roots, mu, eps), "draw_torch": t_draw}, args.warmup, max(20, args.reps))
        agree = {"roots": float((roots - L).abs().max() / L.abs().max()), "logp": float((ops.blocks_logpdf(ctx, roots, logdet, mu, y)[1] - t_logpdf()[1]).abs().max()),
                 "draw": float((ops.blocks_draw(ctx, roots, mu, eps) - t_draw()).abs().max())}
        result["shapes"]["B%d_q%d" % (B, q)] = {"ms": ms, "max_difference": agree}
    text = json.dumps(result)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.summary:
        with open(args.summary, "w") as f:
            f.write("tools/block_roots_probe.py on %s: median of %d alternating calls after %d warm-ups, device events, ms; n = %d draws\n"
                    % (result["device"], result["reps"], result["warmup"], N_DRAWS))
            f.write("%-14s %10s %10s %10s %10s %10s %10s\n" % ("shape", "factor", "torch", "logpdf", "torch", "draw", "torch"))
            for name, r in result["shapes"].items():
                m = r["ms"]
                f.write("%-14s %10.4f %10.4f %10.4f %10.4f %10.4f %10.4f\n" % (name, m["factor"], m["factor_torch"], m["logpdf"], m["logpdf_torch"],
                                                                               m["draw"], m["draw_torch"]))


if __name__ == "__main__":
    main()
