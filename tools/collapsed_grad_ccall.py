#!/usr/bin/env python3
"""dsvgp_collapsed_grad_chunk alone at the config-4 chunk shape (M' = 3000, B' = 24576) on synthetic operands: the C call between device
events (median of --reps after two warm-up calls).  Run it under the kernel tracer to get the durations of the four launches inside the
call -- the residual's reduce and combine, the Q K_ZX product, the epilogue -- beside the call's own time:

  rocprofv3 --kernel-trace --stats -d OUT -- python3 tools/collapsed_grad_ccall.py
  python3 tools/collapsed_grad_ccall.py --summarise OUT          # per-kernel mean of the traced calls, their sum, and the event time

GPU box tool; nothing here is imported by the package.  The timings do not depend on the values (no data-dependent path)."""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(args):
    import torch
    from dsvgp_amd import _ops
    dev = torch.device("cuda", 0)
    Mp, Bp = args.mp, args.bp
    g = torch.Generator(device=dev).manual_seed(0)
    f64 = torch.float64
    ldq = (Mp + 1) & ~1
    Q = torch.randn(Mp, ldq, dtype=f64, device=dev, generator=g)[:, :Mp]
    alpha = torch.randn(Mp, dtype=f64, device=dev, generator=g)
    adj = torch.tensor([1e-3, 0.0, 1e-3, 0.0, 0.0, 0.0, 1.0, float(Bp)], dtype=f64, device=dev)
    Kzx, Kbar = torch.randn(Mp, Bp, device=dev, generator=g), torch.empty(Mp, Bp, device=dev)
    y, c = torch.randn(Bp, device=dev, generator=g), torch.zeros(1, device=dev)
    rho_sum = torch.zeros(1, dtype=f64, device=dev)
    ws = torch.empty(_ops.collapsed_grad_chunk_bytes(Mp, Bp) // 8, dtype=f64, device=dev)
    ctx = _ops.Context.get(dev)
    call = lambda: _ops.collapsed_grad_chunk(ctx, Mp, Kzx, y, c, Q, alpha, adj, Kbar, None, rho_sum, ws)
    for _ in range(2):
        call()
    out = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    print("ccall M' = %d, B' = %d: median %.3f ms (min %.3f, max %.3f) over %d calls between device events"
          % (Mp, Bp, statistics.median(out), min(out), max(out), args.reps), flush=True)


def summarise(directory):
    """per kernel of the call: launches, median / min / max duration without the two warm-up calls; their sum; and the span of a call
    from the first launch's start to the last launch's end.  Reads the tracer's database (``kernels`` view) or its kernel trace CSV"""
    rows = []                                                    # (name, start ns, end ns)
    for f in glob.glob(os.path.join(directory, "**", "*.db"), recursive=True):
        import sqlite3
        rows += sqlite3.connect(f).execute("select name, start, end from kernels order by start").fetchall()
    if not rows:
        for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                rows.append((row.get("Kernel_Name") or row.get("Name"), float(row["Start_Timestamp"]), float(row["End_Timestamp"])))
        rows.sort(key=lambda r: r[1])
    if not rows:
        raise SystemExit("no tracer database and no *kernel_trace.csv under " + directory)
    short = lambda n: n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
    first = next(i for i, r in enumerate(rows) if "cgrad_reduce" in r[0])
    rows = [(short(n), s, e) for n, s, e in rows[first:]]        # (what precedes the first call sets the operands up)
    per, order = {}, []
    for n, s, e in rows:
        if n not in per:
            order.append(n)
        per.setdefault(n, []).append((s, e))
    total = 0.0
    for n in order:
        d = [(e - s) * 1e-6 for s, e in per[n]][2:]
        print("%-40s launches %3d  median %.4f ms (min %.4f, max %.4f)" % (n[:40], len(per[n]), statistics.median(d), min(d), max(d)))
        total += statistics.median(d)
    spans = [(e - s) * 1e-6 for (s, _), (_, e) in zip(per[order[0]], per[order[-1]])][2:]
    print("sum of the launches inside one call: %.3f ms; span first start -> last end: median %.3f ms (min %.3f, max %.3f)"
          % (total, statistics.median(spans), min(spans), max(spans)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mp", type=int, default=3000)
    ap.add_argument("--bp", type=int, default=24576)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--summarise", default=None)
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise)
    else:
        run(args)


if __name__ == "__main__":
    main()
