#!/usr/bin/env python3
"""Bitwise A/B of every entry that runs the tiled assembly kernels (csrc/tiled_assembly.h: the forward and Tbar tiles of the RBF and the
Matern-5/2 family, the contraction, the prior diagonals) between two builds of the library.

    DSVGP_LIB_PATH=<build A>/libdsvgp_hip.so python tools/tiled_ab.py --dump a.pt
    DSVGP_LIB_PATH=<build B>/libdsvgp_hip.so python tools/tiled_ab.py --dump b.pt        (a fresh process per library)
    python tools/tiled_ab.py --compare a.pt b.pt                                         (no GPU; exit status 1 if any output differs)

--dump runs the entries below on seeded inputs and saves every output tensor; --compare reports, per entry and shape, whether the bytes
are equal.  No kernel here uses floating-point atomics, so two builds that compute the same thing agree bit for bit.

Entries: kernel_fwd_rect, kernel_fwd_wide, kernel_fwd / kernel_bwd at d >= 93 (they take the tiled kernels there), kernel_bwd_rect and
kernel_bwd_wide (G float and double), kernel_bwd_ard (symmetric and not, with and without d_ell), kernel_fwd_matern52 (float and double out,
with and without jitter), kernel_bwd_matern52 (G float and double), the four diag entries.  The RBF entries run on plain packs with a
lengthscale of 0.7 (1 / ell is not 1), the ARD and Matern entries on ARD packs.

Shapes (n1, p1, n2, p2, d): the smallest at which each shared part of the kernels can go wrong -- ragged tiles, a split contraction,
p1 = 0 and p2 = 0, 1 x 1 micro-blocks with several column tiles, duplicate points (nn == 0 off the diagonal: the Matern f3 guard), q1 = 96
(Rr = 1) with the backward's column cap at q1 >= 52, the cap at q1 <= 4 (Rc = 69 at 1 x 1), seven K chunks with K4 no multiple of 32, the
wide K_ZZ, one point.

--narrow --dump runs a second entry list instead: dsvgp_kernel_fwd / _bwd on the pair and split kernels and dsvgp_kernel_fwd_canon /
_bwd_canon (csrc/wave_tile.h) at every K depth of the T' product, on ragged, full and single tiles, float and double outputs and
upstreams, 16-byte aligned rows and rows that are not, K_ZZ with jitter and the symmetric backward (NARROW_DP, NARROW_TILES below)."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

S, ELL, JITTER = 1.3, 0.7, 1e-3
#         n1  p1   n2  p2    d
SHAPES = [(37, 2, 41, 3, 5), (37, 2, 130, 3, 5), (20, 5, 45, 5, 20), (11, 2, 23, 1, 200), (9, 0, 30, 2, 7), (12, 3, 30, 0, 6),
          (24, 2, 24, 2, 5), (33, 0, 300, 0, 5), (5, 95, 7, 0, 3), (150, 1, 150, 0, 4), (150, 0, 150, 0, 4), (50, 2, 50, 2, 100),
          (1, 0, 1, 0, 1)]
DUP = (37, 2, 41, 3, 5)         # run a second time with rows of x2 copied from x1


def inputs(shape, duplicates):
    n1, p1, n2, p2, d = shape
    g = torch.Generator().manual_seed(n1 + 31 * n2 + 7 * p1 + 3 * p2 + d + (1000 if duplicates else 0))
    x1, v1 = torch.rand(n1, d, generator=g), torch.randn(n1 * p1, d, generator=g)
    x2, v2 = torch.rand(n2, d, generator=g), torch.randn(n2 * p2, d, generator=g)
    if duplicates:
        x2[[3, 17, 40]] = x1[[5, 0, 36]]
    G = torch.randn(n1 * (p1 + 1), n2 * (p2 + 1), generator=g, dtype=torch.float64)
    ell = 0.4 * math.sqrt(d) * (0.5 + torch.arange(d, dtype=torch.float32) / max(d - 1, 1))
    return x1, v1, x2, v2, G, ell


def run_shape(ops, ctx, dev, shape, duplicates, res):
    n1, p1, n2, p2, d = shape
    tag = "%dx%d-%dx%d-d%d%s" % (shape + ("-dup" if duplicates else "",))
    x1, v1, x2, v2, G64, ell = (t.to(dev).contiguous() for t in inputs(shape, duplicates))
    square = n1 == n2 and p1 == p2
    Gs64 = (G64 + G64.t()).contiguous() if square else None
    hyp = torch.tensor([ELL, S, 0.1, 0.0], device=dev)
    hyp_ard = torch.tensor([1.0, S, 0.1, 0.0], device=dev)
    center = ops.column_mean(ctx, x1)
    pk1, pk2 = ops.pack_points(ctx, x1, v1, p1, hyp, center), ops.pack_points(ctx, x2, v2, p2, hyp, center)
    ak1, ak2 = ops.pack_points_ard(ctx, x1, v1, p1, ell, center), ops.pack_points_ard(ctx, x2, v2, p2, ell, center)

    def keep(name, *tensors):
        for i, t in enumerate(tensors):
            if t is not None:
                res["%s %s [%d]" % (name, tag, i)] = t.detach().cpu()

    def grads(with_ell=True):
        return (torch.zeros(n1, d, device=dev), torch.zeros(max(n1 * p1, 1), d, device=dev),
                torch.zeros(d, device=dev) if with_ell else None, torch.zeros(4, device=dev))

    # the RBF entries
    keep("kernel_fwd_rect", ops.kernel_fwd_rect(ctx, pk1, n1, p1, pk2, n2, p2, d, hyp))
    for G in (G64.float(), G64):
        dx, dv, _, dh = grads(False)
        ops.kernel_bwd_rect(ctx, G, pk1, n1, p1, pk2, n2, p2, d, hyp, dx, dv, dh)
        keep("kernel_bwd_rect G %s" % G.dtype, dx, dv, dh)
    if p1 == p2:
        fwds = [("wide", ops.kernel_fwd_wide, ops.kernel_bwd_wide)]
        if d >= 93:
            fwds.append(("general", ops.kernel_fwd, ops.kernel_bwd))
        for name, fwd, bwd in fwds:
            keep("kernel_fwd %s" % name, fwd(ctx, pk1, n1, pk2, n2, d, p1, hyp, jitter=0.0, dtype=torch.float32))
            if square:
                keep("kernel_fwd %s K_ZZ double jitter" % name, fwd(ctx, pk1, n1, pk1, n1, d, p1, hyp, jitter=JITTER, dtype=torch.float64))
            for G, sym in ((G64.float(), False), (G64, False)) + (((Gs64, True),) if square else ()):
                dx, dv, _, dh = grads(False)
                bwd(ctx, G, pk1, n1, pk1 if sym else pk2, n2, d, p1, hyp, sym, dx, dv, dh)
                keep("kernel_bwd %s G %s sym %d" % (name, G.dtype, sym), dx, dv, dh)
    # the ARD and Matern-5/2 entries
    for fam, bwd in (("ard", ops.kernel_bwd_ard), ("matern52", ops.kernel_bwd_matern52)):
        cases = [(G64.float(), False, True), (G64, False, True), (G64.float(), False, False)]
        if square:
            cases += [(Gs64, True, True), (Gs64.float(), True, False)]
        for G, sym, with_ell in cases:
            dx, dv, dl, dh = grads(with_ell)
            bwd(ctx, G, ak1, n1, p1, ak1 if sym else ak2, n2, p2, d, ell, hyp_ard, sym, dx, dv if p1 else None, dl, dh)
            keep("kernel_bwd_%s G %s sym %d d_ell %d" % (fam, G.dtype, sym, with_ell), dx, dv if p1 else None, dl, dh)
    for dtype in (torch.float32, torch.float64):
        keep("kernel_fwd_matern52 %s" % dtype, ops.kernel_fwd_matern52(ctx, ak1, n1, p1, ak2, n2, p2, d, hyp_ard, dtype=dtype))
        if square:
            keep("kernel_fwd_matern52 K_ZZ jitter %s" % dtype,
                 ops.kernel_fwd_matern52(ctx, ak1, n1, p1, ak1, n1, p1, d, hyp_ard, jitter=JITTER, dtype=dtype))
    gbar = G64[:, 0].float().contiguous()
    for fam, diag, diag_bwd in (("ard", ops.kernel_diag_ard, ops.kernel_diag_ard_bwd),
                                ("matern52", ops.kernel_diag_matern52, ops.kernel_diag_matern52_bwd)):
        out = diag(ctx, ak1, n1, p1, d, hyp_ard)
        dl, dh = torch.zeros(d, device=dev), torch.zeros(4, device=dev)
        diag_bwd(ctx, ak1, n1, p1, d, ell, hyp_ard, out, gbar, dl, dh)
        keep("kernel_diag_%s and its backward" % fam, out, dl, dh)


# ---- the second entry list (--narrow): the one-wave 48 x 48 kernels of csrc/assemble.hip on csrc/wave_tile.h --------------------------
# dsvgp_kernel_fwd / _bwd (pair kernels at q = 3, 6; split kernels at q = 11) and dsvgp_kernel_fwd_canon / _bwd_canon.  (d, p): every K
# depth of the T' product's dispatch -- KSM = 8 (d <= 28, also through the canon entries), KSM = 16 (d <= 60) -- and the split kernels.
# (n1, n2): one tile smaller than 48 rows, exactly one full tile (R = 48 / q points), full tiles plus a ragged last row and column tile.
NARROW_DP = [(d, p) for d in (2, 5, 9, 13, 17, 20, 25, 28, 29, 40, 50, 60) for p in (2, 5)] + [(10, 10), (7, 10)]
NARROW_FULL = {(20, 5), (5, 2), (50, 5), (40, 2), (10, 10), (7, 10)}      # every tile shape; the others: the first two and the full tile
NARROW_TILES = [(3, 5), (33, 70), (50, 131), (9, 300)]


def padded(rows, cols, dtype, dev, aligned):
    """a [rows, cols] view: 16-byte aligned rows with ld % 4 == 0, or rows that are not (ld = cols + 3, offset 1)"""
    if aligned:
        return torch.zeros(rows, (cols + 3) // 4 * 4 + 4, dtype=dtype, device=dev)[:, :cols]
    return torch.zeros(rows, cols + 3, dtype=dtype, device=dev)[:, 1:1 + cols]


def run_narrow(ops, ctx, dev, d, p, n1, n2, res):
    q = p + 1
    tag = "d%d-p%d-%dx%d" % (d, p, n1, n2)
    g = torch.Generator().manual_seed(1000 * d + 100 * p + 7 * n1 + n2)
    x1, v1 = torch.rand(n1, d, generator=g).to(dev), torch.randn(n1 * p, d, generator=g).to(dev)
    x2, v2 = torch.rand(n2, d, generator=g).to(dev), torch.randn(n2 * p, d, generator=g).to(dev)
    G64 = torch.randn(n1 * q, n2 * q, generator=g, dtype=torch.float64).to(dev)
    S64 = torch.randn(n1 * q, n1 * q, generator=g, dtype=torch.float64).to(dev)
    S64 = (S64 + S64.t()).contiguous()
    hyp = torch.tensor([ELL, S, 0.1, 0.0], device=dev)
    center = ops.column_mean(ctx, x1)
    pk1, pk2 = ops.pack_points(ctx, x1, v1, p, hyp, center), ops.pack_points(ctx, x2, v2, p, hyp, center)

    def keep(name, *tensors):
        for i, t in enumerate(tensors):
            res["%s %s [%d]" % (name, tag, i)] = t.detach().contiguous().cpu()

    def grads():
        return torch.zeros(n1, d, device=dev), torch.zeros(n1 * p, d, device=dev), torch.zeros(4, device=dev)

    def upstream(G, aligned):
        V = padded(G.shape[0], G.shape[1], G.dtype, dev, aligned)
        V.copy_(G)
        return V

    for dtype in (torch.float32, torch.float64):
        for aligned in (True, False):
            out = padded(n1 * q, n2 * q, dtype, dev, aligned)
            keep("kernel_fwd %s aligned %d" % (dtype, aligned), ops.kernel_fwd(ctx, pk1, n1, pk2, n2, d, p, hyp, out=out, dtype=dtype))
        keep("kernel_fwd K_ZZ jitter %s" % dtype, ops.kernel_fwd(ctx, pk1, n1, pk1, n1, d, p, hyp, jitter=JITTER, dtype=dtype))
    for G, sym in ((G64.float(), False), (G64, False), (upstream(G64.float(), False), False), (S64.float(), True), (S64, True)):
        dx, dv, dh = grads()
        ops.kernel_bwd(ctx, G, pk1, n1, pk1 if sym else pk2, n1 if sym else n2, d, p, hyp, sym, dx, dv, dh)
        keep("kernel_bwd G %s ld %d sym %d" % (G.dtype, G.stride(0) - G.shape[1], sym), dx, dv, dh)
    if not ops.canon_supported(d, p):
        return
    idx = (torch.arange(p, dtype=torch.int32) % d).to(dev)          # one-hot directions e_idx[b], the same for every point of side 2
    e2 = torch.zeros(n2 * p, d, device=dev)
    e2[torch.arange(n2 * p, device=dev), idx.long().repeat(n2)] = 1.0
    ck2 = ops.pack_points(ctx, x2, e2, p, hyp, center)
    for aligned in (True, False):
        keep("kernel_fwd_canon aligned %d" % aligned,
             ops.kernel_fwd_canon(ctx, pk1, n1, ck2, n2, d, p, idx, 0, hyp, out=padded(n1 * q, n2 * q, torch.float32, dev, aligned)))
    for G in (upstream(G64.float(), True), upstream(G64.float(), False), G64):     # LDS-DMA, registers, double
        dx, dv, dh = grads()
        ops.kernel_bwd_canon(ctx, G, pk1, n1, ck2, n2, d, p, idx, 0, hyp, dx, dv, dh)
        keep("kernel_bwd_canon G %s ld %d" % (G.dtype, G.stride(0) - G.shape[1]), dx, dv, dh)


def dump(path, narrow=False):
    import dsvgp_amd
    assert torch.cuda.is_available(), "tiled_ab --dump needs the GPU"
    dev = torch.device("cuda", 0)
    ops = dsvgp_amd._ops
    ctx = ops.Context.get(dev)
    res = {}
    if narrow:
        for d, p in NARROW_DP:
            R = 48 // (p + 1)
            tiles = NARROW_TILES if (d, p) in NARROW_FULL else NARROW_TILES[:2]
            for n1, n2 in tiles + [(R, R)]:
                run_narrow(ops, ctx, dev, d, p, n1, n2, res)
    else:
        for shape in SHAPES:
            run_shape(ops, ctx, dev, shape, False, res)
        run_shape(ops, ctx, dev, DUP, True, res)
    torch.cuda.synchronize()
    torch.save(res, path)
    print("tiled_ab: %d output tensors of %s -> %s" % (len(res), dsvgp_amd._lib.LIB_PATH, path))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bad = sorted(set(a) ^ set(b))
    for k in bad:
        print("ONLY ONE SIDE  %s" % k)
    for k in sorted(set(a) & set(b)):
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k].contiguous().view(torch.uint8),
                                                                                     b[k].contiguous().view(torch.uint8))
        finite = bool(torch.isfinite(a[k]).all())
        print("%-9s %s%s" % ("equal" if same else "DIFFERENT", k, "" if finite else "   (non-finite entries)"))
        if not same:
            bad.append(k)
    print("tiled_ab: %d outputs compared, %d differ" % (len(set(a) | set(b)), len(bad)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="FILE")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--narrow", action="store_true", help="--dump the second entry list: the one-wave kernels of csrc/wave_tile.h")
    args = ap.parse_args()
    if args.dump:
        dump(args.dump, args.narrow)
    return compare(*args.compare) if args.compare else 0


if __name__ == "__main__":
    sys.exit(main())
