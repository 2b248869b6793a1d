"""Kernel-assembly checks across input scale, offset and lengthscale, block by block.  Shared by tests/test_conditioning_host.py (CPU) and
tests/test_gpu_conditioning.py; imports no GPU code.

Every other kernel test of the suite draws x ~ U[0, 1]^d with a lengthscale of order one and scores max|a - b| / max|b| over the whole
interleaved matrix.  The value block scales as s, the first-derivative blocks as s / ell and the Hessian block as s / ell^2, so away from
ell ~ 1 a wrong derivative block disappears under the value block's maximum.  Here

* a REGIME maps a base case (x ~ U[0, 1]^d, generic directions, ell0 = 0.9 for d <= 30 and 0.4 sqrt(d) otherwise) to another scale, offset
  or lengthscale (``REGIMES``).  Inputs and lengthscales are rounded to float32 FIRST; the float64 truth is computed from the rounded
  values, so input rounding is never charged to a kernel.
* the error is taken PER BLOCK TYPE (``block_errors``: value, right-derivative, left-derivative, Hessian), each relative to the truth's
  maximum over the same block.
* the YARDSTICK is the reference's own op sequence run in float32 on the CPU on inputs shifted by c = the float32 column mean of side 1
  (the centring csrc/assemble.hip claims): ``O.kernel_matrix_refseq(x1 - c, x2 - c, v1, v2, ell)``; for ARD and Matern-5/2 the float32
  run of tests/_ard_yardstick.py / tests/_matern_yardstick.py on the centred inputs.
* the BOUND is the rule of tests/test_oracle_golden.py, per block type: err <= 4 y + 2e-7 (float64 routes: 4 y + 1e-13 with the float64
  run of the same op sequence as y; 1e-13 is the suite's float64 tolerance).
* the CONDITIONS keep a regime from being vacuous (``conditions``): value maximum >= 1e-6, every other block's maximum >= 1e-12 of the
  value block's, yardstick error <= 1e-3 in every block."""
import functools
import math

import numpy as np
import torch

import dsvgp_oracle as O
from _ard_yardstick import ard_kernel, ard_lengthscales
from _matern_yardstick import matern_kernel

f32, f64 = torch.float32, torch.float64
S = float(np.float32(1.3))                                   # outputscale of every case (a float32 value)
REGIMES = ("base", "short", "long8", "long64", "offset", "scaled_up", "scaled_down", "far_side2", "near_dup", "clusters")
BWD_REGIMES = ("base", "long64", "scaled_up", "offset", "near_dup")
BLOCKS = ("value", "right", "left", "hessian")
OLD_KTOL, OLD_BWD_TOL = 2e-5, 2e-4                           # the suite's whole-matrix kernel tolerance and its backward tolerance
BWD_TOL = 2e-4

# name -> (kind, n1, n2, d, p1, p2, directions); the shapes reach the kernels named, as the dispatch in csrc/assemble.hip decides
ROUTES = {
    "general-q4": ("rbf", 37, 53, 20, 3, 3, "generic"),
    "general-q1": ("rbf", 37, 53, 6, 0, 0, "generic"),
    "pair-q6-ksm8": ("rbf", 37, 53, 20, 5, 5, "generic"),
    "pair-q3-ksm8": ("rbf", 37, 53, 5, 2, 2, "generic"),
    "pair-ksm16": ("rbf", 30, 60, 50, 5, 5, "generic"),
    "split-q11": ("rbf", 50, 95, 10, 10, 10, "generic"),
    "canon": ("rbf", 33, 70, 20, 5, 5, "canon"),
    "canon2": ("rbf", 40, 52, 10, 10, 10, "canon2"),
    "wide": ("rbf", 11, 23, 200, 3, 3, "generic"),
    "rect-p2-0": ("rbf", 40, 64, 5, 2, 0, "generic"),
    "rect-p2-4": ("rbf", 40, 64, 5, 2, 4, "generic"),
    # (37, 2, 41, 3, 5): the smallest shape of tests/test_gpu_ard.py / test_gpu_matern.py that has all four block types on several tiles
    "ard": ("ard", 37, 41, 5, 2, 3, "generic"),
    "matern": ("matern", 37, 41, 5, 2, 3, "generic"),
    "fp64-plain": ("rbf64", 20, 45, 20, 5, 5, "generic"),
    "fp64-tiled": ("rbf64", 9, 14, 24, 17, 17, "generic"),
}
SEED_SHIFT = {"fp64-tiled": 1}        # (its `short` value maximum: 4.1e-6 against the 1e-6 condition; 1.0e-6 without the shift)
SYMMETRIC_ROUTES = ("pair-q6-ksm8", "split-q11", "fp64-plain", "fp64-tiled")
BWD_ROUTES = ("general-q4", "general-q1", "pair-q6-ksm8", "pair-q3-ksm8", "pair-ksm16", "split-q11", "canon", "canon2", "wide",
              "rect-p2-0", "rect-p2-4", "ard", "matern", "fp64-plain", "fp64-tiled")


def r32(t):
    """round to float32, keep float64 storage"""
    return t.to(f32).to(f64)


class Case:
    """one kernel call: float32-representable inputs held in float64.  ``ell`` is a 0-d tensor (isotropic) or [d] (ARD, Matern)"""

    def __init__(self, kind, x1, x2, v1, v2, p1, p2, ell, idx=None, symmetric=False):
        self.kind, self.x1, self.x2, self.v1, self.v2, self.p1, self.p2, self.ell = kind, x1, x2, v1, v2, p1, p2, ell
        self.idx, self.symmetric = idx, symmetric
        self.n1, self.d = x1.shape
        self.n2 = x2.shape[0]
        self.q1, self.q2 = p1 + 1, p2 + 1

    def with_(self, **kw):
        c = Case(self.kind, self.x1, self.x2, self.v1, self.v2, self.p1, self.p2, self.ell, self.idx, self.symmetric)
        for k, v in kw.items():
            setattr(c, k, v)
        return c


def ell0_of(kind, d):
    if kind in ("ard", "matern"):
        return r32(ard_lengthscales(d))                          # 0.4 sqrt(d) (0.5 + k / (d - 1)): every d_ell[k] distinct
    return r32(torch.tensor(0.9 if d <= 30 else 0.4 * math.sqrt(d), dtype=f64))


def base_case(route, symmetric=False):
    kind, n1, n2, d, p1, p2, dirs = ROUTES[route]
    g = torch.Generator().manual_seed(1000 * n1 + 7 * n2 + 31 * d + p1 + (5 if symmetric else 0) + SEED_SHIFT.get(route, 0))
    x1, x2 = torch.rand(n1, d, generator=g, dtype=f64), torch.rand(n2, d, generator=g, dtype=f64)
    v1, v2 = torch.randn(n1 * p1, d, generator=g, dtype=f64), torch.randn(n2 * p2, d, generator=g, dtype=f64)
    idx = None
    if dirs == "canon":                                          # one-hot directions shared by all points of side 2
        idx = sorted(torch.randperm(d, generator=g)[:p2].tolist())
        v2 = torch.eye(d, dtype=f64)[idx].repeat(n2, 1)
    elif dirs == "canon2":                                       # all d coordinate directions on both sides
        idx = list(range(d))
        v1, v2 = torch.eye(d, dtype=f64).repeat(n1, 1), torch.eye(d, dtype=f64).repeat(n2, 1)
    if symmetric:
        x2, v2, n2 = x1, v1, n1
    return Case(kind, r32(x1), r32(x2), r32(v1), r32(v2), p1, p2, ell0_of(kind, d), idx, symmetric)


def _near_dup(c, g):
    """ten rows of x2 <- rows of x1 + a random vector of length 1e-3 ell0 (per coordinate 1e-3 ell_k u_k for a lengthscale vector); the rows
    keep their own directions.  The symmetric call has one point set: ten of its rows move next to ten others."""
    nd = min(10, c.n1 // 2) if c.symmetric else 10
    n_from = c.n1 - nd if c.symmetric else c.n1
    rows2 = torch.randperm(nd if c.symmetric else c.n2, generator=g)[:nd] + (n_from if c.symmetric else 0)
    rows1 = torch.randperm(max(n_from, nd), generator=g)[:nd] % n_from
    u = torch.randn(nd, c.d, generator=g, dtype=f64)
    x2 = c.x2.clone()
    x2[rows2] = c.x1[rows1] + 1e-3 * c.ell * u / u.norm(dim=1, keepdim=True)
    return x2


def apply_regime(c, name):
    """the case in another regime; every input rounded to float32 after the change"""
    g = torch.Generator().manual_seed(77 + c.n1 + c.n2)
    x1, x2, ell = c.x1, c.x2, c.ell
    if name == "base":
        pass
    elif name == "short":
        ell = ell / 4
    elif name == "long8":
        ell = 8 * ell
    elif name == "long64":
        ell = 64 * ell
    elif name == "offset":
        x1, x2 = x1 + 1024, x2 + 1024
    elif name == "scaled_up":
        x1, x2, ell = x1 * 1e3, x2 * 1e3, 1e3 * ell
    elif name == "scaled_down":
        x1, x2, ell = x1 * 1e-3, x2 * 1e-3, 1e-3 * ell
    elif name == "far_side2":                                    # (the symmetric call has no side 2 of its own: the base case)
        if not c.symmetric:
            x2 = x2 + 3 * ell / math.sqrt(c.d)
    elif name == "near_dup":
        x2 = _near_dup(c, g)
        if c.symmetric:
            x1 = x2
    elif name == "clusters":
        x1 = x1.clone()
        x1[c.n1 // 2:] += 4
        if not c.symmetric:
            x2 = x2.clone()
            x2[c.n2 // 2:] += 4
    else:
        raise ValueError(name)
    x1 = r32(x1)
    x2 = x1 if c.symmetric else r32(x2)
    return c.with_(x1=x1, x2=x2, ell=r32(ell))


@functools.lru_cache(maxsize=None)
def case(route, regime, symmetric=False):
    return apply_regime(base_case(route, symmetric), regime)


# ------------------------------------------------------------------------------------------------ kernels on the CPU
def rect_kernel(x1, v1, p1, x2, v2, p2, ell, assembly=None):
    """K(x1, x2; v1, v2) [n1 (p1 + 1), n2 (p2 + 1)] with p1 != p2 from a square kernel (the oracle's by default): an entry depends only on
    its own row and column directions, so the shorter side is padded with arbitrary directions and the padded rows / columns are dropped"""
    n1, n2, d = x1.shape[0], x2.shape[0], x1.shape[1]
    P = max(p1, p2, 1)
    g = torch.Generator().manual_seed(11)

    def pad(v, n, p):
        out = torch.randn(n, P, d, generator=g, dtype=x1.dtype)
        if p:
            out[:, :p] = v.reshape(n, p, d)
        return out.reshape(n * P, d)

    K = (assembly or O.kernel_matrix)(x1, x2, pad(v1, n1, p1), pad(v2, n2, p2), ell).reshape(n1, P + 1, n2, P + 1)
    return K[:, :p1 + 1, :, :p2 + 1].reshape(n1 * (p1 + 1), n2 * (p2 + 1))


def _kernel(kind, x1, v1, p1, x2, v2, p2, ell, assembly=None):
    if kind == "ard":
        return ard_kernel(x1, v1, p1, x2, v2, p2, ell)
    if kind == "matern":
        return matern_kernel(x1, v1, p1, x2, v2, p2, ell)
    if p1 == p2:
        return (assembly or O.kernel_matrix)(x1, x2, v1, v2, ell)
    return rect_kernel(x1, v1, p1, x2, v2, p2, ell, assembly)


def truth(c):
    """S K in float64 from the float32-rounded inputs: the oracle's pair-wise kernel (rect_kernel for p1 != p2), the ARD / Matern yardsticks"""
    return S * _kernel(c.kind, c.x1, c.v1, c.p1, c.x2, c.v2, c.p2, c.ell)


def yardstick(c, dtype=None):
    """S K by the reference's own op sequence in float32 on inputs centred by the float32 column mean of side 1 (float64 for the fp64 routes)"""
    dt = dtype or (f64 if c.kind == "rbf64" else f32)
    x1, x2 = c.x1.to(dt), c.x2.to(dt)
    ctr = x1.mean(0)
    ell = c.ell.to(dt)
    K = _kernel(c.kind, x1 - ctr, c.v1.to(dt), c.p1, x2 - ctr, c.v2.to(dt), c.p2, ell if ell.dim() else float(c.ell),
                assembly=O.kernel_matrix_refseq)
    return (torch.tensor(S, dtype=dt) * K).to(f64)


def packed_restatement(c, centre=True, dtype=None):
    """S K by the packed formulation of the HIP kernels restated on the CPU in ``dtype`` (float32; float64 for the fp64 routes): rows
    [(x - c) / ell; v / |v|] (ARD and Matern packs: [(x - c) ./ ell; (v / |v|) ./ ell] and a unit scalar lengthscale), T = P1 P2^T,
    |r|^2 = nrm1 + nrm2 - 2 T00 clamped at 0, u = alpha - Ta0, w = T0b - beta, then [[f0, f1 w / ell], [-f1 u / ell, (f1 Tab - f2 u w) / ell^2]]
    with f0 = f1 = f2 = exp(-|r|^2 / 2) (Matern-5/2: its radial family).  ``centre=False``: the same without the shift."""
    from _matern_yardstick import matern52_family, rbf_family
    dtype = dtype or (f64 if c.kind == "rbf64" else f32)
    x1, x2, ell = c.x1.to(dtype), c.x2.to(dtype), c.ell.to(dtype)
    ctr = x1.mean(0) if centre else torch.zeros(c.d, dtype=dtype)
    vec = ell.dim() > 0
    il = torch.ones((), dtype=dtype) if vec else 1 / ell

    def pack(x, v, p):
        xt = (x - ctr) / ell
        V = (v.to(dtype) / v.to(dtype).norm(dim=1, keepdim=True)).reshape(x.shape[0], p, c.d)
        V = V / ell if vec else V
        return xt, V, (xt * xt).sum(1), torch.einsum("nd,npd->np", xt, V)

    a, V1, nrm1, alpha = pack(x1, c.v1, c.p1)
    b, V2, nrm2, beta = pack(x2, c.v2, c.p2)
    nn = (nrm1[:, None] + nrm2[None, :] - 2 * (a @ b.t())).clamp_min(0)
    s = torch.tensor(S, dtype=dtype)
    f0, f1, f2 = (s * f for f in (matern52_family if c.kind == "matern" else rbf_family)(nn))
    u = alpha[:, :, None] - torch.einsum("iad,jd->iaj", V1, b)                  # [i, a, j]
    w = torch.einsum("id,jbd->ijb", a, V2) - beta[None, :, :]                   # [i, j, b]
    Tab = torch.einsum("iad,jbd->iajb", V1, V2)
    top = torch.cat([f0[:, None, :, None], (w * (f1 * il)[..., None])[:, None, :, :]], dim=3)
    hess = (Tab * f1[:, None, :, None] - u[..., None] * w[:, None, :, :] * f2[:, None, :, None]) * il * il
    low = torch.cat([(-u * (f1 * il)[:, None, :])[..., None], hess], dim=3)
    return torch.cat([top, low], dim=1).reshape(c.n1 * c.q1, c.n2 * c.q2).to(f64)


MUTANTS = ("hessian_zero", "uw_dropped", "right_zero")
MUTANT_BLOCK = {"hessian_zero": "hessian", "uw_dropped": "hessian", "right_zero": "right"}


def mutant_kernel(x1, v1, p1, x2, v2, p2, ell, s, mutant=None):
    """s K of the isotropic kernel, differentiable, with one block formula broken (``mutant`` None: the true kernel)"""
    n1, n2, d = x1.shape[0], x2.shape[0], x1.shape[1]
    V1, V2 = O.normalize_rows(v1).reshape(n1, p1, d), O.normalize_rows(v2).reshape(n2, p2, d)
    r = (x1[:, None, :] - x2[None, :, :]) / ell
    k = s * torch.exp(-0.5 * (r * r).sum(-1))
    u = torch.einsum("ijd,iad->iaj", r, V1)
    w = torch.einsum("ijd,jbd->ijb", r, V2)
    T = torch.einsum("iad,jbd->iajb", V1, V2)
    right = w * k[..., None] / ell
    hess = (T - (0 if mutant == "uw_dropped" else 1) * u[..., None] * w[:, None, :, :]) * k[:, None, :, None] / ell ** 2
    if mutant == "right_zero":
        right = right * 0
    if mutant == "hessian_zero":
        hess = hess * 0
    top = torch.cat([k[:, None, :, None], right[:, None, :, :]], dim=3)
    low = torch.cat([(-u * k[:, None, :] / ell)[..., None], hess], dim=3)
    return torch.cat([top, low], dim=1).reshape(n1 * (p1 + 1), n2 * (p2 + 1))


# ------------------------------------------------------------------------------------------------ the metric
def blocks_of(K, n1, q1, n2, q2):
    """the four block types of an interleaved matrix, as views"""
    K4 = K.reshape(n1, q1, n2, q2)
    return {"value": K4[:, 0, :, 0], "right": K4[:, 0, :, 1:], "left": K4[:, 1:, :, 0], "hessian": K4[:, 1:, :, 1:]}


def block_maxima(K_ref, n1, q1, n2, q2):
    return {k: (float(b.abs().max()) if b.numel() else None) for k, b in blocks_of(K_ref.double().cpu(), n1, q1, n2, q2).items()}


def block_errors(K, K_ref, n1, q1, n2, q2):
    """max|K - K_ref| over each block type / max|K_ref| over the same block -> {value, right, left, hessian}; an absent block (q = 1) is left out"""
    K, K_ref = K.double().cpu(), K_ref.double().cpu()
    a, b = blocks_of(K, n1, q1, n2, q2), blocks_of(K_ref, n1, q1, n2, q2)
    return {k: float((a[k] - b[k]).abs().max() / b[k].abs().max().clamp_min(1e-300)) for k in BLOCKS if b[k].numel()}


def relmax(a, b):
    """the suite's whole-matrix metric"""
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def bounds(y, fp64=False):
    """4 y + 2e-7 per block type (float64 routes: 4 y + 1e-13)"""
    return {k: 4 * v + (1e-13 if fp64 else 2e-7) for k, v in y.items()}


def _off_diagonal(K, K_ref, n, q):
    """K with its diagonal micro-blocks replaced by K_ref's (the symmetric call)"""
    out = K.double().cpu().clone().reshape(n, q, n, q)
    ref = K_ref.reshape(n, q, n, q)
    i = torch.arange(n)
    out[i, :, i, :] = ref[i, :, i, :]
    return out.reshape(n * q, n * q)


@functools.lru_cache(maxsize=None)
def reference(route, regime, symmetric=False):
    """(case, truth, yardstick errors per block): once per (route, regime), shared and never modified.  Symmetric call: the yardstick's
    error is taken off the diagonal micro-blocks.  There the truth has exact zeros (r = 0) that the op sequence misses by its rounding
    noise, which against a small off-diagonal block maximum (``short``) would make y, and so the bound, say nothing; the kernels under test
    are held to the whole matrix, diagonal micro-blocks included."""
    c = case(route, regime, symmetric)
    K = truth(c)
    Y = yardstick(c)
    if symmetric:
        Y = _off_diagonal(Y, K, c.n1, c.q1)
    return c, K, block_errors(Y, K, c.n1, c.q1, c.n2, c.q2)


# The one exception to 4 y + 2e-7, as a table.  ARD and Matern-5/2 have difference-form yardsticks, which carry no quadratic expansion; in
# ``short`` and ``clusters`` the float32 restatement of the packed formulation on the CPU exceeds 4 y + 2e-7 itself and so does the kernel
# (measured on the MI355X, worst block, error against 4 y + 2e-7: ARD short 1.16e-6 / 9.7e-7, clusters 6.5e-6 / 1.3e-6; Matern short
# 1.9e-6 / 1.0e-6, clusters 8.1e-6 / 1.2e-6): the formulation is the limit, not a route.  There, and nowhere else, the route's bound in
# that regime is 4x the restatement's error, block by block.  tests/test_conditioning_host.py asserts that the restatement does exceed.
FORMULATION_LIMITED = (("ard", "short"), ("ard", "clusters"), ("matern", "short"), ("matern", "clusters"))


def restatement_errors(route, regime, symmetric=False):
    c, K, _ = reference(route, regime, symmetric)
    return block_errors(packed_restatement(c), K, c.n1, c.q1, c.n2, c.q2)


@functools.lru_cache(maxsize=None)
def effective_bounds(route, regime, symmetric=False):
    """-> ({block: bound}, {block: (yardstick bound, restatement error)}; the second is empty outside ``FORMULATION_LIMITED``).  The bound
    is 4 y + 2e-7 (fp64: 4 y + 1e-13) for every route and regime but the four pairs of that table.  Nothing here depends on the code
    under test."""
    c, K, y = reference(route, regime, symmetric)
    b = bounds(y, c.kind == "rbf64")
    if (route, regime) not in FORMULATION_LIMITED:
        return b, {}
    pr = restatement_errors(route, regime, symmetric)
    return {k: max(b[k], 4 * pr[k]) for k in b}, {k: (b[k], pr[k]) for k in b}


def conditions(route, regime, symmetric=False):
    """what keeps a regime from being vacuous -> list of violations (empty: fine)"""
    c, K, y = reference(route, regime, symmetric)
    mx = block_maxima(K, c.n1, c.q1, c.n2, c.q2)
    bad = []
    if not mx["value"] >= 1e-6:
        bad.append("value maximum %.2e < 1e-6" % mx["value"])
    for k in BLOCKS[1:]:
        if mx[k] is not None and not mx[k] >= 1e-12 * mx["value"]:
            bad.append("%s maximum %.2e < 1e-12 of the value block's %.2e" % (k, mx[k], mx["value"]))
    for k, v in y.items():
        if not v <= 1e-3:
            bad.append("yardstick error %.2e of the %s block > 1e-3" % (v, k))
    return bad


# ------------------------------------------------------------------------------------------------ the backward
MASKS = BLOCKS + ("dense",)


def masked_upstream(G, which, n1, q1, n2, q2):
    """G with everything outside one block type zeroed (``dense``: G itself)"""
    if which == "dense":
        return G
    out = torch.zeros_like(G)
    blocks_of(out, n1, q1, n2, q2)[which].copy_(blocks_of(G, n1, q1, n2, q2)[which])
    return out


def upstream(c):
    g = torch.Generator().manual_seed(5 + c.n1 * c.q1 + c.n2 * c.q2)
    G = torch.randn(c.n1 * c.q1, c.n2 * c.q2, generator=g, dtype=f64)
    return r32(G + G.t() if c.symmetric else G)


def _differentiable(c, dt, centred):
    x1 = c.x1.to(dt)
    ctr = x1.mean(0) if centred else 0
    x1r = x1.clone().requires_grad_(True)
    v1r = c.v1.to(dt).clone().requires_grad_(True)
    er = c.ell.to(dt).clone().requires_grad_(True)
    sr = torch.tensor(S, dtype=dt, requires_grad=True)
    x2, v2 = (x1r, v1r) if c.symmetric else (c.x2.to(dt), c.v2.to(dt))
    K = sr * _kernel(c.kind, x1r - ctr, v1r, c.p1, x2 - ctr, v2, c.p2, er, assembly=O.kernel_matrix_refseq if centred else None)
    return K, (x1r, v1r, er, sr)


def _grads(K, leaves, G):
    out = torch.autograd.grad((K * G.to(K.dtype)).sum(), leaves, retain_graph=True, allow_unused=True)
    return [(torch.zeros_like(l) if o is None else o).double() for o, l in zip(out, leaves)]


def _tangent(c, k=None):
    """dK / d ell (ell_k for a lengthscale vector) elementwise, S K included, in float64 by forward-mode differentiation"""
    import torch.autograd.forward_ad as fwAD
    t = torch.ones_like(c.ell) if k is None else torch.eye(c.d, dtype=f64)[k]
    kind = "ard" if c.kind in ("rbf", "rbf64") else c.kind          # (equal lengthscales: the same kernel, written without in-place writes)
    with fwAD.dual_level():
        e = fwAD.make_dual(c.ell.expand(c.d).clone() if c.ell.dim() == 0 else c.ell, t.expand(c.d).clone() if t.dim() == 0 else t)
        return fwAD.unpack_dual(S * _kernel(kind, c.x1, c.v1, c.p1, c.x2, c.v2, c.p2, e)).tangent


@functools.lru_cache(maxsize=None)
def backward_reference(route, regime, symmetric=False):
    """per mask: float64 autograd gradients (d_x1, d_v1, d_ell, d_s) of sum(G S K), the reductions' own conditioning scales
    sum|G_ij dK_ij / d theta| (float64), and the float32 autograd yardstick's gradients (centred op sequence)"""
    c = case(route, regime, symmetric)
    G = upstream(c)
    K64, l64 = _differentiable(c, f64, False)
    K32, l32 = _differentiable(c, f64 if c.kind == "rbf64" else f32, True)
    dK = [_tangent(c)] if c.ell.dim() == 0 else [_tangent(c, k) for k in range(c.d)]
    Ks = K64.detach() / S
    out = {}
    for m in MASKS:
        Gm = masked_upstream(G, m, c.n1, c.q1, c.n2, c.q2)
        scale_ell = torch.stack([(Gm * t).abs().sum() for t in dK]).reshape(c.ell.shape)
        out[m] = {"G": Gm, "truth": _grads(K64, l64, Gm), "yard": _grads(K32, l32, Gm), "scale_ell": scale_ell,
                  "scale_s": float((Gm * Ks).abs().sum())}
    return c, out


def backward_errors(got, ref):
    """got = (d_x1, d_v1, d_ell, d_s) against ref (one mask's entry of ``backward_reference``) -> errors in units of their scale: d_x1 and
    d_v1 relative to that gradient's own maximum under that mask, d_ell and d_s relative to sum|G dK / d theta|; ``None`` where the true
    gradient is identically zero (checked for exact zeros by the caller)"""
    tx, tv, te, ts = ref["truth"]
    errs = {}
    for name, a, b in (("d_x1", got[0], tx), ("d_v1", got[1], tv)):
        if b.numel() == 0:
            continue
        errs[name] = float((a.double().cpu() - b).abs().max() / b.abs().max()) if float(b.abs().max()) > 0 else None
    se = ref["scale_ell"]
    errs["d_ell"] = float(((torch.as_tensor(got[2]).double().cpu().reshape(se.shape) - te).abs() / se.clamp_min(1e-300)).max()) if float(se.max()) > 0 else None
    errs["d_s"] = abs(float(got[3]) - float(ts)) / ref["scale_s"] if ref["scale_s"] > 0 else None
    return errs
