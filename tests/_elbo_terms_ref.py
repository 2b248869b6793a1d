"""The float64 yardstick of the ELBO scalar and reduction kernels (csrc/elbo.hip, the fp64 tails of csrc/assemble64.hip, the row
statistics of csrc/ciq.hip): plain torch in float64, written from the closed forms in include/dsvgp.h and independent of the HIP code.

Every reference is evaluated on ``V`` objects: a value and, beside it, the sum of the absolute values of the addends the value is made
of before any cancellation (``V.a``).  Sums add the magnitudes, a product multiplies them (the magnitudes of the expanded product), a
quotient carries the relative magnitude of its divisor, and a ``log`` / ``exp`` adds 4 ulp of its own value.  The two bound helpers at
``bound_elem`` / ``bound_sum`` turn ``V.a`` into the only tolerances of tests/test_gpu_elbo_terms.py; tests/test_elbo_terms_host.py checks the values against
float64 autograd through the oracle's formulas and the case tables against deliberately broken references.

``broken`` selects one deliberately wrong variant of a reference (the sensitivity check of the host file):
    "drop_last"   the last row (triangular sums) or column (column sums) left out of every sum; past 1024 rows or columns one of them is
                  below any bound that grows with the chain of additions (the atomics of a thousand workgroups on one address), and the
                  trailing ceil(n / 1024) are left out (``tail``)
    "diag_offdiag" the diagonal element of the KL gradient treated as an off-diagonal one
    "unmasked"    the four elements of a 16-byte group that straddles the diagonal all used
    "sums3_added" trace(G) added instead of subtracted
    "no_scale"    the scaling flag ignored
"""
import math

import torch

import dsvgp_oracle as O

f64 = torch.float64
U32, U64 = 2.0 ** -24, 2.0 ** -53
LOG2PI = math.log(2.0 * math.pi)
FN_ULP = 0.5            # a library function adds 0.5 |value| to its addends: 4 u |value| under the 8 u of ``bound_elem``.  With an ulp of
#                         2 u that is 2 ulp, half of the 4 ulp that may be charged: the stricter figure


# ---------------------------------------------------------------------------------------------------------------- tracked values
def _t(x):
    return x if torch.is_tensor(x) else torch.tensor(float(x), dtype=f64)


class V:
    """value ``v`` and the sum ``a`` of the absolute values of its addends (both float64 tensors of one shape)"""

    def __init__(self, v, a=None):
        self.v = _t(v).to(f64)
        self.a = self.v.abs() if a is None else _t(a).to(f64)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.a + o.a)

    __radd__ = __add__

    def __neg__(self):
        return V(-self.v, self.a)

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, self.a + o.a)

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, self.a * o.a)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        return V(self.v / o.v, self.a / o.v.abs() * (o.a / o.v.abs()))

    def __rtruediv__(self, o):
        return V.of(o) / self

    def __getitem__(self, k):
        return V(self.v[k], self.a[k])

    def sum(self, dim=None):
        return V(self.v.sum(), self.a.sum()) if dim is None else V(self.v.sum(dim), self.a.sum(dim))

    def log(self):
        l = torch.log(self.v)
        return V(l, l.abs() * (1.0 + FN_ULP) + self.a / self.v.abs())

    def where(self, mask, other):
        other = V.of(other)
        return V(torch.where(mask, self.v, other.v), torch.where(mask, self.a, other.a))


def sigmoid(x):
    """1 / (1 + exp(-x)) of an exact x: the exponential's 4 ulp reach the value with a factor below one"""
    s = torch.sigmoid(_t(x).to(f64))
    return V(s, s * (1.0 + FN_ULP))


def stack(vs):
    return V(torch.stack([V.of(x).v.reshape(()) for x in vs]), torch.stack([V.of(x).a.reshape(()) for x in vs]))


# ---------------------------------------------------------------------------------------------------------------- the two bounds
def bound_elem(a, u):
    """elementwise outputs: |got - ref| <= 8 u sum|addends|"""
    return 8.0 * u * a


def bound_sum(a, u, c):
    """sums: |got - ref| <= (c + 8) u sum|addends|, c the longest chain of additions any partial passes through"""
    return (c + 8.0) * u * a


def ratio(got, ref, bound):
    """max(err / bound) of one output; NaN / Inf in ``got`` gives inf"""
    got = got.detach().to("cpu", f64).reshape(-1)
    refv, b = ref.v.reshape(-1), bound.reshape(-1)
    assert got.shape == refv.shape, (got.shape, refv.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - refv).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / b)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return float(r.max())


# ---------------------------------------------------------------------------------------------------------------- inputs
def r32(x):
    """rounded to float32 first, then widened: input rounding is not charged to the kernel"""
    return x.to(torch.float32).to(f64)


def draw(g, *shape):
    """magnitude in [0.5, 1.5], random sign"""
    mag = 0.5 + torch.rand(*shape, generator=g, dtype=f64)
    return r32(mag * (2.0 * torch.randint(0, 2, shape, generator=g).to(f64) - 1.0))


def tail(n):
    """the columns "drop_last" leaves out of a sum over n columns"""
    return (n + 1023) // 1024


def kept(n, broken):
    return slice(0, n - tail(n)) if broken == "drop_last" else slice(0, n)


def draw_diag(g, n):
    """positive, in [0.5, 0.75] or [1.25, 1.5]: inside [0.5, 1.5] and log L_ii^2 is no vanishing addend"""
    u = torch.rand(n, generator=g, dtype=f64)
    return r32(torch.where(u < 0.5, 0.5 + 0.5 * u, 1.0 + 0.5 * u))


# ---------------------------------------------------------------------------------------------------------------- a. ls_rows
LS_NUM_DATA, LS_ROWS, LS_T1_SCALE, LS_NOISE = 57.0, 997.0, 0.37, 0.004
LS_MPS = (1, 3, 4, 5, 8, 63, 64, 65, 256, 257, 260, 516)
# (op, scale, add_kl)
LS_OPS = (("kl_terms", 0, 1), ("kl_terms_scaled", 1, 0), ("kl_terms_scaled", 1, 1), ("variational_terms", 0, 0),
          ("variational_terms", 0, 1), ("variational_terms", 1, 0), ("variational_terms", 1, 1))
LS_LAYOUTS = ("contiguous", "ld+4", "ld+1")
LS_CASES = tuple((Mp, lay) for Mp in LS_MPS for lay in (LS_LAYOUTS if Mp % 4 == 0 else LS_LAYOUTS[:1]))
LS_BIG_MP = 8196


def ls_inputs(Mp):
    """m, L_S (full square, finite: the GPU file poisons what must not be read), T, the earlier d_m, G's diagonal"""
    g = torch.Generator().manual_seed(1000 + Mp)
    L = draw(g, Mp, Mp)
    L.diagonal().copy_(draw_diag(g, Mp))
    T = draw(g, Mp, Mp)
    T[-1] = T[-1].abs() * L[-1].sign()          # (the last row's products share a sign: leaving the row out is visible in sums2)
    return dict(m=draw(g, Mp), L=L, T=T, dm0=draw(g, Mp), Gd=draw(g, Mp).abs(), noise=r32(torch.tensor(LS_NOISE, dtype=f64)))


def ls_rows_ref(inp, scale, add_kl, broken=None, num_data=LS_NUM_DATA, rows=LS_ROWS, t1_scale=LS_T1_SCALE):
    """d_LS <- [T / (noise rows)] + dKL/dL_S / num_data on the lower triangle (zero above); d_m += m / num_data; KL;
    sums2 = t1_scale sum_{i>=j} L_ij T_ij; sums3 = trace(G)"""
    m, L, T = inp["m"], inp["L"], inp["T"]
    Mp = m.shape[0]
    i, j = torch.arange(Mp)[:, None], torch.arange(Mp)[None, :]
    use = (j <= (i // 4) * 4 + 3) if broken == "unmasked" else (j <= i)
    zero = torch.zeros(Mp, Mp, dtype=f64)
    Lm, Tm = V(torch.where(use, L, zero)), V(torch.where(use, T, zero))
    sc = 1.0 / (V(inp["noise"]) * rows) if (scale and broken != "no_scale") else V(1.0)
    inv_nd = V(1.0 / num_data)
    d = Tm * sc
    out = {}
    rs = slice(0, Mp - 1) if broken == "drop_last" else slice(0, Mp)
    if add_kl:
        diag = (i == j) & use if broken != "diag_offdiag" else torch.zeros_like(use)
        g = (Lm - 1.0 / V(torch.where(use, L, zero + 1.0))).where(diag, Lm) * inv_nd
        d = d + g
        out["d_m"] = V(inp["dm0"]) + V(m) * inv_nd
        rowkl = 0.5 * (V(m) * V(m) + (Lm * Lm).sum(1) - 1.0 - (V(L.diagonal()) * V(L.diagonal())).log())
        out["kl"] = rowkl[rs].sum()
    out["d_LS"] = d.where(use, 0.0)
    out["sums2"] = t1_scale * (Lm * Tm).sum(1)[rs].sum()
    out["sums3"] = V(inp["Gd"])[rs].sum()
    return out


def ls_chain(Mp):
    """longest chain of additions of ls_rows_kernel + ls_rows_reduce_kernel for one scalar: a lane's loop (ceil(Mp / 64) fmas in the
    scalar kernel, 4 ceil(Mp / 256) <= ceil(Mp / 64) + 3 in the 16-byte one), 6 shuffle steps, the 4 operations of the per-row value
    (m^2 +, - 1, - log, * 1/2), then the fixed-order sum in double and its one rounding to float (1), the t1_scale product (1)"""
    return (Mp + 63) // 64 + 3 + 6 + 4 + 1 + 1


# ---------------------------------------------------------------------------------------------------------------- b. residual
RES_NCOLS = (1, 63, 64, 65, 255, 256, 257, 1000, 512 * 256 + 77)
RES_NOISE = 0.004


def res_inputs(ncols):
    g = torch.Generator().manual_seed(2000 + ncols % 9973)
    mu, r = 0.25 * draw(g, ncols), draw(g, ncols)
    r[ncols - tail(ncols):] = r[ncols - tail(ncols):].abs()          # (the columns "drop_last" leaves out share a sign)
    return dict(mu=mu, y=r32(mu + r), noise=r32(torch.tensor(RES_NOISE, dtype=f64)), rows=3.0 * ncols)


def residual_ref(inp, broken=None):
    """mu_bar = -(y - mu) / (noise rows); sums0 = sum r^2, sums1 = sum mu_bar.  y - mu of two floats is one rounding of r itself."""
    r = V(inp["y"]) - inp["mu"] if isinstance(inp["mu"], V) else V(inp["y"] - inp["mu"])        # (a V mu carries its own addends)
    mb = -r / V(inp["noise"]) * (1.0 / inp["rows"])
    n = r.v.shape[0]
    cs = kept(n, broken)
    return dict(mu_bar=mb, sums0=(r * r)[cs].sum(), sums1=mb[cs].sum())


def res_chain(ncols, deterministic):
    """residual_kernel: a lane's loop trips ceil(ncols / (256 blocks)), 6 shuffle steps, 3 additions over the 4 waves, then the atomics
    of all blocks <= 512 on one address -- or, in deterministic mode, the double sum of the partials and its one rounding"""
    blocks = min(512, (ncols + 255) // 256)
    return (ncols + 256 * blocks - 1) // (256 * blocks) + 6 + 3 + (1 if deterministic else blocks)


# ---------------------------------------------------------------------------------------------------------------- c. trace
TRACE_NS = (1, 2, 255, 256, 257, 1030)
TRACE_PRE = (0.75, -1.25)


def trace_inputs(n):
    g = torch.Generator().manual_seed(3000 + n)
    L, T = draw(g, n, n), draw(g, n, n)
    T[-1] = T[-1].abs() * L[-1].sign()          # (as ls_inputs)
    return dict(L=L, T=T, Gd=draw(g, n).abs())


def trace_ref(inp, broken=None, t1_scale=LS_T1_SCALE):
    """sums2 += t1_scale sum_{i>=j} L_ij T_ij; sums3 += trace(G)"""
    n = inp["Gd"].shape[0]
    low = torch.ones(n, n, dtype=torch.bool).tril()
    z = torch.zeros(n, n, dtype=f64)
    rs = kept(n, broken)
    lt =(V(torch.where(low, inp["L"], z)) * V(torch.where(low, inp["T"], z))).sum(1)
    return dict(sums2=TRACE_PRE[0] + t1_scale * lt[rs].sum(), sums3=TRACE_PRE[1] + V(inp["Gd"])[rs].sum())


def trace_chain(n):
    """trace_kernel: workgroup b owns rows b, b + grid, ... (grid = min(n, 1024)); a thread's fma chain is the sum over those rows of
    ceil((i + 1) / 256) <= ceil(n / grid) ceil(n / 256); 6 shuffle steps, 3 additions over the waves, the t1_scale product, then the
    atomics of all workgroups and the earlier content of sums on one address (grid + 1)"""
    grid = min(n, 1024)
    return ((n + grid - 1) // grid) * ((n + 255) // 256) + 6 + 3 + 1 + grid + 1


# ---------------------------------------------------------------------------------------------------------------- d. scalar tails
FIN_SHAPES = ((1, 0), (7, 0), (5, 3), (1000, 20))
FIN_HYPS = ((0.3, 2.5, 0.004), (1.7, 0.2, 1.0001e-4))
FIN_CHAIN = 16      # elbo_fast_finalize_body, scal[0]: 5 roundings in sum_prior, + sums2, - sums3, + sum_r2, / noise, log, 2 additions,
#                     the nrow product, the last addition, * -1/2, and (float)(1 / rows): the longest of the five outputs


def fin_inputs(npts, p, hyp):
    nrow = npts * (p + 1)
    g = torch.Generator().manual_seed(4000 + nrow)
    s2 = r32(torch.tensor(0.9 * nrow * (1.0 + float(torch.rand((), generator=g))), dtype=f64))
    sums = torch.stack([r32(torch.tensor(1.1 * nrow, dtype=f64)), r32(torch.tensor(-0.7, dtype=f64)), s2, r32(s2 * (1.0 - 1e-3))])
    return dict(sums=sums, hyp=r32(torch.tensor(list(hyp) + [0.0], dtype=f64)), npts=npts, p=p, rows=2.0 * nrow + 3.0)


def fast_scalars(sum_r2, sum_mubar, s2, s3, hyp, npts, p, rows, broken=None):
    """scal[0..4] of the ELBO fast path (var_bar constant): sum ll, d loss / d noise, d / d constant, d / d outputscale and
    d / d lengthscale through the prior diagonal; loss = -sum ll / rows"""
    ell, s, noise = V(hyp[0]), V(hyp[1]), V(hyp[2])
    nrow = float(npts * (p + 1))
    tr = (V.of(s2) + V.of(s3)) if broken == "sums3_added" else (V.of(s2) - V.of(s3))
    sum_var = float(npts) * s + float(npts * p) * s / (ell * ell) + nrow * O.KXX_JITTER + tr
    tot = V.of(sum_r2) + sum_var
    vbar = 0.5 / (noise * rows)
    return stack([-0.5 * (tot / noise + nrow * (1.0 + noise.log() + LOG2PI)),
                  (0.5 / rows) * (nrow / noise - tot / (noise * noise)),
                  V.of(sum_mubar),
                  vbar * float(npts) + vbar * float(npts * p) / (ell * ell),
                  vbar * float(npts * p) * (-2.0) * s / (ell * ell * ell)])


def finalize_ref(inp, broken=None):
    s = inp["sums"]
    return fast_scalars(s[0], s[1], s[2], s[3], inp["hyp"], inp["npts"], inp["p"], inp["rows"], broken)


EPI_RAW = (-6.0, 0.0, 9.0)


def epilogue_inputs():
    g = torch.Generator().manual_seed(4500)
    return dict(scal=draw(g, 8), kl0=draw(g, 1).abs(), raw=r32(torch.tensor(EPI_RAW, dtype=f64)), d_hyp=draw(g, 4), d_raw=draw(g, 3),
                d_const=draw(g, 1), rows=391.0, num_data=57.0)


def epilogue_ref(inp):
    """d_hyp += (scal4, scal3, scal1); d_raw_k += d_hyp_k sigmoid(raw_k) (softplus chain rule); d_const += scal2;
    loss = -scal0 / rows + kl0 / num_data (overwritten)"""
    sc, dh = V(inp["scal"]), V(inp["d_hyp"])
    d = [dh[0] + sc[4], dh[1] + sc[3], dh[2] + sc[1]]
    return dict(d_hyp=stack(d), d_raw=stack([V(inp["d_raw"])[k] + d[k] * sigmoid(inp["raw"][k]) for k in range(3)]),
                d_const=V(inp["d_const"])[0] + sc[2],
                loss=-sc[0] * (1.0 / inp["rows"]) + V(inp["kl0"])[0] * (1.0 / inp["num_data"]))


def hyp_backward_ref(inp):
    dh = V(inp["d_hyp"])
    return stack([V(inp["d_raw"])[k] + dh[k] * sigmoid(inp["raw"][k]) for k in range(3)])


SCALE_SIZES = ((9, None, None), (5, None, 2), (257, 300, 2), (2048 * 256 + 13, 1, 1), (3, 0, 4))     # one, two, three tensors; an empty one


def scale_ref(x, noise, rows, broken=None):
    return V(x) if broken == "no_scale" else V(x) * (1.0 / (V(noise) * rows))


# ---------------------------------------------------------------------------------------------------------------- e/f. the general path
def colstats_ref(A, W, m, broken=None):
    """mu0 = A^T m; cs = colsum(W^2 - A^2) (None without W)"""
    Mp = A.shape[0]
    rs = slice(0, Mp - 1) if broken == "drop_last" else slice(0, Mp)
    mu0 = (V(A) * V(m)[:, None])[rs].sum(0)
    cs = (V(W) * V(W) - V(A) * V(A))[rs].sum(0) if W is not None else None
    return mu0, cs


def likelihood_ref(mu0, cs, y, c, p, hyp, mll_type, rows, jitter=O.KXX_JITTER, broken=None):
    """per output: mu = mu0 + c, var = s dg + jitter + cs, varn = max(var + noise, 1e-6); ll of GaussianLikelihood.expected_log_prob
    (mll_type 0) or log_marginal (1) as dsvgp_oracle.elbo_forward; loss = -sum ll / rows.  Returns mu, varn, mu_bar = d loss / d mu0,
    var_bar = d loss / d cs and scal[0..4] = sum ll, d / d noise, d / d constant, d / d outputscale, d / d lengthscale (prior diagonal)."""
    mu0, cs = V.of(mu0), V.of(cs)
    n = mu0.v.shape[0]
    ell, s, noise = V(hyp[0]), V(hyp[1]), V(hyp[2])
    isf = (torch.arange(n) % (p + 1)) == 0
    dg_s = V(torch.ones(n, dtype=f64)).where(isf, 1.0 / (ell * ell) * V(torch.ones(n, dtype=f64)))       # d var / d s
    dg_l = V(torch.zeros(n, dtype=f64)).where(isf, -2.0 * s / (ell * ell * ell) * V(torch.ones(n, dtype=f64)))
    mu = mu0 + V.of(c)
    r = V.of(y) - mu
    vraw = s * dg_s + jitter + cs + noise
    clamped = vraw.v < O.MIN_VARIANCE
    varn = V(torch.full((n,), O.MIN_VARIANCE, dtype=f64)).where(clamped, vraw)
    if mll_type == 0:
        ll = -0.5 * ((r * r + varn) / noise + noise.log() + LOG2PI)
        dmu, dvn = r / noise, -0.5 / noise * V(torch.ones(n, dtype=f64))
        dnoise = 0.5 * (r * r + varn) / (noise * noise) - 0.5 / noise
    else:
        tot = varn + noise
        ll = -0.5 * (r * r / tot + tot.log() + LOG2PI)
        dmu, dvn = r / tot, 0.5 * (r * r / (tot * tot) - 1.0 / tot)
        dnoise = dvn
    dvar = V(torch.zeros(n, dtype=f64)).where(clamped, dvn)
    dnoise = dnoise + dvar
    mb, vb = -dmu * (1.0 / rows), -dvar * (1.0 / rows)
    cs_ = kept(n, broken)
    scal = stack([ll[cs_].sum(), (-dnoise * (1.0 / rows))[cs_].sum(), mb[cs_].sum(), (vb * dg_s)[cs_].sum(), (vb * dg_l)[cs_].sum()])
    return dict(mu=mu, varn=varn, mu_bar=mb, var_bar=vb, scal=scal)


def abar_ref(A, U, m, mu_bar, var_bar):
    """Abar = m mu_bar^T + 2 (U - A) diag(var_bar) (U None: U = A), Av = 2 A diag(var_bar)"""
    vb2 = 2.0 * V(var_bar)[None, :]
    ab = V(m)[:, None] * V(mu_bar)[None, :]
    if U is not None:
        ab = ab + (V(U) - V(A)) * vb2
    return ab, V(A) * vb2


def fast_tail64_ref(mu0, y, c, npts, pd, hyp, tvar, rows, broken=None):
    """the fp64 ELBO fast path's tail: mu = mu0 + c, mu_bar = -(y - mu) / (noise rows); scal = {sum ll, d / d noise, d / d constant,
    d / d outputscale, d / d lengthscale, vbar, sum r^2, sum r} with sum_j var_j = s npts (1 + pd / ell^2) + ncols 1e-4 + tvar"""
    mu = V(mu0) + V.of(c)
    r = V(y) - mu
    n = r.v.shape[0]
    cs_ = kept(n, broken)
    noise = V(hyp[2])
    mb = -r / (noise * rows)
    ss, sr = (r * r)[cs_].sum(), r[cs_].sum()
    sc = fast_scalars(ss, -sr / (noise * rows), tvar, 0.0, hyp, npts, pd, rows)
    return dict(mu=mu, mu_bar=mb, scal=stack([sc[0], sc[1], sc[2], sc[3], sc[4], 0.5 / (noise * rows), ss, sr]))


E_MPS, E_B, E_P = (60, 61), 17, 2


def e_inputs(Mp):
    """case e: A [Mp, B (p + 1)], L_S, m, y, c, hyp (float32-rounded), rows"""
    g = torch.Generator().manual_seed(Mp)
    Bp = E_B * (E_P + 1)
    A = r32(draw(g, Mp, Bp) / math.sqrt(Mp))
    L = r32(torch.tril(draw(g, Mp, Mp)) / math.sqrt(Mp))
    L.diagonal().copy_(draw_diag(g, Mp))
    return dict(A=A, L=L, m=draw(g, Mp), y=draw(g, Bp), c=r32(torch.tensor([0.3], dtype=f64)),
                hyp=r32(torch.tensor([0.7, 1.3, 0.05, 0.0], dtype=f64)), rows=2.0 * Bp + 1.0)


def e_chain_general(Mp):
    """3 Mp (colstats_kernel: one chunk of Mp <= 128 rows, w w - a a + per row) + 4 (chunks, prior diagonal, jitter, noise) + 12 (the per-column
    value of likelihood_kernel) + 1 (its loop) + 6 + 3 + 1 (shuffles, waves, one workgroup's atomic) + 2 (W rounded once to float: 2 u on w w)"""
    return 3 * Mp + 4 + 12 + 1 + 6 + 3 + 1 + 2


def e_chain_fast(Mp):
    """Mp + 2 (mu_j: Mp fmas, + c, then y -) + the residual or the ls_rows chain, whichever is longer, + FIN_CHAIN + 2 (G and T rounded once)"""
    return Mp + 2 + max(res_chain(E_B * (E_P + 1), False), ls_chain(Mp)) + FIN_CHAIN + 2


F64_MPS, F64_BPS = (1, 7, 130), (1, 6, 255, 258, 1026)
F64_HYP = (0.7, 1.3, 0.05, 0.0)


def f64_inputs(Mp, Bp):
    g = torch.Generator().manual_seed(6000 + 7 * Mp + Bp)
    d64 = lambda *s: (0.5 + torch.rand(*s, generator=g, dtype=f64)) * (2.0 * torch.randint(0, 2, s, generator=g).to(f64) - 1.0)
    sc = 1.0 / math.sqrt(2.0 * Mp)
    A = sc * d64(Mp, Bp)
    W = A.abs() * (1.0 + 0.5 * torch.rand(Mp, Bp, generator=g, dtype=f64))      # |W| >= |A|: a positive variance surplus
    return dict(A=A, W=W, U=sc * d64(Mp, Bp), m=d64(Mp), y=d64(Bp), c=torch.tensor([0.3], dtype=f64),
                hyp=torch.tensor(F64_HYP, dtype=f64), mu_bar=d64(Bp), var_bar=d64(Bp))


def f64_p(Bp):
    """directions per point of a [Bp] output vector: the largest of 2, 1, 0 that divides it"""
    return 2 if Bp % 3 == 0 else (1 if Bp % 2 == 0 else 0)


def colstats64_chain(Mp):
    """colstats64_kernel: rows split over min(64, Mp / 64) chunks, 4 row lanes: ceil(per / 4) trips of 3 operations (w w, - a a, +),
    3 additions over the lanes, the atomics of all chunks on one address"""
    splits = max(1, min(64, Mp // 64))
    per = (Mp + splits - 1) // splits
    return 3 * ((per + 3) // 4) + 3 + splits


def cols64_chain(ncols):
    """likelihood64_kernel / fast_tail64_kernel: ceil(ncols / (256 blocks)) trips (blocks <= 256) of one addition, on a per-column value of
    up to 12 roundings; 6 shuffle steps, 3 additions over the waves, the atomics of all blocks; then (fast tail) the 16 of FIN_CHAIN"""
    blocks = min(256, (ncols + 255) // 256)
    return (ncols + 256 * blocks - 1) // (256 * blocks) + 12 + 6 + 3 + blocks + FIN_CHAIN


# ---------------------------------------------------------------------------------------------------------------- g. ciq
CIQ_SHAPES = ((1, 1, 0), (6, 5, 2), (12, 255, 3), (9, 256, 2), (10, 257, 4), (4, 1000, 1))
CIQ_JITTERS = (0.0, 1e-4)
CIQ_HYP = (0.8, 1.4, 0.05, 0.0)


def ciq_clamp_rows(t):
    return sorted({0, t - 1}) if t < 3 else [1, t - 1]


def ciq_inputs(t, n, p, jitter, single):
    """T, ST [t, n]; two rows (one if t < 3) engineered to clamp: ST = 0 there, so var = s dg + jitter - |T_j|^2 < 0"""
    g = torch.Generator().manual_seed(7000 + 31 * t + n)
    rnd = r32 if single else (lambda x: x)
    mag = lambda *s: (0.5 + torch.rand(*s, generator=g, dtype=f64)) * (2.0 * torch.randint(0, 2, s, generator=g).to(f64) - 1.0)
    T = rnd(mag(t, n) / math.sqrt(n))                # |T_j|^2 in [0.25, 2.25]
    ST = rnd(T * (1.5 + torch.rand(t, n, generator=g, dtype=f64)))     # ivar_j >= 1.5 |T_j|^2: the unclamped rows are far from the clamp
    clamp = ciq_clamp_rows(t)
    for j in clamp:
        T[j] = rnd(3.0 * T[j])                       # |T_j|^2 >= 2.25 > s / ell^2 + jitter = 2.1876
        ST[j] = 0.0
    return dict(T=T, ST=ST, m=rnd(mag(n)), c=rnd(torch.tensor([0.3], dtype=f64)), hyp=rnd(torch.tensor(CIQ_HYP, dtype=f64)),
                mu_bar=rnd(mag(t)), var_bar=rnd(mag(t)), p=p, jitter=jitter, clamp=clamp)


def ciq_rowstats_ref(inp, broken=None):
    """imean = T_j . m, mu = imean + c, var = max(s dg_j + jitter - |T_j|^2 + (ST)_j . T_j, 1e-6), live = var not clamped"""
    T, ST = V(inp["T"]), V(inp["ST"])
    t, n = T.v.shape
    cs_ = kept(n, broken)
    ell, s = V(inp["hyp"][0]), V(inp["hyp"][1])
    one = V(torch.ones(t, dtype=f64))
    isf = (torch.arange(t) % (inp["p"] + 1)) == 0
    dg = (s * one).where(isf, s / (ell * ell) * one)
    imean = (T * V(inp["m"])[None, :])[:, cs_].sum(1)
    v = dg + float(inp["jitter"]) - (T * T)[:, cs_].sum(1) + (ST * T)[:, cs_].sum(1)
    live = v.v > O.MIN_VARIANCE
    return dict(imean=imean, mu=imean + V(inp["c"])[0], var=v.where(live, O.MIN_VARIANCE), live=live.to(f64))


def ciq_tbar_ref(inp, live, imean):
    """Tbar = 2 vbar (ST - T) + mu_bar m^T, VT = vbar T, cvec = mu_bar - 2 vbar imean, vbar = var_bar live"""
    vb = V(inp["var_bar"] * live)
    mb = V(inp["mu_bar"])
    T, ST = V(inp["T"]), V(inp["ST"])
    return dict(Tbar=2.0 * vb[:, None] * (ST - T) + mb[:, None] * V(inp["m"])[None, :], VT=vb[:, None] * T,
                cvec=mb - 2.0 * vb * V(imean))


def ciq_chain(n):
    """ciq_rowstats_kernel accumulates in double whatever the type: ceil(n / 256) trips, 6 shuffle steps, 3 additions over the waves, then
    dg + jitter - tsq + ivar (3) and the rounding to the output type (1): counted in units of the output type's u it is generous"""
    return (n + 255) // 256 + 6 + 3 + 3 + 1


# ---------------------------------------------------------------------------------------------------------------- h / i
HELPER_NS = (1, 31, 32, 33, 64, 97)
ADAM_SIZES = (1, 0, 257, 2048 * 256 + 5)
ADAM_HP = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)


def adam_ref(p, g, m, v, step, hp=None):
    """one torch.optim.Adam step (single-tensor rule) on V objects: returns (param, exp_avg, exp_avg_sq)"""
    hp = hp or {k: float(torch.tensor(x, dtype=torch.float32)) for k, x in ADAM_HP.items()}
    b1, b2 = hp["beta1"], hp["beta2"]
    m = b1 * V.of(m) + (1.0 - b1) * V(g)
    v = b2 * V.of(v) + (1.0 - b2) * V(g) * V(g)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    sq = V(v.v.sqrt(), v.a / v.v.sqrt().clamp_min(1e-300))
    denom = sq / math.sqrt(bc2) + hp["eps"]
    return V.of(p) - (hp["lr"] / bc1) * (m / denom), m, v


# ---------------------------------------------------------------------------------------------------------------- bounds per family
def ls_bounds(ref, Mp):
    c = ls_chain(Mp)
    return {k: bound_elem(v.a, U32) if k in ("d_LS", "d_m") else bound_sum(v.a, U32, c) for k, v in ref.items()}


def res_bounds(ref, ncols, deterministic=False):
    c = res_chain(ncols, deterministic)
    return {k: bound_elem(v.a, U32) if k == "mu_bar" else bound_sum(v.a, U32, c) for k, v in ref.items()}


def trace_bounds(ref, n):
    return {k: bound_sum(v.a, U32, trace_chain(n)) for k, v in ref.items()}


def fin_bounds(ref):
    return bound_sum(ref.a, U32, FIN_CHAIN)
