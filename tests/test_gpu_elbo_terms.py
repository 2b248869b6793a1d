"""Term-level tests of the ELBO scalar and reduction kernels against tests/_elbo_terms_ref.py (float64, with the sum of the absolute
values of every output's addends).  The only tolerances are that file's two bound helpers -- ``check`` asserts err <= bound -- and
bitwise comparisons.  Inputs are float32-rounded first and widened for the reference; "poison" is NaN / Inf in memory a kernel must
not use.  Each test records max(err / bound) per output; the table is printed when the module is done and written as JSON to the
file named by DSVGP_ELBO_TERMS_REPORT, if that is set."""
import json
import math
import os

import pytest
import torch

import _elbo_terms_ref as R
from _elbo_terms_ref import U32, U64, V, bound_elem, bound_sum

pytestmark = pytest.mark.gpu

f32, f64 = torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    rows = ["%-28s %-10s %.3f" % (op, out, r) for op in sorted(REPORT) for out, r in sorted(REPORT[op].items())]
    print("\nmax(err / bound) per op and output\n" + "\n".join(rows))
    path = os.environ.get("DSVGP_ELBO_TERMS_REPORT")
    if path:
        with open(path, "w") as fh:
            json.dump(REPORT, fh, indent=1, sort_keys=True)


def check(op, out, got, ref, bound):
    r = R.ratio(got, ref, bound)
    REPORT.setdefault(op, {})
    REPORT[op][out] = max(REPORT[op].get(out, 0.0), r)
    print("%s %s err/bound %.3f" % (op, out, r))
    assert r <= 1.0, (op, out, r)


def bits(t):
    """the bit pattern of a float tensor (a copy), for "bitwise untouched" """
    return t.detach().contiguous().view(torch.int32 if t.dtype == f32 else torch.int64).clone()


def padded(vals, ld, dev, fill=NAN, dtype=f32):
    """vals [r, c] as a view with leading dimension ld of a buffer filled with ``fill``;
    returns (view, the [r, ld] view that holds the padding too)"""
    r, c = vals.shape
    full = torch.full((r, ld), fill, dtype=dtype, device=dev)
    full[:, :c].copy_(vals.to(dtype))
    return full[:, :c], full


def dev32(x, dev):
    return x.to(f32).to(dev)


def hyp32(dev, ell, s, noise):
    return torch.tensor([ell, s, noise, 0.0], dtype=f32, device=dev)


@pytest.fixture(scope="module")
def ops_ctx(dsvgp, gpu_device):
    ops = dsvgp._ops
    return ops, ops.Context.get(gpu_device), gpu_device


# ------------------------------------------------------------------------------------------------------------------ a. ls_rows
_LS_INP, _LS_REF = {}, {}


def _ls_ref(Mp, scale, add_kl):
    """computed once per (Mp, flags), shared by the layouts"""
    key = (Mp, scale, add_kl)
    if Mp not in _LS_INP:
        _LS_INP[Mp] = R.ls_inputs(Mp)
    if key not in _LS_REF:
        _LS_REF[key] = R.ls_rows_ref(_LS_INP[Mp], scale, add_kl)
    return _LS_INP[Mp], _LS_REF[key]


@pytest.mark.parametrize("Mp,layout", R.LS_CASES)
def test_ls_rows_family(ops_ctx, Mp, layout):
    # c = ceil(Mp / 64) + 3 (a lane's fma chain, scalar or 16-byte kernel) + 6 (shuffle steps) + 4 (the per-row value) + 1 (the rounding of
    #     the fixed-order double sum) + 1 (t1_scale): R.ls_chain; no atomics.  d_LS and d_m are elementwise outputs.
    ops, ctx, dev = ops_ctx
    ld = {"contiguous": Mp, "ld+4": Mp + 4, "ld+1": Mp + 1}[layout]
    up = torch.ones(Mp, Mp, dtype=torch.bool).triu(1)
    for op, scale, add_kl in R.LS_OPS:
        inp, ref = _ls_ref(Mp, scale, add_kl)
        b = R.ls_bounds(ref, Mp)
        L, Lfull = padded(torch.where(up, torch.full_like(inp["L"], NAN), inp["L"]), ld, dev)
        D, Dfull = padded(torch.where(up, torch.full_like(inp["T"], INF), inp["T"]), ld, dev)
        vec = Mp % 4 == 0 and ld % 4 == 0 and L.data_ptr() % 16 == 0 and D.data_ptr() % 16 == 0
        assert vec == (Mp % 4 == 0 and layout != "ld+1")                        # the layout reaches the kernel it is meant for
        G, _ = padded(torch.where(torch.eye(Mp, dtype=torch.bool), torch.diag(inp["Gd"]), torch.full((Mp, Mp), NAN, dtype=f64)), Mp + 2, dev)
        L0, D0 = bits(Lfull), bits(Dfull)
        m, dm = dev32(inp["m"], dev), dev32(inp["dm0"], dev)
        dm0 = bits(dm)
        hyp = hyp32(dev, 0.9, 1.1, R.LS_NOISE)
        kl_buf = torch.full((1 + 2 * Mp,), 123.0, dtype=f32, device=dev)
        sums = torch.tensor([11.5, -7.25, NAN, NAN], dtype=f32, device=dev)
        s0 = bits(sums)
        name = "%s(scale=%d,kl=%d)" % (op, scale, add_kl)
        if op == "kl_terms":
            ops.kl_terms(ctx, m, L, R.LS_NUM_DATA, kl_buf, dm, D)
        elif op == "kl_terms_scaled":
            ops.kl_terms_scaled(ctx, m, L, R.LS_NUM_DATA, add_kl, hyp, R.LS_ROWS, kl_buf, dm, D)
        else:
            ops.variational_terms(ctx, m, L, R.LS_NUM_DATA, scale, add_kl, hyp, R.LS_ROWS, G, R.LS_T1_SCALE, kl_buf, sums, dm, D)
        torch.cuda.synchronize()
        assert torch.equal(bits(Lfull), L0), name                                   # L_S is read only
        assert torch.equal(bits(Dfull)[:, Mp:], D0[:, Mp:]), name                   # the padding is bitwise untouched
        out = D.cpu()
        assert bool((out[up] == 0).all()), name                                     # the strict upper triangle is exactly 0
        assert bool(torch.isfinite(out).all()), name
        check(name, "d_LS", out, ref["d_LS"], b["d_LS"])
        if add_kl:
            check(name, "d_m", dm, ref["d_m"], b["d_m"])
            check(name, "kl", kl_buf[0], ref["kl"], b["kl"])
        else:
            assert torch.equal(bits(dm), dm0), name
            assert bits(kl_buf[:1]).item() == 0, name                               # exactly +0
        if op == "variational_terms":
            assert torch.equal(bits(sums)[:2], s0[:2]), name
            check(name, "sums2", sums[2], ref["sums2"], b["sums2"])
            check(name, "sums3", sums[3], ref["sums3"], b["sums3"])
        else:
            assert torch.equal(bits(sums), s0), name


def test_kl_terms_scaled_more_rows_than_waves(ops_ctx):
    """Mp = 8196: rows outnumber the 2048 x 4 waves of the grid, rows 8192.. are a wave's second trip.  The float64 reference of this one
    case is evaluated with torch on the device (inputs drawn there by the rule of R.draw / R.draw_diag)."""
    # c = ceil(8196 / 64) + 3 + 6 + 4 + 1 + 1 (R.ls_chain)
    ops, ctx, dev = ops_ctx
    Mp = R.LS_BIG_MP
    g = torch.Generator(device=dev).manual_seed(Mp)
    mag = lambda *s: (0.5 + torch.rand(*s, generator=g, device=dev, dtype=f32)) * (2.0 * torch.randint(0, 2, s, generator=g, device=dev).to(f32) - 1.0)
    L, T, m, dm = mag(Mp, Mp), mag(Mp, Mp), mag(Mp), mag(Mp)
    u = torch.rand(Mp, generator=g, device=dev, dtype=f32)
    L.diagonal().copy_(torch.where(u < 0.5, 0.5 + 0.5 * u, 1.0 + 0.5 * u))
    low = torch.ones(Mp, Mp, dtype=torch.bool, device=dev).tril()
    hyp = hyp32(dev, 0.9, 1.1, R.LS_NOISE)
    sc = 1.0 / (hyp[2].double() * R.LS_ROWS)
    L6 = torch.where(low, L.double(), torch.zeros((), dtype=f64, device=dev))
    inv_d = torch.diag(1.0 / L.diagonal().double())
    ref_d = torch.where(low, T.double() * sc, torch.zeros((), dtype=f64, device=dev)) + (L6 - inv_d) / R.LS_NUM_DATA
    a_d = torch.where(low, T.double().abs() * sc, torch.zeros((), dtype=f64, device=dev)) + (L6.abs() + inv_d) / R.LS_NUM_DATA
    ld2 = torch.log(L.diagonal().double() ** 2)
    kl = V(0.5 * ((m.double() ** 2).sum() + (L6 * L6).sum() - Mp - ld2.sum()),
           0.5 * ((m.double() ** 2).sum() + (L6 * L6).sum() + Mp + (1.0 + R.FN_ULP) * ld2.abs().sum() + Mp))
    ref_m = V(dm.double() + m.double() / R.LS_NUM_DATA, dm.double().abs() + m.double().abs() / R.LS_NUM_DATA)
    # the sensitivity condition of tests/test_elbo_terms_host.py, on the inputs drawn here: the last row left out of the KL sum is more than
    # ten bounds away (the diagonal and scaling conditions on d_LS are elementwise and hold by the drawn ranges, as at every other Mp)
    last_row = 0.5 * (m.double()[-1] ** 2 + (L6[-1] ** 2).sum() - 1.0 - ld2[-1])
    assert float(last_row.abs()) > 10.0 * float(bound_sum(kl.a, U32, R.ls_chain(Mp)))
    del L6, inv_d
    L.masked_fill_(~low, NAN)
    T.masked_fill_(~low, INF)
    kl_buf = torch.zeros(1 + Mp, dtype=f32, device=dev)
    ops.kl_terms_scaled(ctx, m, L, R.LS_NUM_DATA, 1, hyp, R.LS_ROWS, kl_buf, dm, T)
    torch.cuda.synchronize()
    assert bool((T[~low] == 0).all())
    err = (T.double() - ref_d).abs()
    r = float(torch.where(err == 0, err, err / bound_elem(a_d, U32)).max())
    assert math.isfinite(r)
    REPORT.setdefault("kl_terms_scaled(Mp=8196)", {})["d_LS"] = r
    assert r <= 1.0, r
    check("kl_terms_scaled(Mp=8196)", "d_m", dm, V(ref_m.v.cpu(), ref_m.a.cpu()), bound_elem(ref_m.a.cpu(), U32))
    check("kl_terms_scaled(Mp=8196)", "kl", kl_buf[0], V(kl.v.cpu(), kl.a.cpu()), bound_sum(kl.a.cpu(), U32, R.ls_chain(Mp)))


# ------------------------------------------------------------------------------------------------------------------ b. residual_terms
@pytest.mark.parametrize("ncols", R.RES_NCOLS)
def test_residual_terms(ops_ctx, ncols):
    # c = ceil(ncols / (256 blocks)) (a lane's loop, blocks = min(512, ceil(ncols / 256))) + 6 (shuffle steps) + 3 (the 4 waves) + blocks (the
    #     atomics of every workgroup on one address); deterministic mode: ... + 1 (the rounding of the double sum of the partials): R.res_chain
    ops, ctx, dev = ops_ctx
    inp = R.res_inputs(ncols)
    ref = R.residual_ref(inp)
    mu, y = dev32(inp["mu"], dev), dev32(inp["y"], dev)
    hyp = hyp32(dev, 0.9, 1.1, R.RES_NOISE)

    def run():
        mb = torch.full((ncols,), NAN, dtype=f32, device=dev)
        sums = torch.tensor([3e7, -4e-3, NAN, INF], dtype=f32, device=dev)              # garbage: the call zeroes all four
        ops.residual_terms(ctx, mu, y, hyp, inp["rows"], mb, sums)
        torch.cuda.synchronize()
        return mb, sums

    mb, sums = run()
    b = R.res_bounds(ref, ncols)
    assert bits(sums[2:]).tolist() == [0, 0]
    check("residual_terms", "mu_bar", mb, ref["mu_bar"], b["mu_bar"])
    check("residual_terms", "sums0", sums[0], ref["sums0"], b["sums0"])
    check("residual_terms", "sums1", sums[1], ref["sums1"], b["sums1"])
    scratch = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    ctx.set_deterministic(scratch)
    try:
        mb1, s1 = run()
        mb2, s2 = run()
    finally:
        ctx.set_deterministic(None)
    b = R.res_bounds(ref, ncols, deterministic=True)
    assert torch.equal(bits(s1), bits(s2)) and torch.equal(bits(mb1), bits(mb2))
    assert bits(s1[2:]).tolist() == [0, 0]
    check("residual_terms(det)", "mu_bar", mb1, ref["mu_bar"], b["mu_bar"])
    check("residual_terms(det)", "sums0", s1[0], ref["sums0"], b["sums0"])
    check("residual_terms(det)", "sums1", s1[1], ref["sums1"], b["sums1"])


# ------------------------------------------------------------------------------------------------------------------ c. trace_terms
@pytest.mark.parametrize("n", R.TRACE_NS)
def test_trace_terms(ops_ctx, n):
    # c = ceil(n / grid) ceil(n / 256) (a thread's fma chain over its workgroup's rows, grid = min(n, 1024)) + 6 (shuffle steps) + 3 (the 4
    #     waves) + 1 (t1_scale) + grid + 1 (the atomics of every workgroup and the earlier content of sums on one address): R.trace_chain
    ops, ctx, dev = ops_ctx
    inp = R.trace_inputs(n)
    ref = R.trace_ref(inp)
    b = R.trace_bounds(ref, n)
    up = torch.ones(n, n, dtype=torch.bool).triu(1)
    L, Lf = padded(torch.where(up, torch.full_like(inp["L"], NAN), inp["L"]), n + 1, dev)
    T, Tf = padded(torch.where(up, torch.full_like(inp["T"], NAN), inp["T"]), n + 2, dev)
    G, Gf = padded(torch.where(torch.eye(n, dtype=torch.bool), torch.diag(inp["Gd"]), torch.full((n, n), NAN, dtype=f64)), n + 3, dev)
    before = [bits(x) for x in (Lf, Tf, Gf)]
    sums = torch.tensor([11.5, -7.25, R.TRACE_PRE[0], R.TRACE_PRE[1]], dtype=f32, device=dev)
    s0 = bits(sums)
    ops.trace_terms(ctx, L, T, G, n, sums, R.LS_T1_SCALE)
    torch.cuda.synchronize()
    for x, x0 in zip((Lf, Tf, Gf), before):
        assert torch.equal(bits(x), x0)
    assert torch.equal(bits(sums)[:2], s0[:2])
    check("trace_terms", "sums2", sums[2], ref["sums2"], b["sums2"])
    check("trace_terms", "sums3", sums[3], ref["sums3"], b["sums3"])


# ------------------------------------------------------------------------------------------------------------------ d. scalar tails
@pytest.mark.parametrize("npts,p", R.FIN_SHAPES)
@pytest.mark.parametrize("hyp", R.FIN_HYPS)
def test_elbo_fast_finalize(ops_ctx, npts, p, hyp):
    # c = 16: the roundings of scal[0], the longest chain of elbo_fast_finalize_body (R.FIN_CHAIN lists them); one thread, no reduction
    ops, ctx, dev = ops_ctx
    inp = R.fin_inputs(npts, p, hyp)
    ref = R.finalize_ref(inp)
    scal = torch.full((8,), NAN, dtype=f32, device=dev)
    ops.elbo_fast_finalize(ctx, dev32(inp["sums"], dev), dev32(inp["hyp"], dev), npts, p, inp["rows"], scal)
    torch.cuda.synchronize()
    check("elbo_fast_finalize", "scal0-4", scal[:5], ref, R.fin_bounds(ref))
    assert bits(scal[5:]).tolist() == [0, 0, 0]


def test_step_epilogue_and_hyp_backward(ops_ctx):
    # elementwise: the longest value, d_raw, passes an addition, the exponential (its 4 ulp are in the addends), 1 + e, the quotient and one fma
    ops, ctx, dev = ops_ctx
    inp = R.epilogue_inputs()
    ref = R.epilogue_ref(inp)
    raw = [dev32(inp["raw"][k:k + 1], dev) for k in range(3)]
    d_hyp, d_const = dev32(inp["d_hyp"], dev), dev32(inp["d_const"], dev)
    d_raw = [dev32(inp["d_raw"][k:k + 1], dev) for k in range(3)]
    loss = torch.full((1,), NAN, dtype=f32, device=dev)
    ops.step_epilogue(ctx, dev32(inp["scal"], dev), dev32(inp["kl0"], dev), inp["rows"], inp["num_data"], raw[0], raw[1], raw[2], d_hyp,
                      d_raw[0], d_raw[1], d_raw[2], d_const, loss)
    torch.cuda.synchronize()
    check("step_epilogue", "d_hyp", d_hyp[:3], ref["d_hyp"], bound_elem(ref["d_hyp"].a, U32))
    assert bits(d_hyp[3:]).item() == bits(dev32(inp["d_hyp"][3:], dev)).item()
    check("step_epilogue", "d_raw", torch.cat(d_raw), ref["d_raw"], bound_elem(ref["d_raw"].a, U32))
    check("step_epilogue", "d_const", d_const[0], ref["d_const"], bound_elem(ref["d_const"].a, U32))
    check("step_epilogue", "loss", loss[0], ref["loss"], bound_elem(ref["loss"].a, U32))
    refb = R.hyp_backward_ref(inp)
    d_hyp = dev32(inp["d_hyp"], dev)
    d_raw = [dev32(inp["d_raw"][k:k + 1], dev) for k in range(3)]
    h0 = bits(d_hyp)
    ops.hyp_backward(ctx, raw[0], raw[1], raw[2], d_hyp, d_raw[0], d_raw[1], d_raw[2])
    torch.cuda.synchronize()
    assert torch.equal(bits(d_hyp), h0)
    check("hyp_backward", "d_raw", torch.cat(d_raw), refb, bound_elem(refb.a, U32))


@pytest.mark.parametrize("sizes", R.SCALE_SIZES)
def test_scale_by_vbar(ops_ctx, sizes):
    # elementwise: (float)(1 / rows), the division by the noise, one product
    ops, ctx, dev = ops_ctx
    g = torch.Generator().manual_seed(5)
    hyp = hyp32(dev, 0.9, 1.1, R.RES_NOISE)
    xs = [None if n is None else R.draw(g, n) for n in sizes]
    ts = [None if x is None else dev32(x, dev) for x in xs]
    ops.scale_by_vbar_(ctx, ts, hyp, 391.0)
    torch.cuda.synchronize()
    for x, t in zip(xs, ts):
        if x is not None:
            ref = R.scale_ref(x, hyp[2].double().cpu(), 391.0)
            check("scale_by_vbar_", "x", t, ref, bound_elem(ref.a, U32))
    with pytest.raises(ValueError):
        ops.scale_by_vbar_(ctx, [dev32(R.draw(g, 2), dev) for _ in range(4)], hyp, 391.0)


# ------------------------------------------------------------------------------------------------------------------ e. fast path against general path
@pytest.mark.parametrize("Mp", R.E_MPS)
def test_fast_path_and_general_path_meet_one_reference(ops_ctx, Mp):
    # general: c = 3 Mp + 4 + 12 + 1 + 6 + 3 + 1 + 2 (R.e_chain_general lists the terms)
    # fast:    c = Mp + 2 + R.res_chain(51) or R.ls_chain(Mp), whichever is longer, + 16 (R.FIN_CHAIN) + 2 (R.e_chain_fast)
    ops, ctx, dev = ops_ctx
    B, p = R.E_B, R.E_P
    Bp = B * (p + 1)
    inp = R.e_inputs(Mp)
    A, L, m, y, c, hyp, rows = (inp[k] for k in ("A", "L", "m", "y", "c", "hyp", "rows"))
    W = L.t() @ A
    mu0, cs = R.colstats_ref(A, W, m)
    ref = R.likelihood_ref(mu0, cs, y, c, p, hyp, 0, rows)
    c_gen, c_fast = R.e_chain_general(Mp), R.e_chain_fast(Mp)
    Ad, md, yd, cd, hd = dev32(A, dev), dev32(m, dev), dev32(y, dev), dev32(c, dev), dev32(hyp, dev)
    # general path
    mu, var = torch.empty(Bp, dtype=f32, device=dev), torch.empty(Bp, dtype=f32, device=dev)
    ops.predictive_stats(ctx, Ad, dev32(W, dev), p, md, cd, hd, mu, var)
    mb, vb, vn = (torch.empty(Bp, dtype=f32, device=dev) for _ in range(3))
    scal = torch.empty(8, dtype=f32, device=dev)
    ops.likelihood_terms(ctx, mu, var, yd, p, hd, 0, rows, mb, vb, vn, scal)
    torch.cuda.synchronize()
    check("general path", "scal0-4", scal[:5], ref["scal"], bound_sum(ref["scal"].a, U32, c_gen))
    check("general path", "mu_bar", mb, ref["mu_bar"], bound_sum(ref["mu_bar"].a, U32, Mp + 4))     # (mu_j: Mp fmas, + c, y -, / noise, / rows)
    # fast path: mu from the same column pass with W = A, G and T formed in float64 and rounded once
    G = A @ A.t()
    T = torch.tril(G @ L)
    mu2, var2 = torch.empty(Bp, dtype=f32, device=dev), torch.empty(Bp, dtype=f32, device=dev)
    ops.predictive_stats(ctx, Ad, Ad, p, md, cd, hd, mu2, var2)
    mb2 = torch.empty(Bp, dtype=f32, device=dev)
    sums = torch.full((4,), NAN, dtype=f32, device=dev)
    ops.residual_terms(ctx, mu2, yd, hd, rows, mb2, sums)
    kl_buf = torch.zeros(1 + 2 * Mp, dtype=f32, device=dev)
    dm, dLS = torch.zeros(Mp, dtype=f32, device=dev), dev32(T, dev)
    ops.variational_terms(ctx, md, dev32(L, dev), 57.0, 1, 0, hd, rows, dev32(G, dev), 1.0, kl_buf, sums, dm, dLS)
    scal2 = torch.empty(8, dtype=f32, device=dev)
    ops.elbo_fast_finalize(ctx, sums, hd, B, p, rows, scal2)
    torch.cuda.synchronize()
    # the same reference values; the bound from the fast path's own addends (sum |L_ij T_ij| and trace(G) in the place of sum w^2 + a^2)
    res = R.residual_ref(dict(mu=mu0 + V(c)[0], y=y, noise=hyp[2], rows=rows))
    var = R.ls_rows_ref(dict(m=m, L=L, T=T, dm0=m, Gd=G.diagonal().clone(), noise=hyp[2]), 1, 0, num_data=57.0, rows=rows, t1_scale=1.0)
    fast = R.fast_scalars(res["sums0"], res["sums1"], var["sums2"], var["sums3"], hyp, B, p, rows)
    check("fast path", "scal0-4", scal2[:5], ref["scal"], bound_sum(fast.a, U32, c_fast))
    check("fast path", "mu_bar", mb2, ref["mu_bar"], bound_sum(ref["mu_bar"].a, U32, Mp + 4))


# ------------------------------------------------------------------------------------------------------------------ f. float64 tails
@pytest.mark.parametrize("Mp", R.F64_MPS)
@pytest.mark.parametrize("Bp", R.F64_BPS)
def test_float64_tails(ops_ctx, Mp, Bp):
    # colstats_f64: c = 3 ceil(per / 4) + 3 + splits (R.colstats64_chain: 4 row lanes, 3 operations a row, the atomics of the row chunks)
    # likelihood_terms_f64 / elbo_fast_tail_f64 scalars: c = ceil(ncols / (256 blocks)) + 12 + 6 + 3 + blocks + 16 (R.cols64_chain);
    #     their per-column outputs and abar_f64 are elementwise
    ops, ctx, dev = ops_ctx
    inp = R.f64_inputs(Mp, Bp)
    p = R.f64_p(Bp)
    d = lambda x: x.to(dev)
    A = padded(inp["A"], Bp + 3, dev, dtype=f64)[0]
    W = padded(inp["W"], Bp + 1, dev, dtype=f64)[0]
    mu0r, csr = R.colstats_ref(inp["A"], inp["W"], inp["m"])
    c = R.colstats64_chain(Mp)
    mu0, cs = ops.colstats_f64(ctx, A, W, d(inp["m"]))
    mu0b, cs_none = ops.colstats_f64(ctx, A, None, d(inp["m"]))
    torch.cuda.synchronize()
    assert cs_none is None
    check("colstats_f64", "mu0", mu0, mu0r, bound_sum(mu0r.a, U64, c))
    check("colstats_f64", "cs", cs, csr, bound_sum(csr.a, U64, c))
    check("colstats_f64(W=None)", "mu0", mu0b, mu0r, bound_sum(mu0r.a, U64, c))
    # abar_f64
    for U in (inp["U"], None):
        for want_av in (True, False):
            Ab, Abf = padded(torch.zeros(Mp, Bp, dtype=f64), Bp + 2, dev, dtype=f64)
            Av, Avf = padded(torch.zeros(Mp, Bp, dtype=f64), Bp + 5, dev, dtype=f64)
            b0, v0 = bits(Abf), bits(Avf)
            ops.abar_f64(ctx, A, None if U is None else padded(U, Bp + 4, dev, dtype=f64)[0], d(inp["m"]), d(inp["mu_bar"]), d(inp["var_bar"]),
                         Ab, Av if want_av else None)
            torch.cuda.synchronize()
            abr, avr = R.abar_ref(inp["A"], U, inp["m"], inp["mu_bar"], inp["var_bar"])
            assert torch.equal(bits(Abf)[:, Bp:], b0[:, Bp:])
            check("abar_f64", "Abar", Ab, abr, bound_elem(abr.a, U64))
            if want_av:
                assert torch.equal(bits(Avf)[:, Bp:], v0[:, Bp:])
                check("abar_f64", "Av", Av, avr, bound_elem(avr.a, U64))
            else:
                assert torch.equal(bits(Avf), v0)
    # likelihood_terms_f64, both objectives, on the reference's (mu0, cs)
    rows = 2.0 * Bp + 1.0
    cc = R.cols64_chain(Bp)
    for mll in (0, 1):
        ref = R.likelihood_ref(mu0r.v, csr.v, inp["y"], inp["c"], p, inp["hyp"], mll, rows)
        mu, varn, mb, vb, scal = ops.likelihood_terms_f64(ctx, d(mu0r.v), d(csr.v), d(inp["y"]), d(inp["c"]), p, d(inp["hyp"]), mll, rows)
        torch.cuda.synchronize()
        name = "likelihood_terms_f64(mll=%d)" % mll
        check(name, "mu", mu, ref["mu"], bound_elem(ref["mu"].a, U64))
        check(name, "varn", varn, ref["varn"], bound_elem(ref["varn"].a, U64))
        check(name, "mu_bar", mb, ref["mu_bar"], bound_elem(ref["mu_bar"].a, U64))
        check(name, "var_bar", vb, ref["var_bar"], bound_elem(ref["var_bar"].a, U64))
        check(name, "scal0-4", scal[:5], ref["scal"], bound_sum(ref["scal"].a, U64, cc))
    # elbo_fast_tail_f64, ncols = npts (p + 1)
    tv = torch.tensor(0.37 * Bp, dtype=f64)
    ref = R.fast_tail64_ref(mu0r.v, inp["y"], inp["c"], Bp // (p + 1), p, inp["hyp"], tv, rows)
    mu, mb, scal = ops.elbo_fast_tail_f64(ctx, d(mu0r.v), d(inp["y"]), d(inp["c"]), Bp // (p + 1), p, d(inp["hyp"]), d(tv), rows)
    torch.cuda.synchronize()
    check("elbo_fast_tail_f64", "mu", mu, ref["mu"], bound_elem(ref["mu"].a, U64))
    check("elbo_fast_tail_f64", "mu_bar", mb, ref["mu_bar"], bound_elem(ref["mu_bar"].a, U64))
    check("elbo_fast_tail_f64", "scal0-7", scal, ref["scal"], bound_sum(ref["scal"].a, U64, cc))


@pytest.mark.parametrize("mll", [0, 1])
def test_likelihood_terms_f64_at_the_variance_clamp(ops_ctx, mll):
    """one column with cs negative enough that varn = 1e-6: value and gradient as autograd through the oracle's clamp_min gives them
    (tests/test_elbo_terms_host.py holds the reference to that)"""
    # c as in test_float64_tails
    ops, ctx, dev = ops_ctx
    inp = R.f64_inputs(7, 6)
    mu0, cs = R.colstats_ref(inp["A"], inp["W"], inp["m"])
    csv = cs.v.clone()
    csv[4] = -5.0
    ref = R.likelihood_ref(mu0.v, csv, inp["y"], inp["c"], 2, inp["hyp"], mll, 13.0)
    d = lambda x: x.to(dev)
    mu, varn, mb, vb, scal = ops.likelihood_terms_f64(ctx, d(mu0.v), d(csv), d(inp["y"]), d(inp["c"]), 2, d(inp["hyp"]), mll, 13.0)
    torch.cuda.synchronize()
    assert varn[4].item() == 1e-6 and vb[4].item() == 0.0            # (a zero of either sign: -0 * 1 / rows)
    name = "likelihood_terms_f64(clamp,mll=%d)" % mll
    check(name, "varn", varn, ref["varn"], bound_elem(ref["varn"].a, U64))
    check(name, "mu_bar", mb, ref["mu_bar"], bound_elem(ref["mu_bar"].a, U64))
    check(name, "var_bar", vb, ref["var_bar"], bound_elem(ref["var_bar"].a, U64))
    check(name, "scal0-4", scal[:5], ref["scal"], bound_sum(ref["scal"].a, U64, R.cols64_chain(6)))


# ------------------------------------------------------------------------------------------------------------------ g. ciq row statistics
@pytest.mark.parametrize("t,n,p", R.CIQ_SHAPES)
@pytest.mark.parametrize("jitter", R.CIQ_JITTERS)
@pytest.mark.parametrize("single", [True, False], ids=["float", "double"])
def test_ciq_rowstats_and_tbar(ops_ctx, t, n, p, jitter, single):
    # c = ceil(n / 256) + 6 + 3 (a row's workgroup: loop, shuffles, waves -- accumulated in double for either type) + 3 (dg + jitter - tsq + ivar)
    #     + 1 (the rounding to the output type): R.ciq_chain.  Tbar, VT, cvec are elementwise.
    ops, ctx, dev = ops_ctx
    dt, u = (f32, U32) if single else (f64, U64)
    inp = R.ciq_inputs(t, n, p, jitter, single)
    ref = R.ciq_rowstats_ref(inp)
    d = lambda x: x.to(dt).to(dev).contiguous()
    T, ST, m = d(inp["T"]), d(inp["ST"]), d(inp["m"])
    imean, mu, var, live = ops.ciq_rowstats(ctx, T, ST, p, m, d(inp["c"]), d(inp["hyp"]), jitter)
    torch.cuda.synchronize()
    c = R.ciq_chain(n)
    name = "ciq_rowstats(%s)" % ("float" if single else "double")
    check(name, "imean", imean, ref["imean"], bound_sum(ref["imean"].a, u, c))
    check(name, "mu", mu, ref["mu"], bound_sum(ref["mu"].a, u, c))
    check(name, "var", var, ref["var"], bound_sum(ref["var"].a, u, c))
    assert torch.equal(live.cpu().double(), ref["live"])
    clamp = inp["clamp"]
    one_e6 = torch.tensor(1e-6, dtype=dt)
    for j in clamp:
        assert var[j].cpu() == one_e6 and live[j].item() == 0.0
    mu_bar, var_bar = d(inp["mu_bar"]), d(inp["var_bar"])
    Tbar, VT = torch.full((t, n), NAN, dtype=dt, device=dev), torch.full((t, n), NAN, dtype=dt, device=dev)
    cvec = ops.ciq_tbar(ctx, T, ST, m, mu_bar, var_bar, live, imean, Tbar, VT)
    torch.cuda.synchronize()
    tb = R.ciq_tbar_ref(inp, ref["live"], imean.cpu().double())
    name = "ciq_tbar(%s)" % ("float" if single else "double")
    check(name, "Tbar", Tbar, tb["Tbar"], bound_elem(tb["Tbar"].a, u))
    check(name, "VT", VT, tb["VT"], bound_elem(tb["VT"].a, u))
    check(name, "cvec", cvec, tb["cvec"], bound_elem(tb["cvec"].a, u))
    for j in clamp:
        assert torch.equal(Tbar[j].cpu(), (mu_bar[j] * m).cpu())          # exactly mu_bar_j m: one correctly rounded product
        assert bool((VT[j] == 0).all())
        assert cvec[j].item() == mu_bar[j].item()


# ------------------------------------------------------------------------------------------------------------------ h. in-place matrix helpers
@pytest.mark.parametrize("n", R.HELPER_NS)
def test_matrix_helpers_are_bitwise_exact(ops_ctx, n):
    # no sum and no bound: copies, one correctly rounded addition, and averages that are exact in float
    ops, ctx, dev = ops_ctx
    g = torch.Generator().manual_seed(n)
    X = R.draw(g, n, n)
    low = torch.ones(n, n, dtype=torch.bool).tril()
    # mirror_lower_f32_: garbage above the diagonal is replaced by the transposed lower triangle
    Gv, Gf = padded(torch.where(low, X, torch.full_like(X, NAN)), n + 3, dev)
    g0 = bits(Gf)
    ops.mirror_lower_f32_(ctx, Gv, n)
    torch.cuda.synchronize()
    g1 = bits(Gf)
    assert torch.equal(g1[:, n:], g0[:, n:])
    assert torch.equal(g1[:, :n][low.to(dev)], g0[:, :n][low.to(dev)])
    assert torch.equal(g1[:, :n], torch.where(low.to(dev), g0[:, :n], g0[:, :n].t()))
    # add_diag_f32_: one correctly rounded addition on the diagonal, nothing else
    Av, Af = padded(X, n + 3, dev)
    want = X.float()
    want.diagonal().add_(torch.tensor(0.37, dtype=f32))
    a0 = bits(Af)
    ops.add_diag_f32_(ctx, Av, n, 0.37)
    torch.cuda.synchronize()
    a1 = bits(Af)
    off = ~torch.eye(n, dtype=torch.bool, device=dev)
    assert torch.equal(a1[:, n:], a0[:, n:]) and torch.equal(a1[:, :n][off], a0[:, :n][off])
    assert torch.equal(a1[:, :n].diagonal().cpu(), bits(want.diagonal()))
    # sym_average_f32, out of place: small integers and halves average exactly
    H = torch.randint(-8, 9, (n, n), generator=g).to(f64) * 0.5
    Hv, Hf = padded(H, n + 3, dev)
    Ov, Of = padded(torch.zeros(n, n, dtype=f64), n + 1, dev)
    h0, o0 = bits(Hf), bits(Of)
    ops.sym_average_f32(ctx, Hv, Ov)
    torch.cuda.synchronize()
    assert torch.equal(bits(Hf), h0) and torch.equal(bits(Of)[:, n:], o0[:, n:])
    assert torch.equal(Ov.cpu(), (0.5 * (H + H.t())).float())


# ------------------------------------------------------------------------------------------------------------------ i. adam_step_multi_dev_
def _adam_case(ops_ctx, sizes, guard_value):
    # elementwise, no sum: parameters and both moments are held to 8 u of their addends after each of the three steps
    ops, ctx, dev = ops_ctx
    g = torch.Generator().manual_seed(len(sizes))
    hp = {k: float(torch.tensor(x, dtype=f32)) for k, x in R.ADAM_HP.items()}
    p0 = [R.draw(g, n) for n in sizes]
    pt = [x.clone().requires_grad_(True) for x in p0]
    opt = torch.optim.Adam([x for x in pt if x.numel()], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    pd = [dev32(x, dev) for x in p0]
    md, vd = [torch.zeros_like(x) for x in pd], [torch.zeros_like(x) for x in pd]
    ref = [(V(x), V(torch.zeros_like(x)), V(torch.zeros_like(x))) for x in p0]
    guard = None if guard_value is None else torch.tensor([guard_value], dtype=torch.int32, device=dev)
    for step in (1, 2, 3):
        gr = [R.draw(g, n) for n in sizes]
        gd = [dev32(x, dev) for x in gr]
        hp_dev = torch.tensor([hp["lr"], float(step)], dtype=f32, device=dev)
        before = [bits(torch.cat([a.reshape(-1), b.reshape(-1), c.reshape(-1)])) for a, b, c in zip(pd, md, vd)]
        ops.adam_step_multi_dev_(ctx, pd, gd, md, vd, hp_dev, hp["beta1"], hp["beta2"], hp["eps"], guard)
        torch.cuda.synchronize()
        if guard_value:
            for (a, b, c), x0 in zip(zip(pd, md, vd), before):
                assert torch.equal(bits(torch.cat([a.reshape(-1), b.reshape(-1), c.reshape(-1)])), x0)
            continue
        for x, gx in zip(pt, gr):
            x.grad = gx.clone()
        opt.step()
        ref = [R.adam_ref(r[0], gx, r[1], r[2], step, hp) for r, gx in zip(ref, gr)]
        for k, n in enumerate(sizes):
            if n == 0:
                continue
            name = "adam_step_multi_dev_"          # (values: torch.optim.Adam itself; addends: R.adam_ref, held to it by the host file)
            check(name, "param", pd[k], V(pt[k].detach(), ref[k][0].a), bound_elem(ref[k][0].a, U32))
            check(name, "exp_avg", md[k], V(opt.state[pt[k]]["exp_avg"], ref[k][1].a), bound_elem(ref[k][1].a, U32))
            check(name, "exp_avg_sq", vd[k], V(opt.state[pt[k]]["exp_avg_sq"], ref[k][2].a), bound_elem(ref[k][2].a, U32))


@pytest.mark.parametrize("guard_value", [None, 0, 7])
def test_adam_step_multi_dev_against_torch_adam(ops_ctx, guard_value):
    # elementwise (_adam_case); with a non-zero guard parameters and both moments stay bitwise as they were
    _adam_case(ops_ctx, R.ADAM_SIZES, guard_value)


def test_adam_step_multi_dev_sixteen_tensors_and_the_limit(ops_ctx):
    # elementwise (_adam_case)
    ops, ctx, dev = ops_ctx
    _adam_case(ops_ctx, tuple(3 + 5 * k for k in range(16)), None)
    ts = [torch.zeros(2, dtype=f32, device=dev) for _ in range(17)]
    with pytest.raises(ValueError):
        ops.adam_step_multi_dev_(ctx, ts, ts, ts, ts, torch.tensor([0.01, 1.0], dtype=f32, device=dev), 0.9, 0.999, 1e-8)
