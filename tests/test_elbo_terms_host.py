"""tests/_elbo_terms_ref.py kept honest without a GPU: every reference equals float64 autograd through the oracle's own formulas, the
fast path's closed form equals the general path, and on every case of the shared tables a deliberately broken reference differs from
the true one by more than ten times the bound tests/test_gpu_elbo_terms.py applies there."""
import math

import pytest
import torch
import torch.nn.functional as F

import dsvgp_oracle as O
import _elbo_terms_ref as R

f64 = torch.float64


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=f64), torch.as_tensor(b, dtype=f64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def visible(true, broken, bound):
    """max |broken - true| / bound over one output"""
    d = (broken.v - true.v).abs().reshape(-1)
    return float((d / bound.reshape(-1)).max()) if d.numel() else 0.0


# ------------------------------------------------------------------------------------------------ references against the oracle
@pytest.mark.parametrize("Mp", [1, 5, 8, 65])
@pytest.mark.parametrize("scale,add_kl", [(0, 1), (1, 1), (1, 0), (0, 0)])
def test_ls_rows_reference_is_autograd_of_the_oracle_kl(Mp, scale, add_kl):
    inp = R.ls_inputs(Mp)
    ref = R.ls_rows_ref(inp, scale, add_kl)
    m = inp["m"].clone().requires_grad_(True)
    L = inp["L"].clone().requires_grad_(True)
    Lt = torch.tril(L)
    sc = 1.0 / (inp["noise"] * R.LS_ROWS) if scale else 1.0
    # d_LS is the gradient of  sc <T, L_S> + KL / num_data;  d_m that of  <dm0, m> + KL / num_data
    obj = sc * (torch.tril(inp["T"]) * Lt).sum() + (inp["dm0"] * m).sum()
    kl = O.kl_whitened(m, Lt)
    if add_kl:
        obj = obj + kl / R.LS_NUM_DATA
    obj.backward()
    assert rel(ref["d_LS"].v, L.grad) < 1e-12
    assert float(ref["d_LS"].v.triu(1).abs().max()) == 0.0 if Mp > 1 else True
    if add_kl:
        assert rel(ref["d_m"].v, m.grad) < 1e-12
        assert rel(ref["kl"].v, kl.detach()) < 1e-12
    else:
        assert "d_m" not in ref and "kl" not in ref
    assert rel(ref["sums2"].v, R.LS_T1_SCALE * (torch.tril(inp["T"]) * torch.tril(inp["L"])).sum()) < 1e-12
    assert rel(ref["sums3"].v, inp["Gd"].sum()) < 1e-12


def _oracle_likelihood(mu0, cs, y, c, npts, p, hyp, mll, rows, jitter=O.KXX_JITTER):
    """autograd through the oracle's expressions (dsvgp_oracle.elbo_forward): returns what likelihood_ref returns"""
    mu0, cs, c = (t.clone().requires_grad_(True) for t in (mu0, cs, c))
    ell, s, noise = (hyp[k].clone().requires_grad_(True) for k in range(3))
    mu = mu0 + c
    var = s * O.kernel_diag(npts, p, ell) + jitter + cs
    varn = (var + noise).clamp_min(O.MIN_VARIANCE)
    if mll == 0:
        ll = -0.5 * (((y - mu) ** 2 + varn) / noise + torch.log(noise) + math.log(2 * math.pi))
    else:
        tot = (varn + noise).clamp_min(1e-8)
        ll = -0.5 * ((y - mu) ** 2 / tot + torch.log(tot) + math.log(2 * math.pi))
    (-(ll.sum()) / rows).backward()
    z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(mu=mu.detach(), varn=varn.detach(), mu_bar=z(mu0), var_bar=z(cs),
                scal=torch.stack([ll.sum().detach(), z(noise), z(c).reshape(()), z(s), z(ell)]))


@pytest.mark.parametrize("mll", [0, 1])
@pytest.mark.parametrize("Mp,Bp", [(7, 6), (130, 255), (1, 1)])
def test_likelihood_and_colstats_references_are_autograd_of_the_oracle(Mp, Bp, mll):
    inp = R.f64_inputs(Mp, Bp)
    p = R.f64_p(Bp)
    mu0, cs = R.colstats_ref(inp["A"], inp["W"], inp["m"])
    assert rel(mu0.v, inp["A"].t() @ inp["m"]) < 1e-12
    assert rel(cs.v, (inp["W"] ** 2 - inp["A"] ** 2).sum(0)) < 1e-12
    rows = 2.0 * Bp + 1.0
    ref = R.likelihood_ref(mu0.v, cs.v, inp["y"], inp["c"], p, inp["hyp"], mll, rows)
    orc = _oracle_likelihood(mu0.v, cs.v, inp["y"], inp["c"], Bp // (p + 1), p, inp["hyp"], mll, rows)
    for k in ("mu", "varn", "mu_bar", "var_bar", "scal"):
        assert rel(ref[k].v, orc[k]) < 1e-12, k
    # abar: the backward of mu0 = A^T m, cs = colsum(W^2 - A^2) with U = L_S W / S A in the place of W's pull-back
    A = inp["A"].clone().requires_grad_(True)
    ((A.t() @ inp["m"]) * inp["mu_bar"]).sum().backward()
    ab, av = R.abar_ref(inp["A"], None, inp["m"], inp["mu_bar"], inp["var_bar"])
    assert rel(ab.v, A.grad) < 1e-12
    ab, av = R.abar_ref(inp["A"], inp["U"], inp["m"], inp["mu_bar"], inp["var_bar"])
    assert rel(ab.v, A.grad + 2.0 * (inp["U"] - inp["A"]) * inp["var_bar"]) < 1e-12
    assert rel(av.v, 2.0 * inp["A"] * inp["var_bar"]) < 1e-12


@pytest.mark.parametrize("mll", [0, 1])
def test_likelihood_reference_at_the_variance_clamp_follows_the_oracles_clamp_min(mll):
    inp = R.f64_inputs(7, 6)
    mu0, cs = R.colstats_ref(inp["A"], inp["W"], inp["m"])
    csv = cs.v.clone()
    csv[4] = -5.0
    ref = R.likelihood_ref(mu0.v, csv, inp["y"], inp["c"], 2, inp["hyp"], mll, 13.0)
    orc = _oracle_likelihood(mu0.v, csv, inp["y"], inp["c"], 2, 2, inp["hyp"], mll, 13.0)
    assert float(ref["varn"].v[4]) == O.MIN_VARIANCE and float(ref["var_bar"].v[4]) == 0.0
    for k in ("mu", "varn", "mu_bar", "var_bar", "scal"):
        assert rel(ref[k].v, orc[k]) < 1e-12, k


def test_epilogue_reference_is_autograd_of_softplus_with_the_noise_floor():
    inp = R.epilogue_inputs()
    ref = R.epilogue_ref(inp)
    raw = inp["raw"].clone().requires_grad_(True)
    hyp = torch.stack([F.softplus(raw[0]), F.softplus(raw[1]), F.softplus(raw[2]) + O.NOISE_FLOOR])
    d = inp["d_hyp"][:3] + inp["scal"][[4, 3, 1]]
    (hyp * d).sum().backward()
    assert rel(ref["d_hyp"].v, d) < 1e-12
    assert rel(ref["d_raw"].v, inp["d_raw"] + raw.grad) < 1e-12
    assert rel(ref["d_const"].v, inp["d_const"][0] + inp["scal"][2]) < 1e-12
    assert rel(ref["loss"].v, -inp["scal"][0] / inp["rows"] + inp["kl0"][0] / inp["num_data"]) < 1e-12
    raw.grad = None
    hyp = torch.stack([F.softplus(raw[0]), F.softplus(raw[1]), F.softplus(raw[2]) + O.NOISE_FLOOR])
    (hyp * inp["d_hyp"][:3]).sum().backward()
    assert rel(R.hyp_backward_ref(inp).v, inp["d_raw"] + raw.grad) < 1e-12
    sp = F.softplus(inp["raw"])
    assert float(sp[0]) < 3e-3 and float(sp[2]) > 9.0                                                     # both tails


@pytest.mark.parametrize("npts,p", R.FIN_SHAPES)
@pytest.mark.parametrize("hyp", R.FIN_HYPS)
def test_finalize_reference_is_autograd_of_the_summed_expected_log_prob(npts, p, hyp):
    inp = R.fin_inputs(npts, p, hyp)
    ref = R.finalize_ref(inp)
    s_ = inp["sums"]
    ell, s, noise = (inp["hyp"][k].clone().requires_grad_(True) for k in range(3))
    nrow = npts * (p + 1)
    sum_var = s * O.kernel_diag(npts, p, ell).sum() + nrow * O.KXX_JITTER + s_[2] - s_[3]
    ll = -0.5 * ((s_[0] + sum_var + nrow * noise) / noise + nrow * (torch.log(noise) + math.log(2 * math.pi)))
    ll.backward()
    rows = inp["rows"]
    # (the variance enters through var + noise: d / d noise of the fast path holds var fixed AND counts the + noise, as the oracle does)
    want = torch.stack([ll.detach(), -noise.grad / rows, s_[1], -s.grad / rows, -ell.grad / rows])
    assert rel(ref.v[[0, 2]], want[[0, 2]]) < 1e-12
    # (scal[1]: -(r2 + var) / noise^2 + nrow / noise cancels, so "1e-12 relative" is taken of the larger of the value and its addends;
    #  for scal[3] and scal[4] the two coincide)
    for k in (1, 3, 4):
        assert abs(float(ref.v[k]) - float(want[k])) <= 1e-12 * max(abs(float(want[k])), float(ref.a[k])), k
    # sums[2] - sums[3] cancels to 1e-3 of either
    assert abs(float(s_[2] - s_[3])) < 1.1e-3 * float(s_[2])


# ------------------------------------------------------------------------------------------------ fast-path identity
@pytest.mark.parametrize("Mp,B,p", [(60, 17, 2), (61, 17, 2), (9, 4, 0)])
def test_fast_path_closed_form_equals_the_general_path(Mp, B, p):
    g = torch.Generator().manual_seed(Mp)
    Bp = B * (p + 1)
    A = R.draw(g, Mp, Bp) / math.sqrt(Mp)
    L = torch.tril(R.draw(g, Mp, Mp)) / math.sqrt(Mp)
    L.diagonal().copy_(R.draw_diag(g, Mp))
    m, y, c = R.draw(g, Mp), R.draw(g, Bp), torch.tensor([0.3], dtype=f64)
    hyp = torch.tensor([0.7, 1.3, 0.05, 0.0], dtype=f64)
    rows, nd = 2.0 * Bp + 1.0, 57.0
    # general: W = L_S^T A, column statistics, likelihood terms; d_LS = L_S-bar from W-bar, d_m = A mu_bar
    W = L.t() @ A
    mu0, cs = R.colstats_ref(A, W, m)
    gen = R.likelihood_ref(mu0.v, cs.v, y, c, p, hyp, 0, rows)
    Wbar = 2.0 * W * gen["var_bar"].v[None, :]                 # d loss / d W through cs
    dLS_gen = torch.tril(A @ Wbar.t())                         # W = L_S^T A  ->  L_S-bar = A W-bar^T
    dm_gen = A @ gen["mu_bar"].v
    # fast: G = A A^T, T = tril(G L_S), residual sums, finalize
    G = A @ A.t()
    T = torch.tril(G @ L)
    res = R.residual_ref(dict(mu=mu0.v + c, y=y, noise=hyp[2], rows=rows))
    inp = dict(m=m, L=L, T=T, dm0=A @ res["mu_bar"].v, Gd=G.diagonal().clone(), noise=hyp[2])
    var = R.ls_rows_ref(inp, 1, 0, num_data=nd, rows=rows, t1_scale=1.0)
    fast = R.fast_scalars(res["sums0"], res["sums1"], var["sums2"], var["sums3"], hyp, B, p, rows)
    assert rel(fast.v, gen["scal"].v) < 1e-11
    assert rel(res["mu_bar"].v, gen["mu_bar"].v) < 1e-11
    assert rel(var["d_LS"].v, dLS_gen) < 1e-11
    assert rel(inp["dm0"], dm_gen) < 1e-11


# ------------------------------------------------------------------------------------------------ sensitivity on the shared tables
@pytest.mark.parametrize("Mp", R.LS_MPS)
def test_sensitivity_ls_rows(Mp):
    """every (op, Mp) of LS_CASES (the layouts share their inputs).  LS_BIG_MP is not checked here: its inputs are drawn on the device, and
    tests/test_gpu_elbo_terms.py asserts the dropped-row condition on them there"""
    inp = R.ls_inputs(Mp)
    for _, scale, add_kl in R.LS_OPS:
        true = R.ls_rows_ref(inp, scale, add_kl)
        b = R.ls_bounds(true, Mp)
        drop = R.ls_rows_ref(inp, scale, add_kl, "drop_last")
        for k in ("sums2", "sums3") + (("kl",) if add_kl else ()):
            assert visible(true[k], drop[k], b[k]) > 10, (k, "drop_last")
        if add_kl:
            bad = R.ls_rows_ref(inp, scale, add_kl, "diag_offdiag")
            assert float(((bad["d_LS"].v - true["d_LS"].v).abs() / b["d_LS"]).diagonal().min()) > 10     # every diagonal element
        if Mp % 4 == 0:
            bad = R.ls_rows_ref(inp, scale, add_kl, "unmasked")
            for k in ("d_LS", "sums2") + (("kl",) if add_kl else ()):
                assert visible(true[k], bad[k], b[k].clamp_min(1e-300)) > 10, (k, "unmasked")
        if scale:
            bad = R.ls_rows_ref(inp, scale, add_kl, "no_scale")
            assert float(((bad["d_LS"].v - true["d_LS"].v).abs() / b["d_LS"]).tril().clamp_min(0)[torch.ones(Mp, Mp).tril().bool()].min()) > 10
    # each addend is at least 1e-3 of the sum of their absolute values where the drawn ranges guarantee it: squares of magnitudes in
    # [0.5, 1.5] span a factor 9, so up to about a hundred addends (the "more than 10 bounds" above is what holds on every case)
    if Mp <= 8:
        true = R.ls_rows_ref(inp, 0, 1)
        low = torch.ones(Mp, Mp).tril().bool()
        assert float((inp["L"][low] ** 2 * 0.5).min()) >= 1e-3 * float(true["kl"].a)
        assert float((inp["L"][low] * inp["T"][low]).abs().min()) * R.LS_T1_SCALE >= 1e-3 * float(true["sums2"].a)


@pytest.mark.parametrize("ncols", R.RES_NCOLS)
@pytest.mark.parametrize("deterministic", [False, True])
def test_sensitivity_residual_terms(ncols, deterministic):
    inp = R.res_inputs(ncols)
    true, drop = R.residual_ref(inp), R.residual_ref(inp, "drop_last")
    b = R.res_bounds(true, ncols, deterministic)
    for k in ("sums0", "sums1"):
        assert visible(true[k], drop[k], b[k]) > 10, k
    r = inp["y"] - inp["mu"]
    assert 0.5 - 1e-6 <= float(r.abs().min()) and float(r.abs().max()) <= 1.5 + 1e-6
    if ncols <= 100:       # (as in test_sensitivity_ls_rows)
        assert float((r * r).min()) >= 1e-3 * float(true["sums0"].a)


@pytest.mark.parametrize("n", R.TRACE_NS)
def test_sensitivity_trace_terms(n):
    inp = R.trace_inputs(n)
    true, drop = R.trace_ref(inp), R.trace_ref(inp, "drop_last")
    b = R.trace_bounds(true, n)
    for k in ("sums2", "sums3"):
        assert visible(true[k], drop[k], b[k]) > 10, k


@pytest.mark.parametrize("npts,p", R.FIN_SHAPES)
@pytest.mark.parametrize("hyp", R.FIN_HYPS)
def test_sensitivity_finalize_sign_of_the_trace(npts, p, hyp):
    inp = R.fin_inputs(npts, p, hyp)
    true, bad = R.finalize_ref(inp), R.finalize_ref(inp, "sums3_added")
    b = R.fin_bounds(true)
    for k in (0, 1):
        assert visible(true[k], bad[k], b[k]) > 10, k


@pytest.mark.parametrize("sizes", R.SCALE_SIZES)
def test_sensitivity_scale_by_vbar(sizes):
    g = torch.Generator().manual_seed(5)
    noise = R.r32(torch.tensor(R.RES_NOISE, dtype=f64))
    for n in sizes:
        if n:
            x = R.draw(g, n)
            true, bad = R.scale_ref(x, noise, 391.0), R.scale_ref(x, noise, 391.0, "no_scale")
            assert float(((bad.v - true.v).abs() / R.bound_elem(true.a, R.U32)).min()) > 10


@pytest.mark.parametrize("Mp", R.E_MPS)
def test_sensitivity_fast_and_general_path_case(Mp):
    """case e: a column left out of the general path's sums, a row left out of the fast path's, against the bound of each path"""
    inp = R.e_inputs(Mp)
    A, L, m, y, c, hyp, rows = (inp[k] for k in ("A", "L", "m", "y", "c", "hyp", "rows"))
    mu0, cs = R.colstats_ref(A, L.t() @ A, m)
    true = R.likelihood_ref(mu0, cs, y, c, R.E_P, hyp, 0, rows)
    drop = R.likelihood_ref(mu0, cs, y, c, R.E_P, hyp, 0, rows, broken="drop_last")
    for k in range(5):
        assert visible(true["scal"][k], drop["scal"][k], R.bound_sum(true["scal"].a[k], R.U32, R.e_chain_general(Mp))) > 10, k
    G = A @ A.t()
    res = R.residual_ref(dict(mu=mu0 + R.V(c)[0], y=y, noise=hyp[2], rows=rows))
    var_in = dict(m=m, L=L, T=torch.tril(G @ L), dm0=m, Gd=G.diagonal().clone(), noise=hyp[2])
    fast = {}
    for broken in (None, "drop_last"):
        var = R.ls_rows_ref(var_in, 1, 0, broken, num_data=57.0, rows=rows, t1_scale=1.0)
        fast[broken] = R.fast_scalars(res["sums0"], res["sums1"], var["sums2"], var["sums3"], hyp, R.E_B, R.E_P, rows)
    assert rel(fast[None].v, true["scal"].v) < 1e-11
    for k in (0, 1):
        assert visible(fast[None][k], fast["drop_last"][k], R.bound_sum(fast[None].a[k], R.U32, R.e_chain_fast(Mp))) > 10, k


@pytest.mark.parametrize("Mp", R.F64_MPS)
@pytest.mark.parametrize("Bp", R.F64_BPS)
def test_sensitivity_f64_tails(Mp, Bp):
    inp = R.f64_inputs(Mp, Bp)
    p = R.f64_p(Bp)
    mu0, cs = R.colstats_ref(inp["A"], inp["W"], inp["m"])
    mu0d, csd = R.colstats_ref(inp["A"], inp["W"], inp["m"], "drop_last")
    c = R.colstats64_chain(Mp)
    assert float(((mu0d.v - mu0.v).abs() / R.bound_sum(mu0.a, R.U64, c)).min()) > 10
    # (cs: every column's last row; W^2 - A^2 of one element may be small, the column maximum is not)
    assert visible(cs, csd, R.bound_sum(cs.a, R.U64, c)) > 10
    cc = R.cols64_chain(Bp)
    for mll in (0, 1):
        true = R.likelihood_ref(mu0.v, cs.v, inp["y"], inp["c"], p, inp["hyp"], mll, 2.0 * Bp + 1.0)
        drop = R.likelihood_ref(mu0.v, cs.v, inp["y"], inp["c"], p, inp["hyp"], mll, 2.0 * Bp + 1.0, broken="drop_last")
        for k in range(4):
            assert visible(true["scal"][k], drop["scal"][k], R.bound_sum(true["scal"].a[k], R.U64, cc)) > 10, (mll, k)
    tv = torch.tensor(0.37 * Bp, dtype=f64)
    true = R.fast_tail64_ref(mu0.v, inp["y"], inp["c"], Bp // (p + 1), p, inp["hyp"], tv, 2.0 * Bp + 1.0)
    drop = R.fast_tail64_ref(mu0.v, inp["y"], inp["c"], Bp // (p + 1), p, inp["hyp"], tv, 2.0 * Bp + 1.0, broken="drop_last")
    for k in (0, 1, 2, 6, 7):
        assert visible(true["scal"][k], drop["scal"][k], R.bound_sum(true["scal"].a[k], R.U64, cc)) > 10, k


@pytest.mark.parametrize("t,n,p", R.CIQ_SHAPES)
@pytest.mark.parametrize("jitter", R.CIQ_JITTERS)
@pytest.mark.parametrize("single", [True, False])
def test_sensitivity_and_clamp_rows_of_the_ciq_cases(t, n, p, jitter, single):
    inp = R.ciq_inputs(t, n, p, jitter, single)
    true, drop = R.ciq_rowstats_ref(inp), R.ciq_rowstats_ref(inp, "drop_last")
    u, c = (R.U32 if single else R.U64), R.ciq_chain(n)
    assert float(((drop["imean"].v - true["imean"].v).abs() / R.bound_sum(true["imean"].a, u, c)).min()) > 10
    live = true["live"].bool()
    assert float(((drop["var"].v - true["var"].v).abs() / R.bound_sum(true["var"].a, u, c))[live].min()) > 10 if live.any() else True
    # the engineered rows clamp and no other row does, both with a margin far beyond the bound
    assert [j for j in range(t) if not live[j]] == inp["clamp"]
    tsq, ivar = (inp["T"] ** 2).sum(1), (inp["ST"] * inp["T"]).sum(1)
    s, ell = float(inp["hyp"][1]), float(inp["hyp"][0])
    for j in inp["clamp"]:
        assert float(tsq[j]) > s / ell ** 2 + jitter + float(ivar[j]) + 0.05
        assert float(true["var"].v[j]) == O.MIN_VARIANCE
    tb = R.ciq_tbar_ref(inp, true["live"], true["imean"].v)
    for j in inp["clamp"]:
        assert torch.equal(tb["Tbar"].v[j], inp["mu_bar"][j] * inp["m"]) and float(tb["VT"].v[j].abs().max()) == 0.0
        assert float(tb["cvec"].v[j]) == float(inp["mu_bar"][j])


def test_adam_reference_is_torch_optim_adam():
    g = torch.Generator().manual_seed(9)
    hp = {k: float(torch.tensor(x, dtype=torch.float32)) for k, x in R.ADAM_HP.items()}
    p0 = R.draw(g, 33)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    p, m, v = R.V(p0), R.V(torch.zeros(33, dtype=f64)), R.V(torch.zeros(33, dtype=f64))
    for step in (1, 2, 3):
        gr = R.draw(g, 33)
        pt.grad = gr.clone()
        opt.step()
        p, m, v = R.adam_ref(p, gr, m, v, step, hp)
        assert rel(p.v, pt.detach()) < 1e-12
        assert rel(m.v, opt.state[pt]["exp_avg"]) < 1e-12 and rel(v.v, opt.state[pt]["exp_avg_sq"]) < 1e-12
