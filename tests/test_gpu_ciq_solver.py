"""csrc/ciq.hip against its restatement (tests/_ciq_ref.py) after EXACTLY J iterations on both sides: ``tol < 0`` and
``max_iter = J`` take the two convergence tests out of the comparison, so the solver is held like any other kernel --
truth = the float64 restatement on float32-rounded inputs (pinned to ``O.msminres`` in tests/test_ciq_host.py), yardstick y =
its float32 runs, recomputed here (_ciq_ref.compare says how y is pooled); error per right-hand side (row) relative to that row's
own maximum in the truth.  Float entry points: err <= 4 y + 2e-7.  Double entry points: err <= 5 y 2^-29 + 1e-13 (derived in
_ciq_ref.bound; the float64 STEP at J = 20 is the one place where 4 x the distance of two float64 CPU runs is larger: _step_bounds).
The cases, what each reaches, and the conditions under which a case is admitted are in _ciq_ref.CASES / Case.admit; measured
err / bound figures are printed as [parity] lines."""
import math

import pytest
import torch

import dsvgp_oracle as O
import _ciq_ref as R
from test_ngd import make_ngd_problem, relmax

pytestmark = pytest.mark.gpu
f32, f64 = torch.float32, torch.float64
DTYPES = [pytest.param(f32, id="f32"), pytest.param(f64, id="f64")]
NAN = float("nan")


@pytest.fixture(scope="module")
def cases():
    return {name: R.Case(name) for name in R.CASES}


def _offset_view(numel, shape, dt, dev, offset, fill=NAN):
    """a contiguous tensor of ``shape`` that starts ``offset`` elements into its allocation"""
    buf = torch.full((numel + offset + 4,), fill, dtype=dt, device=dev)
    return buf[offset:offset + numel].view(*shape), buf


def _strided(src, ld, dt, dev, offset):
    """src [r, c] as a row-major device matrix with leading dimension ld, ``offset`` elements into a NaN-filled allocation"""
    r, c = src.shape
    flat, buf = _offset_view(r * ld, (r, ld), dt, dev, offset)
    v = flat[:, :c]
    v.copy_(src.to(dt))
    return v, buf


class Solve:
    """one dsvgp_ciq_solve call on a case and everything it left behind, on the CPU"""

    def __init__(self, dsvgp, dev, c, dt, check_every=10, cap=None, tol=-1.0, max_iter=None, mix=True):
        ops = dsvgp._ops
        ctx = ops.Context.get(dev)
        n, t, Q, J = c.n, c.t, c.Q, c.J
        padded = c.name == "padded"
        off = 1 if padded else 0
        cap = J + 2 if cap is None else cap
        self.cap = cap
        K, _ = _strided(c.K, n + 3 if padded else n, dt, dev, off)
        Rm, _ = _strided(c.R, n + 1 if padded else n, dt, dev, off)
        ldo = n + 5 if padded else n + 4
        self.out_full = torch.full((t, ldo), NAN, dtype=dt, device=dev)
        out = self.out_full[:, :n]
        basis, _ = _offset_view((cap + 1) * t * n, (cap + 1, t, n), dt, dev, off)
        QP = ops.ciq_qp(Q)
        ycoef = torch.full((t, cap, QP), NAN, dtype=dt, device=dev)
        rnorm = torch.full((t,), NAN, dtype=dt, device=dev)
        esz = 4 if dt == f32 else 8
        ws = torch.zeros(ops.ciq_workspace_bytes(Q, t, n, cap, dt) // esz + 1, dtype=dt, device=dev)
        sig, om = c.sigma.to(dt).to(dev), c.omega.to(dt).to(dev)
        self.its = ops.ciq_solve(ctx, K, Rm, sig, om, basis, ycoef, rnorm, out, ws, tol=tol,
                                 max_iter=J if max_iter is None else max_iter, check_every=check_every)
        torch.cuda.synchronize()
        if self.its is None:
            return
        its = self.its
        tn, ro = t * n, R.ratio_offset(Q, t, n)
        b0, b1 = ws[tn + t:tn + 2 * t], ws[tn + 2 * t:tn + 3 * t]
        last, prev = (b1, b0) if its % 2 else (b0, b1)              # the driver swaps the two beta rows after every step but the last
        self.got = {"rnorm": rnorm, "basis": basis[:its + 1], "ycoef": ycoef[:, :its, :Q], "out": out,
                    "ratio": ws[ro:ro + Q * t].view(Q, t), "alpha_last": ws[tn:tn + t], "beta_last": last, "beta_prev": prev}
        if its < 2:
            del self.got["beta_prev"]
        if mix:                                                      # the per-shift solves are not stored: dsvgp_ciq_mix forms them
            self.got["X"] = ops.ciq_mix(ctx, basis, its, ycoef, Q, rnorm, torch.empty(Q, t, n, dtype=dt, device=dev))
        self.got = {k: v.detach().cpu().clone() for k, v in self.got.items()}
        self.untouched = {"out padding": self.out_full[:, n:].cpu(), "basis slots past J": basis[its + 1:].cpu()}
        self.ycoef_pad = ycoef[:, :, Q:].cpu()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_solver_matches_restatement_at_matched_iterations(dsvgp, gpu_device, cases, name, dt):
    c = cases[name]
    s = Solve(dsvgp, gpu_device, c, dt)
    assert s.its == c.J
    R.exact_rows_ok(c, s.got)
    where = {}
    w = R.compare(c, s.got, dt, where)
    print("[parity] ciq solve %s %s (n=%d t=%d Q=%d J=%d) err / bound: %s" % (
        name, "f32" if dt == f32 else "f64", c.n, c.t, c.Q, c.J, ", ".join("%s %.2f" % kv for kv in w.items())))
    assert max(w.values()) <= 1.0, {k: (v, where[k]) for k, v in w.items() if v > 1.0}
    # what the call has no business writing is still NaN; the padding of the coefficient table is the zero it was set to
    assert torch.isnan(s.untouched["out padding"]).all()
    assert torch.isnan(s.untouched["basis slots past J"]).all() and s.untouched["basis slots past J"].numel() > 0
    assert (s.ycoef_pad == 0).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_test_schedule_and_capacity_do_not_change_a_bit(dsvgp, gpu_device, cases, name, dt):
    """check_every decides when the statistic is formed and nothing else; a basis of exactly J rows suffices and one of J - 1
    returns ENOSPACE.  (The products with K run in the library's deterministic mode here: split-K over floating-point atomics
    is a run-to-run difference of its own.)"""
    c = cases[name]
    ctx = dsvgp._ops.Context.get(gpu_device)
    scratch = torch.empty(32 << 20, dtype=torch.uint8, device=gpu_device)
    ctx.set_deterministic(scratch)
    try:
        ref = Solve(dsvgp, gpu_device, c, dt, check_every=10, mix=False)
        assert ref.its == c.J
        for ce, cap in ((3, None), (1, None), (10, c.J)):
            s = Solve(dsvgp, gpu_device, c, dt, check_every=ce, cap=cap, mix=False)
            assert s.its == c.J
            for k, v in ref.got.items():
                assert torch.equal(v, s.got[k]), (k, ce, cap)
        assert Solve(dsvgp, gpu_device, c, dt, cap=c.J - 1, mix=False).its is None
    finally:
        ctx.set_deterministic(None)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", R.STOP_CASES)
def test_solver_stops_at_the_restatements_iteration(dsvgp, gpu_device, name, dt):
    """a tolerance the restatement's mean statistic brackets by >= 4 on both sides (asserted in tests/test_ciq_host.py): the
    solver must pass every earlier test and stop at exactly that one -- the norms kernel, its second pass of shifts included"""
    c, tol, stop, br, m = R.stop_plan(name, f64)
    assert min(br) >= 4.0
    s = Solve(dsvgp, gpu_device, c, dt, tol=tol, max_iter=R.STOP_MAX_ITER, cap=R.STOP_MAX_ITER, mix=False)
    mean = s.got["ratio"].double().mean().item()
    print("[parity] ciq stop %s %s: stopped at %d (restatement %d), mean statistic %.3e (restatement %.3e, tol %.3e)" % (
        name, "f32" if dt == f32 else "f64", s.its, stop, mean, m[stop], tol))
    assert s.its == stop


def _running_bound(ey, dt):
    """the yardstick of step k is the worst float32-restatement error up to step k: the recurrence carries its errors forward"""
    return R.bound(torch.cummax(ey, 0).values, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ["odd", "ragged_trips", "padded"])
def test_lanczos_alone_matches_restatement(dsvgp, gpu_device, cases, name, dt):
    """dsvgp_ciq_lanczos (the Ritz-bound run: ciq_symv_kernel + ciq_lanczos_kernel on one row), 20 steps: alpha and beta against
    the restatement; then a start at an eigenvector -- beta[0] at round-off, everything finite"""
    ops = dsvgp._ops
    ctx = ops.Context.get(gpu_device)
    c = cases[name]
    padded = name == "padded"
    K, _ = _strided(c.K, c.n + 3 if padded else c.n, dt, gpu_device, 1 if padded else 0)
    v0 = c.R[0:1]
    alpha, beta = ops.ciq_lanczos(ctx, K, v0[0].to(dt).to(gpu_device).contiguous(), 20)
    T = R.restate(c.K, v0, c.sigma, c.omega, 20)
    Y = R.restate(c.K.float(), v0.float(), c.sigma, c.omega, 20)
    worst = {}
    for k, got in (("alpha", alpha), ("beta", beta)):
        assert got.dtype == dt and torch.isfinite(got).all()
        e = R.rel(got, T[k][:, 0])
        worst[k] = (e / _running_bound(R.rel(Y[k][:, 0], T[k][:, 0]), dt)).max().item()
    print("[parity] ciq lanczos %s %s err / bound: alpha %.2f, beta %.2f" % (name, "f32" if dt == f32 else "f64", worst["alpha"], worst["beta"]))
    assert max(worst.values()) <= 1.0, worst
    lam, U = torch.linalg.eigh(c.K)
    a, b = ops.ciq_lanczos(ctx, K, U[:, c.n // 2].to(dt).to(gpu_device).contiguous(), 20)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    eps = 2.0 ** -24 if dt == f32 else 2.0 ** -53
    # |K v - (v.Kv) v| for v within eps of a unit eigenvector: a few eps |K| from the rounding of v, sqrt(n) eps |K| from the product
    assert abs(a[0].item() - lam[c.n // 2].item()) <= 8 * eps * lam.max().item()
    assert b[0].item() <= (8 + math.sqrt(c.n)) * eps * lam.max().item()


# ------------------------------------------------------------------ the two limits
def test_lds_limit_largest_accepted_row(dsvgp, gpu_device):
    """n sizeof(T) = 64 KiB exactly, double: ciq_lanczos_kernel keeps one row in dynamic LDS beside 32 bytes of static LDS.
    n = 8192 must run (Lanczos alone and the solve) and be right; n = 8193 must be refused."""
    ops = dsvgp._ops
    dev = gpu_device
    ctx = ops.Context.get(dev)
    n, t, Q, J = 8192, 2, 3, 3
    g = torch.Generator().manual_seed(8192)
    lam = (torch.logspace(0, math.log10(30.0), n, dtype=f64) * 1e-2)[torch.randperm(n, generator=g)]
    u = torch.randn(n, generator=g, dtype=f64) * (0.1 / math.sqrt(n))
    K = torch.outer(u, u)
    K.diagonal().add_(lam)                                           # diag(lam) + u u^T: spectrum inside [1e-2, 0.3 + |u|^2]
    K = K.float().double()                                           # (u_i u_j rounds the same both ways: still symmetric)
    Rm = torch.randn(t, n, generator=g, dtype=f64)
    sigma, omega = O.ciq_quadrature(1e-2, 0.31, Q)
    c = R.Case.from_arrays("lds_limit", K, Rm, sigma, omega, J)
    c.nperm = 0                                                      # (one float32 run: a permuted copy of K is 256 MB and seconds)
    c.K = K
    Kd = K.to(dev)
    alpha, beta = ops.ciq_lanczos(ctx, Kd, c.R[0].to(dev).contiguous(), 3)
    T1 = R.restate(c.K, c.R[0:1], c.sigma, c.omega, 3)
    Y1 = R.restate(c.K.float(), c.R[0:1].float(), c.sigma, c.omega, 3)
    wl = {k: (R.rel(got, T1[k][:, 0]) / _running_bound(R.rel(Y1[k][:, 0], T1[k][:, 0]), f64)).max().item()
          for k, got in (("alpha", alpha), ("beta", beta))}
    cap = J + 2
    basis = torch.full((cap + 1, t, n), NAN, dtype=f64, device=dev)
    ycoef = torch.empty(t, cap, ops.ciq_qp(Q), dtype=f64, device=dev)
    rnorm, out = torch.empty(t, dtype=f64, device=dev), torch.empty(t, n, dtype=f64, device=dev)
    ws = torch.zeros(ops.ciq_workspace_bytes(Q, t, n, cap, f64) // 8 + 1, dtype=f64, device=dev)
    its = ops.ciq_solve(ctx, Kd, c.R.to(dev), c.sigma.to(dev), c.omega.to(dev), basis, ycoef, rnorm, out, ws, tol=-1.0,
                        max_iter=J, check_every=10)
    assert its == J
    ro = R.ratio_offset(Q, t, n)
    got = {"rnorm": rnorm, "basis": basis[:J + 1], "ycoef": ycoef[:, :J, :Q], "out": out, "ratio": ws[ro:ro + Q * t].view(Q, t),
           "X": ops.ciq_mix(ctx, basis, J, ycoef, Q, rnorm, torch.empty(Q, t, n, dtype=f64, device=dev))}
    got = {k: v.cpu() for k, v in got.items()}
    R.exact_rows_ok(c, got)
    w = R.compare(c, got, f64)
    print("[parity] ciq LDS limit n=8192 f64 err / bound: lanczos alpha %.2f, beta %.2f; solve %s" % (
        wl["alpha"], wl["beta"], ", ".join("%s %.2f" % kv for kv in w.items())))
    assert max(wl.values()) <= 1.0 and max(w.values()) <= 1.0, (wl, w)
    assert torch.isnan(basis[J + 1:]).all()
    del Kd, basis
    n1 = n + 1
    K1 = torch.empty(n1, n1, dtype=f64, device=dev)                  # (never read: the entry refuses before any launch)
    with pytest.raises(dsvgp._lib.DsvgpError):
        ops.ciq_lanczos(ctx, K1, torch.ones(n1, dtype=f64, device=dev), 3)
    with pytest.raises(dsvgp._lib.DsvgpError):
        ops.ciq_solve(ctx, K1, torch.ones(t, n1, dtype=f64, device=dev), c.sigma.to(dev), c.omega.to(dev),
                      torch.empty(cap + 1, t, n1, dtype=f64, device=dev), ycoef, rnorm, torch.empty(t, n1, dtype=f64, device=dev),
                      torch.empty(ops.ciq_workspace_bytes(Q, t, n1, cap, f64), dtype=torch.uint8, device=dev), tol=-1.0, max_iter=J)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("t", [65537, 98304])
def test_row_limit_more_rows_than_a_grid_dimension(dsvgp, gpu_device, t, dt):
    """dsvgp_ciq_mix and dsvgp_ciq_tbar with more rows than any HIP device takes in grid.y (65 535 or 65 536; t = B (p + 1) is 98 304
    at B = 16 384, p = 5), against the tensor expressions of test_ciq_mix_and_cross_against_plain_tensor_expressions"""
    ops = dsvgp._ops
    dev = gpu_device
    ctx = ops.Context.get(dev)
    g = torch.Generator().manual_seed(t)
    J, n, Kout = 2, 4, 1
    KP = ops.ciq_qp(Kout)
    basis = torch.randn(J + 1, t, n, generator=g, dtype=dt)
    C = torch.randn(t, J, KP, generator=g, dtype=dt)
    scale = torch.rand(t, generator=g, dtype=dt) + 0.5
    out = ops.ciq_mix(ctx, basis.to(dev), J, C.to(dev), Kout, scale.to(dev), torch.full((Kout, t, n), NAN, dtype=dt, device=dev))
    ref = torch.einsum("rjk,jrn->krn", C[:, :J, :Kout].double(), basis[:J].double()) * scale.double()[None, :, None]
    tol = 2e-6 if dt == f32 else 1e-13
    assert R.row_err(out, ref).max() < tol
    Tm, ST = torch.randn(t, n, generator=g, dtype=dt), torch.randn(t, n, generator=g, dtype=dt)
    m = torch.randn(n, generator=g, dtype=dt)
    mu_bar, var_bar, imean = (torch.randn(t, generator=g, dtype=dt) for _ in range(3))
    live = (torch.rand(t, generator=g) > 0.2).to(dt)
    Tbar, VT = (torch.full((t, n), NAN, dtype=dt, device=dev) for _ in range(2))
    up = lambda a: a.to(dev)
    cvec = ops.ciq_tbar(ctx, up(Tm), up(ST), up(m), up(mu_bar), up(var_bar), up(live), up(imean), Tbar, VT)
    d = lambda a: a.double()
    vb = d(var_bar) * d(live)
    assert R.row_err(Tbar, 2 * vb[:, None] * (d(ST) - d(Tm)) + d(mu_bar)[:, None] * d(m)[None, :]).max() < 4 * tol
    assert R.row_err(VT, vb[:, None] * d(Tm)).max() < tol
    assert relmax(cvec, d(mu_bar) - 2 * vb * d(imean)) < tol


# ------------------------------------------------------------------ the whole step at matched iterations
STEP_PROBLEM = (500, 20, 24, 5, 48)
FAR = 1
_step_cache = {}


def _step_problem(far_point=False):
    """make_ngd_problem(500, 20, 24, 5, 48, seed=520) built in float32; ``far_point`` moves data point FAR to 1e3 lengthscales from
    every inducing point (all inputs lie in [0, 1]^20): its K_XZ rows are exactly zero in float32.  (Not point 0: the spectrum
    estimate starts its Lanczos run at the first right-hand side, in the reference as in the oracle, and the oracle's fails on a zero
    start; the steps here are given the interval.)"""
    P, x, y, D, nd = make_ngd_problem(*STEP_PROBLEM, seed=520)
    if far_point:
        ell = float(torch.nn.functional.softplus(P["raw_lengthscale"]).reshape(()))
        x = x.clone()
        x[FAR] = x[FAR] + 1e3 * ell
    return P, x, y, D, nd


def _oracle_step(monkeypatch, J, Q, far_point=False):
    """-> (float64 oracle run, float32 oracle run, (lmin, lmax), float64 run with the restated solver) with msMINRES held to exactly J iterations on the spectrum interval
    of one free float64 run; each run is (loss, grads, mu, varn)"""
    key = (J, Q, far_point)
    if key not in _step_cache:
        P, x, y, D, nd = _step_problem(far_point)
        w = lambda a: a.double()
        P64 = {k: w(v) for k, v in P.items()}
        if "bounds" not in _step_cache:                             # (K_ZZ does not depend on the data: one interval for both problems)
            st = {}
            P0, x0, y0, D0, _ = _step_problem()
            O.ciq_loss_and_grads(P64, w(x0), w(y0), w(D0), nd, stats=st)
            _step_cache["bounds"] = (st["lmin"], st["lmax"])
        bounds = _step_cache["bounds"]
        free = O.msminres
        with monkeypatch.context() as mp:
            mp.setattr(O, "msminres", lambda K, R, sigma, tol=None, max_iter=None: free(K, R, sigma, tol=-1.0, max_iter=J))
            mp.setattr(O, "lanczos_eig_bounds", lambda K, v0, iters=None: bounds)
            r64 = O.ciq_loss_and_grads(P64, w(x), w(y), w(D), nd, Q=Q)
            r32 = O.ciq_loss_and_grads(P, x, y, D, nd, Q=Q)
            # a second float64 run with the solver restated (basis-resident, tests/_ciq_ref.py): how far two float64 roundings of the
            # same J iterations are apart
            mp.setattr(O, "msminres", lambda K, R_, sigma, tol=None, max_iter=None: (
                R.restate(K, R_.t().contiguous(), sigma, torch.ones_like(sigma), J)["X"].transpose(1, 2).contiguous(), J))
            r64b = O.ciq_loss_and_grads(P64, w(x), w(y), w(D), nd, Q=Q)
        _step_cache[key] = (r64, r32, bounds, r64b)
    return _step_cache[key]


def _step_bounds(r64, r32, r64b, dt, predict=True):
    """4 y + 2e-7 per output, y the float32 oracle run.  Float64 mode: 5 y 2^-29 + 1e-13, or 4 x the distance between the two float64
    CPU runs (oracle solver / restated solver) where that is larger: at J = 20 the Lanczos recurrence of this K_ZZ (an isolated
    largest eigenvalue, found to round-off by step ~12) has lost orthogonality, and two float64 roundings of it are 4e-10 apart in
    the solves where they were 3e-14 apart at J = 12."""
    y = _step_errors(r32, r64, (r32[2], r32[3]) if predict else None)
    b = {k: R.bound(v, dt) for k, v in y.items()}
    d = _step_errors(r64b, r64, (r64b[2], r64b[3]) if predict else None)
    if dt == f64:
        b = {k: max(v, 4.0 * d[k]) for k, v in b.items()}
    return b, y, d


def _step_errors(got, ref, predict=None):
    loss, grads, mu, varn = got
    l_ref, g_ref, mu_ref, var_ref = ref
    e = {"loss": abs(float(loss) - float(l_ref)) / abs(float(l_ref)), "mu": relmax(mu, mu_ref), "var": relmax(varn, var_ref)}
    for k in O.NGD_PARAM_NAMES:
        if g_ref[k].numel() and g_ref[k].abs().max() > 0:
            e["g_" + k] = relmax(grads[k], g_ref[k])
    if predict is not None:
        e["predict_mu"], e["predict_var"] = relmax(predict[0], mu_ref), relmax(predict[1], var_ref)
    return e


def _engine(dsvgp, dev, dt, J, Q, form, bounds):
    if dt == f64:
        from dsvgp_amd._step64 import ElboEngine64
        eng = ElboEngine64(dev)
    else:
        eng = dsvgp.ElboEngine(dev, trsm_nb=4096)
    eng.whitening, eng.ciq_tolerance, eng.ciq_max_iter, eng.ciq_eig_bounds = "ciq", -1.0, J, bounds
    eng.ciq_num_quadrature, eng.ciq_backward_form = Q, form
    return eng


def _run_engine(eng, dev, dt, problem):
    P, x, y, D, nd = problem
    up = lambda a: a.to(dt).to(dev)
    Pg = {k: up(v) for k, v in P.items()}
    got = eng.loss_and_grads(Pg, up(x), up(y), up(D), nd)
    got = (got[0].item(), {k: v.clone() for k, v in got[1].items()}, got[2].clone(), got[3].clone())
    return got, eng.predict(Pg, up(x), up(D))


STEP_COMBOS = [(12, 15, "backward"), (12, 15, "forward"), (12, 15, "shifts"), (20, 15, None), (12, 17, None), (20, 17, None)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("J,Q,form", STEP_COMBOS)
def test_step_matches_oracle_at_matched_iterations(dsvgp, gpu_device, monkeypatch, J, Q, form, dt):
    """ElboEngine._ciq_step / ElboEngine64._ciq_step64 with ciq_tolerance = -1, ciq_max_iter = J and the oracle's spectrum interval
    against the float64 oracle held to the same J: every output within 4 y + 2e-7 (float64 mode: 5 y 2^-29 + 1e-13) of its own
    maximum, y the float32 oracle run.  J = 12 < Q stacks the backward over a basis, J = 20 over the shifts."""
    r64, r32, bounds, r64b = _oracle_step(monkeypatch, J, Q)
    eng = _engine(dsvgp, gpu_device, dt, J, Q, form, bounds)
    got, pred = _run_engine(eng, gpu_device, dt, _step_problem())
    assert eng.ciq_stats["iterations"] == J and eng.ciq_stats["iterations_backward"] == J
    e = _step_errors(got, r64, pred)
    b, y, d = _step_bounds(r64, r32, r64b, dt)
    ratio = {k: e[k] / b[k] for k in e}
    print("[parity] ciq step J=%d Q=%d form=%s %s err / bound: %s | yardstick %s | two float64 CPU runs apart %s" % (
        J, Q, form, "f32" if dt == f32 else "f64", ", ".join("%s %.2f" % kv for kv in ratio.items()), ", ".join("%s %.1e" % kv for kv in y.items()),
        ", ".join("%s %.1e" % kv for kv in d.items())))
    assert max(ratio.values()) <= 1.0, ratio


@pytest.mark.parametrize("dt", DTYPES)
def test_step_with_a_data_point_far_from_every_inducing_point(dsvgp, gpu_device, monkeypatch, dt):
    """one data point whose K_XZ rows are exactly zero (a zero right-hand side for the solver, rows that ciq_init_kernel divides by 1):
    its mean is the constant, its variance the prior diagonal + noise, every gradient is finite, and every other point stays within
    the bound of the run without it"""
    J, Q = 12, 15
    P, x, y, D, nd = prob = _step_problem(far_point=True)
    p1 = STEP_PROBLEM[3] + 1
    rows = slice(FAR * p1, (FAR + 1) * p1)
    r64, r32, bounds, r64b = _oracle_step(monkeypatch, J, Q, far_point=True)
    eng = _engine(dsvgp, gpu_device, dt, J, Q, None, bounds)
    got, pred = _run_engine(eng, gpu_device, dt, prob)
    loss, grads, mu, varn = got
    assert math.isfinite(loss) and all(torch.isfinite(g).all() for g in grads.values())
    ell, s, noise = (float(v.reshape(-1)[0]) for v in O.constrained({k: v.double() for k, v in P.items()}))
    prior = torch.tensor([s] + [s / ell ** 2] * (p1 - 1), dtype=f64) + noise
    assert relmax(r64[2][rows], torch.full((p1,), float(P["constant"]), dtype=f64)) < 1e-15 and relmax(r64[3][rows], prior) < 1e-14
    # the interpolation mean of a zero row is an exact zero: the mean IS the constant; the variance is softplus arithmetic in the
    # model's precision, held to the float32 oracle's own distance from the float64 value
    assert (mu[rows].double().cpu() == float(P["constant"])).all()
    assert relmax(varn[rows], prior) <= R.bound(relmax(r32[3][rows], prior), dt)
    e = _step_errors(got, r64, pred)
    b, _, _ = _step_bounds(r64, r32, r64b, dt)
    ratio = {k: e[k] / b[k] for k in e}
    # every other point against the same oracle, under the yardstick of the problem WITHOUT the far point
    q64, q32, _, q64b = _oracle_step(monkeypatch, J, Q)
    b0, _, _ = _step_bounds(q64, q32, q64b, dt, predict=False)
    other = torch.ones(mu.shape[0], dtype=torch.bool)
    other[rows] = False
    ratio["mu_other"] = relmax(mu.cpu()[other], r64[2][other]) / b0["mu"]
    ratio["var_other"] = relmax(varn.cpu()[other], r64[3][other]) / b0["var"]
    print("[parity] ciq step with a far data point %s err / bound: %s" % ("f32" if dt == f32 else "f64", ", ".join("%s %.2f" % kv for kv in ratio.items())))
    assert max(ratio.values()) <= 1.0, ratio
