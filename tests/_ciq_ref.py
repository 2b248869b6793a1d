"""csrc/ciq.hip restated in plain torch, in the arithmetic of its inputs (float64: the truth; float32: the yardstick).

The oracle's ``msminres`` carries Paige-Saunders' w / x vectors per shift and stops on its own test; the HIP solver keeps the
Lanczos BASIS and per (shift, row) rotation scalars, and forms x_J = V R^-1 phi by a three-band back-substitution.  This file
follows the kernels step for step (row layout [t, n], the 1e-10 norm gate of ciq_init_kernel, the 1e-30 floors, the history
slots of ciq_givens_kernel, ciq_backsub_kernel's recurrences, the statistic of ciq_norms_kernel, ciq_cout_kernel + ciq_mix for
``out``) so that every intermediate the library leaves in memory has a counterpart to be compared with after EXACTLY J
iterations.  tests/test_ciq_host.py pins it to ``O.msminres(tol=-1, max_iter=J)`` in float64.

``broken=`` names one deliberate error (BROKEN): what a subtly wrong kernel would compute.
  no_eps_band        the back-substitution drops R_{i-2,i}
  shift_reused       one shift q >= 1 runs with sigma_{q-1}
  tail_dropped       the alpha dot product ignores the last n % 256 elements
  omega_dropped      one shift is missing from the ``out`` sum
  second_pass_zero   the statistic of shifts >= 16 (the norms kernel's second pass) is 0
  late_tail_dropped  tail_dropped, but only when the loop takes more than one trip (n > 256)
  phi_stale          the statistic is formed with |phi_{J-1}|: the history slot of the previous iteration"""
import math

import torch

import dsvgp_oracle as O

f32, f64 = torch.float32, torch.float64
BROKEN = ("no_eps_band", "shift_reused", "tail_dropped", "omega_dropped", "second_pass_zero", "late_tail_dropped", "phi_stale")
N_EDGE = 3


def spd(n, cond=30.0, seed=5):
    """tests/test_ciq.py's matrix: random orthogonal eigenvectors, eigenvalues 1e-2 * logspace(0, log10 cond)."""
    g = torch.Generator().manual_seed(seed)
    U, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=f64))
    lam = torch.logspace(0, math.log10(cond), n, dtype=f64) * 1e-2
    return (U * lam) @ U.t(), lam


def edge_rows(K):
    """[3, n] float64: a zero right-hand side, one under ciq_init_kernel's 1e-10 norm gate (unit-scale entries times 1e-12:
    it is divided by 1, not by its norm), and an eigenvector of K (Lanczos breaks down at its first step)."""
    n = K.shape[0]
    g = torch.Generator().manual_seed(1000 + n)
    _, U = torch.linalg.eigh(K.to(f64))
    return torch.stack([torch.zeros(n, dtype=f64), torch.randn(n, generator=g, dtype=f64) * 1e-12, U[:, n // 2].clone()])


def ratio_offset(Q, t, n):
    """element offset of ratio[Q * t] in the solve's workspace (ciq_workspace_bytes: Vt[t n], alpha, beta0, beta1 [t] each,
    state[5 Q t], then ratio); alpha sits at t n, beta0 / beta1 at t n + t / t n + 2 t"""
    return t * n + 3 * t + 5 * Q * t


def restate(K, R, sigma, omega, J, check_every=10, broken=None, broken_q=None):
    """J iterations of the basis-resident msMINRES of csrc/ciq.hip on K [n, n], R [t, n] (rows), in R's dtype.
    Returns a dict: rnorm [t]; basis [J + 1, t, n]; alpha, beta [J, t] (beta[j] = |v| of step j + 1); ycoef, zcoef [t, J, Q] of the
    LAST test; stats {it: [Q, t]} for every multiple of check_every <= J and for J; X [Q, t, n] = rnorm * sum_j y_jq q_j;
    cout [t, J]; out [t, n]."""
    assert broken is None or broken in BROKEN
    dt = R.dtype
    K, sigma, omega = K.to(dt), sigma.to(dt), omega.to(dt)
    t, n = R.shape
    Q = sigma.shape[0]
    if broken == "shift_reused":
        qb = Q // 2 if broken_q is None else broken_q
        assert qb >= 1
        sigma = sigma.clone()
        sigma[qb] = sigma[qb - 1]
    rnorm = R.norm(dim=1)
    rnorm = torch.where(rnorm < 1e-10, torch.ones_like(rnorm), rnorm)
    basis = torch.zeros(J + 1, t, n, dtype=dt)
    basis[0] = R / rnorm[:, None]
    alpha, beta = torch.zeros(J, t, dtype=dt), torch.zeros(J, t, dtype=dt)
    cs, sn = -torch.ones(Q, t, dtype=dt), torch.zeros(Q, t, dtype=dt)
    dbar, eps, phibar = torch.zeros(Q, t, dtype=dt), torch.zeros(Q, t, dtype=dt), torch.ones(Q, t, dtype=dt)
    hist = torch.zeros(J, 4, Q, t, dtype=dt)                       # oldeps, delta, 1 / gamma, phi
    ndot = n - n % 256 if broken == "tail_dropped" or (broken == "late_tail_dropped" and n > 256) else n
    stats = {}
    ycoef = zcoef = None
    for it in range(1, J + 1):
        q = basis[it - 1]
        v = q @ K                                                  # K symmetric: the row-major product of the GEMM
        if it >= 2:
            v = v - beta[it - 2][:, None] * basis[it - 2]
        a = (q[:, :ndot] * v[:, :ndot]).sum(1)
        v = v - a[:, None] * q
        bn = v.norm(dim=1)
        alpha[it - 1], beta[it - 1] = a, bn
        basis[it] = v / bn.clamp_min(1e-30)[:, None]
        alfa = a[None, :] + sigma[:, None]
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        gamma = torch.sqrt(gbar * gbar + bn * bn).clamp_min(1e-30)
        cs2, sn2 = gbar / gamma, bn / gamma
        hist[it - 1, 0], hist[it - 1, 1], hist[it - 1, 2], hist[it - 1, 3] = eps, delta, 1.0 / gamma, cs2 * phibar
        dbar, eps, phibar = -cs * bn, sn * bn, sn2 * phibar
        cs, sn = cs2, sn2
        if it % check_every == 0 or it == J:
            ycoef, zcoef = backsub(hist[:it], broken)
            Vy = torch.einsum("jqr,jrn->qrn", ycoef.to(dt), basis[:it])
            Vz = torch.einsum("jqr,jrn->qrn", zcoef.to(dt), basis[:it])
            phi = hist[it - 2, 3] if broken == "phi_stale" and it >= 2 else hist[it - 1, 3]
            s = phi.abs() * Vz.norm(dim=2) / Vy.norm(dim=2).clamp_min(1e-30)
            if broken == "second_pass_zero":
                s[16:] = 0
            stats[it] = s
    yc = ycoef.to(dt)                                              # [J, Q, t]
    X = torch.einsum("jqr,jrn->qrn", yc, basis[:J]) * rnorm[None, :, None]
    om = omega.clone()
    if broken == "omega_dropped":
        om[Q // 2 if broken_q is None else broken_q] = 0
    cout = torch.einsum("q,jqr->rj", om.to(f64), yc.to(f64)).to(dt)     # (ciq_cout_kernel sums in double)
    out = torch.einsum("rj,jrn->rn", cout, basis[:J]) * rnorm[:, None]
    return dict(rnorm=rnorm, basis=basis, alpha=alpha, beta=beta, ycoef=yc.permute(2, 0, 1).contiguous(),
                zcoef=zcoef.to(dt).permute(2, 0, 1).contiguous(), stats=stats, X=X, cout=cout, out=out, hist=hist)


def backsub(hist, broken=None):
    """y = R^-1 phi, z = R^-1 e_J from hist[J, 4, Q, t] (R_ii = gamma_i, R_{i-1,i} = delta_i, R_{i-2,i} = eps_i), in float64 like
    ciq_backsub_kernel -> ([J, Q, t], [J, Q, t]) float64"""
    J = hist.shape[0]
    h = hist.to(f64)
    zero = torch.zeros_like(h[0, 0])
    y, z = [None] * J, [None] * J
    y1 = y2 = z1 = z2 = d1 = e1 = e2 = zero
    for i in range(J - 1, -1, -1):
        epsi, delta, ig, phi = h[i, 0], h[i, 1], h[i, 2], h[i, 3]
        band = zero if broken == "no_eps_band" else e2
        y[i] = (phi - d1 * y1 - band * y2) * ig
        z[i] = ((1.0 if i == J - 1 else 0.0) - d1 * z1 - band * z2) * ig
        y2, y1, z2, z1 = y1, y[i], z1, z[i]
        e2, e1, d1 = e1, epsi, delta
    return torch.stack(y), torch.stack(z)


def stop_iteration(stats, tol, max_iter):
    """the driver's stop: the first tested iteration whose mean statistic is below tol, else max_iter"""
    for it in sorted(stats):
        if it <= max_iter and float(stats[it].to(f64).mean()) < tol:
            return it
    return max_iter


def oracle_solves(K, R, sigma, J):
    """O.msminres (columns) for exactly J iterations -> X [Q, t, n] in the row layout"""
    X, its = O.msminres(K, R.t().contiguous(), sigma.to(R.dtype), tol=-1.0, max_iter=J)
    assert its == J
    return X.transpose(1, 2).contiguous()


def oracle_stat(K, R, sigma, J):
    """the oracle's |upd| / |X| at iteration J, per (shift, row): upd = X_J - X_{J-1}"""
    XJ = oracle_solves(K, R, sigma, J)
    XP = oracle_solves(K, R, sigma, J - 1) if J > 1 else torch.zeros_like(XJ)
    return (XJ - XP).norm(dim=2) / XJ.norm(dim=2).clamp_min(1e-30)


def row_err(a, truth):
    """error per vector (last dimension) relative to that vector's own maximum in the truth -> shape truth.shape[:-1]; a vector
    whose truth is identically zero reports its absolute error"""
    a, truth = a.detach().double().cpu(), truth.detach().double().cpu()
    d = (a - truth).abs().reshape(-1, truth.shape[-1]).amax(1)
    m = truth.abs().reshape(-1, truth.shape[-1]).amax(1)
    return (d / torch.where(m > 0, m, torch.ones_like(m))).reshape(truth.shape[:-1])


# ------------------------------------------------------------------ the matched-iteration cases of tests/test_gpu_ciq_solver.py
# name: (n, t, Q, J, seed); t counts the three edge rows at the end of R.  "single" is t = 1: it runs once per kind of row.
CASES = {
    "odd": (97, 7, 3, 10, 5),               # scalar symv; norms VEC = 1 in float; mix VEC = 1 inside the solve; one G = 1 group; Q t = 21 < 256
    "even_not_x4": (130, 5, 15, 13, 5),     # norms VEC = 2, mix VEC = 1; J off the check_every boundary
    "ragged_trips": (257, 7, 17, 12, 5),    # two trips of the row loops with a 1-element tail; second q0 pass with G = 1
    "long_ragged": (1031, 9, 21, 10, 5),    # five trips; second pass with G = 2; Q t just under 256; the GEMM splits K
    "wide_t": (96, 300, 15, 8, 5),          # Q t = 4500: several blocks of givens / backsub, ragged last block
    "single_random": (64, 1, 15, 8, 5),     # t = 1
    "single_zero": (64, 1, 15, 8, 5),
    "single_gate": (64, 1, 15, 8, 5),
    "single_eig": (64, 1, 15, 8, 5),
    "exhausted": (8, 7, 15, 12, 5),         # J > n: the Krylov space is exhausted
    "padded": (256, 6, 15, 10, 5),          # ldk = n + 3, ldr = n + 1, ldo = n + 5, bases one element in: every 16-byte gate closes
}
STOP_CASES = ("odd", "ragged_trips", "long_ragged")
STOP_MAX_ITER = 60
Y_ORDINARY, Y_GATE = 1e-4, 1e-3


class Case:
    """inputs (float32-rounded, held in float64), the float64 truth and the float32 yardstick run of one case"""

    def __init__(self, name, J=None):
        n, t, Q, J0, seed = CASES[name]
        self.name, self.n, self.t, self.Q, self.J = name, n, t, Q, (J or J0)
        K, lam = spd(n, 30.0, seed)
        g = torch.Generator().manual_seed(seed + 1)
        E = edge_rows(K.float().double())
        if name.startswith("single"):
            R = {"random": torch.randn(1, n, generator=g, dtype=f64), "zero": E[0:1], "gate": E[1:2], "eig": E[2:3]}[name[7:]]
            kinds = [name[7:]]
        else:
            R = torch.cat([torch.randn(t - N_EDGE, n, generator=g, dtype=f64), E])
            kinds = ["random"] * (t - N_EDGE) + ["zero", "gate", "eig"]
        sigma, omega = O.ciq_quadrature(float(lam.min()), float(lam.max()), Q)
        self.K, self.R = K.float().double(), R.float().double()
        self.sigma, self.omega = sigma.float().double(), omega.float().double()
        self.kinds = kinds
        self.rows = {k: [i for i, kk in enumerate(kinds) if kk == k] for k in ("random", "zero", "gate", "eig")}

    @classmethod
    def from_arrays(cls, name, K, R, sigma, omega, J, kinds=None):
        """a case on given float64 arrays (rounded to float32 here), rows all ``random`` unless ``kinds`` says otherwise"""
        c = cls.__new__(cls)
        c.name, c.n, c.t, c.Q, c.J = name, K.shape[0], R.shape[0], sigma.shape[0], J
        c.K, c.R = K.float().double(), R.float().double()
        c.sigma, c.omega = sigma.float().double(), omega.float().double()
        c.kinds = kinds or ["random"] * c.t
        c.rows = {k: [i for i, kk in enumerate(c.kinds) if kk == k] for k in ("random", "zero", "gate", "eig")}
        return c

    def run(self, dtype, check_every=10, broken=None, J=None):
        return restate(self.K.to(dtype), self.R.to(dtype), self.sigma, self.omega, J or self.J, check_every, broken)

    @property
    def truth(self):
        if not hasattr(self, "_truth"):
            self._truth = self.run(f64, 1)
        return self._truth

    @property
    def yard(self):
        if not hasattr(self, "_yard"):
            self._yard = self.run(f32, 1)
        return self._yard

    nperm = 3

    @property
    def yards(self):
        """the float32 run and ``nperm`` more of the SAME problem with its coordinates permuted (K -> P K P^T, R -> R P^T; results
        permuted back): the same operation summed in another order, i.e. further samples of the float32 rounding error.  A kind of
        row that occurs once per case (gate, eigenvector, the one-row cases) would otherwise have a one-sample yardstick."""
        if not hasattr(self, "_yards"):
            runs = [self.yard]
            for i in range(self.nperm):
                perm = torch.randperm(self.n, generator=torch.Generator().manual_seed(77 + i))
                inv = torch.argsort(perm)
                r = restate(self.K[perm][:, perm].float(), self.R[:, perm].float(), self.sigma, self.omega, self.J, 1)
                for k in ("basis", "X", "out"):
                    r[k] = r[k][..., inv]
                runs.append(r)
            self._yards = runs
        return self._yards

    # which entries of which quantity are determined by the inputs (the rest is normalised round-off: a Lanczos vector after a
    # breakdown -- the eigenvector row past q_0, every row past q_{n-1} when J > n -- and what is built on it)
    def defined_basis(self):
        """[J + 1, t] bool"""
        m = torch.ones(self.J + 1, self.t, dtype=torch.bool)
        m[min(self.n, self.J + 1):] = False
        for r in self.rows["eig"]:
            m[1:, r] = False
        for r in self.rows["zero"]:
            m[:, r] = True                                          # exactly zero throughout
        return m

    def defined_steps(self):
        """[J, t] bool for alpha (beta: one step less, its last defined value being round-off)"""
        return self.defined_basis()[:self.J]

    def ratio_rows(self):
        """rows whose statistic is more than round-off (not the eigenvector row; none once the Krylov space is exhausted)"""
        if self.J >= self.n:
            return []
        return self.rows["random"] + self.rows["gate"]

    def admit(self):
        """the four admission conditions (tests/test_ciq_host.py asserts them; returns the yardsticks)"""
        T, Y = self.truth, self.yard
        Xo64 = oracle_solves(self.K, self.R, self.sigma, self.J)
        Xo32 = oracle_solves(self.K.float(), self.R.float(), self.sigma.float(), self.J)
        assert torch.isfinite(Xo32).all(), "float32 oracle run is not finite"
        assert all(torch.isfinite(v).all() for v in (Y["X"], Y["out"], Y["basis"], Y["ycoef"]))
        yo = row_err(Xo32, Xo64).amax(0)                            # per row, worst shift
        yr = torch.maximum(row_err(Y["X"], T["X"]).amax(0), row_err(Y["out"], T["out"]))
        y = torch.maximum(yo, yr)
        for r, k in enumerate(self.kinds):
            lim = Y_GATE if k == "gate" else Y_ORDINARY
            assert y[r] <= lim, "%s row %d (%s): float32 yardstick %.2e above %.0e" % (self.name, r, k, y[r], lim)
        for r in self.rows["zero"]:
            assert T["X"][:, r].abs().max() == 0 and T["out"][r].abs().max() == 0 and Xo64[:, r].abs().max() == 0
            assert T["basis"][:, r].abs().max() == 0
        return y


STOP_AT = {"odd": 20, "ragged_trips": 30, "long_ragged": 40}      # one stop per case, at three different tests


def stop_plan(name, dtype=f64):
    """(case, tol, expected stop iteration, bracket, means) for a stop-iteration case: the restatement's mean statistic at the
    tests of every 10th iteration up to STOP_AT; tol is the geometric mean of the last two, so the solver must pass the test
    before STOP_AT and stop AT it (the GPU run gets max_iter = STOP_MAX_ITER: a later stop shows)"""
    stop = STOP_AT[name]
    c = Case(name, J=stop)
    st = c.run(dtype, 10)["stats"]
    m = {it: float(st[it].to(f64).mean()) for it in sorted(st)}
    tol = math.sqrt(m[stop - 10] * m[stop])
    assert all(m[it] > tol for it in m if it < stop)
    return c, tol, stop, (m[stop - 10] / tol, tol / m[stop]), m


# ------------------------------------------------------------------ the comparison shared by the host and the GPU tests
def bound(y, dtype):
    """float entry points: 4 y + 2e-7 (tests/test_oracle_golden.py, tests/test_gpu_conditioning.py); double entry points against
    the same float64 truth: the float32 yardstick scaled by the ratio of unit round-offs 2^-53 / 2^-24, four shares for the
    kernel and one for the reference's own rounding, plus an absolute floor"""
    return 4.0 * y + 2e-7 if dtype == f32 else 5.0 * y * 2.0 ** -29 + 1e-13


def rel(a, truth):
    a, truth = a.detach().double().cpu(), truth.detach().double().cpu()
    return (a - truth).abs() / torch.where(truth != 0, truth.abs(), torch.ones_like(truth))


def errors(case, got):
    """{quantity: (E, mask)}: E[..., t] the errors of ``got`` against the case's float64 truth (vectors relative to their own
    maximum in the truth, scalars to their own value), mask the entries the inputs determine.  ``got``: rnorm [t],
    basis [J + 1, t, n], ycoef [t, J, Q], X [Q, t, n], out [t, n], ratio [Q, t] and optionally alpha_last, beta_last, beta_prev [t]."""
    T, J, t, n, Q = case.truth, case.J, case.t, case.n, case.Q
    Jd = min(J, n)
    ones = lambda *s: torch.ones(*s, dtype=torch.bool)
    db, ds = case.defined_basis(), case.defined_steps()
    rr = torch.zeros(t, dtype=torch.bool)
    rr[case.ratio_rows()] = True
    E = {
        "rnorm": (rel(got["rnorm"], T["rnorm"]), ones(t)),
        "basis": (row_err(got["basis"], T["basis"]), db),
        "ycoef": (row_err(got["ycoef"][:, :Jd].reshape(t, -1), T["ycoef"][:, :Jd].reshape(t, -1)), ones(t)),
        "X": (row_err(got["X"], T["X"]), ones(Q, t)),
        "out": (row_err(got["out"], T["out"]), ones(t)),
        "ratio": (rel(got["ratio"], T["stats"][J]), rr[None, :].expand(Q, t)),
    }
    if "alpha_last" in got:
        E["alpha_last"] = (rel(got["alpha_last"], T["alpha"][J - 1]), ds[J - 1])
        E["beta_last"] = (rel(got["beta_last"], T["beta"][J - 1]), db[J])
        if J >= 2:
            E["beta_prev"] = (rel(got["beta_prev"], T["beta"][J - 2]), db[J - 1])
    return E


def as_got(res, J):
    """a restate() result in the shape ``errors`` takes"""
    g = {k: res[k] for k in ("rnorm", "basis", "ycoef", "X", "out")}
    g["ratio"] = res["stats"][J]
    g["alpha_last"], g["beta_last"] = res["alpha"][J - 1], res["beta"][J - 1]
    if J >= 2:
        g["beta_prev"] = res["beta"][J - 2]
    return g


def compare(case, got, dtype, where=None):
    """-> {quantity: worst err / bound}; ``where`` (a dict) receives the index of each worst entry.
    The yardstick y of a quantity is one figure per case and kind of row (random, zero, gate, eigenvector): the worst error of the
    float32 restatement runs (Case.yards: the problem and three coordinate permutations of it) over the rows of that kind and over
    the shifts.  Refinements, because a recurrence carries its errors forward: the basis slot j is held to the worst float32 error
    of slots <= j, and the Lanczos coefficients the solve leaves behind (the last alpha, the last two beta) to the worst float32
    error of any coefficient of the J steps.  The statistic is the exception to "one figure per case": see below."""
    Eg = errors(case, got)
    T, J = case.truth, case.J
    db, zero = case.defined_basis(), torch.zeros(())
    Ey, lanczos = None, None
    for Y in case.yards:                                            # elementwise worst over the float32 runs
        e = {k: torch.where(m, v, zero) for k, (v, m) in errors(case, as_got(Y, J)).items()}
        lz = torch.maximum(torch.where(case.defined_steps(), rel(Y["alpha"], T["alpha"]), zero),
                           torch.where(db[1:J + 1], rel(Y["beta"], T["beta"]), zero)).amax(0)
        Ey = e if Ey is None else {k: torch.maximum(Ey[k], e[k]) for k in e}
        lanczos = lz if lanczos is None else torch.maximum(lanczos, lz)
    worst = {}
    for k, (e, mask) in Eg.items():
        ey = lanczos if k in ("alpha_last", "beta_last", "beta_prev") else Ey[k]
        y = torch.zeros_like(e)
        for rows in case.rows.values():
            if not rows:
                continue
            if k == "basis":
                y[:, rows] = torch.cummax(ey[:, rows].amax(1), 0).values[:, None]
            elif k == "ratio":
                # each statistic relative to ITSELF (relative to the row's largest, the shifts of the second pass would vanish: they
                # converge orders of magnitude sooner).  Its float32 error grows by four orders from the smallest shift to the
                # largest, so one figure per case would be the largest shift's: the yardstick of shift q is the worst of shifts
                # q - 2 .. q + 2 over the rows of the kind.
                m = ey[:, rows].amax(1)
                pad = torch.cat([m[:1].expand(2), m, m[-1:].expand(2)])
                y[:, rows] = torch.stack([pad[i:i + m.shape[0]] for i in range(5)]).amax(0)[:, None]
            else:
                y[..., rows] = ey[..., rows].max()
        r = torch.where(mask, e / bound(y, dtype), zero)
        assert not torch.isnan(r).any(), k
        worst[k] = float(r.max())
        if where is not None:
            where[k] = tuple(int(i) for i in torch.unravel_index(r.argmax(), r.shape))
    return worst


def exact_rows_ok(case, got):
    """a zero right-hand side stays exactly zero (solves, sum, basis, statistic); nothing anywhere is NaN or infinite"""
    for k, v in got.items():
        assert torch.isfinite(v).all(), "%s: %s not finite" % (case.name, k)
    for r in case.rows["zero"]:
        for k in ("X", "basis", "ratio"):
            assert got[k][:, r].abs().max() == 0, (case.name, k)
        assert got["out"][r].abs().max() == 0 and got["rnorm"][r] == 1
