"""Deterministic float64 model mode (``ElboEngine64.deterministic`` / ``DSVGP_DETERMINISTIC=1`` / ``dsvgp_set_deterministic``
around the ``*_f64`` entry points): the reference on the CPU is deterministic for a fixed seed; the default float64 engine adds its
split-K slices, column sums, scalar sums and the tiled kernel backward's dP1 through fp64 atomics, whose rounding depends on the
order in which workgroups retire.  With the mode on, every such sum goes through per-workgroup partials in the caller's scratch and
a fixed-order pass (csrc/det64.hip), on one stream: two runs are BITWISE equal.

Stated tolerances (none chosen from what the code gives): the deterministic step is the same step, so its first evaluation meets
the float64 oracle at the tolerances of tests/test_gpu_fp64_step.py / test_gpu_fp64_tiled.py -- loss and predictive mean 1e-9,
gradients 1e-7 relative in max-norm per parameter; the op-level entries meet their default-mode results at the tolerances the
existing op tests apply between two summation orders of the same doubles (kernel backward 1e-11, tests/test_gpu_fp64_tiled.py;
column sums, gemv and the scalar tails 1e-12: plain double sums of O(10^3 .. 10^4) terms of one sign pattern, 1e4 eps = 2e-12
being the worst case bound of a reordered sum)."""
import random

import pytest
import torch

import dsvgp_oracle as O
from test_gpu_fp64 import make_problem64, relmax

pytestmark = pytest.mark.gpu
f64 = torch.float64
EINVAL = -1                                             # DSVGP_EINVAL of include/dsvgp.h


def _engine(dev, variant):
    from dsvgp_amd._step64 import ElboEngine64
    eng = ElboEngine64(dev)
    eng.deterministic = True
    if variant == "python":                             # DSVGP_C_STEP=0: the Python-orchestrated Gram path (_elbo_fast64)
        eng.c_step = False
        eng.fast_min_work = 0
    elif variant == "shared":
        eng.shared_directions = True
    elif variant == "dfree":
        eng.data_outputs = "values"
        eng.fast_min_work = 0
    elif variant == "natural":
        eng.fast_min_work = 0
    return eng


def _problem(variant, N, d, M, p, B):
    """(parameters, x, y, D, num_data, oracle call) of one case"""
    if variant == "natural":
        from test_ngd import make_ngd_problem
        P, x, y, D, nd = make_ngd_problem(N, d, M, p, B, seed=N + d, dtype=f64)
        P["natural_mat"] = 0.5 * (P["natural_mat"] + P["natural_mat"].t())
        return P, x, y, D, nd, O.ngd_loss_and_grads, {}
    P, x, y, D, nd = make_problem64(N, d, M, p, B, seed=N + d)
    if variant == "shared":
        g = torch.Generator().manual_seed(4)
        P["inducing_directions"] = torch.eye(d, dtype=f64)[:p] + 0.2 * torch.randn(p, d, generator=g, dtype=f64)
        P["variational_mean"] = 0.3 * torch.randn(M + p, generator=g, dtype=f64)
        P["chol_variational_covar"] = torch.eye(M + p, dtype=f64) + 0.05 * torch.randn(M + p, M + p, generator=g, dtype=f64)
        return P, x, y, D, nd, O.shared_loss_and_grads, {}
    if variant == "dfree":
        y = y.reshape(B, p + 1)[:, 0].contiguous()
        return P, x, y, D, nd, O.elbo_loss_and_grads, {"data_outputs": "values"}
    return P, x, y, D, nd, O.elbo_loss_and_grads, {}


def _five_steps(dsvgp, dev, variant, P, x, y, D, nd, mll, fast, expect_c_step):
    """five optimisation steps (the float64 fused Adam) from P on one minibatch: losses, first-step outputs, final parameters and the
    last gradients.  The parameters move every step, so every step sums different numbers."""
    names = list(P)
    var_names = [k for k in names if k in ("variational_mean", "chol_variational_covar", "natural_vec", "natural_mat")]
    Pd = {k: torch.nn.Parameter(v.clone().to(dev)) for k, v in P.items()}
    # (natural parameters: Adam's +-lr per entry on the M' x M' precision must leave it positive definite over five steps)
    opts = [dsvgp.optim.make_adam([{"params": [Pd[k] for k in var_names]}], lr=1e-4 if variant == "natural" else 0.01),
            dsvgp.optim.make_adam([{"params": [Pd[k] for k in names if k not in var_names]}], lr=0.01)]
    assert all(isinstance(o, dsvgp.optim.FusedAdam) for o in opts)
    eng = _engine(dev, variant)
    xg, yg, Dg = x.to(dev), y.to(dev), D.to(dev)
    losses, first = [], None
    for step in range(5):
        loss, grads, mu, varn = eng.loss_and_grads({k: v.detach() for k, v in Pd.items()}, xg, yg, Dg, nd, mll, fast=fast)
        assert eng.c_step_used == expect_c_step
        if step == 0:
            first = (loss.clone(), {k: v.clone() for k, v in grads.items()}, mu.clone(), varn.clone())
        losses.append(loss.clone())
        for k in names:
            Pd[k].grad = grads[k].clone()
        for o in opts:
            o.step()
    torch.cuda.synchronize()
    return (torch.stack(losses).cpu(), {k: v.detach().cpu().clone() for k, v in Pd.items()}, {k: v.cpu().clone() for k, v in grads.items()},
            first)


# (variant, N, d, M, p, B, objective, fast, one-call step expected).  B is large enough that every multi-writer site has many
# workgroups on one address: B' >= 1536 columns in up to 64 row chunks of the column sums, hundreds of workgroups on d_hyp / scal,
# 57 sweep groups per tile row of the tiled backward (86 at d = 100).
STEP_CASES = [
    ("c_step", 3000, 5, 200, 2, 512, "ELBO", None, True),
    ("python", 3000, 5, 200, 2, 512, "ELBO", None, False),
    ("c_step", 6000, 20, 260, 5, 1024, "ELBO", None, True),          # M'^3 products that split K
    ("per_output", 3000, 5, 200, 2, 512, "PLL", False, False),
    ("per_output", 3000, 5, 200, 2, 512, "ELBO", False, False),
    ("c_step", 1000, 20, 60, 20, 512, "ELBO", None, True),            # tiled assembly: p > 16, sweeps of 3 column tiles, 57 groups per tile row
    ("per_output", 1000, 20, 60, 20, 512, "PLL", None, False),
    ("c_step", 1000, 100, 40, 20, 512, "ELBO", None, True),           # tiled assembly at packed width 104 > 64: no register sweep
    ("shared", 2000, 5, 150, 2, 512, "ELBO", None, False),
    ("shared", 1000, 24, 40, 17, 256, "PLL", None, False),            # shared directions on the tiled assembly
    ("dfree", 2000, 5, 150, 2, 768, "ELBO", True, False),
    ("dfree", 2000, 5, 150, 2, 768, "ELBO", False, False),
    ("natural", 2000, 5, 150, 2, 512, "ELBO", None, True),
    ("natural", 2000, 5, 150, 2, 512, "PLL", False, False),
]


@pytest.mark.parametrize("variant,N,d,M,p,B,mll,fast,c_step", STEP_CASES)
def test_five_fp64_steps_are_bitwise_reproducible_and_the_same_step(dsvgp, gpu_device, variant, N, d, M, p, B, mll, fast, c_step):
    P, x, y, D, nd, oracle, okw = _problem(variant, N, d, M, p, B)
    l1, P1, g1, first = _five_steps(dsvgp, gpu_device, variant, P, x, y, D, nd, mll, fast, c_step)
    l2, P2, g2, _ = _five_steps(dsvgp, gpu_device, variant, P, x, y, D, nd, mll, fast, c_step)
    assert torch.equal(l1, l2), (l1, l2)
    for k in P1:
        assert torch.equal(P1[k], P2[k]), k
        assert torch.equal(g1[k], g2[k]), k
    # ... and it is the same step, not another one: the first evaluation against the float64 oracle
    l_ref, g_ref, mu_ref, var_ref = oracle(P, x, y, D, nd, mll, **okw)
    loss, grads, mu, varn = first
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref)}
    per_output = varn.numel() > 0                        # (the Gram formulation returns no per-output variances)
    assert per_output == (mll == "PLL" or fast is False or variant == "shared")
    if per_output:
        errs["var"] = relmax(varn, var_ref)
    for k in g_ref:
        if grads[k].numel() and g_ref[k].abs().max().item() > 0.0:
            errs[k] = relmax(grads[k], g_ref[k])
    print("[parity] deterministic fp64 step %s %s %s: %s" % (variant, (N, d, M, p, B), mll, ", ".join("%s %.1e" % kv for kv in errs.items())))
    assert errs["loss"] < 1e-9 and errs["mu"] < 1e-9 and errs.get("var", 0.0) < 1e-9, errs
    assert max(v for k, v in errs.items() if k not in ("loss", "mu", "var")) < 1e-7, errs


def test_default_mode_is_untouched(dsvgp, gpu_device):
    """mode off: the one-call step against the Python-orchestrated path at the C2-like shape, at the tolerance
    tests/test_gpu_fp64_step.py applies between those two (loss, mean 1e-9; gradients 1e-7)"""
    from dsvgp_amd._step64 import ElboEngine64
    P, x, y, D, nd = make_problem64(3000, 5, 200, 2, 512, seed=3005)
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    out = []
    for c_step in (True, False):
        eng = ElboEngine64(gpu_device)
        eng.deterministic = False
        eng.c_step = c_step
        eng.fast_min_work = 0
        loss, grads, mu, _ = eng.loss_and_grads(Pg, x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd, "ELBO")
        torch.cuda.synchronize()
        assert eng.c_step_used == c_step
        out.append((loss.clone(), {k: v.clone() for k, v in grads.items()}, mu.clone()))
    (l1, g1, mu1), (l0, g0, mu0) = out
    errs = {"loss": abs(l1.item() - l0.item()) / abs(l0.item()), "mu": relmax(mu1, mu0)}
    errs.update({k: relmax(g1[k], g0[k]) for k in O.PARAM_NAMES})
    print("[parity] default fp64 mode, one-call step vs Python path: %s" % ", ".join("%s %.1e" % kv for kv in errs.items()))
    assert errs["loss"] < 1e-9 and errs["mu"] < 1e-9, errs
    assert max(errs[k] for k in O.PARAM_NAMES) < 1e-7, errs


def test_a_collective_is_refused_with_a_message_that_says_so(dsvgp, gpu_device):
    from dsvgp_amd._step64 import ElboEngine64

    class TwoRanks:
        world = 2
    P, x, y, D, nd = make_problem64(300, 5, 24, 2, 60, seed=9)
    eng = ElboEngine64(gpu_device)
    eng.deterministic = True
    eng.collective = TwoRanks()
    with pytest.raises(NotImplementedError, match="world > 1"):
        eng.loss_and_grads({k: v.to(gpu_device) for k, v in P.items()}, x.to(gpu_device), y.to(gpu_device), D.to(gpu_device), nd)


# ---- op level, under ctx.set_deterministic(scratch) ----------------------------------------------------------------------------
class _Det:
    def __init__(self, ctx, scratch):
        self.ctx, self.scratch = ctx, scratch

    def __enter__(self):
        self.ctx.set_deterministic(self.scratch)

    def __exit__(self, *a):
        self.ctx.set_deterministic(None)


def _three_ways(dsvgp, dev, call, tol, tag, nbytes=256 << 20):
    """call() -> tuple of tensors: default mode, twice under a large scratch (bitwise equal, equal to the default within tol), twice
    under a 1 MiB scratch -- every scalar-partial launcher fits it, the slabs and partial rows of the shapes below do not, so the
    launchers take fewer chunks / longer sweeps: bitwise equal and correct, no refusal --, and under a 4096-byte scratch (correct, or
    DSVGP_EINVAL -- never atomics)"""
    ctx = dsvgp._ops.Context.get(dev)
    ref = [t.clone() for t in call()]
    big = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with _Det(ctx, big):
        a = [t.clone() for t in call()]
        big.fill_(0x5A)                                 # (nothing is carried in the scratch from call to call)
        b = [t.clone() for t in call()]
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v), tag
    errs = [relmax(u, r) for u, r in zip(a, ref) if r.numel()]
    mid = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    with _Det(ctx, mid):
        c1 = [t.clone() for t in call()]
        mid.fill_(0x5A)
        c2 = [t.clone() for t in call()]
    torch.cuda.synchronize()
    for u, v in zip(c1, c2):
        assert torch.equal(u, v), tag
    errs_mid = [relmax(u, r) for u, r in zip(c1, ref) if r.numel()]
    small = torch.empty(4096, dtype=torch.uint8, device=dev)
    with _Det(ctx, small):
        try:
            c = [t.clone() for t in call()]
            errs_small = [relmax(u, r) for u, r in zip(c, ref) if r.numel()]
        except dsvgp._lib.DsvgpError as e:
            assert "(code %d)" % EINVAL in str(e), e
            errs_small = "DSVGP_EINVAL"
    print("[parity] deterministic %s vs default: %s; 1 MiB scratch: %s; 4096-byte scratch: %s" % (
        tag, ["%.1e" % e for e in errs], ["%.1e" % e for e in errs_mid], errs_small if isinstance(errs_small, str) else ["%.1e" % e for e in errs_small]))
    assert max(errs) < tol, (tag, errs)
    assert max(errs_mid) < tol, (tag, errs_mid)
    if not isinstance(errs_small, str):
        assert max(errs_small) < tol, (tag, errs_small)


# register family (p <= 16) and tiled family (p > 16; the last two at packed widths above 64, where a sweep group adds tile by tile)
BWD_SHAPES = [(200, 512, 5, 2), (60, 400, 20, 16), (60, 512, 20, 20), (150, 130, 24, 17), (150, 130, 100, 17), (40, 512, 100, 20)]


@pytest.mark.parametrize("symmetric", [0, 1])
@pytest.mark.parametrize("n1,n2,d,p", BWD_SHAPES)
def test_kernel_bwd_f64_deterministic(dsvgp, gpu_device, n1, n2, d, p, symmetric):
    ops = dsvgp._ops
    ctx = ops.Context.get(gpu_device)
    if symmetric:
        n2 = n1 = max(n1, 130)
    g = torch.Generator().manual_seed(n1 + 7 * p + d)
    x1, x2 = torch.rand(n1, d, generator=g, dtype=f64), torch.rand(n2, d, generator=g, dtype=f64)
    v1, v2 = torch.randn(n1 * p, d, generator=g, dtype=f64), torch.randn(n2 * p, d, generator=g, dtype=f64)
    ell = 0.9 if d <= 50 else 0.9 * (d / 20.0) ** 0.5
    hyp = torch.tensor([ell, 1.7, 0.1, 0.0], dtype=f64, device=gpu_device)
    x1d = x1.to(gpu_device)
    center = x1d.mean(0).contiguous()
    p1 = ops.pack_points_f64(ctx, x1d, v1.to(gpu_device), p, hyp, center)
    p2 = p1 if symmetric else ops.pack_points_f64(ctx, x2.to(gpu_device), v2.to(gpu_device), p, hyp, center)
    q = p + 1
    G = torch.randn(n1 * q, n2 * q, generator=g, dtype=f64).to(gpu_device)
    if symmetric:
        G = (G + G.t()).contiguous()

    def call():
        dx = torch.zeros(n1, d, dtype=f64, device=gpu_device)
        dv = torch.zeros(n1 * p, d, dtype=f64, device=gpu_device)
        d_hyp = torch.zeros(4, dtype=f64, device=gpu_device)
        ops.kernel_bwd_f64(ctx, G, p1, n1, p2, n2, d, p, hyp, bool(symmetric), dx, dv, d_hyp)
        return dx, dv, d_hyp[:2]
    _three_ways(dsvgp, gpu_device, call, 1e-11, "kernel_bwd_f64 %s symmetric=%d" % ((n1, n2, d, p), symmetric))


def test_column_sums_and_scalar_tails_deterministic(dsvgp, gpu_device):
    ops = dsvgp._ops
    ctx = ops.Context.get(gpu_device)
    g = torch.Generator().manual_seed(8)
    Mp, B, p = 1560, 1024, 5
    Bp = B * (p + 1)
    A = torch.randn(Mp, Bp, generator=g, dtype=f64).to(gpu_device)
    W = torch.randn(Mp, Bp, generator=g, dtype=f64).to(gpu_device)
    m = torch.randn(Mp, generator=g, dtype=f64).to(gpu_device)
    _three_ways(dsvgp, gpu_device, lambda: ops.colstats_f64(ctx, A, W, m), 1e-12, "colstats_f64")
    _three_ways(dsvgp, gpu_device, lambda: (ops.colstats_f64(ctx, A, None, m)[0],), 1e-12, "colstats_f64 (no W)")

    def gemv_t():
        yv = torch.empty(Bp, dtype=f64, device=gpu_device)
        ops.gemv_f64(ctx, A, m, yv, trans=True)
        return (yv,)
    _three_ways(dsvgp, gpu_device, gemv_t, 1e-12, "gemv_f64 transposed")
    hyp = torch.tensor([0.8, 1.3, 0.2, 0.0], dtype=f64, device=gpu_device)
    const = torch.tensor([0.1], dtype=f64, device=gpu_device)
    ncols = 300 * 256 + 17                              # more columns than the 256 workgroups take in one pass
    npts = ncols // (p + 1)
    ncols = npts * (p + 1)
    mu0 = torch.randn(ncols, generator=g, dtype=f64).to(gpu_device)
    yv = torch.randn(ncols, generator=g, dtype=f64).to(gpu_device)
    cs = (0.1 * torch.rand(ncols, generator=g, dtype=f64)).to(gpu_device)
    for mll in (0, 1):
        _three_ways(dsvgp, gpu_device, lambda: ops.likelihood_terms_f64(ctx, mu0, cs, yv, const, p, hyp, mll, float(ncols)), 1e-12,
                    "likelihood_terms_f64 mll_type=%d" % mll)
    tvar = torch.tensor(0.37, dtype=f64, device=gpu_device)
    _three_ways(dsvgp, gpu_device, lambda: ops.elbo_fast_tail_f64(ctx, mu0, yv, const, npts, p, hyp, tvar, float(ncols)), 1e-12,
                "elbo_fast_tail_f64")


# ---- harness level ----------------------------------------------------------------------------------------------------------
def test_train_gp_under_float64_default_is_bitwise_reproducible(dsvgp, gpu_device, monkeypatch):
    """directional_vi.train_gp twice under torch.set_default_dtype(torch.float64) with DSVGP_DETERMINISTIC=1 and the same seeds
    (select_cols_of_y draws from Python's ``random``): every state_dict entry is bitwise equal"""
    from torch.utils.data import TensorDataset
    from dsvgp_amd._step64 import ElboEngine64
    monkeypatch.setenv("DSVGP_DETERMINISTIC", "1")
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        states = []
        for _ in range(2):
            torch.manual_seed(0)
            random.seed(0)
            n, d, M, p, B = 800, 4, 40, 2, 200
            X = torch.rand(n, d)
            Y = O.testfun(X)
            model, lik = dsvgp.train_gp(TensorDataset(X, Y), num_inducing=M, num_directions=p, minibatch_size=B, minibatch_dim=p,
                                        num_epochs=2, seed=0, verbose=False)      # (seed: the minibatch permutation's own generator)
            assert isinstance(model.engine, ElboEngine64) and model.engine.deterministic and model.engine.c_step_used
            sd = {"model." + k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
            sd.update({"likelihood." + k: v.detach().cpu().clone() for k, v in lik.state_dict().items()})
            states.append(sd)
        assert set(states[0]) == set(states[1]) and len(states[0]) >= 7
        for k in states[0]:
            assert states[0][k].dtype == f64 or not states[0][k].is_floating_point(), k
            assert torch.equal(states[0][k], states[1][k]), k
    finally:
        torch.set_default_dtype(prev)
