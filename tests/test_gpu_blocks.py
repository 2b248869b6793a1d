"""Per-point predictive covariance blocks: ``dsvgp_predictive_blocks`` (csrc/predict_blocks.hip), ``ElboEngine.predict_blocks``,
``PredictiveDistribution.point_covariances``, ``ApproximateGP.posterior_gradient`` and ``eval_gradients``.

The yardstick is the float64 one of tests/test_gpu_rect_predict.py (``rect_predictive``): the blocks are the q x q diagonal blocks of its
Sigma (tests/test_abi_blocks.py pins them to the oracle).  The CPU tests here show that the yardstick moves every block away from its
prior and that the formula in float32 stays within 1.8e-6 of it; the GPU tests hold the HIP path to it at the project's own tolerances
for these quantities (tests/test_gpu_rect_predict.py, tests/test_gpu_step.py: mean 2e-4, covariance 5e-4, diagonal against the
variances 1e-4), relative in max-norm over the whole output.  Measured errors are printed as [parity] lines."""
import ctypes as C
import functools

import pytest
import torch

import dsvgp_oracle as O
from test_gpu_rect_predict import _case, rect_kernel, rect_predictive, relmax
from test_gpu_step import make_problem

gpu = pytest.mark.gpu
TOL, CTOL, DTOL = 2e-4, 5e-4, 1e-4

#        d    M   p  pd    B    N
SHAPES = [(5, 40, 2, 0, 128, 600),        # q = 1: the blocks are the variances
          (5, 40, 2, 2, 128, 600),        # pd = p: the square K_ZX path
          (5, 40, 2, 5, 67, 600),         # q = 6: 16 points per group, ragged last group
          (3, 33, 3, 1, 70, 300),         # q = 2: 48 points per group (and two row slices)
          (5, 19, 0, 5, 67, 300),         # plain SVGP model, gradient blocks
          (20, 64, 5, 20, 33, 900),       # q = 21: four points per group, a strip of 84 columns; full gradient at the C4 width
          (200, 24, 3, 7, 40, 400),       # wide inputs: the direction Gram over a packed width > 96
          (100, 9, 2, 95, 5, 300),        # q = 96: one point per group, all 21 tile pairs
          (5, 400, 2, 5, 9, 900)]         # M' = 1200 with a single group: ten row slices (dsvgp_predictive_blocks_workspace_bytes)
IDS = ["d%d-M%d-p%d-pd%d-B%d" % s[:5] for s in SHAPES]


def _report(tag, errs):
    print("[parity] %s: %s" % (tag, ", ".join("%s %.2e" % (k, v) for k, v in errs.items())))


# ------------------------------------------------------------------ the yardstick
def diag_blocks(Sigma, B, q):
    """[B, q, q]: the diagonal q x q blocks of a [B q, B q] matrix"""
    i = torch.arange(B)
    return Sigma.reshape(B, q, B, q)[i, :, i, :]


def prior_blocks(P64, D, B, pd):
    """s K_bb + 1e-4 I, K_bb = [[1, 0], [0, v^_a . v^_b / ell^2]]: the RBF block at r = 0 (RBFKernelDirectionalGrad.py:96-102 with
    x1 = x2), written out here independently of ``rect_kernel``"""
    ell, s, _ = O.constrained(P64)
    q = pd + 1
    K = torch.zeros(B, q, q, dtype=torch.float64)
    K[:, 0, 0] = 1.0
    if pd:
        Vh = D.reshape(B, pd, -1)
        Vh = Vh / Vh.norm(dim=2, keepdim=True)
        K[:, 1:, 1:] = Vh @ Vh.transpose(1, 2) / ell ** 2
    return s * K + O.KXX_JITTER * torch.eye(q, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _blocks_case(d, M, p, pd, B, N):
    """(blocks fp64 without noise, prior blocks, A, W fp64): once per shape, shared, never changed"""
    P, x, D, _, Sigma, _, _, _ = _case(d, M, p, pd, B, N)
    P64 = {k: v.double() for k, v in P.items()}
    ell, s, _ = O.constrained(P64)
    Z, V = P64["inducing_points"], P64["inducing_directions"]
    K_ZZ = s * O.kernel_matrix(Z, Z, V, V, ell)
    L = O.psd_safe_cholesky(K_ZZ + O.KZZ_JITTER * torch.eye(K_ZZ.shape[0], dtype=K_ZZ.dtype))
    A = torch.linalg.solve_triangular(L, s * rect_kernel(Z, V, p, x.double(), D.double(), pd, ell), upper=False)
    W = torch.tril(P64["chol_variational_covar"]).t() @ A
    return diag_blocks(Sigma, B, pd + 1), prior_blocks(P64, D.double(), B, pd), A, W


def _slices(Mp, B, pd):
    """(rows per slice, slices) of the kernel's row split (csrc/pred_blocks_plan.h): about 1024 workgroups, at least 128 rows, at most 32"""
    G = max(1, 96 // (pd + 1))
    ngroups = (B + G - 1) // G
    ns = max(1, min((1024 + ngroups - 1) // ngroups, (Mp + 127) // 128, 32))
    rps = ((Mp + ns - 1) // ns + 31) // 32 * 32
    return rps, (Mp + rps - 1) // rps


def _offdiag_max(T):
    q = T.shape[-1]
    return (T * (1.0 - torch.eye(q, dtype=T.dtype))).abs().max().item()


# ------------------------------------------------------------------ CPU: the yardstick is not trivial, and float32 carries it
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_yardstick_moves_every_block_and_float32_carries_it(shape):
    d, M, p, pd, B, N = shape
    ref, prior, A, W = _blocks_case(*shape)
    q = pd + 1
    top = ref.abs().max().item()
    change = (ref - prior).abs().amax(dim=(1, 2)) / top                 # per block
    errs = {"largest change / max|block|": change.max().item(), "smallest per-block change": change.min().item()}
    assert ref.shape == (B, q, q) and bool((change > 0).all())
    assert 0.05 <= errs["largest change / max|block|"] <= 0.24, errs
    if pd >= 1:
        errs["off-diagonal change / max|block|"] = _offdiag_max(ref - prior) / top
        # (7.8e-3 is the smallest of the nine, 7.79e-3 at q = 96, as the two digits it is stated with: compared at those two digits)
        assert float("%.1e" % errs["off-diagonal change / max|block|"]) >= 7.8e-3, errs
    # the formula in float32: A, W rounded to float, the Gram in float -- in the kernel's own order, so that the figure does not depend
    # on the host's BLAS: per row slice one fmaf chain per entry (the W term, then the A term of every 4 rows), slices added in order
    A32, W32 = A.float().reshape(-1, B, q).permute(1, 0, 2), W.float().reshape(-1, B, q).permute(1, 0, 2)      # [B, Mp, q]
    rps, nslices = _slices(A.shape[0], B, pd)
    fma = lambda acc, u, sign: (acc.double() + sign * u.double().unsqueeze(2) * u.double().unsqueeze(1)).float()
    sq = torch.zeros(B, q, q)
    for s0 in range(0, A.shape[0], rps):
        acc = torch.zeros(B, q, q)
        for k0 in range(s0, min(s0 + rps, A.shape[0]), 4):
            for X, sign in ((W32, 1.0), (A32, -1.0)):
                for i in range(k0, min(k0 + 4, s0 + rps, A.shape[0])):
                    acc = fma(acc, X[:, i], sign)
        sq = sq + acc
    emu = prior.float() + sq
    errs["float32 emulation"] = relmax(emu, ref)
    _report("yardstick d=%d M=%d p=%d pd=%d B=%d" % shape[:5], errs)
    assert errs["float32 emulation"] <= 1.8e-6, errs


def test_the_helper_reports_one_slab_per_row_slice(dsvgp):
    """the last shape is there for the row split: it takes ten slices (more than one), the fourth and the sixth two and three"""
    ws = dsvgp._lib.lib.dsvgp_predictive_blocks_workspace_bytes
    for (d, M, p, pd, B, N), want in zip(SHAPES, (1, 1, 1, 2, 1, 3, 1, 1, 10)):
        Mp, q = M * (p + 1), pd + 1
        assert _slices(Mp, B, pd)[1] == want and ws(Mp, B, pd) == want * B * q * q * 4


# ------------------------------------------------------------------ GPU 1: entry and engine against float64
def _hyp(P, dev):
    ell, s, noise = O.constrained({k: v.double() for k, v in P.items()})
    return torch.tensor([float(ell), float(s), float(noise), 0.0], dtype=torch.float32, device=dev)


def _entry_operands(dsvgp, dev, shape):
    """A, W of the yardstick rounded to float on the device, the data pack, hyp"""
    d, M, p, pd, B, N = shape
    P, x, D, *_ = _case(*shape)
    _, _, A, W = _blocks_case(*shape)
    ops = dsvgp._ops
    ctx = ops.Context.get(dev)
    hyp = _hyp(P, dev)
    center = ops.column_mean(ctx, P["inducing_points"].to(dev).contiguous())
    px = ops.pack_points(ctx, x.to(dev).contiguous(), D.to(dev).contiguous() if pd else None, pd, hyp, center)
    return ops, ctx, hyp, px, A.float().to(dev).contiguous(), W.float().to(dev).contiguous()


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_entry_and_engine_match_fp64(dsvgp, gpu_device, shape):
    d, M, p, pd, B, N = shape
    dev = gpu_device
    P, x, D, mu_ref, Sig_ref, _, noise, c = _case(*shape)
    ref, prior, _, _ = _blocks_case(*shape)
    q = pd + 1
    eye = torch.eye(q, dtype=torch.float64)
    if pd >= 1:     # ten times the tolerance: a kernel that returns the prior block, or the diagonal alone, cannot pass
        assert _offdiag_max(ref - prior) >= 5e-3 * ref.abs().max().item()
    ops, ctx, hyp, px, A, W = _entry_operands(dsvgp, dev, shape)
    entry = ops.predictive_blocks(ctx, A, W, pd, px, d, hyp, True)
    eng = dsvgp.ElboEngine(dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    xg, Dg = x.to(dev), (D.to(dev) if pd else None)
    mu, blocks = eng.predict_blocks(Pg, xg, Dg)
    _, varn = eng.predict(Pg, xg, Dg)
    _, Sigma = eng.predict_joint(Pg, xg, Dg)
    errs = {"entry": relmax(entry, ref + noise * eye), "mean": relmax(mu, mu_ref), "blocks": relmax(blocks, ref + noise * eye),
            "diagonals vs predict": relmax(blocks.diagonal(dim1=1, dim2=2).reshape(-1), varn),
            "blocks vs predict_joint": relmax(blocks, diag_blocks(Sigma.cpu(), B, q)),
            "entry off-diagonal": _offdiag_max(entry.double().cpu() - ref) / ref.abs().max().item()}
    _report("predict_blocks d=%d M=%d p=%d pd=%d B=%d" % shape[:5], errs)
    assert entry.shape == blocks.shape == (B, q, q) and blocks.dtype == torch.float32 and mu.shape == (B * q,)
    assert errs["entry"] < CTOL and errs["blocks"] < CTOL and errs["blocks vs predict_joint"] < CTOL, errs
    assert errs["mean"] < TOL and errs["diagonals vs predict"] < DTOL, errs


# ------------------------------------------------------------------ GPU 2: exact properties
@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_blocks_are_exactly_symmetric_and_noise_sits_on_the_diagonals(dsvgp, gpu_device, shape):
    d, M, p, pd, B, N = shape
    ops, ctx, hyp, px, A, W = _entry_operands(dsvgp, gpu_device, shape)
    q = pd + 1
    b1 = ops.predictive_blocks(ctx, A, W, pd, px, d, hyp, True)
    b0 = ops.predictive_blocks(ctx, A, W, pd, px, d, hyp, False)
    assert torch.equal(b1, b1.transpose(1, 2)) and torch.equal(b0, b0.transpose(1, 2))
    off = 1.0 - torch.eye(q, device=gpu_device)
    assert torch.equal(b1 * off, b0 * off)                                            # off the diagonals: the same bits
    d1, d0 = b1.diagonal(dim1=1, dim2=2), b0.diagonal(dim1=1, dim2=2)
    assert ((d1 - (d0 + hyp[2])).abs().max() <= 2.0 ** -23 * d1.abs().max()).item()   # on them: + hyp[2], one rounding
    assert bool((d1 > d0).all())


@gpu
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[8]], ids=[IDS[2], IDS[8]])
def test_two_identical_calls_are_bitwise_equal(dsvgp, gpu_device, shape):
    d, M, p, pd, B, N = shape
    ops, ctx, hyp, px, A, W = _entry_operands(dsvgp, gpu_device, shape)
    e1, e2 = ops.predictive_blocks(ctx, A, W, pd, px, d, hyp, True), ops.predictive_blocks(ctx, A, W, pd, px, d, hyp, True)
    assert torch.equal(e1, e2)
    # the engine: the blocks are a function of the A and W it holds -- the same bits as the entry on those buffers, and the same bits
    # from call to call whenever A and W are.  (At M' = 1200 they are not: A = L^-1 K_ZX and W = L_S^T A come from the existing fp64
    # solve and split-K product, whose partial sums meet in atomics outside the training step's deterministic mode; predict's
    # variances move in their last bits with them.  That is not this change's to settle: what it adds is reproducible.)
    P, x, D, *_ = _case(*shape)
    eng = dsvgp.ElboEngine(gpu_device)
    Pg = {k: v.to(gpu_device) for k, v in P.items()}
    runs = []
    hyp_e = ops.hyp_forward(ctx, Pg["raw_lengthscale"], Pg["raw_outputscale"], Pg["raw_noise"])       # (the engine's own float32 values)
    for _ in range(2):
        m, b = eng.predict_blocks(Pg, x.to(gpu_device), D.to(gpu_device))
        A32, W32 = eng._buf["A32"].clone(), eng._buf["W"].clone()
        px2 = ops.pack_points(ctx, x.to(gpu_device).contiguous(), D.to(gpu_device).contiguous(), pd, hyp_e, eng.center)
        assert torch.equal(b, ops.predictive_blocks(ctx, A32, W32, pd, px2, d, hyp_e, True))
        runs.append((m, b, A32, W32))
    (m1, b1, A1, W1), (m2, b2, A2, W2) = runs
    same = torch.equal(A1, A2) and torch.equal(W1, W2)
    print("[parity] M' = %d: A and W bitwise equal between two engine calls: %s, mean: %s, blocks: %s" % (
        A1.shape[0], same, torch.equal(m1, m2), torch.equal(b1, b2)))
    assert (torch.equal(b1, b2) and torch.equal(m1, m2)) or not same
    assert relmax(b1, b2) < 1e-5 and relmax(m1, m2) < 1e-5                          # (last bits of the operands, nothing more)


@gpu
def test_out_is_written_inside_its_bounds_only(dsvgp, gpu_device):
    shape = SHAPES[2]
    d, M, p, pd, B, N = shape
    ops, ctx, hyp, px, A, W = _entry_operands(dsvgp, gpu_device, shape)
    q = pd + 1
    buf = torch.full((B + 2, q, q), float("nan"), device=gpu_device)
    out = ops.predictive_blocks(ctx, A, W, pd, px, d, hyp, True, out=buf[1:B + 1])
    assert out.data_ptr() == buf[1].data_ptr() and bool(torch.isfinite(buf[1:B + 1]).all())
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[B + 1]).all())
    assert torch.equal(out, ops.predictive_blocks(ctx, A, W, pd, px, d, hyp, True))
    with pytest.raises(ValueError):
        ops.predictive_blocks(ctx, A, W, pd, px, d, hyp, True, out=buf[:B, :, :q - 1])
    with pytest.raises(ValueError):
        ops.predictive_blocks(ctx, A, W[:, :-1], pd, px, d, hyp, True)
    with pytest.raises(ValueError):
        ops.predictive_blocks(ctx, A, W, pd, None, d, hyp, True)


# ------------------------------------------------------------------ GPU 3: variants
@gpu
def test_natural_parameters(dsvgp, gpu_device):
    from test_ngd import make_ngd_problem
    dev = gpu_device
    B, pd = 128, 3
    P, x, _, _, _ = make_ngd_problem(600, 5, 40, 2, B)
    D = torch.randn(B * pd, 5, generator=torch.Generator().manual_seed(5))
    P64 = {k: v.double() for k, v in P.items()}
    m, LS = O.natural_to_mu_chol(P64["natural_vec"], P64["natural_mat"])
    Pc = {k: v for k, v in P64.items() if not k.startswith("natural_")}
    Pc["variational_mean"], Pc["chol_variational_covar"] = m, LS
    mu_ref, Sig_ref, _ = rect_predictive(Pc, x.double(), D.double(), pd)
    noise = float(O.constrained(P64)[2])
    mu, blocks = dsvgp.ElboEngine(dev).predict_blocks({k: v.to(dev) for k, v in P.items()}, x.to(dev), D.to(dev))
    errs = {"mean": relmax(mu, mu_ref), "blocks": relmax(blocks, diag_blocks(Sig_ref, B, pd + 1) + noise * torch.eye(pd + 1, dtype=torch.float64))}
    _report("natural parameters, pd = 3", errs)
    assert blocks.shape == (B, 4, 4) and errs["mean"] < TOL and errs["blocks"] < CTOL, errs


@gpu
def test_shared_directions_have_a_zero_middle_term(dsvgp, gpu_device):
    dev = gpu_device
    N, d, M, p, B, pd = 600, 5, 40, 2, 128, 3
    P, x, _, _, _ = make_problem(N, d, M, p, B, seed=1)
    g = torch.Generator().manual_seed(4)
    P["inducing_directions"] = torch.eye(d)[:p] + 0.2 * torch.randn(p, d, generator=g)        # ONE shared set
    P["variational_mean"] = 0.3 * torch.randn(M + p, generator=g)
    P["chol_variational_covar"] = torch.eye(M + p) + 0.05 * torch.randn(M + p, M + p, generator=g)
    D = torch.randn(B * pd, d, generator=torch.Generator().manual_seed(5))
    P64 = {k: v.double() for k, v in P.items()}
    V, iv = O.shared_expand(P64["inducing_directions"], P64["variational_mean"], M)
    Q = dict(P64)
    Q["inducing_directions"], Q["variational_mean"] = V, iv
    Q["chol_variational_covar"] = torch.eye(iv.shape[0], dtype=torch.float64)      # zero middle term: S - I = 0
    mu_ref, Sig_ref, _ = rect_predictive(Q, x.double(), D.double(), pd)
    noise = float(O.constrained(P64)[2])
    eng = dsvgp.ElboEngine(dev)
    eng.shared_directions = True
    mu, blocks = eng.predict_blocks({k: v.to(dev) for k, v in P.items()}, x.to(dev), D.to(dev))
    q = pd + 1
    ref = diag_blocks(Sig_ref, B, q) + noise * torch.eye(q, dtype=torch.float64)
    errs = {"mean": relmax(mu, mu_ref), "blocks": relmax(blocks, ref)}
    _report("shared directions, pd = 3", errs)
    assert blocks.shape == (B, q, q) and errs["mean"] < TOL and errs["blocks"] < CTOL, errs
    # the entry: W == A gives the bits of W == NULL (the middle term is not computed as a difference), and they are the prior blocks
    ops, ctx, hyp, px, A, _ = _entry_operands(dsvgp, dev, SHAPES[2])
    dd, _, _, pd2, B2, _ = SHAPES[2]
    none, same = ops.predictive_blocks(ctx, A, None, pd2, px, dd, hyp, True), ops.predictive_blocks(ctx, A, A, pd2, px, dd, hyp, True)
    assert torch.equal(none, same)
    P2, _, D2, *_ = _case(*SHAPES[2])
    P2 = {k: v.double() for k, v in P2.items()}
    want = prior_blocks(P2, D2.double(), B2, pd2) + float(O.constrained(P2)[2]) * torch.eye(pd2 + 1, dtype=torch.float64)
    assert relmax(none, want) < 2e-6


@gpu
def test_derivative_free_data_give_the_variances(dsvgp, gpu_device):
    dev = gpu_device
    P, x, _, D, _ = make_problem(600, 5, 40, 2, 128, seed=1)
    _, _, _, _, Sig_ref, _, noise, _ = _case(*SHAPES[0])                              # (the same problem at pd = 0)
    eng = dsvgp.ElboEngine(dev)
    eng.data_outputs = "values"
    Pg = {k: v.to(dev) for k, v in P.items()}
    mu, blocks = eng.predict_blocks(Pg, x.to(dev), D.to(dev))                         # (the model's own count, ignored)
    _, varn = eng.predict(Pg, x.to(dev), D.to(dev))
    errs = {"blocks": relmax(blocks.reshape(-1), Sig_ref.diagonal() + noise), "vs predict": relmax(blocks.reshape(-1), varn)}
    _report("data_outputs == 'values'", errs)
    assert blocks.shape == (128, 1, 1) and mu.shape == (128,) and errs["blocks"] < CTOL and errs["vs predict"] < DTOL, errs


@gpu
def test_evaluation_cache_is_shared_with_predict(dsvgp, gpu_device):
    dev = gpu_device
    P, x, D, *_ = _case(*SHAPES[2])
    Pg = {k: v.to(dev) for k, v in P.items()}
    xg, Dg = x.to(dev), D.to(dev)
    mu0, b0 = dsvgp.ElboEngine(dev).predict_blocks(Pg, xg, Dg, cache=False)
    eng = dsvgp.ElboEngine(dev)
    eng.predict(Pg, xg, Dg, cache=True)
    key = eng._eval_cache[0]
    mu1, b1 = eng.predict_blocks(Pg, xg, Dg, cache=True)
    assert eng._eval_cache[0] == key                                                  # a hit: the factor was not rebuilt
    assert torch.equal(mu0, mu1) and torch.equal(b0, b1)


# ------------------------------------------------------------------ GPU 4: nothing of size B' x B'
@gpu
def test_nothing_of_the_size_of_the_joint_covariance_is_allocated(dsvgp, gpu_device):
    """d 5, M 16, p 1, pd 5, B 4096: the joint covariance would be 24 576^2 floats = 2.4 GB.  One call may raise the peak by 512 MB: a
    fifth of the joint, four times what K_ZX, A (fp64 + fp32), W, the pack and the solve workspace need by their own size formulas"""
    dev = gpu_device
    d, M, p, pd, B = 5, 16, 1, 5, 4096
    P, x, _, _, _ = make_problem(4200, d, M, p, B, seed=1)
    D = torch.randn(B * pd, d, generator=torch.Generator().manual_seed(5))
    eng = dsvgp.ElboEngine(dev)
    Pg = {k: v.to(dev) for k, v in P.items()}
    xg, Dg = x.to(dev), D.to(dev)
    eng.predict_blocks(Pg, xg, Dg)                                                    # warm-up: the engine's buffers exist
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.max_memory_allocated(dev)
    mu, blocks = eng.predict_blocks(Pg, xg, Dg)
    torch.cuda.synchronize()
    raised = torch.cuda.max_memory_allocated(dev) - before
    print("[parity] peak raised by %.1f MB (joint covariance: %.1f MB)" % (raised / 2 ** 20, (B * (pd + 1)) ** 2 * 4 / 2 ** 20))
    assert blocks.shape == (4096, 6, 6) and mu.shape == (4096 * 6,) and bool(torch.isfinite(blocks).all())
    assert raised <= 512 * 2 ** 20


# ------------------------------------------------------------------ GPU 5: model and harness
@pytest.fixture(scope="module")
def trained(dsvgp, gpu_device):
    """the 600-point, d = 2 drop-in run of tests/test_gpu_rect_predict.py, one epoch: a p = 2 model and a plain SVGP (p = 0)"""
    from torch.utils.data import TensorDataset
    torch.manual_seed(0)
    n, dim, n_test = 600, 2, 300
    train_x, test_x = torch.rand(n, dim), torch.rand(n_test, dim)
    train_y, test_y = O.testfun(train_x), O.testfun(test_x)
    model, likelihood = dsvgp.train_gp(TensorDataset(train_x, train_y), num_inducing=20, num_directions=2, minibatch_size=200,
                                       minibatch_dim=2, num_epochs=1, inducing_data_initialization=False, tqdm=False,
                                       verbose=False, seed=0)
    plain, plain_lik = dsvgp.traditional_vi.train_gp(TensorDataset(train_x, train_y[:, 0].contiguous()), dim, num_inducing=20,
                                                     minibatch_size=200, num_epochs=1, tqdm=False, verbose=False, seed=0)
    for m in (model, likelihood, plain, plain_lik):
        m.eval()
    return model, likelihood, plain, plain_lik, test_x, test_y


def _model_yardstick(model, likelihood, x, D, pd):
    P64 = {k: v.detach().double().cpu() for k, v in model._param_dict(likelihood).items()}
    mu, Sigma, _ = rect_predictive(P64, x.double().cpu(), D.double().cpu(), pd)
    return mu, Sigma, float(O.constrained(P64)[2])


@gpu
def test_point_covariances_are_the_diagonal_blocks_of_the_covariance_matrix(trained, gpu_device):
    model, likelihood, _, _, test_x, _ = trained
    B = 100
    xg = test_x[:B].to(gpu_device)
    eye = torch.eye(3)
    errs = {}
    with torch.no_grad():
        for name, D in (("pd = p", torch.eye(2, device=gpu_device).repeat(B, 1)), ("pd = 1", torch.eye(2, device=gpu_device)[:1].repeat(B, 1)),
                        ("pd = 0", None)):
            q = (D.shape[0] // B if D is not None else 0) + 1
            with_lik, without = model.posterior(xg, D, likelihood), model.posterior(xg, D)
            bl, bf = with_lik.point_covariances, without.point_covariances
            assert bl.shape == bf.shape == (B, q, q) and with_lik.mean.shape == (B * q,)
            errs[name + " with likelihood"] = relmax(bl, diag_blocks(with_lik.covariance_matrix.cpu(), B, q))
            errs[name + " q(f)"] = relmax(bf, diag_blocks(without.covariance_matrix.cpu(), B, q))
            # q(f) itself: what ``_ensure_joint`` takes off the diagonal (the noise, softplus + its 1e-4 floor) is taken off here
            errs[name + " noise"] = relmax((bl - bf).cpu(), float(likelihood.noise.detach().reshape(())) * eye[:q, :q].expand(B, q, q))
        # what model(x, derivative_directions=D) and likelihood(model(...)) return carries the property too
        D = torch.eye(2, device=gpu_device).repeat(B, 1)
        old = likelihood(model(xg, derivative_directions=D))
        errs["likelihood(model(x, D))"] = relmax(old.point_covariances, diag_blocks(old.covariance_matrix.cpu(), B, 3))
        f = model(xg, derivative_directions=D)
        errs["model(x, D)"] = relmax(f.point_covariances, diag_blocks(f.covariance_matrix.cpu(), B, 3))
        fresh = likelihood(model(xg, derivative_directions=D))
        fresh.point_covariances
        assert torch.equal(fresh.mean, old.mean)                                     # (the property fills the mean)
    _report("point_covariances", errs)
    assert all(v < CTOL for k, v in errs.items() if "noise" not in k) and all(v < 1e-3 for k, v in errs.items() if "noise" in k), errs


@gpu
@pytest.mark.parametrize("which", ["p2", "p0"])
def test_posterior_gradient(trained, gpu_device, which):
    model, likelihood, plain, plain_lik, test_x, _ = trained
    if which == "p0":
        model, likelihood = plain, plain_lik
    B, d = 100, 2
    xg = test_x[:B].to(gpu_device)
    with torch.no_grad():
        pg = model.posterior_gradient(xg, likelihood)
        var = model.posterior(xg, None, likelihood).variance
    mu_ref, Sig_ref, noise = _model_yardstick(model, likelihood, xg, torch.eye(d).repeat(B, 1), d)
    ref = diag_blocks(Sig_ref, B, d + 1) + noise * torch.eye(d + 1, dtype=torch.float64)
    errs = {"value mean": relmax(pg.value_mean, mu_ref.reshape(B, d + 1)[:, 0]),
            "gradient mean": relmax(pg.gradient_mean, mu_ref.reshape(B, d + 1)[:, 1:]),
            "gradient covariance": relmax(pg.gradient_covariance, ref[:, 1:, 1:]),
            "value-gradient covariance": relmax(pg.value_gradient_covariance, ref[:, 1:, 0]),
            "value variance vs posterior": relmax(pg.value_variance, var)}
    _report("posterior_gradient, model trained with %s" % which, errs)
    assert pg._fields == ("value_mean", "value_variance", "gradient_mean", "gradient_covariance", "value_gradient_covariance")
    assert pg.value_mean.shape == pg.value_variance.shape == (B,) and pg.gradient_mean.shape == pg.value_gradient_covariance.shape == (B, d)
    assert pg.gradient_covariance.shape == (B, d, d)
    assert errs["value mean"] < TOL and errs["gradient mean"] < TOL and errs["value variance vs posterior"] < DTOL, errs
    assert errs["gradient covariance"] < CTOL and errs["value-gradient covariance"] < CTOL, errs


@gpu
def test_eval_gradients_is_the_per_batch_calls_concatenated(dsvgp, trained, gpu_device):
    from torch.utils.data import TensorDataset
    model, likelihood, _, _, test_x, test_y = trained
    n = 200
    out = dsvgp.eval_gradients(TensorDataset(test_x[:n], test_y[:n]), model, likelihood, minibatch_size=128)
    with torch.no_grad():
        a, b = model.posterior_gradient(test_x[:128].to(gpu_device), likelihood), model.posterior_gradient(test_x[128:n].to(gpu_device), likelihood)
    assert out._fields == a._fields and out.gradient_covariance.shape == (n, 2, 2) and out.value_mean.is_cuda
    for got, first, second in zip(out, a, b):
        assert torch.equal(got, torch.cat([first, second]))


# ------------------------------------------------------------------ GPU 6: refusals
@gpu
def test_refusals(dsvgp, gpu_device, trained):
    """every refused call returns before a launch"""
    from dsvgp_amd._step64 import ElboEngine64
    from test_ngd import make_ngd_problem
    dev = gpu_device
    Pn, xn, _, _, _ = make_ngd_problem(300, 3, 12, 2, 20)
    eng = dsvgp.ElboEngine(dev)
    eng.whitening = "ciq"
    with pytest.raises(ValueError, match="CIQ"):
        eng.predict_blocks({k: v.to(dev) for k, v in Pn.items()}, xn.to(dev), None)
    with pytest.raises(NotImplementedError, match="float64"):
        ElboEngine64(dev).predict_blocks({k: v.double().to(dev) for k, v in Pn.items()}, xn.double().to(dev), None)
    with pytest.raises(ValueError, match="at most 95"):
        trained[0].posterior_gradient(torch.zeros(4, 96, device=dev))
    # the C entry
    shape = SHAPES[2]
    d, M, p, pd, B, N = shape
    ops, ctx, hyp, px, A, W = _entry_operands(dsvgp, dev, shape)
    lib = dsvgp._lib.lib
    Mp, nc, q = A.shape[0], A.shape[1], pd + 1
    need = int(lib.dsvgp_predictive_blocks_workspace_bytes(Mp, B, pd))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(B, q, q, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)

    def entry(A_=A, W_=W, lda=nc, ldw=nc, Mp_=Mp, B_=B, pd_=pd, PX=px[0], d_=d, hyp_=hyp, out_=out, nbytes=need):
        return lib.dsvgp_predictive_blocks(ctx.h, vp(A_), lda, vp(W_), ldw, Mp_, B_, pd_, vp(PX), d_, vp(hyp_), 1, vp(out_), vp(ws), nbytes)

    assert entry() == 0
    assert entry(A_=None) == -1 and entry(out_=None) == -1 and entry(hyp_=None) == -1 and entry(PX=None) == -1
    assert entry(Mp_=0) == -1 and entry(B_=0) == -1 and entry(d_=0) == -1 and entry(pd_=-1) == -1 and entry(pd_=96) == -1
    assert entry(lda=nc - 1) == -1 and entry(ldw=nc - 1) == -1 and entry(nbytes=need - 1) == -1
    assert entry(W_=None, ldw=0) == 0                                                 # (no W: its leading dimension is not read)
    torch.cuda.synchronize()
    assert torch.equal(out, ops.predictive_blocks(ctx, A, None, pd, px, d, hyp, True))
