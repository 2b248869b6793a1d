"""Gradients of the collapsed bound on the GPU (csrc/collapsed.hip: dsvgp_collapsed_grad_prepare / _chunk; ``CollapsedAccumulator.begin_backward``
/ ``add_backward`` / ``finish_backward``; ``collapsed_loss_and_grads``; ``train_collapsed``) against the float64 autograd yardstick of
tests/_collapsed_grad_ref.py and against the engine's own piecewise step at the optimum.

Cases are those of tests/_collapsed_ref.py as they are: M' = 72 / 129 / 65 (one row past a 64-tile, past two), B' ragged past a 64-tile
(and past the 256-column workgroups of the new kernels: 450, 609, 485), rectangular data (values only, pd = d), the wide route (d = 100), ARD
and Matern-5/2.

Bounds.  Every returned tensor: max |g - g_ref| <= 2e-3 max |g_ref| (GRAD_TOL: what the step's gradients are held to in
tests/test_gpu_rect_train.py / test_gpu_ard.py / test_gpu_matern.py); the loss 2e-5 relative (LOSS_TOL, same files).  Two backward passes
from one solved accumulator are bitwise equal at the shapes run here (asserted), and within 1e-6 of the largest entry (REPEAT_TOL: the
cap for shapes where the launcher's split-K mode may order fp64 atomics differently from run to run; fp32 epsilon is 6e-8).

Measured on an MI355X (error / largest entry, worst tensor of the case; loss relative):
    yardstick   a 2.2e-4   b 6.6e-5   c 1.1e-5   d 2.6e-5   e 2.4e-5   f 9.7e-7   g 1.4e-4   h 2.2e-5      loss <= 3.3e-6 (g)
    step        a 1.5e-4   d 9.6e-6   g 7.8e-5   h 1.1e-5
    case b in chunks of 60 points (60 + 60 + 60 + 23) against one chunk 5.4e-5; c + d in one accumulator against the union's yardstick 1.1e-5
    repeats (b, h): bitwise equal, and asserted so -- no product splits K below K = 256, so every sum has one order at these shapes;
    the 1e-6 cap stands beside it for shapes whose M'^3 products in begin_backward split K (M' = 3000: fp64 atomics in the launcher)"""
import ctypes as C
import math

import pytest
import torch

import _collapsed_ref as R
import _collapsed_grad_ref as GR

pytestmark = pytest.mark.gpu
NAMES = sorted(R.CASES)
GRAD_TOL, LOSS_TOL, REPEAT_TOL = 2e-3, 2e-5, 1e-6
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()


def relmax(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _ref(name):
    """(problem, float64 loss, float64 gradients) -- once per case, shared, never changed"""
    key = ("ref", name)
    if key not in _cache:
        prob = R.problem(name)
        P, x, y, D, nd, _, _, kernel = prob
        loss, grads, _, _ = GR.collapsed_loss_and_grads(P, x, y, D, nd, kernel)
        _cache[key] = (prob, loss.item(), grads)
    return _cache[key]


def _engine(dsvgp, dev, kernel):
    eng = dsvgp.ElboEngine(dev)
    eng.kernel = "matern52" if kernel == "matern52" else "rbf"
    return eng


def _backward(acc, res, sets):
    acc.begin_backward(res)
    for x, y, D in sets:
        acc.add_backward(x, y, D)
    return acc.finish_backward()


def _gpu(dsvgp, dev, name):
    """(engine, device parameters, device data, solved accumulator, result, (loss, grads) of one backward pass) -- once per case"""
    key = ("gpu", name)
    if key not in _cache:
        (P, x, y, D, nd, _, _, kernel), _, _ = _ref(name)
        eng = _engine(dsvgp, dev, kernel)
        Pg = {k: v.to(dev) for k, v in P.items()}
        data = (x.to(dev), y.to(dev), None if D is None else D.to(dev))
        acc = eng.collapsed_accumulator(Pg)
        acc.add(*data)
        res = acc.solve(nd)
        _cache[key] = (eng, Pg, data, acc, res, _backward(acc, res, [data]))
    return _cache[key]


def _errors(grads, ref):
    assert set(grads) == set(GR.GRAD_NAMES)
    for k in GR.GRAD_NAMES:
        assert grads[k].dtype == torch.float32 and tuple(grads[k].shape) == tuple(ref[k].shape), (k, grads[k].shape, ref[k].shape)
        assert torch.isfinite(grads[k]).all(), k
    return {k: relmax(grads[k], ref[k]) for k in GR.GRAD_NAMES}


# ------------------------------------------------------------------ 1. against the float64 yardstick
@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_the_yardstick(dsvgp, gpu_device, name):
    _, loss_ref, g_ref = _ref(name)
    _, _, _, _, res, (loss, grads) = _gpu(dsvgp, gpu_device, name)
    errs = _errors(grads, g_ref)
    e_loss = abs(loss - loss_ref) / abs(loss_ref)
    print("[collapsed-grad] case %s: loss %.9f (ref %.9f, error %.2e); " % (name, loss, loss_ref, e_loss)
          + ", ".join("%s %.2e" % (k, v) for k, v in errs.items()))
    # (the backward's loss is recomputed at the float32 (m*, L_S*) it was handed; the solve's at its float64 optimum: second order)
    assert isinstance(loss, float) and abs(loss - res.loss) <= 1e-6 * abs(res.loss)
    assert e_loss <= LOSS_TOL, (e_loss, loss, loss_ref)
    assert all(v <= GRAD_TOL for v in errs.values()), errs


# ------------------------------------------------------------------ 2. the envelope on the device
@pytest.mark.parametrize("name", ["a", "d", "g", "h"])
def test_envelope_against_the_piecewise_step(dsvgp, gpu_device, name):
    dev = gpu_device
    (P, x, y, D, nd, _, _, kernel), _, _ = _ref(name)
    eng, Pg, (xg, yg, Dg), _, res, (loss, grads) = _gpu(dsvgp, dev, name)
    Pq = dict(Pg, variational_mean=res.variational_mean, chol_variational_covar=res.chol_variational_covar)
    Dstep = torch.zeros(0, x.shape[1], device=dev) if Dg is None else Dg
    step_loss, step_grads, _, _ = eng.loss_and_grads(Pq, xg, yg, Dstep, nd, fast=False)
    errs = {k: relmax(grads[k], step_grads[k]) for k in GR.GRAD_NAMES}
    print("[collapsed-grad] case %s: against loss_and_grads at the optimum: " % name + ", ".join("%s %.2e" % (k, v) for k, v in errs.items()))
    assert abs(step_loss.item() - loss) <= LOSS_TOL * abs(loss)
    assert all(v <= GRAD_TOL for v in errs.values()), errs


# ------------------------------------------------------------------ 3. chunking
def test_chunked_backward_equals_one_chunk(dsvgp, gpu_device):
    dev = gpu_device
    (P, x, y, D, nd, _, _, kernel), _, g_ref = _ref("b")
    eng, Pg, data, acc, _, (loss, whole) = _gpu(dsvgp, dev, "b")
    pd = D.shape[0] // x.shape[0]
    small = eng.collapsed_accumulator(Pg, workspace_budget=60 * acc.row_bytes(pd, backward=True))
    rows = small.chunk_rows(pd, backward=True)
    assert rows == 60 and x.shape[0] % rows and -(-x.shape[0] // rows) >= 3 and small.chunk_rows(pd) < rows      # 60 + 60 + 60 + 23
    small.add(*data)
    loss_s, split = _backward(small, small.solve(nd), [data])
    e_whole, e_split = _errors(whole, g_ref), _errors(split, g_ref)
    mutual = {k: relmax(split[k], whole[k]) for k in GR.GRAD_NAMES}
    print("[collapsed-grad] case b in chunks of %d points: against one chunk " % rows + ", ".join("%s %.2e" % (k, v) for k, v in mutual.items()))
    assert all(v <= GRAD_TOL for v in e_whole.values()) and all(v <= GRAD_TOL for v in e_split.values()), (e_whole, e_split)
    assert all(v <= GRAD_TOL for v in mutual.values()), mutual
    assert abs(loss_s - loss) <= 1e-6 * abs(loss)


def test_direction_counts_may_differ_between_calls(dsvgp, gpu_device):
    """cases c (pd = 4) and d (values only) on the same points in one accumulator, cut into chunks: the yardstick of the union"""
    dev = gpu_device
    (Pc, xc, yc, Dc, _, _, _, kernel), _, _ = _ref("c")
    (Pd, xd, yd, _, _, _, _, _), _, _ = _ref("d")
    assert torch.equal(xc, xd) and all(torch.equal(Pc[k], Pd[k]) for k in Pc)
    nd = 1.3 * (yc.numel() + yd.numel())
    loss_ref, g_ref, _, _ = GR.collapsed_loss_and_grads_union(Pc, [(xc, yc, Dc), (xd, yd, None)], nd, kernel)
    eng, Pg, data_c, acc_c, _, _ = _gpu(dsvgp, dev, "c")
    sets = [data_c, (xd.to(dev), yd.to(dev), None)]
    mixed = eng.collapsed_accumulator(Pg, workspace_budget=40 * acc_c.row_bytes(4, backward=True))
    for s in sets:
        mixed.add(*s)
    loss, grads = _backward(mixed, mixed.solve(nd), sets)
    errs = _errors(grads, g_ref)
    print("[collapsed-grad] c + d in one accumulator: loss error %.2e; " % (abs(loss - loss_ref.item()) / abs(loss_ref.item()))
          + ", ".join("%s %.2e" % (k, v) for k, v in errs.items()))
    assert abs(loss - loss_ref.item()) <= LOSS_TOL * abs(loss_ref.item())
    assert all(v <= GRAD_TOL for v in errs.values()), errs


# ------------------------------------------------------------------ 4. repeats
@pytest.mark.parametrize("name", ["b", "h"])
def test_two_backward_passes_agree(dsvgp, gpu_device, name):
    _, _, data, acc, res, (loss, first) = _gpu(dsvgp, gpu_device, name)
    loss2, second = _backward(acc, res, [data])
    diffs = {k: relmax(second[k], first[k]) for k in GR.GRAD_NAMES}
    bitwise = all(torch.equal(second[k], first[k]) for k in GR.GRAD_NAMES)
    print("[collapsed-grad] case %s: repeat %s; " % (name, "bitwise equal" if bitwise else "not bitwise equal")
          + ", ".join("%s %.2e" % (k, v) for k, v in diffs.items()))
    assert all(v <= REPEAT_TOL for v in diffs.values()), diffs
    # at these shapes (K <= 129, below the launcher's split-K threshold of 256) every sum of the pass has one order: bitwise
    assert loss2 == loss
    for k in GR.GRAD_NAMES:
        assert torch.equal(second[k], first[k]), k


# ------------------------------------------------------------------ 5. misuse
def test_misuse_is_refused(dsvgp, gpu_device):
    dev = gpu_device
    (P, x, y, D, nd, _, _, kernel), _, _ = _ref("c")
    eng, Pg, data, _, _, _ = _gpu(dsvgp, dev, "c")
    acc = eng.collapsed_accumulator(Pg)
    with pytest.raises(ValueError, match="begin_backward"):
        acc.add_backward(*data)
    acc.add(*data)
    res = acc.solve(nd)
    other = acc.solve(2.0 * nd)
    with pytest.raises(ValueError, match="num_data"):
        acc.begin_backward(res)                                 # solved for another num_data than the accumulator's last solve
    acc.begin_backward(other)
    q = D.shape[0] // x.shape[0] + 1
    acc.add_backward(data[0][:50], data[1][:50 * q], data[2][:50 * (q - 1)])
    with pytest.raises(ValueError, match=r"seen %d rows.*R = %d" % (50 * q, y.numel())):
        acc.finish_backward()
    with pytest.raises(TypeError, match="on the GPU"):
        acc.add_backward(x, y, D)
    with pytest.raises(ValueError, match="interleaved"):
        acc.add_backward(data[0], data[1][:-1], data[2])
    with pytest.raises(ValueError, match=r"x must be \[B, 5\]"):
        acc.add_backward(data[0][:, :4], data[1], data[2])
    for moved in (lambda: acc.add(data[0][:10], data[1][:10 * q], data[2][:10 * (q - 1)]), lambda: acc.solve(nd)):
        with pytest.raises(ValueError, match="between begin_backward and finish_backward"):
            moved()                                             # neither the statistics nor the solve may move under an open pass
    assert acc.rows == y.numel()
    for m_, L_ in ((other.variational_mean[:-1], other.chol_variational_covar), (other.variational_mean, other.chol_variational_covar[:, :-1])):
        wrong = dsvgp.CollapsedResult(m_, L_, None, None, other.terms, other.num_data)
        with pytest.raises(ValueError, match=r"must be \[65"):
            acc.begin_backward(wrong)                           # a wrongly shaped (m, L_S)
    stale = eng.collapsed_accumulator(Pg)
    stale.add(*data)
    res_s = stale.solve(nd)
    stale.add(data[0][:10], data[1][:10 * q], data[2][:10 * (q - 1)])
    with pytest.raises(ValueError, match="solve"):
        stale.begin_backward(res_s)                             # the statistics moved on since that solve


def test_a_nan_target_raises_without_a_fault(dsvgp, gpu_device):
    dev = gpu_device
    (P, x, y, D, nd, _, _, kernel), _, _ = _ref("c")
    eng, Pg, data, _, _, _ = _gpu(dsvgp, dev, "c")
    acc = eng.collapsed_accumulator(Pg)
    acc.add(*data)
    res = acc.solve(nd)
    bad = data[1].clone()
    bad[11] = float("nan")
    acc.begin_backward(res)
    acc.add_backward(data[0], bad, data[2])
    with pytest.raises(ValueError, match="not finite"):
        acc.finish_backward()
    loss, grads = _backward(acc, res, [data])                   # the accumulator is usable afterwards
    assert math.isfinite(loss) and all(torch.isfinite(g).all() for g in grads.values())


def test_c_entries_refuse(dsvgp, gpu_device):
    dev = gpu_device
    lib, ops = dsvgp._lib.lib, dsvgp._ops
    ctx = ops.Context.get(dev)
    Mp, Bp = 5, 7
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    f64 = torch.float64
    state = torch.zeros(int(lib.dsvgp_collapsed_state_bytes(Mp)) // 8, dtype=f64, device=dev)
    m, LS = torch.zeros(Mp, device=dev), torch.eye(Mp, device=dev)
    inv = torch.eye(Mp, dtype=f64, device=dev).repeat(2, 1).contiguous()
    hyp = torch.tensor([1.0, 1.0, 0.1, 0.0], device=dev)
    alpha, Q, Kb = torch.full((Mp,), 9.0, dtype=f64, device=dev), torch.full((Mp, Mp), 9.0, dtype=f64, device=dev), torch.full((Mp, Mp), 9.0, dtype=f64, device=dev)
    adj, info = torch.full((8,), 9.0, dtype=f64, device=dev), torch.full((1,), 9, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.dsvgp_collapsed_grad_workspace_bytes(Mp)), dtype=torch.uint8, device=dev)
    Kzx, Kbar = torch.full((Mp, Bp), 3.0, device=dev), torch.full((Mp, Bp), 9.0, device=dev)
    y, c, dbar = torch.ones(Bp, device=dev), torch.zeros(1, device=dev), torch.full((Bp,), 9.0, device=dev)
    rsum = torch.full((1,), 9.0, dtype=f64, device=dev)
    cws = torch.empty(int(lib.dsvgp_collapsed_grad_chunk_bytes(Mp, Bp)) // 8, dtype=f64, device=dev)
    EINVAL, EALIGN = -1, -3
    prep = lambda **k: lib.dsvgp_collapsed_grad_prepare(k.get("ctx", ctx.h), k.get("state", p(state)), k.get("Mp", Mp), k.get("m", p(m)),
                                                        k.get("LS", p(LS)), k.get("ldls", Mp), k.get("inv", p(inv)), k.get("hyp", p(hyp)),
                                                        k.get("nd", 10.0), k.get("alpha", p(alpha)), k.get("Q", p(Q)), k.get("ldq", Mp),
                                                        k.get("Kb", p(Kb)), k.get("ldkb", Mp), k.get("adj", p(adj)), k.get("info", p(info)),
                                                        k.get("ws", p(ws)))
    chunk = lambda **k: lib.dsvgp_collapsed_grad_chunk(k.get("ctx", ctx.h), k.get("Mp", Mp), k.get("Bp", Bp), k.get("K", p(Kzx)),
                                                       k.get("ldk", Bp), k.get("y", p(y)), k.get("c", p(c)), k.get("Q", p(Q)), k.get("ldq", Mp),
                                                       k.get("alpha", p(alpha)), k.get("adj", p(adj)), k.get("Kbar", p(Kbar)),
                                                       k.get("ldkb", Bp), p(dbar), k.get("rsum", p(rsum)), k.get("ws", p(cws)))
    for rc in (prep(ctx=null), prep(state=null), prep(m=null), prep(LS=null), prep(inv=null), prep(hyp=null), prep(alpha=null), prep(Q=null),
               prep(Kb=null), prep(adj=null), prep(info=null), prep(ws=null), prep(Mp=0), prep(Mp=8193), prep(ldls=Mp - 1), prep(ldq=Mp - 1),
               prep(ldkb=Mp - 1), prep(nd=0.0), prep(nd=-1.0),
               chunk(ctx=null), chunk(K=null), chunk(y=null), chunk(c=null), chunk(Q=null), chunk(alpha=null), chunk(adj=null),
               chunk(Kbar=null), chunk(rsum=null), chunk(ws=null), chunk(Mp=0), chunk(Mp=8193), chunk(Bp=0), chunk(Bp=-1), chunk(ldk=Bp - 1),
               chunk(ldkb=Bp - 1), chunk(ldq=Mp - 1), chunk(Kbar=p(Kzx)),
               chunk(Kbar=C.c_void_p(Kzx.data_ptr() + 4 * Bp)), chunk(K=C.c_void_p(Kbar.data_ptr() + 4 * (Mp - 1) * Bp))):      # partial overlaps
        assert rc == EINVAL, rc
    off = lambda t: C.c_void_p(t.data_ptr() + 4)
    for rc in (prep(Q=off(Q)), prep(adj=off(adj)), prep(ws=off(ws)), chunk(Q=off(Q)), chunk(alpha=off(alpha)), chunk(rsum=off(rsum)),
               chunk(ws=off(cws))):
        assert rc == EALIGN, rc
    torch.cuda.synchronize()
    assert all((t == 9.0).all() for t in (alpha, Q, Kb, adj, Kbar, dbar, rsum)) and info.item() == 9         # nothing was touched
    # an empty state (R = 0) is reported through the flag, without a fault
    assert prep() == 0
    assert info.item() == 1


# ------------------------------------------------------------------ 6. harness
def _harness_data(dev):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("train_quality", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                "tools", "train_quality.py"))
    tq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tq)
    X, Y = tq.make_data("sin", 300 + 64, 3, dev, seed=0)
    Y = Y.float()
    return (X[:300].contiguous(), Y[:300].contiguous()), (X[300:].contiguous(), Y[300:].contiguous())


def test_collapsed_loss_and_grads_fills_the_hyper_parameter_gradients(dsvgp, gpu_device):
    dev = gpu_device
    (X, Y), _ = _harness_data(dev)
    dvi = dsvgp.directional_vi
    train = torch.utils.data.TensorDataset(X, Y)
    loop = dvi.setup_training(train, num_inducing=24, num_directions=2, minibatch_size=100, minibatch_dim=2, num_epochs=1, seed=4)
    model, likelihood = loop.model, loop.likelihood
    res = model.collapsed_loss_and_grads(likelihood, (X, Y), minibatch_size=100, seed=5)
    vd = model.variational_strategy._variational_distribution
    assert torch.equal(vd.variational_mean.data, res.variational_mean) and torch.equal(vd.chol_variational_covar.data, res.chol_variational_covar)
    named = dict(list(model.named_parameters()) + [("likelihood." + k, v) for k, v in likelihood.named_parameters()])
    variational = {id(q) for q in model.variational_parameters()}
    assert len(variational) == 2 and len(named) >= 8
    for k, prm in named.items():
        if id(prm) in variational:
            assert prm.grad is None, k
        else:
            assert prm.grad is not None and prm.grad.shape == prm.shape and torch.isfinite(prm.grad).all() and prm.grad.abs().max() > 0, k
    first = {k: prm.grad.clone() for k, prm in named.items() if prm.grad is not None}
    fit = dvi.fit_variational(model, likelihood, (X, Y), minibatch_size=100, seed=5)         # the same columns: the same optimum
    assert relmax(fit.variational_mean, res.variational_mean) <= 1e-4 and abs(fit.loss - res.loss) <= 1e-9 * abs(res.loss)
    for prm in named.values():
        prm.grad = None
    again = dvi.collapsed_loss_and_grads(model, likelihood, (X, Y), minibatch_size=100, seed=5, write_variational=False)
    assert abs(again.loss - res.loss) <= 1e-9 * abs(res.loss)
    assert all(relmax(named[k].grad, g) <= REPEAT_TOL for k, g in first.items())
    assert dvi._collapsed_columns(300, 3, 2, 100, 5) == dvi._collapsed_columns(300, 3, 2, 100, 5)
    assert len(dvi._collapsed_columns(300, 3, 2, 100, 5)) == 3 and all(c[0] == 0 and len(c) == 3 for c in dvi._collapsed_columns(300, 3, 2, 100, 5))


@pytest.mark.parametrize("extra", [{}, {"kernel": "matern52", "ard_num_dims": 3}], ids=["rbf", "matern52-ard"])
def test_train_collapsed_lowers_the_collapsed_loss(dsvgp, gpu_device, extra):
    dev = gpu_device
    (X, Y), (Xt, Yt) = _harness_data(dev)
    dvi = dsvgp.directional_vi
    train = torch.utils.data.TensorDataset(X, Y)
    test = torch.utils.data.TensorDataset(Xt, Yt)
    fresh = dvi.setup_training(train, num_inducing=24, num_directions=2, minibatch_size=100, minibatch_dim=2, num_epochs=1, seed=4, **extra)
    start = dvi.fit_variational(fresh.model, fresh.likelihood, (X, Y), minibatch_size=100, seed=9).loss
    model, likelihood = dvi.train_collapsed(train, num_inducing=24, num_directions=2, num_iterations=10, learning_rate_hypers=0.02,
                                            minibatch_size=100, seed=4, verbose=False, **extra)
    end = dvi.fit_variational(model, likelihood, (X, Y), minibatch_size=100, seed=9).loss
    print("[collapsed-grad] train_collapsed %s: full-data collapsed loss %.5f -> %.5f after 10 iterations" % (extra or "rbf", start, end))
    assert math.isfinite(end) and end < start
    means, variances = dvi.eval_gp(test, model, likelihood, num_directions=2, minibatch_size=64, minibatch_dim=2)
    assert means.shape == (64 * 3,) and torch.isfinite(means).all() and (variances > 0).all()
