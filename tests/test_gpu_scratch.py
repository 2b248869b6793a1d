"""GPU: no result may depend on what its scratch memory held before the call.

Every byte of device memory the library touches comes from torch -- ``torch.empty``, the engines' ``_get`` / ``_bytes`` caches, the
predictors' ``_ws`` -- and the hot path has a protocol for who clears what (csrc/step.hip: one memset over the arena for small
problems, the side stream for large ones with overlap, the launchers themselves otherwise; pad columns once per workspace address;
``_get_zeroed`` buffers at allocation only).  A mistake there is wrong only when the memory was not already zero, and newly mapped
device memory normally is.  So every case here makes its call twice on memory that reads as NaN (tests/_poison.py):

  1. the FIRST call of a fresh engine / predictor / plan inside ``poisoned_allocations()``: every ``torch.empty`` is dirty;
  2. the same call again after every scratch buffer -- the engine's ``_buf`` minus ``STATE``, the outputs, ``io->flat`` -- was
     overwritten in place; the one-call plans are replayed through ``plan.run(ctx, ws, flags | 8)``, the header's contract for a
     workspace somebody else wrote to;
  3. every output of both calls is finite and within the tolerance the existing test of that entry states against its reference;
     in deterministic mode the two calls are bitwise equal.

``StepPlan.clear_mode()`` proves which clearing regime a one-call step took."""
import functools

import pytest
import torch

import dsvgp_oracle as O
from _poison import poison_, poison_buffers, poisoned_allocations
from test_gpu_step import GRAD_TOL_FP64, _stated, make_problem, relmax

pytestmark = pytest.mark.gpu
f32, f64 = torch.float32, torch.float64

# ------------------------------------------------------------------ what is NOT scratch
# Buffers of ``ElboEngine._buf`` that may carry content from one call to the next: name -> where the code says so.  Everything else
# is poisoned between the two calls of a case (a buffer added later is poisoned by default).  The table may only hold buffers whose
# allocation site is ``_get_zeroed`` / ``torch.zeros`` or whose state is documented in _step.py, _step64.py or include/dsvgp.h;
# a buffer that merely breaks under poison is a bug, not an entry.
STATE = {
    # _step.py, _elbo_fast.solve_part: "fp32 copy with rows padded to a multiple of 4 floats, pad zeroed once" (``_get_zeroed``): the
    # pad columns must stay zero -- asserted after every call (_pads_still_zero) instead of being poisoned
    "Qe32_pad": "_step.py ElboEngine._elbo_fast / solve_part: _get_zeroed, pad columns zeroed once at allocation",
    # the sharded replicated stage of a data-parallel rank (one-rank cases here never allocate them)
    "Qcols32": "_step.py ElboEngine._elbo_fast: _get_zeroed, 'pad columns beyond the matrix stay zero'",
    "Lrows32": "_step.py ElboEngine._elbo_fast: _get_zeroed, rows beyond the matrix stay zero",
    "pk_early": "_step.py ElboEngine._reduce_tril_async: torch.zeros, '(the tail stays zero)'",
}
# nested: the collective operands of dsvgp_elbo_step_dp_f32 (include/dsvgp.h: q_local / lbar_local 'ZERO-INITIALISED once (the pad
# columns stay zero)', wire 'anything beyond that count is the caller's padding (keep it zero)'); torch.zeros in _c_step_dp_phases
STATE_NESTED = ("wire", "q_local", "lbar_local")


def _keep(buf):
    keep = set(STATE)
    for k, v in buf.items():
        if isinstance(v, dict):
            keep.update("%s/%s" % (k if isinstance(k, str) else repr(k), n) for n in STATE_NESTED)
    return keep


def _holds_tensor(v):
    if isinstance(v, dict):
        v = list(v.values())
    return torch.is_tensor(v) or (isinstance(v, (list, tuple)) and any(_holds_tensor(u) for u in v))


def _poison_scratch(eng):
    """poison every buffer of the engine's table that is not in STATE; the set poisoned must be all of the table minus STATE"""
    names = poison_buffers(eng._buf, keep=_keep(eng._buf))
    table = {k if isinstance(k, str) else repr(k) for k, v in eng._buf.items() if _holds_tensor(v)}
    roots = {n.split("/")[0].split("[")[0] if not n.startswith("(") else n.split("/")[0] for n in names}
    assert roots == table - set(STATE), (sorted(roots), sorted(table))
    return names


def _pads_still_zero(eng):
    t = eng._buf.get("Qe32_pad")
    if t is not None:
        Mp = t.shape[0]
        if t.shape[1] > Mp + 1:
            assert t[:, Mp + 1:].abs().max().item() == 0.0, "Qe32_pad: a pad column was written"


def _base(t):
    return t if t._base is None else t._base


def _tensors(out):
    """every tensor of a nest of tuples / lists / dicts, in order"""
    if torch.is_tensor(out):
        yield out
    elif isinstance(out, dict):
        for v in out.values():
            yield from _tensors(v)
    elif isinstance(out, (tuple, list)):
        for v in out:
            yield from _tensors(v)


def _poison_outputs(out):
    for t in _tensors(out):
        poison_(_base(t))


def _clone(out):
    if torch.is_tensor(out):
        return out.clone()
    if isinstance(out, dict):
        return {k: _clone(v) for k, v in out.items()}
    if isinstance(out, (tuple, list)):
        return tuple(_clone(v) for v in out)
    return out


def _all_finite(tag, out):
    for t in _tensors(out):
        assert bool(torch.isfinite(t).all()), "%s: a non-finite output %s" % (tag, tuple(t.shape))


def _bitwise(a, b):
    ta, tb = list(_tensors(a)), list(_tensors(b))
    assert len(ta) == len(tb) and all(torch.equal(u, v) for u, v in zip(ta, tb)), "the two calls differ bitwise"


def _to(P, dev):
    return {k: v.to(dev) for k, v in P.items()}


@pytest.fixture
def plan_calls(dsvgp, monkeypatch):
    """records (plan, entry, workspace, flags, further arguments) of every one-call step the engines queue"""
    calls = []
    ops = dsvgp._ops
    for cls, name in ((ops.StepPlan, "run"), (ops.StepPlan, "run_po"), (ops.StepPlan64, "run")):
        def wrapped(self, ctx, workspace, flags, *rest, _orig=getattr(cls, name), _name=name):
            calls.append((self, _name, workspace, int(flags), rest))
            return _orig(self, ctx, workspace, flags, *rest)
        monkeypatch.setattr(cls, name, wrapped)
    return calls


def _replay(dsvgp, dev, eng, call, out, slab=None, workspace=None):
    """step 2 of a one-call case: poison the engine's scratch (the plan's workspace among it) and the outputs, then queue the same
    step again through the plan with flag 8.  ``out`` holds the second call's results afterwards (the plan's io names its tensors)."""
    plan, name, ws, flags, rest = call
    _poison_scratch(eng)
    _poison_outputs(out)
    for t in rest:
        poison_(t)
    ctx = dsvgp._ops.Context.get(dev)
    if slab is not None:
        ctx.set_deterministic(eng._buf[slab])
    try:
        getattr(plan, name)(ctx, ws if workspace is None else workspace, flags | 8, *rest)
    finally:
        if slab is not None:
            ctx.set_deterministic(None)
    info, _ = plan.status()
    torch.cuda.synchronize()
    assert info == 0


# ------------------------------------------------------------------ a. the fp32 one-call ELBO step
@functools.lru_cache(maxsize=None)
def _problem(N, d, M, p, B, seed, unit_directions=False):
    P, x, y, D, nd = make_problem(N, d, M, p, B, seed=seed)
    if unit_directions:
        P["inducing_directions"] = torch.eye(d).repeat(M, 1)
    return P, x, y, D, nd


@functools.lru_cache(maxsize=None)
def _oracles(N, d, M, p, B, seed, mll="ELBO", unit_directions=False):
    """(reference-precision oracle, float64 oracle's gradients) of one state: computed once, shared, never changed"""
    P, x, y, D, nd = _problem(N, d, M, p, B, seed, unit_directions)
    ref = O.elbo_loss_and_grads(P, x, y, D, nd, mll)
    _, g64, _, _ = O.elbo_loss_and_grads({k: v.double() for k, v in P.items()}, x.double(), y.double(), D.double(), nd, mll)
    return ref, g64


def _check_step(tag, out, ref, g64, p, large=False, skip=()):
    """tolerances of test_gpu_step.py::test_step_matches_oracle: loss 2e-5, mu 2e-4 against the reference-precision oracle, every
    gradient GRAD_TOL_FP64 = 3e-4 against the float64 oracle.  ``large`` (shapes that test never measured): the gradient tolerance is
    max(3e-4, 3 x yardstick), the yardstick being the reference-precision oracle's own distance to the float64 oracle on this state
    (3 = that test's stated tolerance over its recorded yardstick, 3e-4 / 1.1e-4)."""
    loss, grads, mu, varn = out
    l_ref, g_ref, mu_ref, _ = ref
    _all_finite(tag, out)
    errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref)}
    tol = {}
    for k in O.PARAM_NAMES:
        if (p == 0 and k == "inducing_directions") or k in skip:
            continue
        errs[k] = relmax(grads[k], g64[k])
        yard = relmax(g_ref[k], g64[k])
        errs[k + "(ref-precision oracle)"] = yard
        tol[k] = max(GRAD_TOL_FP64, 3.0 * yard) if large else GRAD_TOL_FP64
    print("[parity] scratch %s: %s" % (tag, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert grads["chol_variational_covar"].triu(1).abs().max().item() == 0.0
    assert errs["loss"] < 2e-5 and errs["mu"] < 2e-4, (tag, errs)
    for k, t in tol.items():
        assert errs[k] < t, (tag, k, errs[k], t)


def _one_call_case(dsvgp, dev, plan_calls, shape, seed, setup=None, stated=None, unit_directions=False, large=False, skip=(),
                   slab=None, workspace_of=None):
    """the three steps of one fp32 one-call case; returns (clear mode of the first call, of the replay, first outputs, second)"""
    N, d, M, p, B = shape
    P, x, y, D, nd = _problem(N, d, M, p, B, seed, unit_directions)
    ref, g64 = _oracles(N, d, M, p, B, seed, "ELBO", unit_directions)
    eng = dsvgp.ElboEngine(dev)
    if setup is not None:
        setup(eng)
    Pg, xd, yd = _to(P, dev), x.to(dev), y.to(dev)
    Dd = D.to(dev) if stated is None else stated(Pg, D)
    with poisoned_allocations() as count:
        out = eng.loss_and_grads(Pg, xd, yd, Dd, nd)
        torch.cuda.synchronize()
    assert count.tensors > 0 and count.bytes > 0 and eng.c_step_used and len(plan_calls) == 1
    plan = plan_calls[-1][0]
    mode1 = plan.clear_mode()
    tag = "N=%d d=%d M=%d p=%d B=%d flags %d mode %d" % (N, d, M, p, B, plan_calls[-1][3], mode1)
    first = _clone(out)
    _check_step(tag + ", first call on dirty memory", first, ref, g64, p, large, skip)
    workspace = None if workspace_of is None else workspace_of(plan)
    _replay(dsvgp, dev, eng, plan_calls[0], out, slab, workspace)
    mode2 = plan.clear_mode()
    _check_step(tag + ", replay on poisoned scratch", out, ref, g64, p, large, skip)
    return mode1, mode2, first, out, eng


@pytest.mark.parametrize("shape,overlap", [((600, 5, 40, 2, 128), False), ((3000, 5, 200, 2, 512), True)],
                         ids=["Mp120-one-stream", "Mp600-two-streams"])
def test_one_call_step_one_memset_mode(dsvgp, gpu_device, plan_calls, shape, overlap):
    """small problems: ONE memset covers the arena of split-K / OUT_LOWER targets and the launchers skip their clears"""
    mode1, mode2, _, _, _ = _one_call_case(dsvgp, gpu_device, plan_calls, shape, shape[0] + shape[1])
    assert bool(plan_calls[0][3] & 1) == overlap
    assert mode1 == 1 and mode2 == 1


# The smallest M' (d = 5, p = 2, B = 64) whose arena is too large for the one-memset mode: measured on MI355X by queueing one step per
# M and reading clear_mode() -- see the test below, which pins both sides of it.
FIRST_PRECLEAR_M = 324          # M' = 972


def test_one_call_step_first_shape_of_the_side_stream_preclear(dsvgp, gpu_device, plan_calls):
    """the boundary between the one-memset mode and the side-stream preclear, d = 5, p = 2, B = 64: the last M of mode 1 and the first
    of mode 2.  Below STEP_S_LATE_MP = 1024 the fills sit under the Cholesky chain and the Gram target is among them (mode 2 + 4)."""
    M = FIRST_PRECLEAR_M
    mode, _, _, _, _ = _one_call_case(dsvgp, gpu_device, plan_calls, (4 * M, 5, M - 1, 2, 64), 7)
    assert mode == 1, mode
    del plan_calls[:]
    mode1, mode2, _, _, _ = _one_call_case(dsvgp, gpu_device, plan_calls, (4 * M, 5, M, 2, 64), 7, large=True)
    assert mode1 & 2 and mode1 == mode2, (mode1, mode2)
    if 3 * M < 1024:
        assert mode1 == 6, mode1


@pytest.mark.parametrize("M", [342, 512], ids=["Mp1026-s-late", "Mp1536-var-late"])
def test_one_call_step_side_stream_preclear(dsvgp, gpu_device, plan_calls, M):
    """large problems with overlap: the targets of the later products are cleared on the side stream.  M' = 1026: the other side of
    STEP_S_LATE_MP (the fills move beside the forward solve; the Gram product's launcher keeps its own).  M' = 1536: STEP_VAR_LATE_MP."""
    mode1, mode2, _, _, _ = _one_call_case(dsvgp, gpu_device, plan_calls, (4 * M, 5, M, 2, 64), 7, large=True)
    assert plan_calls[0][3] & 1
    assert mode1 == 2 and mode2 == 2, (mode1, mode2)


def _set(**kw):
    def setup(eng):
        for k, v in kw.items():
            assert hasattr(eng, k), k
            setattr(eng, k, v)
    return setup


@pytest.mark.parametrize("shape", [(600, 5, 40, 2, 128), (3000, 5, 200, 2, 512)], ids=["Mp120", "Mp600"])
def test_one_call_step_deterministic_mode_is_bitwise_across_the_poison(dsvgp, gpu_device, plan_calls, shape):
    """deterministic mode: one stream, slabs instead of atomics, the launchers clear for themselves -- and the same bits whatever the
    scratch (the slab among it) held"""
    mode1, mode2, first, second, eng = _one_call_case(dsvgp, gpu_device, plan_calls, shape, shape[0] + shape[1],
                                                      setup=_set(deterministic=True), slab="det_slab")
    assert not plan_calls[0][3] & 1 and "det_slab" in eng._buf
    assert mode1 == 0 and mode2 == 0
    _bitwise(first, second)


@pytest.mark.parametrize("attr,flag", [("tail_side", 16), ("phi_arg_fp64", 64), ("solve_pipe", 128), ("split_bf16", 32)])
def test_one_call_step_optional_schedules_at_mp_600(dsvgp, gpu_device, plan_calls, attr, flag):
    """flags 16 / 64 / 128 / 32 at M' = 600.  The arena of this size is cleared by the one memset whatever the flag (step_front:
    ``prezero`` does not read the flags), so clear_mode() is 1 here; flag 32's plane scratch (cstep_split_ws) is poisoned with the rest.
    (Flag 128 is accepted and ignored at this size: the row ranges need 16 block rows.)"""
    shape = (3000, 5, 200, 2, 512)
    mode1, mode2, _, _, eng = _one_call_case(dsvgp, gpu_device, plan_calls, shape, shape[0] + shape[1], setup=_set(**{attr: True}))
    assert plan_calls[0][3] & flag and plan_calls[0][3] & 1
    assert ("cstep_split_ws" in eng._buf) == (attr == "split_bf16")
    assert mode1 == 1 and mode2 == 1


@pytest.mark.parametrize("attr,flag", [("tail_side", 16), ("phi_arg_fp64", 64), ("overlap", 0)])
def test_one_call_step_launchers_clear_for_themselves(dsvgp, gpu_device, plan_calls, attr, flag):
    """M' = 1026, too large for the one memset: flags 16 / 64 and a step without the second stream switch the side-stream preclear
    off, and every launcher clears its own target (clear_mode() == 0).  (Flag 32 needs B' >= 256: not at this batch.)"""
    M = 342
    mode1, mode2, _, _, _ = _one_call_case(dsvgp, gpu_device, plan_calls, (4 * M, 5, M, 2, 64), 7, large=True,
                                           setup=_set(**{attr: attr != "overlap"}))
    assert plan_calls[0][3] & flag == flag and bool(plan_calls[0][3] & 1) == (attr != "overlap")
    assert mode1 == 0 and mode2 == 0, (mode1, mode2)


def test_one_call_step_stated_one_hot_directions(dsvgp, gpu_device, plan_calls, monkeypatch):
    """the canonical-direction kernels (io->dir_idx) for K_ZX and its backward.  (The both-sides route, io->v_one_hot, takes p + 1 = 11
    only: the unit-direction case below.)"""
    monkeypatch.setenv("DSVGP_CHECK_DIRS", "1")
    shape = (600, 5, 40, 2, 128)
    D = _problem(*shape, 608)[3]
    cols = [0] + [int(r.argmax()) + 1 for r in D[:2]]
    _one_call_case(dsvgp, gpu_device, plan_calls, shape, 608, stated=lambda Pg, D_: _stated(dsvgp, D_, cols, gpu_device))
    plan = plan_calls[0][0]
    assert bool(plan.io.dir_idx) and not plan.io.v_one_hot


def test_one_call_step_unit_directions_stated_on_both_sides(dsvgp, gpu_device, plan_calls, monkeypatch):
    """the full-gradient SVGP, d = p = 10, (900, 10, 37, 10, 96) as test_full_gradient_step_with_unit_directions_stated_on_both_sides
    builds it: K_ZZ, K_ZX and both backwards on the both-sides one-hot kernels"""
    monkeypatch.setenv("DSVGP_CHECK_DIRS", "1")
    ops = dsvgp._ops
    N, M, B, d = 900, 37, 96, 10

    def stated(Pg, D):
        Dd = D.to(gpu_device)
        rng = ops.index_range(gpu_device, d)
        ops.state_directions(Dd, rng, 0)
        ops.state_directions(Pg["inducing_directions"], rng, 0)
        return Dd

    _one_call_case(dsvgp, gpu_device, plan_calls, (N, d, M, d, B), N + M, stated=stated, unit_directions=True,
                   skip=("inducing_directions",))
    plan = plan_calls[0][0]
    assert bool(plan.io.dir_idx) and bool(plan.io.v_one_hot)


@pytest.mark.parametrize("shape", [(40, 2, 1, 1, 1), (200, 6, 11, 2, 65)], ids=["one-point-one-row", "one-row-past-a-tile"])
def test_one_call_step_degenerate_shapes(dsvgp, gpu_device, plan_calls, shape):
    mode1, mode2, _, _, _ = _one_call_case(dsvgp, gpu_device, plan_calls, shape, 3 * shape[0] + shape[1])
    assert mode1 == 1 and mode2 == 1


def test_one_call_step_stays_inside_its_workspace(dsvgp, gpu_device, plan_calls):
    """guard bands: the replay runs on a 256-byte aligned view inside a larger buffer with 4 KiB of 0xFF on either side (the view
    itself is 0xFF too); both bands are byte-identical afterwards.  The bands are only read."""
    band = 4096
    held = []

    def view(plan):
        big = torch.empty(plan.bytes + 2 * band + 256, dtype=torch.uint8, device=gpu_device)
        poison_(big)
        lo = band + (-(big.data_ptr() + band)) % 256
        held.append((big, lo, plan.bytes))
        return big[lo:lo + plan.bytes]

    _one_call_case(dsvgp, gpu_device, plan_calls, (600, 5, 40, 2, 128), 605, workspace_of=view)
    big, lo, nbytes = held[0]
    assert (big.data_ptr() + lo) % 256 == 0 and plan_calls[-1][2].data_ptr() == big.data_ptr() + lo
    assert bool((big[lo - band:lo] == 0xFF).all()) and bool((big[lo + nbytes:lo + nbytes + band] == 0xFF).all())
    assert bool((big[:lo] == 0xFF).all()) and bool((big[lo + nbytes:] == 0xFF).all())


# ------------------------------------------------------------------ b. the per-output plan (dsvgp_elbo_step_po_f32)
@pytest.mark.parametrize("shape", [(600, 5, 40, 2, 128), (3000, 5, 200, 2, 512)], ids=["Mp120", "Mp600"])
@pytest.mark.parametrize("mll", ["PLL", "ELBO"])
def test_per_output_plan(dsvgp, gpu_device, plan_calls, shape, mll):
    """tolerances of test_one_call_per_output_step_equals_the_piecewise_step against the oracle: loss 2e-5, mu and varn 2e-4, every
    gradient 3e-3"""
    N, d, M, p, B = shape
    seed = N + d + 3
    P, x, y, D, nd = _problem(N, d, M, p, B, seed)
    l_ref, g_ref, mu_ref, vn_ref = _oracles(N, d, M, p, B, seed, mll)[0]
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    Pg, xd, yd, Dd = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)

    def check(tag, out):
        loss, grads, mu, varn = out
        _all_finite(tag, out)
        errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref), "varn": relmax(varn, vn_ref)}
        errs.update({k: relmax(grads[k], g_ref[k]) for k in O.PARAM_NAMES if g_ref[k].numel() and g_ref[k].abs().max().item() > 0})
        print("[parity] scratch per-output %s %s %s: %s" % (shape, mll, tag, ", ".join("%s %.2e" % kv for kv in errs.items())))
        assert varn.numel() == B * (p + 1) and grads["chol_variational_covar"].triu(1).abs().max().item() == 0.0
        assert errs["loss"] < 2e-5 and errs["mu"] < 2e-4 and errs["varn"] < 2e-4, (tag, errs)
        assert all(errs[k] < 3e-3 for k in O.PARAM_NAMES if k in errs), (tag, errs)

    with poisoned_allocations() as count:
        out = eng.loss_and_grads(Pg, xd, yd, Dd, nd, mll, fast=False)
        torch.cuda.synchronize()
    assert count.tensors > 0 and eng.c_step_used and len(plan_calls) == 1 and plan_calls[0][1] == "run_po"
    assert plan_calls[0][0].clear_mode() == 0
    check("first call on dirty memory", _clone(out))
    _replay(dsvgp, dev, eng, plan_calls[0], out)
    check("replay on poisoned scratch", out)


# ------------------------------------------------------------------ c. the fp64 one-call step
@pytest.mark.parametrize("shape,deterministic", [((600, 5, 40, 2, 128), False), ((600, 5, 40, 2, 128), True), ((300, 20, 12, 17, 40), False),
                                                 ((300, 20, 12, 17, 40), True)],
                         ids=["Mp120", "Mp120-deterministic", "tiled-p17", "tiled-p17-deterministic"])
def test_fp64_one_call_step(dsvgp, gpu_device, plan_calls, shape, deterministic):
    """tolerances of test_gpu_fp64_step.py (loss and mean 1e-9, gradients 1e-7 against the float64 oracle); p = 17: the tiled assembly"""
    from dsvgp_amd._step64 import ElboEngine64
    from test_gpu_fp64 import make_problem64
    from test_gpu_fp64_step import _check_against
    N, d, M, p, B = shape
    P, x, y, D, nd = make_problem64(N, d, M, p, B, seed=N + d)
    l_ref, g_ref, mu_ref, _ = O.elbo_loss_and_grads(P, x, y, D, nd, "ELBO")
    dev = gpu_device
    eng = ElboEngine64(dev)
    eng.deterministic = deterministic
    Pg, xd, yd, Dd = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)
    with poisoned_allocations() as count:
        out = eng.loss_and_grads(Pg, xd, yd, Dd, nd, "ELBO")
        torch.cuda.synchronize()
    assert count.tensors > 0 and eng.c_step_used and eng.c_step_status == 0 and len(plan_calls) == 1
    first = _clone(out)
    _all_finite("fp64 first call", first)
    _check_against("%s first call on dirty memory" % (shape,), first[0], first[1], first[2], l_ref, g_ref, mu_ref, p)
    _replay(dsvgp, dev, eng, plan_calls[0], out, slab="det_slab64" if deterministic else None)
    _all_finite("fp64 replay", out)
    _check_against("%s replay on poisoned scratch" % (shape,), out[0], out[1], out[2], l_ref, g_ref, mu_ref, p)
    if deterministic:
        assert "det_slab64" in eng._buf
        _bitwise(first, out)


# ------------------------------------------------------------------ d. the Python-orchestrated path (c_step = False)
def _python_path_case(eng, call, check, bitwise=False):
    """first call inside poisoned_allocations(); every buffer of the engine's table outside STATE and the outputs poisoned; the same
    call again (its own allocations dirty as well)"""
    with poisoned_allocations() as count:
        out = call()
        torch.cuda.synchronize()
    assert count.tensors > 0 and not getattr(eng, "c_step_used", False)
    _pads_still_zero(eng)
    first = _clone(out)
    check("first call on dirty memory", first)
    names = _poison_scratch(eng)
    assert names, "the Python-orchestrated path keeps its intermediates in the engine's table"
    _poison_outputs(out)
    del out
    with poisoned_allocations():
        second = call()
        torch.cuda.synchronize()
    _pads_still_zero(eng)
    check("second call on poisoned scratch", second)
    if bitwise:
        _bitwise(first, second)
    return first, second


PY_SHAPES = [(600, 5, 40, 2, 128), (500, 20, 30, 5, 96)]
PY_IDS = ["N600-d5-M40-p2-B128", "N500-d20-M30-p5-B96"]


@pytest.mark.parametrize("shape", PY_SHAPES, ids=PY_IDS)
@pytest.mark.parametrize("mode", ["ELBO", "ELBO-general", "PLL"])
def test_python_path_rbf(dsvgp, gpu_device, shape, mode):
    """tolerances of test_step_matches_oracle (loss 2e-5, mu / varn 2e-4, gradients 3e-4 against the float64 oracle)"""
    N, d, M, p, B = shape
    fast, mll = mode == "ELBO", mode.split("-")[0]
    P, x, y, D, nd = _problem(N, d, M, p, B, N + d)
    ref, g64 = _oracles(N, d, M, p, B, N + d, mll)
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    eng.c_step = False
    Pg, xd, yd, Dd = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)

    def check(tag, out):
        _check_step("python path %s, %s" % (mode, tag), out, ref, g64, p)
        if fast:
            assert out[3].numel() == 0
        else:
            assert relmax(out[3], ref[3]) < 2e-4

    _python_path_case(eng, lambda: eng.loss_and_grads(Pg, xd, yd, Dd, nd, mll, fast=fast), check)


@pytest.mark.parametrize("shape", PY_SHAPES, ids=PY_IDS)
@pytest.mark.parametrize("mode", ["ELBO", "PLL"])
def test_python_path_deterministic_is_bitwise_across_the_poison(dsvgp, gpu_device, shape, mode):
    N, d, M, p, B = shape
    P, x, y, D, nd = _problem(N, d, M, p, B, N + d)
    ref, g64 = _oracles(N, d, M, p, B, N + d, mode)
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    eng.c_step = False
    eng.deterministic = True
    Pg, xd, yd, Dd = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)
    _python_path_case(eng, lambda: eng.loss_and_grads(Pg, xd, yd, Dd, nd, mode),
                      lambda tag, out: _check_step("python path deterministic %s, %s" % (mode, tag), out, ref, g64, p), bitwise=True)


def _family_step_case(dsvgp, dev, kernel, shape, mll):
    """ARD lengthscales / kernel = "matern52": problem, yardstick and tolerances of test_gpu_ard.py / test_gpu_matern.py"""
    import test_gpu_ard as TA
    import test_gpu_matern as TM
    from test_gpu_rect_train import _check_step as check_rect
    N, d, M, p, B = shape
    full = (N, d, M, p, p, B)                           # (pd = p: every data point with the model's number of directions)
    P, x, y, D, nd = TA._problem(*full)
    ref = (TM._reference if kernel == "matern52" else TA._reference)(full, mll)
    eng = dsvgp.ElboEngine(dev)
    eng.kernel = kernel
    eng.c_step = False
    Pg, xd, yd, Dd = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)

    def check(tag, out):
        _all_finite(tag, out)
        check_rect("scratch %s step %s %s, %s" % (kernel, shape, mll, tag), out, ref, p, False)

    _python_path_case(eng, lambda: eng.loss_and_grads(Pg, xd, yd, Dd, nd, mll), check)


@pytest.mark.parametrize("shape", PY_SHAPES, ids=PY_IDS)
@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
@pytest.mark.parametrize("kernel", ["rbf", "matern52"], ids=["ard", "matern52"])
def test_python_path_ard_and_matern(dsvgp, gpu_device, kernel, shape, mll):
    """(the Gram fast path is refused for these families: ELBO and PLL on the per-output path)"""
    _family_step_case(dsvgp, gpu_device, kernel, shape, mll)


@functools.lru_cache(maxsize=None)
def _missing_case(name):
    """test_gpu_missing.py's case of that name, or -- a shape (N, d, M, p, B) -- tests/_missing_ref.py's problem built at that shape
    (RBF, pd = p) with its random pattern of NaN targets: (P, x, y, D, nd, kernel, p)"""
    import unittest.mock
    import _missing_ref as MR
    import test_gpu_missing as TMiss
    if isinstance(name, str):
        P, x, y, D, nd, kernel, pd, p = TMiss._case(name, "random")
        return P, x, y, D, nd, kernel, p
    N, d, M, p, B = name
    with unittest.mock.patch.dict(MR.CASES, {"_scratch": (N, d, M, p, p, B, "rbf")}):       # (gone again on the way out)
        P, x, y, D, nd, kernel = MR.problem("_scratch")
    return P, x, MR.random_pattern(y, p), D, nd, kernel, p


@functools.lru_cache(maxsize=None)
def _missing_reference(name, mll):
    import _missing_ref as MR
    P, x, y, D, nd, kernel, _ = _missing_case(name)
    return MR.step(P, x, y, D, nd, mll, kernel)


@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
@pytest.mark.parametrize("name", PY_SHAPES + ["m129", "matern"], ids=PY_IDS + ["m129", "matern"])
def test_python_path_missing_targets(dsvgp, gpu_device, name, mll):
    """NaN targets: test_gpu_missing.py's set-up (tests/_missing_ref.py's problem and random pattern), reference and tolerances, at
    the two shapes of this section and at two of that file's own cases (M' = 129, Matern-5/2).  The Gram fast path is refused."""
    import test_gpu_missing as TMiss
    P, x, y, D, nd, kernel, p = _missing_case(name)
    ref = _missing_reference(name, mll)
    dev = gpu_device
    eng = TMiss._engine(dsvgp, dev, kernel)
    eng.c_step = False
    Pg, xd, yd, Dd = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)
    miss = torch.isnan(y)
    assert 0.2 < miss.double().mean().item() < 0.4

    def check(tag, out):
        _all_finite(tag, out)
        assert bool((out[3].cpu()[miss] == 0).all()), tag
        TMiss._assert_step("scratch missing step %s %s, %s" % (name, mll, tag), TMiss._step_errors(out, ref, p))

    _python_path_case(eng, lambda: eng.loss_and_grads(Pg, xd, yd, Dd, nd, mll), check)


@functools.lru_cache(maxsize=None)
def _noise_case(name):
    """test_gpu_noise_classes.py's case of that name, or -- a shape (N, d, M, p, B) -- tests/_noise_yardstick.py's problem at that
    shape (RBF, pd = p; its N is its own): (P, x, y, D, nd, kernel, p, pd)"""
    import test_gpu_noise_classes as TN
    if isinstance(name, str):
        return TN._step_case(name)
    _, d, M, p, B = name
    return TN.NY.problem(d, M, p, p, B) + ("rbf", p, p)


@functools.lru_cache(maxsize=None)
def _noise_reference(name, mll):
    import test_gpu_noise_classes as TN
    P, x, y, D, nd, kernel, p, pd = _noise_case(name)
    return TN.NY.step(P, x, y, D, pd, nd, mll, TN.matern52_family if kernel == "matern52" else TN.rbf_family)


@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
@pytest.mark.parametrize("name", PY_SHAPES + ["rbf", "matern_ard"], ids=PY_IDS + ["rbf", "matern_ard"])
def test_python_path_derivative_noise_classes(dsvgp, gpu_device, name, mll):
    """two noise classes: test_gpu_noise_classes.py's set-up (tests/_noise_yardstick.py), yardstick and tolerances, at the two shapes
    of this section and at two of that file's own cases.  Always the per-output path."""
    import test_gpu_noise_classes as TN
    from test_gpu_rect_train import GRAD_TOL, LOSS_TOL, MU_TOL, VAR_TOL
    P, x, y, D, nd, kernel, p, pd = _noise_case(name)
    l_ref, g_ref, mu_ref, var_ref = _noise_reference(name, mll)
    dev = gpu_device
    eng = TN._engine(dsvgp, dev, kernel)
    eng.c_step = False
    Pg, xd, yd, Dd = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)

    def check(tag, out):
        loss, grads, mu, varn = out
        _all_finite(tag, out)
        errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref), "varn": relmax(varn, var_ref)}
        errs.update({k: relmax(grads[k].reshape(-1), g_ref[k].reshape(-1)) for k in TN.NY.NAMES})
        print("[parity] scratch two-noise step %s %s, %s: %s" % (name, mll, tag, ", ".join("%s %.2e" % kv for kv in errs.items())))
        assert errs["loss"] < LOSS_TOL and errs["mu"] < MU_TOL and errs["varn"] < VAR_TOL, errs
        assert all(errs[k] < GRAD_TOL for k in TN.NY.NAMES), errs

    _python_path_case(eng, lambda: eng.loss_and_grads(Pg, xd, yd, Dd, nd, mll), check)


OWN = lambda shape: [shape] + PY_SHAPES                 # the covering test's own shape, then the two of this section
OWN_IDS = ["own-shape"] + PY_IDS


@pytest.mark.parametrize("shape", OWN((400, 4, 14, 2, 80)), ids=OWN_IDS)
@pytest.mark.parametrize("mll", ["ELBO", "PLL"])
def test_python_path_shared_directions(dsvgp, gpu_device, mll, shape):
    """test_shared_directions_step_matches_oracle's set-up and tolerances (loss 2e-5, mu / varn 2e-4, gradients 2e-3)"""
    N, d, M, p, B = shape
    P, x, y, D, nd = make_problem(N, d, M, p, B, seed=21)
    g = torch.Generator().manual_seed(4)
    P["inducing_directions"] = torch.eye(d)[:p] + 0.2 * torch.randn(p, d, generator=g)
    P["variational_mean"] = 0.3 * torch.randn(M + p, generator=g)
    P["chol_variational_covar"] = torch.eye(M + p) + 0.05 * torch.randn(M + p, M + p, generator=g)
    l_ref, g_ref, mu_ref, var_ref = O.shared_loss_and_grads(P, x, y, D, nd, mll)
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    eng.shared_directions = True
    eng.c_step = False
    Pg, xd, yd, Dd = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)

    def check(tag, out):
        loss, grads, mu, varn = out
        _all_finite(tag, out)
        assert abs(loss.item() - l_ref.item()) < 2e-5 * abs(l_ref.item()), tag
        assert relmax(mu, mu_ref) < 2e-4 and relmax(varn, var_ref) < 2e-4, tag
        for k in O.PARAM_NAMES:
            assert grads[k].shape == g_ref[k].shape and relmax(grads[k], g_ref[k]) < 2e-3, (tag, k)

    _python_path_case(eng, lambda: eng.loss_and_grads(Pg, xd, yd, Dd, nd, mll), check)


@pytest.mark.parametrize("shape", OWN((400, 3, 16, 2, 96)), ids=OWN_IDS)
@pytest.mark.parametrize("mode", ["ELBO", "ELBO-general", "PLL"])
def test_python_path_derivative_free_data(dsvgp, gpu_device, mode, shape):
    """test_dfree_step_matches_oracle's set-up and tolerances"""
    fast, mll = mode == "ELBO", mode.split("-")[0]
    N, d, M, p, B = shape
    P, x, _, D, nd = make_problem(N, d, M, p, B, seed=11)
    y = O.testfun(x)[:, 0].contiguous()
    l_ref, g_ref, mu_ref, var_ref = O.elbo_loss_and_grads(P, x, y, D, nd, mll, data_outputs="values")
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    eng.data_outputs = "values"
    eng.c_step = False
    Pg, xd, yd, Dd = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)

    def check(tag, out):
        loss, grads, mu, varn = out
        _all_finite(tag, out)
        assert mu.shape == (B,) and abs(loss.item() - l_ref.item()) < 2e-5 * abs(l_ref.item()), tag
        assert relmax(mu, mu_ref) < 2e-4 and (fast or relmax(varn, var_ref) < 2e-4), tag
        for k in O.PARAM_NAMES:
            assert relmax(grads[k], g_ref[k]) < 2e-3, (tag, k)

    _python_path_case(eng, lambda: eng.loss_and_grads(Pg, xd, yd, Dd, nd, mll, fast=fast), check)


@pytest.mark.parametrize("shape", [(400, 2, 20, 2, 100), (500, 20, 24, 5, 48)] + PY_SHAPES, ids=["d2", "d20"] + PY_IDS)
def test_python_path_ciq_strategy(dsvgp, gpu_device, shape):
    """test_ciq.py::test_ciq_step_matches_oracle's set-up and tolerances (loss 1e-3, mu / varn 5e-3, gradients 2e-2)"""
    from test_ngd import make_ngd_problem
    N, d, M, p, B = shape
    P, x, y, D, nd = make_ngd_problem(N, d, M, p, B, seed=N + d)
    l_ref, g_ref, mu_ref, var_ref = O.ciq_loss_and_grads(P, x, y, D, nd)
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev, trsm_nb=4096)
    eng.whitening = "ciq"
    Pg, xd, yd, Dd = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)

    def check(tag, out):
        loss, grads, mu, varn = out
        _all_finite(tag, out)
        assert abs(loss.item() - l_ref.item()) < 1e-3 * abs(l_ref.item()), tag
        assert relmax(mu, mu_ref) < 5e-3 and relmax(varn, var_ref) < 5e-3, tag
        for k in O.NGD_PARAM_NAMES:
            if g_ref[k].numel() and g_ref[k].abs().max() > 0:
                assert relmax(grads[k], g_ref[k]) < 2e-2, (tag, k)

    _python_path_case(eng, lambda: eng.loss_and_grads(Pg, xd, yd, Dd, nd), check)


@pytest.mark.parametrize("shape", PY_SHAPES, ids=PY_IDS)
@pytest.mark.parametrize("mode", ["ELBO-gram", "ELBO", "PLL"])
def test_python_path_float64_model_mode(dsvgp, gpu_device, shape, mode):
    """test_gpu_fp64.py::test_fp64_step_matches_fp64_oracle's set-up and tolerances (loss, mean, variance 1e-9; gradients 1e-7)"""
    from dsvgp_amd._step64 import ElboEngine64
    from test_gpu_fp64 import make_problem64
    N, d, M, p, B = shape
    fast, mll = mode == "ELBO-gram", mode.split("-")[0]
    P, x, y, D, nd = make_problem64(N, d, M, p, B, seed=N + d)
    l_ref, g_ref, mu_ref, var_ref = O.elbo_loss_and_grads(P, x, y, D, nd, mll)
    dev = gpu_device
    eng = ElboEngine64(dev)
    eng.c_step = False
    eng.fast_min_work = 0
    Pg, xd, yd, Dd = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)

    def check(tag, out):
        loss, grads, mu, varn = out
        _all_finite(tag, out)
        errs = {"loss": abs(loss.item() - l_ref.item()) / abs(l_ref.item()), "mu": relmax(mu, mu_ref),
                "var": 0.0 if fast else relmax(varn, var_ref)}
        assert errs["loss"] < 1e-9 and errs["mu"] < 1e-9 and errs["var"] < 1e-9, (tag, errs)
        assert torch.triu(grads["chol_variational_covar"], 1).abs().max().item() == 0.0
        errs.update({k: relmax(grads[k], g_ref[k]) for k in O.PARAM_NAMES})
        print("[parity] scratch fp64 python path %s %s, %s: %s" % (shape, mode, tag, ", ".join("%s %.1e" % kv for kv in errs.items())))
        assert max(errs[k] for k in O.PARAM_NAMES) < 1e-7, (tag, errs)

    _python_path_case(eng, lambda: eng.loss_and_grads(Pg, xd, yd, Dd, nd, mll, fast=fast), check)


# ------------------------------------------------------------------ e. predictors and accumulators
# What a predictor or an accumulator legitimately keeps between calls, and where the code says so (none of it is in a ``_buf`` of scratch):
#   MeanPredictor.weights, VariancePredictor.weights / Q / packZ / hyp, SamplePaths' packed weights
#                                  _step.py: "Holds its own buffers (the weights ...)  Valid for the parameter values it was built from."
#   CollapsedAccumulator._state    _step.py: the collapsed statistics (G, b, yy, R): ``_ops.collapsed_state``, cleared by ``reset``
#   CollapsedAccumulator._buf["trsm_ws"][:2 M'^2 doubles]
#                                  _step.py: "L^-1 | L^-T (2 M'^2 doubles): the head of every solve's workspace", copied in when the
#                                  buffer is allocated and reused by every later solve (``reuse_inverse=True``); its tail is scratch
# Scratch: ``_ws`` of the predictors, ``_solve_ws`` and every other entry of the accumulator's ``_buf`` (``grad_ws`` among them).
def _poison_predictor(obj):
    """poison the scratch a predictor / accumulator holds between two identical calls; returns what was poisoned"""
    done = []
    for name in ("_ws", "_solve_ws"):
        t = getattr(obj, name, None)
        if torch.is_tensor(t):
            poison_(t)
            done.append(name)
    buf = getattr(obj, "_buf", None)
    if isinstance(buf, dict):
        head = {}
        inv = getattr(obj, "_inv", None)
        if torch.is_tensor(inv) and "trsm_ws" in buf:
            nbytes = inv.numel() * inv.element_size()
            head["trsm_ws"] = buf["trsm_ws"][:nbytes].clone()
        done += poison_buffers(buf)
        for k, saved in head.items():                   # (the inverse in the head of the solve workspace: state, see above)
            buf[k][:saved.numel()].copy_(saved)
    return done


def _predictor_case(build, run, check, scratch_expected=None):
    """build and first calls inside poisoned_allocations(); the predictor's scratch and the first outputs poisoned; the same calls again"""
    with poisoned_allocations() as count:
        obj = build()
        out = run(obj)
        torch.cuda.synchronize()
    assert count.tensors > 0
    first = _clone(out)
    check("first call on dirty memory", first)
    done = _poison_predictor(obj)
    assert scratch_expected is None or bool(done) == scratch_expected, done
    _poison_outputs(out)
    del out
    with poisoned_allocations():
        second = run(obj)
        torch.cuda.synchronize()
    check("second call on poisoned scratch", second)
    return obj, first, second


@pytest.mark.parametrize("shape", [(400, 32, 21, 5, 37), (400, 33, 21, 5, 37)], ids=["fused-d32", "composed-d33"])
def test_mean_predictor(dsvgp, gpu_device, shape):
    """tests/test_gpu_mean_predictor.py: the float64 oracle at 2e-4; d = 32 | 33 is the fused / composed boundary (the composed route
    holds a [B, 2M] workspace)"""
    import test_gpu_mean_predictor as TMP
    N, d, M, p, B = shape
    P, x, D, mu_ref, grad_ref, c = TMP._case(*shape)
    dev = gpu_device
    Pg, xd, Dd = _to(P, dev), x.to(dev), D.to(dev)

    def run(pred):
        return (pred.mean(xd, Dd),) + tuple(pred.value_and_gradient(xd))

    def check(tag, out):
        mu, val, grad = out
        _all_finite(tag, out)
        errs = {"mean": relmax(mu, mu_ref), "gradient": relmax(grad, grad_ref), "values": relmax(val, mu_ref[::p + 1])}
        print("[parity] scratch mean predictor %s, %s: %s" % (shape, tag, ", ".join("%s %.2e" % kv for kv in errs.items())))
        assert max(errs.values()) < TMP.TOL, (tag, errs)

    _predictor_case(lambda: dsvgp.ElboEngine(dev).mean_predictor(Pg), run, check, scratch_expected=d > 32)


@pytest.mark.parametrize("shape", [(20, 65, 5, 130), (33, 40, 2, 70)], ids=["fused-d20", "composed-d33"])
def test_variance_acquisition_and_descent(dsvgp, gpu_device, shape):
    """tests/test_gpu_variance.py: the float64 yardstick of tests/_variance_yardstick.py at 2e-4"""
    import test_gpu_variance as TV
    Y = TV.Y
    d, M, p, B = shape
    P, P64, x, mom = TV._case(*shape)
    dev = gpu_device
    Pg, xg = _to(P, dev), x.float().to(dev)
    best = Y.ei_best(P64, x, False)
    lower, upper = torch.zeros(d, device=dev), torch.ones(d, device=dev)

    def run(pred):
        out = {"variance": pred.variance_and_gradient(xg)}
        for kind in Y.KINDS:
            out[kind] = pred.acquisition(xg, kind, beta=2.0, best=best, gradients=True)
        res = pred.descend(1.2 * xg[:9] - 0.1, lower, upper, kind="lcb", beta=2.0, best=best, iterations=3)
        out["descent"] = (res.x, res.values, res.gradients)
        return out

    def check(tag, out):
        _all_finite(tag, out)
        errs = {"variance": relmax(out["variance"][0], mom[2]), "variance_grad": relmax(out["variance"][1], mom[3])}
        for kind in Y.KINDS:
            a_ref, ga_ref = Y.acquisition(*mom, kind, beta=2.0, best=best, maximize=False)
            errs[kind], errs[kind + "_grad"] = relmax(out[kind][0], a_ref), relmax(out[kind][1], ga_ref)
        xs, vals, grads = out["descent"]
        a_ref, ga_ref = Y.acquisition_at(P64, xs.double().cpu(), "lcb", 2.0, best, False)
        errs["descent_value"], errs["descent_grad"] = relmax(vals, a_ref), relmax(grads, ga_ref)
        print("[parity] scratch variance predictor %s, %s: %s" % (shape, tag, ", ".join("%s %.2e" % kv for kv in errs.items())))
        assert bool((xs >= lower).all()) and bool((xs <= upper).all())
        assert max(errs.values()) < TV.TOL, (tag, errs)

    _, first, second = _predictor_case(lambda: dsvgp.ElboEngine(dev).variance_predictor(Pg), run, check)
    _bitwise(first, second)             # (test_two_identical_calls_are_bitwise_equal: these entries have one summation order)


PATHS = (20, 70, 5, 33, 128, 9)               # d, M, p, B, F, n of ((600, 20, 70, 5, 33), F = 128, n = 9)


def test_sample_paths_values_and_gradients(dsvgp, gpu_device):
    """tests/test_gpu_paths.py: fixed base samples, the float64 path yardstick at 2e-4"""
    import test_gpu_paths as TP
    d, M, p, B, F, n = PATHS
    P, x, draws, _, val_ref, grad_ref = TP._case(*PATHS)
    dev = gpu_device
    Pg, xg = _to(P, dev), x.to(dev)

    def check(tag, out):
        vals, grads = out
        _all_finite(tag, out)
        errs = {"values": relmax(vals, val_ref), "gradients": relmax(grads, grad_ref)}
        print("[parity] scratch sample paths, %s: %s" % (tag, ", ".join("%s %.2e" % kv for kv in errs.items())))
        assert vals.shape == (n, B) and grads.shape == (n, B, d) and max(errs.values()) < TP.TOL, (tag, errs)

    _predictor_case(lambda: dsvgp.ElboEngine(dev).sample_paths(Pg, n, F, base_samples=draws),
                    lambda paths: tuple(paths.values_and_gradients(xg)), check)


def test_sample_paths_hvp(dsvgp, gpu_device):
    """tests/test_gpu_paths_hvp.py: Hessian-vector products of every path against the float64 yardstick at 2e-4"""
    import test_gpu_paths_hvp as TH
    d, M, p, B, F, n = PATHS
    P, x, v, draws, _, ref = TH._case(*PATHS)
    dev = gpu_device
    Pg, xg, vg = _to(P, dev), x.to(dev), v.to(dev)

    def check(tag, out):
        _all_finite(tag, out)
        err = relmax(out[0], ref)
        print("[parity] scratch sample paths hvp, %s: Hv %.2e" % (tag, err))
        assert out[0].shape == (n, B, d) and err < TH.TOL, (tag, err)

    _predictor_case(lambda: dsvgp.ElboEngine(dev).sample_paths(Pg, n, F, base_samples=draws),
                    lambda paths: (paths.hvp(xg, vg),), check)


def test_sample_paths_at_their_own_points(dsvgp, gpu_device):
    """tests/test_gpu_paths_own.py: every path at its own points against the float64 yardstick at 2e-4"""
    import test_gpu_paths_own as TO
    d, M, p, B, F, n = PATHS
    P, x, xs, draws, _, ref_v, ref_g = TO._case(*PATHS)
    dev = gpu_device
    Pg, xg = _to(P, dev), xs.to(dev)

    def check(tag, out):
        val, grad = out
        _all_finite(tag, out)
        errs = {"values": relmax(val, ref_v), "gradient": relmax(grad, ref_g)}
        print("[parity] scratch sample paths at own points, %s: %s" % (tag, ", ".join("%s %.2e" % kv for kv in errs.items())))
        assert val.shape == (n, B) and grad.shape == (n, B, d) and max(errs.values()) < TO.TOL, (tag, errs)

    _predictor_case(lambda: dsvgp.ElboEngine(dev).sample_paths(Pg, n, F, base_samples=draws),
                    lambda paths: tuple(paths.values_and_gradients_at(xg)), check)


@pytest.mark.parametrize("shape", [(5, 40, 2, 5, 67, 600), (20, 64, 5, 20, 33, 900)], ids=["q6-ragged-group", "q21-row-slices"])
def test_covariance_blocks_and_their_roots(dsvgp, gpu_device, shape):
    """tests/test_gpu_blocks.py (mean 2e-4, blocks 5e-4 against the float64 yardstick) and tests/test_gpu_block_roots.py (the factor
    reconstructs the block and gives its log-determinant within that file's bounds)"""
    import test_gpu_blocks as TB
    import test_gpu_block_roots as TR
    d, M, p, pd, B, N = shape
    P, x, D, mu_ref, _, _, noise, _ = TB._case(*shape)
    ref, _, _, _ = TB._blocks_case(*shape)
    q = pd + 1
    target = ref + noise * torch.eye(q, dtype=f64)
    dev = gpu_device
    Pg, xg, Dg = _to(P, dev), x.to(dev), D.to(dev)
    eng = dsvgp.ElboEngine(dev)

    def run():
        mu, blocks = eng.predict_blocks(Pg, xg, Dg)
        roots, logdet = eng.block_roots(blocks)
        return mu, blocks, roots, logdet

    def check(tag, out):
        mu, blocks, roots, logdet = out
        _all_finite(tag, out)
        A, _, logdet_ref, kappa = TR.yardstick(blocks)
        L = roots.cpu()
        errs = {"mean": relmax(mu, mu_ref), "blocks": relmax(blocks, target),
                "reconstruction / bound": ((L @ L.transpose(1, 2) - A).abs() / TR.bound_reconstruction(L, q)).max().item(),
                "logdet / bound": ((logdet.cpu() - logdet_ref).abs() / (q * q * TR.U * kappa)).max().item()}
        print("[parity] scratch blocks and roots %s, %s: %s" % (shape[:5], tag, ", ".join("%s %.2e" % kv for kv in errs.items())))
        assert errs["mean"] < TB.TOL and errs["blocks"] < TB.CTOL, (tag, errs)
        assert errs["reconstruction / bound"] <= 1.0 and errs["logdet / bound"] <= 1.0, (tag, errs)

    _python_path_case(eng, run, check)


@pytest.mark.parametrize("name", ["b", "g"])
def test_collapsed_accumulator(dsvgp, gpu_device, name):
    """add / solve / evaluate and the begin / add / finish backward pass; tests/test_gpu_collapsed_grad.py's float64 yardstick
    (tests/_collapsed_grad_ref.py: loss 2e-5, gradients 2e-3), evaluate at the optimum against solve's loss (1e-6,
    tests/test_gpu_collapsed.py), the statistics against tests/_collapsed_ref.py (1e-2, as there).  The second round follows a
    ``reset()`` -- the library's own clear of the statistics -- on poisoned scratch."""
    import _collapsed_ref as R
    import _collapsed_grad_ref as GR
    import test_gpu_collapsed_grad as TG
    P, x, y, D, nd, _, _, kernel = R.problem(name)
    loss_ref, g_ref, _, _ = GR.collapsed_loss_and_grads(P, x, y, D, nd, kernel)
    stats = R.statistics(P, x, y, D, kernel)
    dev = gpu_device
    Pg = _to(P, dev)
    data = (x.to(dev), y.to(dev), None if D is None else D.to(dev))
    half = x.shape[0] // 2
    q = y.numel() // x.shape[0]
    parts = [(data[0][:half], data[1][:half * q], None if D is None else data[2][:half * (q - 1)]),
             (data[0][half:], data[1][half * q:], None if D is None else data[2][half * (q - 1):])]

    def run(acc):
        acc.reset()
        for part in parts:
            acc.add(*part)
        G, b, yy, _, rows = acc.statistics()
        res = acc.solve(nd)
        at = acc.evaluate(res.variational_mean, res.chol_variational_covar, nd)
        acc.begin_backward(res)
        for part in parts:
            acc.add_backward(*part)
        loss, grads = acc.finish_backward()
        return (G, b, yy, rows, res.variational_mean, res.chol_variational_covar, grads,
                torch.tensor([res.loss, at.loss, loss], dtype=f64))

    def check(tag, out):
        G, b, yy, rows, m, LS, grads, losses = out
        _all_finite(tag, out)
        errs = TG._errors(grads, g_ref)
        res_loss, at_loss, loss = losses.tolist()
        errs["loss"] = abs(loss - loss_ref.item()) / abs(loss_ref.item())
        errs["G"], errs["b"] = relmax(torch.tril(G), torch.tril(stats["G"])), relmax(b, stats["b"])
        print("[parity] scratch collapsed accumulator %s, %s: %s" % (name, tag, ", ".join("%s %.2e" % kv for kv in errs.items())))
        assert int(rows.item()) == y.numel()
        assert errs["G"] < 1e-2 and errs["b"] < 1e-2, (tag, errs)
        assert abs(at_loss - res_loss) <= 1e-6 * abs(res_loss) and abs(loss - res_loss) <= 1e-6 * abs(res_loss), (tag, losses)
        assert errs["loss"] <= TG.LOSS_TOL and all(errs[k] <= TG.GRAD_TOL for k in GR.GRAD_NAMES), (tag, errs)

    eng = TG._engine(dsvgp, dev, kernel)
    acc, _, _ = _predictor_case(lambda: eng.collapsed_accumulator(Pg), run, check, scratch_expected=True)
    assert "grad_ws" in acc._buf and acc._solve_ws is not None


@pytest.mark.parametrize("shape", [(2000, 20, 70), (1500, 33, 40)], ids=["fused-d20", "composed-d33"])
def test_kmeans_initialiser(dsvgp, gpu_device, shape):
    """tests/test_gpu_kmeans.py: labels against the restatement's arg-min over the returned centroids (outside the tie band), the
    inertia against the float64 sum over those labels at 2e-4, counts = bincount(labels).  The entry holds no scratch between calls:
    both rounds run inside poisoned_allocations()."""
    import test_gpu_kmeans as TK
    from test_kmeans_host import case
    N, d, M = shape
    X, Z0 = case(N, d, M)
    dev = gpu_device
    ops, ctx, Xg = dsvgp._ops, dsvgp._ops.Context.get(dev), X.to(dev)
    T = 4
    outs = []
    for tag in ("first call on dirty memory", "second call on dirty memory"):
        with poisoned_allocations() as count:
            Z = Z0.to(dev).clone()
            labels, dist2, counts, inertia, moved = ops.kmeans_lloyd_(ctx, Xg, Z, T)
            torch.cuda.synchronize()
        assert count.tensors > 0
        _all_finite(tag, (Z, dist2, inertia))
        ok, _ = TK.labels_agree(X, Z.cpu(), labels)
        own = TK.own_inertia(X, Z, labels)
        assert ok and int(labels.min()) >= 0 and int(labels.max()) < M, tag
        assert abs(inertia[T].item() - own) <= TK.TOL * own, (tag, inertia.tolist(), own)
        assert torch.equal(counts.cpu().long(), torch.bincount(labels.cpu().long(), minlength=M)), tag
        outs.append((Z, labels, dist2, counts, inertia, moved))
    _bitwise(outs[0], outs[1])                  # (test_lloyd_resumes_matches_the_restatement_and_is_reproducible: two identical calls)


@pytest.mark.parametrize("mode", ["ELBO", "PLL"])
def test_predict_and_predict_joint_directly_after_a_poisoned_step(dsvgp, gpu_device, mode):
    """a training step on the Python-orchestrated path, every buffer of the engine poisoned (``trsm_ws`` / the inverse among them:
    both entries below factor K_ZZ again), then predict and predict_joint: the oracle at test_predict_matches_oracle's 2e-4 and
    test_joint_predictive_covariance_matches_oracle's 5e-4"""
    N, d, M, p, B = 600, 5, 40, 2, 128
    P, x, y, D, nd = _problem(N, d, M, p, B, N + d)
    P64 = {k: v.double() for k, v in P.items()}
    mu_ref, var_ref = O.predictive(P, x, D)
    mu64, Sig_ref = O.predictive_joint(P64, x.double(), D.double())
    _, _, noise = O.constrained(P)
    Sig_ref = Sig_ref + noise.double() * torch.eye(B * (p + 1), dtype=f64)
    dev = gpu_device
    eng = dsvgp.ElboEngine(dev)
    eng.c_step = False
    Pg, xd, yd, Dd = _to(P, dev), x.to(dev), y.to(dev), D.to(dev)
    with poisoned_allocations() as count:
        out = eng.loss_and_grads(Pg, xd, yd, Dd, nd, mode, fast=mode == "ELBO")
        torch.cuda.synchronize()
        assert count.tensors > 0
        _poison_scratch(eng)
        _poison_outputs(out)
        mu, varn = eng.predict(Pg, xd, Dd)
        _poison_scratch(eng)
        mu_j, Sigma = eng.predict_joint(Pg, xd, Dd)
        torch.cuda.synchronize()
    _all_finite(mode, (mu, varn, mu_j, Sigma))
    errs = {"mean": relmax(mu, mu_ref), "variance": relmax(varn, var_ref + noise), "joint mean": relmax(mu_j, mu64),
            "joint covariance": relmax(Sigma, Sig_ref)}
    print("[parity] scratch predict after a poisoned %s step: %s" % (mode, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert errs["mean"] < 2e-4 and errs["variance"] < 2e-4 and errs["joint mean"] < 5e-4 and errs["joint covariance"] < 5e-4, errs
