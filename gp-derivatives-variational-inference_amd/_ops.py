"""Tensor-level wrappers over the C ABI (include/dsvgp.h).

torch is used only as the device allocator / stream provider: every function here checks device,
dtype and contiguity, then hands raw device pointers to libdsvgp_hip.so.  There is no CPU path.
"""
import ctypes as C

import os
import torch

from . import _lib
from ._lib import check, lib

f32, f64 = torch.float32, torch.float64


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _req(t, dtype, name, dims=None):
    if not t.is_cuda:
        raise _lib.DsvgpError("%s must live on the GPU: the DSVGP hot path has no CPU fallback" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if dims is not None and t.dim() != dims:
        raise ValueError("%s must be %d-D" % (name, dims))
    if t.dim() == 2:
        if t.stride(1) != 1 and t.shape[1] > 1:
            raise ValueError("%s must be row-major with unit column stride" % name)
    elif not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _ld(t):
    return int(t.stride(0)) if t.shape[0] > 1 else int(max(t.shape[1], t.stride(0)))


class Context:
    """One dsvgp_ctx per device; binds the library to torch's current HIP stream."""
    _cache = {}

    def __init__(self, device):
        self.device = torch.device(device)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.dsvgp_create(C.byref(h)), "dsvgp_create")
        self.h = h
        self._stream = None

    @classmethod
    def get(cls, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.DsvgpError("DSVGP HIP path needs a GPU device, got %s" % device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if idx not in cls._cache:
            cls._cache[idx] = Context(torch.device("cuda", idx))
        ctx = cls._cache[idx]
        ctx.bind()
        return ctx

    def set_deterministic(self, scratch):
        """scratch: a uint8 device tensor (split-K slabs / partial sums go there, no floating-point atomics) or None (atomics)"""
        if scratch is None:
            check(lib.dsvgp_set_deterministic(self.h, None, 0), "dsvgp_set_deterministic")
        else:
            check(lib.dsvgp_set_deterministic(self.h, _ptr(scratch), scratch.numel() * scratch.element_size()), "dsvgp_set_deterministic")

    def bind(self):
        # the library launches on this context's stream without a device guard of its own: make its device current
        # (one process per GPU is the intended use; torch.cuda.set_device(local_rank) has normally done this already)
        if torch.cuda.current_device() != self.device.index:
            torch.cuda.set_device(self.device)
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._stream:
            check(lib.dsvgp_set_stream(self.h, C.c_void_p(s)), "dsvgp_set_stream")
            self._stream = s


class StepPlan:
    """``dsvgp_step_plan`` of one (M, d, p, B): host-side object of the one-call ELBO step (csrc/step.hip)"""

    def __init__(self, ctx, M, d, p, B, world=1, per_output=False):
        h = C.c_void_p()
        self.per_output = bool(per_output)
        if per_output:      # dsvgp_elbo_step_po_f32: PLL objective / per-output variances (one rank)
            if world != 1:
                raise ValueError("the per-output step plan is a one-rank plan")
            check(lib.dsvgp_elbo_step_po_plan_create(ctx.h, int(M), int(d), int(p), int(B), C.byref(h)), "dsvgp_elbo_step_po_plan_create")
        elif world > 1:     # one rank of a data-parallel job (B = this rank's rows)
            check(lib.dsvgp_elbo_step_dp_plan_create(ctx.h, int(M), int(d), int(p), int(B), int(world), C.byref(h)),
                  "dsvgp_elbo_step_dp_plan_create")
            self.dp = _lib.ElboStepDP()
        else:
            check(lib.dsvgp_elbo_step_plan_create(ctx.h, int(M), int(d), int(p), int(B), C.byref(h)), "dsvgp_elbo_step_plan_create")
        self.world = int(world)
        self.h = h
        self.bytes = int(lib.dsvgp_elbo_step_plan_bytes(h))
        self.io = _lib.ElboStepIO()
        self._hyp = (C.c_float * 4)()
        self._info = C.c_int(0)
        self._ms = (C.c_float * 5)()

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            lib.dsvgp_elbo_step_plan_destroy(h)

    def run(self, ctx, workspace, flags):
        check(lib.dsvgp_elbo_step_f32(ctx.h, self.h, C.byref(self.io), _ptr(workspace), workspace.numel(), int(flags)),
              "dsvgp_elbo_step_f32")

    def run_po(self, ctx, workspace, flags, varn):
        check(lib.dsvgp_elbo_step_po_f32(ctx.h, self.h, C.byref(self.io), _ptr(varn), _ptr(workspace), workspace.numel(), int(flags)),
              "dsvgp_elbo_step_po_f32")

    def run_dp(self, ctx, workspace, flags, phase):
        check(lib.dsvgp_elbo_step_dp_f32(ctx.h, self.h, C.byref(self.io), C.byref(self.dp), _ptr(workspace), workspace.numel(),
                                         int(flags), int(phase)), "dsvgp_elbo_step_dp_f32 (phase %d)" % phase)

    def status(self):
        """(potrf status word, [lengthscale, outputscale, noise]) of the step queued last; waits for its factorisation only"""
        check(lib.dsvgp_elbo_step_status(self.h, self._hyp, C.byref(self._info)), "dsvgp_elbo_step_status")
        return int(self._info.value), [float(v) for v in self._hyp]

    def locate(self, workspace, which):
        """torch view of an intermediate of the step queued last inside ``workspace`` (dsvgp_elbo_step_locate)"""
        off, rows, cols, ld = C.c_size_t(0), C.c_int(0), C.c_int(0), C.c_int64(0)
        check(lib.dsvgp_elbo_step_locate(self.h, int(which), C.byref(off), C.byref(rows), C.byref(cols), C.byref(ld)),
              "dsvgp_elbo_step_locate")
        dt = torch.int32 if which == 5 else f32 if which in (0, 1, 4) else torch.float64
        esz = 4 if dt in (f32, torch.int32) else 8
        flat = workspace[off.value:off.value + rows.value * ld.value * esz].view(dt)
        return flat.view(rows.value, ld.value)[:, :cols.value]

    def clear_mode(self):
        """clearing regime of the step queued last: 0 launchers, 1 one memset over the arena, 2 side-stream preclear (+ 4 with the Gram target)"""
        return int(lib.dsvgp_elbo_step_clear_mode(self.h))

    def timed_count(self):
        return int(lib.dsvgp_elbo_step_timed_count(self.h))

    def timings(self, back=0):
        """[solve_fwd, assemble_fwd, assemble_bwd, gram, dense] HIP-event durations (ms) of the timed step ``back`` steps before the last"""
        check(lib.dsvgp_elbo_step_timings5(self.h, int(back), self._ms), "dsvgp_elbo_step_timings5")
        return [float(v) for v in self._ms]


class StepPlan64:
    """``dsvgp_step_plan_f64`` of one (M, d, p, B): host-side object of the float64 model mode's one-call ELBO step (csrc/step64.hip)"""

    def __init__(self, ctx, M, d, p, B):
        h = C.c_void_p()
        check(lib.dsvgp_elbo_step_f64_plan_create(ctx.h, int(M), int(d), int(p), int(B), C.byref(h)), "dsvgp_elbo_step_f64_plan_create")
        self.h = h
        self.bytes = int(lib.dsvgp_elbo_step_f64_workspace_bytes(int(M), int(d), int(p), int(B)))
        self.io = _lib.ElboStepIO64()
        self._hyp = (C.c_double * 4)()
        self._info = C.c_int(0)
        self._ms = (C.c_float * 5)()

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            lib.dsvgp_elbo_step_f64_plan_destroy(h)

    def run(self, ctx, workspace, flags):
        check(lib.dsvgp_elbo_step_f64(ctx.h, self.h, C.byref(self.io), _ptr(workspace), workspace.numel(), int(flags)),
              "dsvgp_elbo_step_f64")

    def status(self):
        """(potrf status word, [lengthscale, outputscale, noise, 0]) of the step queued last; waits for its factorisation only"""
        check(lib.dsvgp_elbo_step_f64_status(self.h, self._hyp, C.byref(self._info)), "dsvgp_elbo_step_f64_status")
        return int(self._info.value), [float(v) for v in self._hyp]

    def timed_count(self):
        return int(lib.dsvgp_elbo_step_f64_timed_count(self.h))

    def timings(self, back=0):
        """[solve_fwd, assemble_fwd, assemble_bwd, gram, dense] HIP-event durations (ms) of the timed step ``back`` steps before the last"""
        check(lib.dsvgp_elbo_step_f64_timings(self.h, int(back), self._ms), "dsvgp_elbo_step_f64_timings")
        return [float(v) for v in self._ms]


def step64_supported(M, d, p, B):
    return bool(lib.dsvgp_elbo_step_f64_supported(int(M), int(d), int(p), int(B)))


def step_supported(M, d, p, B, world=1, per_output=False):
    if per_output:
        return world == 1 and int(lib.dsvgp_elbo_step_po_workspace_bytes(int(M), int(d), int(p), int(B))) > 0
    if world > 1:
        return int(lib.dsvgp_elbo_step_dp_workspace_bytes(int(M), int(d), int(p), int(B), int(world))) > 0
    return int(lib.dsvgp_elbo_step_workspace_bytes(int(M), int(d), int(p), int(B))) > 0


def packed_width(d):
    return int(lib.dsvgp_packed_width(int(d)))


def hyp_forward(ctx, raw_l, raw_s, raw_n):
    hyp = torch.empty(4, dtype=f32, device=raw_l.device)
    check(lib.dsvgp_hyp_forward(ctx.h, _ptr(_req(raw_l.reshape(-1), f32, "raw_lengthscale")),
                                _ptr(_req(raw_s.reshape(-1), f32, "raw_outputscale")),
                                _ptr(_req(raw_n.reshape(-1), f32, "raw_noise")), _ptr(hyp)), "dsvgp_hyp_forward")
    return hyp


def hyp_backward(ctx, raw_l, raw_s, raw_n, d_hyp, d_raw_l, d_raw_s, d_raw_n):
    check(lib.dsvgp_hyp_backward(ctx.h, _ptr(raw_l), _ptr(raw_s), _ptr(raw_n), _ptr(d_hyp), _ptr(d_raw_l),
                                 _ptr(d_raw_s), _ptr(d_raw_n)), "dsvgp_hyp_backward")


def column_mean(ctx, x):
    """Column means of x[n, d]: the common shift ``center`` of the two point sets of one kernel call."""
    _req(x, f32, "x", 2)
    if not x.is_contiguous():
        raise ValueError("x must be contiguous")
    out = torch.empty(x.shape[1], dtype=f32, device=x.device)
    check(lib.dsvgp_column_mean(ctx.h, _ptr(x), x.shape[0], x.shape[1], _ptr(out)), "dsvgp_column_mean")
    return out


def step_epilogue(ctx, scal, kl0, rows, num_data, raw_l, raw_s, raw_n, d_hyp, d_raw_l, d_raw_s, d_raw_n, d_const, loss):
    check(lib.dsvgp_step_epilogue(ctx.h, _ptr(scal), _ptr(kl0), float(rows), float(num_data), _ptr(raw_l), _ptr(raw_s),
                                  _ptr(raw_n), _ptr(d_hyp), _ptr(d_raw_l), _ptr(d_raw_s), _ptr(d_raw_n), _ptr(d_const),
                                  _ptr(loss)), "dsvgp_step_epilogue")


def pack_points(ctx, x, v, p, hyp, center=None):
    """-> (P[n(p+1), DP], self[n(p+1)], vnorm[n p]).  ``center`` [d]: shift subtracted from x (same for both
    operands of a kernel call)."""
    _req(x, f32, "x", 2)
    n, d = x.shape
    if center is not None:
        _req(center, f32, "center", 1)
        if center.shape != (d,):
            raise ValueError("center must have shape [%d]" % d)
    if p > 0:
        _req(v, f32, "v", 2)
        if v.shape != (n * p, d):
            raise ValueError("directions must be [n*p, d] = [%d, %d], got %s" % (n * p, d, tuple(v.shape)))
    if not x.is_contiguous() or (p > 0 and not v.is_contiguous()):
        raise ValueError("x and v must be contiguous")
    DP = packed_width(d)
    P = torch.empty(n * (p + 1), DP, dtype=f32, device=x.device)
    sf = torch.empty(n * (p + 1), dtype=f32, device=x.device)
    vn = torch.empty(max(n * p, 1), dtype=f32, device=x.device)
    check(lib.dsvgp_pack_points(ctx.h, _ptr(x), _ptr(v if p > 0 else None), n, d, p, _ptr(hyp), _ptr(center), _ptr(P),
                                _ptr(sf), _ptr(vn)), "dsvgp_pack_points")
    return P, sf, vn


def kernel_fwd(ctx, pack1, n1, pack2, n2, d, p, hyp, jitter=0.0, out=None, dtype=f32):
    P1, s1 = pack1[0], pack1[1]
    P2, s2 = pack2[0], pack2[1]
    q = p + 1
    if out is None:
        out = torch.empty(n1 * q, n2 * q, dtype=dtype, device=P1.device)
    _req(out, dtype, "out", 2)
    if out.shape != (n1 * q, n2 * q):
        raise ValueError("out has shape %s, expected %s" % (tuple(out.shape), (n1 * q, n2 * q)))
    check(lib.dsvgp_kernel_fwd(ctx.h, _ptr(P1), _ptr(s1), n1, _ptr(P2), _ptr(s2), n2, d, p, _ptr(hyp), float(jitter),
                               _ptr(out), _ld(out), 1 if dtype == f64 else 0), "dsvgp_kernel_fwd")
    return out


def canon_supported(d, p):
    """geometries the canonical-direction assembly kernels take (csrc/assemble.hip): p + 1 in {3, 6}, packed width <= 32"""
    return p >= 1 and bool(lib.dsvgp_kernel_canon_supported(int(d), int(p)))


def state_directions(D, idx, base=0):
    """The caller's statement that the direction matrix ``D`` [B p, d] is one-hot and shared by all points: row j p + b = e_{idx[b] - base}
    for every j (what the reference's training step and evaluation build: directional_vi.py:81-88, 238, 292-294).  ``idx``: int32
    tensor [p] on D's device.  The statement travels with the tensor (``model(x, derivative_directions=D)`` is unchanged); the step
    then assembles K_ZX and its backward on the canonical-direction kernels where they take the geometry.  Returns D."""
    if D is not None and idx is not None and not _NO_CANON:
        D._dsvgp_dir_idx = (idx, int(base))
    return D


_RANGES = {}
_NO_CANON = os.environ.get("DSVGP_NO_CANON") == "1"      # tools: ignore the statements (the general assembly kernels everywhere: A/B runs)


def index_range(device, n):
    """the cached int32 tensor [0, 1, .., n - 1] on ``device`` (ONE object per device and length: statements that name all coordinates in
    order -- eye(d)[:p] tiled -- can be recognised as equal by identity)"""
    key = (str(device), int(n))
    t = _RANGES.get(key)
    if t is None:
        t = _RANGES[key] = torch.arange(int(n), dtype=torch.int32, device=device)
    return t


def same_statement(st_a, st_b):
    """whether two (idx, base) statements name the same list without reading device memory: the same tensor object / storage and base"""
    return (st_a is not None and st_b is not None and st_a[1] == st_b[1] and st_a[0].data_ptr() == st_b[0].data_ptr()
            and st_a[0].numel() == st_b[0].numel())


def detach_keep(t):
    """``t.detach()`` with the caller's statement about a direction matrix (state_directions) carried over to the new tensor object"""
    out = t.detach()
    st = getattr(t, "_dsvgp_dir_idx", None)
    if st is not None:
        out._dsvgp_dir_idx = st
    return out


def stated_directions(D, d, p, supported=None):
    """(idx, base) when ``D`` carries a usable statement (state_directions) for a geometry the canonical kernels take, else None.
    DSVGP_CHECK_DIRS=1: verify the statement against D (a device read: tests / debugging)."""
    st = getattr(D, "_dsvgp_dir_idx", None) if D is not None else None
    if st is None or p < 1 or _NO_CANON or not (supported or canon_supported)(d, p):
        return None
    idx, base = st
    if not (torch.is_tensor(idx) and idx.dtype == torch.int32 and idx.is_cuda and idx.numel() == p and idx.is_contiguous()
            and idx.device == D.device):
        return None
    if os.environ.get("DSVGP_CHECK_DIRS") == "1":
        E = torch.eye(d, device=D.device, dtype=D.dtype)[(idx.long() - base)]
        if not torch.equal(D.reshape(-1, p, d), E.expand(D.shape[0] // p, p, d)):
            raise _lib.DsvgpError("state_directions: D is not the one-hot matrix the index list states")
    return idx, int(base)


def canon2_supported(d, p):
    """geometries the both-sides one-hot assembly kernels take (csrc/assemble.hip: p + 1 = 11, d <= 12 -- the full-gradient SVGP at d = 10)"""
    return p >= 1 and bool(lib.dsvgp_kernel_canon2_supported(int(d), int(p)))


def _req_idx(dir_idx, p):
    if dir_idx.dtype != torch.int32 or not dir_idx.is_cuda or dir_idx.numel() != p or not dir_idx.is_contiguous():
        raise ValueError("dir_idx must be a contiguous int32 GPU tensor with p entries")


def kernel_fwd_canon2(ctx, pack1, n1, pack2, n2, d, p, dir_idx, idx_base, hyp, jitter=0.0, out=None, dtype=None):
    """K(x1, x2; E, E), E = the unit vectors e_{dir_idx - idx_base}, on both sides (GradVariationalStrategy.py:89-99 for dir_idx = 0..d-1)"""
    q = p + 1
    if out is None:
        out = torch.empty(n1 * q, n2 * q, dtype=dtype or f32, device=pack1[0].device)
    if out.dtype not in (f32, torch.float64) or out.dim() != 2 or out.stride(1) != 1 or not out.is_cuda:
        raise ValueError("out must be a float32 / float64 GPU matrix with unit inner stride")
    _req_idx(dir_idx, p)
    check(lib.dsvgp_kernel_fwd_canon2(ctx.h, _ptr(pack1[0]), n1, _ptr(pack2[0]), n2, d, p, _ptr(dir_idx), int(idx_base), _ptr(hyp),
                                      float(jitter), _ptr(out), _ld(out), 1 if out.dtype == torch.float64 else 0), "dsvgp_kernel_fwd_canon2")
    return out


def kernel_bwd_canon2(ctx, G, pack1, n1, pack2, n2, d, p, dir_idx, idx_base, hyp, symmetric, d_x1, d_v1, d_hyp, workspace=None):
    """backward of kernel_fwd_canon2: += d_x1, d_hyp[0..1] (d_v1 untouched: the directions are fixed)"""
    isd = G.dtype == torch.float64
    if G.dtype not in (f32, torch.float64) or G.dim() != 2 or G.stride(1) != 1 or not G.is_cuda:
        raise ValueError("G must be a float32 / float64 GPU matrix with unit inner stride")
    _req_idx(dir_idx, p)
    if workspace is None:
        workspace = torch.empty(int(lib.dsvgp_kernel_bwd_workspace_bytes(n1, n2, d, p)), dtype=torch.uint8, device=G.device)
    check(lib.dsvgp_kernel_bwd_canon2(ctx.h, _ptr(G), _ld(G), 1 if isd else 0, _ptr(pack1[0]), _ptr(pack1[2]), n1, _ptr(pack2[0]), n2, d, p,
                                      _ptr(dir_idx), int(idx_base), _ptr(hyp), 1 if symmetric else 0, _ptr(d_x1), _ptr(d_v1), _ptr(d_hyp),
                                      _ptr(workspace)), "dsvgp_kernel_bwd_canon2")


def kernel_fwd_canon(ctx, pack1, n1, pack2, n2, d, p, dir_idx, idx_base, hyp, out=None):
    """K(x1, x2; v1, E[dir_idx - idx_base]) with canonical (one-hot) directions on side 2 shared by all its points (the reference's K_ZX:
    directional_vi.py:81-88, 238, 292-294).  dir_idx: int32 device tensor with p entries."""
    q = p + 1
    if out is None:
        out = torch.empty(n1 * q, n2 * q, dtype=f32, device=pack1[0].device)
    _req(out, f32, "out", 2)
    if dir_idx.dtype != torch.int32 or not dir_idx.is_cuda or dir_idx.numel() != p or not dir_idx.is_contiguous():
        raise ValueError("dir_idx must be a contiguous int32 GPU tensor with p entries")
    check(lib.dsvgp_kernel_fwd_canon(ctx.h, _ptr(pack1[0]), _ptr(pack1[1]), n1, _ptr(pack2[0]), _ptr(pack2[1]), n2, d, p, _ptr(dir_idx),
                                     int(idx_base), _ptr(hyp), _ptr(out), _ld(out)), "dsvgp_kernel_fwd_canon")
    return out


def kernel_bwd_canon(ctx, G, pack1, n1, pack2, n2, d, p, dir_idx, idx_base, hyp, d_x1, d_v1, d_hyp, workspace=None):
    P1, s1, vn1 = pack1
    isd = G.dtype == f64
    _req(G, f64 if isd else f32, "G", 2)
    nbytes = int(lib.dsvgp_kernel_bwd_workspace_bytes(n1, n2, d, p))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=G.device)
    check(lib.dsvgp_kernel_bwd_canon(ctx.h, _ptr(G), _ld(G), 1 if isd else 0, _ptr(P1), _ptr(s1), _ptr(vn1), n1, _ptr(pack2[0]),
                                     _ptr(pack2[1]), n2, d, p, _ptr(dir_idx), int(idx_base), _ptr(hyp), _ptr(d_x1), _ptr(d_v1), _ptr(d_hyp),
                                     _ptr(workspace)), "dsvgp_kernel_bwd_canon")
    return workspace


# ---- fp64 model mode (csrc/assemble64.hip) ---------------------------------------------------------------------
def pack_points_f64(ctx, x, v, p, hyp, center=None):
    """-> (P[n(p+1), DP], self[n(p+1)], vnorm[n p]) in double precision"""
    _req(x, f64, "x", 2)
    n, d = x.shape
    if p > 0:
        _req(v, f64, "v", 2)
        if v.shape != (n * p, d):
            raise ValueError("directions must be [n*p, d] = [%d, %d], got %s" % (n * p, d, tuple(v.shape)))
    if not x.is_contiguous() or (p > 0 and not v.is_contiguous()):
        raise ValueError("x and v must be contiguous")
    DP = packed_width(d)
    P = torch.empty(n * (p + 1), DP, dtype=f64, device=x.device)
    sf = torch.empty(n * (p + 1), dtype=f64, device=x.device)
    vn = torch.empty(max(n * p, 1), dtype=f64, device=x.device)
    check(lib.dsvgp_pack_points_f64(ctx.h, _ptr(x), _ptr(v if p > 0 else None), n, d, p, _ptr(_req(hyp, f64, "hyp", 1)),
                                    _ptr(center), _ptr(P), _ptr(sf), _ptr(vn)), "dsvgp_pack_points_f64")
    return P, sf, vn


F64_REGISTER_P = 16     # directions per point that csrc/assemble64.hip's transform kernels hold in registers


def kernel_fwd_f64_tiled(ctx, pack1, n1, pack2, n2, d, p, hyp, jitter=0.0, out=None):
    """kernel_fwd_f64 on the tiled kernels (csrc/assemble64_tiled.hip) at any p <= 95: one launch, T never leaves the chip.
    jitter != 0 marks the symmetric (K_ZZ) call, as in kernel_fwd_f64"""
    q = p + 1
    if out is None:
        out = torch.empty(n1 * q, n2 * q, dtype=f64, device=pack1[0].device)
    _req(out, f64, "out", 2)
    if out.shape != (n1 * q, n2 * q):
        raise ValueError("out has shape %s, expected %s" % (tuple(out.shape), (n1 * q, n2 * q)))
    check(lib.dsvgp_kernel_fwd_f64(ctx.h, _ptr(pack1[0]), _ptr(pack1[1]), n1, _ptr(pack2[0]), _ptr(pack2[1]), n2, d, p,
                                   _ptr(_req(hyp, f64, "hyp", 1)), float(jitter), 1 if jitter != 0.0 else 0, _ptr(out), _ld(out)),
          "dsvgp_kernel_fwd_f64")
    return out


def kernel_bwd_f64_tiled(ctx, G, pack1, n1, pack2, n2, d, p, hyp, symmetric, d_x1, d_v1, d_hyp, workspace=None):
    """kernel_bwd_f64 on the tiled kernels at any p <= 95 (no [n1 q, n2 q] scratch); -> the workspace used"""
    _req(G, f64, "G", 2)
    if G.shape != (n1 * (p + 1), n2 * (p + 1)):
        raise ValueError("G has shape %s, expected %s" % (tuple(G.shape), (n1 * (p + 1), n2 * (p + 1))))
    nbytes = int(lib.dsvgp_kernel_bwd_f64_workspace_bytes(n1, n2, d, p))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=G.device)
    check(lib.dsvgp_kernel_bwd_f64(ctx.h, _ptr(G), _ld(G), _ptr(pack1[0]), _ptr(pack1[1]), _ptr(pack1[2]), n1, _ptr(pack2[0]),
                                   _ptr(pack2[1]), n2, d, p, _ptr(_req(hyp, f64, "hyp", 1)), 1 if symmetric else 0,
                                   _ptr(_req(d_x1, f64, "d_x1", 2)), _ptr(d_v1 if p > 0 else None),
                                   _ptr(_req(d_hyp, f64, "d_hyp", 1)), _ptr(workspace), workspace.numel()), "dsvgp_kernel_bwd_f64")
    return workspace


def kernel_fwd_f64(ctx, pack1, n1, pack2, n2, d, p, hyp, jitter=0.0, out=None):
    """outputscale * K(x1, x2; v1, v2) [+ jitter I] in fp64.  p <= 16: T = P1 P2^T on the fp64 MFMA GEMM, micro-block transform in
    place; more directions: the tiled kernels"""
    if p > F64_REGISTER_P:
        return kernel_fwd_f64_tiled(ctx, pack1, n1, pack2, n2, d, p, hyp, jitter, out)
    q = p + 1
    if out is None:
        out = torch.empty(n1 * q, n2 * q, dtype=f64, device=pack1[0].device)
    _req(out, f64, "out", 2)
    K4 = (d + 3) // 4 * 4
    gemm(ctx, _lib.TRANS_B, pack1[0], pack2[0], out, M=n1 * q, N=n2 * q, K=K4)
    check(lib.dsvgp_kernel_transform_f64(ctx.h, _ptr(out), _ld(out), _ptr(pack1[1]), n1, _ptr(pack2[1]), n2, p, _ptr(hyp),
                                         float(jitter)), "dsvgp_kernel_transform_f64")
    return out


def kernel_bwd_f64(ctx, G, pack1, n1, pack2, n2, d, p, hyp, symmetric, d_x1, d_v1, d_hyp, scratch=None):
    """backward of kernel_fwd_f64 w.r.t. (x1, v1, lengthscale, outputscale); accumulates into d_x1, d_v1, d_hyp[0..1]"""
    if p > F64_REGISTER_P:
        kernel_bwd_f64_tiled(ctx, G, pack1, n1, pack2, n2, d, p, hyp, symmetric, d_x1, d_v1, d_hyp)
        return
    q = p + 1
    _req(G, f64, "G", 2)
    K4 = (d + 3) // 4 * 4
    DP = pack1[0].shape[1]
    T = scratch if scratch is not None else torch.empty(n1 * q, n2 * q, dtype=f64, device=G.device)
    gemm(ctx, _lib.TRANS_B, pack1[0], pack2[0], T, M=n1 * q, N=n2 * q, K=K4)
    check(lib.dsvgp_kernel_bwd_transform_f64(ctx.h, _ptr(G), _ld(G), _ptr(T), _ld(T), _ptr(pack1[1]), n1, _ptr(pack2[1]), n2, p,
                                             _ptr(hyp), _ptr(_req(d_hyp, f64, "d_hyp", 1))), "dsvgp_kernel_bwd_transform_f64")
    dP = torch.empty(n1 * q, DP, dtype=f64, device=G.device)
    gemm(ctx, 0, T, pack2[0], dP)                                   # Tbar [P2 | indicator]
    check(lib.dsvgp_kernel_bwd_points_f64(ctx.h, _ptr(dP), _ptr(pack1[0]), _ptr(pack1[2]), n1, d, p, _ptr(hyp),
                                          1 if symmetric else 0, _ptr(_req(d_x1, f64, "d_x1", 2)),
                                          _ptr(d_v1 if p > 0 else None)), "dsvgp_kernel_bwd_points_f64")


def colstats_f64(ctx, A, W, m):
    """(mu0 = A^T m, cs = colsum(W^2 - A^2)) in fp64; W None -> cs None"""
    _req(A, f64, "A", 2); _req(m, f64, "m", 1)
    Mp, Bp = A.shape
    mu = torch.empty(Bp, dtype=f64, device=A.device)
    cs = torch.empty(Bp, dtype=f64, device=A.device) if W is not None else None
    check(lib.dsvgp_colstats_f64(ctx.h, _ptr(A), _ld(A), _ptr(W), _ld(W) if W is not None else 0, _ptr(m), Mp, Bp, _ptr(mu),
                                 _ptr(cs)), "dsvgp_colstats_f64")
    return mu, cs


def abar_f64(ctx, A, U, m, mu_bar, var_bar, Abar, Av=None):
    _req(A, f64, "A", 2); _req(Abar, f64, "Abar", 2)
    Mp, Bp = A.shape
    check(lib.dsvgp_abar_f64(ctx.h, _ptr(A), _ld(A), _ptr(U), _ld(U) if U is not None else 0, _ptr(_req(m, f64, "m", 1)),
                             _ptr(_req(mu_bar, f64, "mu_bar", 1)), _ptr(_req(var_bar, f64, "var_bar", 1)), Mp, Bp, _ptr(Abar),
                             _ld(Abar), _ptr(Av), _ld(Av) if Av is not None else 0), "dsvgp_abar_f64")


def likelihood_terms_f64(ctx, mu0, cs, y, constant, p, hyp, mll_type, rows):
    """(mu, varn, mu_bar, var_bar, scal[8]) of the fp64 model's likelihood + objective in one launch (see dsvgp.h)"""
    n = mu0.shape[0]
    dev = mu0.device
    mu, varn, mu_bar, var_bar = (torch.empty(n, dtype=f64, device=dev) for _ in range(4))
    scal = torch.empty(8, dtype=f64, device=dev)
    check(lib.dsvgp_likelihood_terms_f64(ctx.h, _ptr(_req(mu0, f64, "mu0", 1)), _ptr(_req(cs, f64, "cs", 1)),
                                         _ptr(_req(y, f64, "y", 1)), _ptr(_req(constant, f64, "constant", 1)), n, int(p), _ptr(hyp),
                                         int(mll_type), float(rows), _ptr(mu), _ptr(varn), _ptr(mu_bar), _ptr(var_bar), _ptr(scal)),
          "dsvgp_likelihood_terms_f64")
    return mu, varn, mu_bar, var_bar, scal


def elbo_fast_tail_f64(ctx, mu0, y, constant, npts, pd, hyp, tvar, rows):
    """(mu, mu_bar, scal[8]) of the fp64 ELBO fast path's scalar tail in two launches (see dsvgp.h): scal = {sum ll, d/d noise,
    d/d constant, d/d outputscale, d/d lengthscale, vbar, sum r^2, sum r}"""
    n = mu0.shape[0]
    dev = mu0.device
    mu, mu_bar = torch.empty(n, dtype=f64, device=dev), torch.empty(n, dtype=f64, device=dev)
    scal = torch.empty(8, dtype=f64, device=dev)
    check(lib.dsvgp_elbo_fast_tail_f64(ctx.h, _ptr(_req(mu0, f64, "mu0", 1)), _ptr(_req(y, f64, "y", 1)),
                                       _ptr(_req(constant, f64, "constant", 1)), n, int(npts), int(pd), _ptr(_req(hyp, f64, "hyp", 1)),
                                       _ptr(_req(tvar.reshape(1), f64, "tvar", 1)), float(rows), _ptr(mu), _ptr(mu_bar), _ptr(scal)),
          "dsvgp_elbo_fast_tail_f64")
    return mu, mu_bar, scal


def kernel_diag(ctx, n, p, hyp):
    out = torch.empty(n * (p + 1), dtype=f32, device=hyp.device)
    check(lib.dsvgp_kernel_diag(ctx.h, n, p, _ptr(hyp), _ptr(out)), "dsvgp_kernel_diag")
    return out


def kernel_bwd(ctx, G, pack1, n1, pack2, n2, d, p, hyp, symmetric, d_x1, d_v1, d_hyp, workspace=None):
    P1, s1, vn1 = pack1
    P2, s2 = pack2[0], pack2[1]
    isd = G.dtype == f64
    _req(G, f64 if isd else f32, "G", 2)
    nbytes = int(lib.dsvgp_kernel_bwd_workspace_bytes(n1, n2, d, p))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=G.device)
    check(lib.dsvgp_kernel_bwd(ctx.h, _ptr(G), _ld(G), 1 if isd else 0, _ptr(P1), _ptr(s1), _ptr(vn1), n1, _ptr(P2),
                               _ptr(s2), n2, d, p, _ptr(hyp), 1 if symmetric else 0, _ptr(d_x1),
                               _ptr(d_v1 if p > 0 else None), _ptr(d_hyp), _ptr(workspace)), "dsvgp_kernel_bwd")
    return workspace


def kernel_fwd_wide(ctx, pack1, n1, pack2, n2, d, p, hyp, jitter=0.0, out=None, dtype=f32):
    """kernel_fwd on the wide-input kernels (csrc/assemble_wide.hip) whatever d: kernel_fwd takes them by itself when the packed width
    exceeds 96; this entry runs them at any d (checks against the whole-row kernels)"""
    P1, s1 = pack1[0], pack1[1]
    P2, s2 = pack2[0], pack2[1]
    q = p + 1
    if out is None:
        out = torch.empty(n1 * q, n2 * q, dtype=dtype, device=P1.device)
    _req(out, dtype, "out", 2)
    if out.shape != (n1 * q, n2 * q):
        raise ValueError("out has shape %s, expected %s" % (tuple(out.shape), (n1 * q, n2 * q)))
    check(lib.dsvgp_kernel_fwd_wide(ctx.h, _ptr(P1), _ptr(s1), n1, _ptr(P2), _ptr(s2), n2, d, p, _ptr(hyp), float(jitter),
                                    _ptr(out), _ld(out), 1 if dtype == f64 else 0), "dsvgp_kernel_fwd_wide")
    return out


def kernel_fwd_rect(ctx, pack1, n1, p1, pack2, n2, p2, d, hyp, out=None):
    """out[n1 (p1 + 1), n2 (p2 + 1)] = s K(x1, x2; v1, v2) for packs made with DIFFERENT direction counts p1, p2 (each by
    ``pack_points`` with its own p and the same center); float32 (csrc/assemble_rect.hip; backward: ``kernel_bwd_rect``)"""
    P1, s1 = pack1[0], pack1[1]
    P2, s2 = pack2[0], pack2[1]
    shape = (n1 * (p1 + 1), n2 * (p2 + 1))
    for P, sf, n, p, name in ((P1, s1, n1, p1, "pack1"), (P2, s2, n2, p2, "pack2")):
        _req(P, f32, name, 2)
        _req(sf, f32, name + " self terms", 1)
        if P.shape != (n * (p + 1), packed_width(d)) or sf.shape[0] != n * (p + 1) or not P.is_contiguous():
            raise ValueError("%s is not the contiguous pack of %d points with %d directions at d = %d" % (name, n, p, d))
    if out is None:
        out = torch.empty(shape, dtype=f32, device=P1.device)
    _req(out, f32, "out", 2)
    if out.shape != shape:
        raise ValueError("out has shape %s, expected %s" % (tuple(out.shape), shape))
    check(lib.dsvgp_kernel_fwd_rect(ctx.h, _ptr(P1), _ptr(s1), n1, p1, _ptr(P2), _ptr(s2), n2, p2, d, _ptr(hyp), _ptr(out),
                                    _ld(out)), "dsvgp_kernel_fwd_rect")
    return out


def kernel_bwd_rect_workspace_bytes(n1, p1, n2, p2, d):
    """bytes of the workspace of ``kernel_bwd_rect`` (pure host arithmetic); 0 for a shape it does not take"""
    return int(lib.dsvgp_kernel_bwd_rect_workspace_bytes(int(n1), int(p1), int(n2), int(p2), int(d)))


def kernel_bwd_rect(ctx, G, pack1, n1, p1, pack2, n2, p2, d, hyp, d_x1, d_v1, d_hyp, workspace=None):
    """backward of ``kernel_fwd_rect`` with respect to side 1 (x1, v1) and (lengthscale, outputscale), given G = dLoss/dOut
    [n1 (p1 + 1), n2 (p2 + 1)] (float32 or float64, unit inner stride); accumulates (+=) into d_x1, d_v1, d_hyp[0:2].  Side 2 is data:
    no gradient (csrc/assemble_rect.hip)"""
    P1, s1, vn1 = pack1[0], pack1[1], (pack1[2] if len(pack1) > 2 else None)
    P2, s2 = pack2[0], pack2[1]
    isd = G.dtype == f64
    _req(G, f64 if isd else f32, "G", 2)
    if G.shape != (n1 * (p1 + 1), n2 * (p2 + 1)):
        raise ValueError("G has shape %s, expected %s" % (tuple(G.shape), (n1 * (p1 + 1), n2 * (p2 + 1))))
    for P, sf, n, p, name in ((P1, s1, n1, p1, "pack1"), (P2, s2, n2, p2, "pack2")):
        _req(P, f32, name, 2)
        _req(sf, f32, name + " self terms", 1)
        if P.shape != (n * (p + 1), packed_width(d)) or sf.shape[0] != n * (p + 1) or not P.is_contiguous():
            raise ValueError("%s is not the contiguous pack of %d points with %d directions at d = %d" % (name, n, p, d))
    nbytes = kernel_bwd_rect_workspace_bytes(n1, p1, n2, p2, d)
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=G.device)
    check(lib.dsvgp_kernel_bwd_rect(ctx.h, _ptr(G), _ld(G), 1 if isd else 0, _ptr(P1), _ptr(s1), _ptr(vn1 if p1 > 0 else None), n1, p1,
                                    _ptr(P2), _ptr(s2), n2, p2, d, _ptr(hyp), _ptr(d_x1), _ptr(d_v1 if p1 > 0 else None), _ptr(d_hyp),
                                    _ptr(workspace)), "dsvgp_kernel_bwd_rect")
    return workspace


def _req_ell(ell, d):
    _req(ell, f32, "ell", 1)
    if ell.shape != (d,):
        raise ValueError("ell must have shape [%d], got %s" % (d, tuple(ell.shape)))
    return ell


def hyp_forward_ard(ctx, raw_l, raw_s, raw_n):
    """-> (ell[d], hyp[4]): the softplus-constrained lengthscale vector, and ``hyp_forward``'s hyp with hyp[0] = 1 (the ARD packs carry
    the lengthscales; csrc/assemble_ard.hip)"""
    rl = _req(raw_l.reshape(-1), f32, "raw_lengthscale")
    d = rl.numel()
    ell = torch.empty(d, dtype=f32, device=rl.device)
    hyp = torch.empty(4, dtype=f32, device=rl.device)
    check(lib.dsvgp_hyp_forward_ard(ctx.h, _ptr(rl), d, _ptr(_req(raw_s.reshape(-1), f32, "raw_outputscale")),
                                    _ptr(_req(raw_n.reshape(-1), f32, "raw_noise")), _ptr(ell), _ptr(hyp)), "dsvgp_hyp_forward_ard")
    return ell, hyp


def hyp_backward_ard(ctx, raw_l, raw_s, raw_n, d_ell, d_hyp, d_raw_l, d_raw_s, d_raw_n):
    """d_raw_l[k] += d_ell[k] sigmoid(raw_l[k]); d_raw_s / d_raw_n += as ``hyp_backward`` (d_hyp[0] is not read)"""
    d = raw_l.numel()
    for t, name in ((raw_l, "raw_lengthscale"), (d_raw_l, "d_raw_lengthscale"), (d_ell, "d_ell")):
        if not t.is_contiguous() or t.numel() != d or t.dtype != f32:
            raise ValueError("%s must be %d contiguous float32 values" % (name, d))
    check(lib.dsvgp_hyp_backward_ard(ctx.h, _ptr(raw_l), d, _ptr(raw_s), _ptr(raw_n), _ptr(d_ell), _ptr(d_hyp), _ptr(d_raw_l),
                                     _ptr(d_raw_s), _ptr(d_raw_n)), "dsvgp_hyp_backward_ard")


def pack_points_ard(ctx, x, v, p, ell, center=None):
    """``pack_points`` with a lengthscale per dimension, ell[d]: rows (x - c) / ell and (v / |v|) / ell -> (P, self, vnorm)"""
    _req(x, f32, "x", 2)
    n, d = x.shape
    _req_ell(ell, d)
    if center is not None:
        _req(center, f32, "center", 1)
        if center.shape != (d,):
            raise ValueError("center must have shape [%d]" % d)
    if p > 0:
        _req(v, f32, "v", 2)
        if v.shape != (n * p, d):
            raise ValueError("directions must be [n*p, d] = [%d, %d], got %s" % (n * p, d, tuple(v.shape)))
    if not x.is_contiguous() or (p > 0 and not v.is_contiguous()):
        raise ValueError("x and v must be contiguous")
    DP = packed_width(d)
    P = torch.empty(n * (p + 1), DP, dtype=f32, device=x.device)
    sf = torch.empty(n * (p + 1), dtype=f32, device=x.device)
    vn = torch.empty(max(n * p, 1), dtype=f32, device=x.device)
    check(lib.dsvgp_pack_points_ard(ctx.h, _ptr(x), _ptr(v if p > 0 else None), n, d, p, _ptr(ell), _ptr(center), _ptr(P), _ptr(sf),
                                    _ptr(vn)), "dsvgp_pack_points_ard")
    return P, sf, vn


def _req_pack(pack, n, p, d, name):
    P, sf = pack[0], pack[1]
    _req(P, f32, name, 2)
    _req(sf, f32, name + " self terms", 1)
    if P.shape != (n * (p + 1), packed_width(d)) or sf.shape[0] != n * (p + 1) or not P.is_contiguous():
        raise ValueError("%s is not the contiguous pack of %d points with %d directions at d = %d" % (name, n, p, d))
    return P, sf


def kernel_diag_ard(ctx, pack, n, p, d, hyp):
    """out[n (p + 1)] = s [1, |v~_1|^2, ..., |v~_p|^2] per point: the prior diagonal of the ARD kernel from a ``pack_points_ard`` pack"""
    P, _ = _req_pack(pack, n, p, d, "pack")
    out = torch.empty(n * (p + 1), dtype=f32, device=P.device)
    check(lib.dsvgp_kernel_diag_ard(ctx.h, _ptr(P), n, p, d, _ptr(hyp), _ptr(out)), "dsvgp_kernel_diag_ard")
    return out


def kernel_diag_ard_bwd(ctx, pack, n, p, d, ell, hyp, out, gbar, d_ell, d_hyp):
    """backward of ``kernel_diag_ard`` given gbar[n (p + 1)] and the forward's ``out``: accumulates (+=) into d_ell[d] and d_hyp[1]"""
    P, _ = _req_pack(pack, n, p, d, "pack")
    _req_ell(ell, d)
    _req_ell(d_ell, d)
    for t, name in ((out, "out"), (gbar, "gbar")):
        _req(t, f32, name, 1)
        if t.shape[0] != n * (p + 1):
            raise ValueError("%s must have %d entries" % (name, n * (p + 1)))
    check(lib.dsvgp_kernel_diag_ard_bwd(ctx.h, _ptr(P), n, p, d, _ptr(ell), _ptr(hyp), _ptr(out), _ptr(gbar), _ptr(d_ell), _ptr(d_hyp)),
          "dsvgp_kernel_diag_ard_bwd")


def kernel_bwd_ard_workspace_bytes(n1, p1, n2, p2, d):
    """bytes of the workspace of ``kernel_bwd_ard`` (pure host arithmetic); 0 for a shape it does not take"""
    return int(lib.dsvgp_kernel_bwd_ard_workspace_bytes(int(n1), int(p1), int(n2), int(p2), int(d)))


def kernel_bwd_ard_slabs(n1, p1, n2, p2, d):
    """how many split slabs the contraction of ``kernel_bwd_ard`` writes for these shapes (pure host arithmetic); 0: refused"""
    return int(lib.dsvgp_kernel_bwd_ard_slabs(int(n1), int(p1), int(n2), int(p2), int(d)))


def kernel_bwd_ard(ctx, G, pack1, n1, p1, pack2, n2, p2, d, ell, hyp, symmetric, d_x1, d_v1, d_ell, d_hyp, workspace=None):
    """backward of the ARD kernel (``pack_points_ard`` packs, ``hyp_forward_ard``'s hyp) with respect to side 1 (x1, v1), the
    lengthscale vector (through both sides) and the outputscale, given G = dLoss/dOut [n1 (p1 + 1), n2 (p2 + 1)] (float32 or float64,
    unit inner stride); accumulates (+=) into d_x1, d_v1, d_ell and d_hyp[1].  d_ell and d_v1 may be None (csrc/assemble_ard.hip)"""
    P1, s1 = _req_pack(pack1, n1, p1, d, "pack1")
    P2, s2 = _req_pack(pack2, n2, p2, d, "pack2")
    vn1 = pack1[2] if len(pack1) > 2 else None
    isd = G.dtype == f64
    _req(G, f64 if isd else f32, "G", 2)
    if G.shape != (n1 * (p1 + 1), n2 * (p2 + 1)):
        raise ValueError("G has shape %s, expected %s" % (tuple(G.shape), (n1 * (p1 + 1), n2 * (p2 + 1))))
    _req_ell(ell, d)
    if d_ell is not None:
        _req_ell(d_ell, d)
    _req(d_x1, f32, "d_x1", 2)
    if d_x1.shape != (n1, d) or not d_x1.is_contiguous():
        raise ValueError("d_x1 must be contiguous [%d, %d]" % (n1, d))
    want_v = p1 > 0 and d_v1 is not None
    if want_v:
        _req(d_v1, f32, "d_v1", 2)
        if d_v1.shape != (n1 * p1, d) or not d_v1.is_contiguous() or vn1 is None:
            raise ValueError("d_v1 must be contiguous [%d, %d] and pack1 must carry its direction norms" % (n1 * p1, d))
    nbytes = kernel_bwd_ard_workspace_bytes(n1, p1, n2, p2, d)
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=G.device)
    check(lib.dsvgp_kernel_bwd_ard(ctx.h, _ptr(G), _ld(G), 1 if isd else 0, _ptr(P1), _ptr(s1), _ptr(vn1 if want_v else None), n1, p1,
                                   _ptr(P2), _ptr(s2), n2, p2, d, _ptr(ell), _ptr(hyp), 1 if symmetric else 0, _ptr(d_x1),
                                   _ptr(d_v1 if want_v else None), _ptr(d_ell), _ptr(d_hyp), _ptr(workspace)), "dsvgp_kernel_bwd_ard")
    return workspace


def kernel_fwd_matern52(ctx, pack1, n1, p1, pack2, n2, p2, d, hyp, jitter=0.0, out=None, dtype=f32):
    """out[n1 (p1 + 1), n2 (p2 + 1)] = s K(x1, x2; v1, v2) of the Matern-5/2 kernel with directional derivatives, from ``pack_points_ard``
    packs (same ell and center on both sides) and ``hyp_forward_ard``'s hyp; float32, or float64 storage with ``dtype``; ``jitter`` goes on
    the global diagonal (K_ZZ: both sides the same pack).  csrc/assemble_matern.hip; backward: ``kernel_bwd_matern52``"""
    P1, s1 = _req_pack(pack1, n1, p1, d, "pack1")
    P2, s2 = _req_pack(pack2, n2, p2, d, "pack2")
    shape = (n1 * (p1 + 1), n2 * (p2 + 1))
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=P1.device)
    _req(out, dtype, "out", 2)
    if out.shape != shape:
        raise ValueError("out has shape %s, expected %s" % (tuple(out.shape), shape))
    check(lib.dsvgp_kernel_fwd_matern52(ctx.h, _ptr(P1), _ptr(s1), n1, p1, _ptr(P2), _ptr(s2), n2, p2, d, _ptr(hyp), float(jitter),
                                        _ptr(out), _ld(out), 1 if dtype == f64 else 0), "dsvgp_kernel_fwd_matern52")
    return out


def kernel_diag_matern52(ctx, pack, n, p, d, hyp):
    """out[n (p + 1)] = s [1, (5/3) |v~_1|^2, ..., (5/3) |v~_p|^2] per point: the prior diagonal of the Matern-5/2 kernel from a
    ``pack_points_ard`` pack"""
    P, _ = _req_pack(pack, n, p, d, "pack")
    out = torch.empty(n * (p + 1), dtype=f32, device=P.device)
    check(lib.dsvgp_kernel_diag_matern52(ctx.h, _ptr(P), n, p, d, _ptr(hyp), _ptr(out)), "dsvgp_kernel_diag_matern52")
    return out


def kernel_diag_matern52_bwd(ctx, pack, n, p, d, ell, hyp, out, gbar, d_ell, d_hyp):
    """backward of ``kernel_diag_matern52`` given gbar[n (p + 1)] and the forward's ``out``: accumulates (+=) into d_ell[d] and d_hyp[1]"""
    P, _ = _req_pack(pack, n, p, d, "pack")
    _req_ell(ell, d)
    _req_ell(d_ell, d)
    for t, name in ((out, "out"), (gbar, "gbar")):
        _req(t, f32, name, 1)
        if t.shape[0] != n * (p + 1):
            raise ValueError("%s must have %d entries" % (name, n * (p + 1)))
    check(lib.dsvgp_kernel_diag_matern52_bwd(ctx.h, _ptr(P), n, p, d, _ptr(ell), _ptr(hyp), _ptr(out), _ptr(gbar), _ptr(d_ell),
                                             _ptr(d_hyp)), "dsvgp_kernel_diag_matern52_bwd")


def kernel_bwd_matern52_workspace_bytes(n1, p1, n2, p2, d):
    """bytes of the workspace of ``kernel_bwd_matern52`` (pure host arithmetic; ``kernel_bwd_ard``'s rounded up to a multiple of 16); 0 for
    a shape it does not take"""
    return int(lib.dsvgp_kernel_bwd_matern52_workspace_bytes(int(n1), int(p1), int(n2), int(p2), int(d)))


def kernel_bwd_matern52(ctx, G, pack1, n1, p1, pack2, n2, p2, d, ell, hyp, symmetric, d_x1, d_v1, d_ell, d_hyp, workspace=None):
    """backward of ``kernel_fwd_matern52`` with ``kernel_bwd_ard``'s arguments and semantics: accumulates (+=) into d_x1, d_v1, d_ell
    (through both sides' packed rows) and d_hyp[1]; d_ell and d_v1 may be None (csrc/assemble_matern.hip)"""
    P1, s1 = _req_pack(pack1, n1, p1, d, "pack1")
    P2, s2 = _req_pack(pack2, n2, p2, d, "pack2")
    vn1 = pack1[2] if len(pack1) > 2 else None
    isd = G.dtype == f64
    _req(G, f64 if isd else f32, "G", 2)
    if G.shape != (n1 * (p1 + 1), n2 * (p2 + 1)):
        raise ValueError("G has shape %s, expected %s" % (tuple(G.shape), (n1 * (p1 + 1), n2 * (p2 + 1))))
    _req_ell(ell, d)
    if d_ell is not None:
        _req_ell(d_ell, d)
    _req(d_x1, f32, "d_x1", 2)
    if d_x1.shape != (n1, d) or not d_x1.is_contiguous():
        raise ValueError("d_x1 must be contiguous [%d, %d]" % (n1, d))
    want_v = p1 > 0 and d_v1 is not None
    if want_v:
        _req(d_v1, f32, "d_v1", 2)
        if d_v1.shape != (n1 * p1, d) or not d_v1.is_contiguous() or vn1 is None:
            raise ValueError("d_v1 must be contiguous [%d, %d] and pack1 must carry its direction norms" % (n1 * p1, d))
    nbytes = kernel_bwd_matern52_workspace_bytes(n1, p1, n2, p2, d)
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=G.device)
    check(lib.dsvgp_kernel_bwd_matern52(ctx.h, _ptr(G), _ld(G), 1 if isd else 0, _ptr(P1), _ptr(s1), _ptr(vn1 if want_v else None), n1, p1,
                                        _ptr(P2), _ptr(s2), n2, p2, d, _ptr(ell), _ptr(hyp), 1 if symmetric else 0, _ptr(d_x1),
                                        _ptr(d_v1 if want_v else None), _ptr(d_ell), _ptr(d_hyp), _ptr(workspace)),
          "dsvgp_kernel_bwd_matern52")
    return workspace


def kernel_bwd_wide(ctx, G, pack1, n1, pack2, n2, d, p, hyp, symmetric, d_x1, d_v1, d_hyp, workspace=None):
    """kernel_bwd on the wide-input kernels whatever d (see kernel_fwd_wide)"""
    P1, s1, vn1 = pack1
    P2, s2 = pack2[0], pack2[1]
    isd = G.dtype == f64
    _req(G, f64 if isd else f32, "G", 2)
    nbytes = int(lib.dsvgp_kernel_bwd_wide_workspace_bytes(n1, n2, d, p))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=G.device)
    check(lib.dsvgp_kernel_bwd_wide(ctx.h, _ptr(G), _ld(G), 1 if isd else 0, _ptr(P1), _ptr(s1), _ptr(vn1), n1, _ptr(P2),
                                    _ptr(s2), n2, d, p, _ptr(hyp), 1 if symmetric else 0, _ptr(d_x1),
                                    _ptr(d_v1 if p > 0 else None), _ptr(d_hyp), _ptr(workspace)), "dsvgp_kernel_bwd_wide")
    return workspace


def potrf_workspace(n, device):
    """Scratch of the blocked MFMA Cholesky (inverted 64 x 64 diagonal blocks, W_k tiles).  Owned by the caller, ONE per
    factor: ``trtri_blocks`` later seeds its recursion from the blocks the factorisation left in it."""
    return torch.empty(int(lib.dsvgp_potrf_workspace_bytes(int(n), 1)), dtype=torch.uint8, device=device)


def _potrf_scratch(A, ws):
    need = int(lib.dsvgp_potrf_workspace_bytes(A.shape[0], 1))
    if ws is None:
        return potrf_workspace(A.shape[0], A.device)
    if not ws.is_cuda or ws.numel() * ws.element_size() < need:
        raise ValueError("potrf workspace too small: %d < %d" % (ws.numel() * ws.element_size(), need))
    return ws


def potrf_(ctx, A, info, algo=1, ws=None):
    """In-place lower Cholesky.  algo 0 = rocSOLVER dpotrf, 1 = blocked MFMA Cholesky (default).
    ``ws``: ``potrf_workspace(n)`` owned by the caller for THIS factor (a fresh one is allocated when omitted);
    returned so that ``trtri_blocks(..., potrf_ws=)`` can reuse the inverted diagonal blocks."""
    _req(A, f64, "A", 2)
    n = A.shape[0]
    if algo == 1:
        ws = _potrf_scratch(A, ws)
    else:
        ws = None
    check(lib.dsvgp_potrf(ctx.h, _ptr(A), n, _ld(A), _ptr(info), int(algo), _ptr(ws)), "dsvgp_potrf")
    return ws


def potrf_inverse_(ctx, A, info, nb, workspace, ws=None):
    """In-place lower Cholesky (blocked MFMA algorithm) AND the explicit inverse into the trsm workspace, in the same
    launches.  Only for nb >= n; later ``trsm(..., reuse_inverse=True)`` calls use the inverse.  ``ws`` as in ``potrf_``."""
    _req(A, f64, "A", 2)
    n = A.shape[0]
    ws = _potrf_scratch(A, ws)
    need = int(lib.dsvgp_trsm_workspace_bytes(n, n, int(nb)))       # the inverse and its transposed copy live there
    if workspace.numel() < need:
        raise ValueError("potrf_inverse_: trsm workspace too small: %d < %d" % (workspace.numel(), need))
    check(lib.dsvgp_potrf_inverse(ctx.h, _ptr(A), n, _ld(A), _ptr(info), _ptr(ws), int(nb), _ptr(workspace)),
          "dsvgp_potrf_inverse")
    return ws


def add_diag_(ctx, A, delta):
    check(lib.dsvgp_add_diag(ctx.h, _ptr(A), A.shape[0], _ld(A), float(delta)), "dsvgp_add_diag")


def trsm_workspace(n, nrhs, nb, device):
    return torch.empty(int(lib.dsvgp_trsm_workspace_bytes(n, nrhs, nb)), dtype=torch.uint8, device=device)


def trsm(ctx, L, B, trans, X64, X32, nb, workspace, reuse_inverse=False):
    _req(L, f64, "L", 2)
    isd = B.dtype == f64
    _req(B, f64 if isd else f32, "B", 2)
    if X64 is not None:
        _req(X64, f64, "X64", 2)
    n, nrhs = B.shape
    if L.shape != (n, n) or (X64 is not None and X64.shape != (n, nrhs)) or (X32 is not None and X32.shape != (n, nrhs)):
        raise ValueError("trsm shape mismatch")
    need = int(lib.dsvgp_trsm_workspace_bytes(n, nrhs, nb))
    if workspace.numel() < need:
        raise ValueError("trsm workspace too small: %d < %d" % (workspace.numel(), need))
    check(lib.dsvgp_trsm(ctx.h, _ptr(L), _ld(L), n, 1 if trans else 0, _ptr(B), _ld(B), 1 if isd else 0, nrhs,
                         _ptr(X64), _ld(X64) if X64 is not None else 0, _ptr(X32), _ld(X32) if X32 is not None else 0, nb,
                         _ptr(workspace),
                         1 if reuse_inverse else 0), "dsvgp_trsm")


def trtri_blocks(ctx, L, nrhs_max, nb, workspace, potrf_ws=None):
    """Invert the nb x nb diagonal blocks of L into the trsm workspace (the first phase of dsvgp_trsm).
    ``potrf_ws``: what ``potrf_(algo=1)`` returned for THIS L (its inverted 64 x 64 diagonal blocks are reused)."""
    _req(L, f64, "L", 2)
    n = L.shape[0]
    need = int(lib.dsvgp_trsm_workspace_bytes(n, nrhs_max, nb))
    if workspace.numel() < need:
        raise ValueError("trsm workspace too small: %d < %d" % (workspace.numel(), need))
    check(lib.dsvgp_trtri(ctx.h, _ptr(L), _ld(L), n, nb, _ptr(potrf_ws), _ptr(workspace)), "dsvgp_trtri")


def gemm(ctx, flags, A, B, C_out, alpha=1.0, beta=0.0, Cin=None, C32=None, kscale=None, M=None, N=None, K=None):
    """C_out = alpha*op(A)op(B) + beta*Cin on the MFMA GEMM; compute dtype = C_out.dtype."""
    isd = C_out.dtype == f64
    if M is None:
        M = A.shape[1] if flags & _lib.TRANS_A else A.shape[0]
    if K is None:
        K = A.shape[0] if flags & _lib.TRANS_A else A.shape[1]
    if N is None:
        N = B.shape[0] if flags & _lib.TRANS_B else B.shape[1]
    kb = B.shape[1] if flags & _lib.TRANS_B else B.shape[0]
    if kb < K or C_out.shape[0] < M or C_out.shape[1] < N:
        raise ValueError("gemm shape mismatch")
    _req(A, f64 if isd else f32, "A", 2)
    if isd and B.dtype == f32:
        flags |= _lib.B_IS_FLOAT
    else:
        _req(B, f64 if isd else f32, "B", 2)
    if Cin is not None and isd and Cin.dtype == f32:
        flags |= _lib.CIN_IS_FLOAT
    check(lib.dsvgp_gemm(ctx.h, 1 if isd else 0, flags, M, N, K, float(alpha), _ptr(A), _ld(A), _ptr(B), _ld(B),
                         float(beta), _ptr(Cin), _ld(Cin) if Cin is not None else 0, _ptr(C_out), _ld(C_out),
                         _ptr(C32), _ld(C32) if C32 is not None else 0, _ptr(kscale)), "dsvgp_gemm")
    return C_out


def split3_bf16(ctx, src, transpose=False, out=None):
    """three bf16 planes of the float32 matrix ``src`` [R, C] (or of its transpose): uint8 buffer holding 3 x rows_out x kpad(K) bf16"""
    _req(src, f32, "src", 2)
    R, Cc = src.shape
    rows_out, K = (Cc, R) if transpose else (R, Cc)
    nbytes = int(lib.dsvgp_split3_bytes(rows_out, K))
    if out is None or out.numel() < nbytes:
        out = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    check(lib.dsvgp_split3_bf16(ctx.h, _ptr(src), _ld(src), R, Cc, 1 if transpose else 0, _ptr(out)), "dsvgp_split3_bf16")
    return out


def gemm3b(ctx, flags, M, N, K, Aplanes, a_rows, Bplanes, b_rows, C, alpha=1.0):
    """C[M, N] = alpha A B^T on the bf16 matrix pipe from plane triples (csrc/gemm3b.hip)"""
    _req(C, f32, "C", 2)
    check(lib.dsvgp_gemm3b(ctx.h, int(flags), int(M), int(N), int(K), float(alpha), _ptr(Aplanes), int(a_rows), _ptr(Bplanes), int(b_rows),
                           _ptr(C), _ld(C)), "dsvgp_gemm3b")
    return C


def widen_f32_f64(ctx, src, dst):
    """dst (float64) = src (float32), both 2-D with unit inner stride"""
    M, N = src.shape
    check(lib.dsvgp_widen_f32_f64(ctx.h, _ptr(_req(src, f32, "src", 2)), _ld(src), _ptr(_req(dst, f64, "dst", 2)), _ld(dst), M, N),
          "dsvgp_widen_f32_f64")
    return dst


def predictive_stats(ctx, A, W, p, m, constant, hyp, mu, var, workspace=None):
    Mp, nc = A.shape
    nbytes = int(lib.dsvgp_stats_workspace_bytes(Mp, nc))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=A.device)
    check(lib.dsvgp_predictive_stats(ctx.h, _ptr(_req(A, f32, "A", 2)), _ld(A), _ptr(_req(W, f32, "W", 2)), _ld(W), Mp,
                                     nc, p, _ptr(m), _ptr(constant), _ptr(hyp), _ptr(mu), _ptr(var), _ptr(workspace)),
          "dsvgp_predictive_stats")
    return workspace


def predictive_blocks(ctx, A, W, pd, packX, d, hyp, with_noise, out=None):
    """out[B, pd + 1, pd + 1] = the diagonal blocks of s K_XX + (1e-4 + noise) I + W^T W - A^T A, one per data point, from
    A = L^-1 K_ZX and W = L_S^T A [Mp, B (pd + 1)] (float32, interleaved columns); ``W`` None (or ``A`` itself): zero middle term.
    ``packX``: the data pack of ``pack_points`` made with ``pd`` directions per point (its unit direction rows are read; may be
    None at pd = 0).  Nothing of size B (pd + 1) squared is formed (dsvgp_predictive_blocks, csrc/predict_blocks.hip)."""
    _req(A, f32, "A", 2)
    Mp, nc = A.shape
    q = int(pd) + 1
    if pd < 0 or pd > 95:
        raise ValueError("at most 95 derivative directions per data point, got %d" % pd)
    if nc == 0 or nc % q:
        raise ValueError("A has %d columns, not a positive multiple of pd + 1 = %d" % (nc, q))
    B = nc // q
    if W is not None:
        _req(W, f32, "W", 2)
        if W.shape != A.shape:
            raise ValueError("W has shape %s, A %s" % (tuple(W.shape), tuple(A.shape)))
    PX = None
    if pd > 0:
        if packX is None:
            raise ValueError("the data pack is needed at pd > 0 (its unit direction rows)")
        PX = _req(packX[0], f32, "packX", 2)
        if PX.shape != (nc, packed_width(d)) or not PX.is_contiguous():
            raise ValueError("packX is not the contiguous pack of %d points with %d directions at d = %d" % (B, pd, d))
    _req(hyp, f32, "hyp", 1)
    shape = (B, q, q)
    if out is None:
        out = torch.empty(shape, dtype=f32, device=A.device)
    if not out.is_cuda or out.dtype != f32 or out.shape != shape or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 GPU tensor of shape %s" % (shape,))
    nbytes = int(lib.dsvgp_predictive_blocks_workspace_bytes(Mp, B, int(pd)))
    if nbytes == 0:
        raise ValueError("dsvgp_predictive_blocks does not take Mp = %d, B = %d, pd = %d" % (Mp, B, pd))
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=A.device)
    check(lib.dsvgp_predictive_blocks(ctx.h, _ptr(A), _ld(A), _ptr(W), _ld(W) if W is not None else 0, Mp, B, int(pd), _ptr(PX), int(d),
                                      _ptr(hyp), 1 if with_noise else 0, _ptr(out), _ptr(workspace), nbytes), "dsvgp_predictive_blocks")
    return out


def _req_blocks(t, dtype, name, shape=None, dims=None):
    # (dtype, shape and contiguity first: a bad argument is refused before any device is asked for)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if dims is not None and t.dim() != dims:
        raise ValueError("%s must be %d-D, got shape %s" % (name, dims, tuple(t.shape)))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _blocks_q(t, name):
    if t.dim() != 3 or t.shape[1] != t.shape[2]:
        raise ValueError("%s must be [B, q, q], got shape %s" % (name, tuple(t.shape)))
    B, q = int(t.shape[0]), int(t.shape[1])
    if q < 1 or q > 96:
        raise ValueError("at most 95 derivative directions per data point, got %d" % (q - 1))
    return B, q


def _on_gpu(*named):
    for name, t in named:
        if t is not None and not t.is_cuda:
            raise _lib.DsvgpError("%s must live on the GPU: the DSVGP hot path has no CPU fallback" % name)


def blocks_factor(ctx, blocks, jitter=0.0):
    """(roots f64 [B, q, q], logdet f64 [B], info i32 [B], status i32 [1]) of float32 ``blocks`` [B, q, q], q <= 96: roots[b] the lower
    Cholesky factor of (double) blocks[b] + jitter I (strict upper part 0), logdet[b] = 2 sum log diag, info[b] = 0 or k + 1 for a
    failed pivot k (that block's root and logdet are NaN, every other block is unaffected), status = max(info).  Nothing is read
    back here (dsvgp_blocks_factor, csrc/block_roots.hip)."""
    _req_blocks(blocks, f32, "blocks")
    B, q = _blocks_q(blocks, "blocks")
    _on_gpu(("blocks", blocks))
    roots = torch.empty(B, q, q, dtype=f64, device=blocks.device)
    logdet = torch.empty(B, dtype=f64, device=blocks.device)
    info = torch.empty(B, dtype=torch.int32, device=blocks.device)
    status = torch.zeros(1, dtype=torch.int32, device=blocks.device)
    if B == 0:                                                                        # (an empty tensor has no address to pass)
        return roots, logdet, info, status
    check(lib.dsvgp_blocks_factor(ctx.h, _ptr(blocks), B, q, float(jitter), _ptr(roots), _ptr(logdet), _ptr(info), _ptr(status)),
          "dsvgp_blocks_factor")
    return roots, logdet, info, status


def blocks_draw(ctx, roots, mu, eps):
    """out[n, B q] (float32) = mu + the per-point product roots[b] eps[i, b q : (b + 1) q]: ``roots`` f64 [B, q, q] of
    ``blocks_factor``, ``mu`` float32 with B q entries, ``eps`` float32 [n, B q] (dsvgp_blocks_draw)."""
    _req_blocks(roots, f64, "roots")
    B, q = _blocks_q(roots, "roots")
    _req_blocks(mu, f32, "mu")
    if mu.numel() != B * q:
        raise ValueError("mu has %d entries, not B q = %d x %d" % (mu.numel(), B, q))
    _req_blocks(eps, f32, "eps", dims=2)
    if eps.shape[1] != B * q:
        raise ValueError("eps has %d columns, not B q = %d x %d" % (eps.shape[1], B, q))
    _on_gpu(("roots", roots), ("mu", mu), ("eps", eps))
    n = int(eps.shape[0])
    out = torch.empty(n, B * q, dtype=f32, device=roots.device)
    if n == 0 or B == 0:
        return out
    check(lib.dsvgp_blocks_draw(ctx.h, _ptr(roots), _ptr(mu), _ptr(eps), B, q, n, _ptr(out)), "dsvgp_blocks_draw")
    return out


def blocks_logpdf(ctx, roots, logdet, mu, y, want_z=True):
    """(z float32 [B, q] or None, logp float32 [B]): z[b] = roots[b]^-1 (y[b] - mu[b]) and the joint normal log-density
    -|z|^2 / 2 - logdet[b] / 2 - q log(2 pi) / 2 of every block; ``mu`` and ``y`` float32 with B q entries (dsvgp_blocks_logpdf)."""
    _req_blocks(roots, f64, "roots")
    B, q = _blocks_q(roots, "roots")
    _req_blocks(logdet, f64, "logdet", shape=(B,))
    _req_blocks(mu, f32, "mu")
    _req_blocks(y, f32, "y")
    if mu.numel() != B * q:
        raise ValueError("mu has %d entries, not B q = %d x %d" % (mu.numel(), B, q))
    if y.numel() != B * q:
        raise ValueError("y has %d entries, not B q = %d x %d" % (y.numel(), B, q))
    _on_gpu(("roots", roots), ("logdet", logdet), ("mu", mu), ("y", y))
    z = torch.empty(B, q, dtype=f32, device=roots.device) if want_z else None
    logp = torch.empty(B, dtype=f32, device=roots.device)
    if B == 0:
        return z, logp
    check(lib.dsvgp_blocks_logpdf(ctx.h, _ptr(roots), _ptr(logdet), _ptr(mu), _ptr(y), B, q, _ptr(z), _ptr(logp)), "dsvgp_blocks_logpdf")
    return z, logp


def mean_weights_bytes(M, d):
    return int(lib.dsvgp_mean_weights_bytes(int(M), int(d)))


def mean_workspace_bytes(M, d, B, pd):
    return int(lib.dsvgp_mean_workspace_bytes(int(M), int(d), int(B), int(pd)))


def mean_prepare(ctx, alpha, Z, V, p, hyp, constant, center=None, weights=None):
    """alpha = L^-T m (float64 [M(p+1)]) and the inducing set -> the packed fp32 weights of the posterior-mean predictor
    (dsvgp_mean_prepare; a float32 tensor of dsvgp_mean_weights_bytes(M, d) bytes)"""
    _req(Z, f32, "Z", 2)
    M, d = Z.shape
    _req(alpha, f64, "alpha", 1)
    if alpha.shape[0] != M * (p + 1):
        raise ValueError("alpha must have M (p + 1) = %d entries, got %d" % (M * (p + 1), alpha.shape[0]))
    if p > 0:
        _req(V, f32, "V", 2)
        if V.shape != (M * p, d):
            raise ValueError("directions must be [M*p, d] = [%d, %d], got %s" % (M * p, d, tuple(V.shape)))
    if not Z.is_contiguous() or (p > 0 and not V.is_contiguous()):
        raise ValueError("Z and V must be contiguous")
    if center is not None:
        _req(center, f32, "center", 1)
        if center.shape != (d,):
            raise ValueError("center must have shape [%d]" % d)
    constant = _req(constant.reshape(-1), f32, "constant")
    n = (mean_weights_bytes(M, d) + 3) // 4
    if weights is None:
        weights = torch.empty(n, dtype=f32, device=Z.device)
    _req(weights, f32, "weights", 1)
    if weights.numel() < n:
        raise ValueError("weights buffer too small: %d < %d floats" % (weights.numel(), n))
    check(lib.dsvgp_mean_prepare(ctx.h, _ptr(alpha), _ptr(Z), _ptr(V if p > 0 else None), M, d, p, _ptr(hyp), _ptr(constant),
                                 _ptr(center), _ptr(weights)), "dsvgp_mean_prepare")
    return weights


def mean_predict(ctx, weights, M, d, x, D=None, pd=0, mean_out=None, grad_out=None, workspace=None):
    """mean_out[B(pd+1)] (interleaved) and, when ``grad_out`` [B, d] is given, the gradient of the mean without the constant
    (dsvgp_mean_predict).  ``workspace``: uint8 tensor of dsvgp_mean_workspace_bytes(M, d, B, pd) bytes (None when that is 0)."""
    _req(x, f32, "x", 2)
    _req(weights, f32, "weights", 1)
    B = x.shape[0]
    if x.shape[1] != d or not x.is_contiguous():
        raise ValueError("x must be a contiguous [B, %d] tensor, got %s" % (d, tuple(x.shape)))
    if pd > 0:
        _req(D, f32, "D", 2)
        if D.shape != (B * pd, d) or not D.is_contiguous():
            raise ValueError("directions must be a contiguous [B*pd, d] = [%d, %d] tensor, got %s" % (B * pd, d, tuple(D.shape)))
    if mean_out is None:
        mean_out = torch.empty(B * (pd + 1), dtype=f32, device=x.device)
    _req(mean_out, f32, "mean_out", 1)
    if mean_out.numel() != B * (pd + 1):
        raise ValueError("mean_out must have B (pd + 1) = %d entries" % (B * (pd + 1)))
    if grad_out is not None:
        _req(grad_out, f32, "grad_out", 2)
        if grad_out.shape != (B, d) or not grad_out.is_contiguous():
            raise ValueError("grad_out must be a contiguous [%d, %d] tensor" % (B, d))
    need = mean_workspace_bytes(M, d, B, pd)
    if need and (workspace is None or workspace.numel() * workspace.element_size() < need):
        raise ValueError("mean_predict workspace too small: %d bytes needed" % need)
    check(lib.dsvgp_mean_predict(ctx.h, _ptr(weights), M, d, _ptr(x), B, _ptr(D if pd > 0 else None), pd, _ptr(mean_out),
                                 _ptr(grad_out), _ptr(workspace if need else None)), "dsvgp_mean_predict")
    return mean_out


def paths_weights_bytes(M, d, F, n):
    return int(lib.dsvgp_paths_weights_bytes(int(M), int(d), int(F), int(n)))


def paths_workspace_bytes(M, d, F, n, B, want_grad):
    return int(lib.dsvgp_paths_workspace_bytes(int(M), int(d), int(F), int(n), int(B), 1 if want_grad else 0))


def paths_prepare(ctx, nu, w, omega, phase, Z, V, p, hyp, constant, center=None, weights=None):
    """nu [n, M(p+1)], w [n, F], omega [F, d], phase [F] (float64) and the inducing set -> the packed fp32 weights of n posterior
    paths (dsvgp_paths_prepare; a float32 tensor of dsvgp_paths_weights_bytes(M, d, F, n) bytes)"""
    _req(Z, f32, "Z", 2)
    M, d = Z.shape
    _req(nu, f64, "nu", 2)
    _req(w, f64, "w", 2)
    _req(omega, f64, "omega", 2)
    _req(phase, f64, "phase", 1)
    n, F = w.shape
    if nu.shape != (n, M * (p + 1)):
        raise ValueError("nu must be [n, M (p + 1)] = [%d, %d], got %s" % (n, M * (p + 1), tuple(nu.shape)))
    if omega.shape != (F, d) or phase.shape != (F,):
        raise ValueError("omega / phase must be [F, d] / [F] = [%d, %d] / [%d], got %s / %s"
                         % (F, d, F, tuple(omega.shape), tuple(phase.shape)))
    if p > 0:
        _req(V, f32, "V", 2)
        if V.shape != (M * p, d):
            raise ValueError("directions must be [M*p, d] = [%d, %d], got %s" % (M * p, d, tuple(V.shape)))
    if not (Z.is_contiguous() and nu.is_contiguous() and w.is_contiguous() and omega.is_contiguous()) or (p > 0 and not V.is_contiguous()):
        raise ValueError("Z, V, nu, w and omega must be contiguous")
    if center is not None:
        _req(center, f32, "center", 1)
        if center.shape != (d,):
            raise ValueError("center must have shape [%d]" % d)
    constant = _req(constant.reshape(-1), f32, "constant")
    nfl = (paths_weights_bytes(M, d, F, n) + 3) // 4
    if nfl == 0:
        raise ValueError("paths_prepare: M, d, F, n = %d, %d, %d, %d is not a shape the entry takes" % (M, d, F, n))
    if weights is None:
        weights = torch.empty(nfl, dtype=f32, device=Z.device)
    _req(weights, f32, "weights", 1)
    if weights.numel() < nfl:
        raise ValueError("weights buffer too small: %d < %d floats" % (weights.numel(), nfl))
    check(lib.dsvgp_paths_prepare(ctx.h, _ptr(nu), _ptr(w), _ptr(omega), _ptr(phase), _ptr(Z), _ptr(V if p > 0 else None), M, d, p, F, n,
                                  _ptr(hyp), _ptr(constant), _ptr(center), _ptr(weights)), "dsvgp_paths_prepare")
    return weights


def paths_eval(ctx, weights, M, d, F, n, x, values=None, grads=None, workspace=None):
    """values [n, B] and, when ``grads`` [n, B, d] is given, the gradients of n posterior paths at x [B, d] (dsvgp_paths_eval).
    ``workspace``: uint8 tensor of dsvgp_paths_workspace_bytes(M, d, F, n, B, grads is not None) bytes (None when that is 0)."""
    _req(x, f32, "x", 2)
    _req(weights, f32, "weights", 1)
    B = x.shape[0]
    if x.shape[1] != d or not x.is_contiguous():
        raise ValueError("x must be a contiguous [B, %d] tensor, got %s" % (d, tuple(x.shape)))
    if values is None:
        values = torch.empty(n, B, dtype=f32, device=x.device)
    _req(values, f32, "values", 2)
    if values.shape != (n, B) or not values.is_contiguous():
        raise ValueError("values must be a contiguous [%d, %d] tensor" % (n, B))
    if grads is not None:
        if not grads.is_cuda or grads.dtype != f32 or grads.shape != (n, B, d) or not grads.is_contiguous():
            raise ValueError("grads must be a contiguous float32 [%d, %d, %d] tensor on the GPU" % (n, B, d))
    need = paths_workspace_bytes(M, d, F, n, B, grads is not None)
    if need and (workspace is None or workspace.numel() * workspace.element_size() < need):
        raise ValueError("paths_eval workspace too small: %d bytes needed" % need)
    check(lib.dsvgp_paths_eval(ctx.h, _ptr(weights), M, d, F, n, _ptr(x), B, _ptr(values), _ptr(grads),
                               _ptr(workspace if need else None)), "dsvgp_paths_eval")
    return values


def paths_hvp_workspace_bytes(M, d, F, n, B):
    return int(lib.dsvgp_paths_hvp_workspace_bytes(int(M), int(d), int(F), int(n), int(B)))


def paths_hvp(ctx, weights, M, d, F, n, x, v, hv=None, workspace=None):
    """hv [n, B, d] = grad^2 f_s(x_b) v_b: the Hessian-vector products of n posterior paths at x [B, d] with one vector per point
    v [B, d], shared by the samples and used as given (dsvgp_paths_hvp).  ``workspace``: uint8 tensor of
    dsvgp_paths_hvp_workspace_bytes(M, d, F, n, B) bytes (None when that is 0)."""
    _req(x, f32, "x", 2)
    _req(v, f32, "v", 2)
    _req(weights, f32, "weights", 1)
    B = x.shape[0]
    if x.shape[1] != d or not x.is_contiguous():
        raise ValueError("x must be a contiguous [B, %d] tensor, got %s" % (d, tuple(x.shape)))
    if v.shape != (B, d) or not v.is_contiguous():
        raise ValueError("v must be a contiguous [B, d] = [%d, %d] tensor, got %s" % (B, d, tuple(v.shape)))
    if hv is None:
        hv = torch.empty(n, B, d, dtype=f32, device=x.device)
    if not hv.is_cuda or hv.dtype != f32 or hv.shape != (n, B, d) or not hv.is_contiguous():
        raise ValueError("hv must be a contiguous float32 [%d, %d, %d] tensor on the GPU" % (n, B, d))
    need = paths_hvp_workspace_bytes(M, d, F, n, B)
    if need and (workspace is None or workspace.numel() * workspace.element_size() < need):
        raise ValueError("paths_hvp workspace too small: %d bytes needed" % need)
    check(lib.dsvgp_paths_hvp(ctx.h, _ptr(weights), M, d, F, n, _ptr(x), _ptr(v), B, _ptr(hv), _ptr(workspace if need else None)),
          "dsvgp_paths_hvp")
    return hv


def paths_own_workspace_bytes(M, d, F, n, B, want_grad):
    return int(lib.dsvgp_paths_own_workspace_bytes(int(M), int(d), int(F), int(n), int(B), 1 if want_grad else 0))


def _req_own(t, shape, name, dtype=f32):
    if not t.is_cuda or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s %s tensor on the GPU, got %s %s"
                         % (name, str(dtype).replace("torch.", ""), list(shape), t.dtype, tuple(t.shape)))
    return t


def paths_eval_own(ctx, weights, M, d, F, n, x, values=None, grads=None, workspace=None):
    """values [n, B] = f_s(x[s][b]) and, when ``grads`` [n, B, d] is given, the gradients of n posterior paths, each at its OWN points
    x [n, B, d] (dsvgp_paths_eval_own).  ``workspace``: uint8 tensor of dsvgp_paths_own_workspace_bytes(M, d, F, n, B, grads is not
    None) bytes (None when that is 0)."""
    _req(x, f32, "x", 3)
    _req(weights, f32, "weights", 1)
    if x.shape[0] != n or x.shape[2] != d or not x.is_contiguous():
        raise ValueError("x must be a contiguous [%d, B, %d] tensor, got %s" % (n, d, tuple(x.shape)))
    B = x.shape[1]
    if values is None:
        values = torch.empty(n, B, dtype=f32, device=x.device)
    _req_own(values, (n, B), "values")
    if grads is not None:
        _req_own(grads, (n, B, d), "grads")
    need = paths_own_workspace_bytes(M, d, F, n, B, grads is not None)
    if need and (workspace is None or workspace.numel() * workspace.element_size() < need):
        raise ValueError("paths_eval_own workspace too small: %d bytes needed" % need)
    check(lib.dsvgp_paths_eval_own(ctx.h, _ptr(weights), M, d, F, n, _ptr(x), B, _ptr(values), _ptr(grads),
                                   _ptr(workspace if need else None)), "dsvgp_paths_eval_own")
    return values


def paths_descend_workspace_bytes(M, d, F, n, B):
    return int(lib.dsvgp_paths_descend_workspace_bytes(int(M), int(d), int(F), int(n), int(B)))


def paths_descend(ctx, weights, M, d, F, n, x, lower, upper, iterations, initial_step, maximize, resume, values, grads, steps, accepted,
                  workspace):
    """``iterations`` projected gradient steps of every (sample, start) pair on its own path, in place on x [n, B, d] and the state
    tensors values [n, B], grads [n, B, d], steps [n, B] (float32) and accepted [n, B] (int32) (dsvgp_paths_descend).  ``workspace``:
    uint8 tensor of dsvgp_paths_descend_workspace_bytes(M, d, F, n, B) bytes."""
    _req(x, f32, "x", 3)
    _req(weights, f32, "weights", 1)
    if x.shape[0] != n or x.shape[2] != d or not x.is_contiguous():
        raise ValueError("x must be a contiguous [%d, B, %d] tensor, got %s" % (n, d, tuple(x.shape)))
    B = x.shape[1]
    _req_own(lower, (d,), "lower")
    _req_own(upper, (d,), "upper")
    _req_own(values, (n, B), "values")
    _req_own(grads, (n, B, d), "grads")
    _req_own(steps, (n, B), "steps")
    _req_own(accepted, (n, B), "accepted", torch.int32)
    need = paths_descend_workspace_bytes(M, d, F, n, B)
    if need == 0:
        raise ValueError("paths_descend: M, d, F, n, B = %d, %d, %d, %d, %d is not a shape the entry takes" % (M, d, F, n, B))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        raise ValueError("paths_descend workspace too small: %d bytes needed" % need)
    check(lib.dsvgp_paths_descend(ctx.h, _ptr(weights), M, d, F, n, _ptr(x), B, _ptr(lower), _ptr(upper), int(iterations),
                                  float(initial_step), 1 if maximize else 0, 1 if resume else 0, _ptr(values), _ptr(grads), _ptr(steps),
                                  _ptr(accepted), _ptr(workspace)), "dsvgp_paths_descend")
    return x


ACQ_KINDS = {"lcb_var": 0, "lcb": 1, "ei": 2}


def var_route(d, p):
    """route of dsvgp_var_predict for (d, p): "fused", "composed", or None for arguments it refuses"""
    return {1: "fused", 2: "composed"}.get(int(lib.dsvgp_var_route(int(d), int(p))))


def var_chunk(d, p):
    """inducing points per LDS chunk of the fused variance kernel (0: the composed route)"""
    return int(lib.dsvgp_var_chunk(int(d), int(p)))


def var_weights_bytes(M, d, p):
    return int(lib.dsvgp_var_weights_bytes(int(M), int(d), int(p)))


def var_workspace_bytes(M, d, p, B, want_grad):
    return int(lib.dsvgp_var_workspace_bytes(int(M), int(d), int(p), int(B), 1 if want_grad else 0))


def acq_descend_workspace_bytes(M, d, p, B):
    return int(lib.dsvgp_acq_descend_workspace_bytes(int(M), int(d), int(p), int(B)))


def var_prepare(ctx, Z, V, p, hyp, center=None, weights=None):
    """the inducing set -> the packed fp32 weights of the posterior-variance predictor (dsvgp_var_prepare; a float32 tensor of
    dsvgp_var_weights_bytes(M, d, p) bytes)"""
    _req(Z, f32, "Z", 2)
    M, d = Z.shape
    if p > 0:
        _req(V, f32, "V", 2)
        if V.shape != (M * p, d):
            raise ValueError("directions must be [M*p, d] = [%d, %d], got %s" % (M * p, d, tuple(V.shape)))
    if not Z.is_contiguous() or (p > 0 and not V.is_contiguous()):
        raise ValueError("Z and V must be contiguous")
    if center is not None:
        _req(center, f32, "center", 1)
        if center.shape != (d,):
            raise ValueError("center must have shape [%d]" % d)
    n = (var_weights_bytes(M, d, p) + 3) // 4
    if n == 0:
        raise ValueError("var_prepare: M, d, p = %d, %d, %d is not a shape the entry takes" % (M, d, p))
    if weights is None:
        weights = torch.empty(n, dtype=f32, device=Z.device)
    _req(weights, f32, "weights", 1)
    if weights.numel() < n:
        raise ValueError("weights buffer too small: %d < %d floats" % (weights.numel(), n))
    check(lib.dsvgp_var_prepare(ctx.h, _ptr(Z), _ptr(V if p > 0 else None), M, d, p, _ptr(hyp), _ptr(center), _ptr(weights)),
          "dsvgp_var_prepare")
    return weights


def _req_var_state(weights, Q, packZ, M, d, p):
    _req(weights, f32, "weights", 1)
    _req(Q, f64, "Q", 2)
    Mp = M * (p + 1)
    if Q.shape != (Mp, Mp):
        raise ValueError("Q must be [M (p + 1)]^2 = [%d, %d], got %s" % (Mp, Mp, tuple(Q.shape)))
    PZ, sZ = packZ[0], packZ[1]
    _req(PZ, f32, "packZ", 2)
    _req(sZ, f32, "packZ self terms", 1)
    if PZ.shape != (Mp, packed_width(d)) or sZ.shape[0] != Mp or not PZ.is_contiguous():
        raise ValueError("packZ is not the contiguous pack of %d points with %d directions at d = %d" % (M, p, d))
    return PZ, sZ


def var_predict(ctx, weights, Q, packZ, hyp, M, d, p, x, var_out=None, grad_out=None, workspace=None):
    """var_out [B] = sigma^2 of q(f) at x [B, d] (no likelihood noise) and, when ``grad_out`` [B, d] is given, its gradient
    (dsvgp_var_predict).  ``Q``: float64 [M', M'], symmetric; ``packZ``: ``pack_points`` of the inducing set with the centre the weights
    carry.  ``workspace``: uint8 tensor of dsvgp_var_workspace_bytes(M, d, p, B, grad_out is not None) bytes."""
    PZ, sZ = _req_var_state(weights, Q, packZ, M, d, p)
    _req(x, f32, "x", 2)
    B = x.shape[0]
    if x.shape[1] != d or not x.is_contiguous():
        raise ValueError("x must be a contiguous [B, %d] tensor, got %s" % (d, tuple(x.shape)))
    if var_out is None:
        var_out = torch.empty(B, dtype=f32, device=x.device)
    _req_own(var_out, (B,), "var_out")
    if grad_out is not None:
        _req_own(grad_out, (B, d), "grad_out")
    need = var_workspace_bytes(M, d, p, B, grad_out is not None)
    if need == 0:
        raise ValueError("var_predict: M, d, p, B = %d, %d, %d, %d is not a shape the entry takes (split the batch)" % (M, d, p, B))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        raise ValueError("var_predict workspace too small: %d bytes needed" % need)
    check(lib.dsvgp_var_predict(ctx.h, _ptr(weights), _ptr(Q), _ld(Q), _ptr(PZ), _ptr(sZ), _ptr(hyp), M, d, p, _ptr(x), B, _ptr(var_out),
                                _ptr(grad_out), _ptr(workspace)), "dsvgp_var_predict")
    return var_out


def acq_eval(ctx, kind, maximize, beta, best, mu, gmu, var, gvar, d, out=None, gout=None):
    """acquisition values out [B] and, when ``gout`` [B, d] is given, gradients from mu [B], gmu [B, d], var [B], gvar [B, d]
    (dsvgp_acq_eval; without ``gout`` the two gradients may be None).  ``kind``: a key of ACQ_KINDS; ``beta`` / ``best``: device float32
    scalars (the unused one may be None)."""
    B = mu.shape[0]
    _req_own(mu, (B,), "mu")
    _req_own(var, (B,), "var")
    if gout is not None:
        _req_own(gmu, (B, d), "gmu")
        _req_own(gvar, (B, d), "gvar")
        _req_own(gout, (B, d), "gout")
    if out is None:
        out = torch.empty(B, dtype=f32, device=mu.device)
    _req_own(out, (B,), "out")
    for name, t in (("beta", beta), ("best", best)):
        if t is not None:
            _req_own(t, t.shape, name)
    check(lib.dsvgp_acq_eval(ctx.h, ACQ_KINDS[kind], 1 if maximize else 0, _ptr(beta), _ptr(best), _ptr(mu), _ptr(gmu), _ptr(var), _ptr(gvar),
                             B, d, _ptr(out), _ptr(gout)), "dsvgp_acq_eval")
    return out


def acq_descend(ctx, mean_weights, weights, Q, packZ, hyp, M, d, p, x, lower, upper, kind, beta, best, maximize, iterations, initial_step,
                resume, values, grads, steps, accepted, workspace):
    """``iterations`` projected gradient steps of B starts on the acquisition, in place on x [B, d] and the state tensors values [B],
    grads [B, d], steps [B] (float32) and accepted [B] (int32) (dsvgp_acq_descend).  ``workspace``: uint8 tensor of
    dsvgp_acq_descend_workspace_bytes(M, d, p, B) bytes."""
    PZ, sZ = _req_var_state(weights, Q, packZ, M, d, p)
    _req(mean_weights, f32, "mean_weights", 1)
    _req(x, f32, "x", 2)
    B = x.shape[0]
    _req_own(x, (B, d), "x")
    _req_own(lower, (d,), "lower")
    _req_own(upper, (d,), "upper")
    _req_own(values, (B,), "values")
    _req_own(grads, (B, d), "grads")
    _req_own(steps, (B,), "steps")
    _req_own(accepted, (B,), "accepted", torch.int32)
    for name, t in (("beta", beta), ("best", best)):
        if t is not None:
            _req_own(t, t.shape, name)
    need = acq_descend_workspace_bytes(M, d, p, B)
    if need == 0:
        raise ValueError("acq_descend: M, d, p, B = %d, %d, %d, %d is not a shape the entry takes" % (M, d, p, B))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        raise ValueError("acq_descend workspace too small: %d bytes needed" % need)
    check(lib.dsvgp_acq_descend(ctx.h, _ptr(mean_weights), _ptr(weights), _ptr(Q), _ld(Q), _ptr(PZ), _ptr(sZ), _ptr(hyp), M, d, p, _ptr(x), B,
                                _ptr(lower), _ptr(upper), ACQ_KINDS[kind], _ptr(beta), _ptr(best), 1 if maximize else 0, int(iterations),
                                float(initial_step), 1 if resume else 0, _ptr(values), _ptr(grads), _ptr(steps), _ptr(accepted),
                                _ptr(workspace)), "dsvgp_acq_descend")
    return x


def likelihood_terms(ctx, mu, var, y, p, hyp, mll_type, global_rows, mu_bar, var_bar, varn, scalars):
    check(lib.dsvgp_likelihood_terms(ctx.h, _ptr(mu), _ptr(var), _ptr(_req(y, f32, "y", 1)), mu.shape[0], p, _ptr(hyp),
                                     int(mll_type), float(global_rows), _ptr(mu_bar), _ptr(var_bar), _ptr(varn),
                                     _ptr(scalars)), "dsvgp_likelihood_terms")


def likelihood_terms_masked_workspace(device):
    """scratch of ``likelihood_terms_masked`` (per-workgroup counts and partial sums; a fixed size)"""
    return torch.empty(int(lib.dsvgp_likelihood_terms_masked_workspace_bytes()), dtype=torch.uint8, device=device)


def likelihood_terms_masked(ctx, mu, var, y, p, hyp, mll_type, mu_bar, var_bar, varn, scalars, n_present, workspace):
    """``likelihood_terms`` over the rows whose target is not NaN (csrc/missing.hip): exact zeros on the missing rows, scalars normalised
    by the device-side count (``step_epilogue`` then takes rows = 1), the count itself in ``n_present`` (int32 [1]).  No host read."""
    for t, name in ((mu, "mu"), (var, "var"), (mu_bar, "mu_bar"), (var_bar, "var_bar"), (varn, "varn")):
        _req(t, f32, name, 1)
        if t.numel() != y.numel():
            raise ValueError("%s must have B' = %d entries, got %d" % (name, y.numel(), t.numel()))
    if scalars.dtype != f32 or scalars.numel() < 8 or n_present.dtype != torch.int32 or n_present.numel() < 1:
        raise ValueError("scalars must be 8 float32 values and n_present one int32")
    if workspace is None or workspace.numel() * workspace.element_size() < int(lib.dsvgp_likelihood_terms_masked_workspace_bytes()):
        raise ValueError("likelihood_terms_masked needs the workspace of likelihood_terms_masked_workspace()")
    check(lib.dsvgp_likelihood_terms_masked(ctx.h, _ptr(mu), _ptr(var), _ptr(_req(y, f32, "y", 1)), y.numel(), int(p), _ptr(hyp),
                                            int(mll_type), _ptr(mu_bar), _ptr(var_bar), _ptr(varn), _ptr(scalars), _ptr(n_present),
                                            _ptr(workspace)), "dsvgp_likelihood_terms_masked")


def likelihood_terms_classes_workspace(device):
    """scratch of ``likelihood_terms_classes`` (per-workgroup partial sums; a fixed size)"""
    return torch.empty(int(lib.dsvgp_likelihood_terms_classes_workspace_bytes()), dtype=torch.uint8, device=device)


def likelihood_terms_classes(ctx, mu, var, y, p, hyp, mll_type, global_rows, mu_bar, var_bar, varn, scalars, workspace):
    """``likelihood_terms`` with one noise per output class (csrc/noise_classes.hip): hyp[2] on the value rows (j % (p + 1) == 0), hyp[3]
    on the derivative rows.  scalars[1] = d loss / d hyp[2] (value rows), scalars[5] = d loss / d hyp[3] (derivative rows); fixed-order
    sums, no host read."""
    for t, name in ((mu, "mu"), (var, "var"), (mu_bar, "mu_bar"), (var_bar, "var_bar"), (varn, "varn")):
        _req(t, f32, name, 1)
        if t.numel() != y.numel():
            raise ValueError("%s must have B' = %d entries, got %d" % (name, y.numel(), t.numel()))
    if scalars.dtype != f32 or scalars.numel() < 8 or hyp.dtype != f32 or hyp.numel() < 4:
        raise ValueError("scalars must be 8 float32 values and hyp 4")
    if workspace is None or workspace.numel() * workspace.element_size() < int(lib.dsvgp_likelihood_terms_classes_workspace_bytes()):
        raise ValueError("likelihood_terms_classes needs the workspace of likelihood_terms_classes_workspace()")
    check(lib.dsvgp_likelihood_terms_classes(ctx.h, _ptr(mu), _ptr(var), _ptr(_req(y, f32, "y", 1)), y.numel(), int(p), _ptr(hyp),
                                             int(mll_type), float(global_rows), _ptr(mu_bar), _ptr(var_bar), _ptr(varn), _ptr(scalars),
                                             _ptr(workspace)), "dsvgp_likelihood_terms_classes")


def abar(ctx, A, U, m, mu_bar, var_bar, out):
    Mp, nc = A.shape
    check(lib.dsvgp_abar(ctx.h, _ptr(A), _ld(A), _ptr(U), _ld(U), Mp, nc, _ptr(m), _ptr(mu_bar), _ptr(var_bar),
                         _ptr(out), _ld(out)), "dsvgp_abar")


def rowdot_accum(ctx, A, vec, out):
    Mp, nc = A.shape
    check(lib.dsvgp_rowdot(ctx.h, _ptr(A), _ld(A), Mp, nc, _ptr(vec), _ptr(out)), "dsvgp_rowdot")


def kl_terms(ctx, m, LS, num_data, kl_buf, d_m, d_LS):
    Mp = m.shape[0]
    check(lib.dsvgp_kl_terms(ctx.h, _ptr(m), _ptr(_req(LS, f32, "L_S", 2)), _ld(LS), Mp, float(num_data), _ptr(kl_buf),
                             _ptr(d_m), _ptr(d_LS), _ld(d_LS)), "dsvgp_kl_terms")


def kl_terms_scaled(ctx, m, LS, num_data, add_kl, hyp, global_rows, kl_buf, d_m, d_LS):
    """d_LS(lower) <- d_LS / (noise rows) [+ KL gradient], d_m [+= m / num_data], kl_buf[0] = KL or 0 -- noise read on the device"""
    Mp = m.shape[0]
    check(lib.dsvgp_kl_terms_scaled(ctx.h, _ptr(m), _ptr(_req(LS, f32, "L_S", 2)), _ld(LS), Mp, float(num_data),
                                    1 if add_kl else 0, _ptr(hyp), float(global_rows), _ptr(kl_buf), _ptr(d_m), _ptr(d_LS),
                                    _ld(d_LS)), "dsvgp_kl_terms_scaled")


def scale_by_vbar_(ctx, tensors, hyp, global_rows):
    """x *= 1 / (noise * global_rows) for up to three contiguous float32 tensors, noise read on the device"""
    ts = [t for t in tensors if t is not None and t.numel()]
    if len(ts) > 3:
        raise ValueError("at most three tensors")
    for t in ts:
        if t.dtype != f32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("scale_by_vbar: contiguous float32 GPU tensors only")
    args = []
    for k in range(3):
        if k < len(ts):
            args += [_ptr(ts[k]), ts[k].numel()]
        else:
            args += [C.c_void_p(0), 0]
    check(lib.dsvgp_scale_by_vbar(ctx.h, *args, _ptr(hyp), float(global_rows)), "dsvgp_scale_by_vbar")


def adam_step_multi_dev_(ctx, params, grads, exp_avgs, exp_avg_sqs, lr_step_dev, beta1, beta2, eps, guard=None):
    """``adam_step_multi_`` with (lr, step) read from the device float[2] ``lr_step_dev``; skipped while ``guard[0] != 0``"""
    import ctypes
    n = len(params)
    if n > ADAM_MAX_TENSORS:
        raise ValueError("at most %d tensors per launch" % ADAM_MAX_TENSORS)
    for group in (params, grads, exp_avgs, exp_avg_sqs):
        for t in group:
            if t.dtype != f32 or not t.is_cuda or not t.is_contiguous():
                raise ValueError("adam: tensors must be contiguous float32 GPU tensors")
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    sizes = (ctypes.c_int64 * n)(*[t.numel() for t in params])
    check(lib.dsvgp_adam_step_multi_dev(ctx.h, n, arr(params), arr(grads), arr(exp_avgs), arr(exp_avg_sqs), sizes,
                                        _ptr(_req(lr_step_dev, f32, "lr_step_dev", 1)), float(beta1), float(beta2), float(eps),
                                        _ptr(guard)), "dsvgp_adam_step_multi_dev")


def phi_symmetrize_(ctx, G):
    check(lib.dsvgp_phi_symmetrize(ctx.h, _ptr(G), G.shape[0], _ld(G)), "dsvgp_phi_symmetrize")


def gemv_f64(ctx, A, x, y, trans=False):
    """y = A x (trans False: A [M, N], x [N], y [M]) or y = A^T x (x [M], y [N]) in fp64"""
    _req(A, f64, "A", 2)
    M, N = A.shape
    _req(x, f64, "x", 1)
    _req(y, f64, "y", 1)
    if x.numel() != (M if trans else N) or y.numel() != (N if trans else M):
        raise ValueError("gemv_f64 shape mismatch")
    check(lib.dsvgp_gemv_f64(ctx.h, 1 if trans else 0, _ptr(A), _ld(A), M, N, _ptr(x), _ptr(y)), "dsvgp_gemv_f64")
    return y


def transpose_f64(ctx, src, dst):
    check(lib.dsvgp_transpose_f64(ctx.h, _ptr(src), _ld(src), src.shape[0], src.shape[1], _ptr(dst), _ld(dst)),
          "dsvgp_transpose_f64")


def residual_terms(ctx, mu, y, hyp, global_rows, mu_bar, sums):
    check(lib.dsvgp_residual_terms(ctx.h, _ptr(mu), _ptr(_req(y, f32, "y", 1)), mu.shape[0], _ptr(hyp),
                                   float(global_rows), _ptr(mu_bar), _ptr(sums)), "dsvgp_residual_terms")


def variational_terms(ctx, m, LS, num_data, scale, add_kl, hyp, global_rows, G, t1_scale, kl_buf, sums, d_m, d_LS):
    """trace terms + [scaling by 1 / (noise rows)] + [KL value and gradient] in one pass over (L_S, d_LS = tril(G L_S)); see dsvgp.h"""
    Mp = m.shape[0]
    if kl_buf.numel() < 1 + 2 * Mp:
        raise ValueError("kl_buf needs 1 + 2 M' floats")
    check(lib.dsvgp_variational_terms(ctx.h, _ptr(m), _ptr(_req(LS, f32, "L_S", 2)), _ld(LS), Mp, float(num_data),
                                      (1 if scale else 0) | (2 if add_kl else 0), _ptr(hyp), float(global_rows), _ptr(G), _ld(G),
                                      float(t1_scale), _ptr(kl_buf), _ptr(sums), _ptr(d_m), _ptr(d_LS), _ld(d_LS)),
          "dsvgp_variational_terms")


def trace_terms(ctx, LS, T1, G, n, sums, t1_scale=1.0):
    check(lib.dsvgp_trace_terms(ctx.h, _ptr(LS), _ld(LS), _ptr(T1), _ld(T1), _ptr(G), _ld(G), n, float(t1_scale),
                                _ptr(sums)), "dsvgp_trace_terms")


def elbo_fast_finalize(ctx, sums, hyp, npts, p, global_rows, scalars):
    check(lib.dsvgp_elbo_fast_finalize(ctx.h, _ptr(sums), _ptr(hyp), npts, p, float(global_rows), _ptr(scalars)),
          "dsvgp_elbo_fast_finalize")


def mirror_lower_f32_(ctx, G, n):
    check(lib.dsvgp_mirror_lower_f32(ctx.h, _ptr(_req(G, f32, "G", 2)), n, _ld(G)), "dsvgp_mirror_lower_f32")


def sminus_i_col_(ctx, A, n, m, hyp, rows):
    """A[n, n+1] -> [A[:, :n] - I | m * noise * rows] in place (one launch)"""
    if A.shape != (n, n + 1) or A.dtype != f32 or A.stride(1) != 1:
        raise ValueError("sminus_i_col_ wants a float32 [n, n + 1] view with unit column stride")
    check(lib.dsvgp_sminus_i_col(ctx.h, _ptr(A), n, int(A.stride(0)), _ptr(_req(m, f32, "m", 1)), _ptr(hyp), float(rows)),
          "dsvgp_sminus_i_col")


def add_diag_f32_(ctx, A, n, delta):
    check(lib.dsvgp_add_diag_f32(ctx.h, _ptr(_req(A, f32, "A", 2)), n, _ld(A), float(delta)), "dsvgp_add_diag_f32")


def transpose_f32(ctx, src, dst):
    check(lib.dsvgp_transpose_f32(ctx.h, _ptr(src), _ld(src), src.shape[0], src.shape[1], _ptr(dst), _ld(dst)),
          "dsvgp_transpose_f32")


def tril_packed_numel(n, nextra=0):
    return n * (n + 1) // 2 + nextra


def tril_pack_f32(ctx, src, extra, dst):
    """dst = [packed lower triangle of src[n, n] | extra]: the half-volume data-parallel all-reduce operand."""
    n = src.shape[0]
    _req(src, f32, "src", 2); _req(extra, f32, "extra", 1); _req(dst, f32, "dst", 1)
    if src.shape[1] < n or dst.numel() < tril_packed_numel(n, extra.numel()):
        raise ValueError("tril_pack shape mismatch")
    check(lib.dsvgp_tril_pack_f32(ctx.h, _ptr(src), _ld(src), n, _ptr(extra), extra.numel(), _ptr(dst)),
          "dsvgp_tril_pack_f32")


def tril_unpack_f32(ctx, src, dst, extra):
    n = dst.shape[0]
    _req(src, f32, "src", 1); _req(extra, f32, "extra", 1); _req(dst, f32, "dst", 2)
    if dst.shape[1] < n or src.numel() < tril_packed_numel(n, extra.numel()):
        raise ValueError("tril_unpack shape mismatch")
    check(lib.dsvgp_tril_unpack_f32(ctx.h, _ptr(src), n, _ptr(dst), _ld(dst), _ptr(extra), extra.numel()),
          "dsvgp_tril_unpack_f32")


def gather_batch(ctx, X, Y, idx, cols, p, xb, yb, E=None, Db=None):
    """minibatch rows of X, the selected columns of Y and (with the [d, d] direction table E) the batch's derivative
    directions Db[nb * p, d] in one launch"""
    if E is not None and (E.shape != (X.shape[1], X.shape[1]) or not E.is_contiguous() or E.dtype != f32 or Db is None or
                          Db.shape != (idx.shape[0] * p, X.shape[1]) or not Db.is_contiguous() or Db.dtype != f32):
        raise ValueError("gather_batch: E must be [d, d] and Db [nb * p, d] float32 contiguous")
    check(lib.dsvgp_gather_batch(ctx.h, _ptr(_req(X, f32, "X", 2)), _ptr(_req(Y, f32, "Y", 2)),
                                 _ptr(_req(idx, torch.int64, "idx", 1)), idx.shape[0], X.shape[1], Y.shape[1],
                                 _ptr(_req(cols, torch.int32, "cols", 1)), p, _ptr(xb), _ptr(yb), _ptr(E), _ptr(Db)),
          "dsvgp_gather_batch")


def gather_batch_f64(ctx, X, Y, idx, cols, p, xb, yb, E=None, Db=None):
    """``gather_batch`` of the float64 model mode: minibatch rows of X, the selected (interleaved) columns of Y and, with the [d, d]
    direction table E, the tiled one-hot directions Db[nb * p, d] in one launch"""
    if E is not None and (E.shape != (X.shape[1], X.shape[1]) or not E.is_contiguous() or E.dtype != f64 or Db is None or
                          Db.shape != (idx.shape[0] * p, X.shape[1]) or not Db.is_contiguous() or Db.dtype != f64):
        raise ValueError("gather_batch_f64: E must be [d, d] and Db [nb * p, d] float64 contiguous")
    if not (X.is_contiguous() and Y.is_contiguous()):
        raise ValueError("gather_batch_f64: X and Y must be contiguous")
    if xb.shape != (idx.shape[0], X.shape[1]) or yb.numel() != idx.shape[0] * (p + 1) or cols.numel() != p + 1:
        raise ValueError("gather_batch_f64: output shapes do not match the index lists")
    check(lib.dsvgp_gather_batch_f64(ctx.h, _ptr(_req(X, f64, "X", 2)), _ptr(_req(Y, f64, "Y", 2)),
                                     _ptr(_req(idx, torch.int64, "idx", 1)), idx.shape[0], X.shape[1], Y.shape[1],
                                     _ptr(_req(cols, torch.int32, "cols", 1)), p, _ptr(_req(xb, f64, "xb", 2)), _ptr(_req(yb, f64, "yb", 1)),
                                     _ptr(E), _ptr(Db)), "dsvgp_gather_batch_f64")


ADAM_MAX_TENSORS = 16


def adam_step_multi_(ctx, params, grads, exp_avgs, exp_avg_sqs, lr, beta1, beta2, eps, step, tril=None, guard=None):
    """torch.optim.Adam update of several tensors that share (lr, betas, eps, step) in one launch.  ``tril[k]`` true: params[k] is a square
    matrix of which only the lower triangle is a parameter (its gradient and moments are zero above the diagonal): the strict upper
    triangle is left alone (float32 only)."""
    import ctypes
    n = len(params)
    if n > ADAM_MAX_TENSORS:
        raise ValueError("at most %d tensors per launch" % ADAM_MAX_TENSORS)
    dt = params[0].dtype if n else f32
    for group in (params, grads, exp_avgs, exp_avg_sqs):
        for t in group:
            if t.dtype != dt or dt not in (f32, f64) or not t.is_cuda or not t.is_contiguous():
                raise ValueError("adam: tensors must be contiguous GPU tensors of one dtype (float32 or float64)")
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    sz = [t.numel() for t in params]
    if tril is not None and dt == f32:
        sz = [-t.shape[0] if (tr and t.dim() == 2 and t.shape[0] == t.shape[1] and t.shape[0] > 1) else k for t, k, tr in zip(params, sz, tril)]
    sizes = (ctypes.c_int64 * n)(*sz)
    if guard is not None:       # (``guard``: int32 device tensor, the update is skipped on the device while guard[0] != 0; float32 only)
        if dt != f32 or guard.dtype != torch.int32 or not guard.is_cuda:
            raise ValueError("adam: a guarded update takes float32 tensors and an int32 GPU guard word")
        check(lib.dsvgp_adam_step_multi_guarded(ctx.h, n, arr(params), arr(grads), arr(exp_avgs), arr(exp_avg_sqs), sizes, float(lr), float(beta1),
                                                float(beta2), float(eps), int(step), _ptr(guard)), "dsvgp_adam_step_multi_guarded")
        return
    fn, name = (lib.dsvgp_adam_step_multi_f64, "dsvgp_adam_step_multi_f64") if dt == f64 else (lib.dsvgp_adam_step_multi, "dsvgp_adam_step_multi")
    check(fn(ctx.h, n, arr(params), arr(grads), arr(exp_avgs), arr(exp_avg_sqs), sizes, float(lr), float(beta1), float(beta2),
             float(eps), int(step)), name)


def adam_step_(ctx, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step):
    for t, nm in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        if not t.is_contiguous() or t.dtype != f32 or not t.is_cuda:
            raise ValueError("adam: %s must be a contiguous float32 GPU tensor" % nm)
    check(lib.dsvgp_adam_step(ctx.h, _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(),
                              float(lr), float(beta1), float(beta2), float(eps), int(step)), "dsvgp_adam_step")


def gemm_lib_f32(ctx, flags, A, B, C_out, alpha=1.0, beta=0.0):
    """C_out = alpha op(A) op(B) + beta C_out, plain dense fp32, through rocBLAS (no structure flags)."""
    _req(A, f32, "A", 2); _req(B, f32, "B", 2); _req(C_out, f32, "C", 2)
    M = A.shape[1] if flags & _lib.TRANS_A else A.shape[0]
    K = A.shape[0] if flags & _lib.TRANS_A else A.shape[1]
    N = B.shape[0] if flags & _lib.TRANS_B else B.shape[1]
    kb = B.shape[1] if flags & _lib.TRANS_B else B.shape[0]
    if kb != K or C_out.shape != (M, N):
        raise ValueError("gemm_lib_f32 shape mismatch")
    check(lib.dsvgp_gemm_lib_f32(ctx.h, int(flags), M, N, K, float(alpha), _ptr(A), _ld(A), _ptr(B), _ld(B), float(beta),
                                 _ptr(C_out), _ld(C_out)), "dsvgp_gemm_lib_f32")


# ---- contour-integral-quadrature whitening (csrc/ciq.hip) ------------------------------------------------------
# Every wrapper serves both scalar types: float32 tensors go to dsvgp_ciq_*, float64 tensors (the fp64 model mode) to
# dsvgp_ciq_*_f64; all tensors of one call must share the type of its first matrix argument.
def _ciq_fn(name, dt):
    if dt == f32:
        return getattr(lib, name)
    if dt == f64:
        return getattr(lib, (name[:-4] if name.endswith("_f32") else name) + "_f64")
    raise TypeError("CIQ kernels are built for float32 and float64 tensors, got %s" % dt)


def ciq_workspace_bytes(Q, t, n, cap, dtype=f32):
    return int(_ciq_fn("dsvgp_ciq_workspace_bytes", dtype)(int(Q), int(t), int(n), int(cap)))


def ciq_lanczos(ctx, K, v0, iters):
    """alpha[iters], beta[iters] of `iters` Lanczos steps with the symmetric K started at v0."""
    dt = K.dtype
    _req(K, dt, "K", 2)
    n = K.shape[0]
    alpha = torch.zeros(iters, dtype=dt, device=K.device)
    beta = torch.zeros(iters, dtype=dt, device=K.device)
    ws = torch.empty(3 * n + 8, dtype=dt, device=K.device)
    check(_ciq_fn("dsvgp_ciq_lanczos", dt)(ctx.h, _ptr(K), _ld(K), _ptr(_req(v0, dt, "v0", 1)), n, int(iters), _ptr(alpha),
                                          _ptr(beta), _ptr(ws)), "dsvgp_ciq_lanczos")
    return alpha, beta


def ciq_qp(Q):
    """Shift / output counts of the CIQ coefficient tables are padded to multiples of 4 (csrc/ciq.hip)."""
    return 4 * ((int(Q) + 3) // 4)


def ciq_solve(ctx, K, R, sigma, omega, basis, ycoef, rnorm, out, workspace, tol=1e-4, max_iter=1000, check_every=10):
    """out[t,n] = sum_q omega_q (K + sigma_q)^-1 R rows by basis-resident msMINRES: basis[cap+1,t,n] receives the Lanczos
    rows, ycoef[t,cap,QP] the per-shift coefficients (x_q = rnorm * mix(basis, ycoef)), rnorm[t] the row norms of R.
    Returns the iteration count, or None when `cap` iterations were not enough (call again with a larger basis)."""
    dt = K.dtype
    _req(K, dt, "K", 2)
    _req(R, dt, "R", 2)
    t, n = R.shape
    Q = sigma.shape[0]
    cap = basis.shape[0] - 1
    if (K.shape != (n, n) or basis.shape != (cap + 1, t, n) or cap < 1 or ycoef.shape != (t, cap, ciq_qp(Q)) or
            rnorm.shape != (t,) or out.shape != (t, n) or not basis.is_contiguous() or not ycoef.is_contiguous()):
        raise ValueError("ciq_solve shape mismatch")
    for a, name in ((basis, "basis"), (ycoef, "ycoef"), (rnorm, "rnorm"), (out, "out")):
        if a.dtype != dt or not a.is_cuda:
            raise TypeError("%s must be a %s GPU tensor" % (name, dt))
    need = ciq_workspace_bytes(Q, t, n, cap, dt)
    if workspace.numel() * workspace.element_size() < need:
        raise ValueError("ciq workspace too small")
    its = C.c_int(0)
    rc = _ciq_fn("dsvgp_ciq_solve", dt)(ctx.h, _ptr(K), _ld(K), _ptr(R), _ld(R), t, n, _ptr(_req(sigma, dt, "sigma", 1)),
                                        _ptr(_req(omega, dt, "omega", 1)), Q, float(tol), int(max_iter), int(check_every),
                                        _ptr(basis), cap, _ptr(ycoef), _ptr(rnorm), _ptr(out), _ld(out), _ptr(workspace),
                                        C.byref(its))
    if rc == _lib.ENOSPACE:
        return None
    check(rc, "dsvgp_ciq_solve")
    return its.value


def ciq_mix(ctx, basis, J, coef, Kout, rowscale, out):
    """out[k,row,:] = rowscale[row] * sum_{j<J} coef[row,j,k] basis[j,row,:] for k < Kout (coef[t,ldj,KP], KP % 4 == 0)."""
    _, t, n = basis.shape
    ldj, KP = coef.shape[1], coef.shape[2]
    dt = basis.dtype
    if (coef.shape[0] != t or J > ldj or J > basis.shape[0] or out.shape != (Kout, t, n) or not out.is_contiguous() or
            not coef.is_contiguous() or not basis.is_contiguous() or coef.dtype != dt or out.dtype != dt or
            (rowscale is not None and rowscale.dtype != dt)):
        raise ValueError("ciq_mix shape mismatch")
    check(_ciq_fn("dsvgp_ciq_mix", dt)(ctx.h, _ptr(basis), int(J), t, n, _ptr(coef), ldj, KP, int(Kout), _ptr(rowscale), _ptr(out),
                                      n), "dsvgp_ciq_mix")
    return out


def ciq_cross(ctx, ya, Ja, yb, Jb, omega, rn_a, rn_b):
    """C[t,Jb,KPa] = rn_a rn_b sum_q omega_q ya[:,ia,q] yb[:,jb,q]: coefficients that turn sum_q omega_q A_q^T B_q into
    stack(basisA[:Ja])^T stack(mix(basisB, C)) (A_q = rn_a mix(basisA, ya)_q, B_q likewise)."""
    t = ya.shape[0]
    Q = omega.shape[0]
    dt = ya.dtype
    if yb.shape[0] != t or ya.shape[2] != ciq_qp(Q) or yb.shape[2] != ciq_qp(Q) or Ja > ya.shape[1] or Jb > yb.shape[1]:
        raise ValueError("ciq_cross shape mismatch")
    if any(a.dtype != dt for a in (yb, omega, rn_a, rn_b)):
        raise TypeError("ciq_cross: every tensor must be %s" % dt)
    out = torch.empty(t, Jb, ciq_qp(Ja), dtype=dt, device=ya.device)
    check(_ciq_fn("dsvgp_ciq_cross", dt)(ctx.h, _ptr(ya), int(Ja), ya.shape[1], _ptr(yb), int(Jb), yb.shape[1], _ptr(omega), Q, t,
                                        _ptr(rn_a), _ptr(rn_b), _ptr(out)), "dsvgp_ciq_cross")
    return out


def ciq_rowstats(ctx, T, ST, p, m, constant, hyp, kxx_jitter=0.0):
    t, n = T.shape
    dev = T.device
    dt = T.dtype
    if any(a.dtype != dt for a in (ST, m, constant, hyp)):
        raise TypeError("ciq_rowstats: every tensor must be %s" % dt)
    imean, mu, var, live = (torch.empty(t, dtype=dt, device=dev) for _ in range(4))
    check(_ciq_fn("dsvgp_ciq_rowstats", dt)(ctx.h, _ptr(T), _ptr(ST), t, n, p, _ptr(m), _ptr(constant), _ptr(hyp), float(kxx_jitter),
                                           _ptr(imean), _ptr(mu), _ptr(var), _ptr(live)), "dsvgp_ciq_rowstats")
    return imean, mu, var, live


def ciq_tbar(ctx, T, ST, m, mu_bar, var_bar, live, imean, Tbar, VT):
    t, n = T.shape
    dt = T.dtype
    if any(a.dtype != dt for a in (ST, m, mu_bar, var_bar, live, imean, Tbar, VT)):
        raise TypeError("ciq_tbar: every tensor must be %s" % dt)
    cvec = torch.empty(t, dtype=dt, device=T.device)
    check(_ciq_fn("dsvgp_ciq_tbar", dt)(ctx.h, _ptr(T), _ptr(ST), t, n, _ptr(m), _ptr(mu_bar), _ptr(var_bar), _ptr(live),
                                       _ptr(imean), _ptr(Tbar), _ptr(VT), _ptr(cvec)), "dsvgp_ciq_tbar")
    return cvec


def sym_average_f32(ctx, A, out):
    check(lib.dsvgp_sym_average_f32(ctx.h, _ptr(_req(A, f32, "A", 2)), A.shape[0], _ld(A), _ptr(out), _ld(out)),
          "dsvgp_sym_average_f32")


def sym_average_f64(ctx, A, out):
    check(lib.dsvgp_sym_average_f64(ctx.h, _ptr(_req(A, f64, "A", 2)), A.shape[0], _ld(A), _ptr(_req(out, f64, "out", 2)),
                                    _ld(out)), "dsvgp_sym_average_f64")


def mfma_rate(ctx, is_double=True, millis=40):
    """TFLOP/s this card sustains on back-to-back MFMA instructions from registers (fp64 16x16x4 or fp32 32x32x2): the roof a
    GEMM kernel can reach under the card's power management.  Measurement aid for bench.py."""
    scratch = torch.empty(2 << 20, dtype=torch.uint8, device=ctx.device)
    out = C.c_double(0.0)
    check(lib.dsvgp_mfma_rate(ctx.h, 1 if is_double else 0, int(millis), _ptr(scratch), C.byref(out)), "dsvgp_mfma_rate")
    return out.value


def mfma_rate2(ctx, is_double=True, one_wave_per_simd=False, millis=40):
    """(sustained TFLOP/s, TFLOP/s of the first ~2 ms launch, in-kernel clock in GHz of the last launch) of the same probe with four
    waves per SIMD or one (the form the hardware guide's 155 TF fp32 figure was measured in)."""
    scratch = torch.empty(2 << 20, dtype=torch.uint8, device=ctx.device)
    out, burst, clk = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    check(lib.dsvgp_mfma_rate2(ctx.h, (1 if is_double else 0) | (2 if one_wave_per_simd else 0), int(millis), _ptr(scratch),
                               C.byref(out), C.byref(burst), C.byref(clk)), "dsvgp_mfma_rate2")
    return out.value, burst.value, clk.value


# ---- data-driven initialisation (csrc/kmeans.hip) ---------------------------------------------------------------------------------
i32 = torch.int32


def kmeans_workspace_bytes(N, d, M):
    return int(lib.dsvgp_kmeans_workspace_bytes(int(N), int(d), int(M)))


def _kmeans_xz(x, Z):
    _req(x, f32, "x", 2)
    _req(Z, f32, "Z", 2)
    if not x.is_contiguous() or not Z.is_contiguous() or Z.shape[1] != x.shape[1]:
        raise ValueError("x [N, d] and Z [M, d] must be contiguous with one d, got %s and %s" % (tuple(x.shape), tuple(Z.shape)))
    N, d = x.shape
    M = Z.shape[0]
    if N < 1 or d < 1 or M < 1 or M > N:
        raise ValueError("k-means needs 1 <= M <= N and d >= 1, got N = %d, d = %d, M = %d" % (N, d, M))
    return N, d, M


def _kmeans_ws(N, d, M, workspace, device):
    need = kmeans_workspace_bytes(N, d, M)
    if d > 32 and need == 0:
        raise ValueError("k-means at N = %d, d = %d, M = %d: an intermediate would pass 2^31 entries" % (N, d, M))
    if need and workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
    if need and workspace.numel() * workspace.element_size() < need:
        raise ValueError("k-means workspace too small: %d bytes needed" % need)
    return workspace if need else None


def _kmeans_out(t, dtype, n, name, device):
    if t is None:
        return torch.empty(n, dtype=dtype, device=device)
    _req(t, dtype, name, 1)
    if t.numel() != n:
        raise ValueError("%s must have %d entries, got %d" % (name, n, t.numel()))
    return t


def kmeans_assign(ctx, x, Z, labels=None, dist2=None, workspace=None):
    """(labels int32 [N], dist2 float32 [N]): the nearest centroid of every point and the squared distance to it (dsvgp_kmeans_assign;
    an exact tie goes to the lowest index).  ``workspace``: uint8 tensor of dsvgp_kmeans_workspace_bytes bytes (allocated when None)."""
    N, d, M = _kmeans_xz(x, Z)
    labels = _kmeans_out(labels, i32, N, "labels", x.device)
    dist2 = _kmeans_out(dist2, f32, N, "dist2", x.device)
    workspace = _kmeans_ws(N, d, M, workspace, x.device)
    check(lib.dsvgp_kmeans_assign(ctx.h, _ptr(x), N, d, _ptr(Z), M, _ptr(labels), _ptr(dist2), _ptr(workspace)), "dsvgp_kmeans_assign")
    return labels, dist2


def kmeans_update_(ctx, x, labels, Z, counts=None):
    """Z[m] <- mean of the rows of x labelled m, in place (an empty cluster keeps its row); returns counts int32 [M] (dsvgp_kmeans_update)"""
    N, d, M = _kmeans_xz(x, Z)
    _req(labels, i32, "labels", 1)
    if labels.numel() != N:
        raise ValueError("labels must have N = %d entries" % N)
    counts = _kmeans_out(counts, i32, M, "counts", x.device)
    check(lib.dsvgp_kmeans_update(ctx.h, _ptr(x), N, d, _ptr(labels), _ptr(Z), M, _ptr(counts)), "dsvgp_kmeans_update")
    return counts


def kmeans_lloyd_(ctx, x, Z, iterations, labels=None, dist2=None, counts=None, inertia=None, moved=None, workspace=None):
    """``iterations`` Lloyd steps on Z in place and a closing assignment (dsvgp_kmeans_lloyd): returns (labels, dist2, counts, inertia
    float64 [iterations + 1], moved int32 [iterations]) -- no host read; the caller looks at ``moved`` afterwards if it wants to"""
    N, d, M = _kmeans_xz(x, Z)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("iterations must be >= 0, got %d" % iterations)
    labels = _kmeans_out(labels, i32, N, "labels", x.device)
    dist2 = _kmeans_out(dist2, f32, N, "dist2", x.device)
    counts = _kmeans_out(counts, i32, M, "counts", x.device)
    inertia = _kmeans_out(inertia, f64, iterations + 1, "inertia", x.device)
    moved = _kmeans_out(moved, i32, iterations, "moved", x.device)
    workspace = _kmeans_ws(N, d, M, workspace, x.device)
    check(lib.dsvgp_kmeans_lloyd(ctx.h, _ptr(x), N, d, _ptr(Z), M, iterations, _ptr(labels), _ptr(dist2), _ptr(counts), _ptr(inertia),
                                 _ptr(moved if iterations else None), _ptr(workspace)), "dsvgp_kmeans_lloyd")
    return labels, dist2, counts, inertia, moved


def cluster_moments(ctx, g, labels, M, out=None):
    """C[M, d, d] float64 = sum over the rows of g labelled m of g_i g_i^T (dsvgp_cluster_moments; d <= 128), exactly symmetric"""
    _req(g, f32, "g", 2)
    _req(labels, i32, "labels", 1)
    N, d = g.shape
    M = int(M)
    if not g.is_contiguous() or labels.numel() != N:
        raise ValueError("g must be a contiguous [N, d] tensor with one label per row")
    if N < 1 or M < 1 or M > N or not 1 <= d <= 128:
        raise ValueError("cluster moments need 1 <= M <= N and 1 <= d <= 128, got N = %d, d = %d, M = %d" % (N, d, M))
    if out is None:
        out = torch.empty(M, d, d, dtype=f64, device=g.device)
    _req(out, f64, "out", 3)
    if out.shape != (M, d, d):
        raise ValueError("out must be [%d, %d, %d]" % (M, d, d))
    check(lib.dsvgp_cluster_moments(ctx.h, _ptr(g), N, d, _ptr(labels), M, _ptr(out), None), "dsvgp_cluster_moments")
    return out


# ---- closed-form optimal q(u) from one-pass statistics (csrc/collapsed.hip) ---------------------------------------------------
COLLAPSED_MAX_MP = 8192


def collapsed_state(Mp, device):
    """zeroed statistics of ``collapsed_accumulate``: float64 [8 + (M' + 1)^2] -- sum of the prior diagonal, R, six reserved words, then
    tril([A ; r^T][A ; r^T]^T) row-major (rows < M': tril G; row M': b^T, then yy)"""
    Mp = int(Mp)
    if Mp < 1:
        raise ValueError("collapsed statistics need M' >= 1, got %d" % Mp)
    return torch.zeros(int(lib.dsvgp_collapsed_state_bytes(Mp)) // 8, dtype=f64, device=device)


def _req_collapsed_state(state, Mp):
    _req(state, f64, "state", 1)
    if state.numel() * 8 != int(lib.dsvgp_collapsed_state_bytes(int(Mp))):
        raise ValueError("state is not the collapsed statistics of M' = %d (collapsed_state)" % Mp)
    return state


def collapsed_workspace(Mp, device):
    nbytes = int(lib.dsvgp_collapsed_workspace_bytes(int(Mp)))
    if nbytes == 0:
        raise ValueError("collapsed solve / evaluate take 1 <= M' <= %d, got %d" % (COLLAPSED_MAX_MP, Mp))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def collapsed_reset_(ctx, state, Mp):
    check(lib.dsvgp_collapsed_reset(ctx.h, _ptr(_req_collapsed_state(state, Mp)), int(Mp)), "dsvgp_collapsed_reset")


def collapsed_accumulate_(ctx, state, Mp, A64, Bp, y, constant, prior_diag):
    """state += statistics of one chunk.  A64 [M' + 1, >= Bp] float64: rows < M' hold A = L^-1 K_ZX (``trsm``'s X64); row M' is written here
    (r = y - constant).  y, prior_diag: float32 [Bp]; constant: float32 [1]"""
    _req_collapsed_state(state, Mp)
    _req(A64, f64, "A64", 2)
    if A64.shape[0] != Mp + 1 or A64.shape[1] < Bp:
        raise ValueError("A64 must be [M' + 1, >= B'] = [%d, >= %d], got %s" % (Mp + 1, Bp, tuple(A64.shape)))
    for t, name in ((y, "y"), (prior_diag, "prior_diag")):
        _req(t, f32, name, 1)
        if t.numel() != Bp:
            raise ValueError("%s must have B' = %d entries, got %d" % (name, Bp, t.numel()))
    _req(constant, f32, "constant", 1)
    check(lib.dsvgp_collapsed_accumulate(ctx.h, _ptr(state), int(Mp), _ptr(A64), _ld(A64), int(Bp), _ptr(y), _ptr(constant),
                                         _ptr(prior_diag)), "dsvgp_collapsed_accumulate")


def collapsed_accumulate_masked_(ctx, state, Mp, A64, Bp, pd, y, constant, prior_diag):
    """``collapsed_accumulate_`` over the rows whose target is not NaN (csrc/missing.hip): the missing columns of A64 are zeroed, r = 0
    there, and the prior-diagonal sum, R (state[1]) and the count of present value rows (state[2]) take present rows only"""
    _req_collapsed_state(state, Mp)
    _req(A64, f64, "A64", 2)
    if A64.shape[0] != Mp + 1 or A64.shape[1] < Bp:
        raise ValueError("A64 must be [M' + 1, >= B'] = [%d, >= %d], got %s" % (Mp + 1, Bp, tuple(A64.shape)))
    for t, name in ((y, "y"), (prior_diag, "prior_diag")):
        _req(t, f32, name, 1)
        if t.numel() != Bp:
            raise ValueError("%s must have B' = %d entries, got %d" % (name, Bp, t.numel()))
    _req(constant, f32, "constant", 1)
    check(lib.dsvgp_collapsed_accumulate_masked(ctx.h, _ptr(state), int(Mp), _ptr(A64), _ld(A64), int(Bp), int(pd), _ptr(y),
                                                _ptr(constant), _ptr(prior_diag)), "dsvgp_collapsed_accumulate_masked")


def collapsed_accumulate_classes_(ctx, state, Mp, A64, Bp, pd, y, constant, prior_diag, hyp):
    """``collapsed_accumulate_`` with row weights 1 on value rows and rho = hyp[2] / hyp[3] on derivative rows (csrc/noise_classes.hip): the
    derivative columns of A64 and of r are scaled by sqrt(rho) in place; state[2] counts the value rows"""
    _req_collapsed_state(state, Mp)
    _req(A64, f64, "A64", 2)
    if A64.shape[0] != Mp + 1 or A64.shape[1] < Bp:
        raise ValueError("A64 must be [M' + 1, >= B'] = [%d, >= %d], got %s" % (Mp + 1, Bp, tuple(A64.shape)))
    for t, name in ((y, "y"), (prior_diag, "prior_diag")):
        _req(t, f32, name, 1)
        if t.numel() != Bp:
            raise ValueError("%s must have B' = %d entries, got %d" % (name, Bp, t.numel()))
    _req(constant, f32, "constant", 1)
    _req(hyp, f32, "hyp", 1)
    if hyp.numel() < 4:
        raise ValueError("hyp must have 4 entries, got %d" % hyp.numel())
    check(lib.dsvgp_collapsed_accumulate_classes(ctx.h, _ptr(state), int(Mp), _ptr(A64), _ld(A64), int(Bp), int(pd), _ptr(y),
                                                 _ptr(constant), _ptr(prior_diag), _ptr(hyp)), "dsvgp_collapsed_accumulate_classes")


def collapsed_solve(ctx, state, Mp, hyp, num_data, workspace, want_natural=True):
    """(m*, L_S*, natural_vec, natural_mat, scalars[8] float64, info int32[1]) -- all on the device, nothing read"""
    _req_collapsed_state(state, Mp)
    dev = state.device
    m = torch.empty(Mp, dtype=f32, device=dev)
    LS = torch.empty(Mp, Mp, dtype=f32, device=dev)
    nv = torch.empty(Mp, dtype=f32, device=dev) if want_natural else None
    nm = torch.empty(Mp, Mp, dtype=f32, device=dev) if want_natural else None
    scal = torch.empty(8, dtype=f64, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib.dsvgp_collapsed_solve(ctx.h, _ptr(state), int(Mp), _ptr(hyp), float(num_data), _ptr(m), _ptr(LS), Mp, _ptr(nv), _ptr(nm), Mp,
                                    _ptr(scal), _ptr(info), _ptr(workspace)), "dsvgp_collapsed_solve")
    return m, LS, nv, nm, scal, info


def collapsed_evaluate(ctx, state, Mp, m, LS, hyp, num_data, workspace):
    """scalars[8] float64 (loss, sum ll, KL, sum |residual|^2, sum varn, R, kappa, tr G) of the caller's float32 (m, tril L_S)"""
    _req_collapsed_state(state, Mp)
    _req(m, f32, "variational_mean", 1)
    _req(LS, f32, "chol_variational_covar", 2)
    if m.numel() != Mp or LS.shape != (Mp, Mp):
        raise ValueError("variational_mean / chol_variational_covar must be [%d] / [%d, %d]" % (Mp, Mp, Mp))
    scal = torch.empty(8, dtype=f64, device=state.device)
    check(lib.dsvgp_collapsed_evaluate(ctx.h, _ptr(state), int(Mp), _ptr(m), _ptr(LS), _ld(LS), _ptr(hyp), float(num_data), _ptr(scal),
                                       _ptr(workspace)), "dsvgp_collapsed_evaluate")
    return scal


# ---- gradients of the collapsed bound at the optimum (csrc/collapsed.hip) --------------------------------
COLLAPSED_ADJOINTS = ("w", "d_noise", "d_diag", "loss", "residual", "varn", "kappa", "rows")


def collapsed_grad_workspace_bytes(Mp):
    """bytes of ``collapsed_grad_prepare``'s workspace (pure host arithmetic); 0 for an M' it does not take"""
    return int(lib.dsvgp_collapsed_grad_workspace_bytes(int(Mp)))


def collapsed_grad_chunk_bytes(Mp, Bp):
    """bytes of ``collapsed_grad_chunk``'s workspace (pure host arithmetic); 0 for refused arguments"""
    return int(lib.dsvgp_collapsed_grad_chunk_bytes(int(Mp), int(Bp)))


def collapsed_grad_prepare(ctx, state, Mp, m, LS, inverse, hyp, num_data, workspace=None):
    """(alpha [M'], Q [M', M'], K~-bar [M', M'], adj [8] float64, info int32[1]) of the optimum (m, LS) that ``collapsed_solve`` returned
    for the same statistics, hyp and num_data; ``inverse``: L^-1 | L^-T (2 M'^2 doubles, as bytes or float64).  Nothing is read."""
    _req_collapsed_state(state, Mp)
    _req(m, f32, "variational_mean", 1)
    _req(LS, f32, "chol_variational_covar", 2)
    if m.numel() != Mp or LS.shape != (Mp, Mp):
        raise ValueError("variational_mean / chol_variational_covar must be [%d] / [%d, %d]" % (Mp, Mp, Mp))
    if inverse.numel() * inverse.element_size() < 16 * Mp * Mp:
        raise ValueError("inverse must hold L^-1 | L^-T: 2 M'^2 = %d doubles" % (2 * Mp * Mp))
    nbytes = collapsed_grad_workspace_bytes(Mp)
    if nbytes == 0:
        raise ValueError("the collapsed gradients take 1 <= M' <= %d, got %d" % (COLLAPSED_MAX_MP, Mp))
    dev = state.device
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    alpha = torch.empty(Mp, dtype=f64, device=dev)
    ldq = (Mp + 1) & ~1                    # an even leading dimension: the per-chunk product reads Q 16 bytes at a time also at odd M'
    Q = torch.empty(Mp, ldq, dtype=f64, device=dev)[:, :Mp]
    Kb = torch.empty(Mp, Mp, dtype=f64, device=dev)
    adj = torch.empty(8, dtype=f64, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib.dsvgp_collapsed_grad_prepare(ctx.h, _ptr(state), int(Mp), _ptr(m), _ptr(LS), _ld(LS), _ptr(inverse), _ptr(hyp),
                                           float(num_data), _ptr(alpha), _ptr(Q), ldq, _ptr(Kb), Mp, _ptr(adj), _ptr(info),
                                           _ptr(workspace)), "dsvgp_collapsed_grad_prepare")
    return alpha, Q, Kb, adj, info


def collapsed_grad_chunk(ctx, Mp, Kzx, y, constant, Q, alpha, adj, K_bar, diag_bar, rho_sum, workspace):
    """K_bar [M', B'] (float32) = 2 w (Q Kzx - alpha rho^T) of one chunk, diag_bar [B'] (or None) = dg-bar, rho_sum[0] += sum rho.  Every
    buffer is the caller's: no allocation, no host read"""
    _req(Kzx, f32, "Kzx", 2)
    _req(K_bar, f32, "K_bar", 2)
    Bp = Kzx.shape[1]
    if Kzx.shape[0] != Mp or K_bar.shape != Kzx.shape:
        raise ValueError("Kzx and K_bar must both be [M', B'] = [%d, B'], got %s and %s" % (Mp, tuple(Kzx.shape), tuple(K_bar.shape)))
    _req(y, f32, "y", 1)
    if y.numel() != Bp or (diag_bar is not None and (diag_bar.numel() != Bp or diag_bar.dtype != f32)):
        raise ValueError("y and diag_bar must have B' = %d float32 entries" % Bp)
    _req(constant, f32, "constant", 1)
    _req(Q, f64, "Q", 2)
    if Q.shape != (Mp, Mp):
        raise ValueError("Q must be [M', M'] = [%d, %d], got %s" % (Mp, Mp, tuple(Q.shape)))
    for t, name, numel in ((alpha, "alpha", Mp), (adj, "adj", 8), (rho_sum, "rho_sum", 1)):
        if t.dtype != f64 or t.numel() != numel or not t.is_contiguous():
            raise ValueError("%s must be %d contiguous float64 values" % (name, numel))
    nbytes = collapsed_grad_chunk_bytes(Mp, Bp)
    if nbytes == 0 or workspace is None or workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError("collapsed_grad_chunk needs a workspace of collapsed_grad_chunk_bytes(M', B') = %d bytes" % nbytes)
    check(lib.dsvgp_collapsed_grad_chunk(ctx.h, int(Mp), int(Bp), _ptr(Kzx), _ld(Kzx), _ptr(y), _ptr(constant), _ptr(Q), _ld(Q), _ptr(alpha),
                                         _ptr(adj), _ptr(K_bar), _ld(K_bar), _ptr(diag_bar), _ptr(rho_sum), _ptr(workspace)),
          "dsvgp_collapsed_grad_chunk")


def collapsed_grad_chunk_masked_bytes(Mp, Bp):
    """bytes of ``collapsed_grad_chunk_masked``'s workspace (pure host arithmetic); 0 for refused arguments"""
    return int(lib.dsvgp_collapsed_grad_chunk_masked_bytes(int(Mp), int(Bp)))


def collapsed_grad_chunk_masked(ctx, Mp, Kzx, y, constant, Q, alpha, adj, K_bar, diag_bar, rho_sum, workspace):
    """``collapsed_grad_chunk`` with K_bar's columns, diag_bar and the share of rho_sum exactly 0 on the rows whose target is NaN
    (csrc/missing.hip).  The missing columns of ``Kzx`` are zeroed in place."""
    _req(Kzx, f32, "Kzx", 2)
    _req(K_bar, f32, "K_bar", 2)
    Bp = Kzx.shape[1]
    if Kzx.shape[0] != Mp or K_bar.shape != Kzx.shape:
        raise ValueError("Kzx and K_bar must both be [M', B'] = [%d, B'], got %s and %s" % (Mp, tuple(Kzx.shape), tuple(K_bar.shape)))
    _req(y, f32, "y", 1)
    if y.numel() != Bp or (diag_bar is not None and (diag_bar.numel() != Bp or diag_bar.dtype != f32)):
        raise ValueError("y and diag_bar must have B' = %d float32 entries" % Bp)
    _req(constant, f32, "constant", 1)
    _req(Q, f64, "Q", 2)
    if Q.shape != (Mp, Mp):
        raise ValueError("Q must be [M', M'] = [%d, %d], got %s" % (Mp, Mp, tuple(Q.shape)))
    for t, name, numel in ((alpha, "alpha", Mp), (adj, "adj", 8), (rho_sum, "rho_sum", 1)):
        if t.dtype != f64 or t.numel() != numel or not t.is_contiguous():
            raise ValueError("%s must be %d contiguous float64 values" % (name, numel))
    nbytes = collapsed_grad_chunk_masked_bytes(Mp, Bp)
    if nbytes == 0 or workspace is None or workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError("collapsed_grad_chunk_masked needs a workspace of collapsed_grad_chunk_masked_bytes(M', B') = %d bytes" % nbytes)
    check(lib.dsvgp_collapsed_grad_chunk_masked(ctx.h, int(Mp), int(Bp), _ptr(Kzx), _ld(Kzx), _ptr(y), _ptr(constant), _ptr(Q), _ld(Q),
                                                _ptr(alpha), _ptr(adj), _ptr(K_bar), _ld(K_bar), _ptr(diag_bar), _ptr(rho_sum),
                                                _ptr(workspace)), "dsvgp_collapsed_grad_chunk_masked")
