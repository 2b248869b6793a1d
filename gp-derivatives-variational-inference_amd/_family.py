"""The covariance families of the engine as one table: which ``_ops`` entry assembles, differentiates and packs for each.

``RBF`` (scalar lengthscale in hyp[0]), ``RBF_ARD`` (one lengthscale per input dimension, csrc/assemble_ard.hip) and ``MATERN52``
(csrc/assemble_matern.hip) are records of callables with ONE call shape per slot; where the ``_ops`` signatures differ the entry adapts
them.  The RBF-only specialisations (stated one-hot directions, the values-only slice, the one-call steps) are not families: they keep
their explicit call sites in ``_step.py``.  A family whose ``packs_carry_ell`` is set runs on ``pack_points_ard`` packs with hyp[0] = 1."""
import collections

import torch

from . import _lib, _ops

Family = collections.namedtuple("Family", [
    "name",
    "hyp_forward",      # (ctx, raw_l, raw_s, raw_n) -> (ell [d] or None, hyp [4])
    "pack",             # (ctx, x, v, p, ell, hyp, center) -> pack
    "fwd_square",       # (ctx, pack1, n1, pack2, n2, d, p, hyp, jitter=, out=, dtype=): K_ZZ with jitter / float64 out, K_XX
    "fwd_rect",         # (ctx, pack1, n1, p1, pack2, n2, p2, d, hyp, out=): K_ZX
    "diag",             # (ctx, pack, n, p, d, hyp) -> prior diagonal [n (p + 1)]
    "diag_bwd",         # (ctx, pack, n, p, d, ell, hyp, out, gbar, d_ell, d_hyp), or None: closed form at the call site
    "bwd",              # (ctx, G, pack1, n1, p1, pack2, n2, p2, d, ell, hyp, symmetric, d_x1, d_v1, d_ell, d_hyp, workspace)
    "bwd_bytes",        # (n1, p1, n2, p2, d, symmetric) -> workspace bytes of ``bwd``
    "hyp_backward",     # (ctx, raw_l, raw_s, raw_n, d_ell, d_hyp, d_raw_l, d_raw_s, d_raw_n)
    "packs_carry_ell",  # the packs carry the per-dimension scaling, hyp[0] = 1, d_ell is a vector
    "expands_scalar_ell",   # a scalar raw_lengthscale runs as d equal entries and its gradient is summed back
])


def _rbf_bwd(ctx, G, pack1, n1, p1, pack2, n2, p2, d, ell, hyp, symmetric, d_x1, d_v1, d_ell, d_hyp, workspace=None):
    if symmetric:
        _ops.kernel_bwd(ctx, G, pack1, n1, pack2, n2, d, p1, hyp, True, d_x1, d_v1, d_hyp, workspace)
    else:
        _ops.kernel_bwd_rect(ctx, G, pack1, n1, p1, pack2, n2, p2, d, hyp, d_x1, d_v1, d_hyp, workspace)


def _ell_bwd(op):
    """``kernel_bwd_ard`` / ``kernel_bwd_matern52``: no direction gradient is asked for at p1 = 0"""
    def bwd(ctx, G, pack1, n1, p1, pack2, n2, p2, d, ell, hyp, symmetric, d_x1, d_v1, d_ell, d_hyp, workspace=None):
        op(ctx, G, pack1, n1, p1, pack2, n2, p2, d, ell, hyp, symmetric, d_x1, d_v1 if p1 > 0 else None, d_ell, d_hyp, workspace)
    return bwd


RBF = Family(
    "rbf",
    lambda ctx, rl, rs, rn: (None, _ops.hyp_forward(ctx, rl, rs, rn)),
    lambda ctx, x, v, p, ell, hyp, center: _ops.pack_points(ctx, x, v, p, hyp, center),
    _ops.kernel_fwd, _ops.kernel_fwd_rect,
    lambda ctx, pack, n, p, d, hyp: _ops.kernel_diag(ctx, n, p, hyp), None,
    _rbf_bwd,
    lambda n1, p1, n2, p2, d, symmetric: (int(_lib.lib.dsvgp_kernel_bwd_workspace_bytes(n1, n2, d, p1)) if symmetric
                                          else _ops.kernel_bwd_rect_workspace_bytes(n1, p1, n2, p2, d)),
    lambda ctx, rl, rs, rn, d_ell, d_hyp, g_l, g_s, g_n: _ops.hyp_backward(ctx, rl, rs, rn, d_hyp, g_l, g_s, g_n),
    False, False)

RBF_ARD = Family(
    "rbf_ard",
    _ops.hyp_forward_ard,
    lambda ctx, x, v, p, ell, hyp, center: _ops.pack_points_ard(ctx, x, v, p, ell, center),
    _ops.kernel_fwd_wide, _ops.kernel_fwd_rect,
    _ops.kernel_diag_ard, _ops.kernel_diag_ard_bwd,
    _ell_bwd(_ops.kernel_bwd_ard),
    lambda n1, p1, n2, p2, d, symmetric: _ops.kernel_bwd_ard_workspace_bytes(n1, p1, n2, p2, d),
    _ops.hyp_backward_ard,
    True, False)

MATERN52 = RBF_ARD._replace(
    name="matern52",
    fwd_square=lambda ctx, pack1, n1, pack2, n2, d, p, hyp, **kw: _ops.kernel_fwd_matern52(ctx, pack1, n1, p, pack2, n2, p, d, hyp, **kw),
    fwd_rect=_ops.kernel_fwd_matern52,
    diag=_ops.kernel_diag_matern52, diag_bwd=_ops.kernel_diag_matern52_bwd,
    bwd=_ell_bwd(_ops.kernel_bwd_matern52),
    bwd_bytes=lambda n1, p1, n2, p2, d, symmetric: _ops.kernel_bwd_matern52_workspace_bytes(n1, p1, n2, p2, d),
    expands_scalar_ell=True)


class PackKernelFn(torch.autograd.Function):
    """K(x1, x2; v1, v2) of a family whose packs carry the lengthscales (``RBF_ARD``, ``MATERN52``; ``ell`` [d], float32 inputs): the
    rectangular forward with hyp[0] = 1 and two calls of the family's kernel backward.  The first returns side 1's gradients and the
    whole lengthscale gradient (both sides' packed rows depend on ell); the second, on G^T with the sides swapped, only side 2's points
    and directions -- d_ell is not asked for again."""

    @staticmethod
    def _packs(x1, x2, v1, v2, ell):
        ctx = _ops.Context.get(x1.device)
        n1, d = x1.shape
        n2 = x2.shape[0]
        p1 = v1.shape[0] // n1 if n1 else 0
        p2 = v2.shape[0] // n2 if n2 else 0
        hyp = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float32, device=x1.device)
        ellc = ell.detach().float().reshape(-1).contiguous()
        x1c = x1.detach().float().contiguous()
        center = _ops.column_mean(ctx, x1c)
        pk1 = _ops.pack_points_ard(ctx, x1c, v1.detach().float().contiguous(), p1, ellc, center)
        pk2 = _ops.pack_points_ard(ctx, x2.detach().float().contiguous(), v2.detach().float().contiguous(), p2, ellc, center)
        return ctx, hyp, ellc, pk1, pk2, n1, n2, d, p1, p2

    @staticmethod
    def forward(actx, family, x1, x2, v1, v2, ell):
        ctx, hyp, _, pk1, pk2, n1, n2, d, p1, p2 = PackKernelFn._packs(x1, x2, v1, v2, ell)
        actx.save_for_backward(x1, x2, v1, v2, ell)
        actx.family = family
        return family.fwd_rect(ctx, pk1, n1, p1, pk2, n2, p2, d, hyp)

    @staticmethod
    def backward(actx, G):
        x1, x2, v1, v2, ell = actx.saved_tensors
        ctx, hyp, ellc, pk1, pk2, n1, n2, d, p1, p2 = PackKernelFn._packs(x1, x2, v1, v2, ell)
        need, bwd = actx.needs_input_grad, actx.family.bwd
        G = G.float().contiguous()
        z = lambda t: torch.zeros(t.shape, dtype=torch.float32, device=t.device)
        d_x1, d_v1, d_ell, d_hyp = z(x1), z(v1), torch.zeros_like(ellc), torch.zeros(4, dtype=torch.float32, device=x1.device)
        bwd(ctx, G, pk1, n1, p1, pk2, n2, p2, d, ellc, hyp, False, d_x1, d_v1, d_ell, d_hyp)
        d_x2 = d_v2 = None
        if need[2] or need[4]:
            d_x2, d_v2, scratch = z(x2), z(v2), torch.zeros(4, dtype=torch.float32, device=x1.device)
            bwd(ctx, G.t().contiguous(), pk2, n2, p2, pk1, n1, p1, d, ellc, hyp, False, d_x2, d_v2, None, scratch)
        cast = lambda g, t: None if g is None else g.to(t.dtype)
        return None, cast(d_x1, x1), cast(d_x2, x2), cast(d_v1, v1), cast(d_v2, v2), d_ell.to(ell.dtype).reshape(ell.shape)
