"""Matern-5/2 kernel with directional-derivative blocks: the call surface of ``RBFKernelDirectionalGrad`` (``forward(x1, x2,
diag=False, v1=, v2=)``, ``set_num_directions`` / ``num_outputs_per_input``, ``raw_lengthscale`` [1, 1] or [1, ard_num_dims] under the
same ``state_dict`` key, softplus constraint) on the Matern tile kernels (csrc/assemble_matern.hip).

k(r) = (1 + a + a^2/3) exp(-a), a = sqrt(5) |r|, r = (x1 - x2) ./ ell: twice mean-square differentiable, so value and first-derivative
observations are well defined.  The output is the dense interleaved ``[n1 (p1 + 1), n2 (p2 + 1)]`` block matrix, outputscale 1 (no
ScaleKernel factor), float32 only.  A scalar lengthscale runs as d equal ARD lengthscales: the packed rows carry them either way.
"""
import torch

from . import _ops
from ._family import MATERN52, PackKernelFn


class Matern52KernelDirectionalGrad(torch.nn.Module):
    def __init__(self, ard_num_dims=None):
        super().__init__()
        # gpytorch MaternKernel(nu=2.5): raw_lengthscale [1,1] ([1, ard_num_dims] with ARD), Positive (softplus) constraint, init 0
        self.ard_num_dims = None if ard_num_dims is None else int(ard_num_dims)
        if self.ard_num_dims is not None and self.ard_num_dims < 1:
            raise ValueError("ard_num_dims must be a positive integer or None")
        self.register_parameter("raw_lengthscale", torch.nn.Parameter(torch.zeros(1, self.ard_num_dims or 1)))
        self.n_dir1 = 0

    @property
    def lengthscale(self):
        return torch.nn.functional.softplus(self.raw_lengthscale)

    @lengthscale.setter
    def lengthscale(self, value):
        v = torch.as_tensor(value, dtype=self.raw_lengthscale.dtype, device=self.raw_lengthscale.device)
        with torch.no_grad():   # inverse softplus
            # (a scalar fills every dimension of an ARD kernel; a vector must have ard_num_dims entries)
            self.raw_lengthscale.copy_((v + torch.log(-torch.expm1(-v))).reshape(1, -1).expand_as(self.raw_lengthscale))

    def forward(self, x1, x2, diag=False, **params):
        n1, d = x1.shape[-2:]
        n2 = x2.shape[-2]
        v1, v2 = params["v1"], params["v2"]
        n_dir1 = int(v1.shape[-2] / n1)
        n_dir2 = int(v2.shape[-2] / n2)
        assert n_dir1 == n_dir2, "v1 and v2 must contain same number of directions"
        self.set_num_directions(n_dir1)
        if self.ard_num_dims is not None and d != self.ard_num_dims:
            raise RuntimeError("inputs have %d dimensions, the kernel has ard_num_dims = %d" % (d, self.ard_num_dims))
        if x1.dtype == torch.float64 or x2.dtype == torch.float64:
            raise ValueError("float64 inputs are not supported by the Matern-5/2 kernel")
        # d lengthscales for the pack (a scalar: d equal ones; autograd sums the vector's gradient back into the scalar)
        ell = self.lengthscale.reshape(-1).to(x1.device).expand(d)
        if not diag:    # an autograd participant: gradients reach x1, x2, v1, v2 and the lengthscale through dsvgp_kernel_bwd_matern52
            return PackKernelFn.apply(MATERN52, x1, x2, v1, v2, ell)
        if not (n1 == n2 and torch.eq(x1, x2).all() and torch.eq(v1, v2).all()):
            raise RuntimeError("diag=True only works when x1 == x2 and v1 == v2")
        with torch.no_grad():
            ctx = _ops.Context.get(x1.device)
            pack = _ops.pack_points_ard(ctx, x2.float().contiguous(), v2.float().contiguous(), n_dir2, ell.float().contiguous())
            return _ops.kernel_diag_matern52(ctx, pack, n2, n_dir2, d, torch.tensor([1.0, 1.0, 0.0, 0.0], device=x1.device))

    def set_num_directions(self, num_directions):
        self.n_dir1 = num_directions

    def num_outputs_per_input(self, x1, x2):
        return self.n_dir1 + 1
