"""Generate tests/golden/fp64dirs_*.npz: the reference's kernel file run in float64 at MORE THAN 16 DIRECTIONS per point -- the
geometries the tiled fp64 assembly (csrc/assemble64_tiled.hip) opens: the full-gradient model (p = d) on the Welch (d = 20) and
stellarator (d = 45) inputs, p = 17, the largest micro-block q = p + 1 = 96, a symmetric (K_ZZ) case with its diag=True vector
and canonical (one-hot) directions on side 2.

Runs only where the reference checkout exists (oracle/make_golden.py imports its kernel file from where it lies); the tests
only see the committed vectors.  Storage format of oracle/make_golden.py (read by tests/_golden.kernel_error): ``K`` whole, or
``K_sub`` at ``K_rows`` x ``K_cols`` + the row / column sums of the whole matrix.  The whole-matrix limit is lower than there
(the direction inputs grow with n p d and every file has to stay well below 1 MiB).

Usage:  python tools/make_fp64dirs_fixtures.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
from make_golden import FULL_LIMIT, OUT, load_reference_kernel  # noqa: E402

WHOLE_LIMIT = min(FULL_LIMIT, 60000)

# (name, n1, n2, d, p, lengthscale, same_inputs, one_hot_v2)
CASES = [
    ("welch_fullgrad", 25, 30, 20, 20, 0.8, False, False),
    ("stellarator_fullgrad", 9, 11, 45, 45, 1.6, False, False),
    ("p17_d24", 12, 14, 24, 17, 0.9, False, False),
    ("q96", 4, 5, 95, 95, 2.5, False, False),
    ("sym_p20", 14, 14, 20, 20, 0.7, True, False),
    ("onehot_p17", 12, 14, 24, 17, 1.1, False, True),
]


def main():
    Kern = load_reference_kernel()
    g = torch.Generator().manual_seed(20261016)
    for name, n1, n2, d, p, ell, same, onehot in CASES:
        k = Kern()
        k._ell = torch.tensor([[ell]], dtype=torch.float64)
        x1 = torch.rand(n1, d, dtype=torch.float64, generator=g)
        v1 = torch.randn(n1 * p, d, dtype=torch.float64, generator=g)     # non-unit: exercises normalisation
        if same:
            x2, v2 = x1.clone(), v1.clone()
        else:
            x2 = torch.rand(n2, d, dtype=torch.float64, generator=g)
            if onehot:
                idx = torch.randperm(d, generator=g)[:p].sort().values
                v2 = torch.eye(d, dtype=torch.float64)[idx].repeat(n2, 1)
            else:
                v2 = torch.randn(n2 * p, d, dtype=torch.float64, generator=g)
        with torch.no_grad():
            K = k.forward(x1, x2, v1=v1, v2=v2)
            out = dict(x1=x1.numpy(), x2=x2.numpy(), v1=v1.numpy(), v2=v2.numpy(), lengthscale=np.float64(ell), p=np.int64(p))
            if K.numel() <= WHOLE_LIMIT:
                out["K"] = K.numpy()
            else:
                # rows / columns around every micro-block edge multiple of 48 / 64 / 96 (the tile edges of the assembly kernels),
                # the first and last ones, and a seeded random rest
                def pick(n):
                    edges = [e + o for step in (48, 64, 96, p + 1) for e in range(step, n, step) for o in (-1, 0)][:200] + [0, n - 1]
                    rest = torch.randperm(n, generator=g)[:64].tolist()
                    return torch.tensor(sorted(set(edges + rest)))
                rows, cols = pick(K.shape[0]), pick(K.shape[1])
                out.update(K_rows=rows.numpy(), K_cols=cols.numpy(), K_sub=K[rows][:, cols].numpy(),
                           K_rowsum=K.sum(1).numpy(), K_colsum=K.sum(0).numpy(), K_shape=np.array(K.shape))
            if same:
                out["Kdiag"] = k.forward(x1, x2, diag=True, v1=v1, v2=v2).numpy()
        path = os.path.join(OUT, "fp64dirs_%s.npz" % name)
        np.savez_compressed(path, **out)
        print("wrote %s %s (%d bytes)" % (os.path.basename(path), tuple(K.shape), os.path.getsize(path)))


if __name__ == "__main__":
    main()
