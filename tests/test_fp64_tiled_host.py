"""Host-side contract of the tiled fp64 assembly (csrc/assemble64_tiled.hip, any p <= 95): declared and exported entries,
workspace sizing.  CPU only."""
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64DIRS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "fp64dirs_*.npz")))
ENTRIES = ("dsvgp_kernel_fwd_f64", "dsvgp_kernel_bwd_f64_workspace_bytes", "dsvgp_kernel_bwd_f64")


def test_tiled_entries_are_declared_and_exported(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), "not declared: " + name
        assert hasattr(dsvgp._lib.lib, name), "missing export: " + name
        assert name in dsvgp._lib.SIGNATURES
    assert callable(dsvgp._ops.kernel_fwd_f64_tiled) and callable(dsvgp._ops.kernel_bwd_f64_tiled)


@pytest.mark.parametrize("n1,n2,d,p", [(500, 4096, 20, 5), (100, 512, 20, 20), (50, 256, 45, 45), (4, 6, 95, 95),
                                       (10, 256, 4035, 10)])
def test_workspace_is_sized_for_every_geometry_taken(dsvgp, n1, n2, d, p):
    nbytes = dsvgp._lib.lib.dsvgp_kernel_bwd_f64_workspace_bytes(n1, n2, d, p)
    assert nbytes > 0
    # dP1 = Tbar [P2 | indicator]: n1 (p + 1) rows of the packed width, and nothing of the size of the kernel matrix
    assert nbytes == 8 * n1 * (p + 1) * dsvgp._ops.packed_width(d)


@pytest.mark.parametrize("n1,n2,d,p", [(4, 6, 95, 96), (16, 16, 0, 5), (0, 16, 20, 5), (16, 16, 20, -1)])
def test_workspace_is_zero_for_geometries_not_taken(dsvgp, n1, n2, d, p):
    assert dsvgp._lib.lib.dsvgp_kernel_bwd_f64_workspace_bytes(n1, n2, d, p) == 0


def test_fp64dirs_vectors_cover_the_geometries():
    names = {os.path.basename(p)[len("fp64dirs_"):-len(".npz")]: np.load(p) for p in FP64DIRS}
    assert set(names) == {"welch_fullgrad", "stellarator_fullgrad", "p17_d24", "q96", "sym_p20", "onehot_p17"}
    geo = {k: (g["x1"].shape[1], int(g["p"])) for k, g in names.items()}
    assert geo["welch_fullgrad"] == (20, 20) and geo["stellarator_fullgrad"] == (45, 45) and geo["p17_d24"] == (24, 17)
    assert geo["q96"] == (95, 95) and "Kdiag" in names["sym_p20"]
    v2 = names["onehot_p17"]["v2"]
    assert set(np.unique(v2)) == {0.0, 1.0} and bool((v2.sum(1) == 1.0).all())
    assert all(os.path.getsize(p) <= 1400000 for p in FP64DIRS)
