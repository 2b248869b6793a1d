"""Host-side contract of the wide-input assembly (packed width > 96, d >= 93): workspace sizing, CPU only."""
import pytest


def test_kernel_bwd_workspace_covers_wide_inputs(dsvgp):
    lib = dsvgp._lib.lib
    # the rover geometry of the paper's Bayesian-optimisation runs (d = 200) and the GCN one (d = 4035): both were 0 (rejected)
    assert lib.dsvgp_kernel_bwd_workspace_bytes(500, 4096, 200, 5) > 0
    assert lib.dsvgp_kernel_bwd_workspace_bytes(10, 256, 4035, 10) > 0
    # the largest width of the whole-row kernels and the first of the wide ones
    assert lib.dsvgp_kernel_bwd_workspace_bytes(50, 60, 92, 3) > 0
    assert lib.dsvgp_kernel_bwd_workspace_bytes(50, 60, 93, 3) > 0
    # at d >= 93 the general entry sizes for the wide kernels
    for n1, n2, d, p in [(500, 4096, 200, 5), (10, 256, 4035, 10), (7, 9, 93, 0)]:
        assert (lib.dsvgp_kernel_bwd_workspace_bytes(n1, n2, d, p)
                == lib.dsvgp_kernel_bwd_wide_workspace_bytes(n1, n2, d, p))
    # q = p + 1 > 96 stays outside both
    assert lib.dsvgp_kernel_bwd_workspace_bytes(500, 4096, 20, 200) == 0
    assert lib.dsvgp_kernel_bwd_wide_workspace_bytes(500, 4096, 20, 200) == 0


def test_wide_workspace_at_small_d_and_its_size(dsvgp):
    lib = dsvgp._lib.lib
    assert lib.dsvgp_kernel_bwd_wide_workspace_bytes(16, 16, 20, 5) > 0
    assert lib.dsvgp_kernel_bwd_wide_workspace_bytes(0, 16, 20, 5) == 0
    assert lib.dsvgp_kernel_bwd_wide_workspace_bytes(16, 16, 0, 5) == 0
    # at least the Tbar scratch (n1q x n2q floats) plus one slab (n1q x NP floats)
    n1, n2, d, p = 10, 256, 4035, 10
    q, NP = p + 1, (dsvgp._ops.packed_width(d) + 15) // 16 * 16
    assert lib.dsvgp_kernel_bwd_wide_workspace_bytes(n1, n2, d, p) >= 4 * (n1 * q * n2 * q + n1 * q * NP)


@pytest.mark.parametrize("d", [88, 92, 93, 200, 4035])
def test_packed_width_is_unchanged(dsvgp, d):
    assert dsvgp._ops.packed_width(d) == ((d + 3) // 4) * 4 + 4
