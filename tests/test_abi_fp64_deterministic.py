"""CPU: the C ABI of the deterministic float64 model mode -- ``dsvgp_deterministic_f64_scratch_bytes`` (exported, declared, bound, a
pure host function, monotone, large enough for the tiled kernel backward's slabs) and the engine switch.  Nothing here touches a GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gp-derivatives-variational-inference_amd", "csrc")
NAME = "dsvgp_deterministic_f64_scratch_bytes"

# (M, d, p, B) of the benchmark configurations (bench.py CONFIGS)
C2, C3, C4 = (200, 5, 2, 512), (300, 10, 10, 512), (500, 20, 5, 4096)


def test_scratch_size_function_is_exported_declared_and_bound(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    assert hasattr(dsvgp._lib.lib, NAME), "missing export: " + NAME
    assert NAME in dsvgp._lib.SIGNATURES, "missing binding: " + NAME
    assert re.search(r"\bsize_t\s+%s\s*\(\s*int M, int d, int p, int B\s*\)" % NAME, hdr), "not declared in include/dsvgp.h"


def test_scratch_size_function_is_a_pure_host_function(dsvgp):
    """it answers without a device (this test runs where there is none), names no context and makes no HIP call"""
    lib = dsvgp._lib.lib
    assert lib.dsvgp_deterministic_f64_scratch_bytes(*C2) == lib.dsvgp_deterministic_f64_scratch_bytes(*C2) > 0
    src = open(os.path.join(CSRC, "det64.hip")).read()
    body = src[src.index('extern "C" size_t ' + NAME):]
    body = body[:body.index("\n}\n") + 3]
    assert "dsvgp_ctx" not in body and not re.search(r"\bhip[A-Z]\w*\s*\(", body), body
    # shapes the float64 entry points do not take
    for shape in ((0, 5, 2, 64), (10, 0, 0, 64), (10, 5, -1, 64), (10, 5, 96, 64), (10, 5, 2, 0)):
        assert lib.dsvgp_deterministic_f64_scratch_bytes(*shape) == 0, shape


def test_scratch_size_is_nonzero_at_the_benchmark_shapes_and_monotone(dsvgp):
    f = dsvgp._lib.lib.dsvgp_deterministic_f64_scratch_bytes
    for M, d, p, B in (C2, C3, C4, (60, 20, 20, 1024), (40, 100, 20, 512), (70, 6, 0, 64)):
        Mp, Bp = M * (p + 1), B * (p + 1)
        n = f(M, d, p, B)
        assert n > 0 and n % 256 == 0
        assert n >= 2 * 8 * Mp * (Mp + 1)                  # at least two split-K slabs of an [M', M' + 1] product
        assert n >= 2 * 8 * 2 * Bp                         # ... two partial rows of both column sums over B'
    for d, p in ((5, 2), (20, 5), (20, 20), (100, 20)):
        prev = 0
        for M in (10, 40, 100, 200, 400):
            n = f(M, d, p, 512)
            assert n >= prev, (M, d, p)
            prev = n
        prev = 0
        for B in (16, 64, 512, 2048, 8192):
            n = f(60, d, p, B)
            assert n >= prev, (B, d, p)
            prev = n
    assert f(400, 20, 20, 512) > f(40, 20, 20, 512) and f(60, 20, 20, 8192) > f(60, 20, 20, 512)


def _tiled_slab_doubles(n1, n2, d, p):
    """nsg x n1 q x DP from the launcher's own rules (csrc/assemble64_tiled.hip geo_of, csrc/common.h bwd64_tiled_sweep)"""
    q = p + 1
    R = 64 // q if q <= 64 else 1
    Tt = R * q
    ntr, ntc = -(-n1 * q // Tt), -(-n2 * q // Tt)
    sweep = max(1, min(min(ntr * ntc // 1024, 32), ntc))
    nsg = -(-ntc // sweep)
    DP = (d + 3) // 4 * 4 + 4
    return nsg, nsg * n1 * q * DP


def test_scratch_holds_the_tiled_backward_slabs(dsvgp):
    f = dsvgp._lib.lib.dsvgp_deterministic_f64_scratch_bytes
    src = open(os.path.join(CSRC, "common.h")).read()
    assert re.search(r"sweep = \(int\)\(\(\(int64_t\)ntr \* ntc\) / 1024\);", src) and "sweep < 32 ? sweep : 32" in src      # (the rule recomputed above)
    for M, d, p, B in ((60, 20, 20, 1024), (40, 100, 20, 512), (12, 45, 45, 400), (4, 95, 95, 64), (90, 24, 17, 2048)):
        nsg_zx, zx = _tiled_slab_doubles(M, B, d, p)
        nsg_zz, zz = _tiled_slab_doubles(M, M, d, p)
        assert f(M, d, p, B) >= 8 * max(zx, zz), (M, d, p, B)
    assert _tiled_slab_doubles(60, 1024, 20, 20)[0] == 57 and _tiled_slab_doubles(40, 512, 100, 20)[0] == 86      # several groups per tile row


def test_fp64_engine_takes_the_deterministic_switch(dsvgp, monkeypatch):
    import inspect
    import torch
    from dsvgp_amd._step64 import ElboEngine64
    assert ElboEngine64(torch.device("cpu")).deterministic is False
    monkeypatch.setenv("DSVGP_DETERMINISTIC", "1")
    assert ElboEngine64(torch.device("cpu")).deterministic is True
    src = inspect.getsource(ElboEngine64.loss_and_grads)
    assert "dsvgp_deterministic_f64_scratch_bytes" in src and "set_deterministic(None)" in src and "finally" in src
