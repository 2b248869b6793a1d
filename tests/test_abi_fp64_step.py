"""CPU: the C ABI of the float64 model mode's one-call ELBO step (``dsvgp_elbo_step_f64``, csrc/step64.hip) -- exports, the pure host
functions that size and gate it, the versioned io struct, and the engine switch.  Nothing here touches a GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["dsvgp_elbo_step_f64_supported", "dsvgp_elbo_step_f64_workspace_bytes", "dsvgp_elbo_step_f64_plan_create",
               "dsvgp_elbo_step_f64_plan_destroy", "dsvgp_elbo_step_f64", "dsvgp_elbo_step_f64_status", "dsvgp_elbo_step_f64_timings",
               "dsvgp_gather_batch_f64"]

# (M, d, p, B) of the benchmark configurations (bench.py CONFIGS)
C2, C3, C4 = (200, 5, 2, 512), (300, 10, 10, 512), (500, 20, 5, 4096)


def test_library_exports_the_fp64_step_symbols(dsvgp):
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(dsvgp._lib.lib, n), "missing export: " + n
        assert n in dsvgp._lib.SIGNATURES, "missing binding: " + n
        assert re.search(r"\b%s\s*\(" % n, hdr), "not declared in include/dsvgp.h: " + n


def test_fp64_step_supported_and_workspace_are_pure_host_functions(dsvgp):
    lib = dsvgp._lib.lib
    for shape in (C2, C3, C4, (12, 45, 45, 40), (20, 200, 3, 48), (12, 20, 20, 40), (70, 6, 0, 64)):
        assert lib.dsvgp_elbo_step_f64_supported(*shape) == 1, shape
        assert lib.dsvgp_elbo_step_f64_workspace_bytes(*shape) > 0, shape
    # outside the explicit-inverse regime M (p + 1) <= 8192, beyond the assembly's p <= 95, degenerate shapes
    for shape in ((1366, 20, 5, 512), (8193, 3, 0, 64), (10, 100, 96, 16), (0, 5, 2, 64), (10, 0, 0, 64), (10, 5, -1, 64), (10, 5, 2, 0)):
        assert lib.dsvgp_elbo_step_f64_supported(*shape) == 0, shape
        assert lib.dsvgp_elbo_step_f64_workspace_bytes(*shape) == 0, shape
    assert lib.dsvgp_elbo_step_f64_supported(1365, 20, 5, 512) == 1            # M (p + 1) = 8190
    M, d, p, B = C4
    Mp, Bp = M * (p + 1), B * (p + 1)
    # K_ZX / K_ZX-bar, [A ; mu_bar^T] and the register assembly's T scratch; L, L^-1 and the M' x M' operands
    assert lib.dsvgp_elbo_step_f64_workspace_bytes(M, d, p, B) >= 8 * (3 * Mp * Bp + 3 * Mp * Mp)
    # same shape, more minibatch rows: more bytes
    assert lib.dsvgp_elbo_step_f64_workspace_bytes(M, d, p, 2 * B) > lib.dsvgp_elbo_step_f64_workspace_bytes(M, d, p, B)


def test_fp64_step_io_struct_leads_with_its_size_and_has_no_direction_index_fields(dsvgp):
    io = dsvgp._lib.ElboStepIO64()
    names = [f[0] for f in io._fields_]
    assert names[0] == "struct_size" and io.struct_size == C.sizeof(dsvgp._lib.ElboStepIO64)
    assert "dir_idx" not in names and "v_one_hot" not in names and "split_ws" not in names
    assert all(getattr(io, n) in (None, 0, 0.0) for n in names[1:])              # a fresh struct is zeroed
    # the header's struct and the binding agree on the field list (order included)
    hdr = open(os.path.join(ROOT, "include", "dsvgp.h")).read()
    body = re.search(r"typedef struct dsvgp_elbo_step_io_f64 \{(.*?)\} dsvgp_elbo_step_io_f64;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        first, *rest = stmt.split(",")
        declared.append(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", first)[-1])
        declared += [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", r)[-1] for r in rest]
    assert declared == names


def test_fp64_engine_carries_the_one_call_switch(dsvgp, monkeypatch):
    import torch
    from dsvgp_amd._step64 import ElboEngine64
    assert hasattr(ElboEngine64, "_c_step64") and hasattr(ElboEngine64, "_c_step64_eligible")
    assert hasattr(dsvgp._ops, "StepPlan64") and hasattr(dsvgp._ops, "gather_batch_f64")
    eng = ElboEngine64(torch.device("cpu"))        # (construction allocates nothing)
    assert eng.c_step is True and eng.c_step_used is False
    monkeypatch.setenv("DSVGP_C_STEP", "0")
    assert ElboEngine64(torch.device("cpu")).c_step is False
