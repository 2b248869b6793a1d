"""tests/_conditioning.py kept honest without a GPU: the regimes are not vacuous on any shape tests/test_gpu_conditioning.py uses, and the
per-block metric sees broken block formulas that the suite's whole-matrix ``relmax`` (and its ``2e-4 max(1, |g|)`` backward check) accept.

Mutants of the float64 kernel: Hessian block zero, ``u w`` term dropped, right-derivative block zero, and a float32 restatement of the
packed formulation without the centre shift.  Measured at (37, 53, 20, 5), whole-matrix relmax / worst block error over its bound:

    Hessian zero     scaled_up 6.1e-7 / 7.5e5      u w dropped     long64 1.7e-7 / 5.1e2, scaled_up 6.0e-7 / 7.5e5
    right zero       scaled_up 7.2e-4 / 9.3e5      no centre       offset 3.4 / 3.9e6; elsewhere 1.8e-5 (short), 3.9e-5 (clusters), <= 2.3e-6

The right-derivative block scales as s / ell, so at the longest lengthscale of the table (1e3 ell0) its loss still shows at 7.2e-4 of the
value maximum: no regime hides it from the forward's old metric below 2e-5.  It hides in the backward instead (d_ell off by 1.6e-5 under
the old absolute tolerance), which is asserted; for the forward the test asserts the figure the table gives, a 1000x drop from ``base``."""
import pytest
import torch

import dsvgp_oracle as O
import _conditioning as C

f64 = torch.float64
PAIRS = [(r, g, s) for r in C.ROUTES for g in C.REGIMES for s in ((False, True) if r in C.SYMMETRIC_ROUTES else (False,))]
ROUTE = "pair-q6-ksm8"                                      # (37, 53, 20, 5)


def visible(K, K_ref, c, bound):
    """worst block error / its bound"""
    e = C.block_errors(K, K_ref, c.n1, c.q1, c.n2, c.q2)
    return max(e[k] / bound[k] for k in e)


@pytest.mark.parametrize("route,regime,symmetric", PAIRS, ids=["%s-%s%s" % (r, g, "-sym" if s else "") for r, g, s in PAIRS])
def test_regime_is_not_vacuous(route, regime, symmetric):
    assert C.conditions(route, regime, symmetric) == []


def test_the_bound_is_plain_except_in_the_four_formulation_limited_pairs():
    """every (route, regime) is held to 4 y + 2e-7 (fp64: 4 y + 1e-13) but the pairs of ``C.FORMULATION_LIMITED``: ARD and Matern, whose
    yardsticks are difference-form, in ``short`` and ``clusters``.  There the float32 restatement of the packed formulation on the CPU
    exceeds 4 y + 2e-7 itself (asserted; measured 1.8x ... 6.4x in its worst block), and the bound is 4x its error per block.  For every
    other pair the restatement's distance to the plain bound is printed, not asserted and not used: it is a float32 sum that differs
    between CPUs (isotropic routes: 0.63 of the bound at most on one CPU; on another canon2 ``short`` was seen at 1.01)."""
    assert set(C.FORMULATION_LIMITED) == {("ard", "short"), ("ard", "clusters"), ("matern", "short"), ("matern", "clusters")}
    worst = (0.0, None)
    for route, regime, symmetric in PAIRS:
        bound, exc = C.effective_bounds(route, regime, symmetric)
        plain = C.bounds(C.reference(route, regime, symmetric)[2], C.ROUTES[route][0] == "rbf64")
        pr = C.restatement_errors(route, regime, symmetric)
        if (route, regime) in C.FORMULATION_LIMITED:
            over = max(pr[k] / plain[k] for k in plain)
            print("[parity] formulation-limited %s %s: restatement / (4 y + 2e-7) %s" % (route, regime, ", ".join("%s %.2f" % (k, pr[k] / plain[k]) for k in plain)))
            assert over > 1.0 and max(pr.values()) < C.OLD_KTOL, (route, regime, pr, plain)
            assert bound == {k: max(plain[k], 4 * pr[k]) for k in plain}
        else:
            assert exc == {} and bound == plain
            if not symmetric:
                worst = max(worst, (max(pr[k] / plain[k] for k in plain), (route, regime)))
    print("[parity] restatement / plain bound elsewhere, worst: %.2f at %s" % worst)


def test_truths_agree():
    """the differentiable kernel the mutants are cut from, the ARD yardstick at equal lengthscales and the oracle's kernel are one matrix"""
    c, K, _ = C.reference(ROUTE, "base")
    s = torch.tensor(C.S, dtype=f64)
    assert C.relmax(C.mutant_kernel(c.x1, c.v1, c.p1, c.x2, c.v2, c.p2, c.ell, s), K) < 1e-13
    assert C.relmax(C.S * C.ard_kernel(c.x1, c.v1, c.p1, c.x2, c.v2, c.p2, c.ell.expand(c.d)), K) < 1e-13
    assert C.relmax(C.S * O.kernel_matrix_refseq(c.x1, c.x2, c.v1, c.v2, c.ell), K) < 1e-12
    c, K, _ = C.reference("rect-p2-4", "base")
    assert C.relmax(C.packed_restatement(c, dtype=f64), K) < 1e-12


def _mutant(c, m):
    return C.mutant_kernel(c.x1, c.v1, c.p1, c.x2, c.v2, c.p2, c.ell, torch.tensor(C.S, dtype=f64), m)


@pytest.mark.parametrize("mutant,regimes", [("hessian_zero", ("scaled_up",)), ("uw_dropped", ("scaled_up", "long64"))])
def test_forward_mutant_hides_from_relmax_and_not_from_the_block_bound(mutant, regimes):
    for regime in regimes:
        c, K, y = C.reference(ROUTE, regime)
        Km = _mutant(c, mutant)
        old, new = C.relmax(Km, K), visible(Km, K, c, C.bounds(y))
        print("[parity] mutant %s in %s: whole-matrix relmax %.2e, worst block / bound %.3g" % (mutant, regime, old, new))
        assert old < C.OLD_KTOL and new >= 100


def test_forward_right_zero_mutant():
    """no regime of the table brings a lost right-derivative block below 2e-5 of the value maximum (7.2e-4 at ell = 1e3 ell0): asserted
    is the 1000x drop the s / ell scaling gives, and the block bound's 100x in every regime"""
    fig = {}
    for regime in C.REGIMES:
        c, K, y = C.reference(ROUTE, regime)
        Km = _mutant(c, "right_zero")
        fig[regime] = C.relmax(Km, K)
        assert visible(Km, K, c, C.bounds(y)) >= 100
    print("[parity] mutant right_zero: whole-matrix relmax %s" % ", ".join("%s %.2e" % kv for kv in fig.items()))
    assert fig["scaled_up"] < 1e-3 * 1.001 * fig["base"] and fig["scaled_up"] > C.OLD_KTOL


def test_forward_without_the_centre_shift_shows_only_away_from_the_origin():
    """the float32 packed formulation without the shift: within the old 2e-5 at the origin (asserted but for ``short``, 1.8e-5, and ``clusters``), wrong by more than the
    whole matrix at offset 1024; the block bound sees that at more than 100x.  (``clusters``: 3.9e-5, the centred yardstick itself 1.4e-5.)"""
    for regime in C.REGIMES:
        c, K, y = C.reference(ROUTE, regime)
        Kn = C.packed_restatement(c, centre=False)
        old, new = C.relmax(Kn, K), visible(Kn, K, c, C.bounds(y))
        print("[parity] no-centre restatement in %s: whole-matrix relmax %.2e, worst block / bound %.3g" % (regime, old, new))
        if regime == "offset":
            assert old > C.OLD_KTOL and new >= 100
        elif regime not in ("clusters", "short"):          # (short: 1.8e-5, too close to 2e-5 for a float32 sum that differs between CPUs)
            assert old < C.OLD_KTOL
    # the reference op sequence itself, un-centred in float32 at offset 1024: wrong by ~1e-3 of the maximum; centred it is the yardstick
    c, K, y = C.reference(ROUTE, "offset")
    raw = C.S * O.kernel_matrix_refseq(c.x1.float(), c.x2.float(), c.v1.float(), c.v2.float(), float(c.ell)).double()
    assert C.relmax(raw, K) > 1e-4 and max(y.values()) < 1e-6


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_backward_mutant_hides_from_the_old_check_and_not_from_the_masked_one(mutant):
    """autograd through the mutant: under the upstream masked to the broken block some gradient misses float64 autograd through the true
    kernel by more than 100x the new bound, while the old dense ``|d_ell - ref| < 2e-4 max(1, |ref|)`` accepts it (``scaled_up``)"""
    c, ref = C.backward_reference(ROUTE, "scaled_up")
    leaves = [t.clone().requires_grad_(True) for t in (c.x1, c.v1, c.ell, torch.tensor(C.S, dtype=f64))]
    Km = C.mutant_kernel(leaves[0], leaves[1], c.p1, c.x2, c.v2, c.p2, leaves[2], leaves[3], mutant)
    mask = C.MUTANT_BLOCK[mutant]
    got = torch.autograd.grad((Km * ref[mask]["G"]).sum(), leaves, retain_graph=True)
    errs = {k: v for k, v in C.backward_errors(got, ref[mask]).items() if v is not None}
    dense = torch.autograd.grad((Km * ref["dense"]["G"]).sum(), leaves)
    te = float(ref["dense"]["truth"][2])
    old = abs(float(dense[2]) - te) / max(1.0, abs(te))
    print("[parity] backward mutant %s, %s mask: %s; dense d_ell under the old check %.2e (true d_ell %.3e)"
          % (mutant, mask, ", ".join("%s %.2e" % kv for kv in errs.items()), old, te))
    assert max(errs.values()) > 100 * C.BWD_TOL and old < C.OLD_BWD_TOL
    # the yardstick passes the masked check with room
    yard = {k: v for k, v in C.backward_errors(ref[mask]["yard"], ref[mask]).items() if v is not None}
    assert max(yard.values()) < 0.05 * C.BWD_TOL, yard
