"""The edges of data and state for the three operator-by-operator families of the residual-tolerance solver -- the variable
coefficient (include/mg_varcoef.h), the boundary kinds (mg_bc.h) and the singular solve (mg_singular.h) -- which share one
recorded cycle and keep solver-owned level storage: coef[], the boundary tables and sing_F.  tests/test_solve_truth_gpu.py
shows these edges to the plain solver path only.  Here, at N = 65 (65 -> 32 -> 16 -> 8) with the coefficient "smooth":

  NaN in F           two cycles, every norm NaN, no error, the coarse loop left after one iteration (it ends on !(err > target))
  clean afterwards   one solver sees a NaN problem, a problem whose coarse solve is capped and a problem scaled by 2^-40: the
                     last comes out as from a fresh solver, bit for bit, and as the restatement has it
  magnitudes         F, U0 and the target mean scaled by 2^+-300: U, history, ref_norm, compat_defect and mean_before scale
                     bit for bit; the unscaled solve is first held to the restatement
  F = 0              singular: the answer is the constant `mean`, max|U - mean| <= 2*||r(U)||/(a_min*lambda+) + the gauge term;
                     "vc" and "bc": the harmonic 1 + x^2 - y^2 with a = 2, which is even about the Neumann sides S and W of
                     "ndnd" and which the 5-point stencil solves exactly (_exact.check_mode_solve's bound and teeth)
  no cycle           singular, max_cycles = 0 and a start that already meets the tolerance: U is still shifted to the target
                     mean, F's defect still reported (step 3 of the header, "also when no cycle ran")
The cases are tests/_singular_forms_cases.py's; tests/test_singular_forms_cpu.py proves on the restatements what they rest on
(which problem caps, exact scaling, the distance of the norms from the tolerances).

Measured on the MI355X (16 tests): every bit comparison holds, for 2^300 and 2^-300 alike.  F = 0, singular: 15 cycles,
max|U - mean| 3.4e-13 <= 3.6e-10 with a_min*lambda+ = 4.93.  Laplace: 11 cycles each, |U - U*| 6.1e-12 <= 1.8e-9 ("vc") and
2.4e-12 <= 2.9e-9 ("bc"), res 1.6e-13 and 7.4e-12 from ||r(U)|| against rounding bounds of 6.7e-9 and 6.8e-9.  The solve that
finishes takes 14 cycles to rtol 1e-9 and ends at 0.248 of the tolerance; put back in, its U starts at 0.249 of it (the final
shift rounds every point once more) and no cycle runs.  Every test takes less than 0.1 s."""
import numpy as np
import pytest

import _bc_ref as bref
import _exact as ex
import _singular_forms_cases as cases
import _singular_ref as sref
import _solve_ref as ref
from conftest import assert_bits
from test_singular_gpu import ptable, rtable

pytestmark = pytest.mark.gpu
N = cases.EDGE_N
BC = cases.BC
SINGULAR_KEYS = ("compat_defect", "mean_before")


def _solver(mg, family, a=None, mean=cases.EDGE_MEAN, **opts):
    return mg.Solver(N, 1.0, **cases.edge_kwargs(family, cases.edge_coef() if a is None else a, mean), **opts)


def _restated(mg, oracle, family, F, U0, a=None, mean=cases.EDGE_MEAN, **opts):
    return cases.edge_restated(family, cases.edge_coef() if a is None else a, F, U0, mean, orc=oracle, rtable=rtable(mg),
                               ptable=ptable(mg), **opts)


def _ref_norm(family, F, info):
    return ref.ref_norm(F) if family == "vc" else bref.ref_norm(info["Ft"] if family == "singular" else F, cases.EDGE_KINDS[family])


def _same_as_restated(family, got, ginfo, F, restated, what):
    """bits of U, cycle count, the singular pair with ==, norms to 1e-12 (they differ in summation order alone)"""
    U, hist, k, conv, info, margins, capped = restated
    ref.assert_qualified(margins, what)
    assert_bits(got, U, f"{what}: U against the restatement")
    assert ginfo["cycles"] == k and ginfo["converged"] == conv and bool(ginfo["coarse_capped"]) == any(capped)
    np.testing.assert_allclose(ginfo["history"], hist, rtol=1e-12, atol=0.0)
    rn = _ref_norm(family, F, info)
    assert abs(ginfo["ref_norm"] - rn) <= 1e-12 * rn
    for key in SINGULAR_KEYS if family == "singular" else ():
        assert ginfo[key] == info[key], key


@pytest.mark.parametrize("family", cases.FAMILIES)
def test_nan_in_F_ends_after_max_cycles(mg, family):
    F, U0 = cases.nan_problem()
    s = _solver(mg, family, **cases.NAN_OPTS)
    _, info = s.solve(F, U0)
    s.close()
    assert info["status"] == mg.MG_SOLVE_NOT_CONVERGED and not info["converged"] and info["cycles"] == 2
    assert len(info["history"]) == 3 and all(np.isnan(h) for h in info["history"]) and np.isnan(info["ref_norm"])
    if family == "singular":
        assert np.isnan(info["compat_defect"])
    assert mg.lib().mg_last_error() == 0


@pytest.mark.parametrize("family", cases.FAMILIES)
def test_a_solver_is_clean_after_nan_and_capped_problems(mg, oracle, family):
    """an absolute coarse target of 1e-3 and 3 coarse iterations at most: the problem of unit magnitude runs into the cap, the
    one scaled by 2^-40 meets the target in its first iteration.  After a NaN problem and a capped one the small problem comes
    out as from a fresh solver: no NaN survived in coef[], sing_F or a level buffer, no flag stayed set."""
    Fn, Un = cases.nan_problem()
    Fc, Uc = cases.capped_problem()
    F, U0 = cases.small_problem()
    assert all(_restated(mg, oracle, family, Fc, Uc, **cases.CAP_OPTS)[6])
    small = _restated(mg, oracle, family, F, U0, **cases.CAP_OPTS)
    assert not any(small[6])
    fresh = _solver(mg, family, **cases.CAP_OPTS)
    want_U, want = fresh.solve(F, U0)
    fresh.close()
    assert want["cycles"] == 2 and not want["coarse_capped"] and want["history"][2] < want["history"][0]
    _same_as_restated(family, want_U, want, F, small, f"{family}: the small problem on a fresh solver")
    used = _solver(mg, family, **cases.CAP_OPTS)
    _, ni = used.solve(Fn, Un)
    assert ni["cycles"] == 2 and np.isnan(ni["history"][-1]) and not ni["converged"]
    _, ci = used.solve(Fc, Uc)
    assert ci["cycles"] == 2 and ci["coarse_capped"]
    got_U, got = used.solve(F, U0)
    used.close()
    assert_bits(got_U, want_U, f"{family}: clean solve after a NaN and a capped problem")
    assert got["history"] == want["history"] and got["cycles"] == 2 and got["coarse_capped"] == 0 and got["ref_norm"] == want["ref_norm"]
    assert np.all(np.isfinite(got_U)) and np.all(np.isfinite(got["history"])) and np.isfinite(got["ref_norm"])
    for key in SINGULAR_KEYS if family == "singular" else ():
        assert got[key] == want[key] and np.isfinite(got[key]), key
    assert mg.lib().mg_last_error() == 0


@pytest.mark.parametrize("e", [300, -300])
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_magnitudes_scale_exactly(mg, oracle, family, e):
    """powers of two scale every intermediate exactly and nothing over- or underflows (the largest square is about 2^630); the
    coefficient is not scaled"""
    F, U0 = cases.scale_problem()
    s = _solver(mg, family, **cases.SCALE_OPTS)
    base, bi = s.solve(F, U0)
    s.close()
    _same_as_restated(family, base, bi, F, _restated(mg, oracle, family, F, U0, **cases.SCALE_OPTS), f"{family}: unscaled")
    scale = 2.0 ** e
    s = _solver(mg, family, mean=cases.EDGE_MEAN * scale, **cases.SCALE_OPTS)
    got, gi = s.solve(F * scale, U0 * scale)
    s.close()
    assert np.all(np.isfinite(got)) and gi["cycles"] == 2 and not gi["coarse_capped"] and not bi["coarse_capped"]
    assert_bits(got, base * scale, f"{family}: U of the problem scaled by 2^{e}")
    assert gi["history"] == [h * scale for h in bi["history"]] and gi["ref_norm"] == bi["ref_norm"] * scale
    assert all(0.0 < h < float("inf") for h in gi["history"])
    for key in SINGULAR_KEYS if family == "singular" else ():
        assert gi[key] == bi[key] * scale and gi[key] != 0.0, key


def test_zero_source_of_the_singular_problem(mg):
    """F = 0, random start: ref_norm = 0, so only atol can stop it; the answer is the constant"""
    o = cases.ZERO_F
    a = cases.edge_coef()
    U0 = ref.random_problem(N, o["seed"])[1]
    s = _solver(mg, "singular", a, o["mean"], rtol=o["rtol"], atol=o["atol"])
    U, info = s.solve(np.zeros((N, N)), U0)
    s.close()
    err, bound, lam = cases.zero_source_error_and_bound(a, U, o["mean"])
    print(f"F = 0: {info['cycles']} cycles, max|U - mean| {float(err):.3e} <= {float(bound):.3e}, a_min*lambda+ {float(lam):.4f}")
    assert info["ref_norm"] == 0.0 and info["compat_defect"] == 0.0 and info["converged"] and info["cycles"] > 0
    assert err <= bound


@pytest.mark.parametrize("family", ["vc", "bc"])
def test_laplace_problem(mg, family):
    star, F, U0, lam_min = cases.laplace_problem(family)
    a = np.full((N, N), cases.LAPLACE_COEF)
    s = _solver(mg, family, a, rtol=0.0, atol=cases.LAPLACE_ATOL)
    U, info = s.solve(F, U0)
    s.close()
    assert info["ref_norm"] == 0.0 and info["cycles"] > 0 and not info["coarse_capped"]
    bc = cases.EDGE_KINDS[family]
    ex.check_mode_solve(U, info, star, F, 1.0, 0.0, bc, lam_min, f"Laplace {family}", cases.LAPLACE_COEF)
    m = bref.mask(N, bc)
    assert_bits(U[~m], U0[~m], "data points come back bit-identical")


def test_no_cycle_still_shifts_to_the_mean(mg, oracle):
    """step 3 of include/mg_singular.h runs also when no cycle ran: by max_cycles = 0, and by a start that already meets the
    tolerance -- the U of a finished solve put back in"""
    mean = cases.EDGE_MEAN
    F, U0 = cases.scale_problem()
    c_F = sref.weighted_mean(F)

    def check(U_in, U, info, converged, what):
        assert info["cycles"] == 0 and len(info["history"]) == 1 and info["converged"] == converged
        assert_bits(U, sref.project_mean(U_in, mean)[0], f"{what}: U is the start shifted to the target mean")
        assert info["compat_defect"] == c_F and info["mean_before"] == sref.weighted_mean(U_in) and info["mean"] == mean

    s = _solver(mg, "singular", max_cycles=0, rtol=1e-9)
    U, info = s.solve(F, U0)
    s.close()
    check(U0, U, info, False, "max_cycles = 0")
    s = _solver(mg, "singular", rtol=1e-9)
    U1, i1 = s.solve(F, U0)
    first = _restated(mg, oracle, "singular", F, U0, rtol=1e-9)
    tol = 1e-9 * bref.ref_norm(first[4]["Ft"], BC)
    cases.qualified_history(first[1], tol, "the solve that finishes")
    _same_as_restated("singular", U1, i1, F, first, "the solve that finishes")
    assert i1["converged"] and i1["cycles"] > 0
    cases.qualified_history(_restated(mg, oracle, "singular", F, U1, rtol=1e-9)[1], tol, "the finished solve put back in")
    U2, i2 = s.solve(F, U1)
    s.close()
    check(U1, U2, i2, True, "the finished solve put back in")
