"""What tests/test_singular_forms_gpu.py and tests/test_solve_edges_gpu.py rest on, without a GPU, on the numpy restatements
alone (tests/_singular_ref.py, _bc_ref.py, _solve_vc_ref.py): the qualification of every whole-solve seed, the
distance of every norm from a stopping tolerance where cycle counts are compared, the truth assertions of the mode solves with
their teeth, and the edges of data and state (a capped coarse solve, magnitudes 2^+-300, F = 0, no cycle) as the GPU module
states them."""
import numpy as np
import pytest

import _bc_ref as bref
import _exact as ex
import _singular_forms_cases as cases
import _singular_ref as sref
import _solve_ref as ref

LD = np.longdouble
BC = cases.BC


# ---------------------------------------------------------------- whole solves at the pair sizes
@pytest.mark.parametrize("N,name,pp", cases.SOLVE_CASES)
def test_the_whole_solve_seeds_qualify_on_the_restatement_alone(N, name, pp):
    """every coarse solve of the two cycles has a margin >= 1e-10 (restated_case asserts it), the hierarchy has the even level
    above an odd one, the data are not compatible and the shift to the target mean does something"""
    sz = ref.sizes(N, 8)
    assert sz[0] % 2 == 0 and sz[0] >= 512 and sz[1] % 2 == 1 and (N != 1026 or sz[2] == 256), sz
    assert sref.use_pairs(N) and not sref.use_pairs(sz[1])
    F, U0, a, U, hist, k, conv, info = cases.restated_case(N, name, pp)
    print(f"N={N} a={name} {pp}: margins {info['margins']}, history {hist}, compat_defect {info['compat_defect']!r}")
    assert k == cases.CYCLES == len(info["margins"]) and not conv and hist[2] < hist[1] < hist[0]
    assert min(info["margins"]) >= 1e-3                      # (far from the limit: 0.018 .. 0.044 when the seeds were chosen)
    assert abs(info["compat_defect"] - 0.125) < 1e-2 and abs(info["mean_before"] - cases.SOLVE_MEAN) > 1e-3
    m_ld = sref.weighted_mean_ld(U)
    assert abs(m_ld - LD(cases.SOLVE_MEAN)) <= sref.gamma(N * N) * sref.weighted_mean_ld(np.abs(U)) + 2 * ref.U53 * cases.SOLVE_MEAN


# ---------------------------------------------------------------- exact discrete modes
@pytest.mark.parametrize("N,L,kl,coef,d,mean,rtol,teeth", [c for c in cases.MODE_CASES if c[0] < 4096])
def test_mode_solve_truth_on_the_restatement(N, L, kl, coef, d, mean, rtol, teeth):
    """the assertions of test_singular_forms_gpu.test_mode_solves on sref.solve, at the sizes of the GPU cases (10 cycles take
    0.8 s at 514 and 3.3 s at 1026); no norm within 1e-9 of the tolerance"""
    star, F, lam_plus = cases.mode_problem(N, L, kl, coef, d)
    assert abs(sref.weighted_mean_ld(star)) <= 64 * np.finfo(LD).eps      # (zero but for longdouble's own rounding; measured: at most 2e-20)
    margins = []
    U, hist, cycles, conv, info = sref.solve(cases.mode_coef(N, coef), F, np.zeros((N, N)), mean, L, margins=margins, rtol=rtol)
    ref.assert_qualified(margins, f"N={N} {kl} coef={coef}")
    cases.qualified_history(hist, rtol * bref.ref_norm(info["Ft"], BC), f"N={N} {kl} coef={coef}")
    ex.check_singular_mode_solve(U, dict(info, converged=conv, cycles=cycles), star, F, L, d, mean, lam_plus,
                                 f"restatement N={N} L={L} mode {kl} coef={coef} d={d} mean={mean}", coef, teeth)


def test_the_mode_bound_at_4096_has_teeth_a_priori():
    """the case at 4096 is not repeated on the host (126 s); what its teeth rest on is arithmetic: a converged solve has
    ||r(U)|| <= rtol*||Ft||, and ||r(fp64(U*))|| = 4.0e-6 was measured"""
    N, L, kl, coef, d, mean, rtol, teeth = cases.MODE_CASES[-1]
    assert (N, rtol, teeth) == (4096, cases.MODE_RTOL_NT, cases.MODE_TEETH_NT)
    lam = float(-ex.mixed_mode_eigenvalue(N, L, BC, *kl))
    lam_plus = float(-ex.mixed_mode_eigenvalue(N, L, BC, 0, 1))
    norm_Ft = lam * N / 2.0                                  # (||U*||_2 is about N/2: cos^2 averages 1/2 on either axis)
    bound = 2 * (rtol * norm_Ft + 4.0e-6) / lam_plus
    print(f"4096: lambda {lam:.4f}, lambda+ {lam_plus:.4f}, tolerance {rtol * norm_Ft:.2e}, a-priori bound {bound:.2e}")
    assert abs(lam_plus - 1.579) < 1e-3 and abs(rtol * norm_Ft - 1.6e-5) < 1e-6 and bound <= 2.6e-5 <= teeth


@pytest.mark.parametrize("what", ["factor", "mean", "sign"])
def test_a_wrong_answer_leaves_the_mode_assertions(what):
    """teeth, shown at N = 65: a stencil constant off by one part in 10^5, an answer off by 1e-5 in its mean, and a final shift
    with the wrong sign are each refused"""
    N, L, kl, d, mean = 65, 2.5, (1, 2), 0.375, -1.5
    star, F, lam_plus = cases.mode_problem(N, L, kl, None, d)
    info = dict(compat_defect=sref.weighted_mean(F), converged=True, cycles=0)
    X = ex.r64(star) + mean
    ex.check_singular_mode_solve(X, info, star, F, L, d, mean, lam_plus, "the answer itself")
    wrong = {"factor": ex.r64(star / (1 + LD(1e-5))) + mean, "mean": X + 1e-5, "sign": ex.r64(star) - mean}[what]
    with pytest.raises(AssertionError, match="no teeth"):
        ex.check_singular_mode_solve(wrong, info, star, F, L, d, mean, lam_plus, f"wrong {what}")
    with pytest.raises(AssertionError, match="compat_defect"):
        ex.check_singular_mode_solve(X, dict(info, compat_defect=sref.weighted_mean(F - d)), star, F, L, d, mean, lam_plus, "F not projected")


# ---------------------------------------------------------------- edges of data and state, on the three restatements
def _restated(family, oracle, F, U0, mean=cases.EDGE_MEAN, **opts):
    return cases.edge_restated(family, cases.edge_coef(), F, U0, mean, orc=oracle, **opts)


@pytest.mark.parametrize("family", cases.FAMILIES)
def test_nan_in_F_on_the_restatement(family, oracle):
    """the coarse loop ends on not (err > target): one iteration per cycle, nothing capped, every norm NaN"""
    F, U0 = cases.nan_problem()
    with np.errstate(invalid="ignore"):
        U, hist, k, conv, info, margins, capped = _restated(family, oracle, F, U0, **cases.NAN_OPTS)
    assert k == 2 and not conv and len(hist) == 3 and all(np.isnan(h) for h in hist) and not any(capped)
    if family == "singular":
        assert np.isnan(info["compat_defect"])


@pytest.mark.parametrize("family", cases.FAMILIES)
def test_the_unit_problem_caps_and_the_small_one_does_not(family, oracle):
    Fc, Uc = cases.capped_problem()
    *_, capped = _restated(family, oracle, Fc, Uc, **cases.CAP_OPTS)
    assert len(capped) == 2 and all(capped), capped
    F, U0 = cases.small_problem()
    U, hist, k, conv, info, margins, capped = _restated(family, oracle, F, U0, **cases.CAP_OPTS)
    assert k == 2 and len(capped) == 2 and not any(capped) and hist[2] < hist[0] and np.all(np.isfinite(U))
    ref.assert_qualified(margins, f"{family}: the small problem")


@pytest.mark.parametrize("e", [300, -300])
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_magnitudes_scale_exactly_on_the_restatement(family, oracle, e):
    """F, U0 and the target mean scaled by 2^e, the coefficient not: U, the history, compat_defect and mean_before scale by
    2^e bit for bit, nothing caps, nothing over- or underflows"""
    F, U0 = cases.scale_problem()
    s = 2.0 ** e
    U, hist, k, conv, info, margins, capped = _restated(family, oracle, F, U0, **cases.SCALE_OPTS)
    ref.assert_qualified(margins, f"{family}: magnitudes")
    cases.qualified_history(hist, 0.0, f"{family}: magnitudes")
    Us, hs, ks, convs, infos, _, cappeds = _restated(family, oracle, F * s, U0 * s, cases.EDGE_MEAN * s, **cases.SCALE_OPTS)
    assert k == ks == 2 and not any(capped) and not any(cappeds)
    assert np.array_equal((U * s).view(np.uint64), Us.view(np.uint64)) and np.all(np.isfinite(Us))
    assert hs == [h * s for h in hist] and all(0.0 < h < float("inf") for h in hs)
    if family == "singular":
        assert infos["compat_defect"] == info["compat_defect"] * s and infos["mean_before"] == info["mean_before"] * s
        assert bref.ref_norm(infos["Ft"], BC) == bref.ref_norm(info["Ft"], BC) * s


def test_zero_source_on_the_singular_restatement():
    """F = 0, random start, atol = 1e-9, mean = -0.75: the answer is the constant; 15 cycles, max|U - mean| = 2.3e-13 when the
    case was chosen, a_min*lambda+ = 4.93"""
    o = cases.ZERO_F
    N, a = cases.EDGE_N, cases.edge_coef()
    U0 = ref.random_problem(N, o["seed"])[1]
    margins = []
    U, hist, k, conv, info = sref.solve(a, np.zeros((N, N)), U0, o["mean"], 1.0, margins=margins, rtol=o["rtol"], atol=o["atol"])
    cases.qualified_history(hist, o["atol"], "F = 0")
    assert conv and 0 < k <= 20 and info["compat_defect"] == 0.0 and bref.ref_norm(info["Ft"], BC) == 0.0
    err, bound, lam = cases.zero_source_error_and_bound(a, U, o["mean"])
    print(f"F = 0: {k} cycles, max|U - mean| {float(err):.3e} <= {float(bound):.3e}, a_min*lambda+ {float(lam):.4f}")
    assert err <= bound <= 1e-8 and abs(float(lam) - 4.93) < 0.01


@pytest.mark.parametrize("family", ["vc", "bc"])
def test_laplace_problem_on_the_restatement(family, oracle):
    """F = 0 with a = 2: the harmonic 1 + x^2 - y^2 is the discrete solution, for four Dirichlet sides and for "ndnd" """
    N = cases.EDGE_N
    star, F, U0, lam_min = cases.laplace_problem(family)
    bc = cases.EDGE_KINDS[family]
    r = bref.residual_ld_stencil(cases.LAPLACE_COEF, star, F, 1.0, 0.0, bc)
    assert np.max(np.abs(r)) <= 64 * float(np.finfo(LD).eps) * 8 * 4096 * 2.0     # (the stencil annihilates it)
    a = np.full((N, N), cases.LAPLACE_COEF)
    U, hist, k, conv, info, margins, capped = cases.edge_restated(family, a, F, U0, orc=oracle, rtol=0.0, atol=cases.LAPLACE_ATOL)
    cases.qualified_history(hist, cases.LAPLACE_ATOL, f"Laplace {family}")
    assert conv and k > 0 and not any(capped)
    ex.check_mode_solve(U, None, star, F, 1.0, 0.0, bc, lam_min, f"restatement, Laplace {family}, {k} cycles", cases.LAPLACE_COEF)


def test_no_cycle_on_the_singular_restatement():
    """max_cycles = 0, and a start that already meets the tolerance (the U of a finished solve): no cycle, U projected, F's
    defect still reported; the second start's norm is not within 1e-9 of the tolerance"""
    N, a, mean = cases.EDGE_N, cases.edge_coef(), cases.EDGE_MEAN
    F, U0 = cases.scale_problem()
    U, hist, k, conv, info = sref.solve(a, F, U0, mean, 1.0, max_cycles=0, rtol=1e-9)
    assert k == 0 and not conv and len(hist) == 1 and info["compat_defect"] == sref.weighted_mean(F)
    assert np.array_equal(U, sref.project_mean(U0, mean)[0]) and info["mean_before"] == sref.weighted_mean(U0)
    U1, hist1, k1, conv1, info1 = sref.solve(a, F, U0, mean, 1.0, rtol=1e-9)
    assert conv1 and k1 > 0
    U2, hist2, k2, conv2, info2 = sref.solve(a, F, U1, mean, 1.0, rtol=1e-9)
    cases.qualified_history(hist2, 1e-9 * bref.ref_norm(info2["Ft"], BC), "the finished solve put back in")
    assert k2 == 0 and conv2 and np.array_equal(U2, sref.project_mean(U1, mean)[0])
    assert info2["mean_before"] == sref.weighted_mean(U1) and info2["compat_defect"] == info1["compat_defect"]


def test_the_case_tables_are_the_ones_asked_for():
    assert sorted(cases.SOLVE_CASES, key=str) == sorted([(514, n, pp) for n in (None, "exp") for pp in ((3, 3), (1, 2))] +
                                                       [(1026, n, (3, 3)) for n in (None, "exp")], key=str)
    assert cases.SOLVE_SEED == {514: 5514, 1026: 6026} and cases.SOLVE_MEAN == 2.5 and cases.CYCLES == 2
    assert cases.COMPOSITION_CASES == [(33, 3), (514, 2), (1026, 2), (4096, 2)]
    modes = {(c[0], c[2], c[3]) for c in cases.MODE_CASES}
    assert modes == {(N, (1, 2), coef) for N in (514, 1026) for coef in (None, 2.0)} | {(514, (0, 1), None), (4096, (1, 2), None)}
    assert {(c[4], c[5]) for c in cases.MODE_CASES} == {(0.375, -1.5), (-0.25, 2.5), (0.0, 2.5)}
    assert all(c[5] != 0.0 and c[1] == cases.MODE_L[c[0]] for c in cases.MODE_CASES)
    assert all((c[6], c[7]) == ((1e-9, 1e-4) if c[0] == 4096 else (1e-10, 1e-6)) for c in cases.MODE_CASES)
    assert ref.sizes(cases.EDGE_N, 8) == [65, 32, 16, 8]
