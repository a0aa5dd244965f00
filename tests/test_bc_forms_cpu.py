"""What tests/test_bc_forms_gpu.py and tests/test_bc_exact_gpu.py rest on, without a GPU: the closed-form modes of the mirrored
operator (tests/_exact.py: mixed_mode, mixed_mode_eigenvalue, lambda_min) against the dense longdouble matrix of
tests/_bc_ref.py, which shares no code with them; the matrix-free longdouble residual against the matrix; the truth
assertions of the GPU modules on the numpy restatement; and the qualification of every whole-solve seed."""
import numpy as np
import pytest

import _bc_forms_cases as cases
import _bc_ref as bref
import _exact as ex
import _solve_ref as ref
import _solve_vc_ref as vref

LD = np.longdouble
U53 = ref.U53


def _two_modes(N, bc):
    """one low and one high admissible (k, l), the lowest index of an axis included where it is 0"""
    (kW, kE), (kS, kN) = ex._axis_kinds(bc)
    (k0, k1), (l0, l1) = ex._axis_range(N, kW, kE), ex._axis_range(N, kS, kN)
    return [(k0, l0 + 1), (k1 - 1, l1)]


@pytest.mark.parametrize("bc", bref.ALL_KINDS)
@pytest.mark.parametrize("N", [9, 16])
def test_modes_are_eigenvectors_of_the_dense_operator(N, bc):
    """A m = lambda m over the unknowns to 64*2^-53*|lambda|*max|m| (the mode and lambda are longdouble, the matrix is
    longdouble: what is left is their own rounding, far below), data points exact zeros, and the Rayleigh quotient in the
    trapezoid weights is lambda."""
    L = 1.3
    A, unk = bref.dense_operator(None, N, L, 0.0, bc)
    w = bref.trapezoid_weights(N, bc).reshape(-1)[unk]
    for k, l in _two_modes(N, bc):
        m = ex.mixed_mode(N, bc, k, l)
        lam = ex.mixed_mode_eigenvalue(N, L, bc, k, l)
        assert not m[~bref.mask(N, bc)].any() and np.max(np.abs(m)) > 0.5
        x = m.reshape(-1)
        defect = np.max(np.abs(A @ x - lam * x[unk]))
        tol = 64 * U53 * abs(lam) * np.max(np.abs(m))
        print(f"N={N} {bc} ({k}, {l}): lambda {float(lam):.6e} defect {float(defect):.3e} <= {float(tol):.3e}")
        assert defect <= tol and lam <= 0
        xu = x[unk]
        assert abs(np.sum(w * xu * (A[:, unk] @ xu)) / np.sum(w * xu * xu) - lam) <= 64 * U53 * max(abs(lam), LD(1))


@pytest.mark.parametrize("bc", bref.ALL_KINDS)
@pytest.mark.parametrize("N", [9, 16])
def test_lambda_min_is_the_end_of_the_dense_spectrum(N, bc):
    """diag(w)*A is symmetric, so the spectrum of A is that of the symmetric W^1/2 A W^-1/2: numpy's eigvalsh in fp64, whose
    error is at most n*2^-53*||A|| (8*inv bounds the norm: Gershgorin)"""
    L = 1.3
    A, unk = bref.dense_operator(None, N, L, 0.0, bc)
    s = np.sqrt(bref.trapezoid_weights(N, bc).reshape(-1)[unk])
    S = (s[:, None] * A[:, unk] / s[None, :]).astype(np.float64)
    ev = np.linalg.eigvalsh(0.5 * (S + S.T))
    tol = float((unk.size + 8) * U53 * 8 * ref._inv_ld(N, L))
    lam_min = float(ex.lambda_min(N, L, bc))
    print(f"N={N} {bc}: lambda_min {lam_min:.12e}, dense {-ev[-1]:.12e}, tol {tol:.1e}")
    assert abs(-ev[-1] - lam_min) <= tol and ev[-1] <= tol
    assert (lam_min == 0.0) == (bc == "nnnn")
    # and every eigenvalue of the dense matrix is one of the closed form's
    (kW, kE), (kS, kN) = ex._axis_kinds(bc)
    (k0, k1), (l0, l1) = ex._axis_range(N, kW, kE), ex._axis_range(N, kS, kN)
    closed = sorted(float(ex.mixed_mode_eigenvalue(N, L, bc, k, l)) for k in range(k0, k1 + 1) for l in range(l0, l1 + 1))
    assert len(closed) == unk.size and np.max(np.abs(np.array(closed) - ev)) <= tol


def test_matrix_free_residual_is_the_matrix():
    """_bc_ref.residual_ld_stencil against _bc_ref.residual_ld, every kind, with a field, a constant and no coefficient"""
    N, L, shift = 12, 0.7, 3.0
    F, U = ref.random_problem(N, 5)
    eps = LD(np.finfo(LD).eps)
    for bc in bref.ALL_KINDS:
        for a in (vref.field("exp", N, L), None):
            want = bref.residual_ld(a, U, F, L, shift, bc)
            got = bref.residual_ld_stencil(a, U, F, L, shift, bc)
            assert got.shape == want.shape and np.max(np.abs(got - want)) <= 64 * eps * 8 * ref._inv_ld(N, L) * 2.8, bc
        two = bref.residual_ld_stencil(2.0, U, F, L, shift, bc)
        assert np.max(np.abs(two - bref.residual_ld(np.full((N, N), 2.0), U, F, L, shift, bc))) <= 64 * eps * 16 * ref._inv_ld(N, L)
        R = bref.residual_rounding_bound(None, U, F, L, shift, bc)
        assert R == bref.residual_rounding_bound(None, U, F, L, shift, bc, r=bref.residual_ld(None, U, F, L, shift, bc))


@pytest.mark.parametrize("coef", cases.MODE_COEFS)
@pytest.mark.parametrize("bc,sigma", [("nnnn", 1e2), ("dnnd", 0.0), ("nnnd", 1e2)])
def test_mode_solve_truth_on_the_restatement(bc, sigma, coef):
    """the assertion of test_bc_exact_gpu.py's solves, once on bref.solve at N = 65: error within the bound, bound with teeth"""
    N, L = 65, 2.5
    for kl in ((1, 2), (N // 3, 2)):
        star, F, lam_min = cases.mode_problem(N, L, bc, sigma, kl, coef)
        a = None if coef is None else np.full((N, N), coef)
        U, hist, cycles, conv = bref.solve(a, F, np.zeros((N, N)), bc, L, rtol=cases.MODE_RTOL, shift=sigma)
        assert conv
        ex.check_mode_solve(U, None, star, F, L, sigma, bc, lam_min, f"restatement N={N} {bc} sigma={sigma:g} {kl} coef={coef}, {cycles} cycles", coef)


def test_a_wrong_stencil_constant_leaves_the_bound():
    """teeth, shown: the solution of the system with inv off by one part in 10^5 has a longdouble residual that widens the
    a-posteriori bound to 6e-5*max|U*|, and the teeth line refuses it"""
    N, L, bc, sigma, kl = 65, 2.5, "nnnd", 1e2, (1, 2)
    star, F, lam_min = cases.mode_problem(N, L, bc, sigma, kl)
    lam = ex.mixed_mode_eigenvalue(N, L, bc, *kl)
    wrong = ex.r64(star * (lam - LD(sigma)) / (lam * (1 + LD(1e-5)) - LD(sigma)))       # solves it with inv*(1 + 1e-5)
    with pytest.raises(AssertionError, match="no teeth"):
        ex.check_mode_solve(wrong, None, star, F, L, sigma, bc, lam_min, "wrong inv")


@pytest.mark.parametrize("coef", cases.MODE_COEFS)
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_heat_mode_truth_on_the_restatement(theta, coef):
    """the heat assertion of test_bc_exact_gpu.py on the restatement at N = 65: three steps of {bref.heat_rhs, bref.solve}"""
    N, bc = 65, "ndnd"
    p = ex.Perturbed(N, cases.HEAT["L"], cases.HEAT["nu"], cases.HEAT["dt"], theta, *cases.HEAT["kl"], cases.HEAT["A"], steady=False,
                     bc=bc, coef=coef)
    a = None if coef is None else np.full((N, N), coef)
    U = p.U0
    for _ in range(cases.HEAT_STEPS):
        F = bref.heat_rhs(N, p.L, cases.HEAT["nu"], cases.HEAT["dt"], theta, bc, a, U)
        U, hist, cycles, conv = bref.solve(a, F, U, bc, p.L, rtol=cases.HEAT["rtol"], shift=float(p.sigma))
        assert conv
    ex.check_perturbed(p, U, cases.HEAT_STEPS, cases.HEAT["rtol"], f"restatement N={N} {bc} theta={theta} coef={coef}")
    # the generalisation left the Dirichlet problem as it was
    q = ex.Perturbed(N, 2.5, 0.5, 2e-2, theta, 2, 3, 0.5, steady=False)
    d = ex.Perturbed(N, 2.5, 0.5, 2e-2, theta, 2, 3, 0.5, steady=False, bc="dddd")
    assert q.lam_min == ref.lambda_min(N, 2.5) and abs(d.lam - q.lam) <= 8 * U53 * q.lam and abs(d.lam_min - q.lam_min) <= 8 * U53 * q.lam_min
    assert np.max(np.abs(d.Am - q.Am)) <= 8 * U53


@pytest.mark.parametrize("N,bc,shift,name,pp", cases.SOLVE_CASES)
def test_the_whole_solve_seeds_qualify_on_the_restatement_alone(N, bc, shift, name, pp):
    """every coarse solve of the two cycles has a margin >= 1e-10, and the hierarchy has the even level above an odd one"""
    sz = ref.sizes(N, 8)
    assert sz[0] % 2 == 0 and sz[0] >= 512 and sz[1] % 2 == 1 and (N != 1026 or sz[2] == 256), sz
    *_, hist, margins = cases.restated_cycles(N, bc, shift, name, pp)
    assert len(margins) == cases.CYCLES
    ref.assert_qualified(margins, f"N={N} {bc} shift={shift:g} a={name} {pp}")
    assert hist[2] < hist[1] < hist[0]


def test_the_case_tables_are_the_ones_asked_for():
    for N in (512, 514, 1026, 4096, 4098):
        mine = [c for c in cases.FORM_CASES if c[0] == N]
        kinds, ops = (cases.PAIR_KINDS, cases.PAIR_OPS) if N < 4096 else (cases.NT_KINDS, cases.NT_OPS)
        assert sorted((c[1], c[2]) for c in mine) == sorted((bc, op) for bc in kinds for op in ops)
        for key in (1, 2):      # every kind and every operation meets both shifts at every size
            for value in {c[key] for c in mine}:
                assert {c[4] for c in mine if c[key] == value} == {0.0, 1e4}, (N, value)
    assert [c[0] for c in cases.FORM_CASES] == sorted(c[0] for c in cases.FORM_CASES)      # one block per size
    assert len(cases.SOLVE_CASES) == 12 and {c[0] for c in cases.SOLVE_CASES} == {514, 1026}
    assert [c[4] for c in cases.SOLVE_CASES if c[0] == 1026] == [(3, 3)] * 4
    assert {c[4] for c in cases.SOLVE_CASES if c[0] == 514} == {(3, 3), (1, 2)}
