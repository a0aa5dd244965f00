"""Solves and heat steps with boundary kinds (include/mg_bc.h) on the device against exact DISCRETE modes: for a = 1 the
5-point operator with a mirrored ghost point beyond every Neumann side has closed-form eigenvectors for all 16 kinds
(tests/_exact.py: mixed_mode, mixed_mode_eigenvalue, lambda_min; held against the dense longdouble matrix by
tests/test_bc_forms_cpu.py).  The bit comparisons of tests/test_solve_bc_gpu.py and tests/test_bc_forms_gpu.py prove that the
kernels are the restatement; the dense direct solve stops at N = 33.  Here the truth is a formula, at the sizes whose top
level runs the column-pair form (514, 1026: an odd level below) and the non-temporal form (4096).

  solves   F = (c*lambda - sigma)*U*, homogeneous data, zero start, rtol 1e-10; c = 1, and c = 2 through coef = 2*ones (the
           faces of a constant power of two are exact, so the truth is the same mode with 2*lambda: the HAS_A forms under the
           same closed form).  max|U - U*| <= 2*(||r(U)|| + ||r(U*)||)/(lambda_min + sigma), both residuals in longdouble; the
           bound at most 1e-6*max|U*| (teeth); res within the a-priori rounding bound of ||r(U)||.
           The cases are tests/_bc_forms_cases.py's, which says how the modes and shifts were chosen on the restatement: the
           low mode (1, 2) at sigma 0 and 1e2 ((0, 1) for "nnnd" at sigma 0), the high mode (N/3, 2) at sigma 1e4.
  heat     u_0 = A*mode, no source: u_n = rho^n*u_0, rho = (sigma - beta*lambda)/(sigma + lambda) with lambda the eigenvalue of
           -c*Laplace_h.  _exact.Perturbed(steady=False, bc=...) with its a-priori bound in the w-norm (factor 2) and
           check_perturbed's two conditions.

Measured on the MI355X (46 solves, 14 steppers):
  solves   max|U - U*| / max|U*| between 4.5e-12 and 1.1e-10, the bound between 6.1e-9 and 3.2e-7 (the loosest: 1026, "dnnd",
           sigma 0, mode (1, 2)); at 4096 1.5e-11 <= 1.2e-7 and, with the coefficient, 2.2e-11 <= 1.7e-7.  The numpy
           restatement gives these digits too (tests/_bc_forms_cases.py lists its figures).
  heat     three steps: errors 1.2e-7 .. 9.7e-7 against bounds 3.3e-6 .. 1.3e-5, every bound 3e-8 .. 1.2e-7 of ||u_3 - u_0||; one
           step at 4096: 1.2e-6 against 1.9e-5 and 1.7e-5 (1e-7 and 5e-8 of the movement).
The cases at 4096 take 3.5 s (solves) and 5.4 s (heat) each, nearly all of it the host's longdouble arithmetic on 16.8
million points; everything else is below one second."""
import numpy as np
import pytest

import _bc_forms_cases as cases
import _bc_ref as bref
import _exact as ex
from conftest import assert_bits

pytestmark = pytest.mark.gpu


def _coef(N, coef):
    return None if coef is None else np.full((N, N), coef)


# ---------------------------------------------------------------- solves
@pytest.mark.parametrize("coef", cases.MODE_COEFS)
@pytest.mark.parametrize("N,L,bc,sigma,kl", cases.MODE_CASES)
def test_mode_solves(mg, N, L, bc, sigma, kl, coef):
    """the assertions of _exact.check_mode_solve; data points come back as they went in"""
    star, F, lam_min = cases.mode_problem(N, L, bc, sigma, kl, coef)
    U0 = np.zeros((N, N))
    U, info = mg.solve(F, U0, L, coef=_coef(N, coef), bc=bc, shift=sigma, rtol=cases.MODE_RTOL)
    ex.check_mode_solve(U, info, star, F, L, sigma, bc, lam_min, f"N={N} L={L} {bc} sigma={sigma:g} mode {kl} coef={coef}", coef)
    m = bref.mask(N, bc)
    assert_bits(U[~m], U0[~m], "data points come back bit-identical")


# ---------------------------------------------------------------- heat
def _steps(mg, p, N, bc, theta, coef, steps):
    hs = mg.HeatStepper(N, cases.HEAT["L"], cases.HEAT["nu"], cases.HEAT["dt"], theta, rtol=cases.HEAT["rtol"])
    try:
        if coef is not None:
            hs.set_coefficient(_coef(N, coef))
        hs.set_boundary(bc)
        assert abs(np.longdouble(hs.sigma) - p.sigma) <= 4 * ex.U53 * p.sigma
        U, infos = hs.step(p.U0, steps=steps)
    finally:
        hs.close()
    assert infos[0]["converged"] and infos[0]["steps"] == steps
    return U, infos[0]


@pytest.mark.parametrize("coef", cases.MODE_COEFS)
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("N,bc", cases.HEAT_CASES)
def test_heat_modes(mg, N, bc, theta, coef):
    """u_0 = 0.5*mode (2, 3), three steps in one call through HeatStepper.set_boundary: ||U_3 - u_3|| within the a-priori bound,
    and the bound below 1e-4 of ||u_3 - u_0||.  With the coefficient lambda doubles; sigma, beta, gamma do not change."""
    p = cases.heat_problem(N, bc, theta, coef)
    U, info = _steps(mg, p, N, bc, theta, coef, cases.HEAT_STEPS)
    ex.check_perturbed(p, U, cases.HEAT_STEPS, cases.HEAT["rtol"], f"N={N} {bc} theta={theta} coef={coef} cycles {info['cycles_per_step']}")
    m = bref.mask(N, bc)
    assert_bits(U[~m], p.U0[~m], "data points")


@pytest.mark.parametrize("coef", cases.MODE_COEFS)
def test_heat_mode_at_the_non_temporal_form(mg, coef):
    """one step at N = 4096, four insulated walls, theta = 1/2: k_bc<BC_HEAT, none | a, 2> inside the stepper"""
    N, bc, theta = 4096, "nnnn", 0.5
    p = cases.heat_problem(N, bc, theta, coef)
    U, info = _steps(mg, p, N, bc, theta, coef, 1)
    ex.check_perturbed(p, U, 1, cases.HEAT["rtol"], f"N={N} {bc} theta={theta} coef={coef} cycles {info['cycles_per_step']}")
