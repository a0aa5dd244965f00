"""The restatements of the variable-coefficient solve (tests/_solve_vc_ref.py) and of the heat stepper (tests/_heat_ref.py)
against exact solutions of the continuous equations (tests/_exact.py, np.longdouble), without a GPU.  The older tests hold
the device against these restatements and the restatements against the header; a convention shared by header, restatement and
kernel -- gamma = 1/(theta*nu), the sign of the Q term, beta, the arithmetic face mean -- passes all of them.  Here the
restatements meet fields that none of the three defines.  tests/test_exact_gpu.py asserts the same on the device.

  test                                    what a wrong convention does to it                     measured on the restatement
  vc polynomial is the discrete solution  a face mean that is not the midpoint value of a        residual / ||F|| <= 1.1e-13 at
  (17, 100, 513, 1026)                    linear a (harmonic, geometric) or a wrong sign of      all four sizes
                                          sigma leaves a residual of order ||F||
  vc polynomial through the restatement   the same, through a whole solve: the answer leaves     converges in 10 cycles;
  (129, L 2.5, sigma 0, rtol 1e-8)        the bound (r(U) + r(U*)) / (a_min*lambda_min + sigma)  |U - U*| 8.8e-9 <= 1.3e-7
  vc second order (33, 65, 129)           a face coefficient off by O(h), a first-order          errors 1.23876e-4, 3.09687e-5,
                                          scheme (ratio 2), a wrong a_x in nobody's F            7.74206e-6; ratios 4.00005, 4.00006
  heat perturbed steady state             gamma = 1/nu at theta = 1/2 drives P away from the     error 8.2e-6 .. 4.0e-5 (theta 1),
  (64, 129, 257) x theta (1, 1/2)         steady state; a flipped sign of Q or of beta does at   9.0e-7 .. 5.0e-6 (theta 1/2);
                                          both; each by a fraction of ||u_n - u_0||, four        bounds 2.4e-5 .. 1.0e-4,
                                          orders above the bound                                 3e-6 of ||u_n - u_0||
  heat moving rim, correct order          the same constants on a rim that moves and a source    relative error 3.6e-9 .. 1.1e-8
  (33, 129) x theta (1, 1/2), 3 steps     that is not -nu*Laplace(P)                             (33), 3.5e-11 .. 1.0e-9 (129)
  heat moving rim, naive loop, theta 1/2  pins the limitation include/mg_heat.h states: the      relative error after step 1
  (33, 129)                               rim set before a steps = 1 call puts two time levels   3.9e-7 (33), 2.4e-6 (129): 158x
                                          into Laplace_h(u_old)                                  and 6e4x the correct order's bound

Whoever gives the stepper a rim argument updates the last test."""
import functools

import numpy as np
import pytest

import _exact as ex
import _heat_ref as href
import _solve_ref as ref
import _solve_shift_ref as sref
import _solve_vc_ref as vref
from conftest import assert_bits

LD = np.longdouble


# ---------------------------------------------------------------- variable coefficient: the polynomial
@pytest.mark.parametrize("N,L,sigma", [(17, 1.0, 0.0), (100, 2.5, 1e2), (513, 0.3, 1e4), (1026, 7.0, 0.0)])
def test_vc_polynomial_is_the_discrete_solution(N, L, sigma):
    """The longdouble U leaves the longdouble flux-form residual at the level of the fp64 rounding of a and F (2^-53 = 1.1e-16
    relative, amplified by the cancellation in the differences), not at the level of a truncation error: below 1.1e-13 of
    ||F|| at every size, length and shift.  a_min is the smallest sample of a."""
    a, U, F, a_min = ex.vc_polynomial(N, L, sigma)
    r = vref.residual_norm_ld(a, U, F, L, sigma) / ref.norm_ld(F)
    print(f"N={N} L={L} sigma={sigma:g}: residual / ||F|| = {float(r):.3e}, a_min {float(a_min)}")
    assert r <= 1.1e-13
    assert float(a_min) == a.min() > 0


def test_vc_polynomial_through_the_restatement(oracle):
    N, L, sigma, rtol = 129, 2.5, 0.0, 1e-8
    a, U, F, a_min = ex.vc_polynomial(N, L, sigma)
    assert float(a_min) == 1.625
    got, hist, cycles, conv = vref.solve(oracle, a, F, ref.rim_only(ex.r64(U)), L, shift=sigma, rtol=rtol, max_cycles=60)
    assert conv, hist[-3:]
    ex.check_vc_truth(a, got, U, F, L, sigma, rtol, a_min, f"N={N} L={L} sigma={sigma:g}, {cycles} cycles")


# ---------------------------------------------------------------- variable coefficient: second order
@functools.lru_cache(maxsize=None)
def _smooth_error(oracle, N):
    a, U, F = ex.vc_smooth(N)
    got, hist, cycles, conv = vref.solve(oracle, a, F, ref.rim_only(ex.r64(U)), ex.VC_SMOOTH_L, shift=ex.VC_SMOOTH_SIGMA,
                                         rtol=1e-10, max_cycles=60)
    assert conv, hist[-3:]
    return float(ex.max_error(got, U))


def test_vc_second_order(oracle):
    """The interior max-norm error against the analytic U falls by 4 per halving of h: the limit of the ratio is 4 and the
    measured deviation 6e-5, so [3.95, 4.05] rejects a first-order scheme (2) and a face coefficient off by O(h).  At N = 129
    the error is 7.742e-6 to 1 % (the dense direct solve gives the same errors to 7 digits at 33 and 65: what is measured is
    the discretisation, not the stopping rule)."""
    e = {N: _smooth_error(oracle, N) for N in (33, 65, 129)}
    print("errors", e, "ratios", e[33] / e[65], e[65] / e[129])
    assert 3.95 <= e[33] / e[65] <= 4.05
    assert 3.95 <= e[65] / e[129] <= 4.05
    assert abs(e[129] - 7.742e-6) <= 0.01 * 7.742e-6


# ---------------------------------------------------------------- heat: the perturbed steady state
HEAT = dict(L=2.5, nu=0.5)


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("N", [64, 129, 257])
def test_heat_perturbed_steady_state(oracle, N, theta):
    """Non-zero constant rim, non-zero Q, four steps: ||U_4 - u_4|| within the a-priori bound of ex.Perturbed, and the bound
    below 1e-4 of what the four steps did to the field."""
    dt, steps, rtol = 2e-2, 4, 1e-8
    p = ex.Perturbed(N, HEAT["L"], HEAT["nu"], dt, theta, 2, 3, 0.5)
    U, cycles, conv = href.run(oracle, p.U0, p.Q, steps=steps, dt=dt, theta=theta, rtol=rtol, **HEAT)
    assert conv and len(cycles) == steps
    ex.check_perturbed(p, U, steps, rtol, f"N={N} theta={theta} cycles {cycles}")


# ---------------------------------------------------------------- heat: the moving rim
def _moving_rim(oracle, N, theta, naive):
    """Three steps; returns [(error, bound of this run's own step, U)] per step.  Correct order: right-hand side from the old
    field on its old rim, then the new rim, then the solve.  Naive: the new rim first, then a whole step."""
    L, nu, dt, rtol = HEAT["L"], HEAT["nu"], 2e-4, 1e-8
    m = ex.MovingRim(N, L, nu, dt, theta)
    sigma = href.consts(N, L, nu, dt, theta)[0]
    U, prev = ex.r64(m.exact(0)), m.start_bound()
    out = []
    for n in range(1, 4):
        new = ex.r64(m.exact(n))
        if naive:
            U = ex.with_rim(U, new)
            F = href.rhs(N, L, nu, dt, theta, U, m.Q)
        else:
            F = href.rhs(N, L, nu, dt, theta, U, m.Q)
            U = ex.with_rim(U, new)
        U, _, cycles, conv = sref.solve(oracle, F, U, L, shift=sigma, rtol=rtol)
        assert conv
        what = f"N={N} theta={theta} step {n} ({'naive' if naive else 'correct order'}, {cycles} cycles)"
        if naive:
            err, bound = ex.moving_rim_error_and_bound(U, m.exact(n), F, L, sigma)[:2]
        else:
            err, prev = ex.check_moving_rim_step(m, n, U, F, sigma, rtol, prev, what)
            bound = prev
        out.append((float(err), float(bound), U))
    return out


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("N", [33, 129])
def test_heat_moving_rim_in_the_correct_order(oracle, N, theta):
    _moving_rim(oracle, N, theta, naive=False)


@pytest.mark.parametrize("N", [33, 129])
def test_heat_moving_rim_naive_loop_is_exact_for_backward_euler(oracle, N):
    """theta = 1 reads no neighbour: rim first, then the step, gives the bits of the correct order."""
    for (_, _, good), (_, _, naive) in zip(_moving_rim(oracle, N, 1.0, False), _moving_rim(oracle, N, 1.0, True)):
        assert_bits(naive, good, f"N={N}")


@pytest.mark.parametrize("N", [33, 129])
def test_heat_moving_rim_naive_loop_is_not_the_theta_scheme(oracle, N):
    """theta = 1/2 with the new rim written before the step: Laplace_h(u_old) mixes two time levels next to the rim, and the
    answer misses the correct order's bound by more than 100x in every step (include/mg_heat.h, mg_heat_stepper_step, says
    so).  A stepper that takes the new rim as an argument makes this test fail: update it then."""
    good, naive = _moving_rim(oracle, N, 0.5, False), _moving_rim(oracle, N, 0.5, True)
    for n, ((_, bound, _), (err, _, _)) in enumerate(zip(good, naive), 1):
        print(f"N={N} step {n}: naive error {err:.3e}, correct order's bound {bound:.3e}, ratio {err / bound:.1f}")
        assert err > 100 * bound
