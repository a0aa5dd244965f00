"""Restatement of the heat stepper with a variable coefficient (include/mg_heat_vc.h) on numpy: the right-hand side from
_heat_ref.consts and _solve_vc_ref.apply_operator at shift 0, a step as that right-hand side followed by the restated
variable-coefficient solve with shift = sigma started from U itself (_solve_vc_ref.solve).  The second half holds what the CPU
and the GPU module assert against truth, shared so that both use the same bounds: one step against a dense direct solve, and
the decay of a perturbation of a steady state.  TEST INFRASTRUCTURE."""
import numpy as np

import _exact as ex
import _heat_ref as href
import _solve_ref as ref
import _solve_vc_ref as vref

LD = ref.LD
U53 = ref.U53


def rhs(N, L, nu, dt, theta, a, U, Q=None):
    """F = -(sigma*u) [- beta*(inv*b(u))] [- gamma*q] inside, +0 on the rim; theta == 1 leaves the operator term out (and a
    unread); a = None: a = 1."""
    sigma, beta, gamma, _ = href.consts(N, L, nu, dt, theta)
    U = np.ascontiguousarray(U, dtype=np.float64)
    s = -(sigma * U[1:-1, 1:-1])
    if float(theta) != 1.0:
        s = s - beta * vref.apply_operator(N, L, a, U, 0.0)[1:-1, 1:-1]
    if Q is not None:
        s = s - gamma * np.asarray(Q, dtype=np.float64)[1:-1, 1:-1]
    F = np.zeros((N, N))
    F[1:-1, 1:-1] = s
    return F


def step(orc, a, U, Q=None, L=1.0, nu=1.0, dt=1.0, theta=1.0, margins=None, capped=None, table=None, **opts):
    """One time step.  Returns (U, history, cycles, converged) of its solve."""
    N = U.shape[0]
    sigma = href.consts(N, L, nu, dt, theta)[0]
    F = rhs(N, L, nu, dt, theta, a, U, Q)
    return vref.solve(orc, a, F, U, L, margins=margins, capped=capped, table=table, shift=sigma, **opts)


def run(orc, a, U, Q=None, steps=1, **kw):
    """`steps` steps in the stepper's rule: a step that ends not converged is the last.  Returns (U, cycles per step,
    converged)."""
    U = np.array(U, dtype=np.float64, copy=True)
    cycles, conv = [], True
    for _ in range(steps):
        U, _, k, conv = step(orc, a, U, Q, **kw)
        cycles.append(k)
        if not conv:
            break
    return U, cycles, bool(conv)


# ---------------------------------------------------------------- references in np.longdouble
def rhs_ld(N, L, nu, dt, theta, a, U, Q=None):
    """The right-hand side in longdouble from the fp64 inputs: constants from the equation (_exact.heat_consts), the operator
    in flux form (_solve_vc_ref._residual_ld)."""
    sg, be, ga = ex.heat_consts(nu, dt, theta)
    Au = vref._residual_ld(a, U, np.zeros((N, N)), L, 0.0)
    F = np.zeros((N, N), dtype=LD)
    F[1:-1, 1:-1] = -sg * np.asarray(U, dtype=LD)[1:-1, 1:-1] - be * Au
    if Q is not None:
        F[1:-1, 1:-1] -= ga * np.asarray(Q, dtype=LD)[1:-1, 1:-1]
    return F


def rhs_rounding_bound(N, L, nu, dt, theta, a, U, Q=None):
    """eps = 16 * 2^-53 * || sigma|u| + beta*inv*a_max*(sum|u_nb| + 4|u|) + gamma|q| ||_2: 16 roundings on the magnitude of every
    term of the right-hand side (the kernel's constants take 3, a face 2, the bracket and what follows at most 8)."""
    sg, be, ga = ex.heat_consts(nu, dt, theta)
    inv, amax = ref._inv_ld(N, L), LD(float(np.max(a)))
    A = np.abs(np.asarray(U, dtype=LD))
    mag = sg * A[1:-1, 1:-1] + be * inv * amax * (A[2:, 1:-1] + A[:-2, 1:-1] + A[1:-1, 2:] + A[1:-1, :-2] + 4 * A[1:-1, 1:-1])
    if Q is not None:
        mag = mag + ga * np.abs(np.asarray(Q, dtype=LD))[1:-1, 1:-1]
    return 16 * U53 * np.sqrt(np.sum(mag ** 2))


def smallest_eigenvalue(a, N, L, sigma):
    """sigma + a_min*lambda_min(-Laplace_h): a lower bound of the smallest eigenvalue of sigma - A_h, A_h >= a_min*(-Laplace_h)
    being symmetric."""
    return LD(sigma) + LD(float(np.min(a))) * ref.lambda_min(N, L)


# ---------------------------------------------------------------- truth: one step against a dense direct solve
ONE_STEP_RTOL = 1e-10


def one_step_problem(N, name, seed):
    """(a, U0 random rim included, Q random) on L = 1"""
    rng = np.random.default_rng(seed)
    return vref.field(name, N, 1.0, seed=3), rng.standard_normal((N, N)), rng.standard_normal((N, N))


def check_one_step(a, U0, Q, U, F, L, nu, dt, theta, rtol, what):
    """U: the field after one step from U0 whose solve stopped at rtol; F: the right-hand side that step used.  With F* the
    right-hand side in longdouble and X the dense direct solution of A_h X - sigma X = F* on U0's rim:
        ||F - F*|| <= eps
        ||U - X||  <= (rtol*||F|| + R + eps + r(X)) / (sigma + a_min*lambda_min)
    (the solve leaves a residual of at most rtol*||F|| as fp64 evaluates it, R = _solve_vc_ref.residual_rounding_bound off the
    longdouble one; F is eps off F*; r(X) is the longdouble residual of X), and the teeth condition
    bound <= 1e-6*||U - U0||: a wrong constant, sign or face moves the field differently by a fraction of what the step moved
    it.  R takes magnitudes of U, nothing else in the bound comes from the run."""
    N = U0.shape[0]
    sigma = href.consts(N, L, nu, dt, theta)[0]
    Fs = rhs_ld(N, L, nu, dt, theta, a, U0, Q)
    eps = rhs_rounding_bound(N, L, nu, dt, theta, a, U0, Q)
    dF = ref.norm_ld(np.asarray(F, dtype=LD) - Fs)
    X = vref.direct_solution(a, Fs, U0, L, sigma)
    rX = vref.residual_norm_ld(a, X, Fs, L, sigma)
    R = vref.residual_rounding_bound(a, U, F, L, sigma)
    err = ref.norm_ld(np.asarray(U, dtype=LD) - X)
    bound = (LD(rtol) * ref.norm_ld(F) + R + eps + rX) / smallest_eigenvalue(a, N, L, sigma)
    moved = ref.norm_ld(np.asarray(U, dtype=LD) - np.asarray(U0, dtype=LD))
    print(f"{what}: |F - F*|/eps {float(dF / eps):.2e}, error {float(err):.3e} bound {float(bound):.3e} "
          f"(error/bound {float(err / bound):.2f}), bound/moved {float(bound / moved):.1e}")
    assert dF <= eps, f"{what}: ||F - F*|| = {float(dF):.6e} above its rounding {float(eps):.6e}"
    assert bound <= LD(1e-6) * moved, f"{what}: no teeth: bound {float(bound):.3e}, field moved by {float(moved):.3e}"
    assert err <= bound, f"{what}: ||U - X|| = {float(err):.6e} above the bound {float(bound):.6e}"
    return float(err), float(bound)


# ---------------------------------------------------------------- truth: a perturbed steady state
STEADY = dict(L=2.5, nu=0.3, theta=1.0, steps=4, rtol=1e-10)


class Steady:
    """a, P, F_P = _exact.vc_polynomial(N, 2.5, 0): a linear, P quadratic, and the discrete operator is exact on P, A_h P = F_P.
    With Q = -nu*F_P the field P is a steady state of u_t = nu*div(a grad u) + q on its own rim.  Backward Euler from
    u_0 = P + 0.8*(m_11 + m_32/2) (discrete sine modes, zero rim): the error e_n = u_n - P obeys (sigma - A_h) e_n = sigma e_{n-1},
    and -A_h >= a_min*(-Laplace_h) gives ||e_n|| <= rho*||e_{n-1}||, rho = sigma/(sigma + a_min*lambda_min).  dt is chosen for
    rho = 1/2: dt = 1/(nu*a_min*lambda_min)."""

    def __init__(self, N):
        self.N, self.L, self.nu, self.theta = N, STEADY["L"], STEADY["nu"], STEADY["theta"]
        self.a, P, self.FP, self.a_min = ex.vc_polynomial(N, self.L, 0.0)
        self.X = ex.r64(P)      # compared as the fp64 array P rounds to: U carries exactly this rim
        self.Q = ex.r64(-LD(self.nu) * np.asarray(self.FP, dtype=LD))
        self.lam = ref.lambda_min(N, self.L)
        self.dt = float(1.0 / (LD(self.nu) * self.a_min * self.lam))
        self.sigma = href.consts(N, self.L, self.nu, self.dt, self.theta)[0]
        self.rho = LD(self.sigma) / (LD(self.sigma) + self.a_min * self.lam)
        m = ex.sine_mode(N, 1, 1) + LD(0.5) * ex.sine_mode(N, 3, 2)
        self.U0 = ex.r64(P + LD(0.8) * m)
        # what is left of A_h P = F_P after a, P and F_P were rounded to fp64, measured in longdouble on the reference alone,
        # and the distance of gamma*Q from -F_P (Q rounded once, gamma = 1/nu exact in longdouble)
        self.rX = vref.residual_norm_ld(self.a, self.X, self.FP, self.L, 0.0) + 2 * U53 * ref.norm_ld(self.FP)

    def error(self, U):
        return ref.norm_ld((np.asarray(U, dtype=LD) - self.X.astype(LD))[1:-1, 1:-1])

    def solve_term(self, U_prev, U, F, rtol):
        """(rtol*||F|| + R + eps + r(X)) / (sigma + a_min*lambda_min) of one step: the terms of check_one_step"""
        R = vref.residual_rounding_bound(self.a, U, F, self.L, self.sigma)
        eps = rhs_rounding_bound(self.N, self.L, self.nu, self.dt, self.theta, self.a, U_prev, self.Q)
        return (LD(rtol) * ref.norm_ld(F) + R + eps + self.rX) / (LD(self.sigma) + self.a_min * self.lam)


def check_steady(p, Us, Fs, rtol, what):
    """Us = [U_0, U_1, ..., U_n], Fs[k] the right-hand side step k + 1 used: ||U_n - P|| <= rho^n*||e_0|| + the solve terms of
    the n steps, on the interior, for every n."""
    e0 = p.error(Us[0])
    assert abs(p.rho - LD(0.5)) <= LD(1e-12) and e0 > 0
    terms = LD(0)
    for n in range(1, len(Us)):
        terms = terms + p.solve_term(Us[n - 1], Us[n], Fs[n - 1], rtol)
        err, bound = p.error(Us[n]), p.rho ** n * e0 + terms
        print(f"{what} step {n}: error/e0 {float(err / e0):.4f} rho^n {float(p.rho ** n):.4f}, solve terms {float(terms):.2e}")
        assert terms <= LD(1e-6) * p.rho ** n * e0, f"{what} step {n}: the solve terms {float(terms):.3e} hide the decay"
        assert err <= bound, f"{what} step {n}: ||U_n - P|| = {float(err):.6e} above {float(bound):.6e}"
        for edge in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
            assert np.array_equal(Us[n][edge].view(np.uint64), p.X[edge].view(np.uint64)), f"{what} step {n}: the rim moved"
