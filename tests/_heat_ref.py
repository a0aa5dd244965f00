"""Restatement of the theta-scheme time stepper (include/mg_heat.h) on numpy: the right-hand side in the header's evaluation
order, and a step as that right-hand side followed by the restated solve with shift = sigma started from U itself
(_solve_shift_ref.solve, or _solve_fmg_ref.solve when fmg >= 1).  TEST INFRASTRUCTURE."""
import numpy as np

import _solve_fmg_ref as fref
import _solve_shift_ref as sref


def consts(N, L, nu, dt, theta):
    """(sigma, beta, gamma, inv): Python floats, one rounding per operation, in the header's order."""
    nu, dt, theta = float(nu), float(dt), float(theta)
    a = theta * nu
    sigma = 1.0 / (a * dt)
    beta = (1.0 - theta) / theta
    gamma = 1.0 / a
    _, inv, _, _, _ = sref.level_consts(N, L, 0.0, 1.0)
    return sigma, beta, gamma, inv


def rhs(N, L, nu, dt, theta, U, Q=None):
    """F = -(sigma*u) [- beta*lap] [- gamma*q] inside, +0 on the rim; theta == 1 leaves the Laplacian term out."""
    sigma, beta, gamma, inv = consts(N, L, nu, dt, theta)
    U = np.ascontiguousarray(U, dtype=np.float64)
    u = U[1:-1, 1:-1]
    s = -(sigma * u)
    if float(theta) != 1.0:
        lap = inv * ((((U[2:, 1:-1] + U[:-2, 1:-1]) + U[1:-1, 2:]) + U[1:-1, :-2]) - 4 * u)
        s = s - beta * lap
    if Q is not None:
        s = s - gamma * np.asarray(Q, dtype=np.float64)[1:-1, 1:-1]
    F = np.zeros((N, N))
    F[1:-1, 1:-1] = s
    return F


def step(orc, U, Q=None, L=1.0, nu=1.0, dt=1.0, theta=1.0, margins=None, capped=None, **opts):
    """One time step.  Returns (U, history, cycles, converged) of its solve."""
    N = U.shape[0]
    sigma = consts(N, L, nu, dt, theta)[0]
    F = rhs(N, L, nu, dt, theta, U, Q)
    solve = fref.solve if int(opts.get("fmg", 0)) >= 1 else sref.solve
    return solve(orc, F, U, L, margins=margins, capped=capped, shift=sigma, **opts)


def run(orc, U, Q=None, steps=1, **kw):
    """`steps` steps in the stepper's rule: a step that ends not converged is the last.  Returns (U, cycles per step,
    converged)."""
    U = np.array(U, dtype=np.float64, copy=True)
    cycles, conv = [], True
    for _ in range(steps):
        U, _, k, conv = step(orc, U, Q, **kw)
        cycles.append(k)
        if not conv:
            break
    return U, cycles, bool(conv)
