"""Restatement of the residual-tolerance solver (include/mg_hip.h, mg_solver_*) on the CPU oracle's operators.

One cycle is the reference driver's V(pre, post) node order (src/MG_solver_CPU.cpp:259-416) from the caller's U: the
finest level keeps its guess, coarser levels start from zero.  The smoother is the weighted Jacobi sweep U + c*t,
c = 0.25*omega, with t the reference's bracket in the reference's order (orc_doSmoothing / star_minus4), product and sum
rounded separately (numpy never fuses them).  The coarsest level is orc_doExactSolver (red-black Gauss-Seidel from zero)
with the target max(coarse_atol, coarse_rtol*err0) computed here, err0 = sum_interior|F| / (N-2)^2.  Residual,
restriction, prolongation and addition are the oracle's operators.  TEST INFRASTRUCTURE."""
import numpy as np

DEFAULTS = dict(pre=3, post=3, N_min=8, omega=0.8, coarse_rtol=1e-2, coarse_atol=0.0, rtol=1e-10, atol=0.0, max_cycles=50)


def sizes(N, N_min):
    out, n = [], N
    while n >= N_min:
        out.append(n)
        n //= 2
    return out


def weighted_sweeps(N, L, U, F, omega, steps):
    """`steps` weighted Jacobi sweeps on a copy of U (rim kept)."""
    dx = L / float(N - 1)
    dx2 = dx * dx
    c = 0.25 * omega
    U = np.array(U, dtype=np.float64, copy=True)
    Fi = F[1:-1, 1:-1]
    for _ in range(steps):
        P = U.copy()
        t = P[2:, 1:-1] + P[:-2, 1:-1] + P[1:-1, 2:] + P[1:-1, :-2] - 4 * P[1:-1, 1:-1]
        t = t - dx2 * Fi
        U[1:-1, 1:-1] = P[1:-1, 1:-1] + c * t
    return U


def coarse_target(F, atol, rtol):
    N = F.shape[0]
    err0 = float(np.sum(np.abs(F[1:-1, 1:-1]))) / float((N - 2) * (N - 2))
    return max(atol, rtol * err0)


def residual_norm(orc, N, L, U, F):
    D = orc.getResidual(N, L, U, F)
    return float(np.sqrt(np.sum(D[1:-1, 1:-1] ** 2)))


def ref_norm(F):
    return float(np.sqrt(np.sum(F[1:-1, 1:-1] ** 2)))


def cycle(orc, F, U, L=1.0, **opts):
    o = dict(DEFAULTS, **opts)
    sz = sizes(F.shape[0], o["N_min"])
    nl = len(sz)
    Us, Fs = [None] * nl, [None] * nl
    Fs[0] = np.ascontiguousarray(F, dtype=np.float64)
    for l in range(nl - 1):
        N, M = sz[l], sz[l + 1]
        start = U if l == 0 else np.zeros((N, N))
        Us[l] = weighted_sweeps(N, L, start, Fs[l], o["omega"], o["pre"])
        D = -orc.getResidual(N, L, Us[l], Fs[l])            # :268, :277-280
        Fs[l + 1] = orc.doRestriction(N, D, M)              # :287
    Nc = sz[-1]
    Us[-1] = orc.doExactSolver(Nc, L, Fs[-1], coarse_target(Fs[-1], o["coarse_atol"], o["coarse_rtol"]), 1)
    for l in range(nl - 2, -1, -1):
        tmp = orc.doProlongation(sz[l + 1], Us[l + 1], sz[l])   # :354
        U_l = orc.doGridAddition(sz[l], Us[l], tmp)              # :368
        Us[l] = weighted_sweeps(sz[l], L, U_l, Fs[l], o["omega"], o["post"])
    return Us[0]


def solve(orc, F, U=None, L=1.0, **opts):
    """Returns (U, history, cycles, converged) under the stopping rule of mg_solver_solve."""
    o = dict(DEFAULTS, **opts)
    N = F.shape[0]
    U = np.zeros((N, N)) if U is None else np.array(U, dtype=np.float64, copy=True)
    tol = max(o["rtol"] * ref_norm(F), o["atol"])
    r = residual_norm(orc, N, L, U, F)
    history = [r]
    k = 0
    while not (r <= tol) and k < o["max_cycles"]:
        U = cycle(orc, F, U, L, **opts)
        r = residual_norm(orc, N, L, U, F)
        history.append(r)
        k += 1
    return U, history, k, r <= tol


def vcycle_text(N, N_min, steps, tol, cycles=1, L=1.0):
    """A cycle file of `cycles` V-cycles chained in one node stream (fixed steps, halving sizes)."""
    levels = len(sizes(N, N_min))
    one = ["-1"] * (levels - 1) + ["0", f"{tol:.10f} 1"] + ["1"] * (levels - 1)
    return f"{L} 0.0 0.0\n{steps} 1\n{N} {N_min}\n" + "\n".join(one * cycles) + "\n2"


def write_vcycles(path, N, N_min, steps, tol, cycles=1, L=1.0):
    with open(path, "w") as f:
        f.write(vcycle_text(N, N_min, steps, tol, cycles, L))
    return path


def random_problem(N, seed):
    """Random F, random rim values, random interior guess."""
    rng = np.random.default_rng(seed)
    F = rng.random((N, N)) - 0.5
    U = rng.random((N, N)) - 0.5
    return F, U
