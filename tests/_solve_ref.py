"""Restatement of the residual-tolerance solver (include/mg_hip.h, mg_solver_*) on the CPU oracle's operators.

One cycle is the reference driver's V(pre, post) node order (src/MG_solver_CPU.cpp:259-416) from the caller's U: the
finest level keeps its guess, coarser levels start from zero.  The smoother is the weighted Jacobi sweep U + c*t,
c = 0.25*omega, with t the reference's bracket in the reference's order (orc_doSmoothing / star_minus4), product and sum
rounded separately (numpy never fuses them).  The coarsest level is orc_doExactSolver (red-black Gauss-Seidel from zero)
with the target max(coarse_atol, coarse_rtol*err0) computed here, err0 = sum_interior|F| / (N-2)^2.  Residual,
restriction, prolongation and addition are the oracle's operators.

The second half holds references that share no code with the engine or the oracle, all in np.longdouble: the direct
solution of the discrete system, the residual norm with an a-priori bound on its fp64 evaluation, polynomial problems
the 5-point stencil solves exactly, and a numpy trace of the coarse solve that qualifies an input for bit comparison
(DESIGN.md 4.3).  TEST INFRASTRUCTURE."""
import numpy as np

LD = np.longdouble
U53 = LD(2.0) ** -53          # unit roundoff of fp64
QUALIFY = 1e-10               # smallest relative distance of a coarse error from its target

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


def cycle(orc, F, U, L=1.0, margins=None, **opts):
    """One V(pre, post) cycle.  margins: a list that receives coarse_margin() of this cycle's coarse solve."""
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
    if margins is not None:
        margins.append(coarse_margin(Nc, L, Fs[-1], o["coarse_atol"], o["coarse_rtol"], 1 << 30))
    for l in range(nl - 2, -1, -1):
        tmp = orc.doProlongation(sz[l + 1], Us[l + 1], sz[l])   # :354
        U_l = orc.doGridAddition(sz[l], Us[l], tmp)              # :368
        Us[l] = weighted_sweeps(sz[l], L, U_l, Fs[l], o["omega"], o["post"])
    return Us[0]


def solve(orc, F, U=None, L=1.0, margins=None, **opts):
    """Returns (U, history, cycles, converged) under the stopping rule of mg_solver_solve."""
    o = dict(DEFAULTS, **opts)
    N = F.shape[0]
    U = np.zeros((N, N)) if U is None else np.array(U, dtype=np.float64, copy=True)
    tol = max(o["rtol"] * ref_norm(F), o["atol"])
    r = residual_norm(orc, N, L, U, F)
    history = [r]
    k = 0
    while not (r <= tol) and k < o["max_cycles"]:
        U = cycle(orc, F, U, L, margins=margins, **opts)
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


# ---------------------------------------------------------------- the coarse solve, iteration by iteration
def rbgs_trace(N, L, F, atol, rtol, max_iters):
    """The coarse solve as k_gs_relative states it: zero start, colour 0 = (row + col) even then colour 1, update
    0.25*(left + right + down + up - h^2 F), err = sum|inv*(star - 4U) - F| / (N-2)^2, at least one iteration, stop on
    !(err > max(atol, rtol*err0)) or at max_iters.  Returns (U, err0, [err after every iteration]).  Within one colour
    no point reads another of that colour, so the vectorised update is the sequential one."""
    F = np.ascontiguousarray(F, dtype=np.float64)
    h = L / float(N - 1)
    h2 = h * h
    inv = 1.0 / h2
    denom = float((N - 2) * (N - 2))
    Fi = F[1:-1, 1:-1]
    err0 = float(np.sum(np.abs(Fi))) / denom
    target = max(atol, rtol * err0)
    rr, cc = np.meshgrid(np.arange(1, N - 1), np.arange(1, N - 1), indexing="ij")
    masks = [((rr + cc) & 1) == colour for colour in (0, 1)]
    U = np.zeros((N, N))
    errs = []
    while True:
        for m in masks:
            V = 0.25 * (U[1:-1, :-2] + U[1:-1, 2:] + U[2:, 1:-1] + U[:-2, 1:-1] - h2 * Fi)
            U[1:-1, 1:-1][m] = V[m]
        t = U[2:, 1:-1] + U[:-2, 1:-1] + U[1:-1, 2:] + U[1:-1, :-2] - 4 * U[1:-1, 1:-1]
        err = float(np.sum(np.abs(inv * t - Fi))) / denom
        errs.append(err)
        if not (err > target) or len(errs) >= max_iters:
            break
    return U, err0, errs


def coarse_margin(N, L, F, atol, rtol, max_iters):
    """Smallest |err_k - target| / target over the stopping iteration and the one before it: how far the iteration
    count is from depending on the summation order of err.  inf when the target is met exactly at zero (F = 0)."""
    _, err0, errs = rbgs_trace(N, L, F, atol, rtol, max_iters)
    target = max(atol, rtol * err0)
    if target == 0.0:
        return float("inf") if errs[-1] == 0.0 else 0.0
    return min(abs(e - target) / target for e in errs[-2:])


def assert_qualified(margins, what=""):
    """The precondition of a bit comparison: an input whose coarse errors come within QUALIFY of the target is a badly
    chosen input (pick another seed), not a finding about the engine."""
    worst = min(margins) if margins else float("inf")
    if not worst >= QUALIFY:
        raise ValueError(f"{what}: input not qualified for bit comparison, coarse margin {worst:.3e} < {QUALIFY:g}")


# ---------------------------------------------------------------- references in np.longdouble
def _ld_pi():
    return LD(4) * np.arctan(LD(1))


def _inv_ld(N, L):
    return (LD(N - 1) / LD(L)) ** 2


def lambda_min(N, L):
    """Smallest eigenvalue of the discrete operator -A on the (N-2)^2 interior points: (8/dx^2) sin^2(pi / (2(N-1)))."""
    return 8 * _inv_ld(N, L) * np.sin(_ld_pi() / LD(2 * (N - 1))) ** 2


def direct_solution(F, U, L):
    """The exact solution of inv*(star - 4U) = F on the interior with U's rim as Dirichlet data, by fast
    diagonalisation: S_jk = sqrt(2/(N-1)) sin(pi j k / (N-1)), X = S((S G S) / (lam_i + lam_j))S.  Returns the N x N
    longdouble array (U's rim, the solution inside)."""
    N = F.shape[0]
    n = N - 2
    inv = _inv_ld(N, L)
    X = np.array(U, dtype=LD)
    G = -np.array(F[1:-1, 1:-1], dtype=LD)            # (-A) u = -F + inv * (rim neighbours)
    G[0, :] += inv * X[0, 1:-1]
    G[-1, :] += inv * X[-1, 1:-1]
    G[:, 0] += inv * X[1:-1, 0]
    G[:, -1] += inv * X[1:-1, -1]
    k = np.arange(1, n + 1)
    jk = np.outer(k, k) % (2 * (N - 1))                # the argument reduced in integers: sin has period 2(N-1) in j*k
    S = np.sqrt(LD(2) / LD(N - 1)) * np.sin(_ld_pi() * jk.astype(LD) / LD(N - 1))
    lam = 4 * inv * np.sin(_ld_pi() * k.astype(LD) / LD(2 * (N - 1))) ** 2
    X[1:-1, 1:-1] = S @ ((S @ G @ S) / (lam[:, None] + lam[None, :])) @ S
    return X


def _residual_ld(U, F, L):
    N = F.shape[0]
    U = np.asarray(U, dtype=LD)
    F = np.asarray(F, dtype=LD)
    star = U[2:, 1:-1] + U[:-2, 1:-1] + U[1:-1, 2:] + U[1:-1, :-2]
    return _inv_ld(N, L) * (star - 4 * U[1:-1, 1:-1]) - F[1:-1, 1:-1]


def norm_ld(A):
    """L2 norm over the interior of A, in longdouble."""
    A = np.asarray(A, dtype=LD)
    return np.sqrt(np.sum(A[1:-1, 1:-1] ** 2))


def residual_norm_ld(U, F, L):
    """Interior L2 norm of inv*(star - 4U) - F, every operation in longdouble, inv = ((N-1)/L)^2."""
    return np.sqrt(np.sum(_residual_ld(U, F, L) ** 2))


def residual_rounding_bound(U, F, L):
    """A-priori bound on |fp64 evaluation - residual_norm_ld|: per point at most 8 roundings (five in the bracket, the
    product, the difference, one to spare) of magnitude 2^-53 * (inv*(|U_n|+|U_s|+|U_e|+|U_w|+4|U_c|) + |F|), in the
    2-norm; plus any summation order of the (N-2)^2 squares."""
    N = F.shape[0]
    A = np.abs(np.asarray(U, dtype=LD))
    mag = _inv_ld(N, L) * (A[2:, 1:-1] + A[:-2, 1:-1] + A[1:-1, 2:] + A[1:-1, :-2] + 4 * A[1:-1, 1:-1])
    mag = mag + np.abs(np.asarray(F, dtype=LD)[1:-1, 1:-1])
    return 8 * U53 * np.sqrt(np.sum(mag ** 2)) + LD((N - 2) * (N - 2)) * U53 * residual_norm_ld(U, F, L)


CUBIC = {(0, 0): 0.5, (1, 0): 1.0, (0, 1): -2.0, (1, 1): 1.0, (3, 0): 1.0, (0, 3): -0.7, (2, 1): 0.3}
HARMONIC = {(0, 0): 1.0, (1, 0): 1.0, (0, 1): -2.0, (1, 1): 1.0, (2, 0): 1.0, (0, 2): -1.0}


def cubic_problem(N, L, x0, y0, coeffs):
    """U = sum coeffs[i, j] x^i y^j (i + j <= 3) on the grid x = x0 + col*dx, y = y0 + row*dx, and F its Laplacian.  The
    5-point stencil is exact on cubics, so U is the discrete solution for its own rim at every N.  Built in longdouble,
    each rounded once; returns (F, U) in fp64."""
    assert all(i >= 0 and j >= 0 and i + j <= 3 for i, j in coeffs)
    dx = LD(L) / LD(N - 1)
    x = (LD(x0) + np.arange(N).astype(LD) * dx)[None, :]
    y = (LD(y0) + np.arange(N).astype(LD) * dx)[:, None]
    U = np.zeros((N, N), dtype=LD)
    F = np.zeros((N, N), dtype=LD)
    for (i, j), a in coeffs.items():
        a = LD(a)
        U = U + a * x ** i * y ** j
        if i >= 2:
            F = F + a * (i * (i - 1)) * x ** (i - 2) * y ** j
        if j >= 2:
            F = F + a * (j * (j - 1)) * x ** i * y ** (j - 2)
    return F.astype(np.float64), U.astype(np.float64)


def rim_only(U):
    """U's rim around a zero interior."""
    out = np.array(U, dtype=np.float64, copy=True)
    out[1:-1, 1:-1] = 0.0
    return out
