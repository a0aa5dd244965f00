"""Restatement of the residual-tolerance solver with the `shift` option (include/mg_hip.h: Laplace(U) - sigma*U = F),
written from the header's semantics on numpy and the oracle's transfer operators.  It generalises _solve_ref.cycle,
solve, rbgs_trace and coarse_margin with the per-level constants

    dx2 = (L/(N-1))^2,  inv = 1/dx2,  d = 4 + shift*dx2,  q = 1/d,  c = omega*q      (each operation rounded once)

which are 4, 0.25 and 0.25*omega at shift = 0: there every function below is the one of _solve_ref bit for bit.
The second half holds the references in np.longdouble that share no code with the engine: the direct solution of the
screened system, its residual norm formed from sigma, L, N, U and F alone, and the a-priori bound on the fp64 evaluation
of that norm.  TEST INFRASTRUCTURE."""
import numpy as np

import _solve_ref as ref

LD = ref.LD
U53 = ref.U53
QUALIFY = ref.QUALIFY
DEFAULTS = dict(ref.DEFAULTS, coarse_max_iters=10000, shift=0.0)


def level_consts(N, L, shift, omega):
    """(dx2, inv, d, q, c) of one level: Python floats, one rounding per operation, in the header's order."""
    dx = L / float(N - 1)
    dx2 = dx * dx
    inv = 1.0 / dx2
    d = 4.0 + shift * dx2
    q = 1.0 / d
    c = omega * q
    return dx2, inv, d, q, c


def bracket(U, d):
    """b(U) = (((U[r+1] + U[r-1]) + U[c+1]) + U[c-1]) - d*U on the interior; the product is rounded, then subtracted."""
    return U[2:, 1:-1] + U[:-2, 1:-1] + U[1:-1, 2:] + U[1:-1, :-2] - d * U[1:-1, 1:-1]


def weighted_sweeps(N, L, U, F, omega, steps, shift=0.0):
    """`steps` sweeps U <- U + c*(b(U) - dx2*F) on a copy of U (rim kept)."""
    dx2, _, d, _, c = level_consts(N, L, shift, omega)
    U = np.array(U, dtype=np.float64, copy=True)
    Fi = F[1:-1, 1:-1]
    for _ in range(steps):
        P = U.copy()
        t = bracket(P, d) - dx2 * Fi
        U[1:-1, 1:-1] = P[1:-1, 1:-1] + c * t
    return U


def residual(N, L, U, F, shift=0.0):
    """D = inv*b(U) - F inside, 0 on the rim."""
    _, inv, d, _, _ = level_consts(N, L, shift, 1.0)
    D = np.zeros((N, N))
    D[1:-1, 1:-1] = inv * bracket(np.ascontiguousarray(U, dtype=np.float64), d) - F[1:-1, 1:-1]
    return D


def residual_norm(N, L, U, F, shift=0.0):
    D = residual(N, L, U, F, shift)
    return float(np.sqrt(np.sum(D[1:-1, 1:-1] ** 2)))


def rbgs_trace(N, L, F, atol, rtol, max_iters, shift=0.0):
    """_solve_ref.rbgs_trace with the update q*(left + right + down + up - h^2 F) and the error metric
    sum|inv*b(U) - F| / (N-2)^2.  Returns (U, err0, [err after every iteration])."""
    F = np.ascontiguousarray(F, dtype=np.float64)
    h2, inv, d, q, _ = level_consts(N, L, shift, 1.0)
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
            V = q * (U[1:-1, :-2] + U[1:-1, 2:] + U[2:, 1:-1] + U[:-2, 1:-1] - h2 * Fi)
            U[1:-1, 1:-1][m] = V[m]
        err = float(np.sum(np.abs(inv * bracket(U, d) - Fi))) / denom
        errs.append(err)
        if not (err > target) or len(errs) >= max_iters:
            break
    return U, err0, errs


def coarse_margin(N, L, F, atol, rtol, max_iters, shift=0.0, trace=None):
    """_solve_ref.coarse_margin on the shifted trace (trace: an rbgs_trace result to reuse)."""
    _, err0, errs = trace if trace is not None else rbgs_trace(N, L, F, atol, rtol, max_iters, shift)
    target = max(atol, rtol * err0)
    if target == 0.0:
        return float("inf") if errs[-1] == 0.0 else 0.0
    return min(abs(e - target) / target for e in errs[-2:])


def cycle(orc, F, U, L=1.0, margins=None, capped=None, **opts):
    """One V(pre, post) cycle of the screened equation.  margins receives coarse_margin() of the coarse solve, capped
    (a list) whether it ended at coarse_max_iters above its target."""
    o = dict(DEFAULTS, **opts)
    sh = float(o["shift"])
    sz = ref.sizes(F.shape[0], o["N_min"])
    nl = len(sz)
    Us, Fs = [None] * nl, [None] * nl
    Fs[0] = np.ascontiguousarray(F, dtype=np.float64)
    for l in range(nl - 1):
        N, M = sz[l], sz[l + 1]
        start = U if l == 0 else np.zeros((N, N))
        Us[l] = weighted_sweeps(N, L, start, Fs[l], o["omega"], o["pre"], sh)
        D = -residual(N, L, Us[l], Fs[l], sh)
        Fs[l + 1] = orc.doRestriction(N, D, M)
    Nc = sz[-1]
    tr = rbgs_trace(Nc, L, Fs[-1], o["coarse_atol"], o["coarse_rtol"], o["coarse_max_iters"], sh)
    Us[-1] = tr[0]
    if margins is not None:
        margins.append(coarse_margin(Nc, L, Fs[-1], o["coarse_atol"], o["coarse_rtol"], o["coarse_max_iters"], sh, trace=tr))
    if capped is not None:
        capped.append(tr[2][-1] > max(o["coarse_atol"], o["coarse_rtol"] * tr[1]))
    for l in range(nl - 2, -1, -1):
        tmp = orc.doProlongation(sz[l + 1], Us[l + 1], sz[l])
        U_l = orc.doGridAddition(sz[l], Us[l], tmp)
        Us[l] = weighted_sweeps(sz[l], L, U_l, Fs[l], o["omega"], o["post"], sh)
    return Us[0]


def solve(orc, F, U=None, L=1.0, margins=None, capped=None, **opts):
    """Returns (U, history, cycles, converged) under the stopping rule of mg_solver_solve."""
    o = dict(DEFAULTS, **opts)
    sh = float(o["shift"])
    N = F.shape[0]
    U = np.zeros((N, N)) if U is None else np.array(U, dtype=np.float64, copy=True)
    tol = max(o["rtol"] * ref.ref_norm(F), o["atol"])
    r = residual_norm(N, L, U, F, sh)
    history = [r]
    k = 0
    while not (r <= tol) and k < o["max_cycles"]:
        U = cycle(orc, F, U, L, margins=margins, capped=capped, **opts)
        r = residual_norm(N, L, U, F, sh)
        history.append(r)
        k += 1
    return U, history, k, r <= tol


# ---------------------------------------------------------------- references in np.longdouble
def lambda_11(N, L):
    """Eigenvalue of -Laplace_h for the mode sin(pi x) sin(pi y): (8/dx^2) sin^2(pi / (2(N-1))) (= lambda_min)."""
    return ref.lambda_min(N, L)


def direct_solution(F, U, L, shift):
    """The exact solution of inv*(star - 4U) - shift*U = F on the interior with U's rim as Dirichlet data, by fast
    diagonalisation: the eigenvalues of (-A + shift) are lam_i + lam_j + shift."""
    N = F.shape[0]
    n = N - 2
    inv = ref._inv_ld(N, L)
    X = np.array(U, dtype=LD)
    G = -np.array(F[1:-1, 1:-1], dtype=LD)            # (-A + shift) u = -F + inv * (rim neighbours)
    G[0, :] += inv * X[0, 1:-1]
    G[-1, :] += inv * X[-1, 1:-1]
    G[:, 0] += inv * X[1:-1, 0]
    G[:, -1] += inv * X[1:-1, -1]
    k = np.arange(1, n + 1)
    jk = np.outer(k, k) % (2 * (N - 1))
    S = np.sqrt(LD(2) / LD(N - 1)) * np.sin(ref._ld_pi() * jk.astype(LD) / LD(N - 1))
    lam = 4 * inv * np.sin(ref._ld_pi() * k.astype(LD) / LD(2 * (N - 1))) ** 2
    X[1:-1, 1:-1] = S @ ((S @ G @ S) / (lam[:, None] + lam[None, :] + LD(shift))) @ S
    return X


def _residual_ld(U, F, L, shift):
    N = F.shape[0]
    U = np.asarray(U, dtype=LD)
    F = np.asarray(F, dtype=LD)
    star = U[2:, 1:-1] + U[:-2, 1:-1] + U[1:-1, 2:] + U[1:-1, :-2]
    return ref._inv_ld(N, L) * (star - 4 * U[1:-1, 1:-1]) - LD(shift) * U[1:-1, 1:-1] - F[1:-1, 1:-1]


def residual_norm_ld(U, F, L, shift):
    """Interior L2 norm of Laplace_h(U) - shift*U - F, every operation in longdouble, from shift, L, N, U and F alone."""
    return np.sqrt(np.sum(_residual_ld(U, F, L, shift) ** 2))


def residual_rounding_bound(U, F, L, shift):
    """A-priori bound on |fp64 evaluation - residual_norm_ld|.  _solve_ref.residual_rounding_bound counts per point at
    most 8 roundings (five in the bracket, the product with inv, the difference, one to spare) of magnitude
    2^-53 * (inv*(|U_n| + |U_s| + |U_e| + |U_w| + 4|U_c|) + |F|).  Here the centre term is inv*d*|U_c| with
    d = 4 + shift*dx2 >= 4, which in exact arithmetic is (4*inv + shift)*|U_c| -- the magnitude of the two centre terms
    of the longdouble residual together -- and it carries THREE more roundings than the 4*U_c it replaces, whose product
    was exact: fl(shift*dx2), fl(4 + .) (the two that form d) and fl(d*U_c).  So: 8 on every term as before, 11 on the
    centre term; plus any summation order of the (N-2)^2 squares."""
    N = F.shape[0]
    A = np.abs(np.asarray(U, dtype=LD))
    inv = ref._inv_ld(N, L)
    d = LD(4) + LD(shift) / inv
    nbr = inv * (A[2:, 1:-1] + A[:-2, 1:-1] + A[1:-1, 2:] + A[1:-1, :-2]) + np.abs(np.asarray(F, dtype=LD)[1:-1, 1:-1])
    mag = 8 * nbr + 11 * inv * d * A[1:-1, 1:-1]
    return U53 * np.sqrt(np.sum(mag ** 2)) + LD((N - 2) * (N - 2)) * U53 * residual_norm_ld(U, F, L, shift)
