"""Restatement of the residual-tolerance solver with a variable coefficient, div(a grad U) - sigma*U = F, written from
include/mg_varcoef.h on numpy and the oracle's transfer operators.  It generalises _solve_shift_ref (level constants, sweep,
residual, red-black trace with margins, cycle, solve) with the per-point face coefficients

    aN = 0.5*(a[p] + a[p+N]), aS = 0.5*(a[p] + a[p-N]), aE = 0.5*(a[p] + a[p+1]), aW = 0.5*(a[p] + a[p-1])
    d = (((aN + aS) + aE) + aW) + sd,  q = 1/d,  c = omega*q                        (each operation rounded once)

and adds the coarsening of the nodal coefficient.  With a == 1 every function below is the one of _solve_shift_ref bit for
bit (tests/test_solve_vc_cpu.py).  The second half holds the references that share no code with the engine: the residual in
np.longdouble formed from a, sigma, L, N, U and F alone, its a-priori rounding bound, and a dense direct solve for small N.
TEST INFRASTRUCTURE."""
import math

import numpy as np

import _solve_ref as ref
import _solve_shift_ref as sref

LD = ref.LD
U53 = ref.U53
QUALIFY = ref.QUALIFY
DEFAULTS = dict(sref.DEFAULTS)


def level_consts(N, L, shift):
    """(dx2, inv, sd) of one level: Python floats, one rounding per operation, in the header's order."""
    dx = L / float(N - 1)
    dx2 = dx * dx
    return dx2, 1.0 / dx2, shift * dx2


def faces(a, sd):
    """(aN, aS, aE, aW, d, q) on the interior of the nodal coefficient a; N / S are rows r+1 / r-1."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    ctr = a[1:-1, 1:-1]
    aN = 0.5 * (ctr + a[2:, 1:-1])
    aS = 0.5 * (ctr + a[:-2, 1:-1])
    aE = 0.5 * (ctr + a[1:-1, 2:])
    aW = 0.5 * (ctr + a[1:-1, :-2])
    d = (((aN + aS) + aE) + aW) + sd
    q = 1.0 / d
    return aN, aS, aE, aW, d, q


def bracket(fc, U):
    """b(U) = (((aN*U[r+1] + aS*U[r-1]) + aE*U[c+1]) + aW*U[c-1]) - d*U on the interior."""
    aN, aS, aE, aW, d, _ = fc
    return (((aN * U[2:, 1:-1] + aS * U[:-2, 1:-1]) + aE * U[1:-1, 2:]) + aW * U[1:-1, :-2]) - d * U[1:-1, 1:-1]


def weighted_sweeps(N, L, a, U, F, omega, steps, shift=0.0, zero_start=False):
    """`steps` sweeps U <- U + c*(b(U) - dx2*F) on a copy of U (rim kept).  zero_start: U is the zero field and the first
    sweep is 0.0 + c*(0.0 - dx2*F) (the same bits as the general expression on zeros, stated as the header states it)."""
    dx2, _, sd = level_consts(N, L, shift)
    fc = faces(a, sd)
    c = omega * fc[5]
    U = np.zeros((N, N)) if zero_start else np.array(U, dtype=np.float64, copy=True)
    Fi = np.ascontiguousarray(F, dtype=np.float64)[1:-1, 1:-1]
    for s in range(steps):
        if zero_start and s == 0:
            U[1:-1, 1:-1] = 0.0 + c * (0.0 - dx2 * Fi)
            continue
        P = U.copy()
        U[1:-1, 1:-1] = P[1:-1, 1:-1] + c * (bracket(fc, P) - dx2 * Fi)
    return U


def apply_operator(N, L, a, U, shift=0.0):
    """inv*b(U) inside, +0 on the rim; a = None: a = 1."""
    _, inv, sd = level_consts(N, L, shift)
    out = np.zeros((N, N))
    out[1:-1, 1:-1] = inv * bracket(faces(np.ones((N, N)) if a is None else a, sd), np.ascontiguousarray(U, dtype=np.float64))
    return out


def residual(N, L, a, U, F, shift=0.0, sign=1):
    """D = inv*b(U) - F inside, +0 on the rim; sign < 0: the whole array negated (-0 on the rim)."""
    _, inv, sd = level_consts(N, L, shift)
    D = np.zeros((N, N))
    D[1:-1, 1:-1] = inv * bracket(faces(a, sd), np.ascontiguousarray(U, dtype=np.float64)) - F[1:-1, 1:-1]
    return -D if sign < 0 else D


def residual_norm(N, L, a, U, F, shift=0.0):
    D = residual(N, L, a, U, F, shift)
    return float(np.sqrt(np.sum(D[1:-1, 1:-1] ** 2)))


def restriction_table(N, M):
    """mg_restriction_table's expressions (include/mg_hip.h): lo = floor(i*h_c/h_f), w = fmod(i*h_c, h_f)/h_f."""
    h_f, h_c = 1.0 / float(N - 1), 1.0 / float(M - 1)
    lo = np.array([int(math.floor(float(i) * h_c / h_f)) for i in range(M)], dtype=np.int64)
    w = np.array([math.fmod(float(i) * h_c, h_f) / h_f for i in range(M)], dtype=np.float64)
    return lo, w


def coarsen(a, M, table=None):
    """The nodal coefficient at the M x M coarse points, rim included: doRestriction's expression with the table's end entries
    replaced by (0, 0.0) and (N-2, 1.0), clamped into the range of its four samples."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    N = a.shape[0]
    lo, w = table if table is not None else restriction_table(N, M)
    lo = np.array(lo, dtype=np.int64)
    w = np.array(w, dtype=np.float64)
    lo[0], w[0] = 0, 0.0
    lo[M - 1], w[M - 1] = N - 2, 1.0
    wa, wc = w[None, :], w[:, None]          # a = w[col], c = w[row]
    wb, wd = 1.0 - wa, 1.0 - wc
    r, c = lo[:, None], lo[None, :]
    s0, s1, s2, s3 = a[r, c], a[r, c + 1], a[r + 1, c], a[r + 1, c + 1]
    v = wb * wd * s0 + wa * wd * s1 + wc * wb * s2 + wa * wc * s3
    mn = np.minimum(np.minimum(s0, s1), np.minimum(s2, s3))
    mx = np.maximum(np.maximum(s0, s1), np.maximum(s2, s3))
    return np.minimum(np.maximum(v, mn), mx)


def coarsen_levels(a, N_min, table=None):
    """[a_0, a_1, ...] over the solver's hierarchy; table(N, M) -> (lo, w) replaces the restatement's own table."""
    sz = ref.sizes(a.shape[0], N_min)
    out = [np.ascontiguousarray(a, dtype=np.float64)]
    for l in range(len(sz) - 1):
        out.append(coarsen(out[-1], sz[l + 1], table(sz[l], sz[l + 1]) if table else None))
    return out


def rbgs_trace(N, L, a, F, atol, rtol, max_iters, shift=0.0):
    """The coarse solve: zero start, colour 0 = (row + col) even then colour 1, update
    q*((((aW*U[c-1] + aE*U[c+1]) + aN*U[r+1]) + aS*U[r-1]) - h2*F), err = sum|inv*b(U) - F| / (N-2)^2 after every iteration.
    Returns (U, err0, [err after every iteration])."""
    F = np.ascontiguousarray(F, dtype=np.float64)
    h2, inv, sd = level_consts(N, L, shift)
    fc = faces(a, sd)
    aN, aS, aE, aW, _, q = fc
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
            V = q * ((((aW * U[1:-1, :-2] + aE * U[1:-1, 2:]) + aN * U[2:, 1:-1]) + aS * U[:-2, 1:-1]) - h2 * Fi)
            U[1:-1, 1:-1][m] = V[m]
        err = float(np.sum(np.abs(inv * bracket(fc, U) - Fi))) / denom
        errs.append(err)
        if not (err > target) or len(errs) >= max_iters:
            break
    return U, err0, errs


def coarse_margin(trace, atol, rtol):
    """_solve_ref.coarse_margin on an rbgs_trace result."""
    _, err0, errs = trace
    target = max(atol, rtol * err0)
    if target == 0.0:
        return float("inf") if errs[-1] == 0.0 else 0.0
    return min(abs(e - target) / target for e in errs[-2:])


def cycle(orc, levels, F, U, L=1.0, margins=None, capped=None, **opts):
    """One V(pre, post) cycle; levels = coarsen_levels(a, N_min)."""
    o = dict(DEFAULTS, **opts)
    sh = float(o["shift"])
    sz = ref.sizes(F.shape[0], o["N_min"])
    nl = len(sz)
    assert [A.shape[0] for A in levels] == sz
    Us, Fs = [None] * nl, [None] * nl
    Fs[0] = np.ascontiguousarray(F, dtype=np.float64)
    for l in range(nl - 1):
        N, M = sz[l], sz[l + 1]
        Us[l] = weighted_sweeps(N, L, levels[l], U if l == 0 else None, Fs[l], o["omega"], o["pre"], sh, zero_start=l > 0)
        D = residual(N, L, levels[l], Us[l], Fs[l], sh, sign=-1)
        Fs[l + 1] = orc.doRestriction(N, D, M)
    Nc = sz[-1]
    tr = rbgs_trace(Nc, L, levels[-1], Fs[-1], o["coarse_atol"], o["coarse_rtol"], o["coarse_max_iters"], sh)
    Us[-1] = tr[0]
    if margins is not None:
        margins.append(coarse_margin(tr, o["coarse_atol"], o["coarse_rtol"]))
    if capped is not None:
        capped.append(tr[2][-1] > max(o["coarse_atol"], o["coarse_rtol"] * tr[1]))
    for l in range(nl - 2, -1, -1):
        tmp = orc.doProlongation(sz[l + 1], Us[l + 1], sz[l])
        U_l = orc.doGridAddition(sz[l], Us[l], tmp)
        Us[l] = weighted_sweeps(sz[l], L, levels[l], U_l, Fs[l], o["omega"], o["post"], sh)
    return Us[0]


def solve(orc, a, F, U=None, L=1.0, margins=None, capped=None, table=None, **opts):
    """Returns (U, history, cycles, converged) under the stopping rule of mg_solver_solve."""
    o = dict(DEFAULTS, **opts)
    sh = float(o["shift"])
    N = F.shape[0]
    levels = coarsen_levels(a, o["N_min"], table)
    U = np.zeros((N, N)) if U is None else np.array(U, dtype=np.float64, copy=True)
    tol = max(o["rtol"] * ref.ref_norm(F), o["atol"])
    r = residual_norm(N, L, a, U, F, sh)
    history = [r]
    k = 0
    while not (r <= tol) and k < o["max_cycles"]:
        U = cycle(orc, levels, F, U, L, margins=margins, capped=capped, **opts)
        r = residual_norm(N, L, a, U, F, sh)
        history.append(r)
        k += 1
    return U, history, k, r <= tol


# ---------------------------------------------------------------- the fields of the tests
def grid(N, L=1.0):
    x = np.arange(N) * (L / float(N - 1))
    return x[None, :], x[:, None]       # x along columns, y along rows


def field(name, N, L=1.0, seed=0):
    x, y = grid(N, L)
    if name == "one":
        return np.ones((N, N))
    if name == "smooth":
        return 1.0 + 0.5 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y)
    if name == "exp":
        return np.exp(2.0 * np.sin(3.0 * x + y))                     # contrast 33.6 on the unit square
    if name == "jump":
        return np.where(x < 0.37, 1.0, 10.0) + 0.0 * y                # a 10x jump across the line x = 0.37
    if name == "random":
        return 10.0 ** (3.0 * np.random.default_rng(seed).random((N, N)))   # positive, contrast 1e3
    raise ValueError(name)


# ---------------------------------------------------------------- references in np.longdouble
def _faces_ld(a):
    a = np.asarray(a, dtype=LD)
    ctr = a[1:-1, 1:-1]
    h = LD(1) / LD(2)
    return h * (ctr + a[2:, 1:-1]), h * (ctr + a[:-2, 1:-1]), h * (ctr + a[1:-1, 2:]), h * (ctr + a[1:-1, :-2])


def _residual_ld(a, U, F, L, shift):
    N = F.shape[0]
    U = np.asarray(U, dtype=LD)
    F = np.asarray(F, dtype=LD)
    aN, aS, aE, aW = _faces_ld(a)
    u = U[1:-1, 1:-1]
    flux = aN * (U[2:, 1:-1] - u) + aS * (U[:-2, 1:-1] - u) + aE * (U[1:-1, 2:] - u) + aW * (U[1:-1, :-2] - u)
    return ref._inv_ld(N, L) * flux - LD(shift) * u - F[1:-1, 1:-1]


def residual_norm_ld(a, U, F, L, shift):
    """Interior L2 norm of div_h(a grad_h U) - shift*U - F in flux form, every operation in longdouble."""
    return np.sqrt(np.sum(_residual_ld(a, U, F, L, shift) ** 2))


def residual_rounding_bound(a, U, F, L, shift):
    """A-priori bound on |fp64 evaluation - residual_norm_ld|: _solve_shift_ref.residual_rounding_bound (8 roundings on every
    neighbour term and on F, 11 on the centre term) scaled by max a, with three more roundings per term for the face
    coefficient (sum, halving -- exact --, product) and for the sum that forms d: 11 and 16."""
    N = F.shape[0]
    A = np.abs(np.asarray(U, dtype=LD))
    inv = ref._inv_ld(N, L)
    amax = LD(float(np.max(a)))
    d = LD(4) * amax + LD(shift) / inv
    nbr = inv * amax * (A[2:, 1:-1] + A[:-2, 1:-1] + A[1:-1, 2:] + A[1:-1, :-2]) + np.abs(np.asarray(F, dtype=LD)[1:-1, 1:-1])
    mag = 11 * nbr + 16 * inv * d * A[1:-1, 1:-1]
    return U53 * np.sqrt(np.sum(mag ** 2)) + LD((N - 2) * (N - 2)) * U53 * residual_norm_ld(a, U, F, L, shift)


def direct_solution(a, F, U, L, shift):
    """The solution of the discrete system on the interior with U's rim as Dirichlet data, by a dense solve in longdouble-
    assembled fp64 with one step of longdouble iterative refinement (small N only: (N-2)^2 unknowns)."""
    N = F.shape[0]
    n = N - 2
    inv = ref._inv_ld(N, L)
    aN, aS, aE, aW = _faces_ld(a)
    X = np.array(U, dtype=LD)
    idx = np.arange(n * n).reshape(n, n)
    Mx = np.zeros((n * n, n * n), dtype=LD)
    G = -np.array(F[1:-1, 1:-1], dtype=LD)        # (-A + shift) u = -F + inv * (face * rim neighbour)
    diag = inv * (aN + aS + aE + aW) + LD(shift)
    Mx[idx, idx] = diag
    for fcs, dr, dc in ((aN, 1, 0), (aS, -1, 0), (aE, 0, 1), (aW, 0, -1)):
        for i in range(n):
            for j in range(n):
                ii, jj = i + dr, j + dc
                if 0 <= ii < n and 0 <= jj < n:
                    Mx[idx[i, j], idx[ii, jj]] = -inv * fcs[i, j]
                else:
                    G[i, j] += inv * fcs[i, j] * X[1 + ii, 1 + jj]
    M64 = Mx.astype(np.float64)
    g = G.reshape(-1)
    u = np.linalg.solve(M64, g.astype(np.float64)).astype(LD)
    for _ in range(3):                             # refinement: residual in longdouble, correction in fp64
        r = g - Mx @ u
        u = u + np.linalg.solve(M64, r.astype(np.float64)).astype(LD)
    X[1:-1, 1:-1] = u.reshape(n, n)
    return X
