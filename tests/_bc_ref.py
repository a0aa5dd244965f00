"""Restatement of the solver with boundary kinds per side (include/mg_bc.h), written from the header on numpy alone.  The
pieces that do not change come from _solve_vc_ref: the face coefficients, the bracket, the level constants and the
coefficient hierarchy.  The mirror of a Neumann side is restated as a padded array: X grows a ghost ring whose Neumann parts
hold the mirror points (X[r][-1] := X[r][1], ...), and _solve_vc_ref's interior expressions on the padded array are the
header's expressions at every grid point; what is kept of them is the rectangle of unknowns.  Transfers, coarse solve, cycle
and solve follow.  The second half holds the references that share no code with the engine: the dense matrix of the operator
assembled in np.longdouble from a, sigma, L, N and the kinds alone, and its direct solve with refinement.
TEST INFRASTRUCTURE."""
import itertools
import math

import numpy as np

import _heat_ref as href
import _solve_ref as ref
import _solve_vc_ref as vref

LD = ref.LD
U53 = ref.U53
DEFAULTS = dict(vref.DEFAULTS)
ALL_KINDS = ["".join(k) for k in itertools.product("dn", repeat=4)]


def kinds(bc):
    """(kS, kN, kW, kE) as ints from a 4-sequence or a string of 'd' / 'n'"""
    if isinstance(bc, str):
        assert len(bc) == 4 and set(bc) <= set("dn"), bc
        return tuple(1 if ch == "n" else 0 for ch in bc)
    k = tuple(int(v) for v in bc)
    assert len(k) == 4 and set(k) <= {0, 1}, bc
    return k


def unknowns(N, bc):
    """(row slice, column slice) of the rectangle of unknowns"""
    kS, kN, kW, kE = kinds(bc)
    return slice(0 if kS else 1, N if kN else N - 1), slice(0 if kW else 1, N if kE else N - 1)


def n_unknowns(N, bc):
    rs, cs = unknowns(N, bc)
    return (rs.stop - rs.start) * (cs.stop - cs.start)


def mask(N, bc):
    m = np.zeros((N, N), dtype=bool)
    m[unknowns(N, bc)] = True
    return m


def pad(X, bc):
    """X with a ghost ring: the mirror point beyond a Neumann side (corners of two Neumann sides mirror both ways), the rim
    value itself beyond a Dirichlet side (never used by an unknown)."""
    kS, kN, kW, kE = kinds(bc)
    X = np.asarray(X)
    N = X.shape[0]
    P = np.empty((N + 2, N + 2), dtype=X.dtype)
    P[1:-1, 1:-1] = X
    P[0, 1:-1] = X[1] if kS else X[0]
    P[-1, 1:-1] = X[N - 2] if kN else X[N - 1]
    P[:, 0] = P[:, 2] if kW else P[:, 1]
    P[:, -1] = P[:, -3] if kE else P[:, -2]
    return P


def _a(a, N):
    return np.ones((N, N)) if a is None else np.ascontiguousarray(a, dtype=np.float64)


def faces(a, sd, bc):
    """(aN, aS, aE, aW, d, q) of _solve_vc_ref.faces at EVERY grid point, ghosts mirrored"""
    return vref.faces(pad(a, bc), sd)


def bracket(fc, U, bc):
    return vref.bracket(fc, pad(np.ascontiguousarray(U, dtype=np.float64), bc))


def weighted_sweeps(N, L, bc, a, U, F, omega, steps, shift=0.0, zero_start=False):
    """`steps` sweeps U <- U + c*(b(U) - dx2*F) at the unknowns on a copy of U, data points kept (zero start: +0)"""
    dx2, _, sd = vref.level_consts(N, L, shift)
    fc = faces(_a(a, N), sd, bc)
    c = omega * fc[5]
    u = unknowns(N, bc)
    U = np.zeros((N, N)) if zero_start else np.array(U, dtype=np.float64, copy=True)
    F = np.ascontiguousarray(F, dtype=np.float64)
    for s in range(steps):
        if zero_start and s == 0:
            U[u] = 0.0 + c[u] * (0.0 - dx2 * F[u])
            continue
        P = U.copy()
        U[u] = P[u] + c[u] * (bracket(fc, P, bc)[u] - dx2 * F[u])
    return U


def apply_operator(N, L, bc, a, U, shift=0.0):
    """inv*b(U) at the unknowns, +0 at data points"""
    _, inv, sd = vref.level_consts(N, L, shift)
    u = unknowns(N, bc)
    out = np.zeros((N, N))
    out[u] = inv * bracket(faces(_a(a, N), sd, bc), U, bc)[u]
    return out


def residual(N, L, bc, a, U, F, shift=0.0, sign=1):
    """D = inv*b(U) - F at the unknowns, +0 at data points; sign < 0: the whole array negated"""
    _, inv, sd = vref.level_consts(N, L, shift)
    u = unknowns(N, bc)
    D = np.zeros((N, N))
    D[u] = inv * bracket(faces(_a(a, N), sd, bc), U, bc)[u] - np.asarray(F, dtype=np.float64)[u]
    return -D if sign < 0 else D


def residual_norm(N, L, bc, a, U, F, shift=0.0):
    return float(np.sqrt(np.sum(residual(N, L, bc, a, U, F, shift)[unknowns(N, bc)] ** 2)))


def ref_norm(F, bc):
    return float(np.sqrt(np.sum(np.asarray(F, dtype=np.float64)[unknowns(F.shape[0], bc)] ** 2)))


def neumann_source(N, L, bc, a, F, g, face_averaged=False):
    """F_eff = F - (t*a)*g at the rim unknowns of Neumann sides, t = 2.0/h, in the order S, N, W, E; g: (4, N).
    face_averaged: the first-order variant the header warns of (the face average in the nodal coefficient's place), kept here
    for the accuracy test that tells the two apart -- not what the engine does."""
    k = kinds(bc)
    h = L / float(N - 1)
    t = 2.0 / h
    A = _a(a, N)
    if face_averaged:
        P = pad(A, bc)
        co = [0.5 * (A + P[:-2, 1:-1]), 0.5 * (A + P[2:, 1:-1]), 0.5 * (A + P[1:-1, :-2]), 0.5 * (A + P[1:-1, 2:])]
    else:
        co = [A, A, A, A]
    m = mask(N, bc)
    out = np.array(F, dtype=np.float64, copy=True)
    g = np.asarray(g, dtype=np.float64)
    idx = np.arange(N)
    for side, (rows, cols) in enumerate(((0, idx), (N - 1, idx), (idx, 0), (idx, N - 1))):
        if not k[side]:
            continue
        sel = m[rows, cols]
        cur = out[rows, cols]
        new = cur - (t * co[side][rows, cols]) * g[side]
        out[rows, cols] = np.where(sel, new, cur)
    return out


# ---------------------------------------------------------------- transfers
def restrict(D, M, bc, table=None):
    """doRestriction's expression at the coarse unknowns with the table's end entries replaced, +0 at coarse data points"""
    D = np.ascontiguousarray(D, dtype=np.float64)
    N = D.shape[0]
    lo, w = table if table is not None else vref.restriction_table(N, M)
    lo = np.array(lo, dtype=np.int64)
    w = np.array(w, dtype=np.float64)
    lo[0], w[0] = 0, 0.0
    lo[M - 1], w[M - 1] = N - 2, 1.0
    wa, wc = w[None, :], w[:, None]
    wb, wd = 1.0 - wa, 1.0 - wc
    r, c = lo[:, None], lo[None, :]
    v = wb * wd * D[r, c] + wa * wd * D[r, c + 1] + wc * wb * D[r + 1, c] + wa * wc * D[r + 1, c + 1]
    out = np.zeros((M, M))
    u = unknowns(M, bc)
    out[u] = v[u]
    return out


def prolongation_table(M, N):
    """mg_boundary_prolongation_table's expressions"""
    h_f, h_c = 1.0 / float(N - 1), 1.0 / float(M - 1)
    lo = np.empty(N, dtype=np.int64)
    w = np.empty(N, dtype=np.float64)
    for k in range(N):
        l = min(int(math.floor(float(k) * h_f / h_c)), M - 2)
        wt = (float(k) * h_f - float(l) * h_c) / h_c
        lo[k], w[k] = l, min(max(wt, 0.0), 1.0)
    lo[0], w[0] = 0, 0.0
    lo[N - 1], w[N - 1] = M - 2, 1.0
    return lo, w


def prolong(U_c, N, table=None):
    """P(U_c) at every fine point"""
    U_c = np.ascontiguousarray(U_c, dtype=np.float64)
    M = U_c.shape[0]
    lo, w = table if table is not None else prolongation_table(M, N)
    lo = np.asarray(lo, dtype=np.int64)
    wa, wc = np.asarray(w)[None, :], np.asarray(w)[:, None]
    wb, wd = 1.0 - wa, 1.0 - wc
    r, c = lo[:, None], lo[None, :]
    return wb * wd * U_c[r, c] + wa * wd * U_c[r, c + 1] + wc * wb * U_c[r + 1, c] + wa * wc * U_c[r + 1, c + 1]


def prolong_add(U_c, N, U_in, bc, table=None):
    """U_in + P(U_c) at the fine unknowns, U_in at fine data points"""
    out = np.array(U_in, dtype=np.float64, copy=True)
    u = unknowns(N, bc)
    out[u] = out[u] + prolong(U_c, N, table)[u]
    return out


# ---------------------------------------------------------------- coarse solve, cycle, solve
def rbgs_trace(N, L, bc, a, F, atol, rtol, max_iters, shift=0.0):
    """_solve_vc_ref.rbgs_trace on the unknowns with mirrored neighbours; err and err0 divide by the number of unknowns"""
    F = np.ascontiguousarray(F, dtype=np.float64)
    h2, inv, sd = vref.level_consts(N, L, shift)
    fc = faces(_a(a, N), sd, bc)
    aN, aS, aE, aW, _, q = fc
    u = unknowns(N, bc)
    denom = float(n_unknowns(N, bc))
    err0 = float(np.sum(np.abs(F[u]))) / denom
    target = max(atol, rtol * err0)
    rr, cc = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    m = mask(N, bc)
    masks = [m & (((rr + cc) & 1) == colour) for colour in (0, 1)]
    U = np.zeros((N, N))
    errs = []
    while True:
        for mk in masks:
            P = pad(U, bc)
            V = q * ((((aW * P[1:-1, :-2] + aE * P[1:-1, 2:]) + aN * P[2:, 1:-1]) + aS * P[:-2, 1:-1]) - h2 * F)
            U[mk] = V[mk]
        err = float(np.sum(np.abs(inv * bracket(fc, U, bc)[u] - F[u]))) / denom
        errs.append(err)
        if not (err > target) or len(errs) >= max_iters:
            break
    return U, err0, errs


def cycle(levels, F, U, bc, L=1.0, margins=None, capped=None, rtable=None, ptable=None, iters=None, **opts):
    """One V(pre, post) cycle; levels = _solve_vc_ref.coarsen_levels(a, N_min), or None for a = 1.  rtable(N, M) / ptable(M, N)
    replace the restatement's own tables."""
    o = dict(DEFAULTS, **opts)
    sh = float(o["shift"])
    sz = ref.sizes(F.shape[0], o["N_min"])
    nl = len(sz)
    A = levels if levels is not None else [None] * nl
    Us, Fs = [None] * nl, [None] * nl
    Fs[0] = np.ascontiguousarray(F, dtype=np.float64)
    for l in range(nl - 1):
        N, M = sz[l], sz[l + 1]
        Us[l] = weighted_sweeps(N, L, bc, A[l], U if l == 0 else None, Fs[l], o["omega"], o["pre"], sh, zero_start=l > 0)
        D = residual(N, L, bc, A[l], Us[l], Fs[l], sh, sign=-1)
        Fs[l + 1] = restrict(D, M, bc, rtable(N, M) if rtable else None)
    tr = rbgs_trace(sz[-1], L, bc, A[-1], Fs[-1], o["coarse_atol"], o["coarse_rtol"], o["coarse_max_iters"], sh)
    Us[-1] = tr[0]
    if margins is not None:
        margins.append(vref.coarse_margin(tr, o["coarse_atol"], o["coarse_rtol"]))
    if capped is not None:
        capped.append(tr[2][-1] > max(o["coarse_atol"], o["coarse_rtol"] * tr[1]))
    if iters is not None:
        iters.append(len(tr[2]))
    for l in range(nl - 2, -1, -1):
        U_l = prolong_add(Us[l + 1], sz[l], Us[l], bc, ptable(sz[l + 1], sz[l]) if ptable else None)
        Us[l] = weighted_sweeps(sz[l], L, bc, A[l], U_l, Fs[l], o["omega"], o["post"], sh)
    return Us[0]


def solve(a, F, U, bc, L=1.0, margins=None, capped=None, rtable=None, ptable=None, iters=None, **opts):
    """Returns (U, history, cycles, converged) under the stopping rule of mg_solver_solve, norms over the unknowns"""
    o = dict(DEFAULTS, **opts)
    sh = float(o["shift"])
    N = F.shape[0]
    levels = vref.coarsen_levels(a, o["N_min"], rtable) if a is not None else None
    U = np.zeros((N, N)) if U is None else np.array(U, dtype=np.float64, copy=True)
    tol = max(o["rtol"] * ref_norm(F, bc), o["atol"])
    r = residual_norm(N, L, bc, a, U, F, sh)
    history = [r]
    k = 0
    while not (r <= tol) and k < o["max_cycles"]:
        U = cycle(levels, F, U, bc, L, margins=margins, capped=capped, rtable=rtable, ptable=ptable, iters=iters, **opts)
        r = residual_norm(N, L, bc, a, U, F, sh)
        history.append(r)
        k += 1
    return U, history, k, r <= tol


# ---------------------------------------------------------------- heat
def heat_rhs(N, L, nu, dt, theta, bc, a, U, Q=None):
    """F = -(sigma*u) [- beta*(inv*b(u))] [- gamma*q] at the unknowns, +0 at data points; theta == 1 leaves the operator out"""
    sigma, beta, gamma, _ = href.consts(N, L, nu, dt, theta)
    U = np.ascontiguousarray(U, dtype=np.float64)
    u = unknowns(N, bc)
    s = -(sigma * U[u])
    if float(theta) != 1.0:
        s = s - beta * apply_operator(N, L, bc, a, U, 0.0)[u]
    if Q is not None:
        s = s - gamma * np.asarray(Q, dtype=np.float64)[u]
    F = np.zeros((N, N))
    F[u] = s
    return F


# ---------------------------------------------------------------- references in np.longdouble
def trapezoid_weights(N, bc):
    """w at every grid point: 1 inside, 1/2 on a Neumann rim unknown, 1/4 at the corner of two Neumann sides"""
    wr = np.ones(N, dtype=LD)
    wc = np.ones(N, dtype=LD)
    wr[0] = wr[-1] = LD(1) / LD(2)
    wc[0] = wc[-1] = LD(1) / LD(2)
    return wr[:, None] * wc[None, :]


def dense_operator(a, N, L, shift, bc):
    """The matrix of U -> inv*b(U) (sigma included) in longdouble, from a, sigma, L, N and the kinds alone: one row per
    unknown (row-major over the rectangle of unknowns), one column per GRID point (N*N, data points included).  A neighbour
    beyond a Neumann side is its mirror point, for the value and for the coefficient; faces average their two nodes.
    Returns (A_full, index of the unknowns among the N*N points)."""
    k = kinds(bc)
    a = np.ones((N, N), dtype=LD) if a is None else np.asarray(a, dtype=LD)
    inv = ref._inv_ld(N, L)
    half = LD(1) / LD(2)
    m = mask(N, bc)
    unk = np.flatnonzero(m.reshape(-1))
    row_of = -np.ones(N * N, dtype=np.int64)
    row_of[unk] = np.arange(unk.size)
    A = np.zeros((unk.size, N * N), dtype=LD)

    def mirror(i, lo_kind, hi_kind):
        if i < 0:
            assert lo_kind, "an unknown next to a Dirichlet side has its neighbour inside the grid"
            return 1
        if i > N - 1:
            assert hi_kind
            return N - 2
        return i

    for p in unk:
        r, c = divmod(int(p), N)
        i = row_of[p]
        diag = LD(0)
        for dr, dc in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            rr, cc = mirror(r + dr, k[0], k[1]), mirror(c + dc, k[2], k[3])
            face = half * (a[r, c] + a[rr, cc])
            A[i, rr * N + cc] += inv * face
            diag += face
        A[i, p] += -(inv * diag) - LD(shift)
    return A, unk


def residual_ld(a, U, F, L, shift, bc):
    """A U - F at the unknowns, in longdouble (flat, in the order of the unknowns)"""
    N = F.shape[0]
    A, unk = dense_operator(a, N, L, shift, bc)
    return A @ np.asarray(U, dtype=LD).reshape(-1) - np.asarray(F, dtype=LD).reshape(-1)[unk]


def residual_ld_stencil(a, U, F, L, shift, bc):
    """residual_ld without the matrix, for sizes at which the dense operator does not fit: the same faces (the mean of two
    nodes, the mirror node beyond a Neumann side) and the same diagonal, evaluated on the padded arrays in longdouble.  Flat,
    in the order of the unknowns.  a = None: a = 1; a scalar: that constant."""
    N = F.shape[0]
    u = unknowns(N, bc)
    A = np.ones((N, N), dtype=LD) if a is None else np.broadcast_to(np.asarray(a, dtype=LD), (N, N))
    Pa, P = pad(A, bc), pad(np.asarray(U, dtype=LD), bc)
    half = LD(1) / LD(2)
    c, x = Pa[1:-1, 1:-1], P[1:-1, 1:-1]
    acc, diag = np.zeros((N, N), dtype=LD), np.zeros((N, N), dtype=LD)
    for rows, cols in ((slice(2, None), slice(1, -1)), (slice(None, -2), slice(1, -1)), (slice(1, -1), slice(2, None)),
                       (slice(1, -1), slice(None, -2))):
        face = half * (c + Pa[rows, cols])
        acc = acc + face * P[rows, cols]
        diag = diag + face
    r = ref._inv_ld(N, L) * (acc - diag * x) - LD(shift) * x - np.asarray(F, dtype=LD)
    return r[u].reshape(-1)


def residual_rounding_bound(a, U, F, L, shift, bc, r=None):
    """_solve_vc_ref.residual_rounding_bound extended to the rim unknowns: the same count of roundings per term, the
    neighbours taken through the mirror.  r: the longdouble residual where the caller has it (residual_ld_stencil at the
    sizes the dense operator does not reach); None: residual_ld."""
    N = F.shape[0]
    u = unknowns(N, bc)
    P = np.abs(pad(np.asarray(U, dtype=LD), bc))
    inv = ref._inv_ld(N, L)
    amax = LD(1.0 if a is None else float(np.max(a)))
    d = LD(4) * amax + LD(shift) / inv
    nbr = inv * amax * (P[2:, 1:-1] + P[:-2, 1:-1] + P[1:-1, 2:] + P[1:-1, :-2]) + np.abs(np.asarray(F, dtype=LD))
    mag = (11 * nbr + 16 * inv * d * P[1:-1, 1:-1])[u]
    if r is None:
        r = residual_ld(a, U, F, L, shift, bc)
    return U53 * np.sqrt(np.sum(mag ** 2)) + LD(n_unknowns(N, bc)) * U53 * np.sqrt(np.sum(r ** 2))


def direct_solution(a, F, U, L, shift, bc, want_inverse_norm=False):
    """The solution of the discrete system at the unknowns with U's data points as Dirichlet data, by a dense solve in
    longdouble-assembled fp64 with longdouble iterative refinement, as _solve_vc_ref.direct_solution does (small N only).
    want_inverse_norm: also the infinity norm of the inverse of the matrix over the unknowns (fp64 inverse)."""
    N = F.shape[0]
    A, unk = dense_operator(a, N, L, shift, bc)
    X = np.array(U, dtype=LD).reshape(-1)
    data = np.setdiff1d(np.arange(N * N), unk)
    Auu = A[:, unk]
    g = np.asarray(F, dtype=LD).reshape(-1)[unk] - A[:, data] @ X[data]
    M64 = Auu.astype(np.float64)
    u = np.linalg.solve(M64, g.astype(np.float64)).astype(LD)
    for _ in range(3):
        r = g - Auu @ u
        u = u + np.linalg.solve(M64, r.astype(np.float64)).astype(LD)
    X[unk] = u
    X = X.reshape(N, N)
    if want_inverse_norm:
        return X, LD(float(np.max(np.sum(np.abs(np.linalg.inv(M64)), axis=1))))
    return X
