"""Restatement of the full-multigrid start of the residual-tolerance solver (include/mg_hip.h: mg_solve_opts.fmg,
mg_cubic_table, mg_prolongCubic), written from the header on numpy, the oracle's transfer operators and the cycle of
_solve_shift_ref generalised to a top level.  The interpolation table is taken from the ABI (mg_cubic_table), as the
kernels take it; lagrange_table_ld() is the independent check of that table in np.longdouble.  TEST INFRASTRUCTURE."""
import numpy as np

import _solve_ref as ref
import _solve_shift_ref as sref

LD = ref.LD
DEFAULTS = dict(sref.DEFAULTS, fmg=0)


def abi_table(N_src, N_dst):
    import multigrid_poisson_solver_amd as m
    return m.cubic_table(N_src, N_dst)


def lagrange_table_ld(N_src, N_dst):
    """(base, w) of the header's definition in np.longdouble: every factor (t - x_j) = (i*(N_src-1) - x_j*(N_dst-1)) /
    (N_dst-1) from Python integers, so no weight suffers the cancellation of a rounded t."""
    m = min(4, N_src)
    P, Q = N_src - 1, N_dst - 1
    base = np.zeros(N_dst, dtype=np.int64)
    w = np.zeros((N_dst, 4), dtype=LD)
    for i in range(N_dst):
        b = min(max(i * P // Q - 1, 0), N_src - m)
        base[i] = b
        for k in range(m):
            v = LD(1)
            for j in range(m):
                if j != k:
                    v = v * LD(i * P - (b + j) * Q) / LD((k - j) * Q)
            w[i, k] = v
    return base, w


def interp1(table, S, m):
    """The 1-D interpolation along the last axis of S in the header's order: ((w0 s0 + w1 s1) + w2 s2) + w3 s3 (m = 3: the
    last term left out); every product and sum one numpy operation."""
    base, w = table
    S = np.asarray(S, dtype=np.float64)
    v = w[:, 0] * S[..., base] + w[:, 1] * S[..., base + 1]
    v = v + w[:, 2] * S[..., base + 2]
    if m > 3:
        v = v + w[:, 3] * S[..., base + 3]
    return v


def prolong_cubic(Uc, N_dst, table=None):
    """mg_prolongCubic: the N_dst x N_dst bicubic interpolation of Uc (the caller keeps the interior only)."""
    N_src = Uc.shape[0]
    m = min(4, N_src)
    table = abi_table(N_src, N_dst) if table is None else table
    H = interp1(table, Uc, m)                       # [N_src, N_dst]: along the columns of every source row
    return interp1(table, H.T, m).T                 # then along the rows


def edges(U):
    return [U[0, :].copy(), U[-1, :].copy(), U[:, 0].copy(), U[:, -1].copy()]


def set_rim(U, g):
    U[:, 0], U[:, -1] = g[2], g[3]
    U[0, :], U[-1, :] = g[0], g[1]
    return U


def cycle(orc, F, U, L, sz, top=0, margins=None, capped=None, **opts):
    """_solve_shift_ref.cycle started at level `top` of the hierarchy sz from the field U on the source F (both of size
    sz[top]); the levels below start from zero."""
    o = dict(DEFAULTS, **opts)
    sh = float(o["shift"])
    nl = len(sz)
    Us, Fs = [None] * nl, [None] * nl
    Fs[top] = np.ascontiguousarray(F, dtype=np.float64)
    for l in range(top, nl - 1):
        N, M = sz[l], sz[l + 1]
        start = U if l == top else np.zeros((N, N))
        Us[l] = sref.weighted_sweeps(N, L, start, Fs[l], o["omega"], o["pre"], sh)
        D = -sref.residual(N, L, Us[l], Fs[l], sh)
        Fs[l + 1] = orc.doRestriction(N, D, M)
    Nc = sz[-1]
    tr = sref.rbgs_trace(Nc, L, Fs[-1], o["coarse_atol"], o["coarse_rtol"], o["coarse_max_iters"], sh)
    Us[-1] = tr[0]
    if margins is not None:
        margins.append(sref.coarse_margin(Nc, L, Fs[-1], o["coarse_atol"], o["coarse_rtol"], o["coarse_max_iters"], sh, trace=tr))
    if capped is not None:
        capped.append(tr[2][-1] > max(o["coarse_atol"], o["coarse_rtol"] * tr[1]))
    for l in range(nl - 2, top - 1, -1):
        tmp = orc.doProlongation(sz[l + 1], Us[l + 1], sz[l])
        U_l = orc.doGridAddition(sz[l], Us[l], tmp)
        Us[l] = sref.weighted_sweeps(sz[l], L, U_l, Fs[l], o["omega"], o["post"], sh)
    return Us[top]


def fmg_guess(orc, F, U, L=1.0, margins=None, capped=None, **opts):
    """The FMG pass: U with its interior replaced by the guess (the rim untouched).  margins / capped receive one entry
    per coarse solve of the pass, in launch order."""
    o = dict(DEFAULTS, **opts)
    sh = float(o["shift"])
    sz = ref.sizes(F.shape[0], o["N_min"])
    nl = len(sz)
    Fs = [np.ascontiguousarray(F, dtype=np.float64)]
    g = [edges(np.asarray(U, dtype=np.float64))]
    for l in range(nl - 1):
        Fs.append(orc.doRestriction(sz[l], Fs[l], sz[l + 1]))
        down = abi_table(sz[l], sz[l + 1])
        g.append([interp1(down, e, min(4, sz[l])) for e in g[l]])
    Nc = sz[-1]
    r = -sref.residual(Nc, L, set_rim(np.zeros((Nc, Nc)), g[-1]), Fs[-1], sh)
    tr = sref.rbgs_trace(Nc, L, r, o["coarse_atol"], o["coarse_rtol"], o["coarse_max_iters"], sh)
    if margins is not None:
        margins.append(sref.coarse_margin(Nc, L, r, o["coarse_atol"], o["coarse_rtol"], o["coarse_max_iters"], sh, trace=tr))
    if capped is not None:
        capped.append(tr[2][-1] > max(o["coarse_atol"], o["coarse_rtol"] * tr[1]))
    u = set_rim(tr[0].copy(), g[-1])
    for l in range(nl - 2, -1, -1):
        P = prolong_cubic(u, sz[l])
        u = np.array(U, dtype=np.float64, copy=True) if l == 0 else set_rim(np.zeros((sz[l], sz[l])), g[l])
        u[1:-1, 1:-1] = P[1:-1, 1:-1]
        if l >= 1:
            for _ in range(int(o["fmg"])):
                u = cycle(orc, Fs[l], u, L, sz, top=l, margins=margins, capped=capped, **opts)
    return u


def solve(orc, F, U=None, L=1.0, margins=None, capped=None, **opts):
    """Returns (U, history, cycles, converged) under the stopping rule of mg_solver_solve with the fmg option: history[0]
    is the norm of the caller's start, the pass is not a cycle, a start that meets the tolerance is left alone."""
    o = dict(DEFAULTS, **opts)
    sh = float(o["shift"])
    N = F.shape[0]
    sz = ref.sizes(N, o["N_min"])
    U = np.zeros((N, N)) if U is None else np.array(U, dtype=np.float64, copy=True)
    tol = max(o["rtol"] * ref.ref_norm(F), o["atol"])
    r = sref.residual_norm(N, L, U, F, sh)
    history = [r]
    k = 0
    if int(o["fmg"]) >= 1 and not (r <= tol):
        U = fmg_guess(orc, F, U, L, margins=margins, capped=capped, **opts)
    while not (r <= tol) and k < o["max_cycles"]:
        U = cycle(orc, F, U, L, sz, margins=margins, capped=capped, **opts)
        r = sref.residual_norm(N, L, U, F, sh)
        history.append(r)
        k += 1
    return U, history, k, r <= tol
