"""Restatement of the residual-tolerance solver with a variable reaction term, div(a grad U) - (sigma + s)*U = F, written
from include/mg_reaction.h on numpy.  The header changes ONE quantity of include/mg_varcoef.h, the shift term of the centre,

    t = s[p]*dx2,   sdp = sd + t,   d = (((aN + aS) + aE) + aW) + sdp                (each operation rounded once)

and everything else is the variable-coefficient cycle.  So this module restates that quantity and hands it to the
restatement of the cycle, _solve_vc_ref, whose faces(a, sd) broadcasts an interior-shaped sd: operator(levels) is a context
in which _solve_vc_ref.level_consts returns the per-point sdp of the level of that size, and inside it every function of
_solve_vc_ref and of _krylov_ref (sweeps, residual, coarse trace, cycle, solve, GCR) is the reaction solver's.  a = None is
a = 1 through the same expressions (an array of ones).  engine_norm restates the summation ORDER of the device norm, so
that a history can be compared with ==.  The last part holds a dense direct solution assembled in longdouble, which shares
no code with the engine.  TEST INFRASTRUCTURE."""
import contextlib

import numpy as np

import _krylov_ref as kref
import _solve_ref as ref
import _solve_vc_ref as vref

LD = ref.LD
U53 = ref.U53
DEFAULTS = dict(vref.DEFAULTS)
TB, ROWS, PAIR_MIN_N = 256, 4, 512   # the block of the norm kernels: 256 lanes, 4 rows each, column pairs for even N >= 512
_level_consts = vref.level_consts


def centre_shift(N, L, shift, s):
    """(dx2, inv, sdp): the level constants of _solve_vc_ref.level_consts with sd replaced by the header's per-point
    sdp = sd + s*dx2 on the interior."""
    dx2, inv, sd = _level_consts(N, L, shift)
    t = np.ascontiguousarray(s, dtype=np.float64)[1:-1, 1:-1] * dx2
    return dx2, inv, sd + t


@contextlib.contextmanager
def operator(levels):
    """levels: [s_0, s_1, ...], one array per level of a hierarchy (or one array alone), found by its size."""
    by_N = {int(s.shape[0]): np.ascontiguousarray(s, dtype=np.float64) for s in ([levels] if isinstance(levels, np.ndarray) else levels)}
    assert vref.level_consts is _level_consts, "operator() does not nest"
    vref.level_consts = lambda N, L, shift: centre_shift(N, L, shift, by_N[N])
    try:
        yield
    finally:
        vref.level_consts = _level_consts


def ones_if_none(a, N):
    return np.ones((N, N)) if a is None else np.ascontiguousarray(a, dtype=np.float64)


# ---------------------------------------------------------------- the operations alone
def sweep(N, L, a, s, U, F, omega, shift=0.0, zero_start=False):
    with operator(s):
        return vref.weighted_sweeps(N, L, ones_if_none(a, N), U, F, omega, 1, shift, zero_start=zero_start)


def residual(N, L, a, s, U, F, shift=0.0, sign=1):
    with operator(s):
        return vref.residual(N, L, ones_if_none(a, N), U, F, shift, sign)


def apply_operator(N, L, a, s, U, shift=0.0):
    with operator(s):
        return vref.apply_operator(N, L, ones_if_none(a, N), U, shift)


def rbgs_trace(N, L, a, s, F, atol, rtol, max_iters, shift=0.0):
    with operator(s):
        return vref.rbgs_trace(N, L, ones_if_none(a, N), F, atol, rtol, max_iters, shift)


def coarsen_levels(s, N_min, table=None):
    """s on every level: _solve_vc_ref.coarsen_levels, the coefficient's own coarsening"""
    return vref.coarsen_levels(s, N_min, table)


# ---------------------------------------------------------------- the norm in the device's summation order
def _wave_sum(v):
    """lane 0 of wave_sum: v += shfl_down(v, o) for o = 32, 16, ..., 1 over the last axis of 64"""
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def _block_sum(v):
    """block_sum over the last axis (a multiple of 64 lanes): the waves' sums added in order from 0.0"""
    w = _wave_sum(v.reshape(v.shape[:-1] + (-1, 64)))
    r = np.zeros(w.shape[:-1])
    for i in range(w.shape[-1]):
        r = r + w[..., i]
    return r


def engine_norm(D):
    """sqrt of the sum of D^2 over the interior in the partition and the order of the device norm (csrc/mg_varcoef_impl.h:
    resnorm_vc_body, resnorm_finish_body).  D: N x N with the residual inside; the rim is not read."""
    N = D.shape[0]
    sq = np.zeros((N, N))
    sq[1:-1, 1:-1] = D[1:-1, 1:-1] * D[1:-1, 1:-1]
    pair = N % 2 == 0 and N >= PAIR_MIN_N
    per = 2 if pair else 1
    gx, gy = (N // per + TB - 1) // TB, (N + ROWS - 1) // ROWS
    pad = np.zeros((gy * ROWS, gx * TB * per))
    pad[:N, :N] = sq
    t = pad.reshape(gy, ROWS, gx, TB, per)
    acc = np.zeros((gy, gx, TB))
    for i in range(ROWS):          # a lane: its 4 rows in order, in a row its column (pair: x, then y)
        for j in range(per):
            acc = acc + t[:, i, :, :, j]
    part = _block_sum(acc).reshape(-1)           # partial (by, bx) at by*gx + bx
    n = part.size
    rows = (n + 1023) // 1024
    fin = np.zeros(rows * 1024)
    fin[:n] = part
    fin = fin.reshape(rows, 1024)
    acc = np.zeros(1024)
    for i in range(rows):
        acc = acc + fin[i]
    return float(np.sqrt(_block_sum(acc)))


def residual_norm(N, L, a, s, U, F, shift=0.0, engine=False):
    D = residual(N, L, a, s, U, F, shift)
    return engine_norm(D) if engine else float(np.sqrt(np.sum(D[1:-1, 1:-1] ** 2)))


# ---------------------------------------------------------------- cycle and solves
def cycle(orc, a_levels, s_levels, F, U, L=1.0, margins=None, capped=None, **opts):
    with operator(s_levels):
        return vref.cycle(orc, a_levels, F, U, L, margins=margins, capped=capped, **opts)


def solve(orc, a, s, F, U=None, L=1.0, margins=None, capped=None, table=None, engine_norms=False, keep=None, **opts):
    """(U, history, cycles, converged) under the stopping rule of mg_solver_solve.  engine_norms: the history in the device's
    summation order.  keep: a list that receives U after every cycle."""
    o = dict(DEFAULTS, **opts)
    sh = float(o["shift"])
    N = F.shape[0]
    a = ones_if_none(a, N)
    a_levels = vref.coarsen_levels(a, o["N_min"], table)
    s_levels = coarsen_levels(s, o["N_min"], table)
    U = np.zeros((N, N)) if U is None else np.array(U, dtype=np.float64, copy=True)
    tol = max(o["rtol"] * ref.ref_norm(F), o["atol"])
    r = residual_norm(N, L, a, s, U, F, sh, engine_norms)
    history, k = [r], 0
    while not (r <= tol) and k < o["max_cycles"]:
        U = cycle(orc, a_levels, s_levels, F, U, L, margins=margins, capped=capped, **opts)
        r = residual_norm(N, L, a, s, U, F, sh, engine_norms)
        history.append(r)
        k += 1
        if keep is not None:
            keep.append(U)
    return U, history, k, r <= tol


def krylov_solve(orc, a, s, F, U=None, L=1.0, m=8, log=None, margins=None, table=None, **opts):
    """_krylov_ref.solve (restarted GCR(m), or its replay from an engine log) on the reaction operator"""
    o = dict(DEFAULTS, **opts)
    with operator(coarsen_levels(s, o["N_min"], table)):
        return kref.solve(orc, a, F, U, L, m=m, log=log, margins=margins, table=table, **opts)


# ---------------------------------------------------------------- the fields of the tests
def field(name, N, L=1.0):
    x, y = vref.grid(N, L)
    if name == "smooth":
        return 1e4 * (1.0 + np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y))
    if name == "blob":
        return 1e6 * np.exp(-((x - 0.4) ** 2 + (y - 0.6) ** 2) / 0.01)
    if name == "halfplane":
        return np.where(x >= 0.37, 1e5, 0.0) + 0.0 * y
    if name == "random":
        return 10.0 ** (6.0 * np.random.default_rng(5).random((N, N)))
    raise ValueError(name)


FIELDS = ("smooth", "blob", "halfplane", "random")


# ---------------------------------------------------------------- truth: dense, assembled in longdouble
def dense_operator(a, s, N, L, shift):
    """M = -A on the interior unknowns (symmetric positive definite), assembled in longdouble from a, s, sigma, L and N alone:
    diag = inv*(aN + aS + aE + aW) + sigma + s, off-diagonals -inv*face; and the faces (aN, aS, aE, aW) for the rim terms."""
    n = N - 2
    inv = ref._inv_ld(N, L)
    fc = vref._faces_ld(ones_if_none(a, N))
    idx = np.arange(n * n).reshape(n, n)
    Mx = np.zeros((n * n, n * n), dtype=LD)
    Mx[idx, idx] = inv * (fc[0] + fc[1] + fc[2] + fc[3]) + LD(shift) + np.asarray(s, dtype=LD)[1:-1, 1:-1]
    for f, dr, dc in zip(fc, (1, -1, 0, 0), (0, 0, 1, -1)):
        i0, i1, j0, j1 = max(0, -dr), n - max(0, dr), max(0, -dc), n - max(0, dc)   # the points whose neighbour is an unknown
        Mx[idx[i0:i1, j0:j1], idx[i0 + dr:i1 + dr, j0 + dc:j1 + dc]] = -inv * f[i0:i1, j0:j1]
    return Mx, fc


def direct_solution(a, s, F, U, L, shift):
    """(X, ||M^-1||_inf): the solution of the discrete system with U's rim as data -- fp64 LU of the longdouble-assembled
    matrix with longdouble iterative refinement -- and the infinity norm of the fp64 inverse (the factor between a residual
    and an error, each in the max norm)."""
    N = F.shape[0]
    n = N - 2
    inv = ref._inv_ld(N, L)
    Mx, (aN, aS, aE, aW) = dense_operator(a, s, N, L, shift)
    X = np.array(U, dtype=LD)
    G = -np.array(F[1:-1, 1:-1], dtype=LD)
    G[-1, :] += inv * aN[-1, :] * X[-1, 1:-1]
    G[0, :] += inv * aS[0, :] * X[0, 1:-1]
    G[:, -1] += inv * aE[:, -1] * X[1:-1, -1]
    G[:, 0] += inv * aW[:, 0] * X[1:-1, 0]
    M64 = Mx.astype(np.float64)
    Minv = np.linalg.inv(M64)
    g = G.reshape(-1)
    u = (Minv @ g.astype(np.float64)).astype(LD)
    for _ in range(4):
        u = u + (Minv @ (g - Mx @ u).astype(np.float64)).astype(LD)
    X[1:-1, 1:-1] = u.reshape(n, n)
    return X, LD(float(np.max(np.sum(np.abs(Minv), axis=1))))


def residual_ld(a, s, U, F, L, shift):
    """div_h(a grad_h U) - (sigma + s)*U - F on the interior in flux form, every operation in longdouble"""
    N = F.shape[0]
    return vref._residual_ld(ones_if_none(a, N), U, F, L, shift) - np.asarray(s, dtype=LD)[1:-1, 1:-1] * np.asarray(U, dtype=LD)[1:-1, 1:-1]
