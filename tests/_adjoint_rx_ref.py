"""Restatement of the adjoint of reaction and semilinear solves, written from include/mg_adjoint_rx.h on numpy: the source
gradient in the header's order (every operation rounded once; g by _newton_ref.g_gp, exp per element from the host libm) with
its sum in the device's partition and order, and the dense adjoint solves that go with _reaction_ref.direct_solution and
_newton_ref.dense_newton.  The partition sum is this file's own copy of _reaction_ref.engine_norm without the square and the
square root.  TEST INFRASTRUCTURE.

Rows are the first index, as in _adjoint_ref."""
import numpy as np

import _adjoint_ref as aref
import _newton_ref as nref
import _reaction_ref as rref

LD = rref.LD
U53 = rref.U53
KINDS = nref.KINDS + ("linear",)
TB, ROWS, PAIR_MIN_N = 256, 4, 512   # the block of the pass: 256 lanes, 4 rows each, column pairs for even N >= 512


def g_of(kind, v):
    """g(v) by the header's table: _newton_ref's three kinds, or v itself ("linear")"""
    if kind == "linear":
        return np.asarray(v, dtype=np.float64)
    return nref.g_gp(kind, v)[0]


def _wave_sum(v):
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def _block_sum(v):
    w = _wave_sum(v.reshape(v.shape[:-1] + (-1, 64)))
    r = np.zeros(w.shape[:-1])
    for i in range(w.shape[-1]):
        r = r + w[..., i]
    return r


def engine_sum(T):
    """the sum of T over the interior in the partition and the order of the pass's norm (include/mg_newton.h): a lane's 4 rows
    in order, in a row its column (pair: x, then y); the block sum; the partial of block (bx, by) at by*gx + bx; the finish
    over 1024 lanes.  T: N x N; its rim is not read."""
    N = T.shape[0]
    t0 = np.zeros((N, N))
    t0[1:-1, 1:-1] = T[1:-1, 1:-1]
    pair = N % 2 == 0 and N >= PAIR_MIN_N
    per = 2 if pair else 1
    gx, gy = (N // per + TB - 1) // TB, (N + ROWS - 1) // ROWS
    pad = np.zeros((gy * ROWS, gx * TB * per))
    pad[:N, :N] = t0
    t = pad.reshape(gy, ROWS, gx, TB, per)
    acc = np.zeros((gy, gx, TB))
    for i in range(ROWS):
        for j in range(per):
            acc = acc + t[:, i, :, :, j]
    part = _block_sum(acc).reshape(-1)
    n = part.size
    rows = (n + 1023) // 1024
    fin = np.zeros(rows * 1024)
    fin[:n] = part
    fin = fin.reshape(rows, 1024)
    acc = np.zeros(1024)
    for i in range(rows):
        acc = acc + fin[i]
    return float(_block_sum(acc))


def source_gradient(N, kind, kappa, w, lam, U):
    """(G, sum): at an interior point gv = g(U), m = lam*gv, G = kappa*m, term = w*m (w = None: m); +0.0 for both on the rim,
    where neither g(U) nor lam is used."""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    U = np.ascontiguousarray(U, dtype=np.float64)
    i = (slice(1, -1), slice(1, -1))
    with np.errstate(over="ignore", invalid="ignore"):
        m = lam[i] * g_of(kind, U[i])
        G, T = np.zeros((N, N)), np.zeros((N, N))
        G[i] = float(kappa) * m
        T[i] = m if w is None else np.ascontiguousarray(w, dtype=np.float64)[i] * m
        return G, engine_sum(T)


# ---------------------------------------------------------------- dense references (small N)
def _g_ld(kind, v):
    return np.asarray(v, dtype=LD) if kind == "linear" else nref._g_ld(kind, v)[0]


def linearised_reaction(N, kind, kappa, w, U):
    """S = kappa*w*g'(U) in longdouble, N x N (the rim is not used by the dense operator)"""
    wn = np.ones((N, N), dtype=LD) if w is None else np.asarray(w, dtype=LD)
    return LD(kappa) * wn * nref._g_ld(kind, U)[1]


def direct_adjoint(a, S, Ubar, L, shift):
    """(lam, ||M^-1||_inf): the dense solve of (A - S) lam = Ubar with a zero rim, in longdouble (_reaction_ref.direct_solution:
    the operator is symmetric on the interior)"""
    N = Ubar.shape[0]
    return rref.direct_solution(a, S, Ubar, np.zeros((N, N)), L, shift)


def gradients_reaction(a, s, F, U0, W, L, shift):
    """For J = sum(W*U) over the solve (R): (U, lam, gF, gA, gU, gS, gshift), fields rounded to fp64, gshift in longdouble"""
    N = F.shape[0]
    U = np.asarray(rref.direct_solution(a, s, F, U0, L, shift)[0], dtype=np.float64)
    lam_ld = direct_adjoint(a, s, W, L, shift)[0]
    lam = np.asarray(lam_ld, dtype=np.float64)
    gS = source_gradient(N, "linear", 1.0, None, lam, U)[0]
    gshift = np.sum(lam_ld[1:-1, 1:-1] * np.asarray(U, dtype=LD)[1:-1, 1:-1])
    return U, lam, aref.zero_rim(lam), aref.coefficient_gradient(N, L, lam, U), aref.boundary_gradient(N, L, a, lam, W), gS, gshift


def gradients_newton(a, kind, kappa, w, F, U0, W, L, shift):
    """For J = sum(W*U) over the solve (N): (U, lam, gF, gA, gU, gW, gkappa), fields rounded to fp64, gkappa in longdouble"""
    N = F.shape[0]
    U_ld = nref.dense_newton(a, kind, kappa, w, F, U0, L, shift)[0]
    U = np.asarray(U_ld, dtype=np.float64)
    lam_ld = direct_adjoint(a, linearised_reaction(N, kind, kappa, w, U_ld), W, L, shift)[0]
    lam = np.asarray(lam_ld, dtype=np.float64)
    gW = source_gradient(N, kind, kappa, w, lam, U)[0]
    wn = np.ones((N, N), dtype=LD) if w is None else np.asarray(w, dtype=LD)
    gkappa = np.sum((wn * lam_ld * _g_ld(kind, U_ld))[1:-1, 1:-1])
    return U, lam, aref.zero_rim(lam), aref.coefficient_gradient(N, L, lam, U), aref.boundary_gradient(N, L, a, lam, W), gW, gkappa
