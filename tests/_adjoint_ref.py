"""Restatement of the adjoint sensitivities of include/mg_adjoint.h on numpy: the two point kernels in the header's order
(every difference, product and sum rounded once), the dense adjoint solve that goes with tests/_solve_vc_ref.direct_solution,
and the a-priori error bounds of the GPU truth test.  TEST INFRASTRUCTURE.

Rows are the first index: N is row r+1, S is row r-1, E is column c+1, W is column c-1."""
import numpy as np

import _solve_vc_ref as vref

LD = vref.LD
U53 = vref.U53


def inv_of(N, L):
    """the level-0 constant of the solvers: inv = 1/dx2, dx2 = (L/(N-1))^2, each operation rounded once"""
    return vref.level_consts(N, L, 0.0)[1]


def zero_rim(lam):
    """lam' of the header: lam with every rim value replaced by +0.0"""
    out = np.zeros_like(np.asarray(lam, dtype=np.float64))
    out[1:-1, 1:-1] = np.asarray(lam, dtype=np.float64)[1:-1, 1:-1]
    return out


def coefficient_gradient(N, L, lam, U):
    """gA_k = h*((((0.0 + tN) + tS) + tE) + tW) at every grid point, tX = (lam'_k - lam'_q)*(U_k - U_q), +0.0 when the
    neighbour q lies outside the grid; h = 0.5*inv."""
    h = 0.5 * inv_of(N, L)
    lp = zero_rim(lam)
    U = np.ascontiguousarray(U, dtype=np.float64)
    tN, tS, tE, tW = (np.zeros((N, N)) for _ in range(4))
    tN[:-1, :] = (lp[:-1, :] - lp[1:, :]) * (U[:-1, :] - U[1:, :])
    tS[1:, :] = (lp[1:, :] - lp[:-1, :]) * (U[1:, :] - U[:-1, :])
    tE[:, :-1] = (lp[:, :-1] - lp[:, 1:]) * (U[:, :-1] - U[:, 1:])
    tW[:, 1:] = (lp[:, 1:] - lp[:, :-1]) * (U[:, 1:] - U[:, :-1])
    return h * ((((0.0 + tN) + tS) + tE) + tW)


def boundary_gradient(N, L, a, lam, Ubar):
    """gU: +0.0 inside, Ubar (or +0.0) at the corners, Ubar[b] - inv*(f*lam[p]) at a rim point b with interior neighbour p,
    f = 0.5*(a[b] + a[p]) (a = None: 1.0); Ubar = None: 0.0."""
    inv = inv_of(N, L)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    g = np.zeros((N, N))
    ub = np.zeros((N, N)) if Ubar is None else np.ascontiguousarray(Ubar, dtype=np.float64)
    for edge in (0, N - 1):
        g[edge, :] = ub[edge, :]
        g[:, edge] = ub[:, edge]

    def f(b, p):
        return 1.0 if a is None else 0.5 * (a[b] + a[p])

    s = slice(1, N - 1)
    for b, p in (((0, s), (1, s)), ((N - 1, s), (N - 2, s)), ((s, 0), (s, 1)), ((s, N - 1), (s, N - 2))):
        g[b] = ub[b] - inv * (f(b, p) * lam[p])
    return g


# ---------------------------------------------------------------- dense references (small N)
def direct_adjoint(a, Ubar, L, shift):
    """The adjoint field of the discrete problem by the dense solve of _solve_vc_ref: the forward equation with right-hand
    side Ubar and a zero rim (the operator is symmetric on the interior).  Returned in longdouble."""
    N = Ubar.shape[0]
    return vref.direct_solution(a, Ubar, np.zeros((N, N)), L, shift)


def gradients(a, F, U0, W, L, shift):
    """For J = sum(W*U): (U, lam, gF, gA, gU) through the dense solves and the restatement (fp64 arrays; U and lam are the
    dense solutions rounded to fp64)."""
    N = F.shape[0]
    U = np.asarray(vref.direct_solution(a, F, U0, L, shift), dtype=np.float64)
    lam = np.asarray(direct_adjoint(a, W, L, shift), dtype=np.float64)
    return U, lam, zero_rim(lam), coefficient_gradient(N, L, lam, U), boundary_gradient(N, L, a, lam, W)


# ---------------------------------------------------------------- a-priori bounds of the truth test
def lambda1(N, L):
    """the smallest eigenvalue of -Laplace_h on the (N-2)^2 interior points, spacing L/(N-1)"""
    h = L / float(N - 1)
    return 8.0 / (h * h) * np.sin(np.pi / (2.0 * (N - 1))) ** 2


def mu(a, N, L, shift):
    """a lower bound of the smallest eigenvalue of -(A_h - shift): a_min*lambda_1 + shift (every face value >= a_min)"""
    return float(np.min(a)) * lambda1(N, L) + shift


def max_diff(X):
    X = np.asarray(X, dtype=np.float64)
    return max(float(np.max(np.abs(X[1:, :] - X[:-1, :]))), float(np.max(np.abs(X[:, 1:] - X[:, :-1]))))


def gA_bound(N, L, U, lam, e_U, e_lam):
    """|gA_k(computed fields) - gA_k(exact fields)| for fields whose errors are at most e_U, e_lam at every point (an l2 norm
    bounds the max norm), plus the rounding of the expression itself.
    Each of the four terms is (dl + el)*(du + eu) with |el| <= 2 e_lam, |eu| <= 2 e_U: it moves by at most
    2 e_lam |du| + 2 e_U |dl| + 4 e_lam e_U.  Rounding: two differences, one product, four sums and the product with h put at
    most 8 relative roundings on a term, bounded by 8 u * 4 * max|dl| max|du| for the point (with the perturbed maxima)."""
    h = 0.5 * inv_of(N, L)
    dU, dl = max_diff(U), max_diff(zero_rim(lam))
    pert = 2.0 * e_lam * dU + 2.0 * e_U * dl + 4.0 * e_lam * e_U
    return h * 4.0 * (pert + 8.0 * float(U53) * (dl + 2.0 * e_lam) * (dU + 2.0 * e_U))


def gU_bound(N, L, a, lam, Ubar, e_lam):
    """|gU_b(computed lam) - gU_b(exact lam)| <= inv*a_max*e_lam plus the rounding of Ubar - inv*(f*lam): 4 roundings on the
    product term, one on the difference."""
    inv = inv_of(N, L)
    amax = 1.0 if a is None else float(np.max(a))
    lmax = float(np.max(np.abs(lam))) + e_lam
    ub = 0.0 if Ubar is None else float(np.max(np.abs(Ubar)))
    return inv * amax * e_lam + float(U53) * (5.0 * inv * amax * lmax + ub)
