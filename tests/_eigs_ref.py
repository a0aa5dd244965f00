"""Restatement of the eigen-solver (include/mg_eigs.h) on numpy: LOBPCG on the basis [X, W, P] with _solve_vc_ref.cycle as the
preconditioner and the oracle's transfer operators, the Gram matrices, the Rayleigh-Ritz step and the rotation in the
header's order.  The small dense eigenproblems of the Rayleigh-Ritz step go through numpy.linalg.eigh where the engine runs
its own Jacobi routine: both are backward stable, the step is specified through its result (tests/test_eigs_cpu.py holds the
engine's against this one), and iteration counts of the two may differ by one or two.
The second half holds the references that share no code with the engine: the dense (N-2)^2 matrix assembled in longdouble
from a, L and N alone (as _solve_vc_ref.direct_solution assembles it) with numpy.linalg.eigvalsh, the closed form for
a == 1, and -- for the sizes no dense matrix reaches -- the exact spectrum of a coefficient that is constant along one axis,
by separation of variables (written from include/mg_varcoef.h's face means and the mathematics alone).  TEST INFRASTRUCTURE."""
import functools
import math

import numpy as np

import _solve_ref as ref
import _solve_vc_ref as vc
import _synth

LD = np.longdouble
U53 = 2.0 ** -53
MAX_BLOCK = 12
DROP = 1e-12


def default_guard(k):
    return min(max(2, k // 2), MAX_BLOCK - k)


def gamma(n):
    return n * U53 / (1.0 - n * U53)


def inner(x):
    return x[..., 1:-1, 1:-1]


def dot(x, y):
    return float(np.sum(inner(x) * inner(y)))


def dot_ld(x, y):
    return np.sum(inner(np.asarray(x, dtype=LD)) * inner(np.asarray(y, dtype=LD)))


def sum_bound(N, x, y):
    """the header's bound: |fp64 sum of rounded products in any order - exact sum| <= n*u/(1 - n*u) * sum|x*y|, n = (N-2)^2"""
    n = (N - 2) * (N - 2)
    return gamma(n) * float(np.sum(np.abs(inner(np.asarray(x, dtype=LD)) * inner(np.asarray(y, dtype=LD)))))


def apply(N, L, a, X):
    """AA*x = -(inv*b(x)) inside, +0 on the rim"""
    out = np.zeros((N, N))
    out[1:-1, 1:-1] = -vc.apply_operator(N, L, a, X)[1:-1, 1:-1]
    return out


def gram(S, AS):
    m = len(S)
    G, H = np.zeros((m, m)), np.zeros((m, m))
    for j in range(m):
        for l in range(j, m):
            G[j, l] = G[l, j] = dot(S[j], S[l])
            H[j, l] = H[l, j] = dot(S[j], AS[l])
    return G, H


def rayleigh_ritz(G, H, p, drop=DROP):
    """(kept, C, Cp, theta) of the header's step; kept < p: the breakdown, the rest None"""
    m = G.shape[0]
    g = np.diag(G)
    if not (np.all(np.isfinite(g)) and np.all(g > 0)):
        return 0, None, None, None
    d = 1.0 / np.sqrt(g)
    Gh, Hh = d[:, None] * G * d[None, :], d[:, None] * H * d[None, :]
    w, V = np.linalg.eigh(0.5 * (Gh + Gh.T))
    keep = w > drop * w.max()
    kept = int(keep.sum())
    if kept < p:
        return kept, None, None, None
    T = V[:, keep] / np.sqrt(w[keep])[None, :]
    A2 = T.T @ Hh @ T
    theta, Y = np.linalg.eigh(0.5 * (A2 + A2.T))
    C = d[:, None] * (T @ Y[:, :p])
    Cp = C.copy()
    Cp[:p] = 0.0
    return kept, C, Cp, theta[:p].copy()


def rotate(C, Cp, theta, S, AS):
    """The rotation, bit for bit: every output the sum over j = 0 .. m-1 in this order from +0, products and sums rounded once.
    Returns (X', AX', P', AP', R, res2), interiors set, rims +0."""
    m, p = C.shape
    N = S[0].shape[0]
    out = [np.zeros((p, N, N)) for _ in range(5)]
    res2 = np.zeros(p)
    Si = [inner(np.asarray(s, dtype=np.float64)) for s in S[:m]]
    Ai = [inner(np.asarray(s, dtype=np.float64)) for s in AS[:m]]
    for i in range(p):
        x, ax, pp, ap = (np.zeros((N - 2, N - 2)) for _ in range(4))
        for j in range(m):
            x = x + C[j, i] * Si[j]
            ax = ax + C[j, i] * Ai[j]
            pp = pp + Cp[j, i] * Si[j]
            ap = ap + Cp[j, i] * Ai[j]
        r = ax - theta[i] * x
        for o, v in zip(out, (x, ax, pp, ap, r)):
            o[i, 1:-1, 1:-1] = v
        res2[i] = float(np.sum(r * r))
    return (*out, res2)


def start(N, p, k, seed, X0=None):
    X = np.zeros((p, N, N))
    for i in range(p):
        if X0 is not None and i < k:
            X[i, 1:-1, 1:-1] = X0[i][1:-1, 1:-1]
        else:
            X[i, 1:-1, 1:-1] = (_synth.hash_field(N, seed + i) - 0.5)[1:-1, 1:-1]
    return X


def solve(orc, a, N, L=1.0, k=1, guard=None, rtol=1e-8, atol=0.0, max_iters=60, seed=0, X0=None, blocks=3, **cycle_opts):
    """(lam, X, info): the loop of include/mg_eigs.h.  blocks=2 leaves P out (block steepest descent: the comparison of DESIGN)."""
    guard = default_guard(k) if guard is None else guard
    p = k + guard
    o = dict(vc.DEFAULTS, **cycle_opts)
    levels = vc.coarsen_levels(np.ones((N, N)) if a is None else a, o["N_min"])
    pre = lambda r: vc.cycle(orc, levels, r, np.zeros((N, N)), L, **cycle_opts)
    A = lambda x: apply(N, L, a, x)
    X = start(N, p, k, seed, X0)
    AX = np.stack([A(x) for x in X])
    S, AS = list(X), list(AX)
    it, restarts, history = 0, 0, []
    theta, res = np.zeros(p), np.full(p, np.inf)
    converged = breakdown = False
    locked, prev_res = [False] * p, np.full(p, np.inf)

    def met(res):
        return all(res[i] <= max(rtol * theta[i], atol) for i in range(k))

    def recompute():
        """everything that is reported, from X alone: AX, the Rayleigh quotients (into theta), R and res"""
        AXn = np.stack([A(x) for x in X])
        theta[:] = [dot(x, ax) / dot(x, x) for x, ax in zip(X, AXn)]
        R = AXn - theta[:, None, None] * X
        return AXn, R, np.sqrt(np.array([dot(r, r) for r in R]))

    while True:
        G, H = gram(S, AS)
        act = np.array([j < p or not locked[j % p] for j in range(len(S))])   # soft locking (include/mg_eigs.h)
        kept, Ca, Cpa, th = rayleigh_ritz(G[np.ix_(act, act)], H[np.ix_(act, act)], p)
        if kept >= p:
            C, Cp = np.zeros((len(S), p)), np.zeros((len(S), p))
            C[act], Cp[act] = Ca, Cpa
        if kept < p:
            breakdown = True
            history.append(dict(theta=None, res=None, kept=kept, restarted=False))
            break
        theta = th
        X, AX, P, AP, R, res2 = rotate(C, Cp, theta, S, AS)
        res = np.sqrt(res2)
        locked = [bool(res[i] <= max(rtol * theta[i], atol) and (locked[i] or res[i] >= prev_res[i])) for i in range(p)]
        prev_res = res.copy()
        have_p = len(S) > p and blocks == 3
        history.append(dict(theta=theta[:k].copy(), res=res[:k].copy(), kept=kept, restarted=False))
        recomputed = False
        if met(res):
            AX, R, res = recompute()
            recomputed = True
            if met(res):
                converged = True
                break
            have_p = False
            restarts += 1
            history[-1]["restarted"] = True
        if it == max_iters:
            break
        W = np.stack([pre(r) for r in R])
        AW = np.stack([A(w) for w in W])
        it += 1
        S = list(X) + list(W) + (list(P) if have_p else [])
        AS = list(AX) + list(AW) + (list(AP) if have_p else [])
        recomputed = False
    if not recomputed:
        AX, R, res = recompute()
    info = dict(iters=it, converged=converged, breakdown=breakdown, restarts=restarts, cycles=p * it, res=res[:k].copy(),
                history=history)
    return theta[:k].copy(), X[:k].copy(), info


# ---------------------------------------------------------------- references that share no code with the engine
def dense_matrix(a, N, L):
    """-div_h(a grad_h .) on the (N-2)^2 interior unknowns with a zero rim, assembled in longdouble from a, L and N alone"""
    n = N - 2
    a = np.ones((N, N), dtype=LD) if a is None else np.asarray(a, dtype=LD)
    h = LD(L) / LD(N - 1)
    inv = LD(1) / (h * h)
    half = LD(1) / LD(2)
    ctr = a[1:-1, 1:-1]
    faces = ((half * (ctr + a[2:, 1:-1]), 1, 0), (half * (ctr + a[:-2, 1:-1]), -1, 0), (half * (ctr + a[1:-1, 2:]), 0, 1),
             (half * (ctr + a[1:-1, :-2]), 0, -1))
    idx = np.arange(n * n).reshape(n, n)
    M = np.zeros((n * n, n * n), dtype=LD)
    M[idx, idx] = inv * (faces[0][0] + faces[1][0] + faces[2][0] + faces[3][0])
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    for f, dr, dc in faces:
        ok = (ii + dr >= 0) & (ii + dr < n) & (jj + dc >= 0) & (jj + dc < n)
        M[idx[ii[ok], jj[ok]], idx[ii[ok] + dr, jj[ok] + dc]] = -inv * f[ok]
    return M


@functools.lru_cache(maxsize=None)
def _dense_eigenvalues_cached(name, N, L, seed):
    a = None if name is None else vc.field(name, N, L, seed)
    return np.linalg.eigvalsh(dense_matrix(a, N, L).astype(np.float64))


def dense_eigenvalues(name, N, L=1.0, seed=0, count=None):
    """ascending eigenvalues of the dense matrix of _solve_vc_ref.field(name, N, L, seed) (name None: a = 1), computed once per
    process and shared.  eigvalsh on the fp64 rounding of the matrix: within about (N-2)^2*u*||M|| of the exact ones, which
    the tests' rounding term covers."""
    w = _dense_eigenvalues_cached(name, N, float(L), seed)
    return w if count is None else w[:count]


def quadratic_bound_left_out(sizes, fields, blocks, rtol, seed=1):
    """the (N, field, k, guard) of the table whose k-th gap does not exceed 4*rtol*sqrt(sum_{i<k} lam_i^2) on the dense
    reference: a converged solve has ||R||_F at most that, so only these can miss the gap condition of the quadratic bound"""
    out = []
    for N in sizes:
        for name in fields:
            lam = dense_eigenvalues(name, N, 1.0, seed, 13)
            for k, guard in blocks:
                if not lam[k] - lam[k - 1] > 4.0 * rtol * float(np.sqrt(np.sum(lam[:k] ** 2))):
                    out.append((N, name, k, guard))
    return out


def closed_form(N, L=1.0, count=None):
    """lambda_ij = (4/dx^2)(sin^2(i*pi/(2(N-1))) + sin^2(j*pi/(2(N-1)))), i, j = 1 .. N-2, ascending"""
    dx = L / (N - 1)
    s = np.array([math.sin(i * math.pi / (2.0 * (N - 1))) ** 2 for i in range(1, N - 1)])
    lam = np.sort((4.0 / (dx * dx)) * (s[:, None] + s[None, :]), axis=None)
    return lam if count is None else lam[:count]


# ---------------------------------------------------------------- layered coefficients: an exact reference at any N
# a[r, c] = p[c] ("cols") or p[r] ("rows"): constant along one axis.  The header's arithmetic face means across the constant
# axis are 0.5*(p + p) = p itself, so -div_h(a grad_h .) = inv*(T_p (x) I + diag(p) (x) T) with T = tridiag(-1, 2, -1) along
# the constant axis and T_p the three-point operator of p along the other one (diagonal aE + aW, off-diagonal -aE,
# aE = 0.5*(p[c] + p[c+1]), aW = 0.5*(p[c] + p[c-1])).  The sine modes of T, mu_j = 4 sin^2(j*pi/(2(N-1))), block-diagonalise
# it: the spectrum is the union over j = 1 .. N-2 of the eigenvalues of the (N-2) x (N-2) symmetric tridiagonal
# inv*(T_p + mu_j*diag(p)).  The transpose of a has the same spectrum: one reference serves both orientations.
PROFILES = ("one", "smooth", "jump")


def profile(name, N):
    """p at the N points of one axis.  smooth: 2 + sin(2*pi*t + 0.5), contrast 3, not symmetric about the middle; jump: 1
    below the index j0, 10 from it on, j0 odd (the odd index next to 0.37*(N-1)): a column pair (j0 - 1, j0) straddles it."""
    t = np.arange(N) / float(N - 1)
    if name == "one":
        return np.ones(N)
    if name == "smooth":
        return 2.0 + np.sin(2.0 * np.pi * t + 0.5)
    if name == "jump":
        j0 = 2 * (int(0.37 * (N - 1)) // 2) + 1
        return np.where(np.arange(N) < j0, 1.0, 10.0)
    raise ValueError(name)


def layered(name, N, axis):
    """the N x N coefficient of profile(name, N): axis "cols": a[r, c] = p[c]; "rows": a[r, c] = p[r]"""
    p = profile(name, N)
    a = np.empty((N, N))
    a[:, :] = p[None, :] if axis == "cols" else p[:, None]
    return a


@functools.lru_cache(maxsize=None)
def _separated_cached(name, N, L, count):
    p = np.asarray(profile(name, N), dtype=LD)
    h = LD(L) / LD(N - 1)
    inv = LD(1) / (h * h)
    half = LD(1) / LD(2)
    aE, aW = half * (p[1:-1] + p[2:]), half * (p[1:-1] + p[:-2])
    n = N - 2
    Tp = np.zeros((n, n), dtype=LD)
    i = np.arange(n)
    Tp[i, i] = aE + aW
    Tp[i[:-1], i[:-1] + 1] = Tp[i[:-1] + 1, i[:-1]] = -aE[:-1]
    D = np.zeros((n, n), dtype=LD)
    D[i, i] = p[1:-1]
    pmin = float(np.min(p))
    found = np.zeros(0)
    for j in range(1, N - 1):
        s = np.sin(LD(j) * LD(np.pi) / LD(2 * (N - 1)))
        mu = LD(4) * s * s
        # every eigenvalue of block j is at least inv*mu_j*min(p), T_p being positive semidefinite, and mu_j grows with j
        if found.size >= count and float(inv * mu) * pmin > found[count - 1]:
            break
        w = np.linalg.eigvalsh((inv * (Tp + mu * D)).astype(np.float64))
        found = np.sort(np.concatenate([found, w[:count]]))[:count]
    return found


def separated_eigenvalues(name, N, L=1.0, count=13):
    """the `count` lowest eigenvalues, ascending, of -div_h(a grad_h .) for a = layered(name, N, either axis): blocks assembled
    in longdouble, rounded to fp64, numpy.linalg.eigvalsh on each (dimension N-2: within about (N-2)*u*||block|| of exact)"""
    return _separated_cached(name, N, float(L), int(count)).copy()


def residuals_ld(a, N, L, lam, X):
    """||AA x_i - lam_i x_i|| over the interior, every operation in longdouble (flux form, _solve_vc_ref._residual_ld)"""
    zero = np.zeros((N, N))
    out = []
    for l, x in zip(lam, X):
        r = -vc._residual_ld(np.ones((N, N)) if a is None else a, x, zero, L, 0.0) - LD(l) * np.asarray(x, dtype=LD)[1:-1, 1:-1]
        out.append(np.sqrt(np.sum(r * r)))
    return np.array(out, dtype=LD)
