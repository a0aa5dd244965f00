"""Restatement of the pure Neumann problem (include/mg_singular.h), written from the header on numpy alone, over _bc_ref's
functions: the trapezoid weights, the weighted mean in the header's summation order (vectorised over the partition), the
projection, the coarse solve on a projected right-hand side, the cycle and the solve.  TEST INFRASTRUCTURE."""
import numpy as np

import _bc_ref as bref
import _solve_ref as ref
import _solve_vc_ref as vref

LD = ref.LD
U53 = ref.U53
BC = "nnnn"
DEFAULTS = dict(bref.DEFAULTS)
TB, ROWS, PAIR_MIN_N = 256, 4, 512


def weights(N, dtype=np.float64):
    """w[r][c] = wr[r]*wc[c], 1/2 at index 0 and N-1, 1 elsewhere"""
    w1 = np.ones(N, dtype=dtype)
    w1[0] = w1[-1] = 0.5
    return w1[:, None] * w1[None, :]


def sum_w(N):
    return float(N - 1) * float(N - 1)


def use_pairs(N):
    return N % 2 == 0 and N >= PAIR_MIN_N


def n_partials(N):
    cols = N // 2 if use_pairs(N) else N
    return ((cols + TB - 1) // TB) * ((N + ROWS - 1) // ROWS)


def _wave(v):
    """the header's wave step over the last axis (64 lanes): v[i] = v[i] + v[i+o] for o = 32 .. 1; returns v[0]"""
    assert v.shape[-1] == 64
    o = 32
    while o:
        v = v[..., :o] + v[..., o:2 * o]
        o //= 2
    return v[..., 0]


def _block(lanes):
    """the header's block step: lanes (..., T) with T a multiple of 64 -> s = 0.0; s = s + wave sum, waves in order"""
    T = lanes.shape[-1]
    waves = _wave(lanes.reshape(lanes.shape[:-1] + (T // 64, 64)))
    s = np.zeros(waves.shape[:-1])
    for i in range(T // 64):
        s = s + waves[..., i]
    return s


def partials(X):
    """partial[by*gx + bx] of the header's partition for X's size"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    N = X.shape[0]
    T = weights(N) * X   # (exact products)
    gy = (N + ROWS - 1) // ROWS
    if use_pairs(N):
        gx = (N // 2 + TB - 1) // TB
        P = np.zeros((gy * ROWS, gx * TB * 2))
        P[:N, :N] = T
        P = P.reshape(gy, ROWS, gx, TB, 2)
        acc = np.zeros((gy, gx, TB))
        for i in range(ROWS):
            acc = acc + P[:, i, :, :, 0]
            acc = acc + P[:, i, :, :, 1]
    else:
        gx = (N + TB - 1) // TB
        P = np.zeros((gy * ROWS, gx * TB))
        P[:N, :N] = T
        P = P.reshape(gy, ROWS, gx, TB)
        acc = np.zeros((gy, gx, TB))
        for i in range(ROWS):
            acc = acc + P[:, i]
    part = _block(acc).reshape(-1)
    assert part.size == n_partials(N)
    return part


def weighted_mean(X):
    """mean_w(X) in the header's order: partials, then the finish launch (1024 lanes striding the partials)"""
    N = np.asarray(X).shape[0]
    part = partials(X)
    k = (part.size + 1023) // 1024
    P = np.zeros(k * 1024)
    P[:part.size] = part
    P = P.reshape(k, 1024)
    acc = np.zeros(1024)
    for i in range(k):
        acc = acc + P[i]
    return float(_block(acc)) / sum_w(N)


def project_mean(X, mean=0.0):
    """(X - (mean_w(X) - mean), mean_w(X))"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    m = weighted_mean(X)
    return X - (m - float(mean)), m


def coarse_mean(F):
    """m_c of the coarse solve's prologue: T = min(1024, 64*ceil(M^2/64)) lanes, lane t sums p = t + j*T, j = 0 .. 3"""
    F = np.ascontiguousarray(F, dtype=np.float64)
    M = F.shape[0]
    n = M * M
    T = min(1024, (n + 63) // 64 * 64)
    assert 4 * T >= n
    P = np.zeros(4 * T)
    P[:n] = (weights(M) * F).reshape(-1)
    P = P.reshape(4, T)
    acc = np.zeros(T)
    for j in range(4):
        acc = acc + P[j]
    return float(_block(acc)) / sum_w(M)


def rbgs_trace(N, L, a, F, atol, rtol, max_iters):
    """the projected coarse solve: (U, err0, errs, m_c), _bc_ref.rbgs_trace on F - m_c"""
    m = coarse_mean(F)
    U, err0, errs = bref.rbgs_trace(N, L, BC, a, np.ascontiguousarray(F, dtype=np.float64) - m, atol, rtol, max_iters, 0.0)
    return U, err0, errs, m


def cycle(levels, F, U, L=1.0, margins=None, capped=None, rtable=None, ptable=None, iters=None, project=True, **opts):
    """_bc_ref.cycle with four Neumann sides at shift 0 and the projected coarse solve (project=False: the plain one)"""
    o = dict(DEFAULTS, **opts)
    sz = ref.sizes(F.shape[0], o["N_min"])
    nl = len(sz)
    A = levels if levels is not None else [None] * nl
    Us, Fs = [None] * nl, [None] * nl
    Fs[0] = np.ascontiguousarray(F, dtype=np.float64)
    for l in range(nl - 1):
        N, M = sz[l], sz[l + 1]
        Us[l] = bref.weighted_sweeps(N, L, BC, A[l], U if l == 0 else None, Fs[l], o["omega"], o["pre"], 0.0, zero_start=l > 0)
        D = bref.residual(N, L, BC, A[l], Us[l], Fs[l], 0.0, sign=-1)
        Fs[l + 1] = bref.restrict(D, M, BC, rtable(N, M) if rtable else None)
    if project:
        tr = rbgs_trace(sz[-1], L, A[-1], Fs[-1], o["coarse_atol"], o["coarse_rtol"], o["coarse_max_iters"])[:3]
    else:
        tr = bref.rbgs_trace(sz[-1], L, BC, A[-1], Fs[-1], o["coarse_atol"], o["coarse_rtol"], o["coarse_max_iters"], 0.0)
    Us[-1] = tr[0]
    if margins is not None:
        margins.append(vref.coarse_margin(tr, o["coarse_atol"], o["coarse_rtol"]))
    if capped is not None:
        capped.append(tr[2][-1] > max(o["coarse_atol"], o["coarse_rtol"] * tr[1]))
    if iters is not None:
        iters.append(len(tr[2]))
    for l in range(nl - 2, -1, -1):
        U_l = bref.prolong_add(Us[l + 1], sz[l], Us[l], BC, ptable(sz[l + 1], sz[l]) if ptable else None)
        Us[l] = bref.weighted_sweeps(sz[l], L, BC, A[l], U_l, Fs[l], o["omega"], o["post"], 0.0)
    return Us[0]


def solve(a, F, U, mean=0.0, L=1.0, margins=None, capped=None, rtable=None, ptable=None, iters=None, **opts):
    """A singular solve as the header states it.  Returns (U, history, cycles, converged, info) with info = dict(compat_defect,
    mean_before, Ft): the projection of F, the cycles on Ft under the stopping rule of the boundary path, the final shift."""
    o = dict(DEFAULTS, **opts)
    assert float(o.get("shift", 0.0)) == 0.0
    N = F.shape[0]
    levels = vref.coarsen_levels(a, o["N_min"], rtable) if a is not None else None
    Ft, c_F = project_mean(F, 0.0)
    U = np.zeros((N, N)) if U is None else np.array(U, dtype=np.float64, copy=True)
    tol = max(o["rtol"] * bref.ref_norm(Ft, BC), o["atol"])
    r = bref.residual_norm(N, L, BC, a, U, Ft, 0.0)
    history = [r]
    k = 0
    while not (r <= tol) and k < o["max_cycles"]:
        U = cycle(levels, Ft, U, L, margins=margins, capped=capped, rtable=rtable, ptable=ptable, iters=iters, **opts)
        r = bref.residual_norm(N, L, BC, a, U, Ft, 0.0)
        history.append(r)
        k += 1
    U, before = project_mean(U, mean)
    return U, history, k, r <= tol, dict(compat_defect=c_F, mean_before=before, Ft=Ft)


# ---------------------------------------------------------------- references in np.longdouble
def weighted_mean_ld(X):
    X = np.asarray(X, dtype=LD)
    N = X.shape[0]
    return np.sum(weights(N, LD) * X) / (LD(N - 1) * LD(N - 1))


def gamma(n):
    """gamma_n = n*u / (1 - n*u) in longdouble"""
    return LD(n) * U53 / (LD(1) - LD(n) * U53)


def bordered_solution(a, F, L, mean=0.0):
    """The solution of [[A, 1], [w^T/sw, 0]] [U; lam] = [F; mean] for four Neumann sides at sigma = 0, A assembled with
    _bc_ref.dense_operator: dense fp64 solve with longdouble refinement.  Returns (U (N x N, longdouble), lam, ||B||_inf) with B
    the U-from-F block of the bordered inverse (fp64 inverse)."""
    N = F.shape[0]
    n = N * N
    A, unk = bref.dense_operator(a, N, L, 0.0, BC)
    assert unk.size == n
    K = np.zeros((n + 1, n + 1), dtype=LD)
    K[:n, :n] = A
    K[:n, n] = LD(1)
    K[n, :n] = weights(N, LD).reshape(-1) / (LD(N - 1) * LD(N - 1))
    rhs = np.concatenate([np.asarray(F, dtype=LD).reshape(-1), [LD(mean)]])
    K64 = K.astype(np.float64)
    x = np.linalg.solve(K64, rhs.astype(np.float64)).astype(LD)
    for _ in range(3):
        x = x + np.linalg.solve(K64, (rhs - K @ x).astype(np.float64)).astype(LD)
    B = np.linalg.inv(K64)[:n, :n]
    return x[:n].reshape(N, N), x[n], LD(float(np.max(np.sum(np.abs(B), axis=1))))
