"""Restatement of the semilinear solve div(a grad U) - sigma*U - kappa*w*g(U) = F, written from include/mg_newton.h on numpy:
the pass (trial value, S = kappa*w*g'(v), D = (F + kappa*w*g(v)) - inv*b(v), the norm in the device's order) and the Newton
driver with its backtracking line search around the restated reaction solver (_reaction_ref: operator, solve, krylov_solve,
engine_norm).  exp is math.exp per element: the host libm the device's exp_libm is held against.  The last part holds a
dense Newton solution in longdouble, which shares no code with the engine.  TEST INFRASTRUCTURE."""
import math

import numpy as np

import _reaction_ref as rref
import _solve_ref as ref
import _solve_vc_ref as vref

LD = ref.LD
KINDS = ("cubic", "sinh", "exp")
CONVERGED, NOT_CONVERGED, STALLED = 0, -1, -2
NEWTON_DEFAULTS = dict(rtol=1e-8, atol=0.0, max_iters=20, max_backtracks=12)


EXP_MAX = 709.782712893384   # the largest double whose exp is finite


def _exp(v):
    """libm's exp per element (math.exp), +inf past EXP_MAX as libm gives it"""
    v = np.asarray(v, dtype=np.float64)
    over = v > EXP_MAX
    e = np.fromiter(map(math.exp, np.where(over, 0.0, v).reshape(-1).tolist()), dtype=np.float64, count=v.size).reshape(v.shape)
    e[over] = math.inf
    return e


def g_gp(kind, v):
    """(g(v), g'(v)) by the header's table, every operation rounded once"""
    if kind == "cubic":
        q = v * v
        return q * v, 3.0 * q
    if kind == "sinh":
        e = _exp(v)
        f = 1.0 / e
        return 0.5 * (e - f), 0.5 * (e + f)
    if kind == "exp":
        e = _exp(v)
        return e, e
    raise ValueError(kind)


def trial(U, dlt, t):
    """v: U + t*dlt inside (the product rounded, then the sum), U on the rim"""
    U = np.ascontiguousarray(U, dtype=np.float64)
    V = U.copy()
    if dlt is not None:
        V[1:-1, 1:-1] = U[1:-1, 1:-1] + t * np.ascontiguousarray(dlt, dtype=np.float64)[1:-1, 1:-1]
    return V


def residual(N, L, a, kind, kappa, w, U, F, shift=0.0, dlt=None, t=1.0):
    """(V, D, S, norm) of one pass"""
    V = trial(U, dlt, t)
    kw = float(kappa) if w is None else float(kappa) * np.ascontiguousarray(w, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):   # (a rejected trial may overflow: the norm says so)
        g, gp = g_gp(kind, V)
        S = kw * gp * np.ones((N, N))
        lin = vref.apply_operator(N, L, a, V, shift)
        D = np.zeros((N, N))
        D[1:-1, 1:-1] = ((F + kw * g) - lin)[1:-1, 1:-1]
        norm = rref.engine_norm(D)
    return V, D, S, norm


def newton(orc, a, kind, kappa, w, F, U=None, L=1.0, krylov=0, table=None, margins=None, keep=None, rtol=1e-8, atol=0.0,
           max_iters=20, max_backtracks=12, inner=None):
    """The driver of include/mg_newton.h.  inner: the options of the solver the steps run on (shift, rtol, max_cycles, ...).  Returns a dict with U,
    status, iterations, converged, res0, res, history (norms) and steps (res, t, backtracks, inner_cycles, inner_converged per
    iteration); keep: a list that receives U after every accepted iteration."""
    opts = dict(inner or {})
    sh = float(dict(rref.DEFAULTS, **opts)["shift"])
    N = F.shape[0]
    U = np.zeros((N, N)) if U is None else np.array(U, dtype=np.float64, copy=True)
    _, D, S, r = residual(N, L, a, kind, kappa, w, U, F, sh)
    assert math.isfinite(r), "the residual of the start is not finite"
    res0 = r
    tol = max(atol, rtol * r)
    history, steps, its, stalled = [r], [], 0, False
    while not (r <= tol) and its < max_iters:
        if krylov:
            out = rref.krylov_solve(orc, a, S, D, np.zeros((N, N)), L, m=krylov, margins=margins, table=table, **opts)
            dlt, cycles, conv = out["U"], out["cycles"], out["converged"]
        else:
            dlt, _, cycles, conv = rref.solve(orc, a, S, D, np.zeros((N, N)), L, margins=margins, table=table, engine_norms=True, **opts)
        step = dict(res=r, t=0.0, backtracks=0, inner_cycles=cycles, inner_converged=bool(conv))
        t, accepted = 1.0, False
        while True:
            V, D2, S2, rt = residual(N, L, a, kind, kappa, w, U, F, sh, dlt, t)
            if math.isfinite(rt) and rt < (1.0 - 1e-4 * t) * r:
                U, D, S, r = V, D2, S2, rt
                step.update(res=rt, t=t)
                accepted = True
                break
            step["backtracks"] += 1
            if step["backtracks"] > max_backtracks:
                break
            t *= 0.5
        steps.append(step)
        if not accepted:
            stalled = True
            break
        its += 1
        history.append(r)
        if keep is not None:
            keep.append(U)
    conv = r <= tol
    return dict(U=U, status=CONVERGED if conv else STALLED if stalled else NOT_CONVERGED, iterations=its, converged=conv,
                res0=res0, res=r, history=history, steps=steps)


# ---------------------------------------------------------------- the problems of the tests
def smooth_weight(N, L=1.0):
    x, y = vref.grid(N, L)
    return 1.0 + 0.5 * np.cos(2 * np.pi * x) * np.sin(np.pi * y)


def manufactured(N, kind, kappa, amp=1.0):
    """u* = amp sin(pi x) sin(2 pi y) on the unit square, a = 1, w = 1, sigma = 0: (u*, F = Laplace(u*) - kappa*g(u*))"""
    x, y = vref.grid(N, 1.0)
    u = amp * np.sin(np.pi * x) * np.sin(2 * np.pi * y)
    return u, -5.0 * np.pi ** 2 * u - kappa * g_gp(kind, u)[0]


def problem(N, L=1.0):
    """(F, U0): a right-hand side that makes |u| of order one, and a start that is zero inside with rim data of order one"""
    x, y = vref.grid(N, L)
    F = -40.0 * np.sin(np.pi * x / L) * np.sin(2 * np.pi * y / L) + 5.0 * np.random.default_rng(N).standard_normal((N, N))
    return F, ref.rim_only(np.cos(3.0 * x) * (1.0 - 0.5 * y))


HARD_STARTS = {"cubic": -1e6, "sinh": -1e4, "exp": -1e4}   # F == this constant, kappa = 1, from U = 0


# ---------------------------------------------------------------- truth: dense Newton in longdouble
def _g_ld(kind, v):
    v = np.asarray(v, dtype=LD)
    if kind == "cubic":
        return v * v * v, 3 * v * v
    e = np.exp(v)
    if kind == "sinh":
        return (e - 1 / e) / 2, (e + 1 / e) / 2
    return e, e


def residual_ld(a, kind, kappa, w, U, F, L, shift):
    """N(U) = div_h(a grad_h U) - sigma*U - kappa*w*g(U) - F on the interior in flux form, every operation in longdouble"""
    N = F.shape[0]
    wi = LD(1) if w is None else np.asarray(w, dtype=LD)[1:-1, 1:-1]
    g = _g_ld(kind, np.asarray(U, dtype=LD)[1:-1, 1:-1])[0]
    return vref._residual_ld(rref.ones_if_none(a, N), U, F, L, shift) - LD(kappa) * wi * g


def dense_newton(a, kind, kappa, w, F, U, L, shift, iters=60, chord=False):
    """(X, ||A^-1||_inf): the solution of the discrete nonlinear system with U's rim as data, by exact Newton steps with a
    halving line search on the longdouble residual, each step a dense solve (fp64 inverse of the longdouble-assembled Jacobian,
    longdouble refinement); and the infinity norm of the inverse of the LINEAR part A (s = 0), which dominates the inverse of
    every A - diag(kappa*w*g'(xi)), an M-matrix with a larger diagonal.  chord: U is already close to the solution (a converged
    solve to be judged): the Jacobian of the start is inverted once and kept, which converges from there and costs one inverse."""
    N = F.shape[0]
    n = N - 2
    X = np.array(U, dtype=LD)
    wn = np.ones((N, N), dtype=LD) if w is None else np.asarray(w, dtype=LD)
    M0 = rref.dense_operator(a, np.zeros((N, N)), N, L, shift)[0]
    nA = LD(float(np.max(np.sum(np.abs(np.linalg.inv(M0.astype(np.float64))), axis=1))))
    idx = np.arange(n * n)
    r = residual_ld(a, kind, kappa, w, X, F, L, shift)
    Jinv = None
    for _ in range(iters):
        rn = np.max(np.abs(r))
        if Jinv is None or not chord:
            J = M0.copy()                               # -(A - S) = M0 + diag(S)
            J[idx, idx] += (LD(kappa) * wn * _g_ld(kind, X)[1])[1:-1, 1:-1].reshape(-1)
            Jinv = np.linalg.inv(J.astype(np.float64))
        rhs = r.reshape(-1)                             # (A - S) d = -N(X)  <=>  J d = N(X)
        d = (Jinv @ rhs.astype(np.float64)).astype(LD)
        for _ in range(3):
            d = d + (Jinv @ (rhs - J @ d).astype(np.float64)).astype(LD)
        t = LD(1)
        while True:
            Y = X.copy()
            Y[1:-1, 1:-1] += t * d.reshape(n, n)
            ry = residual_ld(a, kind, kappa, w, Y, F, L, shift)
            if np.all(np.isfinite(ry)) and np.max(np.abs(ry)) < rn:
                break
            t = t / 2
            if t < LD(2) ** -40:
                return X, nA                            # no representable improvement is left
        X, r = Y, ry
    return X, nA
