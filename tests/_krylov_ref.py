"""Restatement of the Krylov acceleration of the residual-tolerance solver, restarted GCR(m) around the V-cycle, written from
include/mg_krylov.h on numpy, the restatement of the cycle (_solve_vc_ref: with a == 1 it is the constant solver bit for bit)
and the oracle's transfer operators.  Two modes:

    solve(...)            every sum is numpy's own (pairwise) sum over the interior
    solve(..., log=...)   a REPLAY: the same vector updates, but d_j, g, h, rho_rec and the recomputed rho of every iteration
                          are taken from an engine log (Solver.krylov_log()), so that the vectors can be compared bit for
                          bit although the engine sums in another order.  b_j = d_j*w_j, w = 1/g and alpha = h*w are
                          formed here, in fp64, one rounding each.

Either mode records, per iteration, its own longdouble sums over its own vectors with the sum of the absolute products: the
a-priori bound of the header, n*u/(1 - n*u)*sum|x*y| with n = (N-2)^2, holds for any summation order, so a logged sum is
checked against them without measuring anything.  TEST INFRASTRUCTURE."""
import numpy as np

import _solve_ref as ref
import _solve_vc_ref as vref

LD = ref.LD
U53 = ref.U53
MAX_M = 16


def gamma(n):
    nu = LD(n) * U53
    return nu / (LD(1) - nu)


def inner(x):
    return x[1:-1, 1:-1]


def dot(x, y):
    """<x, y> over the interior, numpy's summation"""
    return float(np.sum(inner(x) * inner(y)))


def dot_ld(x, y):
    """(<x, y>, sum|x*y|) over the interior, products and sums in longdouble"""
    p = inner(np.asarray(x, dtype=LD)) * inner(np.asarray(y, dtype=LD))
    return np.sum(p), np.sum(np.abs(p))


def sum_bound(N, abs_sum):
    """the header's bound on |any fp64 summation of the rounded products - the exact sum|: one rounding per product and
    n - 1 additions, n = (N-2)^2 terms"""
    return gamma((N - 2) * (N - 2)) * abs_sum


def orthogonalise(q, z, b, Q, Z):
    """q -= b[j]*Q[j], z -= b[j]*Z[j] for j in order, interior only, in place (product and difference rounded once each)"""
    for bj, Qj, Zj in zip(b, Q, Z):
        bj = np.float64(bj)
        inner(q)[...] = inner(q) - bj * inner(Qj)
        inner(z)[...] = inner(z) - bj * inner(Zj)


def update(alpha, U, z, r, q):
    """U += alpha*z, r -= alpha*q on the interior, in place; alpha == 0 keeps both"""
    alpha = np.float64(alpha)
    if alpha != 0.0:
        inner(U)[...] = inner(U) + alpha * inner(z)
        inner(r)[...] = inner(r) - alpha * inner(q)


def step_scalars(g, h):
    """(w, alpha, breakdown) of the header from g and h"""
    with np.errstate(all="ignore"):
        g, h = np.float64(g), np.float64(h)
        w = np.float64(1.0) / g
        alpha = h * w
    bad = (not g > 0.0) or (not np.isfinite(g)) or (not np.isfinite(alpha))
    return w, (np.float64(0.0) if bad else alpha), bool(bad)


def solve(orc, a, F, U=None, L=1.0, m=8, log=None, margins=None, table=None, **opts):
    """Returns dict(U, history, cycles, converged, breakdown, records).  a = None: the constant operator (a == 1).
    records[i]: k, restarted, and the longdouble sums of iteration i over this restatement's vectors -- d, g, h, rr as
    (sum, sum of absolute products) -- and rho_own, the restatement's recomputed norm where the iteration restarted."""
    o = dict(vref.DEFAULTS, **opts)
    assert 1 <= m <= MAX_M
    sh = float(o["shift"])
    N = F.shape[0]
    A = np.ones((N, N)) if a is None else np.ascontiguousarray(a, dtype=np.float64)
    levels = vref.coarsen_levels(A, o["N_min"], table)
    U = np.zeros((N, N)) if U is None else np.array(U, dtype=np.float64, copy=True)
    tol = max(o["rtol"] * ref.ref_norm(F), o["atol"])
    rho = vref.residual_norm(N, L, A, U, F, sh)
    history, records = [rho], []
    Z, Q, w = [None] * m, [None] * m, [None] * m
    cycles, k, breakdown = 0, 0, False
    r = None
    if not (rho <= tol) and cycles < o["max_cycles"]:
        r = vref.residual(N, L, A, U, F, sh, sign=-1)
    while not (rho <= tol) and cycles < o["max_cycles"]:
        e = log[cycles] if log is not None else None
        z = vref.cycle(orc, levels, r, np.zeros((N, N)), L, margins=margins, **opts)
        q = vref.apply_operator(N, L, A, z, sh)
        rec = dict(k=k, d=[dot_ld(q, Q[j]) for j in range(k)])
        d = list(e["d"]) if e else [dot(q, Q[j]) for j in range(k)]
        assert len(d) == k and (e is None or e["k"] == k), (cycles, k, e)
        b = [np.float64(d[j]) * w[j] for j in range(k)]
        orthogonalise(q, z, b, Q[:k], Z[:k])
        rec["g"], rec["h"] = dot_ld(q, q), dot_ld(r, q)
        g, h = (e["g"], e["h"]) if e else (dot(q, q), dot(r, q))
        w[k], alpha, bad = step_scalars(g, h)
        Z[k], Q[k] = z, q
        update(alpha, U, z, r, q)
        rec["alpha"] = float(alpha)
        rec["rr"] = dot_ld(r, r)
        rho_rec = e["rho_rec"] if e else float(np.sqrt(dot(r, r)))
        cycles += 1
        k += 1
        restarted = k == m or rho_rec <= tol
        rec["restarted"] = restarted
        if restarted:
            r = vref.residual(N, L, A, U, F, sh, sign=-1)
            rec["rho_own"] = vref.residual_norm(N, L, A, U, F, sh)
            rho = e["rho"] if e else rec["rho_own"]
            k = 0
        else:
            rho = rho_rec
        history.append(rho)
        records.append(rec)
        if bad:
            breakdown = True
            break
    return dict(U=U, history=history, cycles=cycles, converged=bool(rho <= tol), breakdown=breakdown, records=records, tol=tol)


def plain(orc, a, F, U=None, L=1.0, **opts):
    """the plain cycle iteration on the same operator: (U, history, cycles, converged)"""
    N = F.shape[0]
    return vref.solve(orc, np.ones((N, N)) if a is None else a, F, U, L, **opts)


def nonrestart_steps(history, records):
    """[(rho_{i-1}, rho_i)] over the iterations that did not restart: both ends of such a step are norms of one recurrence
    (rho_{i-1} is the recomputed norm the sequence started from, or the previous recurred one)"""
    return [(history[i], history[i + 1]) for i, rec in enumerate(records) if not rec["restarted"]]
