"""The adjoint of reaction and semilinear solves (include/mg_adjoint_rx.h) without a GPU: the header against the binding and the
library's exports, the Python surface, the refusal without a device, and -- on the numpy restatement (tests/_adjoint_rx_ref.py)
over the dense solves of tests/_reaction_ref.py and tests/_newton_ref.py -- the mathematics: the gradients in F, the rim data,
a, w, kappa, s and sigma against central finite differences, and the adjoint identity <lam, dF> = <Ubar, dU> through the
linearised operator.

Measured on the restatement (J and the differences formed in longdouble): the worst finite-difference mismatch over the five
cases, relative to max |g| of its input, is 2.8e-10 (w, the cubic case; F 8.2e-12, rim data 4.4e-14, a 7.2e-11, kappa 3.0e-12,
s 7.7e-11, sigma 1.4e-12); the adjoint identity holds to 7.4e-20 of sum|lam*dF|."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _adjoint_rx_ref as xref
import _newton_ref as nref
import _reaction_ref as rref
import _solve_vc_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = vref.LD
SYMBOLS = ("mg_sourceGradient", "mg_sourceGradient_batch", "mg_solver_adjoint_reaction", "mg_solver_newton_adjoint",
           "mg_batch_solver_adjoint_reaction", "mg_batch_solver_newton_adjoint")
ADJOINT_SIX = ("mg_coefficientGradient", "mg_boundaryGradient", "mg_coefficientGradient_batch", "mg_boundaryGradient_batch",
               "mg_solver_adjoint", "mg_batch_solver_adjoint")
# (N, shift, kind, coefficient field) of the finite-difference checks; L = 1.3, w = smooth_weight, kappa = 0.7
NEWTON_CASES = [(9, 0.0, "sinh", "smooth"), (12, 30.0, "cubic", "random"), (11, 0.0, "exp", "exp")]
LINEAR_CASES = [(9, 0.0, "smooth"), (12, 30.0, "random")]
L, KAPPA = 1.3, 0.7


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))


def test_header_declares_the_prototypes_of_the_binding():
    import multigrid_poisson_solver_amd as m
    text, names = declared("mg_adjoint_rx.h")
    assert names == sorted(SYMBOLS) == sorted(m.ABI_ADJOINT_RX)
    for name in names:
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(m.ABI_ADJOINT_RX[name][1]), name
    assert re.search(r"#define\s+MG_GRAD_LINEAR\s+3\b", text) and m.GRAD_KINDS == dict(cubic=0, sinh=1, exp=2, linear=3)
    raw = " ".join(re.sub(r"\n \*", "\n", open(os.path.join(ROOT, "include", "mg_adjoint_rx.h")).read()).split())
    for phrase in ("gS[p] = lam'[p]*U[p]", "gW[p] = kappa*(lam'[p]*g(U[p]))", "m = lam[p]*gv", "G[p] = kappa*m", "term = w[p]*m",
                   "no square root", "the solver has no reaction", "heat stepper", "user-supplied g"):
        assert phrase in raw, phrase
    # mg_adjoint.h keeps exactly its six
    assert declared("mg_adjoint.h")[1] == sorted(ADJOINT_SIX) == sorted(m.ABI_ADJOINT)


def test_mg_hip_includes_the_header_once():
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert hip.count('#include "mg_adjoint_rx.h"') == 1
    assert hip.index('#include "mg_newton_batch.h"') < hip.index('#include "mg_adjoint_rx.h"')
    assert not any(name + "(" in hip for name in SYMBOLS)


def test_library_exports_the_symbols():
    import multigrid_poisson_solver_amd as m
    lib = m.load_library()
    others = (m.ABI, m.ABI_FMG, m.ABI_HEAT, m.ABI_VC, m.ABI_VC_BATCH, m.ABI_KRYLOV, m.ABI_ADJOINT, m.ABI_REACTION, m.ABI_NEWTON,
              m.ABI_RX_BATCH, m.ABI_NEWTON_BATCH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert not any(name in abi for abi in others), name
        assert getattr(lib, name).argtypes == m.ABI_ADJOINT_RX[name][1]
        assert getattr(lib, name).restype is m.ABI_ADJOINT_RX[name][0]
    assert b"0.2.2" in lib.mg_version()


def test_python_surface():
    import multigrid_poisson_solver_amd as m
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(m.sourceGradient) == ["N", "kind", "kappa", "w", "lam", "U", "G"]
    assert sig(m.sourceGradient_batch) == ["N", "kind", "kappa", "w", "lam", "U", "G"]
    rx = ["self", "Ubar", "U", "want_coef", "want_rim", "want_reaction"]
    nw = ["self", "Ubar", "U", "F", "kind", "kappa", "weight", "want_coef", "want_rim", "want_weight"]
    assert sig(m.Solver.adjoint_reaction) == rx == sig(m.BatchSolver.adjoint_reaction)
    assert sig(m.Solver.newton_adjoint) == nw == sig(m.BatchSolver.newton_adjoint_batch)
    for f in (m.Solver.newton_adjoint, m.BatchSolver.newton_adjoint_batch):
        p = inspect.signature(f).parameters
        assert p["kind"].default == "sinh" and p["kappa"].default == 1.0 and p["weight"].default is None
        assert all(p[k].default is True for k in ("want_coef", "want_rim", "want_weight"))
    for f, word in ((m.Solver.adjoint_reaction, "gshift"), (m.Solver.newton_adjoint, "gkappa"), (m.Solver.newton_adjoint, "res_forward"),
                    (m.BatchSolver.adjoint_reaction, "bit-identical"), (m.BatchSolver.newton_adjoint_batch, "bit-identical")):
        doc = " ".join(f.__doc__.split())
        assert word in doc and "include/mg_adjoint_rx.h" in doc, f.__qualname__
    # the existing surface keeps its signatures
    for cls in (m.Solver, m.BatchSolver):
        assert sig(cls.adjoint) == ["self", "Ubar", "U", "want_coef", "want_rim"]
    auto = open(os.path.join(ROOT, "multigrid_poisson_solver_amd", "autograd.py")).read()
    assert re.search(r"def solve\(self, F, U0, a=None\)", auto)
    assert re.search(r"def solve_reaction\(self, F, U0, s, a=None\)", auto)
    assert re.search(r'def solve_semilinear\(self, F, U0, kind="sinh", kappa=1\.0, weight=None, a=None, \*\*newton_opts\)', auto)


NOT_INIT_CHILD = r"""
import ctypes as C, sys
import numpy as np
import multigrid_poisson_solver_amd as m
lib = m.load_library()
lib.mg_set_abort_on_error(0)
N = 8
bufs = [np.full((N, N), 7.0) for _ in range(9)]
before = [b.copy() for b in bufs]
p = [b.ctypes.data for b in bufs]
one = lambda x: (C.c_void_p * 1)(x)
res, st = m.SolveResult(), m.BatchSolveStats()
s1, s2, kap = C.c_double(7.0), C.c_double(7.0), (C.c_double * 1)(1.0)
calls = [
    lambda: lib.mg_sourceGradient(N, 1, 1.0, p[0], p[1], p[2], p[3], C.byref(s1)),
    lambda: lib.mg_sourceGradient_batch(1, N, 1, kap, 1, one(p[0]), one(p[1]), one(p[2]), one(p[3]), C.addressof(s1)),
    lambda: lib.mg_solver_adjoint_reaction(None, p[0], p[1], p[2], p[3], p[4], p[5], C.byref(s1), C.byref(res)),
    lambda: lib.mg_solver_newton_adjoint(None, 1, 1.0, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], C.byref(s1), C.byref(s2), C.byref(res)),
    lambda: lib.mg_batch_solver_adjoint_reaction(None, 1, one(p[0]), one(p[1]), one(p[2]), one(p[3]), one(p[4]), one(p[5]),
                                                 C.addressof(s1), C.byref(res), C.byref(st)),
    lambda: lib.mg_batch_solver_newton_adjoint(None, 1, 1, kap, 1, one(p[0]), one(p[1]), one(p[2]), one(p[3]), one(p[4]), one(p[5]),
                                               one(p[6]), one(p[7]), C.addressof(s1), C.addressof(s2), C.byref(res), C.byref(st)),
]
for i, call in enumerate(calls):
    lib.mg_clear_error()
    res.status = 0
    ret = call()
    assert ret == 4 and lib.mg_last_error() == 4, (i, ret, lib.mg_last_error())
    if i in (2, 3):
        assert res.status == 4, (i, res.status)
    assert s1.value == 7.0 and s2.value == 7.0, i
    for b, was in zip(bufs, before):
        assert np.array_equal(b, was), i
print("ADJOINT_RX_NOT_INIT OK")
"""


def test_without_a_device_every_entry_point_refuses_and_writes_nothing():
    """in a process of its own: this one may hold an initialised engine (the GPU session)"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", NOT_INIT_CHILD], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and "ADJOINT_RX_NOT_INIT OK" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------- the mathematics, on the restatement
def points(rng, N, n_rim, n_in):
    """n_rim rim points, a corner among them, and n_in interior points"""
    rim = [(r, c) for r in range(N) for c in range(N) if r in (0, N - 1) or c in (0, N - 1)]
    inner = [(r, c) for r in range(1, N - 1) for c in range(1, N - 1)]
    pick = lambda pts, n: [pts[i] for i in rng.choice(len(pts), size=n, replace=False)]
    return [(0, N - 1)] + pick([p for p in rim if p != (0, N - 1)], n_rim - 1) + pick(inner, n_in)


def fd_check(J, args, grads, pts_of, label):
    """central differences of J(**args) in every input named in grads, step 1e-5*max(1, |x|), against grads[name] to 1e-5 of
    max |g| of that input; arrays at the points pts_of[name], scalars once.  Returns the worst relative mismatch per input."""
    worst = {}
    for what, g in grads.items():
        X = args[what]
        if np.ndim(X) == 0:
            h = 1e-5 * max(1.0, abs(X))
            jp, jm = J(**dict(args, **{what: X + h})), J(**dict(args, **{what: X - h}))
            fd = float((jp - jm) / (LD(X + h) - LD(X - h)))
            scale = abs(float(g))
            assert scale > 0.0
            worst[what] = abs(fd - float(g)) / scale
            assert worst[what] <= 1e-5, (label, what, fd, float(g))
            continue
        scale = float(np.max(np.abs(g)))
        assert scale > 0.0
        for (r, c) in pts_of[what]:
            h = 1e-5 * max(1.0, abs(X[r, c]))
            plus, minus = X.copy(), X.copy()
            plus[r, c] += h
            minus[r, c] -= h
            jp, jm = J(**dict(args, **{what: plus})), J(**dict(args, **{what: minus}))
            fd = float((jp - jm) / (LD(plus[r, c]) - LD(minus[r, c])))
            err = abs(fd - g[r, c]) / scale
            worst[what] = max(worst.get(what, 0.0), err)
            assert err <= 1e-5, (label, what, (r, c), fd, g[r, c], scale)
    print(f"{label}: worst |fd - g|/max|g|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    return worst


def fields(N, name, seed):
    rng = np.random.default_rng(seed)
    a = vref.field(name, N, L, seed=seed)
    F, U0, W = 40.0 * rng.standard_normal((N, N)), rng.standard_normal((N, N)), rng.standard_normal((N, N))
    return a, F, U0, W


@pytest.mark.parametrize("N,shift,kind,name", NEWTON_CASES)
def test_semilinear_gradients_agree_with_central_finite_differences(N, shift, kind, name):
    """J = sum(W*U) over dense_newton; 7 points per array input -- F (2 on the rim, where the gradient is 0), the rim data U0
    (2 in the interior, where it is 0), a and w (a corner, the rim and the interior; the rim of gW is 0) -- and kappa."""
    a, F, U0, W = fields(N, name, 7 + N)
    w = nref.smooth_weight(N, L)
    U, lam, gF, gA, gU, gW, gkappa = xref.gradients_newton(a, kind, KAPPA, w, F, U0, W, L, shift)
    rng = np.random.default_rng(N)

    def J(a, F, U0, w, kappa):
        return np.sum(np.asarray(W, dtype=LD) * nref.dense_newton(a, kind, kappa, w, F, U0, L, shift)[0])

    pts = dict(F=points(rng, N, 2, 5), U0=points(rng, N, 5, 2), a=points(rng, N, 3, 4), w=points(rng, N, 3, 4))
    assert all(len(p) == 7 for p in pts.values())
    fd_check(J, dict(a=a, F=F, U0=U0, w=w, kappa=KAPPA), dict(F=gF, U0=gU, a=gA, w=gW, kappa=float(gkappa)), pts,
             f"N={N} shift={shift} {kind} {name}")
    assert all(gF[p] == 0.0 for p in pts["F"][:2]) and all(gW[p] == 0.0 for p in pts["w"][:3])
    assert all(gU[p] == 0.0 for p in pts["U0"][5:]) and gU[0, N - 1] == W[0, N - 1]
    # the fp64 sum of the restatement is the longdouble one to rounding
    assert abs(xref.source_gradient(N, kind, KAPPA, w, lam, U)[1] - float(gkappa)) <= 1e-12 * float(np.sum(np.abs(w * lam * xref.g_of(kind, U))))


@pytest.mark.parametrize("N,shift,name", LINEAR_CASES)
def test_reaction_gradients_agree_with_central_finite_differences(N, shift, name):
    """J = sum(W*U) over direct_solution with a reaction term s; gS at 7 points (its rim is 0) and gshift = dJ/dsigma, F, the rim
    data and a beside them"""
    a, F, U0, W = fields(N, name, 11 + N)
    s = 50.0 * nref.smooth_weight(N, L) if name == "smooth" else 10.0 ** (2.0 * np.random.default_rng(3).random((N, N)))
    U, lam, gF, gA, gU, gS, gshift = xref.gradients_reaction(a, s, F, U0, W, L, shift)
    rng = np.random.default_rng(N)

    def J(a, F, U0, s, shift):
        return np.sum(np.asarray(W, dtype=LD) * rref.direct_solution(a, s, F, U0, L, shift)[0])

    pts = dict(F=points(rng, N, 2, 5), U0=points(rng, N, 5, 2), a=points(rng, N, 3, 4), s=points(rng, N, 3, 4))
    grads = dict(F=gF, U0=gU, a=gA, s=gS)
    if shift != 0.0:
        grads["shift"] = float(gshift)
    fd_check(J, dict(a=a, F=F, U0=U0, s=s, shift=shift), grads, pts, f"N={N} shift={shift} linear {name}")
    if shift == 0.0:   # (sigma - h < 0 is outside the dense operator's domain only by convention: it is a plain matrix entry)
        h = 1e-5
        fd = float((J(a, F, U0, s, h) - J(a, F, U0, s, -h)) / (LD(h) - LD(-h)))
        assert abs(fd - float(gshift)) <= 1e-5 * abs(float(gshift)), (fd, float(gshift))
    assert all(gS[p] == 0.0 for p in pts["s"][:3]) and all(gU[p] == 0.0 for p in pts["U0"][5:])
    assert abs(xref.source_gradient(N, "linear", 1.0, None, lam, U)[1] - float(gshift)) <= 1e-12 * float(np.sum(np.abs(lam * U)))


@pytest.mark.parametrize("N,shift,kind,name", NEWTON_CASES)
def test_adjoint_identity_through_the_linearised_operator(N, shift, kind, name):
    """<lam, dF> = <Ubar, dU> for a random dF through two dense solves with the reaction S = kappa*w*g'(U): the linearised
    operator is symmetric on the interior.  Both solves carry longdouble refinement."""
    a, F, U0, W = fields(N, name, 70 + N)
    w = nref.smooth_weight(N, L)
    U = nref.dense_newton(a, kind, KAPPA, w, F, U0, L, shift)[0]
    S = xref.linearised_reaction(N, kind, KAPPA, w, U)
    dF = np.random.default_rng(N).standard_normal((N, N))
    lam = xref.direct_adjoint(a, S, W, L, shift)[0]
    dU = rref.direct_solution(a, S, dF, np.zeros((N, N)), L, shift)[0]
    i = (slice(1, -1), slice(1, -1))
    lhs, rhs = np.sum(lam[i] * np.asarray(dF, dtype=LD)[i]), np.sum(np.asarray(W, dtype=LD)[i] * dU[i])
    scale = np.sum(np.abs(lam[i] * np.asarray(dF, dtype=LD)[i]))
    print(f"N={N} {kind}: |lhs - rhs|/sum|lam*dF| = {float(abs(lhs - rhs) / scale):.2e}")
    assert abs(lhs - rhs) <= LD(1e-12) * scale
    assert np.all(lam[0, :] == 0) and np.all(lam[:, 0] == 0)


@pytest.mark.parametrize("N", [3, 4, 5, 12])
def test_restatement_edge_properties(N):
    """the rim of lam and of U is never used; w = None is w = 1; LINEAR with kappa = 1 gives lam'*U"""
    rng = np.random.default_rng(N)
    lam, U, w = rng.standard_normal((N, N)), rng.standard_normal((N, N)), 1.0 + rng.random((N, N))
    dirty, nan_lam, nan_U = lam.copy(), lam.copy(), U.copy()
    dirty[0, :] = dirty[-1, :] = 3.0
    dirty[:, 0] = dirty[:, -1] = -2.0
    for X in (nan_lam, nan_U):
        X[0, :] = X[-1, :] = X[:, 0] = X[:, -1] = np.nan
    for kind in xref.KINDS:
        G, s = xref.source_gradient(N, kind, 0.7, w, lam, U)
        for lam_, U_ in ((dirty, U), (nan_lam, U), (lam, nan_U)):
            G2, s2 = xref.source_gradient(N, kind, 0.7, w, lam_, U_)
            assert np.array_equal(G, G2) and s == s2, kind
        assert np.all(G[0, :] == 0.0) and np.all(G[:, -1] == 0.0) and not np.any(np.signbit(G[0, :]))
        G1, s1 = xref.source_gradient(N, kind, 0.7, None, lam, U)
        Go, so = xref.source_gradient(N, kind, 0.7, np.ones((N, N)), lam, U)
        assert np.array_equal(G1, Go) and s1 == so, kind
    G, s = xref.source_gradient(N, "linear", 1.0, None, lam, U)
    assert np.array_equal(G[1:-1, 1:-1], (lam * U)[1:-1, 1:-1])
    assert abs(s - float(np.sum((lam * U)[1:-1, 1:-1]))) <= 1e-13 * float(np.sum(np.abs(lam * U)))
