"""Adjoint sensitivities (include/mg_adjoint.h) without a GPU: the header against the binding and the library's exports, the
Python surface, the refusal without a device, and -- on the numpy restatement (tests/_adjoint_ref.py) over the dense solves of
tests/_solve_vc_ref.py -- the mathematics: the gradients in F, in the rim data and in a against central finite differences of
direct_solution, and the adjoint identity <lam, dF> = <Ubar, dU>.

Measured on the restatement (J and the differences formed in longdouble): the worst finite-difference mismatch over the three
cases, relative to max |g| of its input, is 4.9e-11 (F), 7.3e-14 (U0), 4.3e-11 (a); the adjoint identity holds to 1.9e-20 of
sum|lam*dF|."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _adjoint_ref as aref
import _solve_vc_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = vref.LD
SYMBOLS = ("mg_coefficientGradient", "mg_boundaryGradient", "mg_coefficientGradient_batch", "mg_boundaryGradient_batch",
           "mg_solver_adjoint", "mg_batch_solver_adjoint")
# (N, shift, field) of the finite-difference check; L = 1.3
CASES = [(9, 0.0, "smooth"), (12, 30.0, "random"), (17, 0.0, "exp")]
L = 1.3


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mg_adjoint.h")).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))


def test_header_declares_the_six_prototypes():
    import multigrid_poisson_solver_amd as m
    text, names = declared()
    assert names == sorted(SYMBOLS) == sorted(m.ABI_ADJOINT)
    for name in names:
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(m.ABI_ADJOINT[name][1]), name
    raw = " ".join(re.sub(r"\n \*", "\n", open(os.path.join(ROOT, "include", "mg_adjoint.h")).read()).split())
    # the specification states the order of the sum, the substituted rim and what is out of scope
    for phrase in ("h*((((0.0 + tN) + tS) + tE) + tW)", "replaced by +0.0", "Ubar[b] - inv*(f*lam[p])", "derivative in shift",
                   "heat stepper", "shared by several instances", "slab / multi-GPU"):
        assert phrase in raw, phrase


def test_mg_hip_includes_the_header():
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert hip.count('#include "mg_adjoint.h"') == 1
    assert hip.index("typedef struct mg_batch_solver mg_batch_solver;") < hip.index('#include "mg_adjoint.h"')
    assert hip.index('#include "mg_varcoef_batch.h"') < hip.index('#include "mg_adjoint.h"')
    # no prototype of the feature in mg_hip.h itself
    assert not any(name + "(" in hip for name in SYMBOLS)


def test_library_exports_the_six_symbols():
    import multigrid_poisson_solver_amd as m
    lib = m.load_library()
    others = (m.ABI, m.ABI_FMG, m.ABI_HEAT, m.ABI_VC, m.ABI_HEAT_VC, m.ABI_VC_BATCH, m.ABI_KRYLOV, m.ABI_KRYLOV_BATCH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert not any(name in abi for abi in others), name
        assert getattr(lib, name).argtypes == m.ABI_ADJOINT[name][1]
        assert getattr(lib, name).restype is m.ABI_ADJOINT[name][0]
    assert b"0.2.2" in lib.mg_version()


def test_python_surface():
    import multigrid_poisson_solver_amd as m
    assert list(inspect.signature(m.coefficientGradient).parameters) == ["N", "L", "lam", "U", "gA"]
    assert list(inspect.signature(m.boundaryGradient).parameters) == ["N", "L", "a", "lam", "Ubar", "gU"]
    for cls in (m.Solver, m.BatchSolver):
        sig = inspect.signature(cls.adjoint)
        assert list(sig.parameters) == ["self", "Ubar", "U", "want_coef", "want_rim"]
        assert sig.parameters["want_coef"].default is True and sig.parameters["want_rim"].default is True
        doc = " ".join(cls.adjoint.__doc__.split())
        assert "(lam, gA, gU, info" in doc and "include/mg_adjoint.h" in doc, cls.__name__
    assert "bit-identical" in " ".join(m.BatchSolver.adjoint.__doc__.split())
    # the torch side is a module of its own, which the package does not import
    src = open(os.path.join(ROOT, "multigrid_poisson_solver_amd", "__init__.py")).read()
    assert not re.search(r"^\s*(from|import)\s+.*\bautograd\b", src, flags=re.M)
    auto = open(os.path.join(ROOT, "multigrid_poisson_solver_amd", "autograd.py")).read()
    assert "class DifferentiableSolver" in auto and "torch.autograd.Function" in auto
    assert re.search(r"def __init__\(self, N, L=1\.0, max_batch=1, strict=True, \*\*opts\)", auto)
    assert re.search(r"def solve\(self, F, U0, a=None\)", auto)


NOT_INIT_CHILD = r"""
import ctypes as C, sys
import numpy as np
import multigrid_poisson_solver_amd as m
lib = m.load_library()
lib.mg_set_abort_on_error(0)
N = 8
bufs = [np.full((N, N), 7.0) for _ in range(6)]
before = [b.copy() for b in bufs]
p = [b.ctypes.data for b in bufs]
one = lambda x: (C.c_void_p * 1)(x)
res, st = m.SolveResult(), m.BatchSolveStats()
calls = [
    lambda: lib.mg_coefficientGradient(N, 1.0, p[0], p[1], p[2]),
    lambda: lib.mg_boundaryGradient(N, 1.0, p[0], p[1], p[2], p[3]),
    lambda: lib.mg_coefficientGradient_batch(1, N, 1.0, one(p[0]), one(p[1]), one(p[2])),
    lambda: lib.mg_boundaryGradient_batch(1, N, 1.0, one(p[0]), one(p[1]), one(p[2]), one(p[3])),
    lambda: lib.mg_solver_adjoint(None, p[0], p[1], p[2], p[3], p[4], C.byref(res)),
    lambda: lib.mg_batch_solver_adjoint(None, 1, one(p[0]), one(p[1]), one(p[2]), one(p[3]), one(p[4]), C.byref(res), C.byref(st)),
]
for i, call in enumerate(calls):
    lib.mg_clear_error()
    ret = call()
    assert lib.mg_last_error() == 4, (i, lib.mg_last_error())
    if i >= 4:
        assert ret == 4 and res.status == 4, (i, ret, res.status)
    for b, was in zip(bufs, before):
        assert np.array_equal(b, was), i
print("ADJOINT_NOT_INIT OK")
"""


def test_without_a_device_every_entry_point_refuses_and_writes_nothing():
    """in a process of its own: this one may hold an initialised engine (the GPU session)"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", NOT_INIT_CHILD], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and "ADJOINT_NOT_INIT OK" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------- the mathematics, on the restatement
def problem(N, shift, name, seed):
    rng = np.random.default_rng(seed)
    a = vref.field(name, N, L, seed=seed)
    F, U0, W = 40.0 * rng.standard_normal((N, N)), rng.standard_normal((N, N)), rng.standard_normal((N, N))
    return a, F, U0, W


def points(rng, N, n_rim, n_in):
    """n_rim rim points, a corner among them, and n_in interior points"""
    rim = [(r, c) for r in range(N) for c in range(N) if r in (0, N - 1) or c in (0, N - 1)]
    inner = [(r, c) for r in range(1, N - 1) for c in range(1, N - 1)]
    pick = lambda pts, n: [pts[i] for i in rng.choice(len(pts), size=n, replace=False)]
    return [(0, N - 1)] + pick([p for p in rim if p != (0, N - 1)], n_rim - 1) + pick(inner, n_in)


@pytest.mark.parametrize("N,shift,name", CASES)
def test_gradients_agree_with_central_finite_differences(N, shift, name):
    """J = sum(W*U); 12 points per input: F (3 on the rim, where the gradient is 0), U0 (3 in the interior, where it is 0)
    and a (rim, a corner and interior).  Step 1e-5*max(1, |x|), bound 1e-5 of max |g| of that input: a wrong sign, factor or
    neighbour gives O(1)."""
    a, F, U0, W = problem(N, shift, name, 7 + N)
    U, lam, gF, gA, gU = aref.gradients(a, F, U0, W, L, shift)
    rng = np.random.default_rng(N)

    def J(a_, F_, U0_):
        return np.sum(np.asarray(W, dtype=LD) * vref.direct_solution(a_, F_, U0_, L, shift))

    worst = {}
    for what, X, g, pts in (("F", F, gF, points(rng, N, 3, 9)), ("U0", U0, gU, points(rng, N, 9, 3)), ("a", a, gA, points(rng, N, 4, 8))):
        assert len(pts) == 12
        scale = float(np.max(np.abs(g)))
        assert scale > 0.0
        for (r, c) in pts:
            h = 1e-5 * max(1.0, abs(X[r, c]))
            args = dict(a=a, F=F, U0=U0)
            plus, minus = X.copy(), X.copy()
            plus[r, c] += h
            minus[r, c] -= h
            jp = J(**{k + "_": (plus if k == what else v) for k, v in args.items()})
            jm = J(**{k + "_": (minus if k == what else v) for k, v in args.items()})
            fd = float((jp - jm) / (LD(plus[r, c]) - LD(minus[r, c])))
            err = abs(fd - g[r, c]) / scale
            worst[what] = max(worst.get(what, 0.0), err)
            assert err <= 1e-5, (what, (r, c), fd, g[r, c], scale)
        if what == "F":
            assert all(g[p] == 0.0 for p in pts[:3])
        if what == "U0":
            assert all(g[p] == 0.0 for p in pts[9:]) and g[0, N - 1] == W[0, N - 1]
    print(f"N={N} shift={shift} {name}: worst |fd - g|/max|g|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("N,shift,name", CASES)
def test_adjoint_identity(N, shift, name):
    """<lam, dF> = <Ubar, dU> for a random dF through two dense solves (dU: the solve of dF with a zero rim): the operator is
    symmetric on the interior.  Both solves carry longdouble refinement, so the two sides agree far below 1e-12 of
    sum|lam*dF| (fp64 rounding of the sums alone would allow (N-2)^2 * 1.1e-16)."""
    a, _, _, W = problem(N, shift, name, 70 + N)
    dF = np.random.default_rng(N).standard_normal((N, N))
    lam = aref.direct_adjoint(a, W, L, shift)
    dU = vref.direct_solution(a, dF, np.zeros((N, N)), L, shift)
    i = (slice(1, -1), slice(1, -1))
    lhs, rhs = np.sum(lam[i] * np.asarray(dF, dtype=LD)[i]), np.sum(np.asarray(W, dtype=LD)[i] * dU[i])
    scale = np.sum(np.abs(lam[i] * np.asarray(dF, dtype=LD)[i]))
    print(f"N={N}: |lhs - rhs|/sum|lam*dF| = {float(abs(lhs - rhs) / scale):.2e}")
    assert abs(lhs - rhs) <= LD(1e-12) * scale
    assert np.all(lam[0, :] == 0) and np.all(lam[:, 0] == 0)


@pytest.mark.parametrize("N", [3, 4, 5, 12])
def test_restatement_edge_properties(N):
    """the rim of lam is never used; a == None is a == 1; Ubar == None is Ubar == 0; corners carry Ubar alone"""
    rng = np.random.default_rng(N)
    lam, U, W = rng.standard_normal((N, N)), rng.standard_normal((N, N)), rng.standard_normal((N, N))
    dirty = lam.copy()
    dirty[0, :] = dirty[-1, :] = 3.0
    dirty[:, 0] = dirty[:, -1] = -2.0
    assert np.array_equal(aref.coefficient_gradient(N, L, lam, U), aref.coefficient_gradient(N, L, dirty, U))
    assert np.array_equal(aref.boundary_gradient(N, L, None, lam, W), aref.boundary_gradient(N, L, np.ones((N, N)), lam, W))
    assert np.array_equal(aref.boundary_gradient(N, L, None, lam, None), aref.boundary_gradient(N, L, None, lam, np.zeros((N, N))))
    g = aref.boundary_gradient(N, L, None, lam, W)
    assert g[0, 0] == W[0, 0] and g[-1, -1] == W[-1, -1] and np.all(g[1:-1, 1:-1] == 0.0)
