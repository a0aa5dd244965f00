"""The semilinear solve (include/mg_newton.h) without a GPU: the header against the binding and the library's exports, and
the maths of the method on the numpy restatement (tests/_newton_ref.py): the restated Newton-multigrid solve against a dense
longdouble Newton solution, the order of accuracy, kappa = 0 as the linear solve, and the line search on a hard start."""
import os
import re

import numpy as np
import pytest

import _newton_ref as nref
import _reaction_ref as rref
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LD = np.longdouble
SYMBOLS = ["mg_newton_opts_default", "mg_solver_newton", "mg_solver_newton_history", "mg_solver_newton_inner_history",
           "mg_nonlinearResidual"]


def test_header_declares_what_the_binding_binds_and_the_library_exports():
    import multigrid_poisson_solver_amd as m
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mg_newton.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))
    assert declared == sorted(SYMBOLS) == sorted(m.ABI_NEWTON)
    lib = m.load_library()
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == m.ABI_NEWTON[name][1] and getattr(lib, name).restype is m.ABI_NEWTON[name][0]
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(m.ABI_NEWTON[name][1]), name
    for struct, fields in (("mg_newton_opts", m.NewtonOpts), ("mg_newton_result", m.NewtonResult), ("mg_newton_iter", m.NewtonIter)):
        body = re.search(r"typedef struct %s \{(.*?)\}" % struct, text, re.S).group(1)
        names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [f for f, _ in fields._fields_], (struct, names)
    assert [int(re.search(r"#define MG_NEWTON_%s\s+\(?(-?\d+)" % k.upper(), text).group(1)) for k in nref.KINDS] == \
        [m.NEWTON_KINDS[k] for k in nref.KINDS]
    assert (m.NEWTON_CONVERGED, m.NEWTON_NOT_CONVERGED, m.NEWTON_STALLED) == (nref.CONVERGED, nref.NOT_CONVERGED, nref.STALLED) == \
        tuple(int(re.search(r"#define MG_NEWTON_%s\s+\(?(-?\d+)" % k, text).group(1)) for k in ("CONVERGED", "NOT_CONVERGED", "STALLED"))
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert hip.count('#include "mg_newton.h"') == 1
    src = open(os.path.join(ROOT, "multigrid_poisson_solver_amd", "build.py")).read()
    assert '"mg_newton_kernels.hip"' in src and "mg_newton_impl.h" in src and "mg_newton.h" in src and "mg_exp_libm.h" in src
    import inspect
    sig = inspect.signature(m.Solver.newton).parameters
    assert {k: sig[k].default for k in nref.NEWTON_DEFAULTS} == nref.NEWTON_DEFAULTS and sig["kind"].default == "sinh"
    assert callable(m.solve_semilinear) and callable(m.nonlinear_residual)


# ---------------------------------------------------------------- truth: a dense Newton solution in longdouble
@pytest.mark.parametrize("weight", [False, True])
@pytest.mark.parametrize("coef", [None, "exp"])
@pytest.mark.parametrize("kind", nref.KINDS)
@pytest.mark.parametrize("N", [17, 24, 33])
def test_restated_newton_lands_on_the_dense_solution(oracle, N, kind, coef, weight):
    """N(U) - N(X) = (A - diag(kappa*w*g'(xi)))(U - X) with g' >= 0: an M-matrix whose inverse is dominated by A^-1, so
    max|U - X| <= ||A^-1||_inf * (||N(U)||_inf + ||N(X)||_inf), the residuals in longdouble from the data alone; 1e-6 relative
    covers the fp64 inverse's own rounding (tests/test_solve_reaction_cpu.py)."""
    L, shift, kappa = 1.5, 2.0, 10.0
    F, U0 = nref.problem(N, L)
    a = None if coef is None else vref.field(coef, N, L)
    w = nref.smooth_weight(N, L) if weight else None
    out = nref.newton(oracle, a, kind, kappa, w, F, U0, L, inner=dict(shift=shift))
    assert out["converged"] and out["iterations"] <= 20, out["history"]
    X, nA = nref.dense_newton(a, kind, kappa, w, F, U0, L, shift)
    rU = np.max(np.abs(nref.residual_ld(a, kind, kappa, w, out["U"], F, L, shift)))
    rX = np.max(np.abs(nref.residual_ld(a, kind, kappa, w, X, F, L, shift)))
    err = np.max(np.abs(out["U"].astype(LD) - X))
    bound = nA * (rU + rX) * (1 + LD(1e-6))
    print(f"N={N} {kind} a={coef} w={weight}: {out['iterations']} iterations, |U-X| {float(err):.3e} <= {float(bound):.3e} "
          f"(N(U) {float(rU):.3e}, N(X) {float(rX):.3e})")
    assert err <= bound


@pytest.mark.parametrize("kappa", [1.0, 100.0])
@pytest.mark.parametrize("kind", nref.KINDS)
def test_second_order_on_a_manufactured_solution(oracle, kind, kappa):
    """u* = sin(pi x) sin(2 pi y), F = Laplace(u*) - kappa*g(u*): the max error falls by 4 from N = 33 to 65, the ratio inside
    [3.9, 4.1] (a dense exact Newton gave 3.994 - 4.005 for every kind at both kappa)"""
    errs = []
    for N in (33, 65):
        u, F = nref.manufactured(N, kind, kappa)
        out = nref.newton(oracle, None, kind, kappa, None, F, ref.rim_only(u), 1.0, rtol=1e-10)
        assert out["converged"], (N, out["history"])
        errs.append(float(np.max(np.abs(out["U"] - u))))
    print(f"{kind} kappa={kappa}: errors {errs}, ratio {errs[0] / errs[1]:.4f}")
    assert 3.9 <= errs[0] / errs[1] <= 4.1


@pytest.mark.parametrize("coef", [None, "exp"])
def test_kappa_zero_is_one_newton_step_and_the_linear_solve(oracle, coef):
    """kappa = 0 from U = 0: S = 0 and D = F, so the one Newton step is the restated linear solve of F from zero, bit for bit"""
    N = 33
    F = ref.random_problem(N, 77)[0]
    a = None if coef is None else vref.field(coef, N)
    for kind in nref.KINDS:
        out = nref.newton(oracle, a, kind, 0.0, None, F, None, 1.0)
        want = rref.solve(oracle, a, np.zeros((N, N)), F, None, 1.0, engine_norms=True)
        assert out["iterations"] == 1 and out["converged"] and out["steps"][0]["t"] == 1.0 and out["steps"][0]["backtracks"] == 0
        assert_bits(out["U"], want[0], f"{kind} a={coef}: U")
        assert out["steps"][0]["inner_cycles"] == want[2] and out["history"] == [want[1][0], out["res"]]


def test_hard_cubic_start_backtracks_and_converges(oracle):
    """F == -1e6, kappa = 1, cubic, from U = 0 at N = 33: the full first step overshoots by orders of magnitude; the line search
    halves it 9 times, the second step 3 times, then full steps converge (the dense exact Newton: the same sequence)"""
    N = 33
    F = np.full((N, N), nref.HARD_STARTS["cubic"])
    out = nref.newton(oracle, None, "cubic", 1.0, None, F, None, 1.0)
    bt = [s["backtracks"] for s in out["steps"]]
    print("backtracks", bt, "history", out["history"])
    assert out["converged"] and out["iterations"] <= 20
    assert bt[:3] == [9, 3, 0] and not any(bt[2:]), bt
    h = out["history"]
    assert all(h[i + 1] < h[i] for i in range(len(h) - 1))
    stalled = nref.newton(oracle, None, "cubic", 1.0, None, F, None, 1.0, max_backtracks=0)
    assert stalled["status"] == nref.STALLED and stalled["iterations"] == 0 and not np.any(stalled["U"])
