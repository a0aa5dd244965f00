"""The variable reaction term (include/mg_reaction.h) without a GPU: the header against the binding and the library's
exports, and the maths of the scheme on the numpy restatement (tests/_reaction_ref.py): the two identity contracts, the
restated solve against a dense direct solution, the order of accuracy, and the cycle counts with and without GCR."""
import os
import re

import numpy as np
import pytest

import _reaction_ref as rref
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LD = np.longdouble
SYMBOLS = ["mg_solver_set_reaction", "mg_solver_has_reaction", "mg_applyOperatorReaction", "mg_sweepReaction",
           "mg_residualReaction", "mg_coarseSolveReaction"]


def test_header_declares_what_the_binding_binds_and_the_library_exports():
    import multigrid_poisson_solver_amd as m
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mg_reaction.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))
    assert declared == sorted(SYMBOLS) == sorted(m.ABI_REACTION)
    lib = m.load_library()
    others = (m.ABI, m.ABI_FMG, m.ABI_HEAT, m.ABI_VC, m.ABI_HEAT_VC, m.ABI_VC_BATCH, m.ABI_KRYLOV, m.ABI_KRYLOV_BATCH,
              m.ABI_ADJOINT, m.ABI_EIGS, m.ABI_BC, m.ABI_SINGULAR, m.ABI_SOLVE_CYCLE)
    for name in declared:
        assert hasattr(lib, name) and not any(name in abi for abi in others), name
        assert getattr(lib, name).argtypes == m.ABI_REACTION[name][1] and getattr(lib, name).restype is m.ABI_REACTION[name][0]
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(m.ABI_REACTION[name][1]), name
    # mg_hip.h declares nothing of it: one include line, after mg_eigs.h and before mg_bc.h
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert hip.count('#include "mg_reaction.h"') == 1 and "reaction" not in hip.replace('#include "mg_reaction.h"', "").lower()
    assert hip.index('#include "mg_eigs.h"') < hip.index('#include "mg_reaction.h"') < hip.index('#include "mg_bc.h"')
    src = open(os.path.join(ROOT, "multigrid_poisson_solver_amd", "build.py")).read()
    assert '"mg_reaction_kernels.hip"' in src and "mg_reaction_impl.h" in src and "mg_reaction.h" in src
    import inspect
    assert "reaction" not in inspect.signature(m.Solver.__init__).parameters   # (it travels in **opts, as bc= and mean= do)
    assert hasattr(m.Solver, "set_reaction") and isinstance(m.Solver.has_reaction, property)


# ---------------------------------------------------------------- the two identity contracts, on the restatement
@pytest.mark.parametrize("coef", [None, "exp"])
@pytest.mark.parametrize("N", [33, 64])
def test_zero_reaction_and_constant_reaction_are_the_known_solvers(oracle, N, coef):
    """s == 0 is the solver without a reaction (sd + 0.0*dx2 == sd), s == c at shift 0 the solver with shift = c
    (0.0 + c*dx2 == shift*dx2): U, history and cycles with =="""
    F, U0 = ref.random_problem(N, 100 + N)
    a = np.ones((N, N)) if coef is None else vref.field(coef, N)
    for shift, s, want_shift in ((0.0, 0.0, 0.0), (25.0, 0.0, 25.0), (0.0, 1e3, 1e3)):
        opts = dict(rtol=1e-9, max_cycles=4)
        want = vref.solve(oracle, a, F, U0, 1.0, shift=want_shift, **opts)
        got = rref.solve(oracle, None if coef is None else a, np.full((N, N), s), F, U0, 1.0, shift=shift, **opts)
        assert_bits(got[0], want[0], f"U, N={N} a={coef} shift={shift} s={s}")
        assert got[1] == want[1] and got[2] == want[2] and got[3] == want[3]


# ---------------------------------------------------------------- truth: a dense direct solution
@pytest.mark.parametrize("coef", [None, "exp"])
@pytest.mark.parametrize("name", rref.FIELDS)
@pytest.mark.parametrize("N", [17, 24, 33])
def test_restated_solve_lands_on_the_direct_solution(oracle, N, name, coef):
    """U - X = A^-1 (r(U) - r(X)) whatever U is, so max|U - X| <= ||A^-1||_inf * (||r(U)||_inf + ||r(X)||_inf), the residuals
    in longdouble from a, s, sigma, L, N, F alone.  ||A^-1||_inf is taken from the fp64 inverse of the longdouble-assembled
    matrix; 1e-6 relative covers that inverse's own rounding (the matrix is an M-matrix with condition below 1e5 here)."""
    L, shift = 1.5, 2.0
    F, U0 = ref.random_problem(N, 300 + N)
    a = None if coef is None else vref.field(coef, N, L)
    s = rref.field(name, N, L)
    U, hist, k, conv = rref.solve(oracle, a, s, F, U0, L, shift=shift, rtol=1e-10, max_cycles=60)
    X, nA = rref.direct_solution(a, s, F, U0, L, shift)
    rU = np.max(np.abs(rref.residual_ld(a, s, U, F, L, shift)))
    rX = np.max(np.abs(rref.residual_ld(a, s, X, F, L, shift)))
    err = np.max(np.abs(U.astype(LD) - X))
    bound = nA * (rU + rX) * (1 + LD(1e-6))
    print(f"N={N} s={name} a={coef}: {k} cycles (converged {conv}), |U-X| {float(err):.3e} <= {float(bound):.3e} "
          f"(||A^-1|| {float(nA):.3e}, r(U) {float(rU):.3e}, r(X) {float(rX):.3e})")
    assert conv, (k, hist[-1])
    assert err <= bound


def test_second_order_on_a_manufactured_solution(oracle):
    """u = sin(pi x) sin(2 pi y), a = 1 + x/2, s = 100 (1 + x): the max error falls by 4 per halving of h, ratios inside
    [3.9, 4.1] for N = 33 -> 65 -> 129"""
    errs = []
    for N in (33, 65, 129):
        x, y = vref.grid(N, 1.0)
        u = np.sin(np.pi * x) * np.sin(2 * np.pi * y)
        a = 1.0 + 0.5 * x + 0.0 * y
        s = 100.0 * (1.0 + x) + 0.0 * y
        F = a * (-5.0 * np.pi ** 2 * u) + 0.5 * (np.pi * np.cos(np.pi * x) * np.sin(2 * np.pi * y)) - s * u
        U, hist, k, conv = rref.solve(oracle, a, s, F, ref.rim_only(u), 1.0, rtol=1e-10)
        assert conv, (N, k)
        errs.append(float(np.max(np.abs(U - u))))
        print(f"N={N}: {k} cycles, max error {errs[-1]:.4e}")
    ratios = [errs[i] / errs[i + 1] for i in range(2)]
    print("ratios", ratios)
    assert all(3.9 <= r <= 4.1 for r in ratios), ratios


# ---------------------------------------------------------------- cycle counts
CASES = [(65, None), (129, None), (129, "exp")]


def _setup(N, coef):
    F, U0 = ref.random_problem(N, 11)
    return F, U0, None if coef is None else vref.field(coef, N)


@pytest.mark.parametrize("name", ["smooth", "blob"])
@pytest.mark.parametrize("N,coef", CASES)
def test_smooth_reaction_terms_converge_like_the_plain_problem(oracle, N, coef, name):
    """V(3,3), omega 0.8, N_min 8, rtol 1e-9: within 20 cycles (13-15 without a reaction)"""
    F, U0, a = _setup(N, coef)
    U, hist, k, conv = rref.solve(oracle, a, rref.field(name, N), F, U0, 1.0, rtol=1e-9, max_cycles=20)
    print(f"N={N} a={coef} s={name}: {k} cycles, converged {conv}")
    assert conv and k <= 20, (k, hist[-1])


@pytest.mark.parametrize("name", ["halfplane", "random"])
@pytest.mark.parametrize("N,coef", CASES)
def test_discontinuous_reaction_terms_converge_under_gcr(oracle, N, coef, name):
    """GCR(8) around the same cycle: within 30 iterations, the history never grows, no breakdown"""
    F, U0, a = _setup(N, coef)
    out = rref.krylov_solve(oracle, a, rref.field(name, N), F, U0, 1.0, m=8, rtol=1e-9, max_cycles=30)
    h = out["history"]
    print(f"N={N} a={coef} s={name}: GCR(8) {out['cycles']} iterations, converged {out['converged']}")
    assert out["converged"] and out["cycles"] <= 30 and not out["breakdown"], (out["cycles"], h[-1])
    assert all(h[i + 1] <= h[i] for i in range(len(h) - 1)), h


def test_halfplane_is_slow_under_the_plain_cycle(oracle):
    """the case the Krylov support is for: s = 1e5 on x >= 0.37 at N = 129, a = 1, is NOT converged after 40 plain cycles"""
    F, U0, a = _setup(129, None)
    U, hist, k, conv = rref.solve(oracle, a, rref.field("halfplane", 129), F, U0, 1.0, rtol=1e-9, max_cycles=40)
    print(f"N=129 a=None s=halfplane: plain, {k} cycles, residual {hist[-1] / ref.ref_norm(F):.3e} of ||F||, converged {conv}")
    assert not conv and k == 40
