"""The variable-coefficient solver (include/mg_varcoef.h) without a GPU: the header against the binding, and the restatement
(tests/_solve_vc_ref.py) against what the header promises -- a == 1 is the constant-coefficient restatement bit for bit, the
coarsened coefficient keeps the bounds of a on every level, and the cycle converges on smooth and on high-contrast fields."""
import os
import re

import numpy as np
import pytest

import _solve_ref as ref
import _solve_shift_ref as sref
import _solve_vc_ref as vref
from conftest import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mg_solver_set_coefficient", "mg_solver_has_coefficient", "mg_applyOperator", "mg_coarsenCoefficient",
           "mg_sweepCoefficient", "mg_residualCoefficient")


def test_header_declares_what_the_binding_binds_and_the_library_exports():
    import multigrid_poisson_solver_amd as m
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mg_varcoef.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))
    assert declared == sorted(SYMBOLS)
    lib = m.load_library()
    for name in declared:
        assert name in m.ABI_VC and name not in m.ABI and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == m.ABI_VC[name][1]
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(m.ABI_VC[name][1]), name
    assert sorted(m.ABI_VC) == declared
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert '#include "mg_varcoef.h"' in hip and hip.index('#include "mg_varcoef.h"') > hip.index('#include "mg_heat.h"')
    assert b"0.2.2" in lib.mg_version()
    for f in (m.Solver, m.Solver.set_coefficient, m.solve):
        assert "a == 1" in f.__doc__ or "set_coefficient" in f.__doc__, f.__name__
    # the batched solver, the batched solve and the heat stepper take no coefficient (and refuse one as an unknown option)
    import inspect
    assert "coef" in inspect.signature(m.Solver.__init__).parameters
    for f in (m.BatchSolver.__init__, m.solve_batched, m.HeatStepper.__init__):
        assert "coef" not in inspect.signature(f).parameters, f.__qualname__
    assert "coef" not in {f for f, _ in m.SolveOpts._fields_}


def test_the_restatements_table_is_the_librarys():
    import multigrid_poisson_solver_amd as m
    for N in (7, 64, 100, 257, 512):
        lo, w = m.restriction_table(N, N // 2)
        mine = vref.restriction_table(N, N // 2)
        assert np.array_equal(lo, mine[0])
        assert_bits(w, mine[1], f"restriction weights {N}")


@pytest.mark.parametrize("shift", [0.0, 1e2, 1e6])
@pytest.mark.parametrize("N", [64, 100, 257])
def test_unit_coefficient_is_the_constant_restatement(oracle, N, shift):
    """a == 1: every level's coefficient is exactly 1, and U, history and cycles are _solve_shift_ref's bit for bit."""
    F, U0 = ref.random_problem(N, 300 + N)
    a = vref.field("one", N)
    for A in vref.coarsen_levels(a, 8):
        assert_bits(A, np.ones_like(A), f"coarsened unit coefficient {A.shape[0]}")
    opts = dict(shift=shift, rtol=1e-8, max_cycles=4)
    m_vc, m_c = [], []
    U, hist, cycles, conv = vref.solve(oracle, a, F, U0, 1.0, margins=m_vc, **opts)
    Uc, hist_c, cycles_c, conv_c = sref.solve(oracle, F, U0, 1.0, margins=m_c, **opts)
    assert min(m_vc) >= vref.QUALIFY and m_vc == m_c, (m_vc, m_c)
    assert_bits(U, Uc, "U")
    assert hist == hist_c and cycles == cycles_c and conv == conv_c
    # the kernels on their own
    _, Ux = ref.random_problem(N, 400 + N)
    assert_bits(vref.weighted_sweeps(N, 1.0, a, Ux, F, 0.8, 1, shift), sref.weighted_sweeps(N, 1.0, Ux, F, 0.8, 1, shift), "sweep")
    assert_bits(vref.residual(N, 1.0, a, Ux, F, shift), sref.residual(N, 1.0, Ux, F, shift), "residual")
    assert_bits(vref.apply_operator(N, 1.0, None, Ux, shift), vref.apply_operator(N, 1.0, a, Ux, shift), "operator")


@pytest.mark.parametrize("N", [100, 256, 257])
def test_coarsened_coefficient_keeps_the_bounds(N):
    a = vref.field("random", N, seed=N)
    lo, hi = float(a.min()), float(a.max())
    assert lo > 0.0 and hi / lo > 500.0
    levels = vref.coarsen_levels(a, 3)
    assert [A.shape[0] for A in levels] == ref.sizes(N, 3)
    for A in levels[1:]:
        assert np.all(np.isfinite(A)) and float(A.min()) >= lo and float(A.max()) <= hi, A.shape
        # the end points of the two grids coincide: the corners are the fine corners
    for fine, coarse in zip(levels, levels[1:]):
        assert coarse[0, 0] == fine[0, 0] and coarse[-1, -1] == fine[-1, -1] and coarse[0, -1] == fine[0, -1]


# cycles to rtol = 1e-9 from ref.random_problem(N, 500 + N) with the defaults (V(3,3), omega 0.8), as measured on the
# restatement; the condition the feature has to meet is convergence within max_cycles = 50
CYCLES = {("one", 129): 14, ("smooth", 129): 14, ("exp", 129): 15,
          ("one", 257): 15, ("smooth", 257): 15, ("exp", 257): 16}


@pytest.mark.parametrize("name", ["one", "smooth", "exp"])
@pytest.mark.parametrize("N", [129, 257])
def test_convergence(oracle, N, name):
    F, U0 = ref.random_problem(N, 500 + N)
    a = vref.field(name, N)
    capped = []
    U, hist, cycles, conv = vref.solve(oracle, a, F, U0, 1.0, capped=capped, rtol=1e-9)
    print(f"N={N} a={name} (contrast {a.max() / a.min():.1f}): {cycles} cycles, res {hist[-1]:.3e} / tol {1e-9 * ref.ref_norm(F):.3e}, "
          f"factors {[round(hist[i + 1] / hist[i], 3) for i in range(len(hist) - 1)]}")
    assert conv and cycles <= 50 and not any(capped)
    assert cycles == CYCLES[(name, N)]
    # the residual the solve stopped on is the residual of the discrete problem, in longdouble
    res_ld = vref.residual_norm_ld(a, U, F, 1.0, 0.0)
    assert abs(res_ld - hist[-1]) <= vref.residual_rounding_bound(a, U, F, 1.0, 0.0)


def test_jump_coefficient_reports_honestly(oracle):
    """A sampled coefficient is not expected to be robust to jumps: only the status is asserted (the count is in DESIGN.md)."""
    N = 129
    F, U0 = ref.random_problem(N, 500 + N)
    a = vref.field("jump", N)
    assert a.min() == 1.0 and a.max() == 10.0
    U, hist, cycles, conv = vref.solve(oracle, a, F, U0, 1.0, rtol=1e-9)
    tol = 1e-9 * ref.ref_norm(F)
    print(f"N={N} jump 10x: {cycles} cycles, converged {conv}, res {hist[-1]:.3e} / tol {tol:.3e}")
    assert conv == (hist[-1] <= tol) and len(hist) == cycles + 1 and (conv or cycles == 50)
    assert vref.residual_norm(N, 1.0, a, U, F) == hist[-1]


def test_direct_solution_solves_the_discrete_system():
    """the dense reference of the GPU truth tests: its longdouble residual is at rounding level"""
    N = 17
    F, U0 = ref.random_problem(N, 77)
    a = vref.field("exp", N)
    X = vref.direct_solution(a, F, U0, 1.0, 25.0)
    assert_bits(np.asarray(X, dtype=np.float64)[0], U0[0], "rim")
    assert vref.residual_norm_ld(a, X, F, 1.0, 25.0) <= 1e-3 * vref.residual_rounding_bound(a, np.asarray(X, dtype=np.float64), F, 1.0, 25.0)
