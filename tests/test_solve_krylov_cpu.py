"""The Krylov acceleration (include/mg_krylov.h) without a GPU: the header against the binding and the library's exports, the
values of m the host refuses, and the method itself on the numpy restatement (tests/_krylov_ref.py): the recurred residual
norm never grows, the hard coefficients of DESIGN 4.3 converge where the plain cycle does not, converged results hold in
longdouble and against a dense direct solve, and m beyond the iteration count changes nothing."""
import inspect
import os
import re

import numpy as np
import pytest

import _krylov_ref as kref
import _solve_ref as ref
import _solve_vc_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
SYMBOLS = ("mg_solver_set_krylov", "mg_solver_krylov", "mg_solver_krylov_breakdown", "mg_solver_krylov_log", "mg_krylovDots",
           "mg_krylovOrth", "mg_krylovUpdate")


def problem(N, name):
    """the problems of the counts pinned below: F and start from seed 1, fields from seed 1"""
    F, U0 = ref.random_problem(N, 1)
    return F, U0, vref.field(name, N, seed=1)


# ---------------------------------------------------------------- header, binding, host-side refusals
def test_header_declares_what_the_binding_binds_and_the_library_exports():
    import multigrid_poisson_solver_amd as m
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mg_krylov.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))
    assert names == sorted(SYMBOLS) == sorted(m.ABI_KRYLOV)
    lib = m.load_library()
    for name in names:
        assert not any(name in abi for abi in (m.ABI, m.ABI_FMG, m.ABI_HEAT, m.ABI_VC, m.ABI_HEAT_VC, m.ABI_VC_BATCH)), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == m.ABI_KRYLOV[name][1]
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(m.ABI_KRYLOV[name][1]), name
    assert b"0.2.2" in lib.mg_version()
    assert int(re.search(r"#define MG_KRYLOV_MAX_M (\d+)", text).group(1)) == m.MG_KRYLOV_MAX_M == kref.MAX_M == 16


def test_mg_hip_includes_the_header_last():
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    includes = re.findall(r'#include "(mg_\w+\.h)"', hip)
    assert includes[-1] == "mg_krylov.h" and includes.index("mg_heat_vc.h") < includes.index("mg_krylov.h")
    assert hip.index("typedef struct mg_solver mg_solver;") < hip.index('#include "mg_krylov.h"')


def test_solve_opts_and_result_are_unchanged():
    import ctypes as C
    import multigrid_poisson_solver_amd as m
    assert [f for f, _ in m.SolveOpts._fields_] == ["pre", "post", "N_min", "omega", "coarse_rtol", "coarse_atol", "coarse_max_iters",
                                                     "rtol", "atol", "max_cycles", "fmg", "shift"]
    assert C.sizeof(m.SolveOpts) == 80 and m.SolveOpts.shift.offset == 72
    assert C.sizeof(m.SolveResult) == 64
    assert "krylov" not in {f for f, _ in m.SolveOpts._fields_}


def test_python_surface():
    import multigrid_poisson_solver_amd as m
    assert list(inspect.signature(m.Solver.__init__).parameters) == ["self", "N", "L", "coef", "krylov", "opts"]
    assert list(inspect.signature(m.Solver.set_krylov).parameters) == ["self", "m"]
    assert isinstance(m.Solver.krylov, property)
    assert "krylov" not in inspect.signature(m.BatchSolver.__init__).parameters
    assert "krylov" not in inspect.signature(m.HeatStepper.__init__).parameters
    for f in (m.Solver, m.Solver.set_krylov, m.solve):
        doc = " ".join(f.__doc__.split())
        assert "GCR(m)" in doc and "(2m + 1)*N^2" in doc and "recomputed residual" in doc, f.__qualname__


def test_restatement_refuses_m_outside_its_range(oracle):
    F, U0, a = problem(17, "smooth")
    for m in (0, -1, 17):
        with pytest.raises(AssertionError):
            kref.solve(oracle, a, F, U0, m=m)


# ---------------------------------------------------------------- the recurred norm never grows
@pytest.mark.parametrize("shift", [0.0, 1e4])
@pytest.mark.parametrize("name", ["one", "smooth", "jump", "random"])
@pytest.mark.parametrize("N", [33, 64, 65, 100])
def test_history_is_monotone_between_restarts(oracle, N, name, shift):
    """rho_i <= rho_{i-1}*(1 + 1e-12), the project's scalar tolerance, over every step that is not a restart: GCR minimises
    the residual along q_k, whatever the preconditioner"""
    F, U0, a = problem(N, name)
    for m in (1, 4, 8):
        out = kref.solve(oracle, a, F, U0, m=m, rtol=1e-9, shift=shift)
        steps = kref.nonrestart_steps(out["history"], out["records"])
        assert m > 1 or not steps           # (m = 1 restarts in every iteration)
        for i, (before, after) in enumerate(steps):
            assert after <= before * (1.0 + 1e-12), (N, name, shift, m, i, before, after)
        assert len(out["history"]) == out["cycles"] + 1 and not out["breakdown"]


def test_no_growth_where_the_plain_cycle_diverges(oracle):
    """V(1, 2) with omega = 1 on the random field at N = 65: the plain iteration grows beyond 1e20"""
    F, U0, a = problem(65, "random")
    opts = dict(pre=1, post=2, omega=1.0, rtol=1e-9)
    _, hist, _, conv = kref.plain(oracle, a, F, U0, **opts)
    assert not conv and hist[-1] > 1e20 * hist[0]
    out = kref.solve(oracle, a, F, U0, m=8, **opts)
    for before, after in kref.nonrestart_steps(out["history"], out["records"]):
        assert after <= before * (1.0 + 1e-12)


# ---------------------------------------------------------------- iteration counts, pinned as the restatement measures them
PINNED = {33: 34, 64: 40, 65: 43}   # GCR(8) iterations to rtol = 1e-9 on `random`; the plain cycle: not converged in 50


@pytest.mark.parametrize("N", sorted(PINNED))
def test_random_field_converges_with_gcr8_and_not_without(oracle, N):
    F, U0, a = problem(N, "random")
    _, hist, cycles, conv = kref.plain(oracle, a, F, U0, rtol=1e-9)
    assert not conv and cycles == 50
    margins = []
    out = kref.solve(oracle, a, F, U0, m=8, rtol=1e-9, margins=margins)
    ref.assert_qualified(margins, f"N={N}")
    print(f"N={N} random: plain {hist[-1]:.3e} after 50, GCR(8) {out['cycles']} iterations to {out['history'][-1]:.3e}")
    assert out["converged"] and out["cycles"] == PINNED[N]
    assert out["records"][-1]["restarted"]           # converged is stated on a recomputed residual
    rU = vref.residual_norm_ld(a, out["U"], F, 1.0, 0.0)
    assert rU <= out["tol"] + vref.residual_rounding_bound(a, out["U"], F, 1.0, 0.0)


@pytest.mark.parametrize("N,pinned", [(65, (24, 15)), (129, (31, 16))])
def test_jump_takes_no_more_iterations_than_plain_cycles(oracle, N, pinned):
    F, U0, a = problem(N, "jump")
    _, _, cycles, conv = kref.plain(oracle, a, F, U0, rtol=1e-9)
    out = kref.solve(oracle, a, F, U0, m=8, rtol=1e-9)
    assert conv and out["converged"] and out["cycles"] <= cycles
    assert (cycles, out["cycles"]) == pinned
    rU = vref.residual_norm_ld(a, out["U"], F, 1.0, 0.0)
    assert rU <= out["tol"] + vref.residual_rounding_bound(a, out["U"], F, 1.0, 0.0)


# ---------------------------------------------------------------- truth
@pytest.mark.parametrize("name", ["smooth", "jump"])
@pytest.mark.parametrize("N", [17, 33])
def test_against_the_direct_solution(oracle, N, name):
    """the bound form of test_heat_vc_cpu.py: ||U - U*|| <= (r(U) + r(U*)) / (a_min*lambda_min + sigma)"""
    L, rtol, shift = 1.5, 1e-10, 10.0
    F, U0 = ref.random_problem(N, 5000 + N)
    a = vref.field(name, N, L)
    out = kref.solve(oracle, a, F, U0, L, m=8, rtol=rtol, shift=shift)
    assert out["converged"]
    U = out["U"]
    X = vref.direct_solution(a, F, U0, L, shift)
    rU, rX = vref.residual_norm_ld(a, U, F, L, shift), vref.residual_norm_ld(a, X, F, L, shift)
    err = ref.norm_ld(U.astype(LD) - X)
    assert err <= (rU + rX) / (LD(float(a.min())) * ref.lambda_min(N, L) + LD(shift))
    assert rU <= rtol * ref.ref_norm(F) + vref.residual_rounding_bound(a, U, F, L, shift)
    assert np.array_equal(U[0], U0[0]) and np.array_equal(U[:, -1], U0[:, -1])     # the rim is never written


# ---------------------------------------------------------------- m beyond the iteration count
def test_large_m_never_restarts_before_convergence_and_histories_agree(oracle):
    F, U0, a = problem(65, "smooth")
    out = {m: kref.solve(oracle, a, F, U0, m=m, rtol=1e-9) for m in (12, 16)}
    n = out[12]["cycles"]
    assert n <= 12 and out[12]["converged"]
    flags = [rec["restarted"] for rec in out[12]["records"]]
    assert flags == [False] * (n - 1) + [True]       # the one restart is the recomputation that states convergence
    assert out[12]["history"] == out[16]["history"]
    assert np.array_equal(out[12]["U"], out[16]["U"])


def test_start_that_meets_the_tolerance_and_zero_problem(oracle):
    N = 33
    F, U0, a = problem(N, "smooth")
    done = kref.solve(oracle, a, F, U0, m=8, rtol=1e-9)
    again = kref.solve(oracle, a, F, done["U"], m=8, rtol=1e-9)
    assert again["cycles"] == 0 and again["converged"] and not again["records"]
    zero = kref.solve(oracle, a, np.zeros((N, N)), np.zeros((N, N)), m=8)
    assert zero["cycles"] == 0 and zero["converged"] and not zero["breakdown"]
