"""The residual-tolerance solver's restatement (tests/_solve_ref.py) against the oracle, on the CPU: the weighted
sweep at omega = 1 is doSmoothing, one restatement cycle is one cycle of the reference driver, and the stall of the
unweighted smoother that motivates omega < 1 ("Solving to a residual tolerance")."""
import ctypes as C
import os

import numpy as np
import pytest

import _solve_ref as ref
from conftest import assert_bits


@pytest.mark.parametrize("N", [33, 64, 100])
def test_weighted_sweep_at_omega_one_is_doSmoothing(oracle, N):
    F, U = ref.random_problem(N, 11)
    want, _ = oracle.doSmoothing(N, 1.0, U, F, 3)
    assert_bits(ref.weighted_sweeps(N, 1.0, U, F, 1.0, 3), want, f"weighted sweep omega=1 N={N}")


@pytest.mark.parametrize("N", [64, 65])
def test_restatement_cycle_is_the_drivers_second_cycle(oracle, tmp_path, N):
    one = oracle.run_cycle_file(ref.write_vcycles(str(tmp_path / "V1.txt"), N, 8, 3, 1e-7, 1), want_report=False)
    two = oracle.run_cycle_file(ref.write_vcycles(str(tmp_path / "V2.txt"), N, 8, 3, 1e-7, 2), want_report=False)
    assert one["status"] == 0 and two["status"] == 0
    F = oracle.getSource(N)
    got = ref.cycle(oracle, F, one["U"], omega=1.0, coarse_rtol=0.0, coarse_atol=1e-7)
    assert_bits(got, two["U"], f"restatement cycle from U_1 vs the chained two-cycle file N={N}", zero_sign=True)


def _relative_history(oracle, N, omega, cycles):
    F = oracle.getSource(N)
    _, hist, k, _ = ref.solve(oracle, F, omega=omega, coarse_rtol=1e-2, rtol=1e-10, max_cycles=cycles)
    return [h / ref.ref_norm(F) for h in hist], k


def test_unweighted_smoother_stalls(oracle):
    rel, k = _relative_history(oracle, 257, 1.0, 10)
    assert k == 10 and min(rel) > 1e-6, rel


def test_weighted_smoother_converges(oracle):
    rel, k = _relative_history(oracle, 257, 0.8, 10)
    assert rel[-1] <= 1e-10 and k <= 10, rel


def test_solver_symbols_and_defaults():
    """The library exports the solver (host-only call: no device needed) with the documented defaults."""
    import multigrid_poisson_solver_amd as m
    lib = m.load_library()
    for name in ("mg_solve_opts_default", "mg_solver_create", "mg_solver_solve", "mg_solver_destroy"):
        assert hasattr(lib, name) and name in m.ABI
    o = m.SolveOpts()
    lib.mg_solve_opts_default(C.byref(o))
    assert (o.pre, o.post, o.N_min, o.omega, o.coarse_rtol, o.rtol, o.max_cycles) == (3, 3, 8, 0.8, 1e-2, 1e-10, 50)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mg_hip.h")).read()
    for name in ("mg_solve_opts_default", "mg_solver_create", "mg_solver_solve", "mg_solver_destroy"):
        assert name + "(" in header


# ---------------------------------------------------------------- the independent references of tests/_solve_ref.py
@pytest.mark.parametrize("N", [3, 4, 7, 16, 33, 63])
def test_rbgs_trace_is_doExactSolver(oracle, N):
    F, _ = ref.random_problem(N, 21 + N)
    for L, rtol in ((1.0, 1e-2), (2.5, 1e-4)):
        U, err0, errs = ref.rbgs_trace(N, L, F, 0.0, rtol, 1 << 30)
        target = ref.coarse_target(F, 0.0, rtol)
        assert target == max(0.0, rtol * err0)
        assert ref.coarse_margin(N, L, F, 0.0, rtol, 1 << 30) >= ref.QUALIFY
        want = oracle.doExactSolver(N, L, F, target, 1)
        assert len(errs) == oracle.gs_iterations(), f"N={N} L={L}: {len(errs)} iterations, the oracle {oracle.gs_iterations()}"
        assert_bits(U, want, f"rbgs_trace N={N} L={L}")
        assert errs[-1] <= target and all(e > target for e in errs[:-1])


def test_rbgs_trace_stops_at_the_cap():
    F, _ = ref.random_problem(16, 2)
    _, _, errs = ref.rbgs_trace(16, 1.0, F, 1e-300, 0.0, 3)
    assert len(errs) == 3 and errs[-1] > 1e-300


@pytest.mark.parametrize("L", [0.3, 1.0, 7.0])
@pytest.mark.parametrize("N", [17, 100, 257])
def test_direct_solution_solves_the_discrete_system(N, L):
    F, U0 = ref.random_problem(N, 31 + N)
    X = ref.direct_solution(F, U0, L)
    assert X.dtype == np.longdouble
    for a, b in ((X[0], U0[0]), (X[-1], U0[-1]), (X[:, 0], U0[:, 0]), (X[:, -1], U0[:, -1])):
        assert np.array_equal(a.astype(np.float64), b)
    r = ref.residual_norm_ld(X, F, L)
    bound = ref.residual_rounding_bound(X, F, L)
    print(f"N={N} L={L}: residual {float(r):.3e}, bound {float(bound):.3e}")
    assert r <= bound
    # and the start is not the solution: the bound is not vacuous
    assert ref.residual_norm_ld(U0, F, L) > 1e6 * bound


def test_lambda_min_is_the_smallest_eigenvalue():
    """-A applied to the lowest sine mode returns lambda_min times it (zero rim)."""
    N, L = 33, 2.5
    k = np.arange(N).astype(np.longdouble)
    s = np.sin(np.longdouble(4) * np.arctan(np.longdouble(1)) * k / (N - 1))
    V = np.outer(s, s)
    V[0] = V[-1] = 0
    V[:, 0] = V[:, -1] = 0
    lam = ref.lambda_min(N, L)
    dx = L / (N - 1)
    assert float(lam) == pytest.approx(8 / dx ** 2 * np.sin(np.pi / (2 * (N - 1))) ** 2, rel=1e-13)
    assert ref.residual_norm_ld(V, -lam * V, L) <= 1e-15 * lam * ref.norm_ld(V)


@pytest.mark.parametrize("N", [64, 1025])
def test_cubic_problem_is_its_own_discrete_solution(N):
    L = 2.5
    F, U = ref.cubic_problem(N, L, 0.25, -0.5, ref.CUBIC)
    assert F.dtype == np.float64 and U.dtype == np.float64
    r = ref.residual_norm_ld(U, F, L)
    bound = ref.residual_rounding_bound(U, F, L)
    print(f"N={N}: residual of the rounded cubic {float(r):.3e}, bound {float(bound):.3e}")
    assert r <= bound
    assert ref.norm_ld(F) > 0 and ref.residual_norm_ld(ref.rim_only(U), F, L) > 1e6 * bound
    Fh, Uh = ref.cubic_problem(N, L, 0.25, -0.5, ref.HARMONIC)
    assert not Fh.any() and ref.residual_norm_ld(Uh, Fh, L) <= ref.residual_rounding_bound(Uh, Fh, L)


TRUTH_CASES = [(65, 2.5, 4), (129, 0.3, 16), (100, 7.0, 3), (127, 1.0, 32), (257, 2.5, 8)]


@pytest.mark.parametrize("N,L,N_min", TRUTH_CASES)
def test_restatement_converges_to_the_direct_solution(oracle, N, L, N_min):
    """||U - U*|| <= (r(U) + r(U*_fp64)) / lambda_min: e = A^-1 r with the smallest eigenvalue of the operator."""
    F, U0 = ref.random_problem(N, 500 + N)
    U, hist, k, conv = ref.solve(oracle, F, U0, L, N_min=N_min, rtol=1e-10, max_cycles=60)
    assert conv and k < 60
    r = ref.residual_norm_ld(U, F, L)
    assert r <= 1e-10 * ref.norm_ld(F) + ref.residual_rounding_bound(U, F, L)
    star = ref.direct_solution(F, U0, L).astype(np.float64)
    err = ref.norm_ld(U.astype(np.longdouble) - star.astype(np.longdouble))
    bound = (r + ref.residual_norm_ld(star, F, L)) / ref.lambda_min(N, L)
    print(f"N={N} L={L} N_min={N_min}: {k} cycles, error {float(err):.3e}, bound {float(bound):.3e}")
    assert err <= bound
