"""The `shift` option of the residual-tolerance solver (Laplace(U) - sigma*U = F) on the CPU: its restatement
(tests/_solve_shift_ref.py) reduces to the Poisson restatement and to the oracle's exact solver at sigma = 0, the option
is declared where the header says, the longdouble references agree with each other, and the shift never costs cycles."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _solve_ref as ref
import _solve_shift_ref as sref
from conftest import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = [1.0, 1e2, 1e4, 1e6, 1e8, 1e12]


@pytest.mark.parametrize("N,pp,omega", [(64, (3, 3), 0.8), (65, (2, 1), 2.0 / 3.0), (100, (1, 1), 1.0), (257, (3, 3), 0.8)])
def test_restatement_at_shift_zero_is_the_poisson_restatement(oracle, N, pp, omega):
    F, U = ref.random_problem(N, 31 + N)
    opts = dict(pre=pp[0], post=pp[1], omega=omega)
    want, got = U, U
    for k in range(2):
        want = ref.cycle(oracle, F, want, **opts)
        got = sref.cycle(oracle, F, got, shift=0.0, **opts)
        assert_bits(got, want, f"N={N} V{pp} omega={omega:.4f} cycle {k + 1}: shift = 0 vs _solve_ref.cycle")
    assert sref.residual_norm(N, 1.0, got, F, 0.0) == ref.residual_norm(oracle, N, 1.0, want, F)


def test_level_constants_at_shift_zero():
    for N, L, omega in ((17, 1.0, 0.8), (100, 1e-3, 2.0 / 3.0), (1025, 1e3, 1.0)):
        dx2, inv, d, q, c = sref.level_consts(N, L, 0.0, omega)
        assert (d, q, c) == (4.0, 0.25, 0.25 * omega) and inv == 1.0 / dx2


@pytest.mark.parametrize("N", [3, 4, 7, 16, 33, 63])
def test_shifted_rbgs_trace_at_zero_is_doExactSolver(oracle, N):
    F, _ = ref.random_problem(N, 21 + N)
    for L, rtol in ((1.0, 1e-2), (2.5, 1e-4)):
        U, err0, errs = sref.rbgs_trace(N, L, F, 0.0, rtol, 1 << 30, 0.0)
        target = ref.coarse_target(F, 0.0, rtol)
        assert sref.coarse_margin(N, L, F, 0.0, rtol, 1 << 30, 0.0) >= ref.QUALIFY
        want = oracle.doExactSolver(N, L, F, target, 1)
        assert_bits(U, want, f"shifted rbgs_trace at sigma = 0 vs doExactSolver N={N} L={L}", zero_sign=True)
        U0, e0, errs0 = ref.rbgs_trace(N, L, F, 0.0, rtol, 1 << 30)
        assert (e0, errs0) == (err0, errs)


def test_shift_is_the_last_option_and_defaults_to_zero():
    import multigrid_poisson_solver_amd as m
    assert m.SolveOpts._fields_[-1] == ("shift", C.c_double)
    lib = m.load_library()
    o = m.SolveOpts()
    o.shift = 123.0
    lib.mg_solve_opts_default(C.byref(o))
    assert o.shift == 0.0
    assert (o.pre, o.post, o.N_min, o.omega, o.coarse_rtol, o.rtol, o.max_cycles) == (3, 3, 8, 0.8, 1e-2, 1e-10, 50)
    for f in (m.solve_opts, m.Solver, m.BatchSolver, m.solve, m.solve_batched):
        assert "shift" in f.__doc__ and "1/(nu*dt)" in f.__doc__, f.__name__


def test_header_declares_shift_last():
    header = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    body = re.search(r"typedef struct mg_solve_opts \{(.*?)\} mg_solve_opts;", header, re.S).group(1)
    fields = [ln.split("/*")[0].strip() for ln in body.splitlines() if ln.split("/*")[0].strip()]
    assert fields[-1] == "double shift;", fields
    assert "d = 4 + shift*dx2" in header and "MG_ERR_ARG" in header
    assert b"0.2" in open(os.path.join(ROOT, "multigrid_poisson_solver_amd", "csrc", "mg_abi.cpp"), "rb").read().split(b"mg_version(void)")[1][:60]


@pytest.mark.parametrize("N,sigma", [(33, 0.0), (33, 1e3), (64, 1e5), (100, 1.0)])
def test_direct_solution_has_no_residual(N, sigma):
    """The two longdouble references against each other: the direct solution's residual is rounding in longdouble."""
    F, U = ref.random_problem(N, 77)
    for L in (1.0, 1e-3):
        X = sref.direct_solution(F, U, L, sigma)
        scale = float(ref._inv_ld(N, L)) * 8 + sigma
        assert float(sref.residual_norm_ld(X, F, L, sigma)) <= 1e-15 * scale * float(ref.norm_ld(X)) + 1e-15 * float(ref.norm_ld(F))
    if sigma == 0.0:
        assert np.array_equal(sref.direct_solution(F, U, 1.0, 0.0), ref.direct_solution(F, U, 1.0))
        assert sref.residual_rounding_bound(U, F, 1.0, 0.0) >= ref.residual_rounding_bound(U, F, 1.0)


@pytest.mark.parametrize("N,sigma", [(65, 1e2), (100, 1e6)])
def test_fp64_residual_within_the_derived_bound(N, sigma):
    F, U = ref.random_problem(N, 5)
    for L in (1.0, 1e3):
        got = sref.residual_norm(N, L, U, F, sigma)
        assert abs(sref.LD(got) - sref.residual_norm_ld(U, F, L, sigma)) <= sref.residual_rounding_bound(U, F, L, sigma)


def _cycles(oracle, N, sigma):
    F, U = ref.random_problem(N, 5)
    _, hist, k, conv = sref.solve(oracle, F, U, rtol=1e-10, shift=sigma)
    assert conv, (N, sigma, hist)
    return k


_BASE = {}


@pytest.mark.parametrize("N,sigma", [(N, s) for N in (256, 257) for s in SIGMAS] + [(1025, 1e4), (1025, 1e8)])
def test_shift_never_costs_cycles(oracle, N, sigma):
    """The convergence condition: on random_problem(N, 5), default options, rtol 1e-10, the shifted solve needs no more
    cycles than the Poisson solve (the shift only adds to the diagonal: the smoothing factor and the two-grid
    contraction do not get worse)."""
    if N not in _BASE:
        _BASE[N] = _cycles(oracle, N, 0.0)
    k = _cycles(oracle, N, sigma)
    print(f"N={N} sigma={sigma:g}: {k} cycles against {_BASE[N]} at sigma = 0")
    assert k <= _BASE[N]
