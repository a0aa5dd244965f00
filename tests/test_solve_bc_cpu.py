"""Boundary kinds per side (include/mg_bc.h) without a GPU: the header against the binding and the library's exports; the
restatement (tests/_bc_ref.py) against what the header promises -- four Dirichlet sides are _solve_vc_ref bit for bit, the
prolongation table reproduces linear fields, the operator is symmetric under the trapezoid weights and conserves, the cycle
converges for every kind the issue names, and flux data is folded in to second order."""
import os
import re

import numpy as np
import pytest

import _bc_ref as bref
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
SYMBOLS = ("mg_solver_set_boundary", "mg_solver_boundary", "mg_neumannSource", "mg_applyOperatorBoundary",
           "mg_boundary_prolongation_table", "mg_sweepBoundary", "mg_residualBoundary", "mg_restrictBoundary",
           "mg_prolongAddBoundary", "mg_heat_rhs_boundary", "mg_heat_stepper_set_boundary")
# the pinned tables of the parent: their symbol sets must not move
ABI_VC_SYMBOLS = ("mg_solver_set_coefficient", "mg_solver_has_coefficient", "mg_applyOperator", "mg_coarsenCoefficient",
                  "mg_sweepCoefficient", "mg_residualCoefficient")
SOLVE_OPTS_FIELDS = ["pre", "post", "N_min", "omega", "coarse_rtol", "coarse_atol", "coarse_max_iters", "rtol", "atol",
                     "max_cycles", "fmg", "shift"]


def test_header_declares_what_the_binding_binds_and_the_library_exports():
    import multigrid_poisson_solver_amd as m
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mg_bc.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))
    assert declared == sorted(SYMBOLS) == sorted(m.ABI_BC)
    lib = m.load_library()
    others = (m.ABI, m.ABI_FMG, m.ABI_HEAT, m.ABI_VC, m.ABI_HEAT_VC, m.ABI_VC_BATCH, m.ABI_KRYLOV, m.ABI_KRYLOV_BATCH,
              m.ABI_ADJOINT, m.ABI_EIGS)
    for name in declared:
        assert hasattr(lib, name) and not any(name in abi for abi in others), name
        assert getattr(lib, name).argtypes == m.ABI_BC[name][1] and getattr(lib, name).restype is m.ABI_BC[name][0]
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(m.ABI_BC[name][1]), name
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    # (after every header it builds on; the last two includes of mg_hip.h are pinned by tests/test_solve_krylov_batched_cpu.py)
    includes = re.findall(r'#include "(mg_\w+\.h)"', hip)
    assert hip.count('#include "mg_bc.h"') == 1 and includes[-3:] == ["mg_bc.h", "mg_krylov_batch.h", "mg_krylov.h"]
    assert all(hip.index('#include "%s"' % h) < hip.index('#include "mg_bc.h"') for h in ("mg_heat_vc.h", "mg_varcoef.h", "mg_eigs.h"))
    assert "oundary(" not in re.sub(r"/\*.*?\*/", "", hip, flags=re.S)   # nothing else went into mg_hip.h
    assert sorted(m.ABI_VC) == sorted(ABI_VC_SYMBOLS)
    assert len(m.ABI) == 96 and not any("oundary" in name or "eumann" in name for name in m.ABI)
    assert [f for f, _ in m.SolveOpts._fields_] == SOLVE_OPTS_FIELDS
    assert b"0.2.2" in lib.mg_version()
    assert (m.DIRICHLET, m.NEUMANN) == (0, 1)
    for f in (m.Solver, m.Solver.set_boundary, m.solve, m.HeatStepper.set_boundary, m.neumann_source, m.heat_rhs_boundary):
        assert "S, N, W, E" in f.__doc__, f.__name__
    for f in (m.Solver, m.Solver.set_boundary, m.solve):
        assert "part of the guess and is written" in f.__doc__, f.__name__
    import inspect
    # (bc= rides in Solver's **opts: tests/test_solve_krylov_cpu.py pins the named parameters)
    assert list(inspect.signature(m.Solver.__init__).parameters) == ["self", "N", "L", "coef", "krylov", "opts"]
    assert 'opts.pop("bc", None)' in inspect.getsource(m.Solver.__init__) and "bc=kinds" in m.Solver.__doc__
    for f in (m.BatchSolver.__init__, m.EigenSolver.__init__):     # the untouched solvers get no setter
        assert "bc" not in inspect.signature(f).parameters, f.__qualname__
    assert not hasattr(m.BatchSolver, "set_boundary") and not hasattr(m.EigenSolver, "set_boundary")


def test_binding_parses_kinds():
    import multigrid_poisson_solver_amd as m
    assert list(m._kinds("ndnd")) == [1, 0, 1, 0] and list(m._kinds((0, 1, 1, 0))) == [0, 1, 1, 0] and list(m._kinds(None)) == [0] * 4
    for bad in ("ndn", "ndnx", (0, 1, 1)):
        with pytest.raises(m.MGError):
            m._kinds(bad)
    assert len(bref.ALL_KINDS) == 16 and bref.kinds("nddn") == (1, 0, 0, 1)


def test_prolongation_table_is_the_librarys():
    import multigrid_poisson_solver_amd as m
    for M, N in ((32, 64), (32, 65), (50, 100), (64, 129), (3, 7), (2, 4), (128, 257)):
        lo, w = m.boundary_prolongation_table(M, N)
        mine = bref.prolongation_table(M, N)
        assert np.array_equal(lo, mine[0])
        assert_bits(w, mine[1], f"prolongation weights {M} -> {N}")


# ---------------------------------------------------------------- four Dirichlet sides: _solve_vc_ref bit for bit
@pytest.mark.parametrize("shift", [0.0, 1e2])
@pytest.mark.parametrize("N", [7, 64, 100, 257])
def test_four_dirichlet_sides_are_the_variable_coefficient_restatement(oracle, N, shift):
    F, U = ref.random_problem(N, 900 + N)
    a = vref.field("exp", N)
    bc = "dddd"
    assert_bits(bref.weighted_sweeps(N, 1.0, bc, a, U, F, 0.8, 2, shift), vref.weighted_sweeps(N, 1.0, a, U, F, 0.8, 2, shift), "sweep")
    assert_bits(bref.weighted_sweeps(N, 1.0, bc, a, None, F, 0.8, 1, shift, zero_start=True),
                vref.weighted_sweeps(N, 1.0, a, None, F, 0.8, 1, shift, zero_start=True), "zero-start sweep")
    for sign in (1, -1):
        assert_bits(bref.residual(N, 1.0, bc, a, U, F, shift, sign), vref.residual(N, 1.0, a, U, F, shift, sign), "residual")
    assert_bits(bref.apply_operator(N, 1.0, bc, None, U, shift), vref.apply_operator(N, 1.0, None, U, shift), "operator, a = 1")
    assert bref.residual_norm(N, 1.0, bc, a, U, F, shift) == vref.residual_norm(N, 1.0, a, U, F, shift)
    assert bref.ref_norm(F, bc) == ref.ref_norm(F)
    M = N // 2
    D = vref.residual(N, 1.0, a, U, F, shift, -1)
    mine, theirs = bref.restrict(D, M, bc), oracle.doRestriction(N, D, M)
    assert_bits(mine[1:-1, 1:-1], theirs[1:-1, 1:-1], "restriction at the interior coarse points")
    assert not mine[0].any() and not mine[:, -1].any() and not np.signbit(mine[0]).any()
    if N <= 100:   # (the coarse solve takes N < 64)
        Nc = N if N == 7 else M
        Fc = F[:Nc, :Nc]
        ac = a[:Nc, :Nc]
        tb, tv = bref.rbgs_trace(Nc, 1.0, bc, ac, Fc, 0.0, 1e-2, 10000, shift), vref.rbgs_trace(Nc, 1.0, ac, Fc, 0.0, 1e-2, 10000, shift)
        assert_bits(tb[0], tv[0], "coarse solve")
        assert tb[1] == tv[1] and tb[2] == tv[2]


# ---------------------------------------------------------------- the prolongation table
@pytest.mark.parametrize("M,N", [(32, 64), (32, 65), (50, 100), (64, 129)])
def test_prolongation_table_reproduces_linear_fields(M, N):
    lo, w = bref.prolongation_table(M, N)
    assert lo.min() >= 0 and lo.max() <= M - 2 and w.min() >= 0.0 and w.max() <= 1.0
    pos = (lo + w) / float(M - 1)            # the position a fine point is interpolated at
    assert np.all(np.diff(pos) >= 0.0) and pos[0] == 0.0 and pos[-1] == 1.0
    xf, xc = np.arange(N) / float(N - 1), np.arange(M) / float(M - 1)
    assert np.max(np.abs(pos - xf)) <= 4 * 2.0 ** -53
    lin = lambda x: 0.7 + 1.3 * x[None, :] - 2.1 * x[:, None]
    got = bref.prolong_add(lin(xc), N, np.zeros((N, N)), "nnnn")
    # 4 products and 3 sums of values below 4 in magnitude, weights within an ulp of exact: 16 roundings of 4 * 2^-53
    assert np.max(np.abs(got - lin(xf))) <= 16 * 4 * 2.0 ** -53
    kept = bref.prolong_add(lin(xc), N, np.full((N, N), 5.0), "dnnd")
    assert np.all(kept[0] == 5.0) and np.all(kept[:, -1] == 5.0) and kept[-1, 0] != 5.0


# ---------------------------------------------------------------- symmetry and conservation of the operator
@pytest.mark.parametrize("N", [9, 12])
@pytest.mark.parametrize("bc", bref.ALL_KINDS)
def test_operator_is_symmetric_under_the_trapezoid_weights(bc, N):
    """B = diag(w)*A over the unknowns is symmetric, and the column sums of diag(w)*A_full -- every column, data points
    included -- vanish at sigma = 0: the rows of A annihilate constants, so by the symmetry the column sum of B at an unknown
    j is minus w_j times its coupling to data points.  It vanishes at every unknown without a data neighbour, which for four
    Neumann sides is every unknown: the scheme conserves sum w*u (the GPU conservation test rests on this).
    Tolerance: longdouble unit roundoff x row size x max |entry| per sum, summed over the at most N^2 rows of a column."""
    L = 1.3
    a = vref.field("exp", N, L)
    A, unk = bref.dense_operator(a, N, L, 0.0, bc)
    w = bref.trapezoid_weights(N, bc).reshape(-1)[unk]
    B = w[:, None] * A[:, unk]
    eps = LD(np.finfo(LD).eps)
    tol = eps * 5 * np.max(np.abs(A))
    assert np.max(np.abs(B - B.T)) <= tol
    assert np.max(np.abs(np.sum(A, axis=1))) <= tol                       # rows annihilate constants
    data = np.setdiff1d(np.arange(N * N), unk)
    coupling = np.sum(A[:, data], axis=1) if data.size else np.zeros(unk.size, dtype=LD)
    col = np.sum(B, axis=0)
    assert np.max(np.abs(col + w * coupling)) <= tol * unk.size
    free = coupling == 0
    assert np.max(np.abs(col[free])) <= tol * unk.size
    if bc == "nnnn":
        assert free.all()
    # and sigma sits on the diagonal alone
    A2, _ = bref.dense_operator(a, N, L, 7.0, bc)
    assert np.max(np.abs((A2 - A)[:, unk] + 7 * np.eye(unk.size, dtype=LD))) <= tol


def test_dense_operator_is_the_restatements_operator():
    """the longdouble matrix and the fp64 restatement agree to the rounding of the latter, at every kind"""
    N, L, shift = 12, 0.7, 3.0
    _, U = ref.random_problem(N, 5)
    a = vref.field("exp", N, L)
    for bc in bref.ALL_KINDS:
        A, unk = bref.dense_operator(a, N, L, shift, bc)
        want = A @ U.astype(LD).reshape(-1)
        got = bref.apply_operator(N, L, bc, a, U, shift).reshape(-1)[unk]
        scale = np.abs(A) @ np.abs(U).astype(LD).reshape(-1)
        assert np.all(np.abs(got - want) <= 16 * ref.U53 * scale), bc
        assert not bref.apply_operator(N, L, bc, a, U, shift).reshape(-1)[np.setdiff1d(np.arange(N * N), unk)].any()


# ---------------------------------------------------------------- convergence of the restatement
CASES = [("nnnn", 1e2), ("nnnn", 1e4), ("ddnd", 0.0), ("ndnd", 0.0), ("nndd", 0.0), ("nnnd", 0.0)]


@pytest.mark.parametrize("name", ["one", "smooth", "exp"])
@pytest.mark.parametrize("N", [33, 64, 65, 100, 129])
def test_convergence(N, name):
    F, U0 = ref.random_problem(N, 500 + N)
    a = vref.field(name, N)
    for bc, shift in CASES:
        capped, iters = [], []
        U, hist, cycles, conv = bref.solve(a, F, U0, bc, 1.0, capped=capped, iters=iters, rtol=1e-9, shift=shift, max_cycles=50)
        print(f"N={N} a={name} {bc} sigma={shift:g}: {cycles} cycles, largest coarse solve {max(iters)} iterations")
        assert conv and cycles <= 50 and not any(capped), (bc, shift, cycles)
        # data points are never written
        m = bref.mask(N, bc)
        assert_bits(U[~m], U0[~m], "data points")


# ---------------------------------------------------------------- second order with flux data
def _exact_problem(N, bc, shift):
    """u = sin(1.3x + 0.4)*cos(0.9y + 0.2) + 0.3xy, a = 1 + x + 2y on the unit square: F = div(a grad u) - sigma*u in closed
    form, g = the outward normal derivative on the four sides, the data rims from u (x along columns, y along rows)"""
    x, y = vref.grid(N, 1.0)
    s, c = np.sin(1.3 * x + 0.4), np.cos(1.3 * x + 0.4)
    sy, cy = np.sin(0.9 * y + 0.2), np.cos(0.9 * y + 0.2)
    u = s * cy + 0.3 * x * y
    ux = 1.3 * c * cy + 0.3 * y
    uy = -0.9 * s * sy + 0.3 * x
    lap = -(1.3 ** 2 + 0.9 ** 2) * s * cy
    a = 1.0 + x + 2.0 * y + 0.0 * u
    F = a * lap + 1.0 * ux + 2.0 * uy - shift * u
    g = np.stack([-uy[0, :], uy[-1, :], -ux[:, 0], ux[:, -1]])
    return u, a, F, g


@pytest.mark.parametrize("bc,shift", [("nnnn", 50.0), ("ddnd", 0.0), ("ndnd", 0.0), ("nnnd", 3.0)])
def test_flux_data_is_second_order(bc, shift):
    """max-error ratios at N = 33 -> 65 -> 129 inside [3.8, 4.2] with the nodal coefficient in the flux term; the face-
    averaged folding is first order (ratios near 2) and must fall outside"""
    errs = {False: [], True: []}
    for N in (33, 65, 129):
        u, a, F, g = _exact_problem(N, bc, shift)
        m = bref.mask(N, bc)
        U0 = np.where(m, 0.0, u)
        for face_averaged in (False, True):
            Fe = bref.neumann_source(N, 1.0, bc, a, F, g, face_averaged=face_averaged)
            U, hist, cycles, conv = bref.solve(a, Fe, U0, bc, 1.0, rtol=1e-11, shift=shift)
            assert conv, (bc, N, cycles, hist[-1])
            errs[face_averaged].append(float(np.max(np.abs(U - u))))
    ratios = {k: [e[0] / e[1], e[1] / e[2]] for k, e in errs.items()}
    print(f"{bc} sigma={shift:g}: nodal {errs[False]} ratios {ratios[False]}; face-averaged {errs[True]} ratios {ratios[True]}")
    assert all(3.8 <= r <= 4.2 for r in ratios[False]), ratios[False]
    assert not all(3.8 <= r <= 4.2 for r in ratios[True]), ratios[True]


def test_direct_solution_solves_the_discrete_system():
    """the dense reference of the GPU truth tests: its longdouble residual is at rounding level, data points untouched"""
    N = 17
    F, U0 = ref.random_problem(N, 77)
    a = vref.field("exp", N)
    for bc, shift in (("nnnn", 25.0), ("ndnd", 0.0), ("dddd", 0.0)):
        X, ninv = bref.direct_solution(a, F, U0, 1.0, shift, bc, want_inverse_norm=True)
        m = bref.mask(N, bc)
        assert_bits(np.asarray(X, dtype=np.float64)[~m], U0[~m], "data points")
        r = bref.residual_ld(a, X, F, 1.0, shift, bc)
        assert np.max(np.abs(r)) <= 1e-3 * bref.residual_rounding_bound(a, np.asarray(X, dtype=np.float64), F, 1.0, shift, bc)
        assert ninv > 0
    Xd = bref.direct_solution(a, F, U0, 1.0, 0.0, "dddd")
    assert np.max(np.abs(Xd - vref.direct_solution(a, F, U0, 1.0, 0.0))) <= 1e-12
