"""The full-multigrid start (mg_solve_opts.fmg) without a GPU: the interpolation table of the ABI against an independent
np.longdouble Lagrange table, and what the option promises, asserted on the restatement (tests/_solve_fmg_ref.py): after the
FMG pass and ONE cycle the algebraic error is below the discretisation error, and a solve to rtol 1e-9 never needs more
cycles than a cold start."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _solve_fmg_ref as fref
import _solve_ref as ref
import _solve_shift_ref as sref
from conftest import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
ULP1 = 2.0 ** -52
PAIRS = [(3, 6), (3, 7), (4, 8), (8, 16), (50, 100), (127, 255), (128, 256), (129, 257), (512, 1024), (513, 1025), (4096, 8192),
         (16, 8), (257, 128), (1024, 512), (1025, 512), (100, 50)]


@pytest.mark.parametrize("N_src,N_dst", PAIRS)
def test_table_against_longdouble_lagrange(N_src, N_dst):
    base, w = fref.abi_table(N_src, N_dst)
    want_base, want = fref.lagrange_table_ld(N_src, N_dst)
    m = min(4, N_src)
    assert np.array_equal(base, want_base)
    assert base.min() >= 0 and base.max() + m <= N_src
    assert np.all(np.abs(w.astype(LD) - want) <= np.spacing(np.abs(w)).astype(LD)), "a weight is more than 1 ulp from the longdouble table"
    assert np.all(w[:, m:] == 0.0)
    assert np.all(np.abs(np.sum(w.astype(LD), axis=1) - 1) <= 4 * ULP1), "a row does not sum to 1 within 4 ulp"
    # a destination point on a node: weight exactly 1 there, exactly +0 elsewhere
    for i in (0, N_dst - 1):
        k = (i * (N_src - 1)) // (N_dst - 1) - base[i]
        assert w[i, k] == 1.0 and np.count_nonzero(w[i]) == 1 and not np.any(np.signbit(w[i]))


@pytest.mark.parametrize("N_src,N_dst", PAIRS)
def test_table_reproduces_cubics(N_src, N_dst):
    """sum_k w_k p(x_k) = p(t) for every polynomial of degree < m: in longdouble with the fp64 weights, up to the weights'
    rounding (each within 1 ulp, |w| <= 1.25 on the interval the table is used on: 4 * 1.25 ulp of max|p|, doubled for the
    longdouble evaluation)."""
    base, w = fref.abi_table(N_src, N_dst)
    m = min(4, N_src)
    assert np.max(np.abs(w)) <= 1.25
    i = np.arange(N_dst)
    t = (i * (N_src - 1)).astype(LD) / LD(N_dst - 1)
    c = t[N_dst // 2]                                    # centred, scaled nodes: |x| <= 1
    s = LD(max(N_src - 1, 1))
    for coeffs in ([1.0, 0, 0, 0], [0.3, -1.0, 0, 0], [0.5, 1.0, -2.0, 0], [0.5, 1.0, -2.0, 0.7][:m] + [0] * (4 - m)):
        p = lambda x: sum(LD(a) * ((x - c) / s) ** k for k, a in enumerate(coeffs))
        nodes = (base[:, None] + np.arange(m)[None, :]).astype(LD)
        got = np.sum(w[:, :m].astype(LD) * p(nodes), axis=1)
        scale = float(np.max(np.abs(p(np.arange(N_src).astype(LD)))))
        assert np.max(np.abs(got - p(t))) <= 10 * ULP1 * scale


def test_prolong_cubic_restatement_is_exact_on_a_bilinear_field_of_small_integers():
    """x + 2y on integers: every product and sum of the fixed evaluation order stays far from rounding only through the
    weights; against longdouble within a few ulp, and the rim rows/columns of the result are the source's rim."""
    Ns, Nd = 9, 18
    y, x = np.meshgrid(np.arange(Ns), np.arange(Ns), indexing="ij")
    Uc = (x + 2.0 * y).astype(np.float64)
    P = fref.prolong_cubic(Uc, Nd)
    t = np.arange(Nd) * (Ns - 1) / (Nd - 1)
    want = t[None, :] + 2.0 * t[:, None]
    np.testing.assert_allclose(P, want, rtol=0, atol=64 * ULP1 * 24)
    assert P[0, 0] == Uc[0, 0] and P[-1, -1] == Uc[-1, -1] and P[0, -1] == Uc[0, -1]


def test_fmg_is_a_struct_field_with_default_zero_and_documented():
    import multigrid_poisson_solver_amd as m
    assert ("fmg", C.c_int) in m.SolveOpts._fields_
    o = m.SolveOpts()
    o.fmg = 5
    m.load_library().mg_solve_opts_default(C.byref(o))
    assert o.fmg == 0 and o.shift == 0.0 and o.max_cycles == 50
    header = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    body = re.search(r"typedef struct mg_solve_opts \{(.*?)\} mg_solve_opts;", header, re.S).group(1)
    assert re.search(r"\bint\s+fmg;", body)
    # the field fills the alignment hole in front of shift: no 0.2 field moves, the struct does not grow
    assert m.SolveOpts.fmg.offset == m.SolveOpts.max_cycles.offset + 4 and m.SolveOpts.shift.offset == m.SolveOpts.max_cycles.offset + 8
    assert C.sizeof(m.SolveOpts) == m.SolveOpts.shift.offset + 8
    for f in (m.solve_opts, m.Solver, m.BatchSolver, m.solve):
        assert "fmg" in f.__doc__, f.__name__
    fmg_header = open(os.path.join(ROOT, "include", "mg_fmg.h")).read()
    assert '#include "mg_fmg.h"' in header
    for name in ("mg_cubic_table", "mg_prolongCubic"):
        assert re.search(r"\b%s\s*\(" % name, fmg_header) and name in m.ABI_FMG and hasattr(m.load_library(), name)


@pytest.mark.parametrize("N,seed", [(64, 1), (100, 2), (129, 3)])
def test_fmg_zero_is_the_shifted_restatement_bit_for_bit(oracle, N, seed):
    F, U0 = ref.random_problem(N, seed)
    for shift in (0.0, 1e3):
        a = sref.solve(oracle, F, U0, max_cycles=3, rtol=1e-6, shift=shift)
        b = fref.solve(oracle, F, U0, max_cycles=3, rtol=1e-6, shift=shift, fmg=0)
        assert_bits(a[0], b[0], f"N={N} shift={shift:g}")
        assert a[1:] == b[1:]
    sz = ref.sizes(N, 8)
    assert_bits(sref.cycle(oracle, F, U0), fref.cycle(oracle, F, U0, 1.0, sz), "cycle at top level 0")
    # a cycle started at level 1 is the cycle of the level-1 problem
    F1, U1 = ref.random_problem(sz[1], seed + 10)
    assert_bits(sref.cycle(oracle, F1, U1), fref.cycle(oracle, F1, U1, 1.0, sz, top=1), "cycle at top level 1")


def test_start_that_meets_the_tolerance_is_left_alone(oracle):
    F, U0 = ref.random_problem(64, 4)
    U, hist, k, conv = fref.solve(oracle, F, U0, fmg=1, atol=1e30)
    assert k == 0 and conv and len(hist) == 1
    assert_bits(U, U0, "converged start")


def test_caller_interior_is_ignored_and_rim_kept(oracle):
    F, U0 = ref.random_problem(65, 5)
    other = U0.copy()
    other[1:-1, 1:-1] = 7.0
    a = fref.solve(oracle, F, U0, fmg=1, rtol=0.0, max_cycles=0)
    b = fref.solve(oracle, F, other, fmg=1, rtol=0.0, max_cycles=0)
    assert_bits(a[0], b[0], "two interiors, one guess")
    assert a[1] != b[1]          # history[0] is the norm of each caller's start
    for sl in ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1)):
        assert_bits(a[0][sl], U0[sl], "rim")
    assert not np.array_equal(a[0][1:-1, 1:-1], U0[1:-1, 1:-1])


# ---------------------------------------------------------------- what the option promises (N = 257, the defaults)
def _grid(N):
    t = np.arange(N).astype(LD) / LD(N - 1)
    return t[None, :], t[:, None]


def exp_sine_problem(N):
    """u = e^x cos 2y + sin(3x + y) on the unit square and its Laplacian -3 e^x cos 2y - 10 sin(3x + y)."""
    x, y = _grid(N)
    u = np.exp(x) * np.cos(2 * y) + np.sin(3 * x + y)
    f = -3 * np.exp(x) * np.cos(2 * y) - 10 * np.sin(3 * x + y)
    return f.astype(np.float64), u.astype(np.float64)


def rms(A):
    A = np.asarray(A, dtype=LD)[1:-1, 1:-1]
    return float(np.sqrt(np.mean(A * A)))


def problems(oracle, N):
    F, exact = exp_sine_problem(N)
    Fc, cubic = ref.cubic_problem(N, 1.0, 0.0, 0.0, ref.CUBIC)
    return {"getSource": (oracle.getSource(N, 1.0), oracle.getAnalytic(N, 1.0) * 0.0, oracle.getAnalytic(N, 1.0)),
            "exp_sine": (F, ref.rim_only(exact), exact), "cubic": (Fc, ref.rim_only(cubic), cubic)}


@pytest.mark.parametrize("name", ["getSource", "exp_sine", "cubic"])
def test_fmg_plus_one_cycle_is_below_the_discretisation_error_and_saves_cycles(oracle, name):
    """N = 257, V(3,3), omega 0.8, N_min 8, fmg = 1.  Measured on the restatement (CPU): cycles to rtol 1e-9 cold / FMG:
    getSource 8 / 5, exp_sine 10 / 4, cubic 11 / <= 4; ||U - U*_h||rms after FMG + 1 cycle over the discretisation error:
    getSource 0.16, exp_sine 0.07.  The 5-point stencil is exact on the cubic problem -- its discretisation error is
    rounding, nothing can be below it -- so there the claim asserted is that FMG + 1 cycle leaves a smaller error and a
    smaller residual than the cold start + 1 cycle."""
    N = 257
    F, U0, exact = problems(oracle, N)[name]
    if name == "getSource":
        assert not np.any(U0) and not np.any(ref.rim_only(exact))     # zero rim
    star = ref.direct_solution(F, U0, 1.0)
    disc = rms(star - exact.astype(LD))
    margins = []
    U1, h1, k1, _ = fref.solve(oracle, F, U0, fmg=1, rtol=0.0, max_cycles=1, margins=margins)
    C1, c1, _, _ = fref.solve(oracle, F, U0, fmg=0, rtol=0.0, max_cycles=1)
    alg = rms(U1.astype(LD) - star)
    cold = rms(C1.astype(LD) - star)
    print(f"{name}: discretisation error {disc:.3e}, after FMG + 1 cycle {alg:.3e} (ratio {alg / max(disc, 1e-300):.3g}), "
          f"cold + 1 cycle {cold:.3e}; residuals {h1[-1]:.3e} vs {c1[-1]:.3e}")
    assert k1 == 1
    if name == "cubic":
        assert disc <= 1e-13 and alg < cold and h1[-1] < c1[-1]
    else:
        assert alg < disc, f"{name}: algebraic error {alg:.3e} not below the discretisation error {disc:.3e}"
    _, hf, kf, cf = fref.solve(oracle, F, U0, fmg=1, rtol=1e-9)
    _, hc, kc, cc = fref.solve(oracle, F, U0, fmg=0, rtol=1e-9)
    print(f"{name}: cycles to rtol 1e-9: cold {kc}, FMG {kf}")
    assert cf and cc and kf <= kc, f"{name}: FMG needs {kf} cycles, the cold start {kc}"
