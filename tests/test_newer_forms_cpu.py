"""What tests/test_newer_forms_gpu.py rests on, without a GPU: the separated eigenvalue reference of tests/_eigs_ref.py
against the dense reference and the closed form, the gap condition of the quadratic bound for every new eigen case, and the
qualification of the FMG cases' seeds on the restatement alone."""
import numpy as np
import pytest

import _eigs_ref as er
import _newer_forms_cases as cases
import _solve_fmg_ref as fref
import _solve_ref as ref
from test_solve_fmg_gpu import problem

U53 = er.U53


def norm_bound(N, a_max, L=1.0):
    """||AA|| <= 8*a_max/dx^2 (Gershgorin), as rounding_term of tests/test_eigs_gpu.py takes it"""
    dx = L / (N - 1)
    return 8.0 * a_max / (dx * dx)


def routine_rounding(N, a_max, n_other):
    """What rounding alone may put between the separated reference and another one: a backward-stable symmetric eigenvalue
    routine on an n x n fp64 matrix returns eigenvalues within n*u*||AA|| of the matrix's own; the separated blocks have
    n = N - 2, the other routine n_other.  8 more u*||AA|| for the rounding of the matrix entries to fp64 on both sides and
    of mu_j (each entry is a sum of at most 5 terms rounded once)."""
    return ((N - 2) + n_other + 8) * U53 * norm_bound(N, a_max)


@pytest.mark.parametrize("axis", ["cols", "rows"])
@pytest.mark.parametrize("name", er.PROFILES)
@pytest.mark.parametrize("N", [17, 33, 65])
def test_separated_reference_meets_the_dense_one(N, name, axis):
    """Both orientations against numpy's eigvalsh of the dense (N-2)^2 matrix of _eigs_ref.dense_matrix.  Measured: the largest
    difference over the 13 lowest eigenvalues is 5.8e-12 at N = 17 (bound 5.6e-11 for `one`), 4.2e-11 at 33 (bound 9.1e-10)
    and 7.1e-10 at 65 (`jump`, bound 1.5e-7)."""
    a = er.layered(name, N, axis)
    sep = er.separated_eigenvalues(name, N, 1.0, 13)
    dense = np.linalg.eigvalsh(er.dense_matrix(a, N, 1.0).astype(np.float64))[:13]
    bound = routine_rounding(N, float(a.max()), (N - 2) * (N - 2))
    diff = float(np.max(np.abs(sep - dense)))
    print(f"N={N} {name}/{axis}: max |separated - dense| = {diff:.3e}, bound {bound:.3e}")
    assert np.all(np.diff(sep) >= 0) and diff <= bound, (N, name, axis, diff, bound)


def test_the_orientations_are_transposes_and_the_jump_sits_at_an_odd_index():
    for N in (17, 512, 514):
        for name in er.PROFILES:
            assert np.array_equal(er.layered(name, N, "cols"), er.layered(name, N, "rows").T)
        p = er.profile("jump", N)
        j0 = int(np.argmax(p > 1.0))
        assert j0 % 2 == 1 and 1 < j0 < N - 2 and p.max() / p.min() == 10.0
        s = er.profile("smooth", N)
        assert 2.9 < s.max() / s.min() <= 3.0


@pytest.mark.parametrize("N", [33, 512])
def test_separated_reference_meets_the_closed_form(N):
    """p == 1 against lambda_ij of the closed form (evaluated in fp64 directly: a few u*lambda).  Measured: 6.8e-13 at N = 33
    (bound 3.5e-11), 4.8e-10 at 512 (bound 1.2e-7)."""
    sep, closed = er.separated_eigenvalues("one", N, 1.0, 13), er.closed_form(N, 1.0, 13)
    bound = routine_rounding(N, 1.0, 0)
    diff = float(np.max(np.abs(sep - closed)))
    print(f"N={N}: max |separated - closed form| = {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound, (N, diff, bound)


def test_the_stopping_bound_on_j_leaves_nothing_out():
    """count = (N-2)^2 takes every block: the 13 lowest of ALL eigenvalues are the 13 the early stop returns"""
    N = 17
    for name in er.PROFILES:
        every = er.separated_eigenvalues(name, N, 1.0, (N - 2) * (N - 2))
        assert every.size == (N - 2) * (N - 2)
        assert np.array_equal(every[:13], er.separated_eigenvalues(name, N, 1.0, 13)), name


def test_every_new_eigen_case_meets_the_gap_condition():
    """From the reference alone: the k-th gap exceeds 4*rtol*sqrt(sum lam_i^2) >= 4||R||_F of any converged solve, so
    check_solution asserts the quadratic bound in every case of the new table -- none is left out."""
    assert len(cases.EIG_CASES) == 31 and {c[0] for c in cases.EIG_CASES} == {512, 513, 514, 1026}
    assert [c for c in cases.EIG_CASES if 3 * (c[3] + c[4]) == 36] == [(512, n, ax, 8, 4) for n, ax in cases.EIG_FIELDS]
    for N in (512, 514):   # the three rotation regimes at even N
        sizes = {3 * (k + g) for k, g in cases.EIG_BLOCKS[N]}
        assert any(m <= 12 for m in sizes) and any(12 < m <= 24 for m in sizes)
    # every case has its recorded restatement count, and each is at most half of the cap
    assert sorted(cases.RESTATEMENT_ITERS) == sorted({(c[0], c[3], c[4]) for c in cases.EIG_CASES})
    assert sum(len(v) for v in cases.RESTATEMENT_ITERS.values()) == len(cases.EIG_CASES)
    assert max(max(v) for v in cases.RESTATEMENT_ITERS.values()) <= cases.MAX_ITERS // 2
    assert cases.gap_left_out() == []
    # and the condition bites: k = 2 splits the pair lam_12 = lam_21 of `one`
    assert cases.gap_left_out([(512, "one", "cols", 2, 2)]) == [(512, "one", "cols", 2, 2)]


@pytest.mark.parametrize("N,fmg,shift", cases.FMG_CASES)
def test_the_fmg_seeds_qualify_on_the_restatement_alone(oracle, N, fmg, shift):
    """every coarse solve of the pass and of the two cycles has a margin >= 1e-10; the hierarchy has the even
    level above an odd one that the case is about"""
    sz = ref.sizes(N, 8)
    assert sz[0] % 2 == 0 and sz[0] >= 512 and sz[1] % 2 == 1, sz
    F, U0 = problem(N, 1.0, cases.SEED_FMG[N])
    margins = []
    fref.solve(oracle, F, U0, 1.0, margins=margins, rtol=0.0, atol=0.0, max_cycles=cases.FMG_CYCLES, fmg=fmg, shift=shift)
    assert len(margins) == 1 + fmg * (len(sz) - 2) + cases.FMG_CYCLES
    ref.assert_qualified(margins, f"N={N} fmg={fmg} shift={shift:g}")
