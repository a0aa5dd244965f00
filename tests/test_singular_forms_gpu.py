"""Whole solves of the pure Neumann problem (include/mg_singular.h) at the sizes whose top level runs the column-pair form (514,
1026: an odd level below) and the non-temporal form (4096): the "nnnn", sigma = 0 instantiations of the streaming boundary
kernels inside a cycle, the solver-owned Ft fed by the pair form of k_shift, s->part shared between the norms and k_wsum, and
the final shift of the caller's U in place.  tests/test_singular_gpu.py holds k_wsum and k_shift to the restatement alone at
512, 514 and 4096 and runs whole solves at sizes with one column per lane; its composition test, parametrised from
tests/_singular_forms_cases.py, is the whole-solve bit check at 4096.

  restatement  two cycles at 514 and 1026, with and without a coefficient, V(3,3) and V(1,2), target mean 2.5: what
               test_singular_gpu._compare asserts -- U bit for bit, cycles, converged, compat_defect and mean_before with ==,
               history and ref_norm to 1e-12, F read only, a second run bit-identical, the gauge of U in longdouble.
  modes        the truth is a formula: F = fp64(c*lambda*U*) + d for a discrete eigenmode U* of the mirrored operator, whose
               weighted mean vanishes, so the answer is U* + mean for any incompatibility d (_exact.check_singular_mode_solve:
               max|U - X| <= 2*(||r(U)|| + ||r(X)||)/lambda+ + the gauge term, residuals in longdouble against Ft; teeth 1e-6,
               at 4096 1e-4 with rtol 1e-9, 1e-10 lying below the rounding floor there).
The cases are tests/_singular_forms_cases.py's, which says how they were chosen; tests/test_singular_forms_cpu.py proves on
the restatement what they rest on.

Measured on the MI355X (6 whole solves, 6 mode solves; every figure is also the numpy restatement's to the digits shown):
  restatement  all six bit-identical; compat_defect 0.12513886418458586 at 514 and 0.1248938780550747 at 1026, mean_before
               between -1.09 and 0.33 for the target 2.5; 0.1 s at 514, 0.35 s at 1026 (the restatement's two cycles).
  modes        514: |U - X| 1.9e-11, 2.0e-11 (c = 2) and 1.5e-12 (mode (0, 1)) against bounds 8.7e-8, 9.3e-8 and 2.7e-8, 10, 10
               and 9 cycles; 1026: 2.0e-11 against 3.3e-7 and 2.6e-7 (c = 2), 10 cycles; 4096: 1.9e-10 against 1.3e-5, 9 cycles,
               r(U) 6.3e-6, r(X) 4.0e-6.  compat_defect is d exactly for d != 0 and -3.3e-17 for d = 0 (bound 2.9e-11); the
               gauge term is at most 2.4e-16; res lies 4e-10 .. 1.2e-6 from ||r(U)|| against rounding bounds 4.1e-7 .. 2.1e-4 (the
               final shift rounds U once more after res was taken); |mean_w(U) - mean| at most 2.4e-16 against 4.4e-11 .. 2.8e-9.
The mode at 4096 takes 3.5 s, nearly all of it the host's longdouble residuals and means on 16.8 million points; everything
else is below half a second."""
import numpy as np
import pytest

import _exact as ex
import _singular_forms_cases as cases
from test_singular_gpu import _compare, ptable, rtable

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,name,pp", cases.SOLVE_CASES)
def test_whole_solves_at_the_pair_sizes(mg, N, name, pp):
    """test_singular_gpu's whole-solve comparison at 514 -> 257 and 1026 -> 513 -> 256, every coarse solve qualified with the
    library's own tables first"""
    case = cases.restated_case(N, name, pp, rtable(mg), ptable(mg))
    got, info = _compare(mg, case, mean=cases.SOLVE_MEAN, **cases.solve_opts(pp))
    assert info["cycles"] == cases.CYCLES and abs(info["mean_before"] - cases.SOLVE_MEAN) > 1e-3   # (the shift did something)


@pytest.mark.parametrize("N,L,kl,coef,d,mean,rtol,teeth", cases.MODE_CASES)
def test_mode_solves(mg, N, L, kl, coef, d, mean, rtol, teeth):
    """zero start; the assertions of _exact.check_singular_mode_solve; F is read only.  At 4096 nearly all of the time is the
    host's longdouble residuals and means on 16.8 million points."""
    star, F, lam_plus = cases.mode_problem(N, L, kl, coef, d)
    F0 = F.copy()
    U, info = mg.solve(F, np.zeros((N, N)), L, coef=cases.mode_coef(N, coef), bc=cases.BC, mean=mean, rtol=rtol)
    assert np.array_equal(F, F0) and info["mean"] == mean
    ex.check_singular_mode_solve(U, info, star, F, L, d, mean, lam_plus, f"N={N} L={L} mode {kl} coef={coef} d={d} mean={mean}", coef, teeth)
