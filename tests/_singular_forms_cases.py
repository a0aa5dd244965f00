"""The case tables of tests/test_singular_forms_gpu.py and tests/test_solve_edges_gpu.py, shared with
tests/test_singular_forms_cpu.py, which checks on the CPU what the GPU cases rest on: the qualification of every seed (DESIGN
4.3), the distance of every norm from a stopping tolerance where cycle counts are compared, and the teeth of the bounds.
TEST INFRASTRUCTURE."""
import numpy as np

import _bc_ref as bref
import _exact as ex
import _singular_ref as sref
import _solve_ref as ref
import _solve_vc_ref as vref

LD = np.longdouble
BC = "nnnn"


# ---------------------------------------------------------------- whole singular solves against the restatement
def qualified_history(hist, tol, what):
    """the stopping decision must not hang on the last bits of a norm (the kernel sums it in its block partition); with a
    tolerance of zero (rtol = 0: the cycle count is max_cycles) no norm may be zero"""
    if tol == 0.0:
        worst = float("inf") if all(h > 0.0 for h in hist) else 0.0
    else:
        worst = min(abs(h - tol) / tol for h in hist)
    if not worst >= 1e-9:
        raise ValueError(f"{what}: input not qualified for comparing cycle counts, a norm within {worst:.3e} of the tolerance")


def restated(N, name, mean=0.0, seed=0, rtable=None, ptable=None, **opts):
    """(F, U0, a, U, history, cycles, converged, info) of one singular solve on the numpy restatement, every coarse solve and
    every stopping decision qualified; F = random + 0.125 (data that are not compatible), name: a field of _solve_vc_ref or
    None (no coefficient); rtable / ptable: the library's tables in the restatement's place"""
    F, U0 = ref.random_problem(N, seed)
    F = F + 0.125
    a = vref.field(name, N) if name else None
    margins = []
    U, hist, k, conv, info = sref.solve(a, F, U0, mean, 1.0, margins=margins, rtable=rtable, ptable=ptable, **opts)
    ref.assert_qualified(margins, f"N={N} a={name} {opts}")
    qualified_history(hist, max(opts["rtol"] * bref.ref_norm(info["Ft"], BC), opts.get("atol", 0.0)), f"N={N} a={name} {opts}")
    info["margins"] = margins
    return F, U0, a, U, hist, k, conv, info


# 514 -> 257 -> 128 ... and 1026 -> 513 -> 256 ...: a pair level on top, an odd level below it.  Seeds chosen on the
# restatement: coarse margins 0.018 .. 0.044 with its own tables (tests/test_singular_forms_cpu.py asserts them); the GPU test
# qualifies them again with the library's tables.
CYCLES = 2
SOLVE_MEAN = 2.5
SOLVE_SEED = {514: 5514, 1026: 6026}
SOLVE_CASES = [(N, name, pp) for N, pps in ((514, ((3, 3), (1, 2))), (1026, ((3, 3),))) for name in (None, "exp") for pp in pps]


def solve_opts(pp):
    return dict(pre=pp[0], post=pp[1], rtol=0.0, max_cycles=CYCLES)


def restated_case(N, name, pp, rtable=None, ptable=None):
    return restated(N, name, SOLVE_MEAN, SOLVE_SEED[N], rtable, ptable, **solve_opts(pp))


# the caller's own composition (test_singular_gpu.test_bit_identical_to_the_callers_own_composition): (N, cycles)
COMPOSITION_CASES = [(33, 3), (514, 2), (1026, 2), (4096, 2)]

# ---------------------------------------------------------------- singular solves of exact discrete modes
# (N, L, (k, l), coef, d, mean, rtol, teeth): F = fp64(c*lambda_kl*U*) + d with U* = mixed_mode(N, "nnnn", k, l), whose weighted
# mean vanishes, so the answer of the singular solve is U* + mean whatever the incompatibility d.  The bound of
# _exact.check_singular_mode_solve must stay below teeth*max|U*|; with ||r(U)|| <= rtol*||Ft|| it is a priori at most 2.6e-7
# at 514 and 6.4e-7 at 1026 (L = 7).  Measured on the numpy restatement (tests/test_singular_forms_cpu.py repeats it), mode
# (1, 2): bound 8.7e-8 and 7.9e-8 at 514, 2.6e-7 and 3.3e-7 at 1026, errors 1.9e-11 .. 2.0e-11 after 10 cycles each.  Mode (3, 4)
# has no teeth (1.15e-6 and 2.4e-6), a high mode has none at sigma = 0 at all: lambda / lambda+ is 1e4 .. 1e5.
# At 4096 rtol = 1e-10 lies below the rounding floor (||r(fp64(U*))|| = 4.0e-6 against a tolerance of 1.6e-6; no convergence in
# 50 cycles), so that case runs at 1e-9 with teeth 1e-4: a priori 2*(1.6e-5 + 4.0e-6)/1.579 = 2.5e-5; on the restatement 9
# cycles, error 1.9e-10, bound 1.3e-5 (126 s on the CPU, so no test repeats it).  A wrong sign or factor moves U by O(1), a
# dropped column of unknowns by about 1/N = 2.4e-4.
MODE_L = {514: 2.5, 1026: 7.0, 4096: 2.5}
MODE_RTOL, MODE_TEETH = 1e-10, 1e-6
MODE_RTOL_NT, MODE_TEETH_NT = 1e-9, 1e-4
GAUGES = [(0.375, -1.5), (-0.25, 2.5)]          # (d, mean)
MODE_CASES = [
    (514, MODE_L[514], (1, 2), None) + GAUGES[0] + (MODE_RTOL, MODE_TEETH),
    (514, MODE_L[514], (1, 2), 2.0) + GAUGES[1] + (MODE_RTOL, MODE_TEETH),
    (514, MODE_L[514], (0, 1), None, 0.0, 2.5, MODE_RTOL, MODE_TEETH),          # compatible data; not symmetric in the axes
    (1026, MODE_L[1026], (1, 2), None) + GAUGES[1] + (MODE_RTOL, MODE_TEETH),
    (1026, MODE_L[1026], (1, 2), 2.0) + GAUGES[0] + (MODE_RTOL, MODE_TEETH),
    (4096, MODE_L[4096], (1, 2), None) + GAUGES[0] + (MODE_RTOL_NT, MODE_TEETH_NT),
]


def mode_problem(N, L, kl, coef, d):
    """(U* in longdouble, F in fp64, lambda+ = the smallest non-zero eigenvalue of -(c*Laplace_h), longdouble)"""
    c = LD(1.0 if coef is None else coef)
    star = ex.mixed_mode(N, BC, *kl)
    lam = c * ex.mixed_mode_eigenvalue(N, L, BC, *kl)
    return star, ex.r64(lam * star) + float(d), -c * ex.mixed_mode_eigenvalue(N, L, BC, 0, 1)


def mode_coef(N, coef):
    return None if coef is None else np.full((N, N), coef)


# ---------------------------------------------------------------- edges of data and state, three operator-by-operator families
# N = 65 -> 32 -> 16 -> 8; each family with the coefficient "smooth" (a_min = 0.5), the restatement beside it
EDGE_N = 65
EDGE_MEAN = 2.5
FAMILIES = ("vc", "bc", "singular")
EDGE_KINDS = {"vc": "dddd", "bc": "ndnd", "singular": BC}
CAP_OPTS = dict(max_cycles=2, rtol=0.0, coarse_rtol=0.0, coarse_atol=1e-3, coarse_max_iters=3)
NAN_OPTS = dict(max_cycles=2, coarse_max_iters=5)
SCALE_OPTS = dict(max_cycles=2, rtol=0.0)


def edge_coef():
    return vref.field("smooth", EDGE_N)


def edge_kwargs(family, a, mean=EDGE_MEAN):
    """what mg.Solver takes for the family"""
    return {"vc": dict(coef=a), "bc": dict(coef=a, bc=EDGE_KINDS["bc"]), "singular": dict(coef=a, bc=BC, mean=mean)}[family]


def edge_restated(family, a, F, U0, mean=EDGE_MEAN, orc=None, rtable=None, ptable=None, **opts):
    """(U, history, cycles, converged, info, margins, capped) of the family's restatement; info: compat_defect, mean_before
    and Ft for "singular", empty otherwise.  orc: the oracle, whose transfers _solve_vc_ref uses."""
    margins, capped = [], []
    if family == "vc":
        out = vref.solve(orc, a, F, U0, 1.0, margins=margins, capped=capped, table=rtable, **opts) + ({},)
    elif family == "bc":
        out = bref.solve(a, F, U0, EDGE_KINDS["bc"], 1.0, margins=margins, capped=capped, rtable=rtable, ptable=ptable, **opts) + ({},)
    else:
        out = sref.solve(a, F, U0, mean, 1.0, margins=margins, capped=capped, rtable=rtable, ptable=ptable, **opts)
    return out + (margins, capped)


def nan_problem():
    F, U0 = ref.random_problem(EDGE_N, 88)
    F = F.copy()
    F[EDGE_N // 3, EDGE_N // 2] = np.nan
    return F, U0


def capped_problem():
    """unit magnitude: the coarse solve runs into CAP_OPTS' three iterations"""
    return ref.random_problem(EDGE_N, 89)


def small_problem():
    """the same kind of problem scaled by 2^-40: the absolute coarse target is met in the first iteration"""
    F, U0 = ref.random_problem(EDGE_N, 90)
    return F * 2.0 ** -40, U0 * 2.0 ** -40


def scale_problem():
    F, U0 = ref.random_problem(EDGE_N, 77)
    return F + 0.125, U0


# F = 0 with a = 2: 1 + x^2 - y^2 on x = c*h, y = r*h is even about column 0 and row 0 and the 5-point stencil annihilates it
# (second differences +2 and -2), so it solves the discrete Laplace problem exactly with the mirrored ghost points of the
# Neumann sides S and W of "ndnd", and with four Dirichlet sides.  atol = 1e-7: the residual's rounding floor is about
# 2^-53*inv*max|U|*N*3 = 2e-10 (inv = 4096), and the bound 2*atol/(2*lambda_min) is at most 2.1e-8 (lambda_min = 4.93 for
# "ndnd", 19.7 for "dddd"): teeth at 1e-6*max|U*| = 2e-6.
LAPLACE_ATOL = 1e-7
LAPLACE_COEF = 2.0


def laplace_problem(family):
    """(U* in longdouble, F = 0, U0 = the data points of U* and zero at the unknowns, c*lambda_min)"""
    N = EDGE_N
    bc = EDGE_KINDS[family]
    t = np.arange(N).astype(LD) / LD(N - 1)
    star = 1 + t[None, :] ** 2 - t[:, None] ** 2
    U0 = ex.r64(star)
    U0[bref.mask(N, bc)] = 0.0
    return star, np.zeros((N, N)), U0, LD(LAPLACE_COEF) * ex.lambda_min(N, 1.0, bc)


ZERO_F = dict(rtol=0.0, atol=1e-9, mean=-0.75, seed=91)


def zero_source_error_and_bound(a, U, mean, L=1.0):
    """F = 0 with four Neumann sides: the answer is the constant `mean`.  (max|U - mean|, its bound, a_min*lambda+): U - mean_w(U)
    is w-orthogonal to the constants and A maps it to r(U), -<x, A x>_w >= a_min * -<x, Laplace_h x>_w face by face, so
    max|U - mean| <= 2*||r(U)||_2 / (a_min*lambda+) + |mean_w(U) - mean|, r and the mean in longdouble."""
    N = U.shape[0]
    r = bref.residual_ld_stencil(a, U, np.zeros((N, N)), L, 0.0, BC)
    lam = LD(float(np.min(a))) * -ex.mixed_mode_eigenvalue(N, L, BC, 0, 1)
    bound = 2 * np.sqrt(np.sum(r ** 2)) / lam + abs(sref.weighted_mean_ld(U) - LD(mean))
    return np.max(np.abs(np.asarray(U, dtype=LD) - LD(mean))), bound, lam
