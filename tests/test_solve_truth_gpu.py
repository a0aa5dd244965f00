"""What a caller relies on, checked against references that share no code with the engine or the oracle
(tests/_solve_ref.py, np.longdouble): the U that comes back solves laplace(U) = F on a square of side L with the caller's
rim, to the residual the call reports.

  residual:  residual_norm_ld(U) <= max(rtol*||F||, atol) + residual_rounding_bound(U)
  answer:    ||U - U*||_2 <= (residual_norm_ld(U) + residual_norm_ld(U*_fp64)) / lambda_min   (e = A^-1 r)
  report:    |res - residual_norm_ld(U)| <= residual_rounding_bound(U), the same for res0 at the start,
             |ref_norm - ||F||| <= (N-2)^2 * 2^-53 * ||F||

U* is the direct solution of the discrete system on the start rim, or a polynomial the 5-point stencil solves exactly.
Then the edges of data and state: F = 0, a Laplace problem, magnitudes 2^+-300, a NaN in F, solvers reused after it."""
import functools

import numpy as np
import pytest

import _solve_ref as ref
from conftest import assert_bits

pytestmark = pytest.mark.gpu

LD = np.longdouble
DIRECT_CASES = [(65, 2.5, 4), (129, 0.3, 16), (100, 7.0, 3), (127, 1.0, 32), (257, 2.5, 8), (256, 1e-3, 8)]
CUBIC_CASES = [(1025, 2.5), (2048, 0.3), (4097, 7.0)]
ORIGIN = (0.25, -0.5)
MODES = [("solver", "stream"), ("solver", "simple"), ("batch", "stream"), ("batch", "simple")]


def power_of_two_hierarchy(N):
    return N & (N - 1) == 0 or (N - 1) & (N - 2) == 0


@functools.lru_cache(maxsize=None)
def direct_problem(N, L, guess):
    """Random F, random rim, random or zero interior guess, and the direct solution on that rim rounded to fp64.
    F is uniform in [-0.5, 0.5); so are rim and guess on squares of side L >= 1, and on smaller squares they shrink with
    L^2, the size of a solution for such an F.  A rim of magnitude u enters the residual as inv*u = u*(N-1)^2/L^2, which
    fp64 evaluates to about 2^-53*inv*u per point: at (N, L) = (256, 1e-3) a rim of unit magnitude puts a rounding
    floor of 1.6e-4 under the residual norm (the restatement stalls there), five orders above rtol*||F|| = 7e-9, and no
    fp64 solver can report convergence.  With u = L^2 the floor is 2^-53*(N-1)^2, below rtol*|F| at every size here."""
    F, U0 = ref.random_problem(N, 500 + N)
    U0 = U0 * min(1.0, L * L)
    if guess == "zero":
        U0 = ref.rim_only(U0)
    return F, U0, ref.direct_solution(F, U0, L).astype(np.float64)


@functools.lru_cache(maxsize=None)
def cubic_problem(N, L):
    F, star = ref.cubic_problem(N, L, ORIGIN[0], ORIGIN[1], ref.CUBIC)
    return F, ref.rim_only(star), star


def laplace_problem():
    N, L = 129, 2.5
    F, star = ref.cubic_problem(N, L, ORIGIN[0], ORIGIN[1], ref.HARMONIC)
    U0 = ref.rim_only(star)
    return N, L, F, U0, star, 1e-8 * float(ref.residual_norm_ld(U0, F, L))


def run(mg, how, smoother, F, U0, L, **opts):
    """One solve of (F, U0): a Solver, or instance 1 of a BatchSolver batch of 3 different problems."""
    N = F.shape[0]
    mg.set_smoother(smoother)
    try:
        if how == "solver":
            s = mg.Solver(N, L, **opts)
            try:
                return s.solve(F, U0)
            finally:
                s.close()
        others = [ref.random_problem(N, 900 + N + i) for i in range(2)]
        Fs = np.stack([others[0][0], F, others[1][0]])
        Us = np.stack([others[0][1], U0, others[1][1]])
        bs = mg.BatchSolver(N, L, max_batch=3, **opts)
        try:
            U, infos = bs.solve(Fs, Us)
        finally:
            bs.close()
        return U[1], infos[1]
    finally:
        mg.set_smoother("stream")


def check_truth(U, info, F, U0, star, L, rtol, atol, what):
    N = F.shape[0]
    assert info["converged"] and info["status"] == 0, f"{what}: not converged after {info['cycles']} cycles, {info['history'][-3:]}"
    normF = ref.norm_ld(F)
    r = ref.residual_norm_ld(U, F, L)
    slack = ref.residual_rounding_bound(U, F, L)
    tol = max(LD(rtol) * normF, LD(atol))
    star_r = ref.residual_norm_ld(star, F, L)
    err = ref.norm_ld(U.astype(LD) - star.astype(LD))
    err_bound = (r + star_r) / ref.lambda_min(N, L)
    r0 = ref.residual_norm_ld(U0, F, L)
    slack0 = ref.residual_rounding_bound(U0, F, L)
    print(f"{what}: {info['cycles']} cycles; residual {float(r):.4e} tol {float(tol):.4e} rounding bound {float(slack):.4e}; "
          f"error {float(err):.4e} bound {float(err_bound):.4e}; res {info['res']:.17g} res0 {info['res0']:.17g} (ld {float(r0):.17g}) "
          f"ref_norm {info['ref_norm']:.17g} (ld {float(normF):.17g})")
    assert r <= tol + slack, f"{what}: residual {float(r):.6e} above {float(tol):.6e} + {float(slack):.6e}"
    assert err <= err_bound, f"{what}: ||U - U*|| = {float(err):.6e} above (r + r*) / lambda_min = {float(err_bound):.6e}"
    assert abs(LD(info["res"]) - r) <= slack, f"{what}: res {info['res']!r} is not the residual of U, {float(r)!r}"
    assert abs(LD(info["res0"]) - r0) <= slack0, f"{what}: res0 {info['res0']!r} is not the residual of the start, {float(r0)!r}"
    assert abs(LD(info["ref_norm"]) - normF) <= LD((N - 2) * (N - 2)) * ref.U53 * normF, f"{what}: ref_norm {info['ref_norm']!r}"
    if power_of_two_hierarchy(N):
        for name, a, b in (("top", U[0], U0[0]), ("bottom", U[-1], U0[-1]), ("left", U[:, 0], U0[:, 0]), ("right", U[:, -1], U0[:, -1])):
            assert_bits(a, b, f"{what}: rim {name}")


@pytest.mark.parametrize("how,smoother", MODES)
@pytest.mark.parametrize("guess", ["random", "zero"])
@pytest.mark.parametrize("N,L,N_min", DIRECT_CASES)
def test_solution_against_the_direct_solve(mg, N, L, N_min, guess, how, smoother):
    F, U0, star = direct_problem(N, L, guess)
    U, info = run(mg, how, smoother, F, U0, L, N_min=N_min, rtol=1e-10, max_cycles=60)
    check_truth(U, info, F, U0, star, L, 1e-10, 0.0, f"N={N} L={L} N_min={N_min} {guess} guess, {how}/{smoother}")


@pytest.mark.parametrize("how,smoother", [("solver", "stream"), ("batch", "stream")])
@pytest.mark.parametrize("N,L", CUBIC_CASES)
def test_solution_against_a_cubic(mg, N, L, how, smoother):
    """The large-grid kernels (pairs, non-temporal, odd forms) against an analytic answer.  rtol = 1e-8: the rounding
    floor of the residual (include/mg_hip.h: 8e-10 at 8192^2, falling with N^2) stays an order below it."""
    F, U0, star = cubic_problem(N, L)
    U, info = run(mg, how, smoother, F, U0, L, rtol=1e-8, max_cycles=60)
    check_truth(U, info, F, U0, star, L, 1e-8, 0.0, f"cubic N={N} L={L}, {how}/{smoother}")


def test_zero_problem_runs_no_cycle(mg):
    N = 65
    Z = np.zeros((N, N))
    for how in ("solver", "batch"):
        Ud = mg.DeviceGrid.from_host(Z)
        Fd = mg.DeviceGrid.from_host(Z)
        if how == "solver":
            s = mg.Solver(N, 2.5)
            _, info = s.solve(Fd, Ud)
        else:
            s = mg.BatchSolver(N, 2.5, max_batch=1)
            info = s.solve_ptrs([Fd.ptr], [Ud.ptr])[0]
        s.close()
        assert info["cycles"] == 0 and info["converged"] and info["status"] == mg.MG_SOLVE_CONVERGED
        assert info["ref_norm"] == 0.0 and info["res0"] == 0.0 and info["res"] == 0.0 and info["history"] == [0.0]
        assert_bits(Ud.to_host(), Z, f"{how}: U untouched")


@pytest.mark.parametrize("how,smoother", MODES)
def test_laplace_problem(mg, how, smoother):
    """F = 0 (ref_norm = 0: only atol can stop it), rim and answer the harmonic 1 + x - 2y + xy + x^2 - y^2."""
    N, L, F, U0, star, atol = laplace_problem()
    U, info = run(mg, how, smoother, F, U0, L, rtol=1e-10, atol=atol, max_cycles=60)
    assert info["ref_norm"] == 0.0 and info["cycles"] > 0
    check_truth(U, info, F, U0, star, L, 1e-10, atol, f"Laplace N={N} L={L}, {how}/{smoother}")


@pytest.mark.parametrize("e", [300, -300])
def test_magnitudes_scale_exactly(mg, oracle, e):
    """F and U scaled by 2^e: powers of two scale every intermediate exactly and nothing over- or underflows (the
    largest square is about 2^630), so two cycles give the scaled U and the scaled history, bit for bit."""
    N = 129
    F, U0 = ref.random_problem(N, 77)
    margins, U = [], U0
    for _ in range(2):
        U = ref.cycle(oracle, F, U, 1.0, margins=margins)
    ref.assert_qualified(margins, "magnitudes N=129")
    opts = dict(rtol=0.0, max_cycles=2)
    base, bi = mg.solve(F, U0, **opts)
    assert_bits(base, U, "unscaled solve vs the restatement", zero_sign=True)
    scale = 2.0 ** e
    got, gi = mg.solve(F * scale, U0 * scale, **opts)
    assert np.all(np.isfinite(got)) and gi["cycles"] == 2 and not gi["coarse_capped"]
    assert_bits(got, base * scale, f"U of the problem scaled by 2^{e}")
    assert gi["history"] == [h * scale for h in bi["history"]] and gi["ref_norm"] == bi["ref_norm"] * scale
    assert all(0.0 < h < float("inf") for h in gi["history"])


def _nan_problem(N):
    F, U0 = ref.random_problem(N, 88)
    F = F.copy()
    F[N // 3, N // 2] = np.nan
    return F, U0


def test_nan_in_F_ends_after_max_cycles(mg):
    N = 129
    F, U0 = _nan_problem(N)
    _, info = mg.solve(F, U0, max_cycles=2, coarse_max_iters=5)
    assert info["status"] == mg.MG_SOLVE_NOT_CONVERGED and not info["converged"] and info["cycles"] == 2
    assert len(info["history"]) == 3 and all(np.isnan(h) for h in info["history"]) and np.isnan(info["ref_norm"])
    assert mg.lib().mg_last_error() == 0


@pytest.mark.parametrize("how", ["solver", "batch"])
def test_a_solver_is_clean_after_nan_and_capped_problems(mg, how):
    """One solver with an absolute coarse target of 1e-3 and 3 coarse iterations at most: a problem of unit magnitude
    runs into the cap, the same kind of problem scaled by 2^-40 meets the target in its first iteration.  After a NaN
    problem and a capped one, the small problem comes out as from a fresh solver."""
    N = 129
    Fn, Un = _nan_problem(N)
    Fc, Uc = ref.random_problem(N, 89)
    F, U0 = ref.random_problem(N, 90)
    F, U0 = F * 2.0 ** -40, U0 * 2.0 ** -40
    opts = dict(max_cycles=2, rtol=0.0, coarse_rtol=0.0, coarse_atol=1e-3, coarse_max_iters=3)
    make = (lambda: mg.Solver(N, 1.0, **opts)) if how == "solver" else (lambda: mg.BatchSolver(N, 1.0, max_batch=3, **opts))

    def solve(s, F, U):
        if how == "solver":
            return s.solve(F, U)
        Us, infos = s.solve(np.stack([F, F, F]), np.stack([U, U, U]))
        assert_bits(Us[0], Us[2], "equal instances of one batch")
        return Us[1], infos[1]

    fresh = make()
    want_U, want = solve(fresh, F, U0)
    fresh.close()
    assert want["cycles"] == 2 and not want["coarse_capped"] and want["history"][2] < want["history"][0]
    used = make()
    _, ni = solve(used, Fn, Un)
    assert ni["cycles"] == 2 and np.isnan(ni["history"][-1]) and not ni["converged"]
    _, ci = solve(used, Fc, Uc)
    assert ci["cycles"] == 2 and ci["coarse_capped"]
    got_U, got = solve(used, F, U0)
    used.close()
    assert_bits(got_U, want_U, f"{how}: clean solve after a NaN and a capped problem")
    assert got["history"] == want["history"] and got["cycles"] == 2 and not got["coarse_capped"]
    assert np.all(np.isfinite(got_U)) and mg.lib().mg_last_error() == 0
