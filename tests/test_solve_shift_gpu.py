"""The `shift` option (Laplace(U) - sigma*U = F, include/mg_hip.h) of the residual-tolerance solver on the device: bit for
bit against the restatement written from the header (tests/_solve_shift_ref.py), shift = 0 against the option left alone,
the fused cycle against MG_SMOOTHER=simple, the truth of the answer in np.longdouble, refusals, the memory contract and
torch tensors.

Bit comparison means: U bit for bit, cycles, converged and coarse_capped equal, and the residual history to 1e-12
relative -- the norm's partial sums are added in the kernel's fixed order, which is no part of the semantics numpy could
restate (the same rule as test_solve_gpu.py).  Every case first qualifies its input (coarse margin >= 1e-10)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _guard
import _solve_ref as ref
import _solve_shift_ref as sref
from conftest import assert_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
SIZES = [16, 17, 100, 255, 256, 257, 1024, 1025]
SIGMAS = [2.0 ** -20, 1.0, 1e4, 1e8]
LENGTHS = [1e-3, 1.0, 1e3]
SWEEPS = [(1, 1), (2, 2), (3, 3), (2, 1)]
OMEGAS = [1.0, 0.8, 2.0 / 3.0]
KEYS = ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm", "history")


def problem(N, L, seed):
    """random_problem with U scaled like a solution of a unit F on a small square (test_solve_truth_gpu.direct_problem)."""
    F, U0 = ref.random_problem(N, seed)
    return F, U0 * min(1.0, L * L)


def against_restatement(mg, oracle, F, U0, L, cycles, what, **opts):
    margins, capped = [], []
    want, hist, k, conv = sref.solve(oracle, F, U0, L, margins=margins, capped=capped, rtol=0.0, atol=0.0, max_cycles=cycles, **opts)
    ref.assert_qualified(margins, what)
    U, info = mg.solve(F, U0, L, rtol=0.0, atol=0.0, max_cycles=cycles, **opts)
    assert_bits(U, want, what + " U", zero_sign=True)
    assert info["cycles"] == k == cycles and info["converged"] == bool(conv), what
    assert info["coarse_capped"] == any(capped), what
    np.testing.assert_allclose(info["history"], hist, rtol=1e-12, atol=0, err_msg=what)
    return info


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("N", SIZES)
def test_sizes_shifts_lengths_bit_identical_to_restatement(mg, oracle, N, sigma, L):
    F, U0 = problem(N, L, 2000 + N)
    against_restatement(mg, oracle, F, U0, L, 2, f"N={N} sigma={sigma:g} L={L:g}", shift=sigma)


SMALL_POINTS = [(17, 1e4, 1.0), (100, 1.0, 1.0), (256, 1e8, 1e3), (257, 2.0 ** -20, 1e-3)]
LARGE_OPTS = [((3, 3), 0.8), ((2, 1), 1.0), ((1, 1), 2.0 / 3.0), ((2, 2), 0.8), ((4, 4), 0.8), ((1, 2), 1.0)]


@pytest.mark.parametrize("N,sigma,L,pp,omega", [(N, s, L, pp, w) for N, s, L in SMALL_POINTS for pp in SWEEPS for w in OMEGAS] +
                         [(N, 1e4, 1.0, pp, w) for N in (1024, 1025) for pp, w in LARGE_OPTS])
def test_sweeps_and_weights_bit_identical_to_restatement(mg, oracle, N, sigma, L, pp, omega):
    F, U0 = problem(N, L, 3000 + N + 7 * pp[0])
    against_restatement(mg, oracle, F, U0, L, 2, f"N={N} sigma={sigma:g} L={L:g} V{pp} omega={omega:.4f}", shift=sigma, pre=pp[0],
                        post=pp[1], omega=omega)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("N,N_min", [(6, 3), (7, 3), (64, 32), (126, 32), (127, 32)])
def test_two_level_hierarchies(mg, oracle, N, N_min, sigma):
    """Coarsest sizes 3, 32 and 63: the coarse solve's shifted update and error metric carry the whole correction."""
    assert len(ref.sizes(N, N_min)) == 2 and ref.sizes(N, N_min)[1] in (3, 32, 63)
    F, U0 = problem(N, 1.0, 4000 + N)
    against_restatement(mg, oracle, F, U0, 1.0, 2, f"N={N} N_min={N_min} sigma={sigma:g}", shift=sigma, N_min=N_min)


@pytest.mark.parametrize("N", [100, 256, 257, 1024])
def test_history_and_stopping_rule_match_restatement(mg, oracle, N):
    F, U0 = problem(N, 1.0, 5)
    opts = dict(rtol=1e-10, shift=1e4)
    margins = []
    want, hist, k, conv = sref.solve(oracle, F, U0, margins=margins, **opts)
    ref.assert_qualified(margins, f"N={N}")
    U, info = mg.solve(F, U0, **opts)
    assert (info["cycles"], info["converged"]) == (k, True) and conv
    assert_bits(U, want, f"N={N} sigma=1e4 to rtol 1e-10", zero_sign=True)
    np.testing.assert_allclose(info["history"], hist, rtol=1e-12, atol=0)


@pytest.mark.parametrize("N", [100, 256, 257, 1024])
def test_explicit_zero_shift_is_the_option_left_alone(mg, N):
    """shift = 0.0 passed explicitly: the same bits and results as options without the field touched, from a Solver and
    from a BatchSolver, and the same number of launches."""
    F, U0 = ref.random_problem(N, 60 + N)
    opts = dict(rtol=1e-9, max_cycles=4)
    a, ia = mg.solve(F, U0, **opts)
    b, ib = mg.solve(F, U0, shift=0.0, **opts)
    assert_bits(a, b, f"N={N}: shift=0.0 vs default")
    for k in KEYS:
        assert ia[k] == ib[k], k
    Fs, Us = np.stack([F, F + 1.0]), np.stack([U0, U0])
    A, IA = mg.solve_batched(Fs, Us, **opts)
    B, IB = mg.solve_batched(Fs, Us, shift=0.0, **opts)
    assert_bits(A, B, f"N={N}: batched shift=0.0 vs default")
    assert IA[0]["stats"]["launches"] == IB[0]["stats"]["launches"] and IA[0]["stats"]["cycles"] == IB[0]["stats"]["cycles"]
    # ... and a shifted batch enqueues as many launches per cycle as the unshifted one: each kernel has one shifted twin
    _, IC = mg.solve_batched(Fs, Us, shift=1e4, rtol=0.0, max_cycles=IA[0]["stats"]["cycles"])
    _, ID = mg.solve_batched(Fs, Us, rtol=0.0, max_cycles=IA[0]["stats"]["cycles"])
    assert IC[0]["stats"]["launches"] == ID[0]["stats"]["launches"]


@pytest.mark.parametrize("N,pp,omega,sigma", [(256, (3, 3), 0.8, 1e4), (64, (2, 1), 1.0, 1.0),       # even nested
                                              (257, (1, 1), 0.8, 1e8), (129, (3, 3), 2.0 / 3.0, 1e4),  # odd
                                              (100, (3, 3), 0.8, 1e4), (1000, (2, 2), 0.8, 1.0),       # non-nested
                                              (1024, (4, 4), 0.8, 1e4), (2048, (2, 2), 1.0, 2.0 ** -20), (1025, (3, 3), 0.8, 1e4)])
def test_fused_path_equals_simple_smoother(mg, N, pp, omega, sigma):
    """The fused shifted nodes against MG_SMOOTHER=simple (k_wjacobi_sh / k_wjacobi_pairs_sh from N = 512, k_residual_sh)."""
    F, U0 = ref.random_problem(N, 50 + N)
    opts = dict(pre=pp[0], post=pp[1], omega=omega, rtol=0.0, max_cycles=2, shift=sigma)
    fused, fi = mg.solve(F, U0, **opts)
    mg.set_smoother("simple")
    try:
        simple, si = mg.solve(F, U0, **opts)
    finally:
        mg.set_smoother("stream")
    assert_bits(fused, simple, f"N={N} V{pp} omega={omega:.4f} sigma={sigma:g}: fused vs simple", zero_sign=True)
    assert fi["history"] == si["history"]


# ---------------------------------------------------------------- truth, in np.longdouble
def check_truth(U, info, F, star, L, sigma, rtol, atol, what):
    N = F.shape[0]
    assert info["converged"] and info["status"] == 0, f"{what}: not converged after {info['cycles']} cycles, {info['history'][-3:]}"
    r = sref.residual_norm_ld(U, F, L, sigma)
    slack = sref.residual_rounding_bound(U, F, L, sigma)
    tol = max(LD(rtol) * ref.norm_ld(F), LD(atol))
    star_r = sref.residual_norm_ld(star, F, L, sigma)
    err = ref.norm_ld(U.astype(LD) - star.astype(LD))
    err_bound = (r + star_r) / (ref.lambda_min(N, L) + LD(sigma))
    print(f"{what}: {info['cycles']} cycles; residual {float(r):.4e} tol {float(tol):.4e} rounding bound {float(slack):.4e}; "
          f"error {float(err):.4e} bound {float(err_bound):.4e}; res {info['res']:.17g}")
    assert r <= tol + slack, f"{what}: residual {float(r):.6e} above {float(tol):.6e} + {float(slack):.6e}"
    assert err <= err_bound, f"{what}: ||U - U*|| = {float(err):.6e} above (r + r*) / (lambda_min + sigma) = {float(err_bound):.6e}"
    assert abs(LD(info["res"]) - r) <= slack, f"{what}: res {info['res']!r} is not the residual of U, {float(r)!r}"


@pytest.mark.parametrize("N,L,sigma", [(65, 2.5, 1.0), (100, 7.0, 1e4), (256, 1e-3, 1e8), (257, 2.5, 1e4), (1024, 1.0, 1e4),
                                       (1025, 1.0, 1e8), (1025, 1.0, 2.0 ** -20)])
def test_solution_against_the_shifted_direct_solve(mg, N, L, sigma):
    F, U0 = problem(N, L, 500 + N)
    star = sref.direct_solution(F, U0, L, sigma).astype(np.float64)
    U, info = mg.solve(F, U0, L, rtol=1e-10, max_cycles=60, shift=sigma)
    check_truth(U, info, F, star, L, sigma, 1e-10, 0.0, f"N={N} L={L} sigma={sigma:g}")


def eigenmode(N):
    x = np.arange(N).astype(LD) / LD(N - 1)
    s = np.sin(ref._ld_pi() * x)
    s[0] = s[-1] = 0
    return np.outer(s, s)


@pytest.mark.parametrize("N,sigma", [(129, 1e2), (256, 1e4), (1025, 1e4)])
def test_backward_euler_step_damps_the_eigenmode(mg, N, sigma):
    """One backward-Euler step of u_t = Laplace(u) on sin(pi x) sin(pi y), L = 1, zero rim: (Laplace_h - sigma) u = -sigma
    u_old has the solution u_old * sigma / (sigma + lambda_11).  8 amplitudes through one BatchSolver."""
    mode = eigenmode(N)
    amps = [1.0, -2.5, 0.125, 3.0, 1e-3, 7.0, -0.5, 1e3]
    factor = LD(sigma) / (LD(sigma) + sref.lambda_11(N, 1.0))
    olds = [(LD(a) * mode).astype(np.float64) for a in amps]
    Fs = np.stack([-sigma * u for u in olds])
    bs = mg.BatchSolver(N, 1.0, max_batch=8, rtol=1e-10, max_cycles=60, shift=sigma)
    try:
        Us, infos = bs.solve(Fs, np.zeros_like(Fs))
    finally:
        bs.close()
    for a, u_old, F, U, info in zip(amps, olds, Fs, Us, infos):
        star = (factor * u_old.astype(LD)).astype(np.float64)
        check_truth(U, info, F, star, 1.0, sigma, 1e-10, 0.0, f"backward Euler N={N} sigma={sigma:g} amplitude {a:g}")


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -float("inf"), -2.0 ** -1074])
def test_bad_shift_is_refused_and_leaves_the_engine_usable(mg, bad):
    N = 64
    F, U0 = ref.random_problem(N, 8)
    opts = dict(rtol=0.0, max_cycles=2, shift=10.0)
    before, _ = mg.solve(F, U0, **opts)
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg.Solver(N, 1.0, shift=bad)
    after, _ = mg.solve(F, U0, **opts)
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg.BatchSolver(N, 1.0, max_batch=2, shift=bad)
    after_b, _ = mg.solve_batched(F[None], U0[None], **opts)
    assert_bits(after, before, "a solve after a refused Solver")
    assert_bits(after_b[0], before, "a batched solve after a refused BatchSolver")


def _worker(mode):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_solve_shift_worker.py"), mode], capture_output=True, text=True,
                         timeout=600)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("SOLVE_SHIFT ")]
    assert out.returncode == 0 and line, out.stdout[-1500:] + out.stderr[-3000:]
    return line[0]


def test_solve_after_refusals_gives_the_bits_of_a_fresh_process():
    """A process whose first calls are the six refused creations (-1, NaN, inf from both creators), each followed by a valid
    create and solve, against a process that only solves: the same digests of U and history from Solver and BatchSolver."""
    fresh, refused = _worker("fresh"), _worker("refused")
    assert fresh.split()[1] == "fresh" and refused.split()[1] == "refused"
    assert fresh.split()[2:] == refused.split()[2:], (fresh, refused)


def test_torch_tensors():
    assert _worker("torch") == "SOLVE_SHIFT torch OK"


# ---------------------------------------------------------------- memory contract
@pytest.mark.parametrize("place", list(_guard.PLACEMENTS))
@pytest.mark.parametrize("N", [256, 257])
def test_shifted_solves_inside_guard_bands(mg, oracle, N, place):
    """One shifted mg_solver_solve and one shifted mg_batch_solver_solve on arrays inside a caller's block: the bits of the
    restatement, F read only, every band intact."""
    sigma = 1e4
    probs = [ref.random_problem(N, 4100 + N + i) for i in range(2)]
    wants = []
    for F, U0 in probs:
        margins = []
        wants.append(sref.cycle(oracle, F, U0, 1.0, margins=margins, shift=sigma))
        ref.assert_qualified(margins, f"N={N}")
    opts = dict(rtol=0.0, atol=0.0, max_cycles=1, shift=sigma)
    b = _guard.block(mg, [N] * 4, place)
    s = mg.Solver(N, 1.0, **opts)
    bs = mg.BatchSolver(N, 1.0, max_batch=2, **opts)
    try:
        F0, U0v, F1, U1v = b.views
        for v, a in ((F0, probs[0][0]), (U0v, probs[0][1]), (F1, probs[1][0]), (U1v, probs[1][1])):
            v.upload(a)
        b.expect_readonly(F0, F1, U1v)
        info = s.solve_ptr(F0.ptr, U0v.ptr)
        assert info["cycles"] == 1 and not info["coarse_capped"]
        assert_bits(U0v.to_host(), wants[0], f"shifted Solver N={N} {place}", zero_sign=True)
        b.check(f"shifted mg_solver_solve N={N}")
        U0v.upload(probs[0][1])
        b.expect_readonly(F0, F1)
        infos = bs.solve_ptrs([F0.ptr, F1.ptr], [U0v.ptr, U1v.ptr])
        assert [i["cycles"] for i in infos] == [1, 1]
        assert_bits(U0v.to_host(), wants[0], f"shifted BatchSolver N={N} {place} instance 0", zero_sign=True)
        assert_bits(U1v.to_host(), wants[1], f"shifted BatchSolver N={N} {place} instance 1", zero_sign=True)
        b.check(f"shifted mg_batch_solver_solve N={N}")
    finally:
        s.close(); bs.close(); b.free()
