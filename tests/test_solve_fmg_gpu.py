"""The full-multigrid start (mg_solve_opts.fmg, include/mg_hip.h) on the device: the cubic prolongation kernel alone and
whole solves bit for bit against the restatement written from the header (tests/_solve_fmg_ref.py), the fused cycle against
MG_SMOOTHER=simple, the caller's interior ignored and the rim kept, refusals, fmg = 0 against the option left out, the
truth of the answer in np.longdouble, guard bands and torch tensors.

Bit comparison means: U bit for bit (the sign of a zero apart, as in test_solve_gpu.py), cycles, converged and
coarse_capped equal, and the residual history to 1e-12 relative.  Every case first qualifies its input: the coarse margin of
EVERY coarse solve of the pass and of the cycles is >= 1e-10; a failure there means another seed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _guard
import _solve_fmg_ref as fref
import _solve_ref as ref
import _solve_shift_ref as sref
from conftest import assert_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
SIZES = [16, 17, 100, 255, 256, 257, 1024, 1025]
SHIFTS = [0.0, 1e2, 1e6]
LENGTHS = [1e-3, 1.0, 1e3]
TRIPLES = [(3, 3, 0.8), (2, 1, 1.0), (1, 2, 2.0 / 3.0)]
KEYS = ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm", "history")
PAIRS = [(3, 6), (3, 7), (4, 8), (8, 16), (50, 100), (127, 255), (128, 256), (129, 257), (512, 1024), (513, 1025), (4096, 8192)]


# ---------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("N_src,N_dst", PAIRS)
def test_prolong_cubic_bit_identical_to_numpy(mg, N_src, N_dst):
    rng = np.random.default_rng(N_src)
    Uc = rng.random((N_src, N_src)) - 0.5
    marker = rng.random((N_dst, N_dst)) + 10.0
    c, f = mg.DeviceGrid.from_host(Uc), mg.DeviceGrid.from_host(marker)
    try:
        mg.prolongCubic(N_src, c, N_dst, f)
        got, src = f.to_host(), c.to_host()
    finally:
        c.free(); f.free()
    want = marker.copy()
    want[1:-1, 1:-1] = fref.prolong_cubic(Uc, N_dst)[1:-1, 1:-1]
    assert_bits(got, want, f"k_prolong_cubic {N_src} -> {N_dst} (rim untouched, interior)")
    assert_bits(src, Uc, "the source is read only")


@pytest.mark.parametrize("place", list(_guard.PLACEMENTS))
@pytest.mark.parametrize("N_src,N_dst", [(8, 16), (127, 255), (128, 256), (512, 1024), (1024, 2048)])
def test_prolong_cubic_inside_guard_bands(mg, N_src, N_dst, place):
    rng = np.random.default_rng(7)
    Uc = rng.random((N_src, N_src)) - 0.5
    b = _guard.block(mg, [N_src, N_dst], place)
    try:
        c, f = b.views
        c.upload(Uc)
        f.poison()
        b.expect_readonly(c)
        mg.prolongCubic(N_src, c, N_dst, f)
        got = f.to_host()
        b.check(f"mg_prolongCubic {N_src} -> {N_dst}")
    finally:
        b.free()
    assert_bits(got[1:-1, 1:-1], fref.prolong_cubic(Uc, N_dst)[1:-1, 1:-1], f"{N_src} -> {N_dst} {place}")
    rim = np.concatenate([got[0], got[-1], got[:, 0], got[:, -1]]).view(np.uint64)
    assert np.all(rim == _guard.PATTERN), "the rim of U_f was written"


# ---------------------------------------------------------------- whole solves
def problem(N, L, seed, zero_rim=False):
    F, U0 = ref.random_problem(N, seed)
    U0 = U0 * min(1.0, L * L)
    return F, (U0 - ref.rim_only(U0) if zero_rim else U0)


def against_restatement(mg, oracle, F, U0, L, cycles, what, **opts):
    margins, capped = [], []
    want, hist, k, conv = fref.solve(oracle, F, U0, L, margins=margins, capped=capped, rtol=0.0, atol=0.0, max_cycles=cycles, **opts)
    nl = len(ref.sizes(F.shape[0], opts.get("N_min", 8)))
    assert len(margins) == 1 + opts["fmg"] * (nl - 2) + cycles, (what, len(margins))   # every coarse solve of pass and cycles
    ref.assert_qualified(margins, what)
    U, info = mg.solve(F, U0, L, rtol=0.0, atol=0.0, max_cycles=cycles, **opts)
    assert_bits(U, want, what + " U", zero_sign=True)
    assert info["cycles"] == k == cycles and info["converged"] == bool(conv), what
    assert info["coarse_capped"] == any(capped), what
    np.testing.assert_allclose(info["history"], hist, rtol=1e-12, atol=0, err_msg=what)
    return U, info


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("fmg", [1, 2])
@pytest.mark.parametrize("N", SIZES)
def test_sizes_fmg_shifts_bit_identical_to_restatement(mg, oracle, N, fmg, shift):
    F, U0 = problem(N, 1.0, 7000 + N)
    against_restatement(mg, oracle, F, U0, 1.0, 2, f"N={N} fmg={fmg} shift={shift:g}", fmg=fmg, shift=shift)


@pytest.mark.parametrize("zero_rim", [False, True])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("N_min", [3, 8, 32])
@pytest.mark.parametrize("N", [100, 256, 257])
def test_lengths_coarsest_sizes_and_rims_bit_identical_to_restatement(mg, oracle, N, N_min, L, zero_rim):
    F, U0 = problem(N, L, 7100 + N + N_min, zero_rim)
    shift = 1e2 / (L * L) if N_min == 8 else 0.0
    against_restatement(mg, oracle, F, U0, L, 1, f"N={N} N_min={N_min} L={L:g} zero_rim={zero_rim}", fmg=1, N_min=N_min, shift=shift)


@pytest.mark.parametrize("pre,post,omega", TRIPLES)
@pytest.mark.parametrize("N,fmg,shift", [(17, 2, 0.0), (100, 1, 1e6), (255, 2, 1e2), (256, 1, 0.0), (257, 2, 1e6), (1024, 1, 1e2),
                                         (1025, 2, 0.0)])
def test_sweeps_and_weights_bit_identical_to_restatement(mg, oracle, N, fmg, shift, pre, post, omega):
    F, U0 = problem(N, 1.0, 7200 + N + 7 * pre)
    against_restatement(mg, oracle, F, U0, 1.0, 1, f"N={N} fmg={fmg} shift={shift:g} V({pre},{post}) omega={omega:.4f}", fmg=fmg,
                        shift=shift, pre=pre, post=post, omega=omega)


@pytest.mark.parametrize("N,N_min,fmg", [(6, 3, 1), (7, 3, 2), (64, 32, 1), (127, 32, 1)])
def test_two_level_hierarchies(mg, oracle, N, N_min, fmg):
    """The pass is the coarsest solve and one cubic prolongation (3 -> 6, 3 -> 7: the 3-point table)."""
    assert len(ref.sizes(N, N_min)) == 2
    F, U0 = problem(N, 1.0, 7300 + N)
    against_restatement(mg, oracle, F, U0, 1.0, 1, f"N={N} N_min={N_min}", fmg=fmg, N_min=N_min)


@pytest.mark.parametrize("N", [100, 256, 257, 1024])
def test_history_and_stopping_rule_match_restatement(mg, oracle, N):
    F, U0 = problem(N, 1.0, 5)
    margins = []
    want, hist, k, conv = fref.solve(oracle, F, U0, margins=margins, rtol=1e-9, fmg=1)
    ref.assert_qualified(margins, f"N={N}")
    _, _, k_cold, _ = fref.solve(oracle, F, U0, rtol=1e-9, fmg=0)
    U, info = mg.solve(F, U0, rtol=1e-9, fmg=1)
    cold, cinfo = mg.solve(F, U0, rtol=1e-9)
    print(f"N={N}: cycles to rtol 1e-9: FMG {info['cycles']}, cold {cinfo['cycles']}")
    assert (info["cycles"], info["converged"]) == (k, True) and conv and cinfo["cycles"] == k_cold
    assert info["cycles"] < cinfo["cycles"]
    assert_bits(U, want, f"N={N} fmg=1 to rtol 1e-9", zero_sign=True)
    np.testing.assert_allclose(info["history"], hist, rtol=1e-12, atol=0)
    assert info["history"][0] == cinfo["history"][0] == info["res0"]      # the norm of the caller's start


@pytest.mark.parametrize("N,fmg,shift,pp,omega", [(256, 1, 0.0, (3, 3), 0.8), (64, 2, 1e2, (2, 1), 1.0), (257, 1, 1e6, (1, 1), 0.8),
                                                  (100, 2, 0.0, (3, 3), 0.8), (1000, 1, 1e2, (2, 2), 0.8), (1024, 2, 0.0, (3, 3), 0.8),
                                                  (2048, 1, 1e2, (2, 2), 1.0), (1025, 1, 0.0, (3, 3), 0.8)])
def test_fused_path_equals_simple_smoother(mg, N, fmg, shift, pp, omega):
    F, U0 = ref.random_problem(N, 50 + N)
    opts = dict(pre=pp[0], post=pp[1], omega=omega, rtol=0.0, max_cycles=2, shift=shift, fmg=fmg)
    fused, fi = mg.solve(F, U0, **opts)
    mg.set_smoother("simple")
    try:
        simple, si = mg.solve(F, U0, **opts)
    finally:
        mg.set_smoother("stream")
    assert_bits(fused, simple, f"N={N} fmg={fmg} V{pp} shift={shift:g}: fused vs simple", zero_sign=True)
    assert fi["history"] == si["history"] and fi["coarse_capped"] == si["coarse_capped"]


@pytest.mark.parametrize("N", [100, 256, 1025])
def test_interior_is_ignored_rim_comes_back_and_a_converged_start_is_left_alone(mg, oracle, N):
    F, U0 = problem(N, 1.0, 7400 + N)
    other = U0.copy()
    other[1:-1, 1:-1] = np.random.default_rng(1).random((N - 2, N - 2)) * 100.0
    a, ia = mg.solve(F, U0, fmg=1, rtol=0.0, max_cycles=0)        # the pass alone
    b, ib = mg.solve(F, other, fmg=1, rtol=0.0, max_cycles=0)
    assert_bits(a, b, f"N={N}: two interiors, one FMG guess")
    assert ia["cycles"] == 0 and len(ia["history"]) == 1 and ia["history"] != ib["history"] and not ia["converged"]
    assert_bits(a, fref.fmg_guess(oracle, F, U0, fmg=1), f"N={N}: the guess of the restatement", zero_sign=True)
    for sl in ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1)):
        assert_bits(a[sl], U0[sl], f"N={N}: rim after the pass")
    c, ic = mg.solve(F, U0, fmg=1, rtol=0.0, max_cycles=2)
    d, idd = mg.solve(F, other, fmg=1, rtol=0.0, max_cycles=2)
    assert_bits(c, d, f"N={N}: two interiors, one result")
    assert ic["history"][1:] == idd["history"][1:]
    e, ie = mg.solve(F, U0, fmg=2, atol=1e30)                      # a start that meets the tolerance
    assert_bits(e, U0, f"N={N}: converged start untouched")
    assert ie["cycles"] == 0 and ie["converged"]


@pytest.mark.parametrize("N", [100, 256, 257, 1024])
def test_explicit_zero_fmg_is_the_option_left_out(mg, N):
    F, U0 = ref.random_problem(N, 60 + N)
    for extra in (dict(), dict(shift=1e2)):
        opts = dict(rtol=1e-9, max_cycles=4, **extra)
        a, ia = mg.solve(F, U0, **opts)
        b, ib = mg.solve(F, U0, fmg=0, **opts)
        assert_bits(a, b, f"N={N}: fmg=0 vs default")
        for k in KEYS:
            assert ia[k] == ib[k], k


@pytest.mark.parametrize("bad", [-1, 9, -2 ** 31, 2 ** 31 - 1])
def test_bad_fmg_is_refused_and_leaves_the_engine_usable(mg, bad):
    N = 64
    F, U0 = ref.random_problem(N, 8)
    opts = dict(rtol=0.0, max_cycles=2, fmg=1)
    before, _ = mg.solve(F, U0, **opts)
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg.Solver(N, 1.0, fmg=bad)
    after, _ = mg.solve(F, U0, **opts)
    assert_bits(after, before, "a solve after a refused Solver")
    s = mg.Solver(N, 1.0, fmg=8)      # the largest accepted value
    s.close()


def test_coarse_cap_in_the_pass_is_reported(mg, oracle):
    """coarse_max_iters = 1: every coarse solve of the pass and of the cycle stops at its cap."""
    N = 64
    F, U0 = problem(N, 1.0, 99)
    opts = dict(fmg=1, coarse_max_iters=1, coarse_rtol=1e-8)
    _, info = against_restatement(mg, oracle, F, U0, 1.0, 1, "capped", **opts)
    assert info["coarse_capped"]
    _, pass_only = mg.solve(F, U0, rtol=0.0, max_cycles=0, **opts)
    assert pass_only["coarse_capped"], "a cap inside the pass alone"


# ---------------------------------------------------------------- truth, in np.longdouble
@pytest.mark.parametrize("N,L,shift", [(65, 2.5, 0.0), (100, 7.0, 1e2), (257, 2.5, 0.0), (1024, 1.0, 1e2), (1025, 1.0, 0.0),
                                       (2049, 1.0, 0.0), (4097, 1.0, 0.0)])
def test_solution_is_true_to_tolerance(mg, N, L, shift):
    """The returned residual is the residual of the returned U (within the a-priori rounding bound of its fp64 evaluation)
    and meets the tolerance; up to N = 1025 also the distance to the direct solution."""
    F, U0 = problem(N, L, 500 + N)
    rtol = 1e-9
    U, info = mg.solve(F, U0, L, rtol=rtol, max_cycles=60, shift=shift, fmg=1)
    what = f"N={N} L={L} shift={shift:g}"
    assert info["converged"] and info["status"] == 0, f"{what}: not converged after {info['cycles']} cycles"
    r = sref.residual_norm_ld(U, F, L, shift)
    slack = sref.residual_rounding_bound(U, F, L, shift)
    tol = LD(rtol) * ref.norm_ld(F)
    print(f"{what}: {info['cycles']} cycles; residual {float(r):.4e} tol {float(tol):.4e} rounding bound {float(slack):.4e}")
    assert r <= tol + slack, f"{what}: residual {float(r):.6e} above {float(tol):.6e} + {float(slack):.6e}"
    assert abs(LD(info["res"]) - r) <= slack, f"{what}: res {info['res']!r} is not the residual of U, {float(r)!r}"
    for sl in ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1)):
        np.testing.assert_allclose(U[sl], U0[sl], rtol=0, atol=1e-12 * min(1.0, L * L), err_msg=what + " rim")
    if N <= 1025:
        star = sref.direct_solution(F, U0, L, shift)
        err = ref.norm_ld(U.astype(LD) - star)
        bound = (r + sref.residual_norm_ld(star.astype(np.float64), F, L, shift)) / (ref.lambda_min(N, L) + LD(shift))
        assert err <= bound, f"{what}: ||U - U*|| = {float(err):.6e} above {float(bound):.6e}"


def test_torch_tensors():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_solve_fmg_torch_worker.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SOLVE_FMG_TORCH OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


# ---------------------------------------------------------------- memory contract
@pytest.mark.parametrize("place", list(_guard.PLACEMENTS))
@pytest.mark.parametrize("N,shift", [(256, 0.0), (257, 1e2), (1024, 0.0)])
def test_fmg_solves_inside_guard_bands(mg, oracle, N, shift, place):
    """mg_solver_solve with fmg = 1 on arrays inside a caller's block: the bits of the restatement, F read only, every band
    intact (the pass reads F and the rim of U and writes the interior of U; everything else it touches is the solver's own)."""
    F, U0 = problem(N, 1.0, 4100 + N)
    margins = []
    want = fref.solve(oracle, F, U0, rtol=0.0, max_cycles=1, fmg=1, shift=shift, margins=margins)[0]
    ref.assert_qualified(margins, f"N={N}")
    b = _guard.block(mg, [N, N], place)
    s = mg.Solver(N, 1.0, rtol=0.0, atol=0.0, max_cycles=1, fmg=1, shift=shift)
    try:
        Fv, Uv = b.views
        Fv.upload(F)
        Uv.upload(U0)
        b.expect_readonly(Fv)
        info = s.solve_ptr(Fv.ptr, Uv.ptr)
        assert info["cycles"] == 1
        assert_bits(Uv.to_host(), want, f"fmg Solver N={N} {place}", zero_sign=True)
        b.check(f"mg_solver_solve fmg=1 N={N}")
    finally:
        s.close(); b.free()
