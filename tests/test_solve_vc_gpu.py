"""The variable-coefficient solver (include/mg_varcoef.h) on the GPU: every kernel alone, bit for bit against the restatement
(tests/_solve_vc_ref.py) and inside guard bands; a == 1 against the constant-coefficient solver; whole solves against the
restatement, cycle by cycle; the returned U against a dense direct solve; lifecycle, refusals, and no collateral change.
Bit comparisons follow the qualification rule of DESIGN.md 4.3: the coarse margin of the restatement is asserted first."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _guard
import _solve_ref as ref
import _solve_shift_ref as sref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble


def lib_table(mg):
    return lambda N, M: mg.restriction_table(N, M)


def problem(N, seed, rim="random"):
    F, U0 = ref.random_problem(N, seed)
    if rim == "zero":
        U0[0, :] = U0[-1, :] = 0.0
        U0[:, 0] = U0[:, -1] = 0.0
    return F, U0


# ---------------------------------------------------------------- kernels alone, inside guard bands
def _kernel_ops(mg, N, L, shift, placement, ops):
    """every operation of `ops` on one guarded block [a, U, F, out, a_c]: bits against the restatement, inputs unchanged,
    nothing outside the output written"""
    M = max(N // 2, 2)
    a = vref.field("random", N, seed=N)
    F, U = ref.random_problem(N, 10 * N + 1)
    omega = 0.8
    with _guard.block(mg, [N, N, N, N, M], placement) as gb:
        ga, gU, gF, gout, gac = gb.views
        ga.upload(a), gU.upload(U), gF.upload(F)

        def run(what, call, want, out=gout):
            out.poison()
            gb.expect_readonly(ga, gU, gF)
            call()
            gb.check(f"{what} N={N} L={L} shift={shift} {placement}")
            assert_bits(out.to_host(), want, f"{what} N={N} L={L} shift={shift}")

        if "sweep" in ops:
            run("sweep", lambda: mg.sweepCoefficient(N, L, shift, omega, ga, gU, gF, gout),
                vref.weighted_sweeps(N, L, a, U, F, omega, 1, shift))
        if "sweep0" in ops:
            run("zero-start sweep", lambda: mg.sweepCoefficient(N, L, shift, omega, ga, None, gF, gout),
                vref.weighted_sweeps(N, L, a, None, F, omega, 1, shift, zero_start=True))
        for sign in (+1, -1):
            if "residual" in ops or ("residual-" in ops and sign < 0):
                run(f"residual sign {sign}", lambda: mg.residualCoefficient(N, L, shift, ga, gU, gF, gout, sign),
                    vref.residual(N, L, a, U, F, shift, sign))
        if "apply" in ops:
            run("applyOperator", lambda: mg.applyOperator(N, L, shift, ga, gU, gout), vref.apply_operator(N, L, a, U, shift))
            run("applyOperator a=None", lambda: mg.applyOperator(N, L, shift, None, gU, gout), vref.apply_operator(N, L, None, U, shift))
        if "coarsen" in ops and N >= 4:
            run("coarsenCoefficient", lambda: mg.coarsenCoefficient(N, ga, M, gac), vref.coarsen(a, M, mg.restriction_table(N, M)),
                out=gac)


ALL_OPS = ("sweep", "sweep0", "residual", "apply", "coarsen")


@pytest.mark.parametrize("shift", [0.0, 1e4])
@pytest.mark.parametrize("L", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("N", [3, 4, 7, 64, 100, 255, 257, 512, 514, 1026])
def test_kernels_alone_bit_for_bit_inside_guard_bands(mg, N, L, shift):
    """single-column form (odd or small N) and pair form (even N >= 512)"""
    _kernel_ops(mg, N, L, shift, "odd16" if N % 4 == 2 else "page", ALL_OPS)


def test_kernels_alone_non_temporal_form(mg):
    """N = 4096: one sweep and one residual through the non-temporal loads of F"""
    _kernel_ops(mg, 4096, 1.0, 1e4, "page", ("sweep", "residual-"))


# ---------------------------------------------------------------- a == 1 is the constant solver
@pytest.mark.parametrize("pp", [(1, 1), (3, 3), (4, 2)])
@pytest.mark.parametrize("shift", [0.0, 1e2])
@pytest.mark.parametrize("N", [64, 100, 257, 512])
def test_unit_coefficient_is_the_constant_solver(mg, oracle, N, shift, pp):
    F, U0 = problem(N, 2000 + N)
    one = mg.DeviceGrid.from_host(np.ones((N, N)))
    for omega in (0.8, 1.0):
        opts = dict(pre=pp[0], post=pp[1], omega=omega, shift=shift, rtol=1e-6, max_cycles=3)
        margins = []
        sref.solve(oracle, F, U0, 1.0, margins=margins, **opts)
        ref.assert_qualified(margins, f"N={N} shift={shift} {pp} omega={omega}")
        plain = mg.Solver(N, 1.0, **opts)
        want_U, want = plain.solve(F, U0)
        mg.set_smoother("simple")
        try:
            simple_U, simple = plain.solve(F, U0)
        finally:
            mg.set_smoother("stream")
        plain.close()
        s = mg.Solver(N, 1.0, coef=one, **opts)
        assert s.has_coefficient
        got_U, got = s.solve(F, U0)
        s.close()
        for other_U, other in ((want_U, want), (simple_U, simple)):
            assert_bits(got_U, other_U, f"U, N={N} shift={shift} {pp} omega={omega}")
            assert got["history"] == other["history"] and got["cycles"] == other["cycles"] == len(got["history"]) - 1
            for key in ("status", "converged", "coarse_capped", "res0", "res", "ref_norm"):
                assert got[key] == other[key], key
    one.free()


# ---------------------------------------------------------------- whole solves against the restatement
# The uncorrelated random field (contrast 1e3 from point to point) is there for the bits, not for the convergence: a sampled
# coefficient does not represent it on the coarse levels, and at most sizes the restatement runs all 50 cycles on it without
# meeting 1e-9 (every coarse solve of those cycles qualifies).  Its full solve is compared like the others: equal cycle count,
# equal status, bit-identical U -- 50 cycles of the numpy restatement at N = 512 take about a second.


def _against_restatement(mg, oracle, N, a, F, U0, what, max_cycles=50, **opts):
    """cycles 1..3 bit for bit (rtol = 0), then the full solve to rtol = 1e-9: equal cycle count and status, norms at 1e-12"""
    levels = vref.coarsen_levels(a, opts.get("N_min", 8), lib_table(mg))
    margins, U, hist, Us = [], np.array(U0, copy=True), [vref.residual_norm(N, 1.0, a, U0, F, opts.get("shift", 0.0))], []
    tol = 1e-9 * ref.ref_norm(F)
    while not (hist[-1] <= tol) and len(hist) <= max_cycles:
        U = vref.cycle(oracle, levels, F, U, 1.0, margins=margins, **opts)
        hist.append(vref.residual_norm(N, 1.0, a, U, F, opts.get("shift", 0.0)))
        if len(Us) < 3:
            Us.append(U)
    ref.assert_qualified(margins, what)
    ad = mg.DeviceGrid.from_host(a)
    for k, want in enumerate(Us, 1):
        s = mg.Solver(N, 1.0, coef=ad, rtol=0.0, max_cycles=k, **opts)
        got, info = s.solve(F, U0)
        s.close()
        assert_bits(got, want, f"{what}: U after cycle {k}")
        assert info["cycles"] == k and not info["converged"]
        np.testing.assert_allclose(info["history"], hist[:k + 1], rtol=1e-12, atol=0.0)
    s = mg.Solver(N, 1.0, coef=ad, rtol=1e-9, max_cycles=max_cycles, **opts)
    got, info = s.solve(F, U0)
    s.close()
    ad.free()
    assert info["converged"] == (hist[-1] <= tol) and info["cycles"] == len(hist) - 1, (info["cycles"], len(hist) - 1)
    assert_bits(got, U, f"{what}: U of the full solve")
    np.testing.assert_allclose(info["history"], hist, rtol=1e-12, atol=0.0)
    assert abs(info["ref_norm"] - ref.ref_norm(F)) <= 1e-12 * ref.ref_norm(F)
    return info


@pytest.mark.parametrize("rim", ["zero", "random"])
@pytest.mark.parametrize("name", ["one", "smooth", "exp", "random"])
@pytest.mark.parametrize("N", [64, 100, 256, 257, 512])
def test_whole_solves_bit_identical_to_restatement(mg, oracle, N, name, rim):
    F, U0 = problem(N, 3000 + N, rim)
    a = vref.field(name, N, seed=N)
    info = _against_restatement(mg, oracle, N, a, F, U0, f"N={N} a={name} rim={rim}")
    print(f"N={N} a={name} rim={rim}: {info['cycles']} cycles, converged {info['converged']}")
    assert info["converged"] or name == "random"   # (the random field: whatever the restatement says, asserted above)


@pytest.mark.parametrize("shift", [0.0, 1e4])
@pytest.mark.parametrize("Nc", [3, 5, 8, 31, 32])
def test_two_level_hierarchies(mg, oracle, Nc, shift):
    """N = 2 Nc and 2 Nc + 1 with N_min = Nc: the coarse solve at the lower end of its range and around the 1024 points of
    one point per thread (31^2 = 961, 32^2 = 1024); Nc = 63 (N_min is at most 32) follows below"""
    for N in (2 * Nc, 2 * Nc + 1):
        F, U0 = problem(N, 4000 + N)
        name = "exp" if shift else "random"
        _against_restatement(mg, oracle, N, vref.field(name, N, seed=N), F, U0, f"two levels N={N} Nc={Nc} shift={shift}",
                             N_min=Nc, shift=shift)


@pytest.mark.parametrize("N", [126, 127])
def test_two_level_hierarchy_coarsest_63(mg, oracle, N):
    """N_min = 32 and N = 126 / 127: the hierarchy is (N, 63), four points per thread in the coarse solve"""
    assert ref.sizes(N, 32) == [N, 63]
    F, U0 = problem(N, 4000 + N)
    _against_restatement(mg, oracle, N, vref.field("exp", N), F, U0, f"two levels N={N} Nc=63", N_min=32, shift=1e2)


# ---------------------------------------------------------------- truth: a dense direct solve, no code shared with the engine
@pytest.mark.parametrize("shift", [0.0, 1e3])
@pytest.mark.parametrize("name", ["smooth", "exp"])
@pytest.mark.parametrize("N", [33, 49])
def test_against_the_direct_solution(mg, N, name, shift):
    """||U - U*|| <= (r(U) + r(U*)) / (a_min*lambda_min(N, L) + sigma): the operator -div_h(a grad_h) + sigma is symmetric
    with smallest eigenvalue >= a_min*lambda_min(-Laplace_h) + sigma.  The longdouble residual of the returned U is within
    max(rtol*||F||, atol) plus the a-priori rounding bound; res, res0 and ref_norm are the norms of the caller's arrays."""
    L, rtol = 1.5, 1e-10
    F, U0 = problem(N, 5000 + N)
    a = vref.field(name, N, L)
    U, info = mg.solve(F, U0, L, coef=a, shift=shift, rtol=rtol)
    assert info["converged"]
    X = vref.direct_solution(a, F, U0, L, shift)
    rU, rX = vref.residual_norm_ld(a, U, F, L, shift), vref.residual_norm_ld(a, X, F, L, shift)
    err = ref.norm_ld(U.astype(LD) - X)
    bound = (rU + rX) / (LD(float(a.min())) * ref.lambda_min(N, L) + LD(shift))
    R = vref.residual_rounding_bound(a, U, F, L, shift)
    print(f"N={N} a={name} shift={shift}: {info['cycles']} cycles, |U-U*| {float(err):.3e} <= {float(bound):.3e}; "
          f"r(U) {float(rU):.3e}, r(U*) {float(rX):.3e}, rounding bound {float(R):.3e}")
    assert err <= bound
    assert rU <= max(rtol * ref.ref_norm(F), 0.0) + R
    assert abs(LD(info["res"]) - rU) <= R
    assert abs(LD(info["res0"]) - vref.residual_norm_ld(a, U0, F, L, shift)) <= vref.residual_rounding_bound(a, U0, F, L, shift)
    assert abs(LD(info["ref_norm"]) - ref.norm_ld(F)) <= 1e-14 * ref.norm_ld(F)
    if N == 33:   # (2^k + 1: the rim comes back bit-identical)
        assert_bits(U[0], U0[0], "rim row")


# ---------------------------------------------------------------- lifecycle
def test_replace_remove_and_reuse(mg, oracle):
    N = 100
    F, U0 = problem(N, 6000)
    a1, a2 = vref.field("smooth", N), vref.field("exp", N)
    opts = dict(rtol=0.0, max_cycles=2)
    plain = mg.Solver(N, 1.0, **opts)
    want_plain, info_plain = plain.solve(F, U0)
    s = mg.Solver(N, 1.0, **opts)
    assert not s.has_coefficient
    g = mg.DeviceGrid.from_host(a1)
    s.set_coefficient(g)
    g.free()                                   # the caller's array may be freed after the call
    junk = mg.DeviceGrid.from_host(np.full((N, N), -7.0))   # (likely the same block, recycled)
    got1, _ = s.solve(F, U0)
    junk.free()
    s.set_coefficient(a2)
    got2, info2 = s.solve(F, U0)
    for a, got in ((a1, got1), (a2, got2)):
        fresh = mg.Solver(N, 1.0, coef=a, **opts)
        want, info = fresh.solve(F, U0)
        fresh.close()
        assert_bits(got, want, "a replaced coefficient solves as a fresh solver's")
    assert info2["history"] == info["history"]
    levels = vref.coarsen_levels(a2, 8, lib_table(mg))
    want = vref.cycle(oracle, levels, F, vref.cycle(oracle, levels, F, U0))
    assert_bits(got2, want, "second coefficient against the restatement")
    # a refused coefficient leaves the one in place
    bad = a2.copy()
    bad[50, 50] = 0.0
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        s.set_coefficient(bad)
    assert s.has_coefficient
    again, _ = s.solve(F, U0)
    assert_bits(again, got2, "after a refused coefficient")
    # None: the constant solver again (the dispatch is on the flag alone: the launches are the ones of a solver without)
    s.set_coefficient(None)
    assert not s.has_coefficient
    back, info_back = s.solve(F, U0)
    assert_bits(back, want_plain, "set_coefficient(None) restores the constant solver")
    assert info_back["history"] == info_plain["history"]
    s.close()
    plain.close()


def test_torch_tensors_on_a_side_stream():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_solve_vc_torch_worker.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SOLVE_VC_TORCH OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("value", [0.0, -1.0, float("nan"), float("inf"), -float("inf")])
def test_bad_coefficient_values_are_refused(mg, value):
    N = 64
    F, U0 = problem(N, 7000)
    a = vref.field("smooth", N)
    a[N - 1, 3] = value                        # (a rim point: the rim is part of the coefficient)
    s = mg.Solver(N, 1.0, rtol=0.0, max_cycles=1)
    want, _ = s.solve(F, U0)
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        s.set_coefficient(a)
    assert not s.has_coefficient
    got, _ = s.solve(F, U0)
    assert_bits(got, want, "the solver is usable after the refusal, and unchanged")
    s.close()
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg.Solver(N, 1.0, coef=a)


def test_fmg_shape_and_null_are_refused(mg):
    N = 64
    F, U0 = problem(N, 7001)
    s = mg.Solver(N, 1.0, fmg=1, rtol=0.0, max_cycles=1)
    want, _ = s.solve(F, U0)
    with pytest.raises(mg.MGError, match=r"\[3\].*fmg"):
        s.set_coefficient(np.ones((N, N)))
    got, _ = s.solve(F, U0)
    assert_bits(got, want, "the fmg solver is usable after the refusal")
    s.close()
    s = mg.Solver(N, 1.0)
    for bad in (np.ones((N, N + 1)), np.ones((N - 1, N - 1)), mg.DeviceGrid(32)):
        with pytest.raises(mg.MGError, match="shape"):
            s.set_coefficient(bad)
    s.close()
    assert mg.lib().mg_solver_set_coefficient(None, None) == 2 and mg.lib().mg_solver_has_coefficient(None) == 0
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg._check()
    with pytest.raises(TypeError):
        mg.BatchSolver(N, 1.0, 2, coef=np.ones((N, N)))
    with pytest.raises(TypeError):
        mg.solve_batched(np.stack([F, F]), None, 1.0, coef=np.ones((N, N)))
    with pytest.raises(TypeError):
        mg.HeatStepper(N, 1.0, coef=np.ones((N, N)))


# ---------------------------------------------------------------- no collateral change
@pytest.mark.parametrize("N", [100, 256])
def test_constant_solvers_are_untouched_by_a_variable_solve(mg, N):
    F, U0 = problem(N, 8000 + N)
    opts = dict(rtol=0.0, max_cycles=2, shift=10.0)

    def constant():
        U, info = mg.solve(F, U0, **opts)
        b = mg.BatchSolver(N, 1.0, 2, **opts)
        Ub, infos = b.solve(np.stack([F, F]), np.stack([U0, ref.rim_only(U0)]))
        b.close()
        return U, info["history"], np.asarray(Ub), [i["history"] for i in infos]

    before = constant()
    mg.solve(F, U0, coef=vref.field("exp", N), **opts)
    after = constant()
    assert_bits(after[0], before[0], "Solver")
    assert_bits(after[2], before[2], "BatchSolver")
    assert after[1] == before[1] and after[3] == before[3]
