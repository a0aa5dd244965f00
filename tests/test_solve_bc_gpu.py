"""Boundary kinds per side (include/mg_bc.h) on the GPU: every kernel alone, bit for bit against the restatement
(tests/_bc_ref.py) and inside guard bands; four Dirichlet sides against the variable-coefficient hooks; whole solves against
the restatement, cycle by cycle; the returned U against a dense direct solve; conservation through the heat stepper;
refusals, lifecycle, and no collateral change.  Bit comparisons follow the qualification rule of DESIGN.md 4.3: the coarse
margin of the restatement is asserted first."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _bc_ref as bref
import _guard
import _heat_ref as href
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
FOUR = ("nnnn", "ddnd", "ndnd", "dndn")


def rtable(mg):
    return lambda N, M: mg.restriction_table(N, M)


def ptable(mg):
    return lambda M, N: mg.boundary_prolongation_table(M, N)


# ---------------------------------------------------------------- kernels alone, inside guard bands
def _kernel_ops(mg, N, L, shift, placement, kinds, ops):
    """every operation of `ops` for every kind of `kinds` on one guarded block [a, U, F, out, coarse, g]: bits against the
    restatement, inputs unchanged, nothing outside the output written"""
    M = max(N // 2, 2)
    a = vref.field("random", N, seed=N)
    F, U = ref.random_problem(N, 10 * N + 1)
    rng = np.random.default_rng(N)
    g, Uc = rng.random((4, N)) - 0.5, rng.random((M, M)) - 0.5
    omega, nu, dt = 0.8, 0.7, 1e-3
    with _guard.block(mg, [N, N, N, N, M, (4, N)], placement) as gb:
        ga, gU, gF, gout, gc, gg = gb.views
        ga.upload(a), gU.upload(U), gF.upload(F), gg.upload(g)

        def run(what, call, want, out=gout, readonly=None):
            out.poison()
            gb.expect_readonly(*(readonly or (ga, gU, gF, gg)))
            call()
            gb.check(f"{what} N={N} L={L} shift={shift} {placement}")
            assert_bits(out.to_host(), want, f"{what} N={N} L={L} shift={shift}")

        for bc in kinds:
            if "sweep" in ops:
                run(f"sweep {bc}", lambda: mg.sweepBoundary(N, L, shift, omega, bc, ga, gU, gF, gout),
                    bref.weighted_sweeps(N, L, bc, a, U, F, omega, 1, shift))
            if "sweep0" in ops:
                run(f"zero-start sweep {bc}", lambda: mg.sweepBoundary(N, L, shift, omega, bc, ga, None, gF, gout),
                    bref.weighted_sweeps(N, L, bc, a, None, F, omega, 1, shift, zero_start=True))
                run(f"sweep a=None {bc}", lambda: mg.sweepBoundary(N, L, shift, omega, bc, None, gU, gF, gout),
                    bref.weighted_sweeps(N, L, bc, None, U, F, omega, 1, shift))
            for sign in (+1, -1):
                if "residual" in ops or ("residual-" in ops and sign < 0):
                    run(f"residual {bc} sign {sign}", lambda: mg.residualBoundary(N, L, shift, bc, ga, gU, gF, gout, sign),
                        bref.residual(N, L, bc, a, U, F, shift, sign))
            if "apply" in ops:
                run(f"apply {bc}", lambda: mg.applyOperatorBoundary(N, L, shift, bc, ga, gU, gout), bref.apply_operator(N, L, bc, a, U, shift))
                run(f"apply a=None {bc}", lambda: mg.applyOperatorBoundary(N, L, shift, bc, None, gU, gout),
                    bref.apply_operator(N, L, bc, None, U, shift))
            if "transfer" in ops and N >= 4:
                run(f"restriction {bc}", lambda: mg.restrictBoundary(N, bc, gU, M, gc), bref.restrict(U, M, bc, mg.restriction_table(N, M)),
                    out=gc)
                gc.upload(Uc)
                run(f"prolongation-add {bc}", lambda: mg.prolongAddBoundary(M, bc, gc, N, gU, gout),
                    bref.prolong_add(Uc, N, U, bc, mg.boundary_prolongation_table(M, N)), readonly=(ga, gU, gF, gg, gc))
            if "source" in ops:
                run(f"neumann_source {bc}", lambda: mg.neumann_source(N, L, bc, gF, gg, coef=ga, out=gout), bref.neumann_source(N, L, bc, a, F, g))
                run(f"neumann_source a=None {bc}", lambda: mg.neumann_source(N, L, bc, gF, gg, out=gout), bref.neumann_source(N, L, bc, None, F, g))
            if "heat" in ops:
                for theta, coef, Q in ((0.5, ga, gF), (0.5, None, None), (1.0, ga, gF), (1.0, ga, None)):
                    run(f"heat rhs {bc} theta={theta} a={coef is not None} q={Q is not None}",
                        lambda: mg.heat_rhs_boundary(N, L, nu, dt, theta, bc, coef, gU, Q, gout),
                        bref.heat_rhs(N, L, nu, dt, theta, bc, a if coef is not None else None, U, F if Q is not None else None))


ALL_OPS = ("sweep", "sweep0", "residual", "apply", "transfer", "source", "heat")


@pytest.mark.parametrize("shift", [0.0, 1e4])
@pytest.mark.parametrize("L", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("N", [3, 4, 7, 64, 257])
def test_kernels_alone_every_kind(mg, N, L, shift):
    """all 16 kind combinations, one column per lane"""
    _kernel_ops(mg, N, L, shift, "odd16" if N % 4 == 0 else "page", bref.ALL_KINDS, ALL_OPS)


@pytest.mark.parametrize("shift", [0.0, 1e4])
@pytest.mark.parametrize("L", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("N", [100, 255, 512, 514, 1026])
def test_kernels_alone_single_column_and_pair_forms(mg, N, L, shift):
    """single-column form (odd or small N) and pair form (even N >= 512)"""
    _kernel_ops(mg, N, L, shift, "odd16" if N % 4 == 2 else "page", FOUR, ALL_OPS)


def test_kernels_alone_non_temporal_form(mg):
    """N = 4096: one sweep and one negative residual through the non-temporal form, four Neumann sides"""
    _kernel_ops(mg, 4096, 1.0, 1e4, "page", ("nnnn",), ("sweep", "residual-"))


@pytest.mark.parametrize("N", [7, 100, 512, 1026])
def test_four_dirichlet_sides_through_the_hooks(mg, N):
    """sweepBoundary / residualBoundary with "dddd" equal sweepCoefficient / residualCoefficient bit for bit"""
    a = vref.field("exp", N)
    F, U = ref.random_problem(N, 11 * N)
    ga, gU, gF = (mg.DeviceGrid.from_host(x) for x in (a, U, F))
    o1, o2 = mg.DeviceGrid((N, N)), mg.DeviceGrid((N, N))
    for shift in (0.0, 1e2):
        for U_in in (gU, None):
            mg.sweepBoundary(N, 1.0, shift, 0.8, "dddd", ga, U_in, gF, o1)
            mg.sweepCoefficient(N, 1.0, shift, 0.8, ga, U_in, gF, o2)
            assert_bits(o1.to_host(), o2.to_host(), f"sweep N={N}")
        for sign in (1, -1):
            mg.residualBoundary(N, 1.0, shift, "dddd", ga, gU, gF, o1, sign)
            mg.residualCoefficient(N, 1.0, shift, ga, gU, gF, o2, sign)
            assert_bits(o1.to_host(), o2.to_host(), f"residual N={N}")
        mg.applyOperatorBoundary(N, 1.0, shift, "dddd", None, gU, o1)
        mg.applyOperator(N, 1.0, shift, None, gU, o2)
        assert_bits(o1.to_host(), o2.to_host(), f"operator N={N}")
    for x in (ga, gU, gF, o1, o2):
        x.free()


# ---------------------------------------------------------------- taking the boundary away
@pytest.mark.parametrize("coef", [False, True])
@pytest.mark.parametrize("N", [100, 256])
def test_four_dirichlet_sides_restore_the_plain_solver(mg, N, coef):
    F, U0 = ref.random_problem(N, 2100 + N)
    a = vref.field("exp", N) if coef else None
    opts = dict(rtol=0.0, max_cycles=2, shift=5.0)
    plain = mg.Solver(N, 1.0, coef=a, **opts)
    want, info = plain.solve(F, U0)
    plain.close()
    s = mg.Solver(N, 1.0, coef=a, bc="ndnn", **opts)
    assert s.boundary == (1, 0, 1, 1)
    other, _ = s.solve(F, U0)
    assert not np.array_equal(other, want)
    for off in ("dddd", None, (0, 0, 0, 0)):
        s.set_boundary("nnnn")
        s.set_boundary(off)
        assert s.boundary == (0, 0, 0, 0)
        got, info2 = s.solve(F, U0)
        assert_bits(got, want, f"set_boundary({off!r}) restores the plain solver")
        assert info2["history"] == info["history"]
    s.close()


# ---------------------------------------------------------------- whole solves against the restatement
@pytest.mark.parametrize("pp", [(3, 3), (1, 2)])
@pytest.mark.parametrize("name", [None, "exp"])
@pytest.mark.parametrize("bc,shift", [("nnnn", 1e2), ("ndnd", 0.0), ("nnnd", 10.0)])
@pytest.mark.parametrize("N", [64, 65, 100, 257])
def test_whole_solves_bit_identical_to_restatement(mg, N, bc, shift, name, pp):
    """every coarse solve qualified, then U (rim included) after cycles 1 and 3 bit for bit; the history to 1e-12 (the
    restatement sums the norm in numpy's order, the kernel in its block partition)"""
    F, U0 = ref.random_problem(N, 3000 + N)
    a = vref.field(name, N) if name else None
    opts = dict(pre=pp[0], post=pp[1], shift=shift)
    levels = vref.coarsen_levels(a, 8, rtable(mg)) if name else None
    margins, Us, U = [], [], U0
    hist = [bref.residual_norm(N, 1.0, bc, a, U0, F, shift)]
    for _ in range(3):
        U = bref.cycle(levels, F, U, bc, 1.0, margins=margins, rtable=rtable(mg), ptable=ptable(mg), **opts)
        Us.append(U)
        hist.append(bref.residual_norm(N, 1.0, bc, a, U, F, shift))
    ref.assert_qualified(margins, f"N={N} {bc} a={name} {pp}")
    m = bref.mask(N, bc)
    for k in (1, 3):
        s = mg.Solver(N, 1.0, coef=a, bc=bc, rtol=0.0, max_cycles=k, **opts)
        got, info = s.solve(F, U0)
        s.close()
        assert_bits(got, Us[k - 1], f"N={N} {bc} a={name} {pp}: U after cycle {k}")
        assert_bits(got[~m], U0[~m], "data points")
        assert info["cycles"] == k and not info["converged"]
        np.testing.assert_allclose(info["history"], hist[:k + 1], rtol=1e-12, atol=0.0)
        assert abs(info["ref_norm"] - bref.ref_norm(F, bc)) <= 1e-12 * bref.ref_norm(F, bc)


# ---------------------------------------------------------------- truth: a dense direct solve, no code shared with the engine
@pytest.mark.parametrize("bc", bref.ALL_KINDS)
@pytest.mark.parametrize("N", [17, 24, 33])
def test_against_the_direct_solution(mg, N, bc):
    """max|U - X| <= ||A^-1||_inf * (||r(U)||_inf + ||r(X)||_inf): r the longdouble residual of the returned U / of the dense
    solution X (its own refinement error), ||A^-1||_inf from the dense inverse on the host.  The reported res equals the
    longdouble residual norm within the a-priori rounding bound extended to the rim unknowns."""
    L, rtol = 1.5, 1e-10
    F, U0 = ref.random_problem(N, 5000 + N)
    a = vref.field("exp", N, L)
    for shift in ((1e2,) if bc == "nnnn" else (0.0, 1e2)):
        if bc == "dddd":
            U, info = mg.solve(F, U0, L, coef=a, shift=shift, rtol=rtol)
        else:
            U, info = mg.solve(F, U0, L, coef=a, bc=bc, shift=shift, rtol=rtol)
        assert info["converged"], (bc, shift, info["cycles"])
        X, ninv = bref.direct_solution(a, F, U0, L, shift, bc, want_inverse_norm=True)
        rU, rX = bref.residual_ld(a, U, F, L, shift, bc), bref.residual_ld(a, X, F, L, shift, bc)
        err = np.max(np.abs(U.astype(LD) - X))
        bound = ninv * (np.max(np.abs(rU)) + np.max(np.abs(rX))) * (1 + LD(1e-6))   # (the fp64 inverse's own rounding)
        R = bref.residual_rounding_bound(a, U, F, L, shift, bc)
        res_ld = np.sqrt(np.sum(rU ** 2))
        print(f"N={N} {bc} shift={shift}: {info['cycles']} cycles, |U-X| {float(err):.3e} <= {float(bound):.3e}, "
              f"res {info['res']:.3e} vs {float(res_ld):.3e} (bound {float(R):.3e})")
        assert err <= bound
        assert abs(LD(info["res"]) - res_ld) <= R
        assert res_ld <= rtol * bref.ref_norm(F, bc) + R
        m = bref.mask(N, bc)
        assert_bits(U[~m], U0[~m], "data points come back bit-identical")


# ---------------------------------------------------------------- flux data, end to end on the device
def test_flux_data_end_to_end(mg):
    """neumann_source on numpy arrays is the restatement bit for bit, and the device solve of the closed-form problem of
    tests/test_solve_bc_cpu.py is second order: max-error ratio 33 -> 65 -> 129 inside [3.8, 4.2]"""
    from test_solve_bc_cpu import _exact_problem
    bc, shift, errs = "nnnd", 3.0, []
    for N in (33, 65, 129):
        u, a, F, g = _exact_problem(N, bc, shift)
        Fe = mg.neumann_source(N, 1.0, bc, F, g, coef=a)
        assert_bits(Fe, bref.neumann_source(N, 1.0, bc, a, F, g), "neumann_source on numpy arrays")
        assert_bits(mg.neumann_source(N, 1.0, "dddd", F, g, coef=a), F, "four Dirichlet sides: a copy")
        U0 = np.where(bref.mask(N, bc), 0.0, u)
        U, info = mg.solve(Fe, U0, 1.0, coef=a, bc=bc, shift=shift, rtol=1e-11)
        assert info["converged"]
        errs.append(float(np.max(np.abs(U - u))))
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print(f"flux data on the device: errors {errs}, ratios {ratios}")
    assert all(3.8 <= r <= 4.2 for r in ratios), ratios


# ---------------------------------------------------------------- conservation, through the heat stepper
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_insulated_walls_conserve_heat(mg, theta):
    """Four insulated walls, no source: sum w*u (trapezoid weights) is conserved by the scheme, because the column sums of
    diag(w)*A vanish (tests/test_solve_bc_cpu.py).  A step solves (A - sigma)u+ = F + r with F = -sigma*u - beta*A u, so
    sigma*(sum w*u+ - sum w*u) = -sum w*r and the change is at most ||w||_2*||r||_2/sigma.  ||r||_2 is the reported res plus
    what fp64 adds: the rounding of the residual's evaluation (R), of the right-hand side (eps), and of the weighted sum
    itself (n*2^-53*sum|w*u| for any order).  k steps are bit-identical to the caller's own loop."""
    N, L, nu, dt, bc = 65, 1.0, 1.0, 1e-3, "nnnn"
    a = vref.field("exp", N, L)
    _, U0 = ref.random_problem(N, 42)
    U0 = U0 + 1.0
    w = bref.trapezoid_weights(N, bc)
    wsum = lambda U: np.sum(w * np.asarray(U, dtype=LD))
    st = mg.HeatStepper(N, L, nu=nu, dt=dt, theta=theta)
    st.set_coefficient(a)
    st.set_boundary(bc)
    assert st.boundary == (1, 1, 1, 1)
    sigma = st.sigma
    assert sigma == href.consts(N, L, nu, dt, theta)[0]
    solver = mg.Solver(N, L, coef=a, bc=bc, shift=sigma)
    ga = mg.DeviceGrid.from_host(a)
    U, mine = U0, U0
    for step in range(3):
        prev = U
        U, infos = st.step(U, steps=1)
        assert infos[0]["converged"]
        # the caller's loop
        gU = mg.DeviceGrid.from_host(mine)
        gF = mg.heat_rhs_boundary(N, L, nu, dt, theta, bc, ga, gU)
        F = gF.to_host()
        assert_bits(F, bref.heat_rhs(N, L, nu, dt, theta, bc, a, mine), "right-hand side")
        mine, info = solver.solve(F, mine)
        gU.free(), gF.free()
        assert_bits(U, mine, f"step {step + 1} against the caller's loop")
        assert infos[0]["res"] == info["res"] and infos[0]["cycles"] == info["cycles"]
        R = bref.residual_rounding_bound(a, U, F, L, sigma, bc)
        sg, be = LD(sigma), LD((1.0 - theta) / theta)
        P = np.abs(bref.pad(prev.astype(LD), bc))
        mag = sg * P[1:-1, 1:-1] + be * ref._inv_ld(N, L) * LD(float(a.max())) * (P[2:, 1:-1] + P[:-2, 1:-1] + P[1:-1, 2:] + P[1:-1, :-2] + 4 * P[1:-1, 1:-1])
        eps = 16 * ref.U53 * np.sqrt(np.sum(mag ** 2))          # _heat_vc_ref.rhs_rounding_bound over every unknown
        bound = np.sqrt(np.sum(w ** 2)) * (LD(info["res"]) + R + eps) / sg + N * N * ref.U53 * np.sum(np.abs(w * U.astype(LD)))
        change = abs(wsum(U) - wsum(prev))
        print(f"theta={theta} step {step + 1}: change {float(change):.3e} <= {float(bound):.3e}, sum {float(wsum(U)):.6e}, "
              f"moved {float(np.max(np.abs(U - prev))):.3e}")
        assert change <= bound
        assert bound <= LD(1e-6) * np.sum(np.abs(w * (U - prev).astype(LD))), "no teeth: the field barely moved"
    three, infos = st.step(U0, steps=3)
    assert_bits(three, U, "3 steps in one call")
    st.close(), solver.close(), ga.free()


# ---------------------------------------------------------------- refusals and lifecycle
def test_refusals_leave_the_solver_as_it_was(mg):
    N = 64
    F, U0 = ref.random_problem(N, 7000)
    a = vref.field("smooth", N)
    opts = dict(rtol=0.0, max_cycles=1)

    def refused(s, code, call, match=""):
        want, winfo = s.solve(F, U0)
        kinds = s.boundary
        with pytest.raises(mg.MGError, match=r"\[%d\].*%s" % (code, match)):
            call()
        assert s.boundary == kinds
        got, ginfo = s.solve(F, U0)
        assert_bits(got, want, "the solver solves as before the refusal")
        assert ginfo["history"] == winfo["history"]

    s = mg.Solver(N, 1.0, bc="ndnd", **opts)
    refused(s, 2, lambda: s.set_boundary((0, 2, 0, 0)))
    refused(s, 2, lambda: s.set_boundary((0, -1, 0, 0)))
    refused(s, 3, lambda: s.set_boundary("nnnn"), "singular")
    refused(s, 3, lambda: s.set_krylov(4), "Krylov")
    refused(s, 3, lambda: s.adjoint(np.ones((N, N)), U0), "adjoint")
    assert mg.lib().mg_solver_set_boundary(s._s, None) == 2
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg._check()
    assert s.boundary == (1, 0, 1, 0)
    s.set_krylov(0)                                    # switching it off stays allowed
    s.close()
    s = mg.Solver(N, 1.0, **opts)                      # a plain solver refuses too, and stays plain
    refused(s, 3, lambda: s.set_boundary("nnnn"), "singular")
    refused(s, 2, lambda: s.set_boundary((1, 1, 1, 7)))
    s.close()
    s = mg.Solver(N, 1.0, fmg=1, **opts)
    refused(s, 3, lambda: s.set_boundary("ndnd"), "fmg")
    s.set_boundary("dddd")                             # asks for the state it is in
    s.close()
    s = mg.Solver(N, 1.0, krylov=4, **opts)
    refused(s, 3, lambda: s.set_boundary("ndnd"), "Krylov")
    s.close()
    with pytest.raises(mg.MGError, match=r"\[3\]"):
        mg.Solver(N, 1.0, krylov=4, bc="ndnd")
    assert mg.lib().mg_solver_set_boundary(None, mg._kinds("ndnd")) == 2 and mg.lib().mg_solver_boundary(None, None) == 0
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg._check()
    # the heat stepper: a batched one refuses, a single one passes the solver's refusals through
    st = mg.HeatStepper(N, 1.0, dt=1e-3, max_batch=2)
    with pytest.raises(mg.MGError, match=r"\[3\].*max_batch"):
        st.set_boundary("nnnn")
    st.set_boundary("dddd")
    assert st.boundary == (0, 0, 0, 0)
    st.close()
    st = mg.HeatStepper(N, 1.0, dt=1e-3)
    st.set_boundary("nnnn")                            # sigma > 0: not singular
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        st.set_boundary((3, 0, 0, 0))
    assert st.boundary == (1, 1, 1, 1)
    st.close()
    # building blocks refuse a bad kind
    g = mg.DeviceGrid.zeros((N, N))
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg.applyOperatorBoundary(N, 1.0, 0.0, (0, 0, 5, 0), None, g, g.copy())
    with pytest.raises(TypeError):
        mg.BatchSolver(N, 1.0, 2, bc="ndnd")
    with pytest.raises(TypeError):
        mg.EigenSolver(N, 1.0, bc="ndnd")


def test_coefficient_and_boundary_in_either_order(mg):
    N = 100
    F, U0 = ref.random_problem(N, 7100)
    a = vref.field("exp", N)
    opts = dict(rtol=0.0, max_cycles=2)
    levels = vref.coarsen_levels(a, 8, rtable(mg))
    margins, want = [], U0
    for _ in range(2):
        want = bref.cycle(levels, F, want, "nndn", margins=margins, rtable=rtable(mg), ptable=ptable(mg))
    ref.assert_qualified(margins, "either order")
    s1 = mg.Solver(N, 1.0, **opts)
    s1.set_coefficient(a), s1.set_boundary("nndn")
    s2 = mg.Solver(N, 1.0, **opts)
    s2.set_boundary("nndn"), s2.set_coefficient(a)
    for s in (s1, s2):
        got, _ = s.solve(F, U0)
        assert_bits(got, want, "coefficient and boundary")
    # the coefficient leaves, the boundary stays: a = 1 through the same expressions
    s1.set_coefficient(None)
    got, _ = s1.solve(F, U0)
    want1 = U0
    for _ in range(2):
        want1 = bref.cycle(None, F, want1, "nndn", rtable=rtable(mg), ptable=ptable(mg))
    assert_bits(got, want1, "boundary without a coefficient")
    one, _ = mg.solve(F, U0, coef=np.ones((N, N)), bc="nndn", **opts)
    assert_bits(one, want1, "a == 1 is the solver without a coefficient")
    # a replaced boundary solves as a fresh solver's
    s2.set_boundary("dnnd")
    got, _ = s2.solve(F, U0)
    fresh, _ = mg.solve(F, U0, coef=a, bc="dnnd", **opts)
    assert_bits(got, fresh, "a replaced boundary")
    s1.close(), s2.close()


# ---------------------------------------------------------------- no collateral change
@pytest.mark.parametrize("N", [100, 256])
def test_other_solvers_are_untouched_by_a_boundary_solve(mg, N):
    F, U0 = ref.random_problem(N, 8000 + N)
    opts = dict(rtol=0.0, max_cycles=2, shift=10.0)

    def others():
        U, info = mg.solve(F, U0, **opts)
        b = mg.BatchSolver(N, 1.0, 2, **opts)
        Ub, infos = b.solve(np.stack([F, F]), np.stack([U0, ref.rim_only(U0)]))
        b.close()
        st = mg.HeatStepper(N, 1.0, dt=1e-3, theta=0.5, rtol=1e-8)
        Uh, hinfo = st.step(U0, steps=2)
        st.close()
        return U, info["history"], np.asarray(Ub), [i["history"] for i in infos], Uh, hinfo[0]["cycles_per_step"]

    before = others()
    mg.solve(F, U0, coef=vref.field("exp", N), bc="nnnd", **opts)
    st = mg.HeatStepper(N, 1.0, dt=1e-3, theta=0.5, rtol=1e-8)
    st.set_boundary("nnnn")
    st.step(U0, steps=1)
    st.close()
    after = others()
    for i, what in ((0, "Solver"), (2, "BatchSolver"), (4, "HeatStepper")):
        assert_bits(after[i], before[i], what)
    assert after[1] == before[1] and after[3] == before[3] and after[5] == before[5]


def test_torch_tensors_on_a_side_stream():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_solve_bc_torch_worker.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SOLVE_BC_TORCH OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
