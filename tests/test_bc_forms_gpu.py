"""The column-pair (PAIR) and non-temporal (NT) forms of the boundary-kind kernels (mg_bc_kernels.hip, include/mg_bc.h) at
the sizes that select them, alone and inside whole solves, and the norm kernels, which only a solve can launch.  The
thresholds are constexpr (PAIR_MIN_N = 512, NT_MIN_N = 4096), so the forms run at real sizes only.  `pair` is "N even and
N >= 512", `nt` is "pair and N >= 4096"; N % 4 == 2 (514, 1026, 4098) has rows that are 16-byte but not 32-byte aligned, a last
block of one lane and, in a hierarchy, an even level above an odd one (514 -> 257, 1026 -> 513 -> 256).

Which test launches which instantiation; read off launch<OP> and the launchers at the bottom of mg_bc_kernels.hip.
bc = test_solve_bc_gpu, exact = test_bc_exact_gpu, here = this module.  FORM 0: one column per lane (not pair); 1: pair, not
nt; 2: pair, nt.  The residual's launcher passes always_nt, so its pair sizes all take FORM 2 and <BC_RESIDUAL, *, 1> is never
instantiated (launch<OP> drops that branch for it).  `a` = a coefficient is set, `none` = a = 1.

k_bc<BC_SWEEP, HAS_A, FORM> -- wjacobi_bc with U_in
  <a, 0>, <none, 0>        not pair            bc::test_kernels_alone_every_kind (3 ... 257), ..._single_column_and_pair_forms (100, 255)
  <a, 1>, <none, 1>        pair, not nt        bc::test_kernels_alone_single_column_and_pair_forms (512, 514, 1026); in a solve:
                                               here::test_whole_solves_at_the_pair_sizes (514, 1026)
  <a, 2>                   nt                  bc::test_kernels_alone_non_temporal_form (4096, nnnn); here::test_four_dirichlet_sides_at_4096;
                                               in a solve: here::test_non_temporal_norms_and_the_cycle_from_the_hooks (exp)
  <none, 2>                nt                  here::test_forms_alone (4096, 4098: sweep); in a solve: ..._norms_... (None);
                                               exact::test_mode_solves (4096)
k_bc<BC_SWEEP_ZERO, HAS_A, FORM> -- wjacobi_bc without U_in (every level below the top one)
  <a, 0>                   not pair            bc::test_kernels_alone_... (3 ... 257, 100, 255); every solve with a coefficient
  <none, 0>                not pair            every solve without a coefficient (bc::test_whole_solves_..., here, exact)
  <a, 1>                   pair, not nt        bc::test_kernels_alone_single_column_and_pair_forms (512, 514, 1026); in a solve:
                                               here::test_non_temporal_norms_... (2048, 1024, 512 below 4096)
  <none, 1>                pair, not nt        here::test_forms_alone (512, 514, 1026: sweep0-none); in a solve: ..._norms_... (None)
  <a, 2>, <none, 2>        nt                  here::test_forms_alone (4096, 4098: sweep0, sweep0-none); no solve below 8192
                                               puts a level of 4096 under the top one
k_bc<BC_RESIDUAL, HAS_A, FORM> -- residual_bc, sign +1 / -1
  <a, 0>                   not pair            bc::test_kernels_alone_... (3 ... 257, 100, 255)
  <none, 0>                not pair            every solve without a coefficient, sign -1 (bc::test_whole_solves_...)
  <a, 2>                   pair (every size)   bc::test_kernels_alone_single_column_and_pair_forms (512, 514, 1026, both signs),
                                               ..._non_temporal_form (4096, sign -1); here::test_forms_alone (4096, 4098: sign +1),
                                               test_four_dirichlet_sides_at_4096 (both signs)
  <none, 2>                pair (every size)   here::test_forms_alone (512, 514, 1026, 4096, 4098: residual-none, both signs); in a
                                               solve: here::test_whole_solves_at_the_pair_sizes
  <*, 1>                   never instantiated  (always_nt)
k_bc<BC_APPLY, HAS_A, FORM> -- apply_bc
  <a, 0 | 1>, <none, 0 | 1>                    bc::test_kernels_alone_... (3 ... 257; 512, 514, 1026)
  <a, 2>, <none, 2>        nt                  here::test_forms_alone (4096, 4098: apply)
k_bc<BC_NORM, HAS_A, FORM> -- resnorm_bc with U: only norm() of mg_solve.cpp launches it
  <a, 0>, <none, 0>        not pair            bc::test_whole_solves_bit_identical_to_restatement (64 ... 257: history to 1e-12)
  <a, 1>, <none, 1>        pair, not nt        here::test_whole_solves_at_the_pair_sizes (514, 1026: history to 1e-12)
  <a, 2>, <none, 2>        nt                  here::test_non_temporal_norms_and_the_cycle_from_the_hooks (4096: history to 1e-12)
k_bc<BC_NORM_F, HAS_A, FORM> -- resnorm_bc without U (the norm of F over the unknowns)
  <none, 0>                not pair            bc::test_whole_solves_... (ref_norm to 1e-12)
  <none, 1>, <none, 2>     pair; nt            here::test_whole_solves_at_the_pair_sizes; ..._non_temporal_norms_... (ref_norm)
  <a, *>                   unreachable         resnorm_bc passes A = nullptr whenever U is null
k_bc<BC_HEAT, HAS_A, FORM> -- heat_rhs_bc, theta != 1
  <a, 0 | 1>, <none, 0 | 1>                    bc::test_kernels_alone_... (3 ... 257; 512, 514, 1026); inside the stepper:
                                               bc::test_insulated_walls_conserve_heat (65), exact::test_heat_modes (514, 1026)
  <a, 2>, <none, 2>        nt                  here::test_forms_alone (4096, 4098: heat-half); inside the stepper:
                                               exact::test_heat_mode_at_the_non_temporal_form (4096)
k_bc<BC_HEAT_LOCAL, HAS_A, FORM> -- heat_rhs_bc, theta == 1
  <none, 0 | 1>                                bc::test_kernels_alone_... (theta = 1, with and without a coefficient passed)
  <none, 2>                nt                  here::test_forms_alone (4096, 4098: heat-one)
  <a, *>                   unreachable         heat_rhs_bc passes A = nullptr when theta == 1 (c.lap is false)
Kernels without forms
  k_resnorm_finish_bc      one block           every solve with a boundary (np = the partials of the form that ran)
  k_gs_relative_bc         N <= 63             every solve with a boundary (coarsest level 8 here); all 16 kinds against a direct
                                               solve: bc::test_against_the_direct_solution (17, 24, 33)
  k_restrict_bc, k_prolong_add_bc              bc::test_kernels_alone_... (4 ... 1026, to and from N / 2); every solve; at
                                               4096 <-> 2048: here::test_non_temporal_norms_and_the_cycle_from_the_hooks
  k_neumann_source                             bc::test_kernels_alone_... (3 ... 1026), test_flux_data_end_to_end

Whole cycles are compared with the numpy restatement at 514 and 1026, every coarse solve qualified (margin >= 1e-10, DESIGN
4.3) with seeds chosen on the restatement alone (tests/test_bc_forms_cpu.py); at 4096 the cycle is compared with the same
cycle made of the test hooks at the top level and a Solver of N = 2048 below it, device to device, and the norms with numpy.
A norm differs from numpy's only in the order of its sum: 1e-12, where one missing column of unknowns moves it by 1/N.
Measured on the MI355X: history and ref_norm agree with numpy to at most 3.5e-16 (514, 1026) and 7.0e-16 (4096), relative; the
cycle made of the hooks gives the solver's bits with and without a coefficient.  The slowest case takes 0.9 s."""
import functools

import numpy as np
import pytest

import _bc_forms_cases as cases
import _bc_ref as bref
import _guard
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits
from test_solve_bc_gpu import ptable, rtable

pytestmark = pytest.mark.gpu
OMEGA, NU, DT = 0.8, 0.7, 1e-3


# ================================================================ 1. kernels alone, inside guard bands
@functools.lru_cache(maxsize=1)
def _inputs(N):
    """(a, U, F) of test_solve_bc_gpu._kernel_ops, shared by the cases of one size (read-only)"""
    F, U = ref.random_problem(N, 10 * N + 1)
    return vref.field("random", N, seed=N), U, F


class _Block:
    """one guarded block [a, U, F, out] per size, kept while the cases of that size run: the inputs are uploaded once and
    every case checks that they, and the bands, are as they were"""
    held = None

    @classmethod
    def get(cls, mg, N, placement):
        if cls.held is not None and cls.held[0] != (N, placement):
            cls.drop()
        if cls.held is None:
            gb = _guard.block(mg, [N, N, N, N], placement)
            for view, x in zip(gb.views, _inputs(N)):
                view.upload(x)
            cls.held = ((N, placement), gb)
        return cls.held[1]

    @classmethod
    def drop(cls):
        if cls.held is not None:
            cls.held[1].free()
        cls.held = None


@pytest.fixture(scope="module", autouse=True)
def _release_the_block():
    yield
    _Block.drop()


def _launches(mg, op, N, L, shift, bc, ga, gU, gF, gout):
    """[(what, launch, reference)] of one case: one or two launches"""
    a, U, F = _inputs(N)
    sweep = lambda A, Uin: lambda: mg.sweepBoundary(N, L, shift, OMEGA, bc, A, Uin, gF, gout)
    res = lambda A, sign: lambda: mg.residualBoundary(N, L, shift, bc, A, gU, gF, gout, sign)
    heat = lambda theta, A, Q: lambda: mg.heat_rhs_boundary(N, L, NU, DT, theta, bc, A, gU, Q, gout)
    href_ = lambda theta, A, Q: lambda: bref.heat_rhs(N, L, NU, DT, theta, bc, A, U, Q)
    if op == "sweep":
        return [("sweep a=None", sweep(None, gU), lambda: bref.weighted_sweeps(N, L, bc, None, U, F, OMEGA, 1, shift))]
    if op == "sweep0":
        return [("zero-start sweep", sweep(ga, None), lambda: bref.weighted_sweeps(N, L, bc, a, None, F, OMEGA, 1, shift, zero_start=True))]
    if op == "sweep0-none":
        return [("zero-start sweep a=None", sweep(None, None),
                 lambda: bref.weighted_sweeps(N, L, bc, None, None, F, OMEGA, 1, shift, zero_start=True))]
    if op == "residual-none":
        return [(f"residual a=None sign {s}", res(None, s), lambda s=s: bref.residual(N, L, bc, None, U, F, shift, s)) for s in (+1, -1)]
    if op == "residual":
        return [("residual sign 1", res(ga, +1), lambda: bref.residual(N, L, bc, a, U, F, shift, +1))]
    if op == "apply":
        return [("apply", lambda: mg.applyOperatorBoundary(N, L, shift, bc, ga, gU, gout), lambda: bref.apply_operator(N, L, bc, a, U, shift)),
                ("apply a=None", lambda: mg.applyOperatorBoundary(N, L, shift, bc, None, gU, gout),
                 lambda: bref.apply_operator(N, L, bc, None, U, shift))]
    if op == "heat-half":      # the (theta, coef, Q) tuples of test_solve_bc_gpu._kernel_ops
        return [("heat theta=0.5 a q", heat(0.5, ga, gF), href_(0.5, a, F)), ("heat theta=0.5", heat(0.5, None, None), href_(0.5, None, None))]
    if op == "heat-one":
        return [("heat theta=1 a q", heat(1.0, ga, gF), href_(1.0, a, F)), ("heat theta=1 a", heat(1.0, ga, None), href_(1.0, a, None))]
    raise ValueError(op)


@pytest.mark.parametrize("N,bc,op,L,shift", cases.FORM_CASES)
def test_forms_alone(mg, N, bc, op, L, shift):
    """one operation, one combination of kinds, one or two launches: bits against the restatement, the inputs unchanged,
    nothing outside the output written (the output starts as all-ones bytes)"""
    gb = _Block.get(mg, N, "odd16" if N % 4 == 2 else "page")
    ga, gU, gF, gout = gb.views
    for what, call, want in _launches(mg, op, N, L, shift, bc, ga, gU, gF, gout):
        label = f"{what} {bc} N={N} L={L} shift={shift}"
        gout.poison()
        gb.expect_readonly(ga, gU, gF)
        call()
        gb.check(label)
        assert_bits(gout.to_host(), want(), label)


def test_four_dirichlet_sides_at_4096(mg):
    """bc::test_four_dirichlet_sides_through_the_hooks at the non-temporal form: sweepBoundary / residualBoundary with "dddd"
    equal sweepCoefficient / residualCoefficient, device to device"""
    N = 4096
    _, U, F = _inputs(N)
    ga, gU, gF = (mg.DeviceGrid.from_host(x) for x in (vref.field("exp", N), U, F))
    o1, o2 = mg.DeviceGrid((N, N)), mg.DeviceGrid((N, N))
    zero = mg.DeviceGrid.zeros((N, N)).checksum()
    try:
        for shift in (0.0, 1e2):
            for U_in in (gU, None):
                mg.sweepBoundary(N, 1.0, shift, OMEGA, "dddd", ga, U_in, gF, o1)
                mg.sweepCoefficient(N, 1.0, shift, OMEGA, ga, U_in, gF, o2)
                assert o1.checksum() != zero
                assert_bits(o1.to_host(), o2.to_host(), f"sweep N={N} shift={shift} U_in={U_in is not None}")
            for sign in (1, -1):
                mg.residualBoundary(N, 1.0, shift, "dddd", ga, gU, gF, o1, sign)
                mg.residualCoefficient(N, 1.0, shift, ga, gU, gF, o2, sign)
                assert_bits(o1.to_host(), o2.to_host(), f"residual N={N} shift={shift} sign={sign}")
    finally:
        for x in (ga, gU, gF, o1, o2):
            x.free()


# ================================================================ 2. whole solves and norms at the pair sizes
@pytest.mark.parametrize("N,bc,shift,name,pp", cases.SOLVE_CASES)
def test_whole_solves_at_the_pair_sizes(mg, N, bc, shift, name, pp):
    """bc::test_whole_solves_bit_identical_to_restatement at 514 -> 257 and 1026 -> 513 -> 256: every coarse solve qualified,
    then U (rim included) after cycles 1 and 2 bit for bit, data points untouched, and history and ref_norm -- k_bc<BC_NORM, *, 1>
    and k_bc<BC_NORM_F, none, 1> -- to 1e-12 against numpy's sums of the same residual bits"""
    what = f"N={N} {bc} shift={shift:g} a={name} {pp}"
    F, U0, a, Us, hist, margins = cases.restated_cycles(N, bc, shift, name, pp, rtable(mg), ptable(mg))
    ref.assert_qualified(margins, what)
    m = bref.mask(N, bc)
    want_ref = bref.ref_norm(F, bc)
    for k in (1, 2):
        s = mg.Solver(N, 1.0, coef=a, bc=bc, rtol=0.0, max_cycles=k, pre=pp[0], post=pp[1], shift=shift)
        try:
            got, info = s.solve(F, U0)
        finally:
            s.close()
        worst = max(abs(g - h) / h for g, h in zip(info["history"], hist))
        print(f"{what}: cycle {k}, largest relative disagreement of the history {worst:.2e}, of ref_norm "
              f"{abs(info['ref_norm'] - want_ref) / want_ref:.2e}")
        assert_bits(got, Us[k - 1], f"{what}: U after cycle {k}")
        assert_bits(got[~m], U0[~m], "data points")
        assert info["cycles"] == k and not info["converged"]
        np.testing.assert_allclose(info["history"], hist[:k + 1], rtol=1e-12, atol=0.0)
        assert abs(info["ref_norm"] - want_ref) <= 1e-12 * want_ref


def _cycle_from_the_hooks(mg, N, bc, shift, ga, gF, gU, pre=3, post=3):
    """One V(pre, post) cycle on gU in place: the test hooks at the top level, a Solver of N / 2 on the restricted right-hand
    side below it -- its top level starts from a zero field where the cycle's level 1 starts from nothing, the same bits: a
    sweep of a zero field adds b(0) = +0 where the zero-start sweep adds the constant 0.0."""
    M = N // 2
    cur, other = gU, mg.DeviceGrid((N, N))
    gFc, gUc = mg.DeviceGrid((M, M)), mg.DeviceGrid.zeros((M, M))
    gac = None
    if ga is not None:
        gac = mg.DeviceGrid((M, M))
        mg.coarsenCoefficient(N, ga, M, gac)
    sub = mg.Solver(M, 1.0, coef=gac, bc=bc, shift=shift, rtol=0.0, max_cycles=1, pre=pre, post=post)
    try:
        for _ in range(pre):
            mg.sweepBoundary(N, 1.0, shift, OMEGA, bc, ga, cur, gF, other)
            cur, other = other, cur
        mg.residualBoundary(N, 1.0, shift, bc, ga, cur, gF, other, -1)
        mg.restrictBoundary(N, bc, other, M, gFc)
        info = sub.solve(gFc, gUc)[1]
        assert info["cycles"] == 1
        mg.prolongAddBoundary(M, bc, gUc, N, cur, other)
        cur, other = other, cur
        for _ in range(post):
            mg.sweepBoundary(N, 1.0, shift, OMEGA, bc, ga, cur, gF, other)
            cur, other = other, cur
        out = cur.to_host()
    finally:
        sub.close()
        for g in (cur if cur is not gU else other, gFc, gUc) + ((gac,) if gac is not None else ()):
            g.free()
    return out


@pytest.mark.parametrize("name", [None, "exp"])
def test_non_temporal_norms_and_the_cycle_from_the_hooks(mg, name):
    """N = 4096, "nnnd", shift 10, one cycle: history[0] and ref_norm against numpy on the inputs, history[1] against numpy on
    the returned U (k_bc<BC_NORM, *, 2>, k_bc<BC_NORM_F, none, 2>), all to 1e-12; the returned U bit for bit the cycle made of
    the hooks; data points untouched"""
    N, bc, shift = 4096, "nnnd", 10.0
    _, U0, F = _inputs(N)
    a = vref.field("exp", N) if name else None
    s = mg.Solver(N, 1.0, coef=a, bc=bc, rtol=0.0, max_cycles=1, shift=shift)
    try:
        U, info = s.solve(F, U0)
    finally:
        s.close()
    want = [bref.residual_norm(N, 1.0, bc, a, U0, F, shift), bref.residual_norm(N, 1.0, bc, a, U, F, shift)]
    want_ref = bref.ref_norm(F, bc)
    print(f"N={N} a={name}: history {info['history']} vs numpy {want}: relative {[abs(g - h) / h for g, h in zip(info['history'], want)]}, "
          f"ref_norm {info['ref_norm']!r} vs {want_ref!r}: {abs(info['ref_norm'] - want_ref) / want_ref:.2e}")
    assert info["cycles"] == 1 and len(info["history"]) == 2 and info["history"][1] < info["history"][0]
    np.testing.assert_allclose(info["history"], want, rtol=1e-12, atol=0.0)
    assert abs(info["ref_norm"] - want_ref) <= 1e-12 * want_ref
    m = bref.mask(N, bc)
    assert_bits(U[~m], U0[~m], "data points")
    ga = mg.DeviceGrid.from_host(a) if name else None
    gF, gU = mg.DeviceGrid.from_host(F), mg.DeviceGrid.from_host(U0)
    try:
        mine = _cycle_from_the_hooks(mg, N, bc, shift, ga, gF, gU)
    finally:
        for g in (gF, gU) + ((ga,) if ga is not None else ()):
            g.free()
    assert_bits(U, mine, f"N={N} a={name}: the solver's cycle against the cycle made of the hooks")
