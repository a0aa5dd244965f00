"""The two-column (PAIR) and non-temporal (NT) forms of the shifted solve, the heat stepper and the variable-coefficient solve
at the sizes that select them.  In mg_solve_kernels.hip, mg_heat_kernels.hip and mg_varcoef_kernels.hip the thresholds are
constexpr (PAIR_MIN_N = 512, NT_MIN_N = 4096; the MG_*_MIN_N overrides of conftest.py do not reach them), so these forms run
at real sizes only: 512, 514 and 1026 for the pair form, 4096 and 4098 for the non-temporal one.  4098 is even with
N % 4 == 2: 2049 column pairs (a last block of one lane), a last row block of two rows, and rows that are 16-byte but not
32-byte aligned; the N % 4 == 2 sizes lie on the "odd16" placement of tests/_guard.py wherever the test places the arrays.

Every comparison with a whole cycle of a numpy restatement first asserts the qualification rule (coarse margin >= 1e-10,
DESIGN 4.3); the seeds below were chosen so that the restatement alone qualifies.  Norms are compared at rtol 1e-12, fields
bit for bit (zero_sign where the solve tests of the feature use it; device checksums above _guard.DOWNLOAD_MAX_N).

Which test launches which instantiation.  `pair` is "N even and N >= 512", `nt` is "pair and N >= 4096"; vc = test_solve_vc_gpu,
shift = test_solve_shift_gpu, heat = test_heat_gpu, solve = test_solve_gpu, batched = test_solve_batched_gpu, here = this module.

mg_solve_kernels.hip -- wjacobi (MG_SMOOTHER=simple), resnorm, resnorm_batch
  k_wjacobi<true>, k_wjacobi_sh<true>   U_in == NULL, any N           every simple-smoother test with three or more levels (below)
  k_wjacobi<false>                  not pair, shift == 0            solve::test_fused_path_equals_simple_smoother (100 ... 1025)
  k_wjacobi_sh<false>               not pair, shift != 0            shift::test_fused_path_equals_simple_smoother (256 ... 1025)
  k_wjacobi_pairs<false>            pair, not nt, shift == 0        solve::test_fused_path_equals_simple_smoother (1024, 2048)
  k_wjacobi_pairs<true>             nt, shift == 0                  here::test_unit_coefficient_at_the_nt_size (its simple run)
  k_wjacobi_pairs_sh<false>         pair, not nt, shift != 0        shift::test_fused_path_equals_simple_smoother (1024, 2048)
  k_wjacobi_pairs_sh<true>          nt, shift != 0                  here::test_shifted_cycle_at_the_nt_size_in_both_smoothers
  k_resnorm<true>, k_resnorm<false> not pair, shift == 0 or no U    solve::test_history_matches_restatement_and_is_reproducible
  k_resnorm_sh                      not pair, U, shift != 0         shift::test_history_and_stopping_rule_match_restatement (100, 257)
  k_resnorm_pairs<true, false>      pair, not nt, U, shift == 0     solve::test_fused_path_equals_simple_smoother (1024, 2048: the histories)
  k_resnorm_pairs<false, false>     pair, not nt, U == NULL         the same (ref_norm of every solve); shift::test_history_and_stopping_rule_... (1024)
  k_resnorm_pairs<true, true>       nt, U, shift == 0               solve::test_product_size_two_cycles; here::test_unit_coefficient_at_the_nt_size
  k_resnorm_pairs<false, true>      nt, U == NULL (ref_norm)        solve::test_product_size_two_cycles; here::test_shifted_norm_kernels_alone
  k_resnorm_pairs_sh<false>         pair, not nt, U, shift != 0     shift::test_sizes_shifts_lengths_bit_identical_to_restatement (1024)
  k_resnorm_pairs_sh<true>          nt, U, shift != 0               here::test_shifted_norm_kernels_alone, test_shifted_cycle_at_the_nt_size_...
  k_resnorm_b<true>, <false>        batch: not pair                 batched::test_fused_batch_equals_simple_batch (129, 1025)
  k_resnorm_sh_b                    batch: not pair, shift != 0     test_solve_shift_batched_gpu::test_batch_against_restatement (100, 255)
  k_resnorm_pairs_b<true, false>    batch: pair, not nt, shift == 0 shift::test_explicit_zero_shift_is_the_option_left_alone (1024)
  k_resnorm_pairs_b<false, false>   batch: pair, not nt, ref_norm   the same; test_solve_shift_batched_gpu::test_batch_against_restatement (1024)
  k_resnorm_pairs_b<true, true>     batch: nt, shift == 0           batched::test_large_sizes (4096)
  k_resnorm_pairs_b<false, true>    batch: nt, ref_norm             batched::test_large_sizes; here::test_shifted_norm_kernels_alone
  k_resnorm_pairs_sh_b<false>       batch: pair, not nt, shift != 0 test_solve_shift_batched_gpu::test_batch_against_restatement (1024)
  k_resnorm_pairs_sh_b<true>        batch: nt, shift != 0           here::test_shifted_norm_kernels_alone, test_shifted_batch_equals_single_at_4098

mg_heat_kernels.hip -- heat_rhs (mg_heat_rhs), heat_rhs_batch (every step of a stepper, max_batch == 1 included); LAP: theta != 1
  k_heat_rhs<LAP, false, false>     not pair                        heat::test_heat_rhs_bit_identical_to_restatement (6 ... 1025), both LAP
  k_heat_rhs<LAP, true, false>      pair, not nt                    the same (512, 1024), both LAP; heat::test_heat_rhs_inside_guard_bands (512)
  k_heat_rhs<LAP, true, true>       nt                              heat::test_heat_rhs_non_temporal_form (4096), both LAP
  k_heat_rhs_b<LAP, false, false>   not pair                        heat::test_stepper_equals_its_building_blocks (both LAP, one instance),
                                                                    test_batch_instances_equal_single_steppers (LAP = true, three instances);
                                                                    here::test_batched_step_inside_guard_bands (257)
  k_heat_rhs_b<LAP, true, false>    pair, not nt                    here::test_stepper_equals_its_building_blocks (512, 514; both LAP, one and
                                                                    two instances), test_stepper_bit_identical_to_restatement_at_the_pair_form,
                                                                    test_batched_step_inside_guard_bands (512, 514; LAP = true)
  k_heat_rhs_b<LAP, true, true>     nt                              here::test_stepper_equals_its_building_blocks (4096: both LAP; 4098: LAP = true)

mg_varcoef_kernels.hip -- wjacobi_vc, residual_vc, resnorm_vc
  k_wjacobi_vc<false, false, false> not pair, U_in given            vc::test_kernels_alone_bit_for_bit_inside_guard_bands (3 ... 257)
  k_wjacobi_vc<true, false, false>  not pair, U_in == NULL          the same ("zero-start sweep")
  k_wjacobi_vc<false, true, false>  pair, not nt, U_in given        the same (512, 514, 1026)
  k_wjacobi_vc<true, true, false>   pair, not nt, U_in == NULL      the same; in a cycle: here::test_vc_several_pair_form_levels (1024 and 512 of 2048)
  k_wjacobi_vc<false, true, true>   nt, U_in given                  here::test_vc_kernels_alone_at_the_nt_size, test_vc_cycle_at_the_nt_size
  k_wjacobi_vc<true, true, true>    nt, U_in == NULL                here::test_vc_kernels_alone_at_the_nt_size ("zero-start sweep")
  k_residual_vc<false>              not pair                        vc::test_kernels_alone_bit_for_bit_inside_guard_bands (3 ... 257)
  k_residual_vc<true>               pair (non-temporal at every N)  the same (512, 514, 1026); here::test_vc_kernels_alone_at_the_nt_size (4096, 4098,
                                                                    both signs), test_vc_several_pair_form_levels (several levels of one cycle)
  k_resnorm_vc<false, false>        not pair                        vc::test_whole_solves_bit_identical_to_restatement (64 ... 257)
  k_resnorm_vc<true, false>         pair, not nt                    the same (512); here::test_vc_several_pair_form_levels (1026, 2048)
  k_resnorm_vc<true, true>          nt                              here::test_vc_norm_at_the_nt_size, test_unit_coefficient_at_the_nt_size,
                                                                    test_vc_cycle_at_the_nt_size"""
import numpy as np
import pytest

import _guard
import _heat_ref as href
import _solve_ref as ref
import _solve_shift_ref as sref
import _solve_vc_ref as vref
from conftest import assert_bits
from test_solve_vc_gpu import _against_restatement, _kernel_ops, lib_table

pytestmark = pytest.mark.gpu

NT_SIZES = [4096, 4098]
NU, DT = 0.5, 2e-4          # the heat tests' scheme: sigma = 1e4 (theta = 1), 2e4 (theta = 0.5)
# seeds of the cases that compare a whole restatement cycle: each one qualifies (checked on the restatement alone)
SEED_SHIFT_CYCLE = 4096
SEED_HEAT_PAIR = 600
SEED_VC_CYCLE = 4096
SEED_VC_LEVELS = {1026: 4026, 2048: 5048}


def place(N):
    """the placement of tests/_guard.py for arrays of side N: rows that are 16-byte aligned and no more get a base that is, too"""
    return "odd16" if N % 4 == 2 else "page"


def same_field(got, want, what):
    """two device arrays hold the same bits (up to the sign of zeros above DOWNLOAD_MAX_N: mg_checksum canonicalises it)"""
    if got.shape[0] <= _guard.DOWNLOAD_MAX_N:
        assert_bits(got.to_host(), want.to_host(), what)
    else:
        assert got.checksum() == want.checksum(), f"{what}: device checksums differ"


def heat_fields(N, seed):
    Q, U = ref.random_problem(N, seed)
    return U, 40.0 * Q


# ================================================================ 1. shifted solve
@pytest.mark.parametrize("sigma", [1e4, 2.0 ** -20])
@pytest.mark.parametrize("N", NT_SIZES)
def test_shifted_norm_kernels_alone(mg, N, sigma):
    """atol = 1e300: the solve is its two norms.  k_resnorm_pairs_sh<true> from Solver, k_resnorm_pairs_sh_b<true> from
    BatchSolver (two different problems in one launch): res0 is the norm of the caller's arrays, the batch's equals the single
    solver's, nothing is written."""
    L = 2.5
    probs = [ref.random_problem(N, 100 + N + i) for i in range(2)]
    want = [sref.residual_norm(N, L, U0, F, sigma) for F, U0 in probs]
    assert abs(want[0] - want[1]) > 1e-9 * want[0]   # (a norm of the wrong instance would show)
    opts = dict(shift=sigma, atol=1e300)
    with _guard.block(mg, [N] * 4, place(N)) as b:
        F0, U0, F1, U1 = b.views
        for v, a in ((F0, probs[0][0]), (U0, probs[0][1]), (F1, probs[1][0]), (U1, probs[1][1])):
            v.upload(a)
        b.expect_readonly(F0, U0, F1, U1)
        s = mg.Solver(N, L, **opts)
        try:
            single = [s.solve_ptr(F0.ptr, U0.ptr), s.solve_ptr(F1.ptr, U1.ptr)]
        finally:
            s.close()
        bs = mg.BatchSolver(N, L, max_batch=2, **opts)
        try:
            batch = bs.solve_ptrs([F0.ptr, F1.ptr], [U0.ptr, U1.ptr])
        finally:
            bs.close()
        b.check(f"zero-cycle shifted solves N={N} sigma={sigma:g}")
    for i, (F, _) in enumerate(probs):
        for who, info in (("Solver", single[i]), ("BatchSolver", batch[i])):
            what = f"{who} N={N} sigma={sigma:g} instance {i}"
            print(f"{what}: res0 {info['res0']!r}, restatement {want[i]!r}")
            assert info["cycles"] == 0 and info["converged"] and info["status"] == 0, what
            assert info["history"] == [info["res0"]] and info["res"] == info["res0"], what
            np.testing.assert_allclose(info["res0"], want[i], rtol=1e-12, atol=0, err_msg=what)
            np.testing.assert_allclose(info["ref_norm"], ref.ref_norm(F), rtol=1e-12, atol=0, err_msg=what)
        assert batch[i]["res0"] == single[i]["res0"] and batch[i]["ref_norm"] == single[i]["ref_norm"], i


def test_shifted_cycle_at_the_nt_size_in_both_smoothers(mg, oracle):
    """One V(1,1) cycle at N = 4096, sigma = 1e4, against _solve_shift_ref.cycle: through the fused nodes, and operator by
    operator (MG_SMOOTHER=simple: k_wjacobi_pairs_sh<true>, which nothing else launches)."""
    N, sigma = 4096, 1e4
    F, U0 = ref.random_problem(N, SEED_SHIFT_CYCLE)
    opts = dict(pre=1, post=1, shift=sigma)
    margins = []
    want = sref.cycle(oracle, F, U0, 1.0, margins=margins, **opts)
    ref.assert_qualified(margins, f"N={N} sigma={sigma:g}")
    hist = [sref.residual_norm(N, 1.0, U, F, sigma) for U in (U0, want)]
    Fd = mg.DeviceGrid.from_host(F)
    s = mg.Solver(N, 1.0, rtol=0.0, max_cycles=1, **opts)
    infos = {}
    try:
        for smoother in ("stream", "simple"):
            mg.set_smoother(smoother)
            got, info = s.solve(Fd, U0)
            assert info["cycles"] == 1 and not info["converged"] and not info["coarse_capped"], smoother
            assert_bits(got, want, f"N={N} sigma={sigma:g} smoother {smoother}: U after one cycle", zero_sign=True)
            np.testing.assert_allclose(info["history"], hist, rtol=1e-12, atol=0, err_msg=smoother)
            infos[smoother] = info
    finally:
        mg.set_smoother("stream")
        s.close()
        Fd.free()
    assert infos["stream"]["history"] == infos["simple"]["history"]


def test_shifted_batch_equals_single_at_4098(mg):
    """Two instances, two cycles, sigma = 1e4 on the odd16 placement: every instance is its single solve (the pattern of
    test_solve_batched_gpu.py::test_large_sizes), F is read only and nothing outside the arrays is written."""
    N = 4098
    probs = [ref.random_problem(N, 300 + i) for i in range(2)]
    opts = dict(rtol=0.0, max_cycles=2, shift=1e4)
    with _guard.block(mg, [N] * 6, place(N)) as b:
        F0, U0, F1, U1, W0, W1 = b.views
        for v, a in ((F0, probs[0][0]), (U0, probs[0][1]), (W0, probs[0][1]), (F1, probs[1][0]), (U1, probs[1][1]), (W1, probs[1][1])):
            v.upload(a)
        b.expect_readonly(F0, F1)
        bs = mg.BatchSolver(N, 1.0, max_batch=2, **opts)
        try:
            infos = bs.solve_ptrs([F0.ptr, F1.ptr], [U0.ptr, U1.ptr])
        finally:
            bs.close()
        s = mg.Solver(N, 1.0, **opts)
        try:
            singles = [s.solve_ptr(F0.ptr, W0.ptr), s.solve_ptr(F1.ptr, W1.ptr)]
        finally:
            s.close()
        b.check(f"shifted batch and single solves N={N}")
        for i, (U, W) in enumerate(((U0, W0), (U1, W1))):
            assert U.checksum() == W.checksum(), f"N={N} instance {i}"
            assert infos[i]["history"] == singles[i]["history"] and infos[i]["cycles"] == singles[i]["cycles"] == 2
            assert infos[i]["history"][2] < infos[i]["history"][0]
        assert U0.checksum() != U1.checksum()


# ================================================================ 2. heat stepper
STEPPER_CASES = [(N, theta, n) for N in (512, 514, 4096) for theta in (1.0, 0.5) for n in (1, 2)] + [(4098, 0.5, 2)]


@pytest.mark.parametrize("N,theta,n", STEPPER_CASES)
def test_stepper_equals_its_building_blocks(mg, N, theta, n):
    """Two steps of a stepper (k_heat_rhs_b, whatever max_batch is) against two times {mg_heat_rhs, Solver(shift = sigma)} on
    every instance: the single kernel k_heat_rhs is pinned to numpy at these forms by test_heat_gpu.py, the shifted solver at
    4096 by the tests above, so the chain does not run the batched kernel it checks.  Two instances: different fields, with
    a Q each, one shared Q, and a NULL entry of Q."""
    steps, opts = 2, dict(rtol=1e-8)
    data = [heat_fields(N, 400 + N + i) for i in range(n)]
    hs = mg.HeatStepper(N, 1.0, NU, DT, theta, max_batch=n, **opts)
    sv = mg.Solver(N, 1.0, shift=hs.sigma, **opts)
    try:
        assert hs.sigma == href.consts(N, 1.0, NU, DT, theta)[0]
        with _guard.block(mg, [N] * (3 * n + 1), place(N)) as b:
            Ua, Ub, Qs, Fv = b.views[:n], b.views[n:2 * n], b.views[2 * n:3 * n], b.views[3 * n]
            for q, (_, Q) in zip(Qs, data):
                q.upload(Q)
            Fv.poison()
            variants = [("a Q each", list(Qs))]
            variants += [("one shared Q", [Qs[0], Qs[0]]), ("a NULL entry of Q", [None, Qs[1]])] if n == 2 else [("no Q", [None])]
            for name, qs in variants:
                for ua, ub, (U, _) in zip(Ua, Ub, data):
                    ua.upload(U), ub.upload(U)
                b.expect_readonly(*Qs)
                infos = hs.step_ptrs([u.ptr for u in Ua], [q.ptr if q is not None else None for q in qs], steps=steps)
                total = 0
                for i in range(n):
                    what = f"N={N} theta={theta} n={n}, {name}, instance {i}"
                    cycles = []
                    for _ in range(steps):
                        mg.heat_rhs(N, 1.0, NU, DT, theta, Ub[i], qs[i], Fv)
                        info = sv.solve_ptr(Fv.ptr, Ub[i].ptr)
                        cycles.append(info["cycles"])
                    same_field(Ua[i], Ub[i], what + ": stepper vs heat_rhs + Solver")
                    assert infos[i]["cycles_per_step"] == cycles and infos[i]["steps"] == steps and infos[i]["cycles"] == sum(cycles), what
                    assert infos[i]["status"] == 0 and infos[i]["res"] == info["res"] and infos[i]["ref_norm"] == info["ref_norm"], what
                    total += sum(cycles)
                assert total > 0, name
                b.check(f"stepper N={N} theta={theta} n={n}, {name}")
                if n == 2:
                    assert Ua[0].checksum() != Ua[1].checksum()
    finally:
        hs.close(); sv.close()


@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_stepper_bit_identical_to_restatement_at_the_pair_form(mg, oracle, theta):
    """N = 512: one step of a single stepper and of a batch of two against _heat_ref.run."""
    N = 512
    data = [heat_fields(N, SEED_HEAT_PAIR + i) for i in range(2)]
    wants = []
    for i, (U, Q) in enumerate(data):
        margins = []
        want, cycles, conv = href.run(oracle, U, Q, steps=1, L=2.5, nu=NU, dt=DT, theta=theta, rtol=1e-8, margins=margins)
        ref.assert_qualified(margins, f"N={N} theta={theta} field {i}")
        assert conv and sum(cycles) > 0
        wants.append((want, cycles))
    single = mg.HeatStepper(N, 2.5, NU, DT, theta, rtol=1e-8)
    batch = mg.HeatStepper(N, 2.5, NU, DT, theta, max_batch=2, rtol=1e-8)
    try:
        got, infos = single.step(data[0][0], data[0][1], steps=1)
        assert_bits(got, wants[0][0], f"N={N} theta={theta}: single stepper", zero_sign=True)
        assert infos[0]["converged"] and infos[0]["cycles_per_step"] == wants[0][1]
        got, infos = batch.step(np.stack([d[0] for d in data]), np.stack([d[1] for d in data]), steps=1)
        for i, (want, cycles) in enumerate(wants):
            assert_bits(got[i], want, f"N={N} theta={theta}: batch instance {i}", zero_sign=True)
            assert infos[i]["converged"] and infos[i]["cycles_per_step"] == cycles
    finally:
        single.close(); batch.close()


@pytest.mark.parametrize("placement", list(_guard.PLACEMENTS))
@pytest.mark.parametrize("N", [257, 512, 514])
def test_batched_step_inside_guard_bands(mg, N, placement):
    """One batched Crank-Nicolson step of two instances on [U0, U1, Q] inside a caller's block: Q is read only, every band
    is intact, both U are the ones of the step on plain arrays."""
    (U0, Q), (U1, _) = heat_fields(N, 700 + N), heat_fields(N, 701 + N)
    hs = mg.HeatStepper(N, 1.0, NU, DT, 0.5, max_batch=2, rtol=1e-8)
    try:
        want, winfos = hs.step(np.stack([U0, U1]), Q, steps=1)
        with _guard.block(mg, [N] * 3, placement) as b:
            g0, g1, gQ = b.views
            g0.upload(U0), g1.upload(U1), gQ.upload(Q)
            b.expect_readonly(gQ)
            infos = hs.step_ptrs([g0.ptr, g1.ptr], [gQ.ptr, gQ.ptr], steps=1)
            b.check(f"mg_heat_stepper_step N={N} {placement}")
            for i, g in enumerate((g0, g1)):
                assert_bits(g.to_host(), want[i], f"N={N} {placement} instance {i}: guarded vs plain arrays")
                assert infos[i]["cycles_per_step"] == winfos[i]["cycles_per_step"] and infos[i]["status"] == 0
            assert sum(i["cycles"] for i in infos) > 0
    finally:
        hs.close()


# ================================================================ 3. variable coefficient
@pytest.mark.parametrize("ops", [("sweep", "sweep0"), ("residual",)], ids=["sweeps", "residuals"])
@pytest.mark.parametrize("L,shift", [(1.0, 0.0), (2.5, 1e4)])
@pytest.mark.parametrize("N", NT_SIZES)
def test_vc_kernels_alone_at_the_nt_size(mg, N, L, shift, ops):
    """k_wjacobi_vc<false, true, true>, k_wjacobi_vc<true, true, true> and k_residual_vc<true> (both signs) inside guard bands,
    bit for bit against the restatement on the random coefficient; at 4098 the last block of a row holds one lane."""
    _kernel_ops(mg, N, L, shift, place(N), ops)


@pytest.mark.parametrize("L,shift", [(1.0, 0.0), (2.5, 1e4)])
@pytest.mark.parametrize("N", NT_SIZES)
def test_vc_norm_at_the_nt_size(mg, N, L, shift):
    """atol = 1e300: k_resnorm_vc<true, true> alone; res0 is the restatement's norm and nothing is written"""
    a = vref.field("random", N, seed=N)
    F, U0 = ref.random_problem(N, 800 + N)
    want = vref.residual_norm(N, L, a, U0, F, shift)
    with _guard.block(mg, [N] * 3, place(N)) as b:
        ga, gF, gU = b.views
        ga.upload(a), gF.upload(F), gU.upload(U0)
        b.expect_readonly(ga, gF, gU)
        s = mg.Solver(N, L, coef=ga, shift=shift, atol=1e300)
        try:
            assert s.has_coefficient
            info = s.solve_ptr(gF.ptr, gU.ptr)
        finally:
            s.close()
        b.check(f"zero-cycle coefficient solve N={N} L={L} shift={shift}")
    print(f"N={N} L={L} shift={shift}: res0 {info['res0']!r}, restatement {want!r}")
    assert info["cycles"] == 0 and info["converged"] and info["history"] == [info["res0"]]
    np.testing.assert_allclose(info["res0"], want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(info["ref_norm"], ref.ref_norm(F), rtol=1e-12, atol=0)


@pytest.mark.parametrize("shift", [0.0, 1e2])
def test_unit_coefficient_at_the_nt_size(mg, shift):
    """N = 4096, V(1,1), two cycles: a == 1 is the constant solver, fused and operator by operator -- U by checksum, the
    history with ==, which holds k_resnorm_vc<true, true> to the partition and the summation order of k_resnorm_pairs."""
    N = 4096
    F, U0 = ref.random_problem(N, 900)
    opts = dict(pre=1, post=1, shift=shift, rtol=0.0, max_cycles=2)
    Fd, Ud = mg.DeviceGrid.from_host(F), mg.DeviceGrid.from_host(U0)
    one = mg.DeviceGrid.from_host(np.ones((N, N)))
    start = Ud.checksum()
    others = []
    plain = mg.Solver(N, 1.0, **opts)
    try:
        for smoother in ("stream", "simple"):
            mg.set_smoother(smoother)
            info = plain.solve_ptr(Fd.ptr, Ud.ptr)
            others.append((smoother, Ud.checksum(), info))
            Ud.free()
            Ud = mg.DeviceGrid.from_host(U0)
    finally:
        mg.set_smoother("stream")
        plain.close()
    s = mg.Solver(N, 1.0, coef=one, **opts)
    try:
        assert s.has_coefficient
        got = s.solve_ptr(Fd.ptr, Ud.ptr)
    finally:
        s.close()
    sum_got = Ud.checksum()
    for g in (Fd, Ud, one):
        g.free()
    assert got["cycles"] == 2 and sum_got != start and got["history"][2] < got["history"][0]
    for smoother, sum_other, other in others:
        assert sum_got == sum_other, f"U, shift={shift}: coefficient 1 vs the constant solver ({smoother})"
        assert got["history"] == other["history"], smoother
        for key in ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm"):
            assert got[key] == other[key], (smoother, key)


def test_vc_cycle_at_the_nt_size(mg, oracle):
    """One V(1,1) cycle at N = 4096 on the `exp` coefficient, sigma = 1e4, against _solve_vc_ref.cycle (the one slow case of
    the module: about 8 s of numpy)."""
    N, shift = 4096, 1e4
    F, U0 = ref.random_problem(N, SEED_VC_CYCLE)
    a = vref.field("exp", N)
    opts = dict(pre=1, post=1, shift=shift)
    levels = vref.coarsen_levels(a, 8, lib_table(mg))
    margins = []
    want = vref.cycle(oracle, levels, F, U0, 1.0, margins=margins, **opts)
    ref.assert_qualified(margins, f"N={N} a=exp shift={shift:g}")
    hist = [vref.residual_norm(N, 1.0, a, U, F, shift) for U in (U0, want)]
    got, info = mg.solve(F, U0, coef=a, rtol=0.0, max_cycles=1, **opts)
    assert info["cycles"] == 1 and not info["converged"] and not info["coarse_capped"]
    assert_bits(got, want, f"N={N} a=exp shift={shift:g}: U after one cycle")
    np.testing.assert_allclose(info["history"], hist, rtol=1e-12, atol=0)


@pytest.mark.parametrize("N", [1026, 2048])
def test_vc_several_pair_form_levels(mg, oracle, N):
    """Cycles 1 to 3 of V(1,1) on the smooth coefficient, bit for bit: 1026 -> 513 -> 256 (pair form, then odd, then one
    column per lane), 2048 -> 1024 -> 512 -> 256 (three pair-form levels, the lower two from a zero start)."""
    assert [n for n in ref.sizes(N, 8) if n % 2 == 0 and n >= 512] == ([1026] if N == 1026 else [2048, 1024, 512])
    F, U0 = ref.random_problem(N, SEED_VC_LEVELS[N])
    _against_restatement(mg, oracle, N, vref.field("smooth", N), F, U0, f"N={N} a=smooth V(1,1)", max_cycles=3, pre=1, post=1)
