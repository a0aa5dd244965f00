"""The two-column (PAIR) and non-temporal (NT) forms of the kernel files added after tests/test_large_forms_gpu.py was
written -- the full-multigrid start, the Krylov acceleration and its batched form, the batched variable-coefficient solve,
the variable-coefficient heat right-hand side, the adjoint contractions and the eigen-solver -- at the sizes that select
them.  The thresholds are constexpr in every one of these files (PAIR_MIN_N = 512, NT_MIN_N = 4096), so the forms run at
real sizes only.  `pair` is "N even and N >= 512", `nt` is "pair and N >= 4096"; N % 4 == 2 (514, 1026, 4098) has rows that
are 16-byte but not 32-byte aligned, a last block of one lane and, in a hierarchy, an even level above an odd one
(514 -> 257, 1026 -> 513 -> 256).

Which test launches which instantiation; read off the launchers at the bottom of each file.  fmg = test_solve_fmg_gpu,
kry = test_solve_krylov_gpu, kryb = test_solve_krylov_batched_gpu, vcb = test_solve_vc_batched_gpu, hvc = test_heat_vc_gpu,
adj = test_adjoint_gpu, adjL = test_adjoint_large_forms_gpu, eig = test_eigs_gpu, here = this module.

mg_fmg_kernels.hip -- prolong_cubic (pair, nt of N_dst; inside the pair form `vec` = N_src even: 16-byte window loads, the
window's first column rounded down to even; N_src odd: scalar window loads from the unrounded first column)
  k_prolong_cubic<false, false>        N_dst not pair                fmg::test_prolong_cubic_bit_identical_to_numpy (6 ... 257, 1025)
  k_prolong_cubic<true, false>, vec    pair, not nt, N_src even      the same (512 -> 1024); fmg::test_prolong_cubic_inside_guard_bands
                                                                     (512 -> 1024, 1024 -> 2048)
  k_prolong_cubic<true, false>, scalar pair, not nt, N_src odd       here::test_prolong_cubic_from_an_odd_source (257 -> 514, 513 -> 1026),
                                                                     test_prolong_cubic_from_an_odd_source_inside_guard_bands;
                                                                     in a solve: here::test_fmg_solves_with_an_odd_level_below_an_even_one
  k_prolong_cubic<true, true>, vec     nt, N_src even                fmg::test_prolong_cubic_bit_identical_to_numpy (4096 -> 8192);
                                                                     here::test_prolong_cubic_non_temporal_from_an_even_source (2048 -> 4096)
  k_prolong_cubic<true, true>, scalar  nt, N_src odd                 here::test_prolong_cubic_from_an_odd_source (2049 -> 4098)
  k_rim_extract, k_rim_sample, k_rim_only, k_rim_write, k_flag_or    every solve with fmg >= 1, no forms (fmg::test_sizes_fmg_shifts_...,
                                                                     here::test_fmg_solves_with_an_odd_level_below_an_even_one)

mg_krylov_kernels.hip -- krylov_dots, krylov_orth (bucket K = k, the number of stored directions), krylov_update
  k_krylov_dots<K, false>, k_krylov_orth<K, false>   not pair        kry::test_dots_and_orthogonalisation_alone (3 ... 511, 513)
  k_krylov_dots<K, true>, k_krylov_orth<K, true>     pair            the same (512, 1024, 1026)
  k_krylov_update<false>, <true>                     not pair, pair  kry::test_update_alone (the same sizes)
  k_krylov_*_finish, k_krylov_log_restart            no forms        kry::test_whole_solves_replayed_from_the_log
  The 16 buckets K = 0 .. 15 are one family: one body, `#pragma unroll` over j < K, the pointers of the stored directions
  indexed by constants.  The kernel tests run k = 0 (nothing stored: no dots launch, an orthogonalisation that stores
  nothing), 1, 2 (the first loop bodies), 7 and 15 (the largest bucket: every pointer of KrylovVecs); whole solves with
  m = 8 run every k from 0 to 7 in order.  A bucket can differ from its neighbours only in the trip count, and both ends and
  the middle of the range are run in both forms.

mg_krylov_batch_kernels.hip -- the batched forms (bucket K = the largest k of the active set, a block's own k <= K)
  k_krylov_dots_b<K, false>, k_krylov_orth_b<K, false>, k_krylov_update_b<false>   not pair
                                                                     kryb::test_instance_equals_single_solve (33 ... 257; m = 8: K = 0 .. 7)
  k_krylov_dots_b<K, true>, k_krylov_orth_b<K, true>, k_krylov_update_b<true>      pair
                                                                     the same (512); here::test_batched_krylov_at_the_quarter_sizes (514, 1026)
  a block's k below its launch's K                   not pair        kryb::test_diverging_k (33 or 65)
                                                     pair            here::test_diverging_k_at_a_pair_size (512)
  k_krylov_dots_finish_b, k_krylov_orth_finish_b, k_krylov_update_finish_b, k_krylov_log_restart_b, k_krylov_zero_b
                                                     no forms        every batched solve above (k_krylov_zero_b with an odd count: odd N)

mg_varcoef_batch_kernels.hip -- wjacobi_vc_batch, residual_vc_batch, apply_vc_batch, resnorm_vc_batch
  k_wjacobi_vc_b<false, false, false>  not pair, U_in given          vcb::test_instance_equals_single_solve (33, 100, 257)
  k_wjacobi_vc_b<true, false, false>   not pair, zero start          the same (every level below the top)
  k_wjacobi_vc_b<false, true, false>   pair, not nt, U_in given      the same (512: the top level); here::test_batched_coefficients_at_514
  k_wjacobi_vc_b<true, true, false>    pair, not nt, zero start      vcb::test_large_forms (2048, 1024, 512 below 4096)
  k_wjacobi_vc_b<false, true, true>    nt, U_in given                vcb::test_large_forms (4096: the top level)
  k_wjacobi_vc_b<true, true, true>     nt, zero start                here::test_batched_zero_start_sweep_at_the_nt_form (4096 below 8192)
  k_residual_vc_b<false>, <true>       not pair, pair                vcb::test_instance_equals_single_solve (33 ... 257; 512),
                                                                     here::test_batched_coefficients_at_514
  k_apply_vc_b (column form only)      a given / NULL per instance   kryb::test_instance_equals_single_solve; every eigen-solve (eig, here)
  k_resnorm_vc_b<false, false>         not pair                      vcb::test_instance_equals_single_solve (33, 100, 257)
  k_resnorm_vc_b<true, false>          pair, not nt                  the same (512); here::test_batched_coefficients_at_514
  k_resnorm_vc_b<true, true>           nt                            vcb::test_large_forms (4096)
  k_resnorm_finish_vc_b, k_gs_relative_vc_b, k_coef_coarsen_b, k_coef_check_b      no forms: every test above

mg_heat_vc_kernels.hip -- heat_rhs_vc (theta != 1)
  k_heat_rhs_vc<false, false>          not pair                      hvc::test_kernel_bit_identical_to_restatement_inside_guard_bands (3 ... 511)
  k_heat_rhs_vc<true, false>           pair, not nt                  the same (512, 514, 1026)
  k_heat_rhs_vc<true, true>            nt                            hvc::test_kernel_non_temporal_form (4096, 4098)

mg_adjoint_kernels.hip -- coef_grad, coef_grad_batch, rim_grad, rim_grad_batch
  k_coef_grad<false, false>            not pair                      adj::test_point_kernels_bit_identical_to_restatement (3 ... 130, 513)
  k_coef_grad<true, false>             pair, not nt                  the same (512, 514)
  k_coef_grad<true, true>              nt                            adjL::test_point_kernels_non_temporal_form (4096)
  k_coef_grad_b<false, false>          not pair                      adj::test_batched_twins_equal_the_single_launches (33)
  k_coef_grad_b<true, false>           pair, not nt                  the same (512); here::test_batched_coefficient_gradient (514)
  k_coef_grad_b<true, true>            nt                            here::test_batched_coefficient_gradient (4096)
  k_rim_grad, k_rim_grad_b             column form only              adj::test_point_kernels_..., test_batched_twins_... (33, 512)

mg_eigs_kernels.hip -- eigs_gram, eigs_rotate (bucket M >= the basis size m; the pair form up to M = 12), eigs_resnorm
  k_eig_gram<false>                    not pair                      eig::test_gram_alone (5 ... 129), ..._at_the_sixteen_byte_form (513)
  k_eig_gram<true>                     pair                          eig::test_gram_alone_at_the_sixteen_byte_form (512, 514); in a solve:
                                                                     here::test_eigen_solves_in_the_sixteen_byte_forms
  k_eig_rotate<3 | 6 | 12, false>      not pair, m <= 3 | 6 | 12     eig::test_rotate_alone (m = 1, 2, 3; 12), ..._sixteen_byte_form (513: m = 6)
  k_eig_rotate<18 | 24 | 36, false>    m <= 18 | 24 | 36, any N      eig::test_rotate_alone (m = 13, 24, 36), ..._sixteen_byte_form (514: m = 13;
                                                                     512: m = 36); at a pair size in a solve: here (p = 6, 8, 12)
  k_eig_rotate<3, true>                pair, m <= 3                  eig::test_rotate_alone_at_the_sixteen_byte_form (512: m = 3)
  k_eig_rotate<6, true>                pair, 3 < m <= 6              here::test_rotate_alone_in_the_pair_form (512: m = 6); solves with p = 3, 6
  k_eig_rotate<12, true>               pair, 6 < m <= 12             eig::test_rotate_alone_at_the_sixteen_byte_form (512: m = 12);
                                                                     here::test_rotate_alone_in_the_pair_form (514: m = 9)
  k_eig_resnorm<false>                 not pair                      every whole solve of eig (N <= 65); here (513)
  k_eig_resnorm<true>                  pair                          here::test_eigen_solves_in_the_sixteen_byte_forms (512, 514, 1026: res
                                                                     against longdouble), test_a_converged_start_at_512_returns_at_once
  k_eig_finish, k_eig_start            no forms                      every launch above; k_eig_start with a source: the converged start

Eigen-solves: the reference is _eigs_ref.separated_eigenvalues, exact for a coefficient constant along one axis, which
shares no code with the engine or its restatement; the assertions are test_eigs_gpu.check_solution's.  Iterations of the
numpy restatement on the CPU (seed 3), every one at most half of max_iters = 60: N = 512 -- (1, 2): 11, 11, 12, 16, 16 over
_newer_forms_cases.EIG_FIELDS; (4, 2): 17, 18, 19, 17, 17; (8, 4): 16, 17, 16, 18, 18.  N = 514 -- (1, 2): 11, 12, 13, 16, 17;
(4, 4): 14, 16, 15, 16, 15.  N = 513 -- (4, 2): 17, 18, 17, 18, 18.  N = 1026 jump / cols (1, 2): 18.  The MI355X took
the same counts in all 31 cases; the test prints them and asserts at most 30.
Measured on the MI355X: max |lam - ref| between 2.2e-11 and 6.7e-10 against ||R||_F + rounding_term >= 2.4e-4 (the rounding
term dominates: 2.4e-4 ... 2.5e-3 at 512 to 514, 3.9e-2 at 1026; against the closed form of `one`: at most 4.6e-13);
|res - longdouble res| at most 3.3e-12 at every size against bounds from 3.1e-9 (512 to 514) and 1.3e-7 (1026);
|X^T X - I| at most 9.1e-15 against 1.2e-10.
Whole cycles of a numpy restatement are compared at 514 and 1026 only, every coarse solve qualified (margin >= 1e-10,
DESIGN 4.3) with seeds chosen on the restatement alone; above 1026 the tests are kernel launches and device-to-device
comparisons."""
import numpy as np
import pytest

import _eigs_ref as er
import _guard
import _newer_forms_cases as cases
import _solve_ref as ref
import _solve_vc_ref as vref
import test_adjoint_gpu as adj
import test_eigs_gpu as eig
import test_solve_fmg_gpu as fmg
import test_solve_krylov_batched_gpu as kryb
import test_solve_vc_batched_gpu as vcb
from conftest import assert_bits
from test_large_forms_gpu import same_field

pytestmark = pytest.mark.gpu


# ================================================================ 1. the eigen-solver in the 16-byte forms
def references(name, N):
    refs = [er.separated_eigenvalues(name, N, 1.0, 13)]
    if name == "one":
        refs.append(er.closed_form(N, 1.0, 13))
    return refs


@pytest.mark.parametrize("N,name,axis,k,guard", cases.EIG_CASES)
def test_eigen_solves_in_the_sixteen_byte_forms(mg, N, name, axis, k, guard):
    """Whole solves at 512 (pair), 514 and 1026 (pair, N % 4 == 2, an odd level below) and 513 (odd above the threshold)
    against the separated reference, with every assertion of test_eigs_gpu.check_solution: the reported residuals within
    residual_rounding_bound of the longdouble ones (k_eig_resnorm<true>), orthonormality, Kahan's bound, the quadratic bound
    (its gap condition holds for every case: test_newer_forms_cpu.py)."""
    a = er.layered(name, N, axis)
    what = f"N={N} {name}/{axis} k={k} guard={guard}"
    with mg.EigenSolver(N, 1.0, k=k, guard=guard, coef=None if name == "one" else a, max_iters=cases.MAX_ITERS) as e:
        lam, X, info = e.solve(seed=3)
        hist = e.history()
    info["guard"] = guard
    print(f"{what}: iters {info['iters']} restarts {info['restarts']}")
    assert len(hist) == info["iters"] + 1
    assert info["converged"] and info["iters"] <= cases.MAX_ITERS // 2, (what, info)
    eig.check_solution(N, name, a, k, lam, X, info, what, refs=references(name, N))


@pytest.mark.parametrize("N,m,p", [(512, 6, 2), (514, 9, 3)])
def test_rotate_alone_in_the_pair_form(mg, N, m, p):
    """k_eig_rotate<6, true> and, on rows that are 16-byte aligned and no more, k_eig_rotate<12, true>: bit for bit"""
    eig.rotate_case(mg, N, m, p, placements=("odd16" if N % 4 == 2 else "page",))


def test_a_converged_start_at_512_returns_at_once(mg):
    """the second solve is the start, the Gram launch and k_eig_resnorm<true> alone: nothing is touched, the same bits"""
    N, k = 512, 4
    with mg.EigenSolver(N, 1.0, k=k, guard=2, coef=er.layered("smooth", N, "rows")) as e:
        lam, X, info = e.solve(seed=1)
        lam2, X2, info2 = e.solve(X0=X, seed=1)
    assert info["converged"] and info2["converged"]
    assert info2["iters"] == 0 and info2["cycles"] == 0, info2
    assert_bits(lam2, lam, "lam of the restart")
    assert_bits(X2, X, "X of the restart: returned untouched")
    assert_bits(info2["res"], info["res"], "res of the restart")


def test_one_seed_gives_identical_bits_at_514(mg):
    N, k = 514, 4
    with mg.EigenSolver(N, 1.0, k=k, guard=4, coef=er.layered("jump", N, "cols")) as e:
        lam0, X0, info0 = e.solve(seed=2)
        lam1, X1, info1 = e.solve(seed=2)
    assert info0["converged"] and info1["iters"] == info0["iters"]
    assert_bits(lam1, lam0, "lam twice")
    assert_bits(X1, X0, "X twice")
    assert_bits(info1["res"], info0["res"], "res twice")


# ================================================================ 2. cubic prolongation from an odd source
@pytest.mark.parametrize("N_src,N_dst", [(257, 514), (513, 1026), (2049, 4098)])
def test_prolong_cubic_from_an_odd_source(mg, N_src, N_dst):
    """the scalar window load of the pair form: bit for bit, the rim untouched, the source read only"""
    fmg.test_prolong_cubic_bit_identical_to_numpy(mg, N_src, N_dst)


def test_prolong_cubic_non_temporal_from_an_even_source(mg):
    fmg.test_prolong_cubic_bit_identical_to_numpy(mg, 2048, 4096)


@pytest.mark.parametrize("place", list(_guard.PLACEMENTS))
@pytest.mark.parametrize("N_src,N_dst", [(257, 514), (513, 1026)])
def test_prolong_cubic_from_an_odd_source_inside_guard_bands(mg, N_src, N_dst, place):
    fmg.test_prolong_cubic_inside_guard_bands(mg, N_src, N_dst, place)


@pytest.mark.parametrize("N,fmg_cycles,shift", cases.FMG_CASES)
def test_fmg_solves_with_an_odd_level_below_an_even_one(mg, oracle, N, fmg_cycles, shift):
    """514 -> 257 and 1026 -> 513: the pass and two cycles bit for bit against the restatement"""
    F, U0 = fmg.problem(N, 1.0, cases.SEED_FMG[N])
    fmg.against_restatement(mg, oracle, F, U0, 1.0, cases.FMG_CYCLES, f"N={N} fmg={fmg_cycles} shift={shift:g}", fmg=fmg_cycles,
                            shift=shift)


# ================================================================ 3. batched twins
def gradient_fields(N, seed):
    rng = np.random.default_rng(seed)
    lam, U = rng.standard_normal((N, N)), rng.standard_normal((N, N))
    lam[0, :] += 3.0      # (a rim that must not reach a result)
    lam[:, -1] -= 2.0
    return lam, U


@pytest.mark.parametrize("N,B", [(514, 3), (4096, 2)])
def test_batched_coefficient_gradient(mg, N, B):
    """k_coef_grad_b<true, false> on rows that are 16-byte aligned and no more, and k_coef_grad_b<true, true>: every instance
    of one launch is the single launch on its lam and U alone (the single kernel is held against numpy at 514 and 4096 by
    test_adjoint_gpu.py and test_adjoint_large_forms_gpu.py); the instances differ in both inputs, the outputs start as NaN"""
    L = 1.3
    sets = [gradient_fields(N, 70 + 11 * i + N) for i in range(B)]
    lam = [mg.DeviceGrid.from_host(s[0]) for s in sets]
    U = [mg.DeviceGrid.from_host(s[1]) for s in sets]
    gA = mg.coefficientGradient_batch(N, L, lam, U, [adj.poisoned(mg, N) for _ in range(B)])
    sums = set()
    for i in range(B):
        single = mg.coefficientGradient(N, L, lam[i], U[i], adj.poisoned(mg, N))
        same_field(gA[i], single, f"gA N={N} instance {i}: batched vs single launch")
        sums.add(gA[i].checksum())
        single.free()
    assert len(sums) == B, "the instances' gradients differ"
    for g in lam + U + list(gA):
        g.free()


@pytest.mark.parametrize("shift,pp", [(0.0, (3, 3)), (1e4, (2, 1))])
def test_batched_coefficients_at_514(mg, shift, pp):
    """BatchSolver with a coefficient per instance at N = 514 (514 -> 257 -> 128 ...): every instance is its single solve, in
    the given and in the reversed order"""
    N = 514
    As, Fs, Us = vcb.problems(N, 100 + N)
    opts = dict(pre=pp[0], post=pp[1], shift=shift, rtol=1e-9, max_cycles=12)
    want = vcb.singles(mg, N, As, Fs, Us, **opts)
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    b.set_coefficient(np.stack(As))
    Ub, infos = b.solve(np.stack(Fs), np.stack(Us))
    vcb.assert_batch(Ub, infos, want, f"N={N} shift={shift} {pp}")
    b.set_coefficient(As[::-1])
    Ur, infos_r = b.solve(np.stack(Fs[::-1]), np.stack(Us[::-1]))
    b.close()
    vcb.assert_batch(Ur, infos_r, want[::-1], f"N={N} shift={shift} {pp} reversed")
    assert all(i["cycles"] >= 1 for i in infos)


@pytest.mark.parametrize("N", [514, 1026])
def test_batched_krylov_at_the_quarter_sizes(mg, N):
    """set_krylov(4) at N % 4 == 2, a coefficient per instance: U, info, history and the whole log of every instance equal its
    single solve's, in the given and in the reversed order; at most 12 cycles"""
    m = 4
    Fs, Us = kryb.problems(N, 100 + N + m)
    names = ("smooth", "jump", "random")
    As = [kryb.coefficient(name, N, seed=7 + i) for i, name in enumerate(names)]
    opts = dict(rtol=1e-9, max_cycles=12)
    want = kryb.singles(mg, N, As, Fs, Us, m, **opts)
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    b.set_krylov(m)
    b.set_coefficient(np.stack(As))
    Ub, infos = b.solve(np.stack(Fs), np.stack(Us))
    kryb.assert_batch(b, Ub, infos, want, f"N={N} m={m} {names}")
    assert all(i["cycles"] >= 2 for i in infos)      # (dots and an orthogonalisation at k > 0)
    b.set_coefficient(As[::-1])
    Ur, infos_r = b.solve(np.stack(Fs[::-1]), np.stack(Us[::-1]))
    kryb.assert_batch(b, Ur, infos_r, want[::-1], f"N={N} m={m} {names} reversed")
    b.close()


def test_batched_zero_start_sweep_at_the_nt_form(mg):
    """k_wjacobi_vc_b<true, true, true> runs on a level of 4096 or more BELOW the top one: one V(1,1) cycle at N = 8192 (no
    smaller size selects it), one instance, against Solver(coef=a) by device checksums; no host arithmetic at this size
    beyond the inputs."""
    N = 8192
    assert ref.sizes(N, 8)[:2] == [8192, 4096]      # (the level below the top starts its pre-smoothing from zero)
    opts = dict(pre=1, post=1, rtol=0.0, max_cycles=1, shift=1e4)
    a = mg.DeviceGrid.from_host(vref.field("smooth", N))
    F = mg.DeviceGrid.from_host(np.random.default_rng(N).random((N, N)) - 0.5)
    Us, Ub = mg.DeviceGrid.zeros((N, N)), mg.DeviceGrid.zeros((N, N))
    s = mg.Solver(N, 1.0, coef=a, **opts)
    try:
        single = s.solve_ptr(F.ptr, Us.ptr)
    finally:
        s.close()
    b = mg.BatchSolver(N, 1.0, max_batch=1, **opts)
    try:
        b.set_coefficient([a])
        batch = b.solve_ptrs([F.ptr], [Ub.ptr])[0]
    finally:
        b.close()
    sums = Us.checksum(), Ub.checksum(), mg.DeviceGrid.zeros((N, N)).checksum()
    for g in (a, F, Us, Ub):
        g.free()
    assert single["cycles"] == batch["cycles"] == 1 and sums[0] != sums[2]
    assert sums[0] == sums[1], "U after one cycle: batch vs single solver"
    assert batch["history"] == single["history"] and batch["history"][1] < batch["history"][0]


# the candidates of the diverging-k case at a pair size: (N, field, m, rtol, max_cycles, the two seeds of F, U0) with rtol
# near the rounding floor of the recurred norm, as tests/test_solve_krylov_batched_cpu.py chooses them at 33 and 65
DIVERGING_PAIR = [(512, "smooth", 4, 1e-14, 30, (1, 2)), (512, "jump", 8, 1e-13, 30, (2, 3)), (512, "smooth", 4, 1e-14, 30, (2, 3))]


def test_diverging_k_at_a_pair_size(mg):
    """kryb::test_diverging_k at N = 512: the first candidate on which the two SINGLE solves sit at different k in one
    iteration (a condition on the single solver alone), then the batch [A, a zero problem, B] against the singles: blocks
    of one launch of k_krylov_dots_b<K, true> / k_krylov_orth_b<K, true> with their own k below K.  Measured on the MI355X:
    the first candidate diverges (seeds 1 and 2 sit at different k in iterations 18 to 21 and 24 to 27 of 30); on the numpy
    restatement the first two candidates do (iterations 21 ... 29 and 27 ... 29)."""
    chosen = None
    for N, name, m, rtol, max_cycles, seeds in DIVERGING_PAIR:
        a = kryb.coefficient(name, N)
        opts = dict(rtol=rtol, max_cycles=max_cycles)
        FU = [ref.random_problem(N, seed) for seed in seeds]
        want = [kryb.single(mg, N, a, F, U, m, **opts) for F, U in FU]
        ks = [[e["k"] for e in log] for _, _, log in want]
        differ = [i for i, (x, y) in enumerate(zip(*ks)) if x != y]
        print(f"N={N} {name} m={m} rtol={rtol:g}: the single solves sit at different k in iterations {differ}")
        if differ:
            chosen = (N, a, m, opts, FU, want)
            break
    assert chosen, "no candidate on which the single solves' k diverge"
    N, a, m, opts, FU, want = chosen
    zero = np.zeros((N, N))
    want = [want[0], kryb.single(mg, N, a, zero, zero, m, **opts), want[1]]
    assert want[1][1]["cycles"] == 0
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    b.set_coefficient(a)
    b.set_krylov(m)
    Ub, infos = b.solve(np.stack([FU[0][0], zero, FU[1][0]]), np.stack([FU[0][1], zero, FU[1][1]]))
    kryb.assert_batch(b, Ub, infos, want, "diverging k at a pair size")
    assert b.krylov_log(1) == []
    b.close()
