"""The batched variable-coefficient solver (include/mg_varcoef_batch.h) on the GPU.  The contract is bit identity with code
that is tested on its own (tests/test_solve_vc_gpu.py holds Solver(coef=a) against the numpy restatement): instance i of a
BatchSolver with coefficients equals Solver(coef=a_i) on F_i, U_i alone -- U, history, cycles and flags, compared with ==.
Sizes are the smallest at which each kernel form runs: one column per lane for odd or small N, column pairs from even
N = 512 on, non-temporal loads from N = 4096 on."""
import numpy as np
import pytest

import _guard
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
KEYS = ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm")
FIELDS = ("smooth", "exp", "random")   # contrast 3, 33.6 (a smooth field of contrast 34) and 1e3 from point to point


def problems(N, seed, names=FIELDS):
    """per instance: coefficient, F, U0 with its own random rim"""
    As = [vref.field(name, N, seed=seed + i) for i, name in enumerate(names)]
    FU = [ref.random_problem(N, seed + i) for i in range(len(names))]
    return As, [f for f, _ in FU], [u for _, u in FU]


def singles(mg, N, As, Fs, Us, **opts):
    """[(U, info)] of Solver(coef=a_i).solve(F_i, U_i): the reference of every comparison below"""
    out = []
    for a, F, U in zip(As, Fs, Us):
        s = mg.Solver(N, 1.0, coef=a, **opts)
        out.append(s.solve(F, U))
        s.close()
    return out


def assert_same(got_U, got, want_U, want, what):
    assert_bits(got_U, want_U, f"{what}: U")
    assert got["history"] == want["history"], what
    assert len(got["history"]) == got["cycles"] + 1
    for key in KEYS:
        assert got[key] == want[key], (what, key, got[key], want[key])


def assert_batch(Ub, infos, want, what):
    assert len(infos) == len(want)
    for i, (U, info) in enumerate(want):
        assert_same(Ub[i], infos[i], U, info, f"{what}, instance {i}")


# ---------------------------------------------------------------- 1. an instance is its single solve
@pytest.mark.parametrize("pp", [(3, 3), (2, 1)])     # (the result ends in the solver's field / in the caller's U)
@pytest.mark.parametrize("shift", [0.0, 1e4])
@pytest.mark.parametrize("N", [33, 100, 257, 512])
def test_instance_equals_single_solve(mg, N, shift, pp):
    As, Fs, Us = problems(N, 100 + N)
    opts = dict(pre=pp[0], post=pp[1], shift=shift, rtol=1e-9)
    want = singles(mg, N, As, Fs, Us, **opts)
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    b.set_coefficient(np.stack(As))
    assert b.has_coefficient and b.n_coefficients == 3
    Ub, infos = b.solve(np.stack(Fs), np.stack(Us))
    assert_batch(Ub, infos, want, f"N={N} shift={shift} {pp}")
    # the same instances in reverse order: where an instance sits in the batch does not matter
    b.set_coefficient(As[::-1])
    Ur, infos_r = b.solve(np.stack(Fs[::-1]), np.stack(Us[::-1]))
    b.close()
    assert_batch(Ur, infos_r, want[::-1], f"N={N} shift={shift} {pp} reversed")
    print(f"N={N} shift={shift} {pp}: cycles {[i['cycles'] for i in infos]}, launches {infos[0]['stats']['launches']}")


# ---------------------------------------------------------------- 2. one coefficient shared by every instance
@pytest.mark.parametrize("N", [100, 512])
def test_shared_coefficient(mg, N):
    a = vref.field("exp", N)
    _, Fs, Us = problems(N, 200 + N, names=("exp",) * 4)
    opts = dict(rtol=1e-9, shift=3.0)
    want = singles(mg, N, [a] * 4, Fs, Us, **opts)
    b = mg.BatchSolver(N, 1.0, max_batch=4, **opts)
    b.set_coefficient(a)
    assert b.has_coefficient and b.n_coefficients == 1
    Ub, infos = b.solve(np.stack(Fs), np.stack(Us))
    assert_batch(Ub, infos, want, f"N={N} shared")
    b.set_coefficient([a, a, a, a])
    assert b.n_coefficients == 4
    Up, infos_p = b.solve(np.stack(Fs), np.stack(Us))
    b.close()
    assert_batch(Up, infos_p, want, f"N={N} four copies")
    # the one-shot function, both ways
    Uo, infos_o = mg.solve_batched_coef(np.stack(Fs), a, np.stack(Us), 1.0, **opts)
    assert_batch(Uo, infos_o, want, f"N={N} solve_batched_coef shared")
    Uo, infos_o = mg.solve_batched_coef(np.stack(Fs), np.stack([a] * 4), np.stack(Us), 1.0, **opts)
    assert_batch(Uo, infos_o, want, f"N={N} solve_batched_coef per instance")


# ---------------------------------------------------------------- 3. a == 1 is the batch solver without a coefficient
@pytest.mark.parametrize("shift", [0.0, 10.0])
@pytest.mark.parametrize("N", [100, 512])
def test_unit_coefficient_is_the_constant_batch_solver(mg, N, shift):
    _, Fs, Us = problems(N, 300 + N)
    F, U0 = np.stack(Fs), np.stack(Us)
    b = mg.BatchSolver(N, 1.0, max_batch=3, shift=shift, rtol=1e-9)
    want_U, want = b.solve(F, U0)
    one = np.ones((N, N))
    for mode, coef in (("shared", one), ("per instance", np.stack([one] * 3))):
        b.set_coefficient(coef)
        got_U, got = b.solve(F, U0)
        for i in range(3):
            assert_same(got_U[i], got[i], want_U[i], want[i], f"N={N} shift={shift} a == 1 {mode}, instance {i}")
    b.close()


# ---------------------------------------------------------------- 4. instances leave the active set at different cycles
def test_active_set(mg):
    N = 129
    opts = dict(rtol=1e-9, atol=1e-20)
    As, Fs, Us = problems(N, 500 + N, names=("smooth", "smooth", "exp"))
    # instances 1 and 2 share ref.random_problem(N, 500 + N) and differ in the coefficient alone: 14 and 15 cycles on the
    # restatement (tests/test_solve_vc_cpu.py: CYCLES)
    Fs[1], Us[1] = ref.random_problem(N, 500 + N)
    Fs[2], Us[2] = ref.random_problem(N, 500 + N)
    # instance 0: F = 0 and a zero rim; its interior is a pattern far below atol, so it meets the tolerance at the start
    Fs[0] = np.zeros((N, N))
    Us[0] = ref.rim_only(np.zeros((N, N)))
    Us[0][1:-1, 1:-1] = 1e-40 * (1.0 + np.random.default_rng(7).random((N - 2, N - 2)))
    want = singles(mg, N, As, Fs, Us, **opts)
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    b.set_coefficient(As)
    Ub, infos = b.solve(np.stack(Fs), np.stack(Us))
    b.close()
    cycles = [i["cycles"] for i in infos]
    print(f"cycles {cycles}")
    assert cycles[0] == 0 and infos[0]["converged"] and len(set(cycles)) >= 2 and len(set(cycles[1:])) >= 2, cycles
    assert_bits(Ub[0], Us[0], "the instance that met its tolerance at the start is untouched")
    assert_batch(Ub, infos, want, "active set")
    assert infos[0]["stats"]["cycles"] == max(cycles)


# ---------------------------------------------------------------- 5. launches do not depend on the batch size
def test_launch_count_is_independent_of_the_batch(mg):
    N = 65
    a = vref.field("exp", N)
    F, U0 = ref.random_problem(N, 600)
    stats = {}
    for B in (1, 16):
        b = mg.BatchSolver(N, 1.0, max_batch=B, rtol=1e-9)
        b.set_coefficient(np.stack([a] * B))
        _, infos = b.solve(np.stack([F] * B), np.stack([U0] * B))
        b.close()
        stats[B] = infos[0]["stats"]
        assert all(i["history"] == infos[0]["history"] for i in infos)
    assert stats[1]["launches"] == stats[16]["launches"] > 0 and stats[1]["cycles"] == stats[16]["cycles"] > 0
    # per cycle (nl - 1)*(pre + post + 3) + 1 launches, one copy (pre + post even) and 2 for the norm; 4 norms launches before
    nl = len(ref.sizes(N, 8))
    assert stats[1]["launches"] == 4 + stats[1]["cycles"] * ((nl - 1) * 9 + 1 + 1 + 2)


# ---------------------------------------------------------------- 6. the non-temporal forms, one cycle
def test_large_forms(mg):
    N = 4096
    opts = dict(rtol=0.0, max_cycles=1, shift=1e4)
    rng = np.random.default_rng(4096)
    F = rng.random((N, N)) - 0.5
    Us = [rng.random((N, N)) - 0.5 for _ in range(2)]
    As = [vref.field("smooth", N), vref.field("exp", N)]
    Fd = mg.DeviceGrid.from_host(F)
    Ad = [mg.DeviceGrid.from_host(a) for a in As]
    want = []
    for a, U in zip(Ad, Us):
        s = mg.Solver(N, 1.0, coef=a, **opts)
        Ud = mg.DeviceGrid.from_host(U)
        _, info = s.solve(Fd, Ud)
        want.append((Ud.to_host(), info))
        Ud.free()
        s.close()
    b = mg.BatchSolver(N, 1.0, max_batch=2, **opts)
    b.set_coefficient(Ad)
    Ud = [mg.DeviceGrid.from_host(U) for U in Us]
    _, infos = b.solve([Fd, Fd], Ud)
    b.close()
    assert [i["cycles"] for i in infos] == [1, 1]
    assert_batch([u.to_host() for u in Ud], infos, want, "N=4096")
    for g in [Fd] + Ad + Ud:
        g.free()


# ---------------------------------------------------------------- 7. set, replace, remove
def test_set_replace_remove(mg):
    N = 100
    opts = dict(rtol=0.0, max_cycles=2)
    As, Fs, Us = problems(N, 700)
    Bs = [vref.field("exp", N), vref.field("smooth", N, L=2.0), vref.field("random", N, seed=9)]
    F, U0 = np.stack(Fs), np.stack(Us)
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    assert not b.has_coefficient and b.n_coefficients == 0
    plain_U, plain = b.solve(F, U0)
    grids = [mg.DeviceGrid.from_host(a) for a in As]
    b.set_coefficient(grids)
    for g in grids:
        g.free()                                  # the caller's arrays may be freed after the call
    junk = [mg.DeviceGrid.from_host(np.full((N, N), -7.0)) for _ in As]   # (likely the same blocks, recycled)
    assert b.has_coefficient and b.n_coefficients == 3
    U1, infos1 = b.solve(F, U0)
    for g in junk:
        g.free()
    assert_batch(U1, infos1, singles(mg, N, As, Fs, Us, **opts), "first coefficients")
    b.set_coefficient(np.stack(Bs))
    assert b.has_coefficient and b.n_coefficients == 3
    U2, infos2 = b.solve(F, U0)
    assert_batch(U2, infos2, singles(mg, N, Bs, Fs, Us, **opts), "replaced coefficients")
    b.set_coefficient(Bs[1])                      # per instance -> shared
    assert b.has_coefficient and b.n_coefficients == 1
    U3, infos3 = b.solve(F, U0)
    assert_batch(U3, infos3, singles(mg, N, [Bs[1]] * 3, Fs, Us, **opts), "shared after per instance")
    b.set_coefficient(None)
    assert not b.has_coefficient and b.n_coefficients == 0
    back_U, back = b.solve(F, U0)
    b.close()
    for i in range(3):
        assert_same(back_U[i], back[i], plain_U[i], plain[i], f"set_coefficient(None), instance {i}")
    assert back[0]["stats"]["launches"] == plain[0]["stats"]["launches"]


def test_storage_grows_with_the_number_of_coefficients(mg):
    """shared first (one copy stored), then per instance: the level storage is replaced by a larger one"""
    N = 65
    opts = dict(rtol=0.0, max_cycles=2)
    As, Fs, Us = problems(N, 750)
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    b.set_coefficient(As[0])
    U1, infos1 = b.solve(np.stack(Fs), np.stack(Us))
    assert_batch(U1, infos1, singles(mg, N, [As[0]] * 3, Fs, Us, **opts), "shared")
    b.set_coefficient(As)
    U2, infos2 = b.solve(np.stack(Fs), np.stack(Us))
    # fewer instances than coefficients: instance i still uses coefficient i
    U3, infos3 = b.solve(np.stack(Fs[:2]), np.stack(Us[:2]))
    b.close()
    want = singles(mg, N, As, Fs, Us, **opts)
    assert_batch(U2, infos2, want, "per instance after shared")
    assert_batch(U3, infos3, want[:2], "two instances on three coefficients")


# ---------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_solver_as_it_was(mg):
    N = 64
    opts = dict(rtol=0.0, max_cycles=2)
    As, Fs, Us = problems(N, 800)
    F, U0 = np.stack(Fs), np.stack(Us)
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)

    def unchanged(want_U, want, n_coef, what):
        assert b.n_coefficients == n_coef, what
        got_U, got = b.solve(F, U0)
        for i in range(3):
            assert_same(got_U[i], got[i], want_U[i], want[i], f"after {what}, instance {i}")

    def refusals(want_U, want, n_coef):
        for bad in (np.ones((N, N + 1)), np.ones((3, N - 1, N - 1)), [As[0], np.ones((N + 1, N + 1))], mg.DeviceGrid(32),
                    np.ones(N)):
            with pytest.raises(mg.MGError, match=r"\[2\].*shape"):
                b.set_coefficient(bad)
            unchanged(want_U, want, n_coef, "a wrong shape")
        with pytest.raises(mg.MGError, match=r"\[2\].*max_batch"):
            b.set_coefficient(np.stack([As[0]] * 4))
        unchanged(want_U, want, n_coef, "n > max_batch")
        for value in (0.0, -1.0, float("nan"), float("inf")):
            bad = [a.copy() for a in As]
            bad[1][N - 1, 3] = value               # (a rim point: the rim is part of the coefficient)
            with pytest.raises(mg.MGError, match=r"\[2\].*instance 1"):
                b.set_coefficient(bad)
            unchanged(want_U, want, n_coef, f"the value {value}")

    plain = b.solve(F, U0)
    refusals(*plain, 0)                            # without a coefficient: the constant solver stays
    b.set_coefficient(As)
    with_a = b.solve(F, U0)
    refusals(*with_a, 3)                           # with coefficients: they stay in place
    # more instances than coefficients
    b.set_coefficient(As[:2])
    assert b.n_coefficients == 2
    two_U, two = b.solve(F[:2], U0[:2])
    with pytest.raises(mg.MGError, match=r"\[2\].*3 instances.*2 coefficients"):
        b.solve(F, U0)
    again_U, again = b.solve(F[:2], U0[:2])
    for i in range(2):
        assert_same(again_U[i], again[i], two_U[i], two[i], f"after a refused solve, instance {i}")
        assert_same(again_U[i], again[i], with_a[0][i], with_a[1][i], f"two coefficients, instance {i}")
    b.close()
    lib = mg.lib()
    assert lib.mg_batch_solver_set_coefficient(None, 0, None) == 2 and lib.mg_batch_solver_has_coefficient(None) == 0
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg._check()


# ---------------------------------------------------------------- 9. memory contract
@pytest.mark.parametrize("placement", _guard.PLACEMENTS)
@pytest.mark.parametrize("N", [33, 512])
def test_memory_contract(mg, N, placement):
    """instances 0 and 1 run cycles, instance 2 (F = 0, an interior far below atol) meets its tolerance at the start"""
    opts = dict(rtol=0.0, atol=1e-20, max_cycles=2)
    As, Fs, Us = problems(N, 900 + N)
    Fs[2] = np.zeros((N, N))
    Us[2] = np.zeros((N, N))
    Us[2][1:-1, 1:-1] = 1e-40 * (1.0 + np.random.default_rng(N).random((N - 2, N - 2)))
    want = singles(mg, N, As, Fs, Us, **opts)
    with _guard.block(mg, [N] * 9, placement) as gb:
        ga, gF, gU = gb.views[0:3], gb.views[3:6], gb.views[6:9]
        for views, arrays in ((ga, As), (gF, Fs), (gU, Us)):
            for v, x in zip(views, arrays):
                v.upload(x)
        b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
        gb.expect_readonly(*gb.views)
        b.set_coefficient(ga)
        gb.check(f"set_coefficient N={N} {placement}")
        gb.expect_readonly(*ga, *gF, gU[2])
        infos = b.solve_ptrs([v.ptr for v in gF], [v.ptr for v in gU])
        gb.check(f"solve N={N} {placement}")
        b.close()
        assert [i["cycles"] for i in infos] == [2, 2, 0]
        assert_batch([v.to_host() for v in gU], infos, want, f"N={N} {placement}")
        assert_bits(gU[2].to_host(), Us[2], "the U of the instance that converged at the start")


# ---------------------------------------------------------------- 10. the smoother setting does not matter
def test_simple_smoother_setting_gives_the_same_bits(mg):
    N = 100
    opts = dict(rtol=0.0, max_cycles=3, shift=2.0)
    As, Fs, Us = problems(N, 1000)
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    b.set_coefficient(As)
    want_U, want = b.solve(np.stack(Fs), np.stack(Us))
    mg.set_smoother("simple")
    try:
        got_U, got = b.solve(np.stack(Fs), np.stack(Us))
    finally:
        mg.set_smoother("stream")
    b.close()
    for i in range(3):
        assert_same(got_U[i], got[i], want_U[i], want[i], f"MG_SMOOTHER=simple, instance {i}")
        assert got[i]["stats"]["launches"] == want[i]["stats"]["launches"]
