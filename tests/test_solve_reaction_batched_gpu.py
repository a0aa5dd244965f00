"""The batched solver with a reaction term (include/mg_rx_batch.h) on the GPU.  The contract is bit identity with code that is
tested on its own (tests/test_solve_reaction_gpu.py holds Solver(reaction=s) against the numpy restatement): instance i of a
BatchSolver with reactions equals Solver(reaction=s_i, coef=a_i) on F_i, U_i alone -- U, history, cycles and flags, compared
with ==.  Sizes are the smallest at which each kernel form runs: one column per lane for odd or small N (33, 100, 257: one and
two column blocks), column pairs from even N = 512 on, non-temporal loads from N = 4096 on."""
import ctypes as C

import numpy as np
import pytest

import _guard
import _reaction_ref as rref
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
KEYS = ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm")
COEFS = ("smooth", "exp", "random")


def problems(N, seed, n=3):
    FU = [ref.random_problem(N, seed + i) for i in range(n)]
    return [f for f, _ in FU], [u for _, u in FU]


def reactions(N, first=0, n=3):
    """n different fields of _reaction_ref.FIELDS, from FIELDS[first] on"""
    return [rref.field(rref.FIELDS[(first + i) % len(rref.FIELDS)], N) for i in range(n)]


def coefficients(N, seed, n=3):
    return [vref.field(COEFS[i % 3], N, seed=seed + i) for i in range(n)]


def single(mg, N, a, s, F, U, krylov=0, **opts):
    """(U, info, log) of Solver(reaction=s, coef=a, krylov=m).solve(F, U): the reference of every comparison below"""
    extra = dict(krylov=krylov) if krylov else {}
    if a is not None:
        extra["coef"] = a
    if s is not None:
        extra["reaction"] = s
    solver = mg.Solver(N, 1.0, **extra, **opts)
    out_U, info = solver.solve(F, U)
    log = solver.krylov_log() if krylov else None
    solver.close()
    return out_U, info, log


def singles(mg, N, As, Ss, Fs, Us, **opts):
    As = As if As is not None else [None] * len(Fs)
    return [single(mg, N, a, s, F, U, **opts) for a, s, F, U in zip(As, Ss, Fs, Us)]


def assert_same(got_U, got, want_U, want, what):
    assert_bits(got_U, want_U, f"{what}: U")
    assert got["history"] == want["history"], what
    assert len(got["history"]) == got["cycles"] + 1
    for key in KEYS:
        assert got[key] == want[key], (what, key, got[key], want[key])


def assert_batch(Ub, infos, want, what):
    assert len(infos) == len(want)
    for i, w in enumerate(want):
        assert_same(Ub[i], infos[i], w[0], w[1], f"{what}, instance {i}")


# ---------------------------------------------------------------- 1. an instance is its single solve
@pytest.mark.parametrize("with_a", [False, True])
@pytest.mark.parametrize("pp", [(3, 3), (2, 1)])     # (the result ends in the solver's field / in the caller's U)
@pytest.mark.parametrize("shift", [0.0, 1e4])
@pytest.mark.parametrize("N", [33, 100, 257, 512])
def test_instance_equals_single_solve(mg, N, shift, pp, with_a):
    Fs, Us = problems(N, 100 + N)
    Ss = reactions(N, first=N % 4)
    As = coefficients(N, 100 + N) if with_a else None
    opts = dict(pre=pp[0], post=pp[1], shift=shift, rtol=1e-9)
    want = singles(mg, N, As, Ss, Fs, Us, **opts)
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    if with_a:
        b.set_coefficient(np.stack(As))
    b.set_reaction(np.stack(Ss))
    assert b.has_reaction and b.n_reactions == 3 and b.n_coefficients == (3 if with_a else 0)
    Ub, infos = b.solve(np.stack(Fs), np.stack(Us))
    assert_batch(Ub, infos, want, f"N={N} shift={shift} {pp} a={with_a}")
    # the same instances in reverse order: where an instance sits in the batch does not matter
    b.set_reaction(Ss[::-1])
    if with_a:
        b.set_coefficient(As[::-1])
    Ur, infos_r = b.solve(np.stack(Fs[::-1]), np.stack(Us[::-1]))
    b.close()
    assert_batch(Ur, infos_r, want[::-1], f"N={N} shift={shift} {pp} a={with_a} reversed")
    print(f"N={N} shift={shift} {pp} a={with_a}: cycles {[i['cycles'] for i in infos]}, launches {infos[0]['stats']['launches']}")


# ---------------------------------------------------------------- 2. the counts of a and s are independent
@pytest.mark.parametrize("N", [100, 512])
def test_count_combinations(mg, N):
    n = 3
    Fs, Us = problems(N, 200 + N)
    F, U0 = np.stack(Fs), np.stack(Us)
    Ss, As = reactions(N, first=1), coefficients(N, 200 + N)
    opts = dict(rtol=1e-9, shift=3.0)
    b = mg.BatchSolver(N, 1.0, max_batch=n, **opts)
    for a_mode in ("none", "shared", "per instance"):
        a_of = {"none": [None] * n, "shared": [As[1]] * n, "per instance": As}[a_mode]
        b.set_coefficient({"none": None, "shared": As[1], "per instance": np.stack(As)}[a_mode])
        for s_mode in ("shared", "per instance"):
            s_of = [Ss[0]] * n if s_mode == "shared" else Ss
            want = singles(mg, N, a_of, s_of, Fs, Us, **opts)
            b.set_reaction(Ss[0] if s_mode == "shared" else Ss)
            assert b.n_reactions == (1 if s_mode == "shared" else n)
            assert b.n_coefficients == {"none": 0, "shared": 1, "per instance": n}[a_mode]
            Ub, infos = b.solve(F, U0)
            assert_batch(Ub, infos, want, f"N={N} a {a_mode}, s {s_mode}")
            if s_mode == "shared":   # the same bits as per-instance copies of one array
                b.set_reaction([Ss[0]] * n)
                assert b.n_reactions == n
                Uc, infos_c = b.solve(F, U0)
                assert_batch(Uc, infos_c, want, f"N={N} a {a_mode}, s three copies")
    b.close()
    # the one-shot function
    want = singles(mg, N, As, [Ss[0]] * n, Fs, Us, **opts)
    Uo, infos_o = mg.solve_batched_reaction(F, Ss[0], U0, 1.0, coef=np.stack(As), **opts)
    assert_batch(Uo, infos_o, want, f"N={N} solve_batched_reaction")


# ---------------------------------------------------------------- 3. the two identities
@pytest.mark.parametrize("with_a", [False, True])
@pytest.mark.parametrize("N", [100, 512])
def test_zero_reaction_is_the_batch_solver_without_one(mg, N, with_a):
    Fs, Us = problems(N, 300 + N)
    F, U0 = np.stack(Fs), np.stack(Us)
    b = mg.BatchSolver(N, 1.0, max_batch=3, shift=10.0, rtol=1e-9)
    if with_a:
        b.set_coefficient(coefficients(N, 300 + N))
    want_U, want = b.solve(F, U0)
    zero = np.zeros((N, N))
    for mode, s in (("shared", zero), ("per instance", np.stack([zero] * 3))):
        b.set_reaction(s)
        got_U, got = b.solve(F, U0)
        for i in range(3):
            assert_same(got_U[i], got[i], want_U[i], want[i], f"N={N} a={with_a} s == 0 {mode}, instance {i}")
    b.close()


@pytest.mark.parametrize("with_a", [False, True])
@pytest.mark.parametrize("N", [100, 512])
def test_constant_reaction_is_the_shift(mg, N, with_a):
    c = 1234.5
    Fs, Us = problems(N, 350 + N)
    F, U0 = np.stack(Fs), np.stack(Us)
    As = coefficients(N, 350 + N)
    b = mg.BatchSolver(N, 1.0, max_batch=3, shift=c, rtol=1e-9)
    if with_a:
        b.set_coefficient(As)
    want_U, want = b.solve(F, U0)
    b.close()
    b = mg.BatchSolver(N, 1.0, max_batch=3, shift=0.0, rtol=1e-9)
    if with_a:
        b.set_coefficient(As)
    b.set_reaction(np.full((N, N), c))
    got_U, got = b.solve(F, U0)
    b.close()
    for i in range(3):
        assert_same(got_U[i], got[i], want_U[i], want[i], f"N={N} a={with_a} s == c, instance {i}")


# ---------------------------------------------------------------- 4. instances leave the active set at different cycles
def test_active_set(mg):
    N = 129
    opts = dict(rtol=1e-9, atol=1e-20)
    Fs, Us = problems(N, 500 + N, n=3)
    Fs[2], Us[2] = Fs[1].copy(), Us[1].copy()      # instances 1 and 2 differ in the reaction alone: 0 and 1e6*blob
    Ss = [np.zeros((N, N)), np.zeros((N, N)), rref.field("blob", N)]
    # instance 0: F = 0 and a zero rim; its interior is a pattern far below atol, so it meets the tolerance at the start
    Fs[0] = np.zeros((N, N))
    Us[0] = ref.rim_only(np.zeros((N, N)))
    Us[0][1:-1, 1:-1] = 1e-40 * (1.0 + np.random.default_rng(7).random((N - 2, N - 2)))
    want = singles(mg, N, None, Ss, Fs, Us, **opts)
    single_cycles = [w[1]["cycles"] for w in want]
    assert single_cycles[0] == 0 and len(set(single_cycles[1:])) == 2, single_cycles   # (from the single solves)
    b = mg.BatchSolver(N, 1.0, max_batch=4, **opts)
    b.set_reaction(Ss)
    gF = [mg.DeviceGrid.from_host(F) for F in Fs]
    gU = [mg.DeviceGrid.from_host(U) for U in Us]
    sentinel = np.full((N, N), -12345.678)
    gS = mg.DeviceGrid.from_host(sentinel)         # a fourth U, beyond the three instances of the solve
    infos = b.solve_ptrs([g.ptr for g in gF], [g.ptr for g in gU])
    b.close()
    Ub = [g.to_host() for g in gU]
    cycles = [i["cycles"] for i in infos]
    print(f"cycles {cycles}")
    assert cycles == single_cycles
    assert_bits(Ub[0], Us[0], "the instance that met its tolerance at the start is untouched")
    assert_bits(gS.to_host(), sentinel, "a U beyond the solved count is untouched")
    assert_batch(Ub, infos, want, "active set")
    assert infos[0]["stats"]["cycles"] == max(cycles)
    for g in gF + gU + [gS]:
        g.free()


# ---------------------------------------------------------------- 5. launches do not depend on the batch size
@pytest.mark.parametrize("pp", [(3, 3), (2, 1)])
def test_launch_count_is_independent_of_the_batch(mg, pp):
    N = 65
    s = rref.field("smooth", N)
    F, U0 = ref.random_problem(N, 600)
    stats = {}
    for B in (1, 16):
        b = mg.BatchSolver(N, 1.0, max_batch=B, rtol=1e-9, pre=pp[0], post=pp[1])
        b.set_reaction(np.stack([s] * B))
        _, infos = b.solve(np.stack([F] * B), np.stack([U0] * B))
        b.close()
        stats[B] = infos[0]["stats"]
        assert all(i["history"] == infos[0]["history"] for i in infos)
    assert stats[1]["launches"] == stats[16]["launches"] > 0 and stats[1]["cycles"] == stats[16]["cycles"] > 0
    # per cycle (nl - 1)*(pre + post + 3) + 1 launches, one copy when pre + post is even, and 2 for the norm; 4 norm launches
    # before the first cycle
    nl = len(ref.sizes(N, 8))
    per_cycle = (nl - 1) * (sum(pp) + 3) + 1 + (1 if sum(pp) % 2 == 0 else 0) + 2
    assert stats[1]["launches"] == 4 + stats[1]["cycles"] * per_cycle


# ---------------------------------------------------------------- 6. the non-temporal forms, one cycle
def test_large_forms(mg):
    N = 4096
    opts = dict(rtol=0.0, max_cycles=1, shift=1e4)
    rng = np.random.default_rng(4096)
    F = rng.random((N, N)) - 0.5
    Us = [rng.random((N, N)) - 0.5 for _ in range(2)]
    As = [vref.field("smooth", N), vref.field("exp", N)]
    Ss = [rref.field("smooth", N), rref.field("blob", N)]
    Fd = mg.DeviceGrid.from_host(F)
    Ad = [mg.DeviceGrid.from_host(a) for a in As]
    Sd = [mg.DeviceGrid.from_host(s) for s in Ss]
    want = []
    for a, s, U in zip(Ad, Sd, Us):
        solver = mg.Solver(N, 1.0, coef=a, reaction=s, **opts)
        Ud = mg.DeviceGrid.from_host(U)
        _, info = solver.solve(Fd, Ud)
        want.append((Ud.to_host(), info))
        Ud.free()
        solver.close()
    b = mg.BatchSolver(N, 1.0, max_batch=2, **opts)
    b.set_coefficient(Ad)
    b.set_reaction(Sd)
    Ud = [mg.DeviceGrid.from_host(U) for U in Us]
    _, infos = b.solve([Fd, Fd], Ud)
    b.close()
    assert [i["cycles"] for i in infos] == [1, 1]
    assert_batch([u.to_host() for u in Ud], infos, want, "N=4096")
    for g in [Fd] + Ad + Sd + Ud:
        g.free()


# ---------------------------------------------------------------- 7. Krylov acceleration
def bits(values):
    return np.asarray(values, dtype=np.float64).view(np.uint64).tolist()


def log_bits(log):
    return [(e["k"], bits(e["d"]), bits([e["g"], e["h"], e["alpha"], e["rho_rec"], e["rho"]]), e["restarted"]) for e in log]


@pytest.mark.parametrize("with_a", [False, True])
def test_halfplane_needs_and_gets_gcr(mg, with_a):
    """s = 1e5 on x >= 0.37 at N = 129 beside a smooth instance: the plain batch is not converged after 40 cycles on the half
    plane; with GCR(8) every instance is Solver(krylov=8, reaction=s_i[, coef=a_i]) alone, log included"""
    N, m = 129, 8
    Fs, Us = problems(N, 11, n=2)
    F, U0 = np.stack(Fs), np.stack(Us)
    Ss = [rref.field("halfplane", N), rref.field("smooth", N)]
    As = coefficients(N, 700, n=2) if with_a else None
    b = mg.BatchSolver(N, 1.0, max_batch=2, rtol=1e-9, max_cycles=40)
    if with_a:
        b.set_coefficient(As)
    b.set_reaction(Ss)
    _, plain = b.solve(F, U0)
    b.close()
    if not with_a:   # (the statement of include/mg_reaction.h, made for a = 1)
        assert not plain[0]["converged"] and plain[0]["cycles"] == 40 and plain[1]["converged"]
    opts = dict(rtol=1e-9, max_cycles=60)
    want = singles(mg, N, As, Ss, Fs, Us, krylov=m, **opts)
    if not with_a:
        assert want[0][1]["converged"] and not want[0][1]["breakdown"]

    def check(b, what):
        Ub, infos = b.solve(F, U0)
        for i, (U, info, log) in enumerate(want):
            assert_same(Ub[i], infos[i], U, info, f"{what}, instance {i}")
            assert infos[i]["breakdown"] == info["breakdown"]
            assert log_bits(b.krylov_log(i)) == log_bits(log) and len(log) == infos[i]["cycles"], (what, i)
        return infos

    b = mg.BatchSolver(N, 1.0, max_batch=2, **opts)
    if with_a:
        b.set_coefficient(As)
    b.set_reaction(Ss)
    b.set_krylov(m)
    infos = check(b, f"GCR({m}) a={with_a}: reaction, then krylov")
    b.close()
    print(f"a={with_a}: plain cycles {[i['cycles'] for i in plain]}, GCR({m}) iterations {[i['cycles'] for i in infos]}")
    b = mg.BatchSolver(N, 1.0, max_batch=2, **opts)
    b.set_krylov(m)
    b.set_reaction(Ss)
    if with_a:
        b.set_coefficient(As)
    check(b, f"GCR({m}) a={with_a}: krylov, then reaction")
    b.close()
    Uo, infos_o = mg.solve_batched_reaction(F, Ss, U0, 1.0, coef=As, krylov=m, **opts)
    for i, (U, info, _) in enumerate(want):
        assert_same(Uo[i], infos_o[i], U, info, f"solve_batched_reaction krylov a={with_a}, instance {i}")


# ---------------------------------------------------------------- 8. set, replace, grow, remove
def test_set_replace_grow_remove(mg):
    N = 100
    opts = dict(rtol=0.0, max_cycles=2)
    Fs, Us = problems(N, 800)
    F, U0 = np.stack(Fs), np.stack(Us)
    Ss = reactions(N)
    Ts = reactions(N, first=1)
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    assert not b.has_reaction and b.n_reactions == 0
    plain_U, plain = b.solve(F, U0)
    # n = 1: one shared copy
    g = mg.DeviceGrid.from_host(Ss[0])
    b.set_reaction(g)
    g.free()                                       # the caller's array may be freed after the call
    junk = mg.DeviceGrid.from_host(np.full((N, N), 7e7))   # (likely the same block, recycled)
    assert b.has_reaction and b.n_reactions == 1
    U1, infos1 = b.solve(F, U0)
    junk.free()
    assert_batch(U1, infos1, singles(mg, N, None, [Ss[0]] * 3, Fs, Us, **opts), "shared")
    # n = 3: the storage grows
    b.set_reaction(Ts)
    assert b.n_reactions == 3
    U2, infos2 = b.solve(F, U0)
    want3 = singles(mg, N, None, Ts, Fs, Us, **opts)
    assert_batch(U2, infos2, want3, "three after one: the storage has grown")
    # n = 2: the storage is reused; a solve takes at most two instances, instance i on term i
    b.set_reaction(Ss[1:])
    assert b.n_reactions == 2
    U3, infos3 = b.solve(F[:2], U0[:2])
    assert_batch(U3, infos3, singles(mg, N, None, Ss[1:], Fs[:2], Us[:2], **opts), "two after three")
    b.set_reaction(Ts)
    U4, infos4 = b.solve(F[:2], U0[:2])            # fewer instances than terms
    assert_batch(U4, infos4, want3[:2], "two instances on three terms")
    b.set_reaction(None)
    assert not b.has_reaction and b.n_reactions == 0
    back_U, back = b.solve(F, U0)
    b.close()
    for i in range(3):
        assert_same(back_U[i], back[i], plain_U[i], plain[i], f"set_reaction(None), instance {i}")
    assert back[0]["stats"]["launches"] == plain[0]["stats"]["launches"]


# ---------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_solver_as_it_was(mg):
    N = 64
    opts = dict(rtol=0.0, max_cycles=2)
    Fs, Us = problems(N, 900)
    F, U0 = np.stack(Fs), np.stack(Us)
    Ss = reactions(N)
    lib = mg.lib()
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)

    def unchanged(want_U, want, n_react, what):
        assert b.n_reactions == n_react, what
        got_U, got = b.solve(F, U0)
        for i in range(3):
            assert_same(got_U[i], got[i], want_U[i], want[i], f"after {what}, instance {i}")

    def raw(n, ptrs, pattern):
        arr = None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)
        assert lib.mg_batch_solver_set_reaction(b._s, n, arr) == 2
        with pytest.raises(mg.MGError, match=pattern):
            mg._check()

    def refusals(want_U, want, n_react):
        for bad in (np.ones((N, N + 1)), np.ones((3, N - 1, N - 1)), [Ss[0], np.ones((N + 1, N + 1))], mg.DeviceGrid(32), np.ones(N)):
            with pytest.raises(mg.MGError, match=r"\[2\].*shape"):
                b.set_reaction(bad)
            unchanged(want_U, want, n_react, "a wrong shape")
        with pytest.raises(mg.MGError, match=r"\[2\].*max_batch"):
            b.set_reaction(np.stack([Ss[0]] * 4))
        unchanged(want_U, want, n_react, "n > max_batch")
        g = mg.DeviceGrid.from_host(Ss[0])
        raw(-1, [g.ptr], r"\[2\].*n = -1 outside")
        raw(2, [g.ptr, None], r"\[2\].*instance 1 is NULL or not 16-byte aligned")
        raw(2, [g.ptr, g.ptr + 8], r"\[2\].*instance 1 is NULL or not 16-byte aligned")
        raw(2, None, r"\[2\].*NULL array")
        raw(0, [g.ptr], r"\[2\].*n = 0")
        g.free()
        unchanged(want_U, want, n_react, "a NULL or misaligned entry, n out of range, n == 0 with an array")
        for value in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
            bad = [s.copy() for s in Ss]
            bad[1][N - 1, 3] = value               # (a rim point: the rim is part of the term)
            with pytest.raises(mg.MGError, match=r"\[2\].*instance 1"):
                b.set_reaction(bad)
            unchanged(want_U, want, n_react, f"the value {value}")

    refusals(*b.solve(F, U0), 0)                   # without a reaction: the plain solver stays
    b.set_reaction(Ss)
    with_s = b.solve(F, U0)
    refusals(*with_s, 3)                           # with reactions: they stay in place
    # the adjoint is refused, the solver unchanged
    with pytest.raises(mg.MGError, match=r"\[3\].*reaction"):
        b.adjoint(F, U0)
    unchanged(*with_s, 3, "a refused adjoint")
    # more instances than reactions
    b.set_reaction(Ss[:2])
    assert b.n_reactions == 2
    two_U, two = b.solve(F[:2], U0[:2])
    with pytest.raises(mg.MGError, match=r"\[2\].*3 instances.*2 reaction"):
        b.solve(F, U0)
    again_U, again = b.solve(F[:2], U0[:2])
    for i in range(2):
        assert_same(again_U[i], again[i], two_U[i], two[i], f"after a refused solve, instance {i}")
        assert_same(again_U[i], again[i], with_s[0][i], with_s[1][i], f"two reactions, instance {i}")
    # each count bounds a solve on its own: three coefficients, two reactions
    b.set_coefficient(coefficients(N, 900))
    with pytest.raises(mg.MGError, match=r"\[2\].*3 instances.*2 reaction"):
        b.solve(F, U0)
    b.close()
    assert lib.mg_batch_solver_set_reaction(None, 0, None) == 2 and lib.mg_batch_solver_has_reaction(None) == 0
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg._check()
    with pytest.raises(TypeError):
        mg.BatchSolver(N, 1.0, 2, reaction=Ss[0])


# ---------------------------------------------------------------- 10. memory contract
@pytest.mark.parametrize("placement", _guard.PLACEMENTS)
@pytest.mark.parametrize("N", [33, 512])
def test_memory_contract(mg, N, placement):
    """instances 0 and 1 run cycles, instance 2 (F = 0, an interior far below atol) meets its tolerance at the start"""
    opts = dict(rtol=0.0, atol=1e-20, max_cycles=2)
    Fs, Us = problems(N, 1000 + N)
    Ss, As = reactions(N), coefficients(N, 1000 + N)
    Fs[2] = np.zeros((N, N))
    Us[2] = np.zeros((N, N))
    Us[2][1:-1, 1:-1] = 1e-40 * (1.0 + np.random.default_rng(N).random((N - 2, N - 2)))
    want = singles(mg, N, As, Ss, Fs, Us, **opts)
    with _guard.block(mg, [N] * 12, placement) as gb:
        gs, ga, gF, gU = gb.views[0:3], gb.views[3:6], gb.views[6:9], gb.views[9:12]
        for views, arrays in ((gs, Ss), (ga, As), (gF, Fs), (gU, Us)):
            for v, x in zip(views, arrays):
                v.upload(x)
        b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
        gb.expect_readonly(*gb.views)
        b.set_reaction(gs)
        gb.check(f"set_reaction N={N} {placement}")
        b.set_coefficient(ga)
        gb.check(f"set_coefficient N={N} {placement}")
        gb.expect_readonly(*gs, *ga, *gF, gU[2])
        infos = b.solve_ptrs([v.ptr for v in gF], [v.ptr for v in gU])
        gb.check(f"solve N={N} {placement}")
        b.close()
        assert [i["cycles"] for i in infos] == [2, 2, 0]
        assert_batch([v.to_host() for v in gU], infos, want, f"N={N} {placement}")
        assert_bits(gU[2].to_host(), Us[2], "the U of the instance that converged at the start")


# ---------------------------------------------------------------- 11. the smoother setting does not matter
@pytest.mark.parametrize("with_a", [False, True])
def test_simple_smoother_setting_gives_the_same_bits(mg, with_a):
    N = 100
    opts = dict(rtol=0.0, max_cycles=3, shift=2.0)
    Fs, Us = problems(N, 1100)
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    if with_a:
        b.set_coefficient(coefficients(N, 1100))
    b.set_reaction(reactions(N))
    want_U, want = b.solve(np.stack(Fs), np.stack(Us))
    mg.set_smoother("simple")
    try:
        got_U, got = b.solve(np.stack(Fs), np.stack(Us))
    finally:
        mg.set_smoother("stream")
    b.close()
    for i in range(3):
        assert_same(got_U[i], got[i], want_U[i], want[i], f"MG_SMOOTHER=simple a={with_a}, instance {i}")
        assert got[i]["stats"]["launches"] == want[i]["stats"]["launches"]
