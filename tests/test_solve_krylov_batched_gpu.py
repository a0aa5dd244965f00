"""The batched Krylov acceleration (include/mg_krylov_batch.h) on the GPU.  The contract is bit identity with code that is
tested on its own (tests/test_solve_krylov_gpu.py replays Solver(krylov=m) from its log against the numpy restatement):
instance i of a BatchSolver after set_krylov(m) equals Solver(krylov=m, coef=a_i) on F_i, U_i alone -- U, the info keys, the
history, the breakdown flag and the whole log, compared with == and assert_bits.  Sizes: one column per lane for odd and
small even N, column pairs with their edge lanes at 512."""
import numpy as np
import pytest

import _guard
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
KEYS = ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm", "breakdown")
FIELDS = ("one", "smooth", "jump", "random")
# the inputs of tests/test_solve_krylov_batched_cpu.py on which two instances sit at different k in one iteration
DIVERGING = [(33, "smooth", 4, 1e-14, 30, (1, 2)), (65, "jump", 8, 1e-13, 30, (2, 3))]


def coefficient(name, N, seed=1):
    return None if name is None else vref.field(name, N, seed=seed)


def single(mg, N, a, F, U, m, **opts):
    """(U, info, log) of Solver(krylov=m, coef=a).solve(F, U): the reference of every comparison below"""
    s = mg.Solver(N, 1.0, coef=a, krylov=m, **opts)
    out_U, info = s.solve(F, U)
    log = s.krylov_log()
    s.close()
    return out_U, info, log


def singles(mg, N, As, Fs, Us, m, **opts):
    return [single(mg, N, a, F, U, m, **opts) for a, F, U in zip(As, Fs, Us)]


def bits(values):
    """the values as bit patterns: == on them holds for a NaN too (the instance with a NaN in F has them in its history and log)"""
    return np.asarray(values, dtype=np.float64).view(np.uint64).tolist()


def log_bits(log):
    return [(e["k"], bits(e["d"]), bits([e["g"], e["h"], e["alpha"], e["rho_rec"], e["rho"]]), e["restarted"]) for e in log]


def assert_same(got_U, got, got_log, want, what):
    want_U, info, log = want
    assert_bits(got_U, want_U, f"{what}: U")
    assert bits(got["history"]) == bits(info["history"]), what
    assert len(got["history"]) == got["cycles"] + 1
    for key in KEYS:
        assert bits([got[key]]) == bits([info[key]]), (what, key, got[key], info[key])
    assert log_bits(got_log) == log_bits(log), what  # k, d_j, g, h, alpha, rho_rec, restarted, rho of every iteration
    assert len(got_log) == got["cycles"]


def assert_batch(b, Ub, infos, want, what):
    assert len(infos) == len(want)
    for i in range(len(want)):
        assert_same(Ub[i], infos[i], b.krylov_log(i), want[i], f"{what}, instance {i}")
    assert infos[0]["stats"]["cycles"] == max(i["cycles"] for i in infos)


def problems(N, seed, n=3):
    FU = [ref.random_problem(N, seed + i) for i in range(n)]
    return [f for f, _ in FU], [u for _, u in FU]


# ---------------------------------------------------------------- 1. an instance is its single solve
@pytest.mark.parametrize("m", [1, 4, 8])
@pytest.mark.parametrize("N", [33, 64, 100, 257, 512])
def test_instance_equals_single_solve(mg, N, m):
    """at most 12 iterations each: restarts at k = m for every m, and for m = 8 every k from 0 to 7"""
    Fs, Us = problems(N, 100 + N + m)
    F, U0 = np.stack(Fs), np.stack(Us)
    case = 0
    for shift in (0.0, 1e4):
        for pp in ((3, 3), (2, 1)):
            opts = dict(pre=pp[0], post=pp[1], shift=shift, rtol=1e-9, max_cycles=12)
            what = f"N={N} m={m} shift={shift:g} V{pp}"
            names = [FIELDS[(case + N + i) % 4] for i in range(3)]      # three of the four fields, rotating over the cases
            case += 1
            As = [coefficient(name, N, seed=7 + i) for i, name in enumerate(names)]
            want = singles(mg, N, As, Fs, Us, m, **opts)
            b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
            b.set_krylov(m)
            assert b.krylov == m
            b.set_coefficient(np.stack(As))
            Ub, infos = b.solve(F, U0)
            assert_batch(b, Ub, infos, want, f"{what} {names}")
            assert all(i["cycles"] >= 1 for i in infos)
            # the same instances in reverse order: where an instance sits in the batch does not matter
            b.set_coefficient(As[::-1])
            Ur, infos_r = b.solve(F[::-1], U0[::-1])
            assert_batch(b, Ur, infos_r, want[::-1], f"{what} {names} reversed")
            # one coefficient shared by every instance
            b.set_coefficient(As[1])
            Ush, infos_s = b.solve(F, U0)
            assert_batch(b, Ush, infos_s, singles(mg, N, [As[1]] * 3, Fs, Us, m, **opts), f"{what} shared {names[1]}")
            # and none: the constant operator
            b.set_coefficient(None)
            Un, infos_n = b.solve(F, U0)
            assert_batch(b, Un, infos_n, singles(mg, N, [None] * 3, Fs, Us, m, **opts), f"{what} no coefficient")
            b.close()
    print(f"N={N} m={m}: cycles {[i['cycles'] for i in infos_n]}, launches {infos_n[0]['stats']['launches']}")


# ---------------------------------------------------------------- 2. instances at different k in one launch
def test_diverging_k(mg):
    """Two instances of one batch at different k in the same iteration (one restarted on its recurred norm, found the
    recomputed norm above its tolerance and went on from k = 0), and between them an instance that never iterates, so the
    active slots are not the positions in the call."""
    chosen = None
    for N, name, m, rtol, max_cycles, seeds in DIVERGING:
        a = coefficient(name, N)
        opts = dict(rtol=rtol, max_cycles=max_cycles)
        FU = [ref.random_problem(N, seed) for seed in seeds]
        want = [single(mg, N, a, F, U, m, **opts) for F, U in FU]
        ks = [[e["k"] for e in log] for _, _, log in want]
        differ = [i for i, (x, y) in enumerate(zip(*ks)) if x != y]
        print(f"N={N} {name} m={m}: the single solves sit at different k in iterations {differ}")
        if differ:   # (a condition on the single solver alone)
            chosen = (N, a, m, opts, FU, want)
            break
    assert chosen, "no input on which the single solves' k diverge"
    N, a, m, opts, FU, want = chosen
    zero = np.zeros((N, N))
    want = [want[0], single(mg, N, a, zero, zero, m, **opts), want[1]]
    assert want[1][1]["cycles"] == 0
    b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    b.set_coefficient(a)
    b.set_krylov(m)
    Ub, infos = b.solve(np.stack([FU[0][0], zero, FU[1][0]]), np.stack([FU[0][1], zero, FU[1][1]]))
    assert_batch(b, Ub, infos, want, "diverging k")
    assert b.krylov_log(1) == [] and b.krylov_log(3) == [] and b.krylov_log(-1) == []
    b.close()


# ---------------------------------------------------------------- 3. the active set
def test_active_set(mg):
    N, m = 129, 8
    opts = dict(rtol=1e-9, atol=1e-20)
    names = ("smooth", "smooth", "jump", "exp", "smooth")
    As = [coefficient(name, N, seed=3 + i) for i, name in enumerate(names)]
    Fs, Us = problems(N, 500 + N, n=5)
    # instance 0: F = 0 and a zero rim; its interior is a pattern far below atol, so it meets the tolerance at the start
    Fs[0] = np.zeros((N, N))
    Us[0] = np.zeros((N, N))
    Us[0][1:-1, 1:-1] = 1e-40 * (1.0 + np.random.default_rng(7).random((N - 2, N - 2)))
    # instance 4: a NaN in F -- the first g is NaN: a breakdown after one iteration
    Fs[4] = Fs[4].copy()
    Fs[4][20, 30] = np.nan
    want = singles(mg, N, As, Fs, Us, m, **opts)
    b = mg.BatchSolver(N, 1.0, max_batch=5, **opts)
    b.set_coefficient(As)
    b.set_krylov(m)
    Ub, infos = b.solve(np.stack(Fs), np.stack(Us))
    cycles = [i["cycles"] for i in infos]
    print(f"cycles {cycles}")
    assert cycles[0] == 0 and infos[0]["converged"] and b.krylov_log(0) == [] and not infos[0]["breakdown"]
    assert_bits(Ub[0], Us[0], "the instance that met its tolerance at the start is untouched")
    assert all(i["converged"] and not i["breakdown"] for i in infos[1:4]) and len(set(cycles[1:4])) >= 2, cycles
    assert infos[4]["breakdown"] and not infos[4]["converged"] and cycles[4] == 1 and len(b.krylov_log(4)) == 1
    assert b.krylov_log(4)[0]["alpha"] == 0.0
    assert_bits(Ub[4], Us[4], "U after a breakdown")
    assert_batch(b, Ub, infos, want, "active set")
    b.close()


# ---------------------------------------------------------------- 4. launches do not depend on the batch size
def test_launch_count_is_independent_of_the_batch(mg):
    N, m = 65, 4
    a = coefficient("jump", N)
    F, U0 = ref.random_problem(N, 600)
    stats, logs = {}, {}
    for B in (1, 16):
        b = mg.BatchSolver(N, 1.0, max_batch=B, rtol=1e-9)
        b.set_coefficient(np.stack([a] * B))
        b.set_krylov(m)
        _, infos = b.solve(np.stack([F] * B), np.stack([U0] * B))
        stats[B], logs[B] = infos[0]["stats"], b.krylov_log(B - 1)
        assert all(i["history"] == infos[0]["history"] and i["converged"] for i in infos)
        b.close()
    assert stats[1]["launches"] == stats[16]["launches"] > 0 and stats[1]["cycles"] == stats[16]["cycles"] > m
    assert logs[1] == logs[16]
    # the header's formula: the two norms (4), the residual that starts the loop (1), and per iteration the zeroing, the
    # cycle -- (nl - 1)*(pre + post + 3) + 1 launches and one copy (pre + post even) --, A*z, the dots and their finish
    # while k > 0, the orthogonalisation and the update with their finishes, and 4 for a restart
    nl = len(ref.sizes(N, 8))
    cycle = (nl - 1) * 9 + 1 + 1
    want = 4 + 1 + sum(cycle + 6 + (2 if e["k"] > 0 else 0) + (4 if e["restarted"] else 0) for e in logs[1])
    assert stats[1]["launches"] == want, (stats[1]["launches"], want)
    assert any(e["restarted"] and e["k"] + 1 == m for e in logs[1])      # (restarts known before the read-back ...)
    print(f"restarts found by the read-back: {sum(e['restarted'] and e['k'] + 1 < m for e in logs[1])}, launches {want}")


# ---------------------------------------------------------------- 5. m = 0 is the batch solver without the option
def _names(mg, run):
    mg.profile_begin(0)
    try:
        out = run()
    finally:
        prof = mg.profile_end(1024)
    return out, sorted((p["name"], p["N"], p["launches"]) for p in prof)


@pytest.mark.parametrize("name", [None, "smooth"])
def test_krylov_zero_is_the_plain_batch_solver(mg, name):
    N = 100
    Fs, Us = problems(N, 1100)
    F, U0 = np.stack(Fs), np.stack(Us)
    a = coefficient(name, N)
    opts = dict(rtol=1e-9, max_cycles=4)

    def plain(b):
        (U, infos), names = _names(mg, lambda: b.solve(F, U0))
        assert all("breakdown" not in i for i in infos) and not any(n.startswith("krylov") for n, _, _ in names)
        return U, [i["history"] for i in infos], infos[0]["stats"]["launches"], names

    never = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    if a is not None:
        never.set_coefficient(a)
    want = plain(never)
    never.close()
    zero = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    if a is not None:
        zero.set_coefficient(a)
    zero.set_krylov(0)
    assert zero.krylov == 0
    got = plain(zero)
    assert_bits(got[0], want[0], "set_krylov(0)")
    assert got[1:] == want[1:]
    # on, then off again: the plain bits and launches, none of the new ones
    zero.set_krylov(8)
    (_, on), on_names = _names(mg, lambda: zero.solve(F, U0))
    assert {"krylov_zero_batch", "krylov_apply_batch", "krylov_dots_batch", "krylov_orth_batch", "krylov_update_batch"} <= \
        {n for n, _, _ in on_names}
    assert all("breakdown" in i for i in on)
    zero.set_krylov(0)
    assert zero.krylov == 0
    back = plain(zero)
    zero.close()
    assert_bits(back[0], want[0], "set_krylov(8) then set_krylov(0)")
    assert back[1:] == want[1:]


# ---------------------------------------------------------------- 6. the same solve twice
def test_same_solve_twice_gives_identical_bits_and_logs(mg):
    N = 257
    Fs, Us = problems(N, 1200)
    As = [coefficient(name, N, seed=5) for name in ("jump", "random", "smooth")]
    b = mg.BatchSolver(N, 1.0, max_batch=3, rtol=1e-9, max_cycles=20)
    b.set_coefficient(As)
    b.set_krylov(4)
    first_U, first = b.solve(np.stack(Fs), np.stack(Us))
    first_logs = [b.krylov_log(i) for i in range(3)]
    second_U, second = b.solve(np.stack(Fs), np.stack(Us))
    assert_bits(second_U, first_U, "second solve")
    assert [i["history"] for i in second] == [i["history"] for i in first]
    assert [b.krylov_log(i) for i in range(3)] == first_logs and all(first_logs)
    assert second[0]["stats"]["launches"] == first[0]["stats"]["launches"]
    b.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_solver_as_it_was(mg):
    N = 64
    Fs, Us = problems(N, 1300)
    F, U0 = np.stack(Fs), np.stack(Us)
    b = mg.BatchSolver(N, 1.0, max_batch=3, rtol=0.0, max_cycles=3)
    b.set_krylov(4)
    want_U, want = b.solve(F, U0)
    want_logs = [b.krylov_log(i) for i in range(3)]

    def unchanged(what):
        assert b.krylov == 4
        got_U, got = b.solve(F, U0)
        assert_bits(got_U, want_U, f"after {what}")
        assert [i["history"] for i in got] == [i["history"] for i in want]
        assert [b.krylov_log(i) for i in range(3)] == want_logs

    for m in (-1, 17):
        with pytest.raises(mg.MGError, match=r"\[2\]"):
            b.set_krylov(m)
        unchanged(f"the refused m = {m}")
    lib = mg.lib()
    assert lib.mg_batch_solver_set_krylov(None, 4) == 2
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg._check()
    unchanged("a NULL solver")
    assert lib.mg_batch_solver_krylov(None) == 0 and lib.mg_batch_solver_krylov_breakdown(None, 0) == 0
    assert lib.mg_batch_solver_krylov_log(None, 0, None, 0) == 0
    b.close()


# ---------------------------------------------------------------- 8. lifecycle
def test_lifecycle(mg):
    N = 100
    opts = dict(rtol=1e-9, max_cycles=10)
    Fs, Us = problems(N, 1400, n=4)
    As = [coefficient(name, N, seed=2 + i) for i, name in enumerate(("smooth", "jump", "random", "smooth"))]
    Bs = [coefficient(name, N, seed=9 + i) for i, name in enumerate(("random", "smooth", "jump", "jump"))]
    b = mg.BatchSolver(N, 1.0, max_batch=4, **opts)
    b.set_krylov(2)                                # before any coefficient, on two of the four instances
    U, infos = b.solve(np.stack(Fs[:2]), np.stack(Us[:2]))
    assert_batch(b, U, infos, singles(mg, N, [None] * 2, Fs[:2], Us[:2], 2, **opts), "m = 2, two instances")
    b.set_krylov(8)                                # a larger m: more slots; and more instances than the last call
    U, infos = b.solve(np.stack(Fs), np.stack(Us))
    assert_batch(b, U, infos, singles(mg, N, [None] * 4, Fs, Us, 8, **opts), "m = 8, four instances")
    b.set_coefficient(As)                          # the coefficient after the acceleration
    U, infos = b.solve(np.stack(Fs), np.stack(Us))
    assert_batch(b, U, infos, singles(mg, N, As, Fs, Us, 8, **opts), "coefficients set")
    b.set_coefficient(Bs)
    U, infos = b.solve(np.stack(Fs), np.stack(Us))
    assert_batch(b, U, infos, singles(mg, N, Bs, Fs, Us, 8, **opts), "coefficients replaced")
    b.set_krylov(3)                                # a smaller m on the storage it has
    U, infos = b.solve(np.stack(Fs[:3]), np.stack(Us[:3]))
    assert_batch(b, U, infos, singles(mg, N, Bs[:3], Fs[:3], Us[:3], 3, **opts), "m = 3, three instances")
    assert b.krylov_log(3) == []                   # outside the last solve
    b.set_coefficient(None)
    U, infos = b.solve(np.stack(Fs), np.stack(Us))
    want = singles(mg, N, [None] * 4, Fs, Us, 3, **opts)
    assert_batch(b, U, infos, want, "coefficients removed")
    b.close()
    b.close()
    c = mg.BatchSolver(N, 1.0, max_batch=4, **opts)   # closed and recreated; krylov after the coefficient
    c.set_coefficient(Bs[0])
    c.set_krylov(3)
    U, infos = c.solve(np.stack(Fs), np.stack(Us))
    assert_batch(c, U, infos, singles(mg, N, [Bs[0]] * 4, Fs, Us, 3, **opts), "recreated")
    del c


# ---------------------------------------------------------------- 9. memory contract
@pytest.mark.parametrize("placement", _guard.PLACEMENTS)
@pytest.mark.parametrize("N", [33, 512])
def test_memory_contract(mg, N, placement):
    """F, U and the coefficients inside guard bands: instances 0 and 1 iterate, instance 2 (F = 0, an interior far below
    atol) meets its tolerance at the start and is never written.  The rims the header speaks of -- those of q_j, z_j and r --
    are the solver's own storage; the kernels' bodies are held against NaN rims on caller arrays by
    tests/test_solve_krylov_gpu.py, and of the caller's arrays here the rim of U must keep its bits."""
    m = 4
    opts = dict(rtol=0.0, atol=1e-20, max_cycles=6)
    Fs, Us = problems(N, 900 + N)
    As = [coefficient(name, N, seed=4) for name in ("jump", "random", "smooth")]
    Fs[2] = np.zeros((N, N))
    Us[2] = np.zeros((N, N))
    Us[2][1:-1, 1:-1] = 1e-40 * (1.0 + np.random.default_rng(N).random((N - 2, N - 2)))
    want = singles(mg, N, As, Fs, Us, m, **opts)
    with _guard.block(mg, [N] * 9, placement) as gb:
        ga, gF, gU = gb.views[0:3], gb.views[3:6], gb.views[6:9]
        for views, arrays in ((ga, As), (gF, Fs), (gU, Us)):
            for v, x in zip(views, arrays):
                v.upload(x)
        b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
        gb.expect_readonly(*gb.views)
        b.set_krylov(m)
        b.set_coefficient(ga)
        gb.check(f"set_krylov, set_coefficient N={N} {placement}")
        gb.expect_readonly(*ga, *gF, gU[2])
        infos = b.solve_ptrs([v.ptr for v in gF], [v.ptr for v in gU])
        gb.check(f"solve N={N} {placement}")
        got = [v.to_host() for v in gU]
        assert [i["cycles"] for i in infos] == [6, 6, 0]
        assert_batch(b, got, infos, want, f"N={N} {placement}")
        b.close()
        assert_bits(got[2], Us[2], "the U of the instance that converged at the start")
        for i in range(3):
            rim = np.ones((N, N), dtype=bool)
            rim[1:-1, 1:-1] = False
            assert_bits(got[i][rim], Us[i][rim], f"the rim of U, instance {i}")


# ---------------------------------------------------------------- 10. MG_SMOOTHER=simple
def test_simple_smoother(mg):
    """the constant batch solver then runs its cycle instance by instance: the bits of the single solver under the setting"""
    N, m = 100, 4
    opts = dict(rtol=1e-9, max_cycles=10, shift=2.0)
    Fs, Us = problems(N, 1500)
    As = [coefficient(name, N, seed=6) for name in ("jump", "smooth", "random")]
    mg.set_smoother("simple")
    try:
        b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
        b.set_krylov(m)
        U, infos = b.solve(np.stack(Fs), np.stack(Us))
        assert_batch(b, U, infos, singles(mg, N, [None] * 3, Fs, Us, m, **opts), "simple, no coefficient")
        b.set_coefficient(As)                      # (with a coefficient the cycle is the variable one, whatever the setting)
        U, infos = b.solve(np.stack(Fs), np.stack(Us))
        assert_batch(b, U, infos, singles(mg, N, As, Fs, Us, m, **opts), "simple, coefficients")
        b.close()
    finally:
        mg.set_smoother("stream")


# ---------------------------------------------------------------- 11. the one-shot function
def test_solve_batched_krylov_equals_the_class(mg):
    N, m = 65, 8
    opts = dict(rtol=1e-9, shift=3.0)
    Fs, Us = problems(N, 1600)
    As = [coefficient(name, N, seed=8) for name in ("random", "jump", "smooth")]
    F, U0 = np.stack(Fs), np.stack(Us)
    for coef, what in ((np.stack(As), "per instance"), (As[0], "shared"), (None, "none")):
        b = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
        if coef is not None:
            b.set_coefficient(coef)
        b.set_krylov(m)
        want_U, want = b.solve(F, U0)
        b.close()
        got_U, got = mg.solve_batched_krylov(F, m, U0, 1.0, coef=coef, **opts)
        assert_bits(got_U, want_U, f"solve_batched_krylov, {what}")
        for g, w in zip(got, want):
            assert g["history"] == w["history"] and all(g[key] == w[key] for key in KEYS), what
    # U = None: the zero start
    got_U, got = mg.solve_batched_krylov(F, m, coef=As[0], **opts)
    want_U, want = mg.solve_batched_krylov(F, m, np.zeros_like(U0), coef=As[0], **opts)
    assert_bits(got_U, want_U, "U = None")
    assert [g["history"] for g in got] == [w["history"] for w in want] and all(g["converged"] for g in got)
