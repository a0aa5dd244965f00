"""The Krylov acceleration (include/mg_krylov.h) on the GPU: every kernel alone through its test hook -- vectors bit for bit
against numpy, sums within the a-priori bound of the longdouble sum, NaN rims, guard bands, both placements; whole solves
replayed from the engine's log (tests/_krylov_ref.py) with every coarse solve qualified; krylov = 0 against
the option never set; determinism; the hard coefficients; refusals, breakdown and lifecycle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _guard
import _krylov_ref as kref
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
U53 = ref.U53


def lib_table(mg):
    return lambda N, M: mg.restriction_table(N, M)


def nan_rim(x):
    x[0, :] = x[-1, :] = np.nan
    x[:, 0] = x[:, -1] = np.nan
    return x


def vectors(N, count, seed):
    rng = np.random.default_rng(seed)
    return [nan_rim(rng.random((N, N)) - 0.5) for _ in range(count)]


def within(got, want, N):
    """a device sum against (longdouble sum, sum of absolute products): the header's bound, any summation order"""
    total, abs_sum = want
    return abs(LD(got) - total) <= kref.sum_bound(N, abs_sum)


# ---------------------------------------------------------------- kernels alone, inside guard bands
# one column per lane below N = 512 and for odd N, 16-byte accesses for even N >= 512; no form switches at a larger size
SIZES = [3, 4, 5, 17, 63, 64, 65, 100, 255, 256, 510, 511, 512, 513, 1024, 1026]


@pytest.mark.parametrize("k", [0, 1, 2, 7, 15])
@pytest.mark.parametrize("N", SIZES)
def test_dots_and_orthogonalisation_alone(mg, N, k):
    q, z, r, *rest = vectors(N, 3 + 2 * k, 100 * N + k)
    Q, Z = rest[:k], rest[k:]
    b = np.random.default_rng(k).random(k) - 0.5
    want_q, want_z = q.copy(), z.copy()
    kref.orthogonalise(want_q, want_z, b, Q, Z)
    for placement in _guard.PLACEMENTS:
        what = f"N={N} k={k} {placement}"
        with _guard.block(mg, [N] * (3 + 2 * k), placement) as gb:
            gq, gz, gr = gb.views[:3]
            gQ, gZ = gb.views[3:3 + k], gb.views[3 + k:]
            for view, x in zip(gb.views, [q, z, r] + Q + Z):
                view.upload(x)
            gb.expect_readonly(*gb.views)
            d = mg.krylovDots(N, gq, gQ)
            gb.check("dots " + what)
            assert len(d) == k
            for j in range(k):
                assert within(d[j], kref.dot_ld(q, Q[j]), N), (what, j, d[j])
            # k == 0 stores nothing: q and z stay read-only too
            gb.expect_readonly(*([gr] + gQ + gZ + ([gq, gz] if k == 0 else [])))
            g, h = mg.krylovOrth(N, b, gq, gz, gr, gQ, gZ)
            gb.check("orth " + what)
            assert_bits(gq.to_host(), want_q, "q " + what)
            assert_bits(gz.to_host(), want_z, "z " + what)
            assert within(g, kref.dot_ld(want_q, want_q), N), (what, g)
            assert within(h, kref.dot_ld(r, want_q), N), (what, h)


@pytest.mark.parametrize("N", SIZES)
def test_update_alone(mg, N):
    U, z, r, q = vectors(N, 4, 7 * N)
    for placement in _guard.PLACEMENTS:
        for alpha in (0.37, 0.0, -1e-3):
            what = f"N={N} alpha={alpha} {placement}"
            want_U, want_r = U.copy(), r.copy()
            kref.update(alpha, want_U, z, want_r, q)
            with _guard.block(mg, [N] * 4, placement) as gb:
                gU, gz, gr, gq = gb.views
                for view, x in zip(gb.views, (U, z, r, q)):
                    view.upload(x)
                gb.expect_readonly(*([gz, gq] + ([gU, gr] if alpha == 0.0 else [])))
                rr = mg.krylovUpdate(N, alpha, gU, gz, gr, gq)
                gb.check("update " + what)
                assert_bits(gU.to_host(), want_U, "U " + what)
                assert_bits(gr.to_host(), want_r, "r " + what)
                assert within(rr, kref.dot_ld(want_r, want_r), N), (what, rr)


def test_hooks_refuse_bad_arguments(mg):
    g = mg.DeviceGrid.zeros(8)
    for call in (lambda: mg.krylovDots(2, g, [g]), lambda: mg.krylovDots(8, g, [g] * 16),
                 lambda: mg.krylovUpdate(2, 1.0, g, g, g, g)):
        with pytest.raises(mg.MGError, match=r"\[2\]"):
            call()
    g.free()


# ---------------------------------------------------------------- whole solves by replay
def problem(N, seed=1):
    return ref.random_problem(N, seed)


def coefficient(name, N):
    return None if name == "none" else vref.field(name, N, seed=1)


def solve_and_replay(mg, oracle, N, name, m, what, seed=1, **opts):
    """One accelerated solve and its replay from the log: U bit for bit, the logged sums within their bounds, the history and
    the restart flags where the rule puts them.  Returns (info, log, replay)."""
    F, U0 = problem(N, seed)
    a = coefficient(name, N)
    s = mg.Solver(N, 1.0, coef=a, krylov=m, **opts)
    assert s.krylov == m
    U, info = s.solve(F, U0)
    log = s.krylov_log()
    s.close()
    margins = []
    out = kref.solve(oracle, a, F, U0, 1.0, m=m, log=log, margins=margins, table=lib_table(mg), **opts)
    ref.assert_qualified(margins, what)
    assert info["cycles"] == len(log) == out["cycles"], (what, info["cycles"], len(log), out["cycles"])
    # (the zero_sign rule where the house applies it: the constant solver's cycles against the restatement)
    assert_bits(U, out["U"], what + ": U", zero_sign=a is None)
    assert info["converged"] == out["converged"] and info["breakdown"] == out["breakdown"]
    assert info["history"][1:] == [e["rho"] for e in log] and info["res"] == info["history"][-1]
    assert abs(info["history"][0] - out["history"][0]) <= 1e-12 * out["history"][0]
    tol = max(opts.get("rtol", 1e-10) * info["ref_norm"], opts.get("atol", 0.0))
    k = 0
    for i, (e, rec) in enumerate(zip(log, out["records"])):
        at = f"{what}, iteration {i}"
        assert e["k"] == k == rec["k"], at
        for j in range(k):
            assert within(e["d"][j], rec["d"][j], N), (at, j)
        assert within(e["g"], rec["g"], N) and within(e["h"], rec["h"], N), at
        assert e["alpha"] == rec["alpha"], at            # formed on the device as the header forms it: h*(1/g)
        rr = np.sqrt(rec["rr"][0])
        assert abs(LD(e["rho_rec"]) - rr) <= (kref.gamma((N - 2) ** 2) + 2 * U53) * rr, at
        k += 1
        assert e["restarted"] == (k == m or e["rho_rec"] <= tol) == rec["restarted"], at
        if e["restarted"]:
            assert abs(e["rho"] - rec["rho_own"]) <= 1e-12 * rec["rho_own"], at
            k = 0
        else:
            assert e["rho"] == e["rho_rec"], at
    return info, log, out


@pytest.mark.parametrize("m", [1, 4, 8])
@pytest.mark.parametrize("name", ["none", "smooth", "jump", "random"])
@pytest.mark.parametrize("N", [33, 65, 100, 129, 257])
def test_whole_solves_replayed_from_the_log(mg, oracle, N, name, m):
    """at most 12 iterations each: restarts at k = m for every m, and for m = 8 every k from 0 to 7"""
    for shift in (0.0, 1e4):
        for pp in ((3, 3), (2, 1)):
            opts = dict(pre=pp[0], post=pp[1], shift=shift, rtol=1e-9, max_cycles=12)
            what = f"N={N} a={name} m={m} shift={shift:g} V{pp}"
            info, log, _ = solve_and_replay(mg, oracle, N, name, m, what, **opts)
            assert info["cycles"] >= 1
            if name == "none":   # the constant solver runs the fused cycle by default: the operator-by-operator one too
                mg.set_smoother("simple")
                try:
                    simple, _, _ = solve_and_replay(mg, oracle, N, name, m, what + " simple", **opts)
                finally:
                    mg.set_smoother("stream")
                assert simple["cycles"] == info["cycles"]
                np.testing.assert_allclose(simple["history"], info["history"], rtol=1e-12, atol=0.0)


# ---------------------------------------------------------------- krylov = 0 is the solver without the option
def _names(mg, run):
    mg.profile_begin(0)
    try:
        out = run()
    finally:
        prof = mg.profile_end(1024)
    return out, sorted((p["name"], p["N"], p["launches"]) for p in prof)


@pytest.mark.parametrize("name", ["none", "smooth"])
def test_krylov_zero_is_the_plain_solver(mg, name):
    N = 100
    F, U0 = problem(N, 11)
    a = coefficient(name, N)
    opts = dict(rtol=1e-9, max_cycles=4)
    never = mg.Solver(N, 1.0, coef=a, **opts)
    (want_U, want), want_names = _names(mg, lambda: never.solve(F, U0))
    never.close()
    zero = mg.Solver(N, 1.0, coef=a, krylov=0, **opts)
    zero.set_krylov(0)
    (got_U, got), got_names = _names(mg, lambda: zero.solve(F, U0))
    assert_bits(got_U, want_U, "krylov = 0")
    assert got["history"] == want["history"] and got_names == want_names and "breakdown" not in got
    assert not any(n.startswith("krylov") for n, _, _ in got_names)
    # on, then off again: the plain bits, and none of the new launches
    zero.set_krylov(8)
    (_, on), on_names = _names(mg, lambda: zero.solve(F, U0))
    assert {"krylov_dots", "krylov_orth", "krylov_update"} <= {n for n, _, _ in on_names} and "breakdown" in on
    zero.set_krylov(0)
    assert zero.krylov == 0
    (back_U, back), back_names = _names(mg, lambda: zero.solve(F, U0))
    zero.close()
    assert_bits(back_U, want_U, "set_krylov(8) then set_krylov(0)")
    assert back["history"] == want["history"] and back_names == want_names


def test_same_solve_twice_gives_identical_bits_and_log(mg):
    N = 257
    F, U0 = problem(N, 12)
    s = mg.Solver(N, 1.0, coef=vref.field("jump", N), krylov=4, rtol=1e-9)
    first_U, first = s.solve(F, U0)
    first_log = s.krylov_log()
    second_U, second = s.solve(F, U0)
    assert_bits(second_U, first_U, "second solve")
    assert second["history"] == first["history"] and s.krylov_log() == first_log and first["converged"]
    s.close()


# ---------------------------------------------------------------- the hard coefficients
def test_random_field_converges_with_krylov_and_not_without(mg, oracle):
    N = 65
    F, U0 = problem(N)
    a = vref.field("random", N, seed=1)
    _, plain = mg.solve(F, U0, coef=a, rtol=1e-9)
    assert plain["status"] == mg.MG_SOLVE_NOT_CONVERGED and plain["cycles"] == 50
    info, log, out = solve_and_replay(mg, oracle, N, "random", 8, "N=65 random to 1e-9", rtol=1e-9)
    print(f"N=65 random: plain {plain['res']:.3e} after 50 cycles, krylov=8 {info['cycles']} iterations to {info['res']:.3e}")
    assert info["converged"] and info["status"] == mg.MG_SOLVE_CONVERGED and not info["breakdown"]
    assert log[-1]["restarted"]
    rU = vref.residual_norm_ld(a, out["U"], F, 1.0, 0.0)
    R = vref.residual_rounding_bound(a, out["U"], F, 1.0, 0.0)
    assert info["res"] <= 1e-9 * info["ref_norm"] and rU <= 1e-9 * ref.ref_norm(F) + R and abs(LD(info["res"]) - rU) <= R


def test_no_growth_where_the_plain_history_grows(mg):
    N = 129
    F, U0 = problem(N)
    a = vref.field("random", N, seed=1)
    _, plain = mg.solve(F, U0, coef=a, rtol=1e-9)
    grows = [b > a for a, b in zip(plain["history"], plain["history"][1:])]
    assert not plain["converged"] and sum(grows) >= 40 and plain["history"][-1] > min(plain["history"])
    s = mg.Solver(N, 1.0, coef=a, krylov=8, rtol=1e-9)
    _, info = s.solve(F, U0)
    log = s.krylov_log()
    s.close()
    hist = info["history"]
    steps = [(hist[i], hist[i + 1]) for i, e in enumerate(log) if not e["restarted"]]
    assert len(steps) >= 40
    for before, after in steps:
        assert after <= before * (1.0 + 1e-12), (before, after)
    assert hist[-1] < 1e-6 * hist[0]


# ---------------------------------------------------------------- refusals, breakdown, lifecycle
def test_refusals_leave_the_solver_as_it_was(mg):
    N = 64
    F, U0 = problem(N, 13)
    s = mg.Solver(N, 1.0, krylov=4, rtol=0.0, max_cycles=3)
    want_U, want = s.solve(F, U0)
    for m in (-1, 17):
        with pytest.raises(mg.MGError, match=r"\[2\]"):
            s.set_krylov(m)
        assert s.krylov == 4
        got_U, got = s.solve(F, U0)
        assert_bits(got_U, want_U, f"after the refused m = {m}")
        assert got["history"] == want["history"]
    s.close()
    f = mg.Solver(N, 1.0, fmg=1, rtol=0.0, max_cycles=1)
    want_U, _ = f.solve(F, U0)
    with pytest.raises(mg.MGError, match=r"\[3\].*fmg"):
        f.set_krylov(4)
    assert f.krylov == 0
    got_U, _ = f.solve(F, U0)
    assert_bits(got_U, want_U, "the fmg solver after the refusal")
    f.close()
    with pytest.raises(mg.MGError, match=r"\[3\].*fmg"):
        mg.Solver(N, 1.0, fmg=1, krylov=4)
    lib = mg.lib()
    assert lib.mg_solver_set_krylov(None, 4) == 2
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg._check()
    assert lib.mg_solver_krylov(None) == 0 and lib.mg_solver_krylov_breakdown(None) == 0 and lib.mg_solver_krylov_log(None, None, 0) == 0
    with pytest.raises(TypeError):
        mg.solve_opts(krylov=4)            # an option of Solver, not a field of mg_solve_opts
    with pytest.raises(TypeError):
        mg.BatchSolver(N, 1.0, 2, krylov=4)
    with pytest.raises(TypeError):
        mg.HeatStepper(N, 1.0, krylov=4)


def test_zero_problem_and_a_start_that_meets_the_tolerance(mg):
    N = 65
    s = mg.Solver(N, 1.0, krylov=8, rtol=1e-9)
    U, info = s.solve(np.zeros((N, N)), np.zeros((N, N)))
    assert info["converged"] and info["cycles"] == 0 and not info["breakdown"] and s.krylov_log() == []
    assert not U.any()
    F, U0 = problem(N, 14)
    U1, first = s.solve(F, U0)
    assert first["converged"] and first["cycles"] >= 1
    U2, again = s.solve(F, U1)
    assert again["converged"] and again["cycles"] == 0 and again["history"] == [first["res"]] and s.krylov_log() == []
    assert_bits(U2, U1, "a start that meets the tolerance is not touched")
    s.close()


def test_breakdown_stops_the_solve(mg):
    """g = <q, q> cannot vanish while r != 0 (A and the cycle are non-singular), so the flag guards against what is not a
    number: with a NaN in F the first g is NaN, alpha is 0, U keeps its bits and the solve ends after that iteration -- where
    the plain iteration runs all its cycles and returns NaN everywhere"""
    N = 64
    F, U0 = problem(N, 15)
    F[20, 30] = np.nan
    for m in (1, 4):
        s = mg.Solver(N, 1.0, krylov=m, rtol=1e-9)
        U, info = s.solve(F, U0)
        log = s.krylov_log()
        s.close()
        assert info["breakdown"] and not info["converged"] and info["cycles"] == 1 == len(log)
        assert log[0]["alpha"] == 0.0 and not log[0]["g"] > 0.0 and log[0]["restarted"] == (m == 1)
        assert_bits(U, U0, f"m={m}: U after a breakdown")


def test_lifecycle(mg, oracle):
    N = 100
    F, U0 = problem(N, 16)
    a = vref.field("smooth", N, seed=1)
    opts = dict(rtol=1e-9, max_cycles=10)

    def fresh(coef, m):
        f = mg.Solver(N, 1.0, coef=coef, krylov=m, **opts)
        U, info = f.solve(F, U0)
        f.close()
        return U, info["history"]

    s = mg.Solver(N, 1.0, **opts)
    s.set_krylov(2)
    s.set_coefficient(a)                        # the coefficient after the acceleration
    U, info = s.solve(F, U0)
    want = fresh(a, 2)
    assert_bits(U, want[0], "coefficient after krylov")
    assert info["history"] == want[1]
    s.set_krylov(8)                             # a larger m: more slots
    U, info = s.solve(F, U0)
    want = fresh(a, 8)
    assert_bits(U, want[0], "m replaced by a larger one")
    assert info["history"] == want[1]
    s.set_krylov(3)                             # and a smaller one on the storage it has
    U, info = s.solve(F, U0)
    want = fresh(a, 3)
    assert_bits(U, want[0], "m replaced by a smaller one")
    assert info["history"] == want[1] and len(s.krylov_log()) == info["cycles"]
    s.set_coefficient(None)                     # the constant operator under the same m
    U, info = s.solve(F, U0)
    want = fresh(None, 3)
    assert_bits(U, want[0], "coefficient removed")
    assert info["history"] == want[1]
    s.close()
    s.close()
    t = mg.Solver(N, 1.0, coef=a, **opts)       # krylov after the coefficient
    t.set_krylov(2)
    U, info = t.solve(F, U0)
    want = fresh(a, 2)
    assert_bits(U, want[0], "krylov after the coefficient")
    del t


def test_torch_tensors_on_a_side_stream():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_solve_krylov_torch_worker.py")], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "SOLVE_KRYLOV_TORCH OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
