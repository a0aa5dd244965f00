"""The semilinear solve (include/mg_newton.h) on the GPU: the pass alone in both forms, bit for bit against the restatement
(tests/_newton_ref.py) and inside guard bands; whole Newton solves against the restatement, iterate by iterate; the driver
against the caller's own loop over its building blocks; all three kinds against a dense longdouble Newton solution; the hard
starts; a discontinuous weight under GCR; the solver's state after a call; the refusals.  Bit comparisons of whole solves follow
the qualification rule of DESIGN.md 4.3: the coarse margins of the restatement are asserted first."""
import numpy as np
import pytest

import _guard
import _newton_ref as nref
import _reaction_ref as rref
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
LD = np.longdouble


def lib_table(mg):
    return lambda N, M: mg.restriction_table(N, M)


def need_exp_bits(mg, kind):
    """sinh and exp go through exp_libm, which equals the host's exp() where the engine's self-check says so"""
    if kind != "cubic" and mg.lib().mg_source_is_bit_identical() != 1:
        pytest.skip("exp_libm does not reproduce this host's libm bit for bit (mg_source_is_bit_identical() != 1)")


# ---------------------------------------------------------------- the pass alone, inside guard bands
def pass_inputs(N):
    """U of order one with a -0.0 on the rim, a step of order 100 for t = 2^-9, a weight over six decades with exact zeros"""
    rng = np.random.default_rng(50 + N)
    U = 2.0 * rng.random((N, N)) - 1.0
    U[0, 1] = -0.0
    U[N - 1, N - 2] = -0.0
    dlt = 100.0 * rng.standard_normal((N, N))
    w = 10.0 ** (6.0 * rng.random((N, N)) - 3.0)
    w[::3, ::5] = 0.0
    F = 50.0 * rng.standard_normal((N, N))
    return U, dlt, w, F


# one interior point; block and row-tile edges; the second column block of both lane shapes (257, 258 / 514, 770, 1026);
# the first pair size (512); the first non-temporal size (4096)
@pytest.mark.parametrize("kind", nref.KINDS)
@pytest.mark.parametrize("weight", [False, True])
@pytest.mark.parametrize("coef", [None, "random"])
@pytest.mark.parametrize("N", [3, 4, 5, 17, 24, 255, 256, 257, 258, 511, 512, 514, 770, 1026, 4096])
def test_pass_alone_bit_for_bit_inside_guard_bands(mg, N, coef, weight, kind):
    need_exp_bits(mg, kind)
    L, shift, kappa, t = 1.0, (1e4 if N % 2 else 0.0), 3.7, 2.0 ** -9
    a = None if coef is None else vref.field(coef, N, seed=N)
    U, dlt, w, F = pass_inputs(N)
    if not weight:
        w = None
    what = f"N={N} {kind} a={coef} w={weight}"
    with _guard.block(mg, [N] * 8, "odd16" if N % 4 == 2 else "page") as gb:
        ga, gw, gU, gdlt, gF, gV, gD, gS = gb.views
        ga.upload(a if a is not None else np.ones((N, N))), gw.upload(w if w is not None else np.ones((N, N)))
        gU.upload(U), gdlt.upload(dlt), gF.upload(F)
        da, dw = (ga if a is not None else None), (gw if w is not None else None)

        def run(name, Ug, step, want):
            gV.poison(), gD.poison(), gS.poison()
            gb.expect_readonly(*([ga, gw, gU, gdlt, gF] + ([] if step else [gV])))
            norm = mg.nonlinear_residual(N, L, shift, da, kind, kappa, dw, Ug, gF, gD, gS, dlt=gdlt if step else None, t=t,
                                         V=gV if step else None)
            gb.check(f"{name} {what}")
            got = (gV.to_host() if step else None, gD.to_host(), gS.to_host(), norm)
            for g, x, label in zip(got, want, ("V", "D", "S")):
                if g is not None:
                    assert_bits(g, x, f"{name} {what}: {label}")
            assert norm == want[3], (name, what, norm, want[3])
            return got

        run("no step", gU, False, nref.residual(N, L, a, kind, kappa, w, U, F, shift))
        want = nref.residual(N, L, a, kind, kappa, w, U, F, shift, dlt, t)
        V, D, S, norm = run("step", gU, True, want)
        # the step form is numpy's U + t*dlt (U's own rim, -0.0 included) followed by the no-step form
        Vn = U.copy()
        Vn[1:-1, 1:-1] = U[1:-1, 1:-1] + t * dlt[1:-1, 1:-1]
        assert_bits(V, Vn, f"{what}: V against numpy")
        assert np.signbit(V[0, 1]) and np.signbit(V[N - 1, N - 2])
        gU.upload(Vn)
        run("no step on the trial", gU, False, (None, D, S, norm))


# ---------------------------------------------------------------- whole solves against the restatement
def whole_solve_against_restatement(mg, oracle, N, coef, kind):
    """a smooth weight at kappa = 10, inner solves of two cycles (unconverged: their steps are used and counted), three Newton
    iterations: U after every iteration, the Newton history and the status with ==.  (tests/_newton_ref.py on the CPU: three
    iterations are accepted without a backtrack for every kind at every size used here, |u| of order one.)"""
    need_exp_bits(mg, kind)
    F, U0 = nref.problem(N)
    a, w, kappa = (None if coef is None else vref.field(coef, N)), nref.smooth_weight(N), 10.0
    inner = dict(rtol=0.0, max_cycles=2)
    margins, Us = [], []
    want = nref.newton(oracle, a, kind, kappa, w, F, U0, 1.0, table=lib_table(mg), margins=margins, keep=Us, rtol=0.0,
                       max_iters=3, inner=inner)
    ref.assert_qualified(margins, f"N={N} a={coef} {kind}")
    assert want["iterations"] == 3 and len(Us) == 3
    solver = mg.Solver(N, 1.0, coef=a, **inner)
    for k in (1, 2, 3):
        got, info = solver.newton(F, U0, kind=kind, kappa=kappa, weight=w, rtol=0.0, max_iters=k)
        assert_bits(got, Us[k - 1], f"N={N} a={coef} {kind}: U after Newton iteration {k}")
        assert info["history"] == want["history"][:k + 1], (info["history"], want["history"])
        assert info["status"] == nref.NOT_CONVERGED and info["iterations"] == k and not solver.has_reaction
        for s, x in zip(info["steps"], want["steps"]):
            assert (s["res"], s["t"], s["backtracks"], s["inner_cycles"], s["inner_converged"]) == \
                (x["res"], x["t"], x["backtracks"], x["inner_cycles"], x["inner_converged"]), (s, x)
    solver.close()


@pytest.mark.parametrize("N,coef", [(33, None), (33, "exp"), (100, None), (100, "exp"), (257, None), (257, "exp"), (514, "exp")])
def test_whole_solves_bit_identical_to_restatement(mg, oracle, N, coef):
    """cubic: no exp in it, so it runs on every host"""
    whole_solve_against_restatement(mg, oracle, N, coef, "cubic")


@pytest.mark.parametrize("kind", ["sinh", "exp"])
@pytest.mark.parametrize("N,coef", [(33, None), (257, "exp"), (514, "exp")])
def test_whole_solves_of_sinh_and_exp_bit_identical_to_restatement(mg, oracle, N, coef, kind):
    """the kinds that go through exp_libm, |v| of order one (the verified path), where the engine's self-check vouches for the
    host libm's bits: one column per lane (33, 257) and column pairs (514)"""
    whole_solve_against_restatement(mg, oracle, N, coef, kind)


def test_hard_cubic_start_reproduces_the_backtrack_sequence(mg, oracle):
    """F == -1e6 from U = 0 at N = 33: U, the history and every step's t, backtracks and inner cycles equal the restatement's;
    the backtracks are 9, 3, 0, ..."""
    N = 33
    F = np.full((N, N), nref.HARD_STARTS["cubic"])
    margins = []
    want = nref.newton(oracle, None, "cubic", 1.0, None, F, None, 1.0, table=lib_table(mg), margins=margins)
    ref.assert_qualified(margins, "hard cubic start")
    U, info = mg.solve_semilinear(F, kind="cubic", kappa=1.0)
    bt = [s["backtracks"] for s in info["steps"]]
    print("backtracks", bt, "inner cycles", [s["inner_cycles"] for s in info["steps"]], "history", info["history"])
    assert bt[:3] == [9, 3, 0] and not any(bt[2:]) and info["converged"] and info["status"] == nref.CONVERGED
    assert bt == [s["backtracks"] for s in want["steps"]] and [s["t"] for s in info["steps"]] == [s["t"] for s in want["steps"]]
    assert [s["inner_cycles"] for s in info["steps"]] == [s["inner_cycles"] for s in want["steps"]]
    assert info["history"] == want["history"] and info["iterations"] == want["iterations"]
    assert_bits(U, want["U"], "hard cubic start: U")


# ---------------------------------------------------------------- composition
@pytest.mark.parametrize("kind", nref.KINDS)
@pytest.mark.parametrize("N", [65, 514])
def test_newton_is_the_callers_own_loop(mg, N, kind):
    """Solver.newton against the loop a caller writes from nonlinear_residual, set_reaction, solve on a zero delta and the step
    form: U, the history and the steps, bit for bit (device against device: no libm in it)"""
    F, U0 = nref.problem(N)
    a, w, kappa = vref.field("exp", N), nref.smooth_weight(N), 10.0
    opts = dict(rtol=1e-8, max_iters=6, max_backtracks=12)
    inner = dict(rtol=1e-3, max_cycles=4)
    solver = mg.Solver(N, 1.0, coef=a, **inner)
    U, info = solver.newton(F, U0, kind=kind, kappa=kappa, weight=w, **opts)
    assert info["iterations"] >= 2

    G = mg.DeviceGrid
    ga, gw, gF = G.from_host(a), G.from_host(w), G.from_host(F)
    cur, oth, D, D2, S, S2, dlt = G.from_host(U0), G((N, N)), G((N, N)), G((N, N)), G((N, N)), G((N, N)), G((N, N))
    r = mg.nonlinear_residual(N, 1.0, 0.0, ga, kind, kappa, gw, cur, gF, D, S)
    tol, history, steps = max(0.0, opts["rtol"] * r), [r], []
    while not (r <= tol) and len(history) - 1 < opts["max_iters"]:
        solver.set_reaction(S)
        mg.lib().mg_fill_zero(dlt.ptr, dlt.size)
        _, lin = solver.solve(D, dlt)
        solver.set_reaction(None)
        t, bt = 1.0, 0
        while True:
            rt = mg.nonlinear_residual(N, 1.0, 0.0, ga, kind, kappa, gw, cur, gF, D2, S2, dlt=dlt, t=t, V=oth)
            if np.isfinite(rt) and rt < (1.0 - 1e-4 * t) * r:
                break
            bt, t = bt + 1, 0.5 * t
            assert bt <= opts["max_backtracks"]
        cur, oth, D, D2, S, S2, r = oth, cur, D2, D, S2, S, rt
        history.append(r)
        steps.append((r, t, bt, lin["cycles"], lin["converged"]))
    assert_bits(U, cur.to_host(), f"N={N} {kind}: U")
    assert info["history"] == history and info["converged"] == (r <= tol)
    assert [(s["res"], s["t"], s["backtracks"], s["inner_cycles"], s["inner_converged"]) for s in info["steps"]] == steps
    solver.close()


@pytest.mark.parametrize("coef", [None, "exp"])
@pytest.mark.parametrize("N", [65, 100])
def test_kappa_zero_is_the_linear_solve(mg, N, coef):
    """kappa = 0 from U = 0: one Newton step, U and the inner history those of Solver.solve(F).  N = 65 (nested levels): the
    whole array.  N = 100: the linear solve's prolongation leaves rounding-sized values on the rim of its U, which the Newton
    step does not carry over (include/mg_newton.h: the rim of V is the rim of U) -- the interior with ==, the rim the start's."""
    F = ref.random_problem(N, 77)[0]
    a = None if coef is None else vref.field(coef, N)
    want_U, want = mg.solve(F, coef=a)
    for kind in nref.KINDS:
        U, info = mg.solve_semilinear(F, kind=kind, kappa=0.0, coef=a)
        if N == 65:
            assert_bits(U, want_U, f"N={N} {kind} a={coef}: U")
        assert_bits(U[1:-1, 1:-1], want_U[1:-1, 1:-1], f"N={N} {kind} a={coef}: the interior of U")
        assert_bits(ref.rim_only(U), np.zeros((N, N)), f"N={N} {kind} a={coef}: the rim of U")
        assert info["iterations"] == 1 and info["converged"] and info["steps"][0]["t"] == 1.0
        assert info["last_inner_history"] == want["history"] and info["steps"][0]["inner_cycles"] == want["cycles"]
        assert info["res0"] == want["res0"]


# ---------------------------------------------------------------- truth, and the hard starts
@pytest.mark.parametrize("kind", nref.KINDS)
def test_all_kinds_converge_onto_the_dense_solution(mg, kind):
    """N = 65, a = exp, a smooth weight, the defaults: converged within 20 iterations and
    max|U - X| <= ||A^-1||_inf * (||N(U)||_inf + ||N(X)||_inf), the bound of tests/test_newton_cpu.py"""
    N, L, shift, kappa = 65, 1.5, 2.0, 10.0
    F, U0 = nref.problem(N, L)
    a, w = vref.field("exp", N, L), nref.smooth_weight(N, L)
    U, info = mg.solve_semilinear(F, U0, L, kind=kind, kappa=kappa, weight=w, coef=a, shift=shift)
    assert info["converged"] and info["iterations"] <= 20, info["history"]
    X, nA = nref.dense_newton(a, kind, kappa, w, F, U, L, shift, iters=8, chord=True)
    rU = np.max(np.abs(nref.residual_ld(a, kind, kappa, w, U, F, L, shift)))
    rX = np.max(np.abs(nref.residual_ld(a, kind, kappa, w, X, F, L, shift)))
    err = np.max(np.abs(U.astype(LD) - X))
    bound = nA * (rU + rX) * (1 + LD(1e-6))
    print(f"{kind}: {info['iterations']} iterations, {info['inner_cycles']} inner cycles, |U-X| {float(err):.3e} <= {float(bound):.3e} "
          f"(N(U) {float(rU):.3e}, N(X) {float(rX):.3e})")
    assert err <= bound


@pytest.mark.parametrize("kind", ["sinh", "exp"])
def test_hard_starts_converge_with_backtracking(mg, kind):
    """F == -1e4 from U = 0 at N = 65: full steps overflow g (a norm that is not finite is a rejection); converged within 20
    iterations with at least one backtrack"""
    N = 65
    U, info = mg.solve_semilinear(np.full((N, N), nref.HARD_STARTS[kind]), kind=kind, kappa=1.0)
    bt = [s["backtracks"] for s in info["steps"]]
    print(f"{kind}: backtracks {bt}, history {info['history']}")
    assert info["converged"] and info["iterations"] <= 20 and sum(bt) >= 1 and np.all(np.isfinite(U))
    h = info["history"]
    assert all(h[i + 1] < h[i] for i in range(len(h) - 1))


# ---------------------------------------------------------------- a discontinuous weight; the solver's state
def test_halfplane_weight_converges_under_gcr(mg):
    """w = 1e5 on x >= 0.37 at N = 129, sinh: every Newton matrix has the reaction the plain cycle is slow on; with krylov=8
    the solve converges"""
    N = 129
    F, U0 = nref.problem(N)
    w = rref.field("halfplane", N)
    U, info = mg.solve_semilinear(F, U0, kind="sinh", kappa=1.0, weight=w, krylov=8, max_cycles=60)
    print(f"halfplane: {info['iterations']} iterations, inner {[s['inner_cycles'] for s in info['steps']]}, history {info['history']}")
    assert info["converged"] and info["iterations"] <= 20 and all(s["inner_converged"] for s in info["steps"])


@pytest.mark.parametrize("outcome", ["converged", "stalled", "iteration cap"])
def test_solver_has_no_reaction_afterwards_and_solves_as_a_fresh_one(mg, outcome):
    N = 100
    F, U0 = nref.problem(N)
    a = vref.field("exp", N)
    opts = dict(rtol=1e-9, max_cycles=5)
    want = mg.solve(F, U0, coef=a, **opts)
    solver = mg.Solver(N, 1.0, coef=a, **opts)
    if outcome == "stalled":
        _, info = solver.newton(np.full((N, N), -1e6), kind="cubic", max_backtracks=1)
        assert info["stalled"] and info["status"] == nref.STALLED
    else:
        _, info = solver.newton(F, U0, kind="exp", kappa=5.0, max_iters=20 if outcome == "converged" else 1)
        assert info["converged"] == (outcome == "converged")
    assert not solver.has_reaction and solver.has_coefficient
    got = solver.solve(F, U0)
    assert_bits(got[0], want[0], f"after a Newton call ({outcome}): U")
    for key in ("history", "cycles", "status", "converged", "res0", "res", "ref_norm"):
        assert got[1][key] == want[1][key], key
    solver.close()


# ---------------------------------------------------------------- refusals, the stalled line search, max_iters = 0
def test_refusals_leave_the_solver_and_U_as_they_were(mg):
    N = 64
    F, U0 = nref.problem(N)
    opts = dict(rtol=0.0, max_cycles=1)
    s = mg.Solver(N, 1.0, **opts)
    want = s.solve(F, U0)
    Ud = mg.DeviceGrid.from_host(U0)

    def same_after(what):
        assert_bits(Ud.to_host(), U0, what + ": U untouched")
        got = s.solve(F, U0)
        assert_bits(got[0], want[0], what + ": the next solve")
        assert got[1]["history"] == want[1]["history"] and not s.has_reaction

    for kappa in (-1.0, float("nan"), float("inf")):
        with pytest.raises(mg.MGError, match=r"\[2\].*kappa"):
            s.newton(F, Ud, kind="cubic", kappa=kappa)
        same_after(f"kappa = {kappa}")
    with pytest.raises(mg.MGError, match=r"\[2\].*unknown kind"):
        s.newton(F, Ud, kind=7)
    with pytest.raises(mg.MGError, match="kind"):
        s.newton(F, Ud, kind="tanh")
    same_after("an unknown kind")
    for value, what in ((-1.0, "negative"), (float("nan"), "not finite"), (float("inf"), "not finite")):
        w = np.ones((N, N))
        w[N - 1, 3] = value                    # (a rim point: the rim is part of the array)
        with pytest.raises(mg.MGError, match=r"\[2\].*w must be finite.*" + what):
            s.newton(F, Ud, kind="cubic", weight=w)
        same_after(f"w = {value}")
    g = mg.DeviceGrid.zeros((N + 1, N))        # a pointer 8 bytes past a 16-byte boundary
    for args in ((g.ptr + 8, Ud.ptr, None), (Ud.ptr, g.ptr + 8, None), (g.ptr, Ud.ptr, g.ptr + 8)):
        with pytest.raises(mg.MGError, match=r"\[2\].*16-byte aligned"):
            s.newton_ptr(args[0], args[1], kind="cubic", w_ptr=args[2])
    with pytest.raises(mg.MGError, match=r"\[2\].*NULL"):
        s.newton_ptr(None, Ud.ptr)
    assert mg.lib().mg_solver_newton(None, 0, 1.0, None, g.ptr, Ud.ptr, None, None) == 2
    with pytest.raises(mg.MGError, match=r"\[2\].*NULL"):
        mg._check()
    g.free()
    same_after("misaligned and NULL arrays")
    for bad in (dict(rtol=-1.0), dict(atol=float("nan")), dict(max_iters=-1), dict(max_backtracks=-1)):
        with pytest.raises(mg.MGError, match=r"\[2\].*max_iters"):
            s.newton(F, Ud, kind="cubic", **bad)
    for shape in (np.ones((N, N + 1)), np.ones((N - 1, N - 1))):
        with pytest.raises(mg.MGError, match="shape"):
            s.newton(shape, Ud)
    same_after("options and shapes")
    s.close()

    s = mg.Solver(N, 1.0, reaction=rref.field("smooth", N), **opts)   # the caller has a reaction set
    want = s.solve(F, U0)
    with pytest.raises(mg.MGError, match=r"\[3\].*reaction term is set"):
        s.newton(F, Ud, kind="cubic")
    assert s.has_reaction
    got = s.solve(F, U0)
    assert_bits(got[0], want[0], "after the refusal with a reaction set")
    s.close()
    s = mg.Solver(N, 1.0, bc="ndnd", **opts)
    with pytest.raises(mg.MGError, match=r"\[3\].*Neumann"):
        s.newton(F, Ud, kind="cubic")
    assert s.boundary == (1, 0, 1, 0)
    s.close()
    s = mg.Solver(N, 1.0, fmg=1, **opts)
    with pytest.raises(mg.MGError, match=r"\[3\].*fmg"):
        s.newton(F, Ud, kind="cubic")
    s.close()
    assert_bits(Ud.to_host(), U0, "U after every refusal")
    for cls, args in ((mg.BatchSolver, (N, 1.0, 2)), (mg.HeatStepper, (N, 1.0))):   # (out of scope: no Newton there)
        assert not hasattr(cls, "newton")


def test_stalled_line_search_and_zero_iterations(mg):
    """max_backtracks = 0 on the F == -1e6 start: the one trial is rejected, the status says stalled and U is unchanged;
    max_iters = 0 returns the start's norm and runs no solve"""
    N = 33
    F = np.full((N, N), nref.HARD_STARTS["cubic"])
    U0 = ref.rim_only(0.25 * np.ones((N, N)))
    r0 = nref.residual(N, 1.0, None, "cubic", 1.0, None, U0, F)[3]
    s = mg.Solver(N, 1.0)
    U, info = s.newton(F, U0, kind="cubic", max_backtracks=0)
    assert info["status"] == nref.STALLED and info["stalled"] and not info["converged"] and info["iterations"] == 0
    assert info["res0"] == info["res"] == r0 and info["trials"] == 1 and info["history"] == [r0]
    assert len(info["steps"]) == 1 and info["steps"][0]["backtracks"] == 1 and info["steps"][0]["t"] == 0.0
    assert_bits(U, U0, "stalled: U unchanged")
    U, info = s.newton(F, U0, kind="cubic", max_iters=0)
    assert info["status"] == nref.NOT_CONVERGED and info["iterations"] == 0 and info["inner_cycles"] == 0 and info["trials"] == 0
    assert info["res0"] == info["res"] == r0 and info["steps"] == [] and info["history"] == [r0]
    assert_bits(U, U0, "max_iters = 0: U unchanged")
    assert not s.has_reaction
    s.close()
