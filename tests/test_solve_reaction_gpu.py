"""The variable reaction term (include/mg_reaction.h) on the GPU: every kernel and every form alone, bit for bit against the
restatement (tests/_reaction_ref.py) and inside guard bands; the coarse solve alone; whole solves against the restatement,
cycle by cycle, U and history; the two identity contracts; state handling; the Krylov acceleration on the case it is for; the
returned U against a dense direct solution; the refusals.  Bit comparisons follow the qualification rule of DESIGN.md 4.3:
the coarse margin of the restatement is asserted first."""
import numpy as np
import pytest

import _guard
import _reaction_ref as rref
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
LD = np.longdouble


def lib_table(mg):
    return lambda N, M: mg.restriction_table(N, M)


def coefficient(coef, N, L=1.0):
    return None if coef is None else vref.field(coef, N, L)


def reaction_for_kernels(N):
    """values over six decades with exact zeros among them: sd + s*dx2 takes every path of the centre"""
    s = 10.0 ** (6.0 * np.random.default_rng(N).random((N, N)))
    s[::3, ::5] = 0.0
    return s


# ---------------------------------------------------------------- kernels alone, inside guard bands
# one interior point; block and row-tile edges; the second column block of both lane shapes (257, 258 / 514, 770, 1026);
# the first pair size (512); the first non-temporal size (4096)
@pytest.mark.parametrize("coef", [None, "random"])
@pytest.mark.parametrize("N", [3, 4, 5, 17, 24, 255, 256, 257, 258, 511, 512, 514, 770, 1026, 4096])
def test_kernels_alone_bit_for_bit_inside_guard_bands(mg, N, coef):
    L, shift, omega = 1.0, (1e4 if N % 2 else 0.0), 0.8
    a = None if coef is None else vref.field(coef, N, seed=N)
    s = reaction_for_kernels(N)
    F, U = ref.random_problem(N, 10 * N + 1)
    with _guard.block(mg, [N, N, N, N, N], "odd16" if N % 4 == 2 else "page") as gb:
        ga, gs, gU, gF, gout = gb.views
        ga.upload(a if a is not None else np.ones((N, N))), gs.upload(s), gU.upload(U), gF.upload(F)
        da = ga if a is not None else None

        def run(what, call, want):
            gout.poison()
            gb.expect_readonly(ga, gs, gU, gF)
            call()
            gb.check(f"{what} N={N} a={coef}")
            assert_bits(gout.to_host(), want, f"{what} N={N} a={coef}")

        run("sweep", lambda: mg.sweepReaction(N, L, shift, omega, da, gs, gU, gF, gout), rref.sweep(N, L, a, s, U, F, omega, shift))
        run("zero-start sweep", lambda: mg.sweepReaction(N, L, shift, omega, da, gs, None, gF, gout),
            rref.sweep(N, L, a, s, None, F, omega, shift, zero_start=True))
        for sign in (+1, -1):
            run(f"residual sign {sign}", lambda: mg.residualReaction(N, L, shift, da, gs, gU, gF, gout, sign),
                rref.residual(N, L, a, s, U, F, shift, sign))
        run("operator", lambda: mg.applyOperatorReaction(N, L, shift, da, gs, gU, gout), rref.apply_operator(N, L, a, s, U, shift))


# ---------------------------------------------------------------- the coarse solve alone
def _qualified_seed(N, L, a, s, atol, rtol, cap, shift):
    """the first seed whose right-hand side the restatement stops on with a qualified margin"""
    for seed in range(400 + N, 420 + N):
        F = ref.random_problem(N, seed)[0]
        tr = rref.rbgs_trace(N, L, a, s, F, atol, rtol, cap, shift)
        if vref.coarse_margin(tr, atol, rtol) >= ref.QUALIFY:
            return F, tr
    raise AssertionError(f"no qualified seed for N={N}")


@pytest.mark.parametrize("coef", [None, "exp"])
@pytest.mark.parametrize("N", [8, 9, 33, 63])
def test_coarse_solve_alone(mg, N, coef):
    """U and the iteration count against rbgs_trace; 33 and 63 put 2 and 4 points on a thread"""
    L, shift, atol, rtol, cap = 1.0, 3.0, 0.0, 1e-2, 100000
    a = coefficient(coef, N)
    s = rref.field("blob", N) + rref.field("halfplane", N) * 1e-2
    F, tr = _qualified_seed(N, L, a, s, atol, rtol, cap, shift)
    ref.assert_qualified([vref.coarse_margin(tr, atol, rtol)], f"N={N} a={coef}")
    with _guard.block(mg, [N, N, N, N], "page" if N % 2 else "odd16") as gb:
        ga, gs, gF, gout = gb.views
        ga.upload(a if a is not None else np.ones((N, N))), gs.upload(s), gF.upload(F)
        gout.poison()
        gb.expect_readonly(ga, gs, gF)
        iters = mg.coarseSolveReaction(N, L, shift, ga if a is not None else None, gs, gF, atol, rtol, cap, gout)
        gb.check(f"coarseSolveReaction N={N} a={coef}")
        assert_bits(gout.to_host(), tr[0], f"coarse solve N={N} a={coef}")
        assert iters == len(tr[2]), (iters, len(tr[2]))


# ---------------------------------------------------------------- whole solves against the restatement
def _as_input(mg, kind, s):
    """s as the three things set_reaction takes; returns (input, release)"""
    if kind == "numpy":
        return s, lambda: None
    if kind == "grid":
        g = mg.DeviceGrid.from_host(s)
        return g, g.free
    torch = pytest.importorskip("torch")
    t = torch.from_numpy(s).cuda()
    torch.cuda.synchronize()
    return t, lambda: None


@pytest.mark.parametrize("coef", [None, "exp"])
@pytest.mark.parametrize("name", rref.FIELDS)
@pytest.mark.parametrize("N", [33, 100, 257, 514, 1026])
def test_whole_solves_bit_identical_to_restatement(mg, oracle, N, name, coef):
    """cycles 1, 2, 3 at rtol = 0: U and the whole history with ==; s is given once as a numpy array, once as a DeviceGrid
    and once as a torch tensor"""
    F, U0 = ref.random_problem(N, 3000 + N)
    a, s = coefficient(coef, N), rref.field(name, N)
    margins, Us = [], []
    _, hist, _, _ = rref.solve(oracle, a, s, F, U0, 1.0, margins=margins, table=lib_table(mg), engine_norms=True, keep=Us,
                               rtol=0.0, max_cycles=3)
    ref.assert_qualified(margins, f"N={N} s={name} a={coef}")
    for k, kind in ((1, "numpy"), (2, "grid"), (3, "torch")):
        sin, release = _as_input(mg, kind, s)
        solver = mg.Solver(N, 1.0, coef=a, reaction=sin, rtol=0.0, max_cycles=k)
        release()
        assert solver.has_reaction and solver.has_coefficient == (a is not None)
        got, info = solver.solve(F, U0)
        solver.close()
        assert_bits(got, Us[k - 1], f"N={N} s={name} a={coef}: U after cycle {k} (s as {kind})")
        assert info["cycles"] == k and not info["converged"]
        assert info["history"] == hist[:k + 1], (info["history"], hist[:k + 1])


# ---------------------------------------------------------------- the two identity contracts
def _same(got, want, what):
    assert_bits(got[0], want[0], what + ": U")
    for key in ("history", "cycles", "status", "converged", "coarse_capped", "res0", "res", "ref_norm"):
        assert got[1][key] == want[1][key], (what, key)


@pytest.mark.parametrize("coef", [None, "exp"])
@pytest.mark.parametrize("N", [65, 514])
def test_identity_contracts(mg, N, coef):
    """s == 0 is the solver without a reaction; s == 1e3 at shift 0 is Solver(shift=1e3): U, history, cycles and flags"""
    F, U0 = ref.random_problem(N, 5000 + N)
    a = coefficient(coef, N)
    opts = dict(rtol=1e-7, max_cycles=4)
    for shift in (0.0, 50.0):
        want = mg.solve(F, U0, coef=a, shift=shift, **opts)
        got = mg.solve(F, U0, coef=a, shift=shift, reaction=np.zeros((N, N)), **opts)
        _same(got, want, f"s == 0, N={N} a={coef} shift={shift}")
    want = mg.solve(F, U0, coef=a, shift=1e3, **opts)
    got = mg.solve(F, U0, coef=a, reaction=np.full((N, N), 1e3), **opts)
    _same(got, want, f"s == 1e3, N={N} a={coef}")


# ---------------------------------------------------------------- state handling
def test_set_remove_order_and_reuse(mg):
    N = 100
    F, U0 = ref.random_problem(N, 6000)
    a, s1, s2 = vref.field("exp", N), rref.field("smooth", N), rref.field("blob", N)
    opts = dict(rtol=0.0, max_cycles=2)
    plain = mg.solve(F, U0, **opts)
    with_a = mg.solve(F, U0, coef=a, **opts)
    both = mg.solve(F, U0, coef=a, reaction=s1, **opts)
    only_s = mg.solve(F, U0, reaction=s1, **opts)
    assert not np.array_equal(both[0], with_a[0]) and not np.array_equal(only_s[0], plain[0])

    s = mg.Solver(N, 1.0, **opts)
    assert not s.has_reaction
    g = mg.DeviceGrid.from_host(s1)
    s.set_reaction(g)
    g.free()                                   # the caller's array is not kept
    junk = mg.DeviceGrid.from_host(np.full((N, N), -7.0))
    _same(s.solve(F, U0), only_s, "reaction alone")
    junk.free()
    s.set_coefficient(a)                       # reaction first, coefficient second
    _same(s.solve(F, U0), both, "set_reaction, then set_coefficient")
    s.set_reaction(None)
    assert not s.has_reaction and s.has_coefficient
    _same(s.solve(F, U0), with_a, "set_reaction(None) restores the coefficient solver")
    s.set_reaction(s1)                         # coefficient first, reaction second
    _same(s.solve(F, U0), both, "set_coefficient, then set_reaction")
    s.set_reaction(s2)
    _same(s.solve(F, U0), mg.solve(F, U0, coef=a, reaction=s2, **opts), "a replaced reaction")
    s.set_reaction(s1)
    bad = s2.copy()
    bad[N - 1, 3] = -1.0                       # (a rim point: the rim is part of the array)
    with pytest.raises(mg.MGError, match=r"\[2\].*negative or not finite"):
        s.set_reaction(bad)
    assert s.has_reaction
    _same(s.solve(F, U0), both, "after a refused array")
    s.set_coefficient(None)
    _same(s.solve(F, U0), only_s, "set_coefficient(None) keeps the reaction")
    s.set_reaction(None)
    _same(s.solve(F, U0), plain, "both removed: the plain solver")
    s.close()


# ---------------------------------------------------------------- Krylov acceleration
def test_halfplane_needs_and_gets_gcr(mg, oracle):
    """s = 1e5 on x >= 0.37 at N = 129: the plain solver is not converged after 40 cycles, GCR(8) converges within 60
    iterations to rtol 1e-9 with a history that never grows; the log replays to the same U and history"""
    N, m = 129, 8
    F, U0 = ref.random_problem(N, 11)
    s = rref.field("halfplane", N)
    _, plain = mg.solve(F, U0, reaction=s, rtol=1e-9, max_cycles=40)
    assert not plain["converged"] and plain["cycles"] == 40
    opts = dict(rtol=1e-9, max_cycles=60)
    solver = mg.Solver(N, 1.0, reaction=s, krylov=m, **opts)
    U, info = solver.solve(F, U0)
    log = solver.krylov_log()
    solver.close()
    h = info["history"]
    print(f"halfplane N={N}: plain {plain['res'] / plain['ref_norm']:.3e} of ||F|| after 40 cycles; GCR({m}) {info['cycles']} iterations")
    assert info["converged"] and info["cycles"] <= 60 and not info["breakdown"]
    assert all(h[i + 1] <= h[i] for i in range(len(h) - 1)), h
    margins = []
    out = rref.krylov_solve(oracle, None, s, F, U0, 1.0, m=m, log=log, margins=margins, table=lib_table(mg), **opts)
    ref.assert_qualified(margins, "halfplane GCR")
    assert info["cycles"] == len(log) == out["cycles"] and out["converged"] and not out["breakdown"]
    assert_bits(U, out["U"], "GCR: U against the replay")
    assert h[1:] == out["history"][1:] and info["res"] == h[-1]
    assert h[0] == rref.residual_norm(N, 1.0, None, s, U0, F, engine=True)
    for e, rec in zip(log, out["records"]):    # the replay's own sums agree with the logged ones
        assert e["alpha"] == rec["alpha"]
        if e["restarted"]:
            assert abs(e["rho"] - rec["rho_own"]) <= 1e-12 * rec["rho_own"]
    # krylov first, reaction second: the same solve
    solver = mg.Solver(N, 1.0, krylov=m, **opts)
    solver.set_reaction(s)
    U2, info2 = solver.solve(F, U0)
    solver.close()
    _same((U2, info2), (U, info), "set_krylov, then set_reaction")


# ---------------------------------------------------------------- truth
@pytest.mark.parametrize("coef", [None, "exp"])
@pytest.mark.parametrize("name", ["smooth", "blob", "random"])
def test_against_the_direct_solution(mg, name, coef):
    """N = 65 to rtol 1e-10: max|U - X| <= ||A^-1||_inf * (||r(U)||_inf + ||r(X)||_inf), residuals in longdouble (the bound
    of tests/test_solve_reaction_cpu.py, with its 1e-6 for the fp64 inverse)"""
    N, L, shift = 65, 1.5, 2.0
    F, U0 = ref.random_problem(N, 7000 + N)
    a, s = coefficient(coef, N, L), rref.field(name, N, L)
    U, info = mg.solve(F, U0, L, coef=a, reaction=s, shift=shift, rtol=1e-10, max_cycles=60)
    assert info["converged"], info["cycles"]
    X, nA = rref.direct_solution(a, s, F, U0, L, shift)
    rU = np.max(np.abs(rref.residual_ld(a, s, U, F, L, shift)))
    rX = np.max(np.abs(rref.residual_ld(a, s, X, F, L, shift)))
    err = np.max(np.abs(U.astype(LD) - X))
    bound = nA * (rU + rX) * (1 + LD(1e-6))
    print(f"s={name} a={coef}: {info['cycles']} cycles, |U-X| {float(err):.3e} <= {float(bound):.3e}")
    assert err <= bound


@pytest.mark.parametrize("N", [257, 1025])
def test_smooth_field_converges_at_size(mg, N):
    """rtol 1e-9 on the smooth field; the count is printed (recorded in DESIGN.md 4.3.10), not pinned"""
    F, U0 = ref.random_problem(N, 11)
    U, info = mg.solve(F, U0, reaction=rref.field("smooth", N), rtol=1e-9)
    print(f"N={N} s=smooth: {info['cycles']} cycles, res/||F|| {info['res'] / info['ref_norm']:.3e}")
    assert info["converged"]


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_solver_as_it_was(mg):
    N = 64
    F, U0 = ref.random_problem(N, 8000)
    good = rref.field("smooth", N)
    opts = dict(rtol=0.0, max_cycles=1)
    s = mg.Solver(N, 1.0, reaction=good, **opts)
    want = s.solve(F, U0)
    for value, what in ((-1.0, "negative"), (-1e-300, "negative"), (float("nan"), "not finite"), (float("inf"), "not finite")):
        bad = good.copy()
        bad[17, 40] = value
        with pytest.raises(mg.MGError, match=r"\[2\].*" + what):
            s.set_reaction(bad)
        assert s.has_reaction
        _same(s.solve(F, U0), want, f"after s = {value}")
        with pytest.raises(mg.MGError, match=r"\[2\]"):
            mg.Solver(N, 1.0, reaction=bad)
    g = mg.DeviceGrid.zeros((N + 1, N))        # a pointer 8 bytes past a 16-byte boundary
    assert mg.lib().mg_solver_set_reaction(s._s, g.ptr + 8) == 2
    with pytest.raises(mg.MGError, match=r"\[2\].*16-byte aligned"):
        mg._check()
    g.free()
    _same(s.solve(F, U0), want, "after a misaligned pointer")
    for shape in (np.ones((N, N + 1)), np.ones((N - 1, N - 1))):
        with pytest.raises(mg.MGError, match="reaction.*shape"):
            s.set_reaction(shape)
    with pytest.raises(mg.MGError, match=r"\[3\].*reaction"):   # a Neumann side while a reaction is set
        s.set_boundary("ndnd")
    assert s.boundary == (0, 0, 0, 0) and s.has_reaction
    s.set_boundary("dddd")                     # four Dirichlet sides are no boundary kind: accepted
    with pytest.raises(mg.MGError, match=r"\[3\].*reaction"):   # the adjoint while a reaction is set
        s.adjoint(F, want[0])
    _same(s.solve(F, U0), want, "after the refused boundary and adjoint")
    s.close()

    s = mg.Solver(N, 1.0, bc="ndnd", **opts)   # a reaction while a Neumann side is set
    want = s.solve(F, U0)
    with pytest.raises(mg.MGError, match=r"\[3\].*Neumann"):
        s.set_reaction(good)
    assert not s.has_reaction
    _same(s.solve(F, U0), want, "after the refusal on a Neumann solver")
    s.close()

    s = mg.Solver(N, 1.0, fmg=1, **opts)
    want = s.solve(F, U0)
    with pytest.raises(mg.MGError, match=r"\[3\].*fmg"):
        s.set_reaction(good)
    assert not s.has_reaction
    _same(s.solve(F, U0), want, "after the refusal on an fmg solver")
    s.close()
    with pytest.raises(mg.MGError, match=r"\[3\].*fmg"):
        mg.Solver(N, 1.0, fmg=1, reaction=good)

    assert mg.lib().mg_solver_set_reaction(None, None) == 2 and mg.lib().mg_solver_has_reaction(None) == 0
    with pytest.raises(mg.MGError, match=r"\[2\].*NULL solver"):
        mg._check()
    for cls, args in ((mg.BatchSolver, (N, 1.0, 2)), (mg.HeatStepper, (N, 1.0))):   # (out of scope: no reaction there)
        with pytest.raises(TypeError):
            cls(*args, reaction=good)
