"""The batched semilinear solve (include/mg_newton_batch.h) on the GPU.  The contract is bit identity with the single driver, so
every comparison is device against device through the same arithmetic, with ==: the batched pass against the single pass inside
guard bands; whole Newton solves of a mixed batch against Solver.newton on each instance alone (U and the whole info dict), in
both orders; stalled and capped instances; GCR; coefficients; the launch count; the refusals; torch tensors on a side stream."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _guard
import _newton_ref as nref
import _reaction_ref as rref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------- the pass alone, against the single pass
def pass_inputs(N, i):
    """instance i: U of order one with a -0.0 on the rim, a step of order one for t = 0.25, a weight with exact zeros, a > 0"""
    rng = np.random.default_rng(1000 * i + N)
    U = 2.0 * rng.random((N, N)) - 1.0
    U[0, 1] = -0.0
    U[N - 1, N - 2] = -0.0
    dlt = 3.0 * rng.standard_normal((N, N))
    w = 10.0 ** (4.0 * rng.random((N, N)) - 2.0)
    w[::3, ::5] = 0.0
    F = 50.0 * rng.standard_normal((N, N))
    a = 10.0 ** (2.0 * rng.random((N, N)))
    return dict(U=U, dlt=dlt, w=w, F=F, a=a)


def run_pass_case(mg, N, kind, order, numpy_ref=False):
    """The batched pass on the instances `order` (indices into distinct inputs; an index may repeat) against the single pass on
    each, in every combination of (a, w shared / own, step): V, D, S with == and the norm, nothing written outside the outputs.
    Up to _guard.DOWNLOAD_MAX_N arrays are downloaded and compared by bits; above it inputs are filled on the device and
    outputs compared through mg_checksum, the outputs of the two sides starting from different fills."""
    B, distinct = len(order), sorted(set(order))
    big = N > _guard.DOWNLOAD_MAX_N
    L, shift, t = 1.0, (1e4 if N % 2 else 0.0), 0.25
    kappas = [3.7, 0.0, 12.5, 1.0][:max(distinct) + 1]
    # per distinct input: U, dlt, F, w, a; per position: V, D, S; one more set for the single pass
    shapes = [N] * (5 * len(distinct) + 3 * B + 3)
    with _guard.block(mg, shapes, "odd16" if N % 4 == 2 else "page") as gb:
        views = list(gb.views)
        inp, host = {}, {}
        for d in distinct:
            inp[d] = dict(zip(("U", "dlt", "F", "w", "a"), views[:5]))
            views = views[5:]
            if big:
                for j, v in enumerate(inp[d].values()):
                    v.fill_uniform(100 * d + j + 1)
            else:
                host[d] = pass_inputs(N, d)
                for name, v in inp[d].items():
                    v.upload(host[d][name])
        outs = [dict(zip(("V", "D", "S"), views[3 * p:3 * p + 3])) for p in range(B)]
        one = dict(zip(("V", "D", "S"), views[3 * B:3 * B + 3]))
        readonly = [v for d in distinct for v in inp[d].values()]
        take = lambda name: [inp[i][name] for i in order]
        kap = [kappas[i] for i in order]

        def fresh(vs, seed):
            for j, v in enumerate(vs):
                v.fill_uniform(seed + j) if big else v.poison()

        def content(v):
            return v.checksum() if big else v.to_host()

        def same(x, y, what):
            if big:
                assert x == y, what
            else:
                assert_bits(x, y, what)

        for with_a in (False, True):
            for shared_w in (True, False):
                for step in (False, True):
                    what = f"N={N} {kind} B={B} a={with_a} shared w={shared_w} step={step}"
                    names = ("V", "D", "S") if step else ("D", "S")
                    fresh([o[n] for o in outs for n in ("V", "D", "S")], 7000)
                    gb.expect_readonly(*(readonly + ([] if step else [o["V"] for o in outs]) + list(one.values())))
                    norms = mg.nonlinear_residual_batch(
                        N, L, shift, take("a") if with_a else None, kind, kap, inp[order[0]]["w"] if shared_w else take("w"),
                        take("U"), take("F"), [o["D"] for o in outs], [o["S"] for o in outs],
                        dlt=take("dlt") if step else None, t=t, V=[o["V"] for o in outs] if step else None)
                    gb.check(what)
                    for p, i in enumerate(order):
                        wi = order[0] if shared_w else i
                        fresh(one.values(), 9000)
                        norm = mg.nonlinear_residual(N, L, shift, inp[i]["a"] if with_a else None, kind, kap[p], inp[wi]["w"],
                                                     inp[i]["U"], inp[i]["F"], one["D"], one["S"],
                                                     dlt=inp[i]["dlt"] if step else None, t=t, V=one["V"] if step else None)
                        assert norms[p] == norm, (what, p, norms[p], norm)
                        for n in names:
                            same(content(outs[p][n]), content(one[n]), f"{what}: {n} of position {p}")
                        if numpy_ref:
                            h, hw = host[i], host[wi]["w"]
                            want = nref.residual(N, L, h["a"] if with_a else None, kind, kap[p], hw, h["U"], h["F"], shift,
                                                 h["dlt"] if step else None, t)
                            for n, x in zip(("V", "D", "S"), want[:3]):
                                if n in names:
                                    assert_bits(outs[p][n].to_host(), x, f"{what}: {n} of position {p} against numpy")
                            assert norms[p] == want[3], (what, p)
                    # positions that hold the same instance hold the same bits, whatever stands beside them
                    for p in range(B):
                        for q in range(p + 1, B):
                            if order[p] == order[q]:
                                for n in names:
                                    same(content(outs[p][n]), content(outs[q][n]), f"{what}: {n} of positions {p} and {q}")


# both sides of the pair threshold (odd sizes and 24, 256, 258 below it; 514, 1026 above) and of the non-temporal one (4096),
# one interior point, the second column block of both lane shapes
@pytest.mark.parametrize("kind", nref.KINDS)
@pytest.mark.parametrize("N", [3, 4, 5, 17, 24, 255, 256, 257, 258, 514, 1026])
def test_batched_pass_equals_the_single_pass_inside_guard_bands(mg, N, kind):
    run_pass_case(mg, N, kind, [0, 1, 2])


@pytest.mark.parametrize("kind", nref.KINDS)
def test_batched_pass_non_temporal_form(mg, kind):
    run_pass_case(mg, 4096, kind, [0, 1])


@pytest.mark.parametrize("N", [24, 257, 514])
def test_batched_pass_one_instance_and_a_repeated_instance(mg, N):
    run_pass_case(mg, N, "sinh", [0])
    run_pass_case(mg, N, "sinh", [0, 1, 0, 2])   # instance 0 after nothing and between 1 and 2


@pytest.mark.parametrize("N", [17, 258, 514])
def test_batched_pass_against_the_numpy_restatement(mg, N):
    """cubic: no exp in it, so the restatement's bits do not depend on the host's libm"""
    run_pass_case(mg, N, "cubic", [0, 1, 2], numpy_ref=True)


# ---------------------------------------------------------------- whole solves
INFO_KEYS = ("status", "iterations", "converged", "stalled", "res0", "res", "inner_cycles", "trials", "history", "steps",
             "last_inner_history")


def mixed_batch(N, kind):
    """the instances of the mixed batch but the last: (F, U0, kappa, w) of the hard start, and of nref.problem with a smooth
    weight at kappa = 10, 0 (one iteration) and 100.  (w = 1 as an array is w = NULL bit for bit: kappa*1.0 == kappa.)"""
    F, U0 = nref.problem(N)
    w = nref.smooth_weight(N)
    hard = (np.full((N, N), nref.HARD_STARTS[kind]), np.zeros((N, N)), 1.0, np.ones((N, N)))
    return [hard] + [(F, U0, kappa, w) for kappa in (10.0, 0.0, 100.0)]


def with_converged_start(mg, N, kind, a, inst, **solver_opts):
    """appends the instance whose start is the converged U of an earlier call; returns the atol above its residual"""
    F, U0, kappa, w = inst[1]
    s = mg.Solver(N, 1.0, coef=a, **solver_opts)
    U, info = s.newton(F, U0, kind=kind, kappa=kappa, weight=w)
    s.close()
    assert info["converged"] and info["iterations"] >= 2
    inst.append((F, U, kappa, w))
    return 2.0 * info["res"]


def singles(mg, N, kind, a_of, inst, krylov=0, solver_opts=None, **opts):
    """Solver.newton on every instance alone: [(U, info, krylov log)]"""
    out = []
    for i, (F, U0, kappa, w) in enumerate(inst):
        s = mg.Solver(N, 1.0, coef=a_of(i), krylov=krylov, **(solver_opts or {}))
        U, info = s.newton(F, U0, kind=kind, kappa=kappa, weight=w, **opts)
        out.append((U, info, s.krylov_log() if krylov else None))
        assert not s.has_reaction
        s.close()
    return out


def run_batch_in_guards(mg, b, kind, inst, order, untouched=(), **opts):
    """BatchSolver.newton_ptrs on the instances inst[order[0]], inst[order[1]], ... with every U inside guard bands; the U of
    the positions `untouched` are declared read-only for the call.  Returns ([U], infos) by position."""
    N = b.N
    G = mg.DeviceGrid
    keep = [(G.from_host(inst[i][0]), G.from_host(inst[i][3])) for i in order]
    with _guard.block(mg, [N] * len(order), "page") as gb:
        for v, i in zip(gb.views, order):
            v.upload(inst[i][1])
        gb.expect_readonly(*[gb.views[p] for p in untouched])
        infos = b.newton_ptrs([f.ptr for f, _ in keep], [v.ptr for v in gb.views], kind=kind, kappa=[inst[i][2] for i in order],
                              w_ptrs=[w.ptr for _, w in keep], **opts)
        gb.check(f"N={N} {kind} order {order}")
        Us = [v.to_host() for v in gb.views]
    for f, w in keep:
        f.free(), w.free()
    return Us, infos


def assert_instances_equal(Us, infos, want, order, what):
    for p, i in enumerate(order):
        assert_bits(Us[p], want[i][0], f"{what}: U of instance {i} at position {p}")
        assert set(infos[p]) == set(INFO_KEYS) == set(want[i][1])
        for key in INFO_KEYS:
            assert infos[p][key] == want[i][1][key], (what, i, p, key, infos[p][key], want[i][1][key])
        assert infos[p] == want[i][1]


@pytest.mark.parametrize("kind", nref.KINDS)
@pytest.mark.parametrize("N,coef", [(33, None), (100, None), (257, None), (514, "exp")])
def test_mixed_batch_at_defaults_equals_the_single_driver(mg, N, coef, kind):
    """the hard start (backtracks), kappa = 10, 0 and 100, and a start that already meets the tolerance, in one call and in the
    reversed order: per instance U and the whole info dict of Solver.newton alone.  (tests/_newton_ref.py on the CPU at N = 33:
    iterations 7, 4, 1, 5, 0 for cubic, 9, 3, 1, 3, 0 for sinh, 9, 3, 1, 5, 0 for exp; backtracks 9, 3 / 6, 4, 2 / 7, 5, 3, 1.)"""
    a = None if coef is None else vref.field(coef, N)
    inst = mixed_batch(N, kind)
    atol = with_converged_start(mg, N, kind, a, inst)
    want = singles(mg, N, kind, lambda i: a, inst, atol=atol)
    its = [info["iterations"] for _, info, _ in want]
    bts = [sum(s["backtracks"] for s in info["steps"]) for _, info, _ in want]
    print(f"N={N} {kind} a={coef}: iterations {its}, backtracks {bts}, atol {atol}")
    assert len(set(its)) >= 3 and its[4] == 0 and its[2] == 1 and bts[0] >= 1
    b = mg.BatchSolver(N, 1.0, max_batch=5)
    if a is not None:
        b.set_coefficient(a)
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0]):
        Us, infos = run_batch_in_guards(mg, b, kind, inst, order, untouched=[order.index(4)], atol=atol)
        assert_instances_equal(Us, infos, want, order, f"N={N} {kind} a={coef} order {order}")
        assert_bits(Us[order.index(4)], inst[4][1], "the converged start: U untouched")
        st = infos.stats
        every = all(info["converged"] for _, info, _ in want)
        assert st["status"] == (nref.CONVERGED if every else nref.NOT_CONVERGED) and st["iterations"] == max(its) and not b.has_reaction
        # lockstep: the rounds of an iteration are those of its slowest line search (a step's trials: its rejections, and the
        # accepted one when t > 0), the iterations those of the slowest instance
        steps = [info["steps"] for _, info, _ in want]
        rounds = sum(max(x[k]["backtracks"] + (x[k]["t"] > 0.0) for x in steps if len(x) > k) for k in range(max(len(x) for x in steps)))
        assert st["trial_rounds"] == rounds
    b.close()


@pytest.mark.parametrize("N", [33, 514])
def test_an_instance_beyond_minus_512_next_to_an_ordinary_one(mg, N):
    """F == +1e4 with kind = "exp" (tests/test_newton_exp_domain_gpu.py: its solution has a minimum near -737, so accepted trials
    evaluate exp through the device library's branch of exp_libm, into subnormal results) beside nref.problem at kappa = 10: per
    instance U and the whole info dict of Solver.newton alone, in both orders"""
    F, U0 = nref.problem(N)
    inst = [(np.full((N, N), 1e4), np.zeros((N, N)), 1.0, np.ones((N, N))), (F, U0, 10.0, nref.smooth_weight(N))]
    want = singles(mg, N, "exp", lambda i: None, inst)
    assert all(info["converged"] for _, info, _ in want)
    assert want[0][0].min() < -512.0 and np.abs(want[1][0]).max() < 512.0
    b = mg.BatchSolver(N, 1.0, max_batch=2)
    for order in ([0, 1], [1, 0]):
        Us, infos = run_batch_in_guards(mg, b, "exp", inst, order)
        assert_instances_equal(Us, infos, want, order, f"N={N} beyond -512, order {order}")
        assert infos.stats["status"] == nref.CONVERGED and not b.has_reaction
    b.close()


@pytest.mark.parametrize("kind", nref.KINDS)
@pytest.mark.parametrize("N", [33, 100])
def test_stalled_and_capped_instances(mg, N, kind):
    """max_backtracks = 2, max_iters = 2: the hard start stalls on its first iteration, kappa = 10 and 100 reach the cap, kappa = 0
    and the converged start converge.  Per instance status, U and records are the single driver's; the solver has no reaction
    afterwards and solves as a fresh one."""
    inst = mixed_batch(N, kind)
    atol = with_converged_start(mg, N, kind, None, inst)
    opts = dict(max_backtracks=2, max_iters=2, rtol=1e-8, atol=atol)
    want = singles(mg, N, kind, lambda i: None, inst, **opts)
    statuses = [info["status"] for _, info, _ in want]
    assert {nref.CONVERGED, nref.NOT_CONVERGED, nref.STALLED} == set(statuses), statuses
    b = mg.BatchSolver(N, 1.0, max_batch=6)
    order = [3, 0, 4, 1, 2]
    Us, infos = run_batch_in_guards(mg, b, kind, inst, order, untouched=[order.index(4)], **opts)
    assert_instances_equal(Us, infos, want, order, f"N={N} {kind}")
    assert infos.stats["status"] == nref.NOT_CONVERGED
    for p, i in enumerate(order):
        if infos[p]["status"] == nref.STALLED:   # the extra record, and U the last accepted iterate
            assert len(infos[p]["steps"]) == infos[p]["iterations"] + 1 and infos[p]["steps"][-1]["t"] == 0.0
            assert infos[p]["steps"][-1]["backtracks"] == 3 and infos[p]["res"] == infos[p]["history"][-1]
            if infos[p]["iterations"] == 0:
                assert_bits(Us[p], inst[i][1], "stalled on the first iteration: U is the start")
    assert not b.has_reaction and b.n_reactions == 0
    F = np.stack([x[0] for x in inst])
    U0 = np.stack([x[1] for x in inst])
    got = b.solve(F, U0)
    fresh = mg.BatchSolver(N, 1.0, max_batch=6)
    new = fresh.solve(F, U0)
    assert_bits(got[0], new[0], "a plain solve after the Newton call")
    for x, y in zip(got[1], new[1]):
        for key in ("history", "cycles", "status", "converged", "res0", "res", "ref_norm"):
            assert x[key] == y[key], key
        assert x["stats"]["launches"] == y["stats"]["launches"]
    b.close(), fresh.close()


def test_with_gcr_equals_the_single_driver_with_krylov(mg):
    """the half-plane weight of tests/test_newton_gpu.py beside two smooth instances under GCR(8): U, the info dict and the
    Krylov log of the last inner solve"""
    N, m, kind = 129, 8, "sinh"
    F, U0 = nref.problem(N)
    inst = [(F, U0, 10.0, nref.smooth_weight(N)), (F, U0, 1.0, rref.field("halfplane", N)), (0.5 * F, U0, 3.0, nref.smooth_weight(N))]
    sopts = dict(max_cycles=60)
    want = singles(mg, N, kind, lambda i: None, inst, krylov=m, solver_opts=sopts)
    assert all(info["converged"] for _, info, _ in want) and all(log for _, _, log in want)
    b = mg.BatchSolver(N, 1.0, max_batch=3, **sopts)
    b.set_krylov(m)
    for order in ([0, 1, 2], [1, 2, 0]):
        Us, infos = run_batch_in_guards(mg, b, kind, inst, order)
        assert_instances_equal(Us, infos, want, order, f"GCR order {order}")
        for p, i in enumerate(order):
            assert b.krylov_log(p) == want[i][2], (order, p)
    assert b.krylov == m and not b.has_reaction
    b.close()


@pytest.mark.parametrize("kind", nref.KINDS)
@pytest.mark.parametrize("coefs", ["none", "shared", "own"])
def test_coefficients_and_weights_shared_or_per_instance(mg, coefs, kind):
    """N = 65 through BatchSolver.newton_batch on numpy arrays: no a, one shared, one per instance ("exp", "random"), each with one
    shared weight and with one per instance, against Solver(coef=a_i).newton with w_i"""
    N, B = 65, 3
    F, U0 = nref.problem(N)
    Fs = np.stack([F, 0.5 * F, 2.0 * F])
    U0s = np.stack([U0, U0, 0.5 * U0])
    kappas = [10.0, 1.0, 30.0]
    fields = [vref.field("exp", N), vref.field("random", N, seed=3), vref.field("smooth", N)]
    a_of = {"none": lambda i: None, "shared": lambda i: fields[0], "own": lambda i: fields[i]}[coefs]
    ws = [nref.smooth_weight(N), 1.0 + nref.smooth_weight(N), np.where(vref.grid(N)[0] > 0.5, 2.0, 0.0) + 0.0 * vref.grid(N)[1]]
    b = mg.BatchSolver(N, 1.0, max_batch=B)
    if coefs != "none":
        b.set_coefficient(fields[0] if coefs == "shared" else np.stack(fields))
    for weight in (ws[0], np.stack(ws), None):
        w_of = (lambda i: None) if weight is None else (lambda i: ws[0]) if weight is ws[0] else (lambda i: ws[i])
        inst = [(Fs[i], U0s[i], kappas[i], w_of(i)) for i in range(B)]
        want = singles(mg, N, kind, a_of, inst, max_iters=6)
        U, infos = b.newton_batch(Fs, U0s, kind=kind, kappa=kappas, weight=weight, max_iters=6)
        assert_instances_equal(list(U), infos, want, [0, 1, 2], f"{kind} a {coefs} w {'none' if weight is None else weight.ndim}")
        assert b.n_coefficients == {"none": 0, "shared": 1, "own": B}[coefs] and not b.has_reaction
    U, info = mg.solve_semilinear_batched(Fs, U0s, kind=kind, kappa=kappas, weight=np.stack(ws),
                                          coef=None if coefs == "none" else fields[0] if coefs == "shared" else np.stack(fields), max_iters=6)
    inst = [(Fs[i], U0s[i], kappas[i], ws[i]) for i in range(B)]
    assert_instances_equal(list(U), info, singles(mg, N, kind, a_of, inst, max_iters=6), [0, 1, 2], "solve_semilinear_batched")
    b.close()


def test_launches_do_not_depend_on_the_number_of_instances(mg):
    """B = 1 and B = 8 copies of one problem: every iteration and every round is one set of launches over the active set, so the
    call enqueues the same number of kernels"""
    N = 100
    F, U0 = nref.problem(N)
    w = nref.smooth_weight(N)
    stats = []
    for B in (1, 8):
        b = mg.BatchSolver(N, 1.0, max_batch=8)
        U, infos = b.newton_batch(np.stack([F] * B), np.stack([U0] * B), kind="sinh", kappa=10.0, weight=w)
        assert all(i == infos[0] for i in infos) and all(np.array_equal(u, U[0]) for u in U) and infos[0]["converged"]
        stats.append(infos.stats)
        b.close()
    for key in ("launches", "trial_rounds", "iterations", "inner_cycles", "status"):
        assert stats[0][key] == stats[1][key], (key, stats)
    assert stats[0]["launches"] > 0 and stats[0]["trial_rounds"] >= stats[0]["iterations"] >= 2


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_solver_and_every_U_as_they_were(mg):
    N, B = 64, 3
    F, U0 = nref.problem(N)
    G = mg.DeviceGrid
    opts = dict(rtol=0.0, max_cycles=1)
    Fs, U0s = np.stack([F, 0.5 * F, 2.0 * F]), np.stack([U0, 0.5 * U0, U0])
    fresh = mg.BatchSolver(N, 1.0, max_batch=B, **opts)
    want = fresh.solve(Fs, U0s)
    fresh.close()
    b = mg.BatchSolver(N, 1.0, max_batch=B, **opts)
    Fd, Ud = [G.from_host(f) for f in Fs], [G.from_host(u) for u in U0s]
    Fp, Up = [f.ptr for f in Fd], [u.ptr for u in Ud]

    def same_after(what):
        for u, u0 in zip(Ud, U0s):
            assert_bits(u.to_host(), u0, what + ": U untouched")
        assert not b.has_reaction
        got = b.solve(Fs, U0s)
        assert_bits(got[0], want[0], what + ": the next solve")
        assert [i["history"] for i in got[1]] == [i["history"] for i in want[1]]
        assert got[1][0]["stats"]["launches"] == want[1][0]["stats"]["launches"]

    def refused(code, pattern, *args, **kw):
        with pytest.raises(mg.MGError, match=r"\[%d\].*%s" % (code, pattern)):
            b.newton_ptrs(*args, **kw)

    refused(2, "outside", [], [])
    more = [G.zeros((N, N)) for _ in range(B)]
    refused(2, "outside", Fp * 2, Up + [u.ptr for u in more])
    same_after("n outside [1, max_batch]")
    refused(2, "2 w arrays for 3 instances", Fp, Up, w_ptrs=[Fp[0], Fp[1]])
    same_after("n_w not in {0, 1, n}")
    refused(2, "unknown kind", Fp, Up, kind=7)
    with pytest.raises(mg.MGError, match="kind"):
        b.newton_ptrs(Fp, Up, kind="tanh")
    same_after("an unknown kind")
    for kappa in (-1.0, float("nan"), float("inf")):
        refused(2, "kappa.*instance 1", Fp, Up, kappa=[1.0, kappa, 1.0])
    with pytest.raises(mg.MGError, match=r"\[2\].*kappa"):
        b.newton_ptrs(Fp, Up, kappa=[1.0, 2.0])
    same_after("a bad kappa")
    for value in (-1.0, float("nan"), float("inf")):
        w = np.ones((B, N, N))
        w[2, N - 1, 3] = value                 # (a rim point of instance 2: the rim is part of the array)
        with pytest.raises(mg.MGError, match=r"\[2\].*w must be finite.*instance 2"):
            b.newton_batch(Fd, Ud, kind="cubic", weight=w)
        with pytest.raises(mg.MGError, match=r"\[2\].*w must be finite.*instance 0"):
            b.newton_batch(Fd, Ud, kind="cubic", weight=w[2])
    same_after("a bad value of w")
    g = G.zeros((N + 1, N))                    # a pointer 8 bytes past a 16-byte boundary
    refused(2, "16-byte aligned", [Fp[0], g.ptr + 8, Fp[2]], Up)
    refused(2, "16-byte aligned", Fp, [Up[0], Up[1], g.ptr + 8])
    refused(2, "16-byte aligned", Fp, Up, w_ptrs=[g.ptr + 8])
    refused(2, "NULL", [Fp[0], None, Fp[2]], Up)
    refused(2, "NULL", Fp, Up, w_ptrs=[Fp[0], None, Fp[2]])
    assert mg.lib().mg_batch_solver_newton(None, 1, 0, None, 0, None, None, None, None, None, None) == 2
    with pytest.raises(mg.MGError, match=r"\[2\].*NULL"):
        mg._check()
    g.free()
    same_after("misaligned and NULL arrays")
    refused(2, "U of instances 0 and 2 overlap", Fp, [Up[0], Up[1], Up[0]])
    refused(2, "U of instance 1 overlaps F of instance 0", [Up[1], Fp[1], Fp[2]], Up)
    same_after("overlapping arrays")
    for bad in (dict(rtol=-1.0), dict(atol=float("nan")), dict(max_iters=-1), dict(max_backtracks=-1)):
        refused(2, "max_iters", Fp, Up, **bad)
    with pytest.raises(mg.MGError, match="shape"):
        b.newton_batch(np.ones((B, N, N + 1)), Ud)
    with pytest.raises(mg.MGError, match=r"\[2\].*weight"):
        b.newton_batch(Fd, Ud, weight=np.ones((B, N + 1, N)))
    same_after("options and shapes")
    # a start whose residual is not finite: the whole call is refused, the message names the instance
    bad = U0s[1].copy()
    bad[5, 5] = float("inf")
    Ud[1].free()
    Ud[1] = G.from_host(bad)
    refused(2, "residual of the start of instance 1 is not finite", Fp, [Ud[0].ptr, Ud[1].ptr, Ud[2].ptr], kind="cubic")
    assert_bits(Ud[1].to_host(), bad, "a refused start: U untouched")
    Ud[1].free()
    Ud[1] = G.from_host(U0s[1])
    Up[1] = Ud[1].ptr
    same_after("a start that is not finite")
    # more instances than per-instance coefficients
    b.set_coefficient(np.stack([vref.field("exp", N), vref.field("smooth", N)]))
    refused(2, "holds 2 coefficients", Fp, Up)
    b.set_coefficient(None)
    same_after("beyond the coefficient count")
    # the caller has a reaction set: refused, and the reaction stays
    b.set_reaction(rref.field("smooth", N))
    before = b.solve(Fs, U0s)
    refused(3, "reaction term is set", Fp, Up)
    assert b.has_reaction and b.n_reactions == 1
    after = b.solve(Fs, U0s)
    assert_bits(after[0], before[0], "after the refusal with a reaction set")
    b.set_reaction(None)
    same_after("a caller's reaction")
    # and after a Newton call that ran, the solver is the plain one again
    infos = b.newton_ptrs(Fp, Up, kind="cubic", kappa=[1.0, 2.0, 3.0], max_iters=2)
    assert len(infos) == B and all(i["iterations"] == 2 for i in infos)
    for u, u0 in zip(Ud, U0s):
        mg.lib().mg_upload(u.ptr, np.ascontiguousarray(u0).ctypes.data, u0.size)
    same_after("a Newton call")
    b.close()


# ---------------------------------------------------------------- torch
def test_torch_tensors_on_a_side_stream():
    """a child process: torch first, tensors on a non-default stream, the same bits as the numpy path"""
    out = subprocess.run([sys.executable, os.path.join(HERE, "_newton_batched_torch_worker.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "NEWTON_BATCHED_TORCH OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
