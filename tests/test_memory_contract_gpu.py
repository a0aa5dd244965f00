"""The memory side of the C ABI (include/mg_hip.h): a call writes its outputs and nothing else, and only reads its inputs.

Every array of every call lies inside one larger mg_alloc block between guard bands (tests/_guard.py): a stray store
changes a band or an input, a consumed out-of-window read poisons the output -- nothing can fault, the access stays in
memory the process owns.  Each case asserts the output bits against the oracle (the expressions of test_parity_gpu.py /
test_mixed_gpu.py / _solve_ref.py) AND check(): every band and every read-only array unchanged, by bits.  Which arguments
are read only is written down once, in _guard.CONTRACT, from the header (tests/test_memory_contract_cpu.py holds the table
to the prototypes).  Both placements of _guard.PLACEMENTS: 4 KiB-aligned arrays, and arrays that are 16-byte aligned and
nothing more.

Sizes follow the dispatch boundaries of the code: one-workgroup and tail forms (N <= 64), the register-tile range
(MG_TILE_MIN_N .. MG_TILE_MAX_N, 65 .. 1024) and its neighbours, the streaming kernel with widths that are no multiple of
a strip (2050 = 8*256 + 2, 2178 = 2048 + 130, 2302 = 8*256 + 254, odd 2049), N mod PR != 0 and N mod ROWS_PB != 0, the
n >= 2^20 boundary of the flat kernels (1023, 1024, 1025; odd n takes the scalar form).  The product thresholds
(MG_BIG_GRID_MIN_N = 4096, MG_PAIR_ROWS_MIN_N = 8192, non-temporal and 4-column forms without the suite's overrides) run
in a child process at N = 4096, 4098, 8192 and 8194 (tests/_memory_contract_big_worker.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _guard
import _oracle_f32 as o32
import _solve_ref as ref
import _synth
from conftest import assert_bits
from test_mixed_gpu import bits32
from test_parity_gpu import PAIRS_P, PAIRS_R, REL, rand_pair

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PLACE = list(_guard.PLACEMENTS)
TILE_LO = int(os.environ.get("MG_TILE_MIN_N", "65"))
TILE_HI = int(os.environ.get("MG_TILE_MAX_N", "1024")) or 1024
SMALL = [4, 5, 8, 17, 33, 64]
TILE = sorted({65, 100, 129, 256, 257, 724, 1024, TILE_LO - 1, TILE_LO, TILE_HI, TILE_HI + 1})
STREAM = [1025, 1448, 2048, 2049, 2050, 2048 + 130, 8 * 256 + 254]
SIZES = SMALL + TILE + STREAM
FLAT = [4, 5, 17, 64, 65, 257, 1023, 1024, 1025, 2048, 2049]   # n = N*N on both sides of 2^20, odd and even
STEPS = [1, 2, 3, 4, 6]
NODE_PAIRS = sorted({(N, N // 2) for N in SIZES if N >= 8} | {(16, 15), (100, 37), (33, 16), (250, 124), (1022, 511)})


def with_smoothers(cases):
    """(smoother, *case) for both smoothers"""
    out = []
    for c in cases:
        c = c if isinstance(c, tuple) else (c,)
        out += [(sm,) + c for sm in ("stream", "simple")]
    return out


@pytest.fixture
def smoother(request, mg):
    """sets the smoother named by the test's `sm` parameter for the duration of the test"""
    name = request.node.callspec.params["sm"]
    mg.set_smoother(name)
    yield name
    mg.set_smoother("stream")


# ------------------------------------------------------------------ the six operators
@pytest.mark.parametrize("place", PLACE)
@pytest.mark.parametrize("sm,N", with_smoothers(SIZES))
def test_smoothing_and_residual(mg, oracle, smoother, sm, N, place):
    """mg_doSmoothing (U in place, F read only; odd and even step counts: both ping-pong partners) and mg_getResidual."""
    U0, F = rand_pair(N, N)
    b = _guard.block(mg, [N, N, N], place)
    try:
        U, Fd, D = b.views
        Fd.upload(F)
        for step in (1, 2, 3, 4, 5):
            U.upload(U0)
            D.poison()
            b.expect_readonly(Fd)
            err = mg.doSmoothing(N, 1.0, U, Fd, step)
            want, werr = oracle.doSmoothing(N, 1.0, U0, F, step)
            assert_bits(U.to_host(), want, f"doSmoothing N={N} step={step} {place}")
            assert err == pytest.approx(werr, rel=REL)
            b.check(f"mg_doSmoothing N={N} step={step} ({smoother})")
        U.upload(U0)
        b.expect_readonly(U, Fd)
        mg.getResidual(N, 1.7, U, Fd, D)
        assert_bits(D.to_host(), oracle.getResidual(N, 1.7, U0, F), f"getResidual N={N} {place}")
        b.check(f"mg_getResidual N={N}")
    finally:
        b.free()


@pytest.mark.parametrize("place", PLACE)
@pytest.mark.parametrize("N", FLAT)
def test_flat_operators(mg, oracle, N, place):
    """mg_doGridAddition, mg_negate, mg_copy, mg_fill_zero, mg_fill_uniform, mg_checksum, mg_to_f32, mg_to_f64."""
    A0, B0 = rand_pair(N, 3 * N)
    n = N * N
    b = _guard.block(mg, [N, N, N], place)
    b32 = _guard.block(mg, [N], place, np.float32)
    try:
        A, B, Cv = b.views
        A.upload(A0); B.upload(B0); Cv.poison()
        b.expect_readonly(B, Cv)
        mg.doGridAddition(N, A, B)
        assert_bits(A.to_host(), oracle.doGridAddition(N, A0, B0), "doGridAddition")
        b.check(f"mg_doGridAddition N={N}")
        b.expect_readonly(B, Cv)
        mg.negate(N, A)
        assert_bits(A.to_host(), -oracle.doGridAddition(N, A0, B0), "negate")
        b.check(f"mg_negate N={N}")
        b.expect_readonly(A, B)
        mg.lib().mg_copy(Cv.ptr, B.ptr, n)
        assert_bits(Cv.to_host(), B0, "mg_copy")
        b.check(f"mg_copy N={N}")
        b.expect_readonly(A, B)
        mg.lib().mg_fill_zero(Cv.ptr, n)
        assert_bits(Cv.to_host(), np.zeros((N, N)), "mg_fill_zero")
        b.check(f"mg_fill_zero N={N}")
        b.expect_readonly(A, B)
        mg.lib().mg_fill_uniform(Cv.ptr, n, 11)
        host = _synth.hash_field(N, 11)
        assert_bits(Cv.to_host(), host, "mg_fill_uniform")
        b.check(f"mg_fill_uniform N={N}")
        b.expect_readonly(A, B, Cv)
        assert Cv.checksum() == _synth.checksum(host)
        b.check(f"mg_checksum N={N}")
        # conversions: fp64 -> fp32 (round to nearest) -> fp64 (exact)
        S = b32.views[0]
        b.expect_readonly(A, B, Cv)
        mg.lib().mg_to_f32(S.ptr, B.ptr, n)
        assert np.array_equal(S.to_host().view(np.uint32), B0.astype(np.float32).view(np.uint32)), "mg_to_f32"
        b.check(f"mg_to_f32 N={N} (source)"); b32.check(f"mg_to_f32 N={N}")
        b.expect_readonly(A, B); b32.expect_readonly(S)
        mg.lib().mg_to_f64(Cv.ptr, S.ptr, n)
        assert_bits(Cv.to_host(), B0.astype(np.float32).astype(np.float64), "mg_to_f64")
        b.check(f"mg_to_f64 N={N}"); b32.check(f"mg_to_f64 N={N} (source)")
    finally:
        b.free(); b32.free()


@pytest.mark.parametrize("place", PLACE)
@pytest.mark.parametrize("N,M", PAIRS_R + [(2050, 1025), (2049, 1024)])
def test_restriction(mg, oracle, N, M, place):
    Uf = np.random.default_rng(N + M).random((N, N)) - 0.3
    b = _guard.block(mg, [N, M], place)
    try:
        f, c = b.views
        f.upload(Uf); c.poison()
        b.expect_readonly(f)
        mg.doRestriction(N, f, M, c)
        assert_bits(c.to_host(), oracle.doRestriction(N, Uf, M), f"doRestriction {N}->{M}")
        b.check(f"mg_doRestriction {N}->{M}")
        c.poison()
        b.expect_readonly(f)
        mg.restrict_signed(N, f, M, c, -1)
        assert_bits(c.to_host(), oracle.doRestriction(N, -Uf, M), "restrict_signed", zero_sign=True)
        b.check(f"mg_restrict_signed {N}->{M}")
    finally:
        b.free()


@pytest.mark.parametrize("place", PLACE)
@pytest.mark.parametrize("N,M", PAIRS_P + [(1025, 2050), (1024, 2049)])
def test_prolongation(mg, oracle, N, M, place):
    Uc = np.random.default_rng(N * M).random((N, N)) - 0.3
    base = np.random.default_rng(1).random((M, M))
    b = _guard.block(mg, [N, M, M], place)
    try:
        c, f, o = b.views
        c.upload(Uc); f.upload(np.zeros((M, M))); o.poison()
        b.expect_readonly(c, o)
        mg.doProlongation(N, c, M, f)
        want = oracle.doProlongation(N, Uc, M, fill=0.0)
        assert_bits(f.to_host(), want, f"doProlongation {N}->{M}")
        b.check(f"mg_doProlongation {N}->{M}")
        f.upload(base)
        b.expect_readonly(c, f)
        mg.prolongAdd(N, c, M, f, o)
        assert_bits(o.to_host(), oracle.doGridAddition(M, base, want), "prolongAdd")
        b.check(f"mg_prolongAdd {N}->{M}")
    finally:
        b.free()


@pytest.mark.parametrize("place", PLACE)
@pytest.mark.parametrize("N", [4, 5, 8, 17, 33, 64, 96, 100, 160])
def test_exact_solver(mg, oracle, N, place):
    F = np.random.default_rng(N).random((N, N)) - 0.5
    tol = 1e-7 if N <= 33 else 5e-3
    b = _guard.block(mg, [N, N], place)
    try:
        U, Fd = b.views
        Fd.upload(F); U.upload(np.full((N, N), 3.0))
        b.expect_readonly(Fd)
        mg.doExactSolver(N, 1.0, U, Fd, tol, 1)
        want = oracle.doExactSolver(N, 1.0, F, tol)
        assert mg.lastExactSolverIterations() == oracle.gs_iterations()
        assert_bits(U.to_host(), want, f"GaussSeidel N={N}")
        b.check(f"mg_doExactSolver N={N}")
    finally:
        b.free()


@pytest.mark.parametrize("place", PLACE)
@pytest.mark.parametrize("N", [16, 129, 1024, 2050])
def test_problem_definition(mg, oracle, N, place):
    """mg_getSource, mg_getAnalytic (outputs), mg_analyticError (U read only)."""
    b = _guard.block(mg, [N, N], place)
    try:
        F, U = b.views
        F.poison()
        U0 = np.random.default_rng(N).random((N, N))
        U.upload(U0)
        b.expect_readonly(U)
        mg.lib().mg_getSource(N, 1.5, F.ptr, 0.25, -0.5)
        mg._check()
        assert_bits(F.to_host(), oracle.getSource(N, 1.5, 0.25, -0.5), "getSource")
        b.check(f"mg_getSource N={N}")
        b.expect_readonly(U)
        mg.lib().mg_getAnalytic(N, 1.0, F.ptr, 0.0, 0.0)
        mg._check()
        np.testing.assert_allclose(F.to_host(), oracle.getAnalytic(N), rtol=2e-15, atol=0)
        b.check(f"mg_getAnalytic N={N}")
        b.expect_readonly(U, F)
        got = mg.analyticError(N, 1.0, U)
        assert got == pytest.approx(np.abs(oracle.getAnalytic(N) - U0).sum() / (N * N), rel=1e-12)
        b.check(f"mg_analyticError N={N}")
    finally:
        b.free()


# ------------------------------------------------------------------ fused forms
@pytest.mark.parametrize("place", PLACE)
@pytest.mark.parametrize("sm,N", with_smoothers([8, 64, 65, 257, 1024, 1025, 2048, 2050]))
def test_smooth_pp(mg, oracle, smoother, sm, N, place):
    """mg_smooth_pp with and without D_out / error_dev / U_in: F read only; U_in is the documented clobber (its
    contents are not asserted, its bands are)."""
    U0, F = rand_pair(N, 7 * N)
    b = _guard.block(mg, [N, N, N, N, (1, 2)], place)
    try:
        Uin, out, Fd, D, e = b.views
        Fd.upload(F)
        for step in STEPS:
            out.poison(); D.poison(); Uin.upload(U0)
            b.expect_readonly(Fd, Uin)   # zero start: U_in is not passed, so it must not change either
            err = mg.smooth_pp(N, 1.0, None, out, Fd, step, want_error=True, D_out=D, d_sign=-1)
            want, werr = oracle.doSmoothing(N, 1.0, np.zeros((N, N)), F, step)
            assert_bits(out.to_host(), want, f"smooth_pp zero start N={N} step={step}")
            assert_bits(D.to_host(), -oracle.getResidual(N, 1.0, want, F), "fused -residual")
            assert err == pytest.approx(werr, rel=REL)
            b.check(f"mg_smooth_pp(U_in=NULL, D_out) N={N} step={step} ({smoother})")
            out.poison(); D.poison()
            b.expect_readonly(Fd, D)    # no D_out: D must stay as it is
            mg.lib().mg_smooth_pp(N, 1.0, Uin.ptr, out.ptr, Fd.ptr, step, e.ptr, None, +1)
            mg._check()
            want, werr = oracle.doSmoothing(N, 1.0, U0, F, step)
            assert_bits(out.to_host(), want, f"smooth_pp N={N} step={step}")
            assert float(e.to_host()[0, 0]) == pytest.approx(werr, rel=REL)
            b.check(f"mg_smooth_pp(U_in, error_dev) N={N} step={step} ({smoother})")
    finally:
        b.free()


@pytest.mark.parametrize("place", PLACE)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("sm,N,M", with_smoothers(NODE_PAIRS))
def test_smooth_restrict(mg, oracle, smoother, sm, N, M, step, place):
    """One `-1` node: U_in and F read only, U_out and F_c written."""
    U0, F = rand_pair(N, 11 * N + M)
    b = _guard.block(mg, [N, N, N, M, (1, 2)], place)
    try:
        Uin, out, Fd, Fc, e = b.views
        Fd.upload(F); Uin.upload(U0)
        for zero in (True, False):
            start = np.zeros((N, N)) if zero else U0
            want_U, want_err = oracle.doSmoothing(N, 1.0, start, F, step)
            want_Fc = oracle.doRestriction(N, -oracle.getResidual(N, 1.0, want_U, F), M)
            out.poison(); Fc.poison()
            b.expect_readonly(Fd, Uin)
            mg.lib().mg_smooth_restrict(N, 1.0, None if zero else Uin.ptr, out.ptr, Fd.ptr, step, e.ptr, M, Fc.ptr)
            mg._check()
            what = f"mg_smooth_restrict {N}->{M} step={step} zero={zero} ({smoother}, {place})"
            assert_bits(out.to_host(), want_U, what + " U")
            assert_bits(Fc.to_host(), want_Fc, what + " F_c")
            assert float(e.to_host()[0, 0]) == pytest.approx(want_err, rel=REL)
            b.check(what)
    finally:
        b.free()


@pytest.mark.parametrize("place", PLACE)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("sm,N,Nc", with_smoothers(NODE_PAIRS))
def test_prolong_smooth(mg, oracle, smoother, sm, N, Nc, step, place):
    """One `1` node: U_c, U_in and F read only, U_out written."""
    rng = np.random.default_rng(13 * N + Nc)
    Uc, Uf, F = rng.random((Nc, Nc)) - 0.5, rng.random((N, N)), rng.random((N, N)) - 0.5
    want0 = oracle.doGridAddition(N, Uf, oracle.doProlongation(Nc, Uc, N, fill=0.0))
    want, want_err = oracle.doSmoothing(N, 1.0, want0, F, step)
    b = _guard.block(mg, [Nc, N, N, N, (1, 2)], place)
    try:
        c, Uin, out, Fd, e = b.views
        c.upload(Uc); Uin.upload(Uf); Fd.upload(F); out.poison()
        b.expect_readonly(c, Uin, Fd)
        mg.lib().mg_prolong_smooth(Nc, c.ptr, N, 1.0, Uin.ptr, out.ptr, Fd.ptr, step, e.ptr)
        mg._check()
        what = f"mg_prolong_smooth {Nc}->{N} step={step} ({smoother}, {place})"
        assert_bits(out.to_host(), want, what)
        assert float(e.to_host()[0, 0]) == pytest.approx(want_err, rel=REL)
        b.check(what)
    finally:
        b.free()


@pytest.mark.parametrize("place", PLACE)
@pytest.mark.parametrize("step", [1, 2, 3, 4])
@pytest.mark.parametrize("N,M", [(8, 4), (16, 8), (64, 32), (66, 33), (256, 128), (257, 128), (100, 37), (1024, 512), (1448, 724), (2048, 1024), (2050, 1025)])
def test_fused_nodes_f32(mg, N, M, step, place):
    """mg_smooth_restrict_f32 / mg_prolong_smooth_f32 (one launch on even N with a nested coarse size, operator by
    operator otherwise) against the numpy fp32 restatement; F, U_c, U_in read only."""
    rng = np.random.default_rng(N + step)
    F = (rng.random((N, N)) - 0.5).astype(np.float32)
    Uc = (rng.random((M, M)) - 0.5).astype(np.float32)
    Uf = rng.random((N, N)).astype(np.float32)
    b = _guard.block(mg, [N, N, N, M, M], place, np.float32)
    e = _guard.block(mg, [(1, 2)], place)
    try:
        Fd, out, Uin, Fc, c = b.views
        Fd.upload(F); Uin.upload(Uf); c.upload(Uc); out.poison(); Fc.poison()
        b.expect_readonly(Fd, Uin, c)
        mg.lib().mg_smooth_restrict_f32(N, 1.0, None, out.ptr, Fd.ptr, step, e.views[0].ptr, M, Fc.ptr)
        mg._check()
        U, werr = o32.smooth(np.zeros((N, N), dtype=np.float32), F, step, 1.0)
        assert bits32(out.to_host(), U), f"fp32 smoothing N={N} step={step}"
        assert bits32(Fc.to_host(), o32.restrict_neg_residual(mg, U, F, 1.0, M)), f"fp32 restriction {N}->{M}"
        assert float(e.views[0].to_host()[0, 0]) == pytest.approx(werr, rel=1e-12)
        b.check(f"mg_smooth_restrict_f32 {N}->{M} step={step}"); e.check("error slot")
        out.poison()
        b.expect_readonly(Fd, Uin, c, Fc)
        mg.lib().mg_prolong_smooth_f32(M, c.ptr, N, 1.0, Uin.ptr, out.ptr, Fd.ptr, step, e.views[0].ptr)
        mg._check()
        want, werr = o32.smooth(o32.prolong_add(mg, Uc, Uf), F, step, 1.0)
        assert bits32(out.to_host(), want), f"fp32 prolong+smooth {M}->{N} step={step}"
        assert float(e.views[0].to_host()[0, 0]) == pytest.approx(werr, rel=1e-12)
        b.check(f"mg_prolong_smooth_f32 {M}->{N} step={step}"); e.check("error slot")
    finally:
        b.free(); e.free()


# ------------------------------------------------------------------ solvers
SOLVE_N = [64, 65, 100, 257, 1024, 1025, 2048]
SOLVE_OPTS = [dict(pre=a, post=a, omega=w) for a in (1, 3, 4) for w in (0.8, 1.0)]


def _opts_id(o):
    return f"V{o['pre']}{o['post']}-w{o['omega']:g}"


@pytest.mark.parametrize("place", PLACE)
@pytest.mark.parametrize("opts", SOLVE_OPTS, ids=_opts_id)
@pytest.mark.parametrize("N", SOLVE_N)
def test_solver_on_a_caller_block(mg, oracle, N, opts, place):
    """Solver.solve_ptr on arrays inside a caller's block: one cycle against the restatement (input qualified, DESIGN.md
    4.3), F read only, bands intact."""
    F, U0 = ref.random_problem(N, 4000 + N + 13 * opts["pre"])
    margins = []
    want = ref.cycle(oracle, F, U0, 1.0, margins=margins, **opts)
    ref.assert_qualified(margins, f"N={N} {opts}")
    b = _guard.block(mg, [N, N], place)
    s = mg.Solver(N, 1.0, rtol=0.0, atol=0.0, max_cycles=1, **opts)
    try:
        Fd, Ud = b.views
        Fd.upload(F); Ud.upload(U0)
        b.expect_readonly(Fd)
        info = s.solve_ptr(Fd.ptr, Ud.ptr)
        assert info["cycles"] == 1 and not info["coarse_capped"]
        assert_bits(Ud.to_host(), want, f"Solver N={N} {opts} {place}", zero_sign=True)
        b.check(f"mg_solver_solve N={N} {opts}")
    finally:
        s.close(); b.free()


KEYS = ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm", "history")


@pytest.mark.parametrize("place", PLACE)
@pytest.mark.parametrize("N,B", [(N, B) for N in SOLVE_N for B in (1, 3, 16)])
def test_batch_solver_on_one_packed_block(mg, oracle, N, B, place):
    """BatchSolver.solve_ptrs on B instances packed back to back in ONE block (a band between neighbours), the last
    instance sharing the first one's F, and -- for B >= 3 -- the middle instance converged at the start (a start that one
    sweep would visibly change): its U and both its bands come back bit-identical while its neighbours run every cycle.  Each instance against its single solve."""
    opts = dict(rtol=0.0, atol=1e-2, max_cycles=2)
    mid = B // 2 if B >= 3 else -1
    probs = [ref.random_problem(N, 700 + N + 97 * i) for i in range(B)]
    if mid >= 0:
        # a random U with F = A U + d, |d| <= 5e-4 / N: the residual norm is about 3e-4, below atol, so the instance is
        # converged at the start -- but one sweep would move U by 0.2 dx^2 |d| (7e-11 at N = 64, 1e-14 = 100 ulp at
        # N = 2048): an instance wrongly kept in the batch comes back with other bits.  (The random neighbours start
        # with residuals above 1e4 and stay far above atol after two cycles.)
        F_mid, U_mid = probs[mid]
        probs[mid] = (oracle.getResidual(N, 1.0, U_mid, np.zeros((N, N))) + F_mid * (1e-3 / N), U_mid)
    share = B >= 3
    nF = B - 1 if share else B
    b = _guard.block(mg, [N] * (nF + B), place)
    bs = mg.BatchSolver(N, 1.0, max_batch=B, **opts)
    s = mg.Solver(N, 1.0, **opts)
    try:
        Fv = [b.views[2 * i] if i < nF else None for i in range(B)]        # F_0 U_0 F_1 U_1 ... interleaved
        Uv = [b.views[2 * i + 1] if i < nF else b.views[2 * nF + (i - nF)] for i in range(B)]
        if share:
            Fv[B - 1] = Fv[0]
            probs[B - 1] = (probs[0][0], probs[B - 1][1])
        for i in range(B):
            if i < nF:
                Fv[i].upload(probs[i][0])
            Uv[i].upload(probs[i][1])
        ro = [v for v in Fv[:nF]] + ([Uv[mid]] if mid >= 0 else [])
        b.expect_readonly(*ro)
        infos = bs.solve_ptrs([f.ptr for f in Fv], [u.ptr for u in Uv])
        for i, (F, U0) in enumerate(probs):
            want_U, want = s.solve(F, U0)
            what = f"N={N} B={B} instance {i} ({place})"
            assert_bits(Uv[i].to_host(), want_U, what + " U")
            if i == mid:
                assert_bits(Uv[i].to_host(), U0, what + " U of the converged start")
                assert infos[i]["cycles"] == 0 and infos[i]["converged"], what
            else:
                assert infos[i]["cycles"] == 2, what
            for k in KEYS:
                assert infos[i][k] == want[k], f"{what} {k}: {infos[i][k]} != {want[k]}"
        b.check(f"mg_batch_solver_solve N={N} B={B}")
    finally:
        s.close(); bs.close(); b.free()


# ------------------------------------------------------------------ uninitialised scratch of the operators
def _prime_pool(mg, byte_sizes):
    """mg_alloc blocks of exactly the sizes the coming call will ask the (exact-size, 256 B-rounded) pool for, fill them
    with the NaN pattern and free them: the call then gets those very blocks.  Returns mg_pool_bytes() afterwards."""
    lib = mg.lib()
    ptrs = []
    for nbytes in byte_sizes:
        n = (nbytes + 255) // 256 * 256 // 8
        p = lib.mg_alloc(n)
        mg._check()
        pat = np.full(n, _guard.PATTERN, dtype=np.uint64)
        lib.mg_upload(p, pat.ctypes.data, n)
        ptrs.append(p)
    for p in ptrs:
        lib.mg_free(p)
    mg.sync()
    return lib.mg_pool_bytes()


@pytest.mark.parametrize("sm,N,M", with_smoothers([(64, 32), (65, 32), (100, 37), (256, 128), (257, 128), (1024, 512), (1025, 512), (2050, 1025)]))
@pytest.mark.parametrize("step", [1, 2, 3, 6])
def test_operator_scratch_may_hold_anything(mg, oracle, smoother, sm, N, M, step):
    """The scratch of mg_doSmoothing (odd and even step counts: the ping-pong partner), mg_smooth_restrict and
    mg_prolong_smooth (fusable and operator-by-operator sizes) is handed out holding NaN: results unchanged, and the
    call allocated nothing new (so it did get the poisoned blocks)."""
    U0, F = rand_pair(N, 5 * N + step)
    Uc = np.random.default_rng(N).random((M, M)) - 0.5
    nb = N * N * 8
    Fd, U, out, Fc, c = (mg.DeviceGrid.from_host(F), mg.DeviceGrid.from_host(U0), mg.DeviceGrid(N), mg.DeviceGrid(M),
                         mg.DeviceGrid.from_host(Uc))
    try:
        held = _prime_pool(mg, [nb, nb, nb])
        err = mg.doSmoothing(N, 1.0, U, Fd, step)
        want, werr = oracle.doSmoothing(N, 1.0, U0, F, step)
        assert_bits(U.to_host(), want, f"doSmoothing on poisoned scratch N={N} step={step}")
        assert err == pytest.approx(werr, rel=REL)
        assert mg.lib().mg_pool_bytes() == held
        U.free(); U = mg.DeviceGrid.from_host(U0)
        for Uin, start in ((None, np.zeros((N, N))), (U, U0)):
            held = _prime_pool(mg, [nb, nb, nb])
            mg.smooth_restrict(N, 1.0, Uin, out, Fd, step, M, Fc)
            want_U, _ = oracle.doSmoothing(N, 1.0, start, F, step)
            assert_bits(out.to_host(), want_U, f"smooth_restrict on poisoned scratch N={N} step={step}")
            assert_bits(Fc.to_host(), oracle.doRestriction(N, -oracle.getResidual(N, 1.0, want_U, F), M), "F_c")
            assert mg.lib().mg_pool_bytes() == held
        held = _prime_pool(mg, [nb, nb, nb])
        mg.prolong_smooth(M, c, N, 1.0, U, out, Fd, step)
        want0 = oracle.doGridAddition(N, U0, oracle.doProlongation(M, Uc, N, fill=0.0))
        assert_bits(out.to_host(), oracle.doSmoothing(N, 1.0, want0, F, step)[0], f"prolong_smooth on poisoned scratch N={N}")
        assert mg.lib().mg_pool_bytes() == held
    finally:
        for g in (Fd, U, out, Fc, c):
            g.free()
        mg.lib().mg_pool_trim()


@pytest.mark.parametrize("N,M", [(64, 32), (66, 33), (257, 128), (100, 37), (1024, 512)])
@pytest.mark.parametrize("step", [1, 3, 4])
def test_operator_scratch_f32_may_hold_anything(mg, N, M, step):
    rng = np.random.default_rng(N + step)
    F = (rng.random((N, N)) - 0.5).astype(np.float32)
    Uc, Uf = (rng.random((M, M)) - 0.5).astype(np.float32), rng.random((N, N)).astype(np.float32)
    Fd, out, Fc = mg.DeviceGrid32.from_host(F), mg.DeviceGrid32((N, N)), mg.DeviceGrid32((M, M))
    c, Uin = mg.DeviceGrid32.from_host(Uc), mg.DeviceGrid32.from_host(Uf)
    try:
        held = _prime_pool(mg, [N * N * 4, N * N * 4])
        mg.smooth_restrict_f32(N, 1.0, out, Fd, step, M, Fc)
        U, _ = o32.smooth(np.zeros((N, N), dtype=np.float32), F, step, 1.0)
        assert bits32(out.to_host(), U) and bits32(Fc.to_host(), o32.restrict_neg_residual(mg, U, F, 1.0, M))
        assert mg.lib().mg_pool_bytes() == held
        held = _prime_pool(mg, [N * N * 4, N * N * 4])
        mg.prolong_smooth_f32(M, c, N, 1.0, Uin, out, Fd, step)
        assert bits32(out.to_host(), o32.smooth(o32.prolong_add(mg, Uc, Uf), F, step, 1.0)[0])
        assert mg.lib().mg_pool_bytes() == held
    finally:
        for g in (Fd, out, Fc, c, Uin):
            g.free()
        mg.lib().mg_pool_trim()


# ------------------------------------------------------------------ MG_POOL_POISON: plans and solvers
def _run_plan(mg, path, **kw):
    plan = mg.CyclePlan(path, **kw)
    try:
        a = plan.execute(fetch_U=True)
        bb = plan.execute(fetch_U=True)
    finally:
        plan.close()
    assert a["status"] == 0 and bb["status"] == 0
    assert_bits(a["U"], bb["U"], "two windows of one plan")
    return a


@pytest.mark.parametrize("mode", ["fused", "unfused", "graph"])
@pytest.mark.parametrize("name", ["test.txt", "Vcycle.txt", "Wcycle.txt", "VcycleTrigger.txt", "genV", "genW"])
def test_plans_on_poisoned_pools(mg, oracle, cycle_dir, tmp_path, monkeypatch, name, mode):
    """Every array a cycle plan's pool hands out starts as NaN (MG_POOL_POISON): the shipped files and a generated V and W
    still give the oracle's bits, and two windows back to back agree."""
    if name == "genV":
        path = str(tmp_path / "v.txt"); mg.write_vcycle_file(path, 1024, 8, 3, 1e-7)
    elif name == "genW":
        path = str(tmp_path / "w.txt"); mg.write_wcycle_file(path, 512, 8, 2, 1e-7)
    else:
        path = os.path.join(cycle_dir, name)
    want = oracle.run_cycle_file(path)
    monkeypatch.setenv("MG_POOL_POISON", "1")
    got = _run_plan(mg, path, fused=mode != "unfused", graph=mode == "graph")
    assert_bits(got["U"], want["U"], f"{name} {mode} on a poisoned pool", zero_sign=True)
    assert got["mg_error"] == pytest.approx(want["mg_error"], rel=1e-12)


@pytest.mark.parametrize("mode", ["fused", "unfused"])
@pytest.mark.parametrize("name", ["Wcycle.txt", "genV", "genW"])
def test_interpreted_plans_on_poisoned_pools(oracle, cycle_dir, tmp_path, name, mode):
    """The same with MG_CYCLE_BATCH=0 (read once per process: a child): the W-cycles node by node, in file order -- level
    arrays returned to the plan's pool and handed out again between visits, tempU, the ping-pong partners -- every block
    NaN-filled each time it is handed out."""
    if name == "genV":
        path = str(tmp_path / "v.txt"); mgmod_write(path, "V")
    elif name == "genW":
        path = str(tmp_path / "w.txt"); mgmod_write(path, "W")
    else:
        path = os.path.join(cycle_dir, name)
    want = oracle.run_cycle_file(path)
    out_npy = str(tmp_path / "U.npy")
    env = dict(os.environ, MG_POOL_POISON="1", MG_CYCLE_BATCH="0")
    run = subprocess.run([sys.executable, os.path.join(HERE, "_poison_plan_worker.py"), path, mode, out_npy], env=env,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "POISON_PLAN OK" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
    got = json.loads([l for l in run.stdout.splitlines() if l.startswith("POISON_PLAN OK ")][-1][len("POISON_PLAN OK "):])
    assert got["schedule_launches"] == 0, "the plan was to run node by node"
    assert_bits(np.load(out_npy), want["U"], f"{name} {mode} interpreted on a poisoned pool", zero_sign=True)
    assert got["mg_error"] == pytest.approx(want["mg_error"], rel=1e-12)


def mgmod_write(path, kind):
    import multigrid_poisson_solver_amd as m
    if kind == "V":
        m.write_vcycle_file(path, 1024, 8, 3, 1e-7)
    else:
        m.write_wcycle_file(path, 512, 8, 2, 1e-7)


def test_mixed_plan_with_refinement_on_a_poisoned_pool(mg, oracle, tmp_path, monkeypatch):
    N, n_min = 256, 8
    path = str(tmp_path / "c.txt")
    mg.write_vcycle_file(path, N, n_min, 3, 1e-7)
    plain = _run_plan(mg, path, fused=True, mixed=True, refinement=2)
    monkeypatch.setenv("MG_POOL_POISON", "1")
    got = _run_plan(mg, path, fused=True, mixed=True, refinement=2)
    assert_bits(got["U"], plain["U"], "mixed plan, refinement 2: poisoned pool vs plain")
    assert got["refinement_errors"] == plain["refinement_errors"]
    toks = open(path).read().split()
    U, _ = o32.refine(mg, oracle, oracle.getSource(N), 1.0, 3, ref.sizes(N, n_min), toks[7:], 2)[:2]
    assert_bits(got["U"], U, "mixed plan, refinement 2 vs the numpy restatement")


@pytest.mark.parametrize("N", [100, 257, 1024])
def test_solvers_on_poisoned_level_arrays(mg, oracle, monkeypatch, N):
    F, U0 = ref.random_problem(N, 4000 + N + 13 * 3)
    margins = []
    want = ref.cycle(oracle, F, U0, 1.0, margins=margins)
    ref.assert_qualified(margins, f"N={N}")
    monkeypatch.setenv("MG_POOL_POISON", "1")
    for smoother in ("stream", "simple"):
        mg.set_smoother(smoother)
        try:
            got, info = mg.solve(F, U0, 1.0, rtol=0.0, max_cycles=1)
            assert_bits(got, want, f"Solver on poisoned level arrays N={N} ({smoother})", zero_sign=True)
            Us, infos = mg.solve_batched(np.stack([F] * 3), np.stack([U0] * 3), 1.0, rtol=0.0, max_cycles=1)
            for i in range(3):
                assert_bits(Us[i], want, f"BatchSolver on poisoned level arrays N={N} instance {i} ({smoother})", zero_sign=True)
        finally:
            mg.set_smoother("stream")


def test_poison_knob_unset_leaves_the_launch_sequence_alone(mg, tmp_path, monkeypatch):
    """The same plan with and without MG_POOL_POISON: equal kernel lists (name, N, launches) from mg_profile_end."""
    path = str(tmp_path / "v.txt")
    mg.write_vcycle_file(path, 1024, 8, 3, 1e-7)

    def launches():
        plan = mg.CyclePlan(path, fused=True)
        plan.execute()
        mg.profile_begin(0)
        plan.execute()
        prof = mg.profile_end()
        plan.close()
        return sorted((p["name"], p["N"], p["launches"]) for p in prof)

    monkeypatch.delenv("MG_POOL_POISON", raising=False)
    plain = launches()
    monkeypatch.setenv("MG_POOL_POISON", "1")
    assert launches() == plain and plain


# ------------------------------------------------------------------ product thresholds
@pytest.mark.parametrize("N", [4096, 4098, 8192, 8194])
def test_product_thresholds_in_guarded_blocks(golden_fullsize, N):
    """A child process without the suite's MG_* overrides: smoothing (1 and 3 sweeps), residual, restriction,
    prolongation, the two fused nodes and two solver cycles at N on mg_fill_uniform inputs inside guarded blocks.  Outputs
    against tests/golden/golden_fullsize.json where it has the entry, else against the same call on plain mg_alloc arrays
    in the child; bands and inputs by checksum before / after (asserted in the child)."""
    env = {k: v for k, v in os.environ.items() if not (k.startswith("MG_") and k not in ("MG_LIB", "MG_DEVICE", "MG_HIP_RUNTIME"))}
    out = subprocess.run([sys.executable, os.path.join(HERE, "_memory_contract_big_worker.py"), str(N)], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("MEMORY_BIG ")][-1]
    got = json.loads(line[len("MEMORY_BIG "):])
    if f"residual_N{N}" in golden_fullsize:   # (4098 and 8194 -- N mod PR = 2, N/2 no whole number of blocks -- have no
        # entry: the child holds them to the same calls on plain arrays, in both smoothers)
        assert got["residual"] == golden_fullsize[f"residual_N{N}"]["checksum"]
        assert got["smooth3"] == golden_fullsize[f"smooth3_N{N}"]["checksum"]
        assert got["smooth3_err"] == pytest.approx(golden_fullsize[f"smooth3_N{N}"]["error"], rel=REL)
    if f"restrict_{N}to{N // 2}" in golden_fullsize:
        assert got["restrict"] == golden_fullsize[f"restrict_{N}to{N // 2}"]["checksum"]
    if f"prolong_{N // 2}to{N}" in golden_fullsize:
        assert got["prolong"] == golden_fullsize[f"prolong_{N // 2}to{N}"]["checksum"]
    assert got["checks"] >= 2 * 11
