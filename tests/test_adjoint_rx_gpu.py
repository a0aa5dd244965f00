"""The adjoint of reaction and semilinear solves (include/mg_adjoint_rx.h) on the device: the source-gradient kernel and its
batched twin bit for bit against the restatement (tests/_adjoint_rx_ref.py), G and the sum, over every form and inside guard
bands; the four drivers against the caller's own sequence of public calls and against one another, bit for bit; the adjoint
field and the gradients in w and kappa against the dense solve at the device's own U within an a-priori bound; state and
refusals; torch.autograd in a child process.

Measured on the MI355X (error / a-priori bound of test_truth, the largest over its six cases): lam 1.0e-01, gW 1.0e-01,
gkappa 2.1e-02."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import _adjoint_ref as aref
import _adjoint_rx_ref as xref
import _guard
import _newton_ref as nref
import _reaction_ref as rref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LD = vref.LD
NAN_BITS = np.uint64(0xFFFFFFFFFFFFFFFF)
KERNEL_SIZES = [3, 4, 5, 33, 64, 65, 130, 512, 513, 514]   # column form, pair form (even N >= 512), odd N above the threshold
INFO_KEYS = ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm", "history")
KAPPA = 0.7


def poison_host(N):
    return np.full((N, N), NAN_BITS, dtype=np.uint64).view(np.float64)


def poisoned(mg, N):
    return mg.DeviceGrid.from_host(poison_host(N))


def kernel_fields(N, seed):
    """lam with a non-zero random rim (the kernel must not use it), U of order one, w in [1, 2)"""
    rng = np.random.default_rng(seed)
    lam, U, w = rng.standard_normal((N, N)), rng.standard_normal((N, N)), 1.0 + rng.random((N, N))
    lam[0, :] += 3.0
    lam[-1, :] -= 5.0
    lam[:, 0] += 7.0
    lam[:, -1] -= 2.0
    return lam, U, w


def same_sum(got, want, what):
    assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (what, got, want)


def check_kernel(mg, N, kinds):
    lam, U, w = kernel_fields(N, 10 + N)
    ld, Ud, wd, clean = (mg.DeviceGrid.from_host(x) for x in (lam, U, w, aref.zero_rim(lam)))
    for kind in kinds:
        for w_dev, w_host in ((wd, w), (None, None)):
            what = f"N={N} {kind} w={'given' if w_host is not None else 'NULL'}"
            want_G, want_sum = xref.source_gradient(N, kind, KAPPA, w_host, lam, U)
            out = poisoned(mg, N)
            G, s = mg.sourceGradient(N, kind, KAPPA, w_dev, ld, Ud, out)
            assert_bits(G.to_host(), want_G, what + ": G")
            same_sum(s, want_sum, what + ": sum")
            # the rim of lam is never used
            G0, s0 = mg.sourceGradient(N, kind, KAPPA, w_dev, clean, Ud)
            assert_bits(G0.to_host(), want_G, what + ": G, zero rim of lam")
            same_sum(s0, want_sum, what + ": sum, zero rim of lam")


# ---------------------------------------------------------------- 1. the kernel against the restatement
@pytest.mark.parametrize("N", KERNEL_SIZES)
def test_kernel_bit_identical_to_restatement(mg, N):
    check_kernel(mg, N, xref.KINDS)


def test_kernel_non_temporal_form(mg):
    """N = 4096: non-temporal loads of w and stores of G; cubic and linear only (numpy's exp restatement is slow there)"""
    check_kernel(mg, 4096, ("cubic", "linear"))


def test_kernel_front_ends(mg):
    """numpy arrays in, numpy arrays out: the same call"""
    N = 33
    lam, U, w = kernel_fields(N, 1)
    G, s = mg.sourceGradient(N, "sinh", KAPPA, w, lam, U)
    want_G, want_sum = xref.source_gradient(N, "sinh", KAPPA, w, lam, U)
    assert isinstance(G, np.ndarray)
    assert_bits(G, want_G, "numpy front end")
    same_sum(s, want_sum, "numpy front end: sum")


@pytest.mark.parametrize("N", [33, 512])
def test_batched_twins_equal_the_single_launches(mg, N):
    """B = 3 distinct instances with distinct kappa in one launch; w none, one shared, one per instance"""
    B = 3
    kap = [0.7, 0.0, 2.5]
    sets = [kernel_fields(N, 50 + 7 * i + N) for i in range(B)]
    lam = [mg.DeviceGrid.from_host(s[0]) for s in sets]
    U = [mg.DeviceGrid.from_host(s[1]) for s in sets]
    w = [mg.DeviceGrid.from_host(s[2]) for s in sets]
    for kind in xref.KINDS:
        for mode, w_arg, w_of in (("none", None, lambda i: None), ("shared", w[0], lambda i: 0), ("each", w, lambda i: i)):
            G, sums = mg.sourceGradient_batch(N, kind, kap, w_arg, lam, U, [poisoned(mg, N) for _ in range(B)])
            for i in range(B):
                what = f"N={N} {kind} w {mode} instance {i}"
                j = w_of(i)
                G1, s1 = mg.sourceGradient(N, kind, kap[i], None if j is None else w[j], lam[i], U[i])
                assert_bits(G[i].to_host(), G1.to_host(), what + ": G against the single launch")
                same_sum(sums[i], s1, what + ": sum against the single launch")
                want_G, want_sum = xref.source_gradient(N, kind, kap[i], None if j is None else sets[j][2], sets[i][0], sets[i][1])
                assert_bits(G[i].to_host(), want_G, what + ": G against numpy")
                same_sum(sums[i], want_sum, what + ": sum against numpy")


# ---------------------------------------------------------------- 2. guard bands
@pytest.mark.parametrize("place", list(_guard.PLACEMENTS))
@pytest.mark.parametrize("N", [65, 512])
def test_kernels_inside_guard_bands(mg, N, place):
    """the output is written inside its array only (every element of it), inputs are unchanged; single and batched"""
    lam, U, w = kernel_fields(N, 90 + N)
    with _guard.block(mg, [N] * 5, place) as b:
        wv, lv, Uv, Gv, G2v = b.views
        for v, x in ((wv, w), (lv, lam), (Uv, U)):
            v.upload(x)
        for kind in ("sinh", "linear"):
            want_G, want_sum = xref.source_gradient(N, kind, KAPPA, w, lam, U)
            Gv.poison()
            G2v.poison()
            b.expect_readonly(wv, lv, Uv, G2v)
            _, s = mg.sourceGradient(N, kind, KAPPA, wv, lv, Uv, Gv)
            assert_bits(Gv.to_host(), want_G, f"G N={N} {kind} {place}")
            same_sum(s, want_sum, f"sum N={N} {kind} {place}")
            b.check(f"mg_sourceGradient N={N} {kind} {place}")
            # the batched twin on the same block: two instances sharing the inputs, the second without its kappa
            Gv.poison()
            b.expect_readonly(wv, lv, Uv)
            _, sums = mg.sourceGradient_batch(N, kind, [KAPPA, 1.0], wv, [lv, lv], [Uv, Uv], [Gv, G2v])
            assert_bits(Gv.to_host(), want_G, f"batched G N={N} {kind} {place}")
            assert_bits(G2v.to_host(), xref.source_gradient(N, kind, 1.0, w, lam, U)[0], f"batched G N={N} {kind} {place}: second")
            same_sum(sums[0], want_sum, f"batched sum N={N} {kind} {place}")
            same_sum(sums[1], want_sum, f"batched sum N={N} {kind} {place}: second (the sum does not hold kappa)")
            b.check(f"mg_sourceGradient_batch N={N} {kind} {place}")


# ---------------------------------------------------------------- 3. the drivers are the caller's sequence of public calls
CONFIGS = {
    "plain": dict(),
    "coef": dict(coef="smooth"),
    "coef_shift": dict(coef="smooth", shift=1e2),
    "krylov_jump": dict(coef="jump", krylov=4),
}


def driver_problem(N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, N)), rng.standard_normal((N, N))   # Ubar, U


def same_info(info, want, what):
    for key in INFO_KEYS:
        assert info[key] == want[key], (what, key)
    if "breakdown" in want:
        assert info["breakdown"] == want["breakdown"], what


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("N", [33, 65, 514])
def test_reaction_driver_equals_the_public_calls(mg, N, config):
    """mg_solver_adjoint_reaction against {set_reaction, mg_fill_zero, mg_solver_solve, mg_coefficientGradient,
    mg_boundaryGradient, mg_sourceGradient(linear, 1, NULL)}: lam, gA, gU, gS, gshift, history, cycles and flags bit for bit"""
    L = 1.0
    opts = dict(CONFIGS[config])
    name = opts.pop("coef", None)
    a = vref.field(name, N, seed=N) if name else None
    react = rref.field("smooth", N)
    Ubar, U = driver_problem(N, 300 + N)
    ubd, Ud = mg.DeviceGrid.from_host(Ubar), mg.DeviceGrid.from_host(U)
    ad = mg.DeviceGrid.from_host(a) if a is not None else None
    s = mg.Solver(N, L, coef=a, **opts)
    try:
        s.set_reaction(react)
        lam2 = poisoned(mg, N)
        mg.lib().mg_fill_zero(lam2.ptr, N * N)
        want_info = s.solve_ptr(ubd.ptr, lam2.ptr)
        gA2 = mg.coefficientGradient(N, L, lam2, Ud)
        gU2 = mg.boundaryGradient(N, L, ad, lam2, ubd)
        gS2, gshift2 = mg.sourceGradient(N, "linear", 1.0, None, lam2, Ud)
        lam, gA, gU, gS, info = s.adjoint_reaction(ubd, Ud)
        what = f"N={N} {config}"
        assert info["cycles"] > 0 and info["converged"] and s.has_reaction, what
        same_info(info, want_info, what)
        for got, want, nm in ((lam, lam2, "lam"), (gA, gA2, "gA"), (gU, gU2, "gU"), (gS, gS2, "gS")):
            assert_bits(got.to_host(), want.to_host(), f"{what}: {nm}")
        same_sum(info["gshift"], gshift2, what + ": gshift")
        assert_bits(gS.to_host(), xref.source_gradient(N, "linear", 1.0, None, lam.to_host(), U)[0], what + ": gS against numpy")
        # the numpy front end is the same call; gradients that are not wanted are not made
        lam_h, gA_h, gU_h, gS_h, info_h = s.adjoint_reaction(Ubar, U, want_coef=False, want_rim=False)
        assert gA_h is None and gU_h is None
        assert_bits(lam_h, lam2.to_host(), what + ": numpy lam")
        assert_bits(gS_h, gS2.to_host(), what + ": numpy gS")
        same_sum(info_h["gshift"], gshift2, what + ": numpy gshift")
        assert s.adjoint_reaction(Ubar, U, want_reaction=False)[4]["gshift"] is None
    finally:
        s.close()


@pytest.mark.parametrize("kind", nref.KINDS)
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("N", [33, 65, 514])
def test_newton_driver_equals_the_public_calls(mg, N, config, kind):
    """mg_solver_newton_adjoint against {mg_nonlinearResidual (no step) -> S, set_reaction(S), mg_fill_zero, mg_solver_solve,
    mg_coefficientGradient, mg_boundaryGradient, mg_sourceGradient(kind, kappa, w)}, bit for bit, res_forward included"""
    L = 1.0
    opts = dict(CONFIGS[config])
    name = opts.pop("coef", None)
    shift = opts.get("shift", 0.0)
    a = vref.field(name, N, seed=N) if name else None
    w = nref.smooth_weight(N, L)
    rng = np.random.default_rng(400 + N)
    Ubar, U, F = rng.standard_normal((N, N)), rng.standard_normal((N, N)), 40.0 * rng.standard_normal((N, N))
    ubd, Ud, Fd, wd = (mg.DeviceGrid.from_host(x) for x in (Ubar, U, F, w))
    ad = mg.DeviceGrid.from_host(a) if a is not None else None
    s = mg.Solver(N, L, coef=a, **opts)
    try:
        D, S = poisoned(mg, N), poisoned(mg, N)
        res2 = mg.nonlinear_residual(N, L, shift, ad, kind, KAPPA, wd, Ud, Fd, D, S)
        s.set_reaction(S)
        lam2 = poisoned(mg, N)
        mg.lib().mg_fill_zero(lam2.ptr, N * N)
        want_info = s.solve_ptr(ubd.ptr, lam2.ptr)
        s.set_reaction(None)
        gA2 = mg.coefficientGradient(N, L, lam2, Ud)
        gU2 = mg.boundaryGradient(N, L, ad, lam2, ubd)
        gW2, gkappa2 = mg.sourceGradient(N, kind, KAPPA, wd, lam2, Ud)
        lam, gA, gU, gW, info = s.newton_adjoint(ubd, Ud, Fd, kind=kind, kappa=KAPPA, weight=wd)
        what = f"N={N} {config} {kind}"
        assert info["cycles"] > 0 and info["converged"] and not s.has_reaction, what
        same_info(info, want_info, what)
        for got, want, nm in ((lam, lam2, "lam"), (gA, gA2, "gA"), (gU, gU2, "gU"), (gW, gW2, "gW")):
            assert_bits(got.to_host(), want.to_host(), f"{what}: {nm}")
        same_sum(info["gkappa"], gkappa2, what + ": gkappa")
        same_sum(info["res_forward"], res2, what + ": res_forward")
    finally:
        s.close()


@pytest.mark.parametrize("N", [33, 514])
def test_reaction_driver_identity_contracts(mg, N):
    """without a reaction set lam, gA and gU are Solver.adjoint's; s == c at sigma = 0 gives Solver(shift=c).adjoint's"""
    L, c = 1.0, 1e3
    a = vref.field("smooth", N, seed=N)
    Ubar, U = driver_problem(N, 500 + N)
    plain, shifted, react = mg.Solver(N, L, coef=a), mg.Solver(N, L, coef=a, shift=c), mg.Solver(N, L, coef=a, reaction=np.full((N, N), c))
    try:
        want = plain.adjoint(Ubar, U)
        got = plain.adjoint_reaction(Ubar, U)
        for x, y, nm in zip(got[:3], want[:3], ("lam", "gA", "gU")):
            assert_bits(x, y, f"N={N} no reaction: {nm}")
        same_info(got[4], want[3], f"N={N} no reaction")
        assert_bits(got[3], xref.source_gradient(N, "linear", 1.0, None, got[0], U)[0], f"N={N} no reaction: gS at s = 0")
        want = shifted.adjoint(Ubar, U)
        got = react.adjoint_reaction(Ubar, U)
        for x, y, nm in zip(got[:3], want[:3], ("lam", "gA", "gU")):
            assert_bits(x, y, f"N={N} s == c: {nm}")
        same_info(got[4], want[3], f"N={N} s == c")
    finally:
        plain.close(); shifted.close(); react.close()


# ---------------------------------------------------------------- 4. truth at the device's own U
TRUTH_RATIOS = {}


@pytest.mark.parametrize("kind", nref.KINDS)
@pytest.mark.parametrize("N", [17, 33])
def test_truth(mg, N, kind):
    """The device's forward solution U (Newton to rtol 1e-10) is taken as given; lam* is the dense longdouble solve of
    (A - S(U)) lam = Ubar with S = kappa*w*g'(U) (tests/_adjoint_rx_ref.py).  With M = -(A - S) and r(x) its longdouble residual,
    lam_dev - lam* = M^-1 (r(lam_dev) - r(lam*)), so at every point
        |lam_dev - lam*| <= ||M^-1||_inf * (||r(lam_dev)||_inf + ||r(lam*)||_inf) =: e
    (the norm from the fp64 inverse, with test_solve_reaction_gpu's 1e-6 for it).  This is the issue's
    ||A^-1||_inf * ||r_ld(lam_dev)||_inf plus the residual of the dense reference itself, which the identity needs because lam*
    is computed, not exact (the test prints both residuals: the reference's is 2e-18 or less beside 5e-11 .. 1e-10).  Then
        |gW - kappa*lam* g(U)| <= kappa*e*|g(U)| + 4 ulp of the product       (g, lam*g, kappa*m: at most 4 roundings)
        |gkappa - sum w lam* g(U)| <= sum w*e*|g(U)| + gamma_(n+4) * sum |w lam g(U)|,   n = (N-2)^2 terms.
    Measured on the MI355X, the largest error/bound over the six cases: lam 1.0e-01, gW 1.0e-01, gkappa 2.1e-02."""
    L, shift = 1.0, 0.0
    rng = np.random.default_rng(1000 + N)
    a, w = vref.field("smooth", N, L), nref.smooth_weight(N, L)
    F, U0, W = 40.0 * rng.standard_normal((N, N)), rng.standard_normal((N, N)), rng.standard_normal((N, N))
    s = mg.Solver(N, L, coef=a, shift=shift, rtol=1e-10)
    try:
        U, fi = s.newton(F, U0, kind=kind, kappa=KAPPA, weight=w, rtol=1e-10)
        lam, gA, gU, gW, ai = s.newton_adjoint(W, U, F, kind=kind, kappa=KAPPA, weight=w)
    finally:
        s.close()
    assert fi["converged"] and ai["converged"]
    u53 = float(vref.U53)
    S = xref.linearised_reaction(N, kind, KAPPA, w, U)
    lam_ref, nA = xref.direct_adjoint(a, S, W, L, shift)
    lam0 = aref.zero_rim(lam)
    r_dev = float(np.max(np.abs(rref.residual_ld(a, S, lam0, W, L, shift))))
    r_ref = float(np.max(np.abs(rref.residual_ld(a, S, lam_ref, W, L, shift))))
    e = float(nA) * (1.0 + 1e-6) * (r_dev + r_ref)
    g = np.asarray(xref._g_ld(kind, U), dtype=LD)
    i = (slice(1, -1), slice(1, -1))
    gW_ref = LD(KAPPA) * lam_ref * g
    bW = KAPPA * e * np.abs(g) + 4.0 * u53 * np.abs(gW_ref)
    rL = float(np.max(np.abs(lam0 - lam_ref))) / e
    rW = float(np.max((np.abs(gW - gW_ref) / bW)[i]))
    terms = np.asarray(w, dtype=LD) * lam_ref * g
    n = (N - 2) ** 2 + 4
    bK = float(np.sum((w * e * np.abs(g))[i])) + n * u53 / (1.0 - n * u53) * float(np.sum(np.abs(terms[i])))
    rK = abs(float(LD(ai["gkappa"]) - np.sum(terms[i]))) / bK
    TRUTH_RATIOS[(N, kind)] = (rL, rW, rK)
    print(f"N={N} {kind}: res_forward {ai['res_forward']:.2e} r_dev {r_dev:.2e} r_ref {r_ref:.2e} e {e:.2e}; error/bound lam {rL:.3e} gW {rW:.3e} gkappa {rK:.3e}; largest so far "
          + " ".join(f"{nm} {max(v[k] for v in TRUTH_RATIOS.values()):.3e}" for k, nm in enumerate(("lam", "gW", "gkappa"))))
    assert rL <= 1.0 and rW <= 1.0 and rK <= 1.0, (rL, rW, rK)
    assert np.all(gW[0, :] == 0.0) and np.all(gW[:, 0] == 0.0)
    assert ai["res_forward"] == fi["res"]   # (the pass at the solution is the Newton driver's last accepted trial)


# ---------------------------------------------------------------- 5. the batched drivers
def batch_problem(N):
    """three instances with fields of their own; the second has Ubar == 0 (0 cycles, every gradient 0)"""
    x, y = vref.grid(N)
    rng = np.random.default_rng(5)
    a = [vref.field(n, N, seed=1) for n in ("smooth", "exp", "jump")]
    react = [rref.field("smooth", N), rref.field("blob", N), 1e2 * nref.smooth_weight(N)]
    w = [nref.smooth_weight(N), 1.0 + rng.random((N, N)), np.ones((N, N))]
    Ubar = [rng.standard_normal((N, N)), np.zeros((N, N)), np.sin(np.pi * x) * np.sin(np.pi * y)]
    U = [rng.standard_normal((N, N)) for _ in range(3)]
    F = [40.0 * rng.standard_normal((N, N)) for _ in range(3)]
    return a, react, w, Ubar, U, F


def test_batched_reaction_adjoint_equals_the_single_solver(mg):
    N, L, B = 65, 1.0, 3
    a, react, _, Ubar, U, _ = batch_problem(N)
    single = []
    for i in range(B):
        s = mg.Solver(N, L, coef=a[i], reaction=react[i])
        try:
            single.append(s.adjoint_reaction(Ubar[i], U[i]))
        finally:
            s.close()
    b = mg.BatchSolver(N, L, max_batch=B)
    try:
        for order in ((0, 1, 2), (2, 0, 1)):   # whatever their position
            pick = lambda X: np.stack([X[i] for i in order])
            b.set_coefficient(pick(a))
            b.set_reaction(pick(react))
            lam, gA, gU, gS, infos = b.adjoint_reaction(pick(Ubar), pick(U))
            assert b.has_reaction
            for j, i in enumerate(order):
                what = f"order {order} instance {i}"
                same_info(infos[j], single[i][4], what)
                same_sum(infos[j]["gshift"], single[i][4]["gshift"], what + ": gshift")
                for got, want, nm in zip((lam[j], gA[j], gU[j], gS[j]), single[i][:4], ("lam", "gA", "gU", "gS")):
                    assert_bits(got, want, f"{what}: {nm}")
            j = order.index(1)
            assert infos[j]["cycles"] == 0 and infos[j]["gshift"] == 0.0
            assert not (np.any(lam[j]) or np.any(gA[j]) or np.any(gU[j]) or np.any(gS[j]))
        # the gradient stage is four launches (coefficient, rim, source and its finish) whatever B is
        b.set_coefficient(np.stack(a))
        b.set_reaction(np.stack(react))
        infos3 = b.adjoint_reaction(np.stack(Ubar), np.stack(U))[4]
        stage3 = infos3[0]["stats"]["launches"] - b.solve(np.stack(Ubar))[1][0]["stats"]["launches"]
        one = b.adjoint_reaction(Ubar[0][None], U[0][None])[4]
        solve_one = b.solve(Ubar[0][None])[1]
        stage1 = one[0]["stats"]["launches"] - solve_one[0]["stats"]["launches"]
        assert stage1 == stage3 == 4, (stage1, stage3)
        none = b.adjoint_reaction(Ubar[0][None], U[0][None], want_coef=False, want_rim=False, want_reaction=False)[4]
        assert none[0]["stats"]["launches"] == solve_one[0]["stats"]["launches"]
    finally:
        b.close()


@pytest.mark.parametrize("weights", ["each", "shared", "none"])
def test_batched_newton_adjoint_equals_the_single_solver(mg, weights):
    N, L, B, kind = 65, 1.0, 3, "sinh"
    a, _, w, Ubar, U, F = batch_problem(N)
    kap = [0.7, 1.5, 0.2]
    w_of = {"each": lambda i: w[i], "shared": lambda i: w[0], "none": lambda i: None}[weights]
    w_arg = {"each": np.stack(w), "shared": w[0], "none": None}[weights]
    single = []
    for i in range(B):
        s = mg.Solver(N, L, coef=a[i])
        try:
            single.append(s.newton_adjoint(Ubar[i], U[i], F[i], kind=kind, kappa=kap[i], weight=w_of(i)))
        finally:
            s.close()
    b = mg.BatchSolver(N, L, max_batch=B)
    try:
        for order in ((0, 1, 2), (2, 0, 1)):   # whatever their position
            pick = lambda X: np.stack([X[i] for i in order])
            b.set_coefficient(pick(a))
            lam, gA, gU, gW, infos = b.newton_adjoint_batch(pick(Ubar), pick(U), pick(F), kind=kind, kappa=[kap[i] for i in order],
                                                            weight=pick(w) if weights == "each" else w_arg)
            assert not b.has_reaction
            for j, i in enumerate(order):
                what = f"w {weights} order {order} instance {i}"
                same_info(infos[j], single[i][4], what)
                same_sum(infos[j]["gkappa"], single[i][4]["gkappa"], what + ": gkappa")
                same_sum(infos[j]["res_forward"], single[i][4]["res_forward"], what + ": res_forward")
                for got, want, nm in zip((lam[j], gA[j], gU[j], gW[j]), single[i][:4], ("lam", "gA", "gU", "gW")):
                    assert_bits(got, want, f"{what}: {nm}")
            j = order.index(1)
            assert infos[j]["cycles"] == 0 and infos[j]["gkappa"] == 0.0 and not (np.any(lam[j]) or np.any(gW[j]))
        # three copies of one instance against that instance alone: the same launches, whatever B is
        b.set_coefficient(a[0])
        rep = lambda X: np.stack([X] * B)
        three = b.newton_adjoint_batch(rep(Ubar[0]), rep(U[0]), rep(F[0]), kind=kind, kappa=kap[0], weight=w_of(0))[4]
        one = b.newton_adjoint_batch(Ubar[0][None], U[0][None], F[0][None], kind=kind, kappa=kap[0], weight=w_of(0))[4]
        assert three[0]["stats"]["launches"] == one[0]["stats"]["launches"] > 0
        # and a following solve gives the bits of a fresh solver
        fresh = mg.BatchSolver(N, L, max_batch=B)
        try:
            fresh.set_coefficient(a[0])
            want = fresh.solve(F[0][None])
        finally:
            fresh.close()
        got = b.solve(F[0][None])
        assert_bits(got[0], want[0], "solve after newton_adjoint_batch")
        same_info(got[1][0], want[1][0], "solve after newton_adjoint_batch")
    finally:
        b.close()


# ---------------------------------------------------------------- 6. state and refusals
def test_state_after_newton_adjoint(mg):
    N, L = 65, 1.0
    a, w = vref.field("smooth", N, seed=N), nref.smooth_weight(N)
    rng = np.random.default_rng(9)
    Ubar, U, F = rng.standard_normal((N, N)), rng.standard_normal((N, N)), 40.0 * rng.standard_normal((N, N))
    s, fresh = mg.Solver(N, L, coef=a), mg.Solver(N, L, coef=a)
    try:
        s.newton_adjoint(Ubar, U, F, kind="exp", kappa=KAPPA, weight=w)
        assert not s.has_reaction
        got, want = s.solve(F), fresh.solve(F)
        assert_bits(got[0], want[0], "solve after newton_adjoint")
        same_info(got[1], want[1], "solve after newton_adjoint")
    finally:
        s.close(); fresh.close()


def test_not_converged_still_writes_the_gradients(mg):
    N, L = 65, 1.0
    rng = np.random.default_rng(7)
    Ubar, U, F = rng.standard_normal((N, N)), rng.standard_normal((N, N)), 40.0 * rng.standard_normal((N, N))
    w = nref.smooth_weight(N)
    s = mg.Solver(N, L, max_cycles=1, reaction=rref.field("smooth", N))
    try:
        lam, gA, gU, gS, info = s.adjoint_reaction(Ubar, U)
        assert info["status"] == mg.MG_SOLVE_NOT_CONVERGED and info["cycles"] == 1 and not info["converged"]
        assert_bits(gA, aref.coefficient_gradient(N, L, lam, U), "gA of an unconverged adjoint solve")
        assert_bits(gU, aref.boundary_gradient(N, L, None, lam, Ubar), "gU of an unconverged adjoint solve")
        want_G, want_sum = xref.source_gradient(N, "linear", 1.0, None, lam, U)
        assert_bits(gS, want_G, "gS of an unconverged adjoint solve")
        same_sum(info["gshift"], want_sum, "gshift of an unconverged adjoint solve")
        s.set_reaction(None)
        lam, gA, gU, gW, info = s.newton_adjoint(Ubar, U, F, kind="cubic", kappa=KAPPA, weight=w)
        assert info["status"] == mg.MG_SOLVE_NOT_CONVERGED and info["cycles"] == 1 and not s.has_reaction
        want_G, want_sum = xref.source_gradient(N, "cubic", KAPPA, w, lam, U)
        assert_bits(gW, want_G, "gW of an unconverged adjoint solve")
        same_sum(info["gkappa"], want_sum, "gkappa of an unconverged adjoint solve")
        assert_bits(gA, aref.coefficient_gradient(N, L, lam, U), "gA of an unconverged semilinear adjoint solve")
    finally:
        s.close()


def test_refusals_leave_things_as_they_were(mg):
    import ctypes as C
    N, L = 65, 1.0
    lam_h, U_h, w_h = kernel_fields(N, 77)
    rng = np.random.default_rng(78)
    ub_h, F_h = rng.standard_normal((N, N)), 40.0 * rng.standard_normal((N, N))
    nan_U = U_h.copy()
    nan_U[N // 2, N // 2] = np.nan
    lam, U, w, ub, F, Un = (mg.DeviceGrid.from_host(x) for x in (lam_h, U_h, w_h, ub_h, F_h, nan_U))
    outs = [poisoned(mg, N) for _ in range(4)]
    arrays = [(lam, lam_h), (U, U_h), (w, w_h), (ub, ub_h), (F, F_h), (Un, nan_U)] + [(o, poison_host(N)) for o in outs]
    null = types.SimpleNamespace(ptr=None, shape=(N, N))
    off = lambda g: types.SimpleNamespace(ptr=g.ptr + 8, shape=(N, N))
    react_h = rref.field("smooth", N)
    s, with_rx, fresh = mg.Solver(N, L), mg.Solver(N, L, reaction=react_h), mg.Solver(N, L, reaction=react_h)
    neumann = mg.Solver(N, L, bc="ndnd", shift=1.0)
    fmg = mg.Solver(N, L, fmg=1)
    b = mg.BatchSolver(N, L, max_batch=2)
    lib = mg.lib()
    p = lambda g: g.ptr
    res, one_d = mg.SolveResult(), C.c_double(0.0)

    def raw(fn, *args):
        def call():
            if getattr(lib, fn)(*args) > 0:
                mg._check()
        return call

    rx = lambda sv, *args: raw("mg_solver_adjoint_reaction", sv._s, *args, C.byref(res))
    nw = lambda sv, *args: raw("mg_solver_newton_adjoint", sv._s, *args, C.byref(res))
    refused2 = [
        ("kernel: NULL lam", lambda: mg.sourceGradient(N, "sinh", 1.0, None, null, U, outs[0])),
        ("kernel: misaligned w", lambda: mg.sourceGradient(N, "sinh", 1.0, off(w), lam, U, outs[0])),
        ("kernel: G is U", lambda: mg.sourceGradient(N, "sinh", 1.0, None, lam, U, U)),
        ("kernel: G overlaps lam", lambda: mg.sourceGradient(N, "sinh", 1.0, None, lam, U, types.SimpleNamespace(ptr=lam.ptr + 16, shape=(N, N)))),
        ("kernel: unknown kind", lambda: mg.sourceGradient(N, 4, 1.0, None, lam, U, outs[0])),
        ("kernel: kappa not finite", lambda: mg.sourceGradient(N, "sinh", float("inf"), None, lam, U, outs[0])),
        ("kernel: N = 2", lambda: mg.sourceGradient(2, "sinh", 1.0, None, *(types.SimpleNamespace(ptr=g.ptr, shape=(2, 2)) for g in (lam, U, outs[0])))),
        ("batch kernel: outputs overlap", lambda: mg.sourceGradient_batch(N, "sinh", 1.0, None, [lam, lam], [U, U], [outs[0], outs[0]])),
        ("batch kernel: two w for three", lambda: mg.sourceGradient_batch(N, "sinh", 1.0, [w, w], [lam] * 3, [U] * 3, outs[:3])),
        ("reaction: NULL Ubar", rx(s, None, p(U), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), None)),
        ("reaction: gS without U", rx(s, p(ub), None, p(outs[0]), None, p(outs[2]), p(outs[3]), None)),
        ("reaction: gshift without gS", rx(s, p(ub), p(U), p(outs[0]), p(outs[1]), p(outs[2]), None, C.byref(one_d))),
        ("reaction: misaligned", rx(s, p(ub), p(U), p(outs[0]) + 8, p(outs[1]), p(outs[2]), p(outs[3]), None)),
        ("reaction: gS is gA", rx(s, p(ub), p(U), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[1]), None)),
        ("reaction: lam is Ubar", rx(s, p(ub), p(U), p(ub), p(outs[1]), p(outs[2]), p(outs[3]), None)),
        ("newton: NULL F", nw(s, 1, 1.0, None, None, p(U), p(ub), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), None, None)),
        ("newton: gkappa without gW", nw(s, 1, 1.0, None, p(F), p(U), p(ub), p(outs[0]), p(outs[1]), p(outs[2]), None, C.byref(one_d), None)),
        ("newton: misaligned w", nw(s, 1, 1.0, p(w) + 8, p(F), p(U), p(ub), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), None, None)),
        ("newton: gW is F", nw(s, 1, 1.0, None, p(F), p(U), p(ub), p(outs[0]), p(outs[1]), p(outs[2]), p(F), None, None)),
        ("newton: unknown kind", nw(s, 3, 1.0, None, p(F), p(U), p(ub), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), None, None)),
        ("newton: kappa < 0", nw(s, 1, -1.0, None, p(F), p(U), p(ub), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), None, None)),
        ("newton: NaN in U", lambda: s.newton_adjoint(ub, Un, F, kind="sinh")),
        ("batch reaction: n > max_batch", lambda: b.adjoint_reaction([ub] * 3, [U] * 3)),
        ("batch newton: kappa count", lambda: b.newton_adjoint_batch([ub, ub], [U, U], [F, F], kappa=[1.0, 2.0, 3.0])),
        ("batch newton: NaN in U", lambda: b.newton_adjoint_batch([ub, ub], [U, Un], [F, F])),
    ]
    refused3 = [
        ("newton: a reaction is set", lambda: with_rx.newton_adjoint(ub, U, F)),
        ("newton: a Neumann side", lambda: neumann.newton_adjoint(ub, U, F)),
        ("newton: fmg", lambda: fmg.newton_adjoint(ub, U, F)),
        ("reaction: a Neumann side", lambda: neumann.adjoint_reaction(ub, U)),
        ("adjoint with a reaction keeps refusing", lambda: with_rx.adjoint(ub, U)),
    ]
    try:
        for code, cases in ((2, refused2), (3, refused3)):
            for what, call in cases:
                with pytest.raises(mg.MGError, match=r"\[%d\]" % code):
                    call()
                    pytest.fail(what + " was not refused")
                for g, was in arrays:
                    assert_bits(g.to_host(), was, what + ": an array was touched")
                assert with_rx.has_reaction and not s.has_reaction and not b.has_reaction, what
        # the next valid calls give the bits of fresh solvers
        got, want = with_rx.adjoint_reaction(ub_h, U_h), fresh.adjoint_reaction(ub_h, U_h)
        for x, y, nm in zip(got[:4], want[:4], ("lam", "gA", "gU", "gS")):
            assert_bits(x, y, "after the refusals: " + nm)
        same_info(got[4], want[4], "after the refusals")
    finally:
        for x in (s, with_rx, fresh, neumann, fmg, b):
            x.close()


# ---------------------------------------------------------------- 7. torch.autograd, in a process that imports torch first
def test_torch_autograd():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_adjoint_rx_torch_worker.py")], capture_output=True, text=True, timeout=600)
    sys.stdout.write(out.stdout[-3000:])
    assert out.returncode == 0 and "ADJOINT_RX_TORCH OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
