"""Adjoint sensitivities (include/mg_adjoint.h) on the device: the two point kernels and their batched twins bit for bit
against the restatement (tests/_adjoint_ref.py) over every form they have and inside guard bands; the drivers against the
caller's own sequence of public calls, bit for bit; the gradients against the dense direct solution within an a-priori bound;
the batched driver against the single one; the refusals; torch.autograd in a child process.

Measured (error / a-priori bound of the truth test, the largest over its cases): see test_truth's docstring."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import _adjoint_ref as aref
import _guard
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAN_BITS = np.uint64(0xFFFFFFFFFFFFFFFF)
KERNEL_SIZES = [3, 4, 5, 33, 64, 65, 130, 512, 513, 514]   # column form, pair form (even N >= 512), odd N above the threshold
INFO_KEYS = ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm", "history")


def poison_host(N):
    return np.full((N, N), NAN_BITS, dtype=np.uint64).view(np.float64)


def poisoned(mg, N):
    """an output no element of which a call may leave unwritten"""
    return mg.DeviceGrid.from_host(poison_host(N))


def kernel_fields(N, seed):
    """lam with a non-zero random rim (finite: the substitution must make it irrelevant), U, Ubar, a"""
    rng = np.random.default_rng(seed)
    lam, U, Ubar = rng.standard_normal((N, N)), rng.standard_normal((N, N)), rng.standard_normal((N, N))
    lam[0, :] += 3.0
    lam[-1, :] -= 5.0
    lam[:, 0] += 7.0
    lam[:, -1] -= 2.0
    return lam, U, Ubar, vref.field("random", N, seed=seed)


def check_point_kernels(mg, N, L=1.3):
    lam, U, Ubar, a = kernel_fields(N, 10 + N)
    ld, Ud, ubd, ad = (mg.DeviceGrid.from_host(x) for x in (lam, U, Ubar, a))
    out = poisoned(mg, N)
    assert_bits(mg.coefficientGradient(N, L, ld, Ud, out).to_host(), aref.coefficient_gradient(N, L, lam, U), f"gA N={N}")
    # the rim of lam is substituted, never read into a result
    clean = mg.DeviceGrid.from_host(aref.zero_rim(lam))
    assert_bits(mg.coefficientGradient(N, L, clean, Ud).to_host(), out.to_host(), f"gA N={N}: rim of lam")
    for a_dev, a_host in ((ad, a), (None, None)):
        for ub_dev, ub_host in ((ubd, Ubar), (None, None)):
            out = poisoned(mg, N)
            got = mg.boundaryGradient(N, L, a_dev, ld, ub_dev, out).to_host()
            assert_bits(got, aref.boundary_gradient(N, L, a_host, lam, ub_host),
                        f"gU N={N} a={'random' if a_host is not None else 'NULL'} Ubar={'given' if ub_host is not None else 'NULL'}")


# ---------------------------------------------------------------- 1. the kernels against the restatement
@pytest.mark.parametrize("N", KERNEL_SIZES)
def test_point_kernels_bit_identical_to_restatement(mg, N):
    check_point_kernels(mg, N)


@pytest.mark.parametrize("N", [33, 512])
def test_batched_twins_equal_the_single_launches(mg, N):
    """B = 3 distinct instances in one launch each; one a entry and one Ubar entry NULL"""
    L, B = 1.3, 3
    sets = [kernel_fields(N, 50 + 7 * i + N) for i in range(B)]
    lam = [mg.DeviceGrid.from_host(s[0]) for s in sets]
    U = [mg.DeviceGrid.from_host(s[1]) for s in sets]
    Ubar = [mg.DeviceGrid.from_host(sets[0][2]), mg.DeviceGrid.from_host(sets[1][2]), None]
    a = [mg.DeviceGrid.from_host(sets[0][3]), None, mg.DeviceGrid.from_host(sets[2][3])]
    gA = mg.coefficientGradient_batch(N, L, lam, U, [poisoned(mg, N) for _ in range(B)])
    gU = mg.boundaryGradient_batch(N, L, a, lam, Ubar, [poisoned(mg, N) for _ in range(B)])
    for i in range(B):
        assert_bits(gA[i].to_host(), mg.coefficientGradient(N, L, lam[i], U[i]).to_host(), f"gA N={N} instance {i}")
        assert_bits(gU[i].to_host(), mg.boundaryGradient(N, L, a[i], lam[i], Ubar[i]).to_host(), f"gU N={N} instance {i}")
        assert_bits(gA[i].to_host(), aref.coefficient_gradient(N, L, sets[i][0], sets[i][1]), f"gA N={N} instance {i}: numpy")
    # a and Ubar absent altogether
    gU = mg.boundaryGradient_batch(N, L, None, lam, None, [poisoned(mg, N) for _ in range(B)])
    for i in range(B):
        assert_bits(gU[i].to_host(), aref.boundary_gradient(N, L, None, sets[i][0], None), f"gU N={N} instance {i}: no a, no Ubar")


# ---------------------------------------------------------------- 2. guard bands
@pytest.mark.parametrize("place", list(_guard.PLACEMENTS))
@pytest.mark.parametrize("N", [65, 512])
def test_kernels_inside_guard_bands(mg, N, place):
    """outputs are written inside their arrays only (every element of them), inputs are unchanged"""
    L = 1.0
    lam, U, Ubar, a = kernel_fields(N, 90 + N)
    with _guard.block(mg, [N] * 6, place) as b:
        lv, Uv, ubv, av, gAv, gUv = b.views
        for v, x in ((lv, lam), (Uv, U), (ubv, Ubar), (av, a)):
            v.upload(x)
        gAv.poison()
        gUv.poison()
        b.expect_readonly(lv, Uv, ubv, av, gUv)
        mg.coefficientGradient(N, L, lv, Uv, gAv)
        assert_bits(gAv.to_host(), aref.coefficient_gradient(N, L, lam, U), f"gA N={N} {place}")
        b.check(f"mg_coefficientGradient N={N} {place}")
        b.expect_readonly(lv, Uv, ubv, av, gAv)
        mg.boundaryGradient(N, L, av, lv, ubv, gUv)
        assert_bits(gUv.to_host(), aref.boundary_gradient(N, L, a, lam, Ubar), f"gU N={N} {place}")
        b.check(f"mg_boundaryGradient N={N} {place}")
        # the batched twins on the same block: two instances sharing the inputs, the second one's outputs in DeviceGrids
        gAv.poison()
        gUv.poison()
        extra = [poisoned(mg, N), poisoned(mg, N)]
        b.expect_readonly(lv, Uv, ubv, av)
        mg.coefficientGradient_batch(N, L, [lv, lv], [Uv, Uv], [gAv, extra[0]])
        mg.boundaryGradient_batch(N, L, [av, None], [lv, lv], [ubv, ubv], [gUv, extra[1]])
        assert_bits(gAv.to_host(), aref.coefficient_gradient(N, L, lam, U), f"batched gA N={N} {place}")
        assert_bits(gUv.to_host(), aref.boundary_gradient(N, L, a, lam, Ubar), f"batched gU N={N} {place}")
        assert_bits(extra[1].to_host(), aref.boundary_gradient(N, L, None, lam, Ubar), f"batched gU N={N} {place}: a NULL")
        b.check(f"batched twins N={N} {place}")


# ---------------------------------------------------------------- 3. the driver is the caller's sequence of public calls
def driver_problem(N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, N)), rng.standard_normal((N, N))   # Ubar, U


CONFIGS = {
    "fused": dict(),
    "coef_smooth": dict(coef="smooth"),
    "coef_smooth_shift": dict(coef="smooth", shift=1e2),
    "krylov_jump": dict(coef="jump", krylov=4),
    "fmg": dict(fmg=1),
}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("N", [65, 64])
def test_driver_equals_the_public_calls(mg, N, config):
    """mg_solver_adjoint against {mg_fill_zero, mg_solver_solve, mg_coefficientGradient, mg_boundaryGradient}: lam, gA, gU,
    history, cycles and flags bit for bit; Ubar == 0 gives zeros and 0 cycles; gA = gU = NULL is just the solve"""
    L = 1.0
    opts = dict(CONFIGS[config])
    name = opts.pop("coef", None)
    a = vref.field(name, N, seed=N) if name else None
    Ubar, U = driver_problem(N, 300 + N)
    ubd, Ud = mg.DeviceGrid.from_host(Ubar), mg.DeviceGrid.from_host(U)
    ad = mg.DeviceGrid.from_host(a) if a is not None else None
    s = mg.Solver(N, L, coef=a, **opts)
    try:
        # the caller's own sequence
        lam2 = poisoned(mg, N)
        mg.lib().mg_fill_zero(lam2.ptr, N * N)
        want_info = s.solve_ptr(ubd.ptr, lam2.ptr)
        gA2 = mg.coefficientGradient(N, L, lam2, Ud)
        gU2 = mg.boundaryGradient(N, L, ad, lam2, ubd)
        # the driver
        lam, gA, gU = poisoned(mg, N), poisoned(mg, N), poisoned(mg, N)
        info = s.adjoint_ptr(ubd.ptr, Ud.ptr, lam.ptr, gA.ptr, gU.ptr)
        what = f"N={N} {config}"
        assert info["cycles"] > 0 and info["converged"], what
        for key in INFO_KEYS:
            assert info[key] == want_info[key], (what, key)
        if "breakdown" in want_info:
            assert info["breakdown"] == want_info["breakdown"]
        assert_bits(lam.to_host(), lam2.to_host(), what + ": lam")
        assert_bits(gA.to_host(), gA2.to_host(), what + ": gA")
        assert_bits(gU.to_host(), gU2.to_host(), what + ": gU")
        # and both are the restatement applied to the device's lam
        assert_bits(gA.to_host(), aref.coefficient_gradient(N, L, lam.to_host(), U), what + ": gA against numpy")
        assert_bits(gU.to_host(), aref.boundary_gradient(N, L, a, lam.to_host(), Ubar), what + ": gU against numpy")
        # gA = gU = NULL: just the solve
        lam3 = poisoned(mg, N)
        info3 = s.adjoint_ptr(ubd.ptr, None, lam3.ptr, None, None)
        assert_bits(lam3.to_host(), lam2.to_host(), what + ": lam alone")
        assert [info3[k] for k in INFO_KEYS] == [want_info[k] for k in INFO_KEYS]
        # Ubar == 0: 0 cycles, zeros
        zero = mg.DeviceGrid.zeros((N, N))
        lam, gA, gU = poisoned(mg, N), poisoned(mg, N), poisoned(mg, N)
        info = s.adjoint_ptr(zero.ptr, Ud.ptr, lam.ptr, gA.ptr, gU.ptr)
        assert info["cycles"] == 0 and info["converged"], what
        for g in (lam, gA, gU):
            assert not np.any(g.to_host()), what + ": Ubar == 0"
        # the numpy / DeviceGrid front end is the same call
        lam_h, gA_h, gU_h, info_h = s.adjoint(Ubar, U)
        assert_bits(lam_h, lam2.to_host(), what + ": Solver.adjoint lam")
        assert_bits(gA_h, gA2.to_host(), what + ": Solver.adjoint gA")
        assert_bits(gU_h, gU2.to_host(), what + ": Solver.adjoint gU")
        lam_h, gA_h, gU_h, _ = s.adjoint(Ubar, U, want_coef=False, want_rim=False)
        assert gA_h is None and gU_h is None
    finally:
        s.close()


def test_not_converged_still_writes_the_gradients(mg):
    N, L = 65, 1.0
    Ubar, U = driver_problem(N, 7)
    s = mg.Solver(N, L, max_cycles=2)
    try:
        lam, gA, gU, info = s.adjoint(Ubar, U)
    finally:
        s.close()
    assert info["status"] == mg.MG_SOLVE_NOT_CONVERGED and info["cycles"] == 2 and not info["converged"]
    assert_bits(gA, aref.coefficient_gradient(N, L, lam, U), "gA of an unconverged adjoint solve")
    assert_bits(gU, aref.boundary_gradient(N, L, None, lam, Ubar), "gU of an unconverged adjoint solve")


# ---------------------------------------------------------------- 4. truth
TRUTH_RATIOS = {}


@pytest.mark.parametrize("shift", [0.0, 1e2])
@pytest.mark.parametrize("name", ["smooth", "exp"])
@pytest.mark.parametrize("N", [17, 33])
def test_truth(mg, N, name, shift):
    """gA and gU of the device (forward solve and adjoint solve at rtol 1e-10) against the restatement applied to the dense
    direct solutions U*, lam*, inside an a-priori bound (tests/_adjoint_ref.py: gA_bound, gU_bound):
      mu = a_min*lambda_1(-Laplace_h) + sigma bounds the operator away from 0, so a field whose residual norm is r lies
      within e = (r + rounding of the residual evaluation)/mu of the solution, in l2 and hence at every point;
      |dgA_k| <= 0.5*inv*4*(2 e_lam max|dU*| + 2 e_U max|dlam*| + 4 e_lam e_U) + rounding;  |dgU_b| <= inv*a_max*e_lam + rounding.
    Measured on the MI355X, the largest error/bound over the eight cases: gA 1.1e-3, gU 4.7e-2."""
    L = 1.0
    rng = np.random.default_rng(1000 + N)
    a = vref.field(name, N, L)
    F, U0, W = 40.0 * rng.standard_normal((N, N)), rng.standard_normal((N, N)), rng.standard_normal((N, N))
    s = mg.Solver(N, L, coef=a, shift=shift, rtol=1e-10)
    try:
        U, fi = s.solve(F, U0)
        lam, gA, gU, ai = s.adjoint(W, U)
    finally:
        s.close()
    assert fi["converged"] and ai["converged"]
    U_ref, lam_ref, _, gA_ref, gU_ref = aref.gradients(a, F, U0, W, L, shift)
    mu = aref.mu(a, N, L, shift)
    u53 = float(vref.U53)
    e_U = (fi["res"] + float(vref.residual_rounding_bound(a, U, F, L, shift))) / mu + u53 * float(np.max(np.abs(U_ref)))
    e_lam = (ai["res"] + float(vref.residual_rounding_bound(a, lam, W, L, shift))) / mu + u53 * float(np.max(np.abs(lam_ref)))
    bA = aref.gA_bound(N, L, U_ref, lam_ref, e_U, e_lam)
    bU = aref.gU_bound(N, L, a, lam_ref, W, e_lam)
    rA, rU = float(np.max(np.abs(gA - gA_ref))) / bA, float(np.max(np.abs(gU - gU_ref))) / bU
    TRUTH_RATIOS[(N, name, shift)] = (rA, rU)
    print(f"N={N} a={name} shift={shift}: e_U {e_U:.2e} e_lam {e_lam:.2e}; gA error/bound {rA:.3e}, gU error/bound {rU:.3e}; "
          f"largest so far gA {max(v[0] for v in TRUTH_RATIOS.values()):.3e} gU {max(v[1] for v in TRUTH_RATIOS.values()):.3e}")
    assert rA <= 1.0 and rU <= 1.0, (rA, rU)
    # the field errors themselves obey their bounds (the premise of the two above)
    assert float(np.max(np.abs(U - U_ref))) <= e_U and float(np.max(np.abs(aref.zero_rim(lam) - lam_ref))) <= e_lam


# ---------------------------------------------------------------- 5. the batched driver
def batch_problem(N):
    """three instances with coefficients of their own: a random right-hand side on `smooth`, Ubar == 0 on `exp` (0 cycles), a
    smooth right-hand side on `jump` (on the restatement: 10 against 22 cycles, so the first leaves the batch early)"""
    x, y = vref.grid(N)
    rng = np.random.default_rng(5)
    a = [vref.field(n, N, seed=1) for n in ("smooth", "exp", "jump")]
    Ubar = [rng.standard_normal((N, N)), np.zeros((N, N)), np.sin(np.pi * x) * np.sin(np.pi * y)]
    U = [rng.standard_normal((N, N)) for _ in range(3)]
    return a, Ubar, U


def test_batched_adjoint_equals_the_single_solver(mg):
    N, L, B = 65, 1.0, 3
    a, Ubar, U = batch_problem(N)
    b = mg.BatchSolver(N, L, max_batch=B)
    try:
        b.set_coefficient(a)
        lam, gA, gU, infos = b.adjoint(np.stack(Ubar), np.stack(U))
        # the gradient stage is two launches whatever B is: against the solve of the same right-hand sides alone
        _, solve_infos = b.solve(np.stack(Ubar))
        stage3 = infos[0]["stats"]["launches"] - solve_infos[0]["stats"]["launches"]
        b.set_coefficient(a[0])
        _, _, _, one = b.adjoint(Ubar[0][None], U[0][None])
        _, solve_one = b.solve(Ubar[0][None])
        stage1 = one[0]["stats"]["launches"] - solve_one[0]["stats"]["launches"]
        assert stage1 == stage3 == 2, (stage1, stage3)
        _, _, _, none = b.adjoint(Ubar[0][None], U[0][None], want_coef=False, want_rim=False)
        assert none[0]["stats"]["launches"] == solve_one[0]["stats"]["launches"]
    finally:
        b.close()
    cycles = [i["cycles"] for i in infos]
    assert cycles[1] == 0 and 0 < cycles[0] < cycles[2], cycles
    for i in range(B):
        s = mg.Solver(N, L, coef=a[i])
        try:
            lam1, gA1, gU1, info1 = s.adjoint(Ubar[i], U[i])
        finally:
            s.close()
        for key in INFO_KEYS:
            assert infos[i][key] == info1[key], (i, key)
        assert_bits(lam[i], lam1, f"instance {i}: lam")
        assert_bits(gA[i], gA1, f"instance {i}: gA")
        assert_bits(gU[i], gU1, f"instance {i}: gU")
    assert not np.any(lam[1]) and not np.any(gA[1]) and not np.any(gU[1])


# ---------------------------------------------------------------- 6. refusals leave things as they were
def test_refusals_leave_things_as_they_were(mg):
    N, L = 65, 1.0
    lam_h, U_h, ub_h, a_h = kernel_fields(N, 77)
    lam, U, ub, a = (mg.DeviceGrid.from_host(x) for x in (lam_h, U_h, ub_h, a_h))
    outs = [poisoned(mg, N) for _ in range(3)]
    arrays = [(lam, lam_h), (U, U_h), (ub, ub_h), (a, a_h)] + [(o, poison_host(N)) for o in outs]
    null = types.SimpleNamespace(ptr=None, shape=(N, N))
    off = lambda g: types.SimpleNamespace(ptr=g.ptr + 8, shape=(N, N))
    s = mg.Solver(N, L, coef=a_h)
    b = mg.BatchSolver(N, L, max_batch=2)
    fresh = mg.Solver(N, L, coef=a_h)
    p = lambda g: g.ptr
    refused = [
        ("gA: NULL lam", lambda: mg.coefficientGradient(N, L, null, U, outs[0])),
        ("gA: NULL U", lambda: mg.coefficientGradient(N, L, lam, null, outs[0])),
        ("gA: NULL out", lambda: mg.coefficientGradient(N, L, lam, U, null)),
        ("gA: misaligned", lambda: mg.coefficientGradient(N, L, off(lam), U, outs[0])),
        ("gA: out is U", lambda: mg.coefficientGradient(N, L, lam, U, U)),
        ("gA: out overlaps lam", lambda: mg.coefficientGradient(N, L, lam, U, types.SimpleNamespace(ptr=lam.ptr + 16, shape=(N, N)))),
        ("gA: N = 2", lambda: mg.coefficientGradient(2, L, lam, U, outs[0])),
        ("gU: NULL lam", lambda: mg.boundaryGradient(N, L, a, null, ub, outs[0])),
        ("gU: NULL out", lambda: mg.boundaryGradient(N, L, a, lam, ub, null)),
        ("gU: misaligned a", lambda: mg.boundaryGradient(N, L, off(a), lam, ub, outs[0])),
        ("gU: out is Ubar", lambda: mg.boundaryGradient(N, L, a, lam, ub, ub)),
        ("gU: N = 2", lambda: mg.boundaryGradient(2, L, a, lam, ub, outs[0])),
        ("batch gA: n = 0", lambda: mg.coefficientGradient_batch(N, L, [], [], [])),
        ("batch gA: NULL entry", lambda: mg.coefficientGradient_batch(N, L, [lam, null], [U, U], outs[:2])),
        ("batch gA: outputs overlap", lambda: mg.coefficientGradient_batch(N, L, [lam, lam], [U, U], [outs[0], outs[0]])),
        ("batch gU: misaligned", lambda: mg.boundaryGradient_batch(N, L, None, [lam, lam], None, [outs[0], off(outs[1])])),
        ("batch gU: N = 2", lambda: mg.boundaryGradient_batch(2, L, None, [lam], None, [outs[0]])),
        ("driver: NULL Ubar", lambda: s.adjoint_ptr(None, p(U), p(outs[0]), p(outs[1]), p(outs[2]))),
        ("driver: NULL lam", lambda: s.adjoint_ptr(p(ub), p(U), None, p(outs[1]), p(outs[2]))),
        ("driver: gA without U", lambda: s.adjoint_ptr(p(ub), None, p(outs[0]), p(outs[1]), p(outs[2]))),
        ("driver: misaligned", lambda: s.adjoint_ptr(p(ub), p(U), p(outs[0]) + 8, p(outs[1]), p(outs[2]))),
        ("driver: lam is Ubar", lambda: s.adjoint_ptr(p(ub), p(U), p(ub), p(outs[1]), p(outs[2]))),
        ("driver: gA is gU", lambda: s.adjoint_ptr(p(ub), p(U), p(outs[0]), p(outs[1]), p(outs[1]))),
        ("batch driver: n = 0", lambda: b.adjoint_ptrs([], [], [], [], [])),
        ("batch driver: n > max_batch", lambda: b.adjoint_ptrs([p(ub)] * 3, [p(U)] * 3, [p(outs[0])] * 3, None, None)),
        ("batch driver: NULL lam", lambda: b.adjoint_ptrs([p(ub)], [p(U)], [None], [p(outs[1])], [p(outs[2])])),
        ("batch driver: lam shared", lambda: b.adjoint_ptrs([p(ub)] * 2, [p(U)] * 2, [p(outs[0])] * 2, None, None)),
        ("batch driver: gU is U", lambda: b.adjoint_ptrs([p(ub)], [p(U)], [p(outs[0])], [p(outs[1])], [p(U)])),
    ]
    try:
        for what, call in refused:
            with pytest.raises(mg.MGError, match=r"\[2\]"):
                call()
                pytest.fail(what + " was not refused")
            for g, was in arrays:
                assert_bits(g.to_host(), was, what + ": an array was touched")
        # the next valid call gives the bits of a fresh solver's
        got = s.adjoint(ub_h, U_h)
        want = fresh.adjoint(ub_h, U_h)
        for x, y, name in zip(got[:3], want[:3], ("lam", "gA", "gU")):
            assert_bits(x, y, "after the refusals: " + name)
        assert [got[3][k] for k in INFO_KEYS] == [want[3][k] for k in INFO_KEYS]
        lam_b, gA_b, gU_b, infos = b.adjoint(ub_h[None], U_h[None])
        plain = mg.Solver(N, L)
        try:
            want = plain.adjoint(ub_h, U_h)
        finally:
            plain.close()
        for x, y, name in zip((lam_b[0], gA_b[0], gU_b[0]), want[:3], ("lam", "gA", "gU")):
            assert_bits(x, y, "batch after the refusals: " + name)
    finally:
        s.close(); b.close(); fresh.close()


# ---------------------------------------------------------------- 7. torch.autograd, in a process that imports torch first
def test_torch_autograd():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_adjoint_torch_worker.py")], capture_output=True, text=True, timeout=600)
    sys.stdout.write(out.stdout[-3000:])
    assert out.returncode == 0 and "ADJOINT_TORCH OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
