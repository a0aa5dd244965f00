"""The heat stepper with a variable coefficient (include/mg_heat_vc.h) on the device: the right-hand-side kernel bit for bit
against the restatement (tests/_heat_vc_ref.py) over every form it has (one column per lane, two columns from even N = 512,
non-temporal from 4096) and inside guard bands; theta = 1 and a == 1 against the constant stepper; the stepper against its own
building blocks (heat_rhs_coef + Solver with shift = sigma and the coefficient) and against the numpy restatement; against
truth with the bounds of tests/test_heat_vc_cpu.py; the launches, the lifecycle, the refusals and torch tensors.

Bit comparison of a step means: U bit for bit and the cycles of every step equal; every case against numpy first qualifies
its input (coarse margin >= 1e-10)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import _guard
import _heat_ref as href
import _heat_vc_ref as hvref
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NU, DT = 0.5, 2e-4          # sigma = 1/(theta*1e-4)
COLS_SIZES = [3, 4, 5, 8, 17, 63, 64, 100, 257, 511]
PAIR_SIZES = [512, 514, 1026]
NAN_BITS = np.uint64(0xFFFFFFFFFFFFFFFF)


def poisoned(mg, N):
    """an F no element of which the kernel may leave unwritten"""
    return mg.DeviceGrid.from_host(np.full((N, N), NAN_BITS, dtype=np.uint64).view(np.float64))


def fields(N, seed):
    Q, U = ref.random_problem(N, seed)
    return U, 40.0 * Q


def lib_table(mg):
    return lambda N, M: mg.restriction_table(N, M)


def stepper(mg, N, L, theta, a=None, **opts):
    hs = mg.HeatStepper(N, L, NU, DT, theta, **opts)
    if a is not None:
        hs.set_coefficient(a)
    return hs


# ---------------------------------------------------------------- 1. the kernel
def _kernel_cases(mg, N, place, cases):
    """every (field name, theta, with Q, L) of `cases` on one guarded block [a, U, Q, F]: bits against the restatement, inputs
    and guard bands unchanged"""
    U, Q = fields(N, 100 + N)
    with _guard.block(mg, [N] * 4, place) as b:
        av, Uv, Qv, Fv = b.views
        Uv.upload(U)
        Qv.upload(Q)
        name_up = None
        for name, theta, with_q, L in cases:
            if name != name_up:
                a = vref.field(name, N, seed=N)
                av.upload(a)
                name_up = name
            Fv.poison()
            b.expect_readonly(av, Uv, Qv)
            mg.heat_rhs_coef(N, L, NU, DT, theta, av, Uv, Qv if with_q else None, Fv)
            what = f"N={N} {place} a={name} theta={theta} L={L} Q={'yes' if with_q else 'no'}"
            assert_bits(Fv.to_host(), hvref.rhs(N, L, NU, DT, theta, a, U, Q if with_q else None), what)
            b.check("mg_heat_rhs_coef " + what)


@pytest.mark.parametrize("place", list(_guard.PLACEMENTS))
@pytest.mark.parametrize("N", COLS_SIZES + PAIR_SIZES)
def test_kernel_bit_identical_to_restatement_inside_guard_bands(mg, N, place):
    """one column per lane (odd or small N) and two columns per lane (even N >= 512)"""
    _kernel_cases(mg, N, place, [(name, theta, with_q, L) for name in ("exp", "random") for theta in (0.75, 0.5)
                                 for with_q in (True, False) for L in (1.0, 2.5)])


@pytest.mark.parametrize("N,place", [(4096, "page"), (4098, "odd16")])
def test_kernel_non_temporal_form(mg, N, place):
    """even N >= 4096: non-temporal loads of Q and stores of F"""
    _kernel_cases(mg, N, place, [("exp", 0.5, True, 1.0)])


# ---------------------------------------------------------------- 2. theta = 1 reads no coefficient; corners never count
@pytest.mark.parametrize("N", [17, 64, 512, 514])
def test_theta_one_and_the_corners_of_a(mg, N):
    U, Q = fields(N, 200 + N)
    a = vref.field("exp", N)
    Ud, Qd, Fd = mg.DeviceGrid.from_host(U), mg.DeviceGrid.from_host(Q), poisoned(mg, N)
    nan = Fd.to_host()
    ad, nand = mg.DeviceGrid.from_host(a), mg.DeviceGrid.from_host(np.full((N, N), np.nan))
    for qd in (Qd, None):
        want = mg.heat_rhs(N, 2.5, NU, DT, 1.0, Ud, qd).to_host()
        for coef in (ad, nand):
            mg.lib().mg_upload(Fd.ptr, nan.ctypes.data, nan.size)
            assert_bits(mg.heat_rhs_coef(N, 2.5, NU, DT, 1.0, coef, Ud, qd, Fd).to_host(), want, f"N={N} theta=1")
    corners = a.copy()
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = np.nan
    cd = mg.DeviceGrid.from_host(corners)
    for theta in (0.75, 0.5):
        want = mg.heat_rhs_coef(N, 1.0, NU, DT, theta, ad, Ud, Qd).to_host()
        assert_bits(want, hvref.rhs(N, 1.0, NU, DT, theta, a, U, Q), f"N={N} theta={theta}")
        mg.lib().mg_upload(Fd.ptr, nan.ctypes.data, nan.size)
        assert_bits(mg.heat_rhs_coef(N, 1.0, NU, DT, theta, cd, Ud, Qd, Fd).to_host(), want, f"N={N} theta={theta}: NaN corners of a")


# ---------------------------------------------------------------- 3. a == 1 is the constant stepper
@pytest.mark.parametrize("N", [64, 257, 512])
def test_unit_coefficient_right_hand_side(mg, N):
    U, Q = fields(N, 300 + N)
    Ud, Qd, one = mg.DeviceGrid.from_host(U), mg.DeviceGrid.from_host(Q), mg.DeviceGrid.from_host(np.ones((N, N)))
    for theta in (1.0, 0.75, 0.5):
        for qd in (Qd, None):
            want = mg.heat_rhs(N, 2.5, NU, DT, theta, Ud, qd).to_host()
            assert_bits(mg.heat_rhs_coef(N, 2.5, NU, DT, theta, one, Ud, qd).to_host(), want, f"N={N} theta={theta} a == 1")
            assert_bits(mg.heat_rhs_coef(N, 2.5, NU, DT, theta, None, Ud, qd).to_host(), want, f"N={N} theta={theta} a = None")


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("N", [64, 257])
def test_unit_coefficient_is_the_constant_stepper(mg, N, theta):
    U, Q = fields(N, 400 + N)
    plain = stepper(mg, N, 1.0, theta, rtol=1e-8)
    unit = stepper(mg, N, 1.0, theta, np.ones((N, N)), rtol=1e-8)
    try:
        assert unit.has_coefficient and not plain.has_coefficient
        want, wi = plain.step(U, Q, steps=3)
        got, gi = unit.step(U, Q, steps=3)
    finally:
        plain.close(); unit.close()
    assert_bits(got, want, f"N={N} theta={theta}: a == 1 against no coefficient")
    assert sum(wi[0]["cycles_per_step"]) > 0
    for key in ("status", "converged", "steps", "cycles", "cycles_per_step", "coarse_capped", "res", "ref_norm"):
        assert gi[0][key] == wi[0][key], key


# ---------------------------------------------------------------- 4. the stepper is its building blocks
@pytest.mark.parametrize("theta", [1.0, 0.75, 0.5])
@pytest.mark.parametrize("N", [33, 100, 256])
def test_stepper_equals_its_building_blocks(mg, N, theta):
    U, Q = fields(N, 500 + N)
    a = vref.field("exp", N)
    opts = dict(rtol=1e-8)
    ad = mg.DeviceGrid.from_host(a)
    hs = stepper(mg, N, 1.0, theta, ad, **opts)
    sv = mg.Solver(N, 1.0, shift=hs.sigma, coef=ad, **opts)
    try:
        assert hs.sigma == href.consts(N, 1.0, NU, DT, theta)[0]
        Ua, Ub, Qd, Fd = mg.DeviceGrid.from_host(U), mg.DeviceGrid.from_host(U), mg.DeviceGrid.from_host(Q), poisoned(mg, N)
        _, infos = hs.step(Ua, Qd, steps=3)
        cycles = []
        for _ in range(3):
            mg.heat_rhs_coef(N, 1.0, NU, DT, theta, ad, Ub, Qd, Fd)
            _, info = sv.solve(Fd, Ub)
            cycles.append(info["cycles"])
        assert_bits(Ua.to_host(), Ub.to_host(), f"N={N} theta={theta}: stepper vs heat_rhs_coef + Solver")
        assert infos[0]["cycles_per_step"] == cycles and infos[0]["steps"] == 3 and infos[0]["cycles"] == sum(cycles)
        assert infos[0]["status"] == 0 and infos[0]["res"] == info["res"] and infos[0]["ref_norm"] == info["ref_norm"]
        assert sum(cycles) > 0
        assert_bits(Qd.to_host(), Q, "Q")
        # ... and the coefficient does something: the constant stepper ends elsewhere
        plain = stepper(mg, N, 1.0, theta, **opts)
        other, _ = plain.step(U, Q, steps=3)
        plain.close()
        assert not np.array_equal(other, Ua.to_host())
    finally:
        hs.close(); sv.close()


# ---------------------------------------------------------------- 5. the stepper against the restatement
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_stepper_bit_identical_to_restatement(mg, oracle, theta):
    N, L = 65, 2.5
    U, Q = fields(N, 600 + N)
    a = vref.field("exp", N, L)
    margins = []
    want, cycles, conv = hvref.run(oracle, a, U, Q, steps=2, L=L, nu=NU, dt=DT, theta=theta, rtol=1e-8, margins=margins,
                                   table=lib_table(mg))
    ref.assert_qualified(margins, f"N={N} theta={theta}")
    hs = stepper(mg, N, L, theta, a, rtol=1e-8)
    try:
        got, infos = hs.step(U, Q, steps=2)
    finally:
        hs.close()
    assert_bits(got, want, f"N={N} theta={theta}")
    assert conv and infos[0]["converged"] and infos[0]["cycles_per_step"] == cycles and sum(cycles) > 0


# ---------------------------------------------------------------- 6. truth, with the bounds of tests/test_heat_vc_cpu.py
@pytest.mark.parametrize("nu,dt", [(0.3, 1e-2), (1.0, 1e-4)])
@pytest.mark.parametrize("theta", [1.0, 0.75, 0.5])
@pytest.mark.parametrize("name", ["exp", "smooth"])
def test_one_step_against_the_direct_solution(mg, name, theta, nu, dt):
    N, rtol = 33, hvref.ONE_STEP_RTOL
    a, U0, Q = hvref.one_step_problem(N, name, 5 + N)
    ad, Ud, Qd = mg.DeviceGrid.from_host(a), mg.DeviceGrid.from_host(U0), mg.DeviceGrid.from_host(Q)
    F = mg.heat_rhs_coef(N, 1.0, nu, dt, theta, ad, Ud, Qd).to_host()
    hs = mg.HeatStepper(N, 1.0, nu, dt, theta, rtol=rtol, max_cycles=80)
    try:
        hs.set_coefficient(ad)
        _, infos = hs.step(Ud, Qd, steps=1)
    finally:
        hs.close()
    assert infos[0]["converged"]
    hvref.check_one_step(a, U0, Q, Ud.to_host(), F, 1.0, nu, dt, theta, rtol,
                         f"N={N} a={name} theta={theta} nu={nu} dt={dt}, {infos[0]['cycles']} cycles")


def test_perturbed_steady_state_decays(mg):
    N = 65
    p, s = hvref.Steady(N), hvref.STEADY
    ad, Ud, Qd = mg.DeviceGrid.from_host(p.a), mg.DeviceGrid.from_host(p.U0), mg.DeviceGrid.from_host(p.Q)
    hs = mg.HeatStepper(N, p.L, p.nu, p.dt, p.theta, rtol=s["rtol"])
    Us, Fs = [p.U0], []
    try:
        hs.set_coefficient(ad)
        assert hs.sigma == p.sigma
        for _ in range(s["steps"]):
            Fs.append(mg.heat_rhs_coef(N, p.L, p.nu, p.dt, p.theta, ad, Ud, Qd).to_host())
            _, infos = hs.step(Ud, Qd, steps=1)
            assert infos[0]["converged"]
            Us.append(Ud.to_host())
    finally:
        hs.close()
    hvref.check_steady(p, Us, Fs, s["rtol"], f"N={N}")


# ---------------------------------------------------------------- 7. the launches
@pytest.mark.parametrize("theta,name", [(0.5, "heat_rhs_vc"), (1.0, "heat_rhs")])
def test_one_right_hand_side_launch_per_step(mg, theta, name):
    """with a coefficient and theta != 1 every step launches the variable kernel and nothing of the constant one; with theta = 1
    the launch is the constant stepper's"""
    N, steps = 64, 3
    U, Q = fields(N, 700)
    hs = stepper(mg, N, 1.0, theta, vref.field("exp", N), rtol=1e-8)
    try:
        mg.profile_begin(0)
        hs.step(U, Q, steps=steps)
        counts = {}
        for e in mg.profile_end():
            if e["name"].startswith("heat_rhs"):
                counts[e["name"]] = counts.get(e["name"], 0) + e["launches"]
    finally:
        hs.close()
    assert counts == {name: steps}


# ---------------------------------------------------------------- 8. lifecycle and refusals
def test_set_replace_and_remove(mg):
    N, theta = 100, 0.5
    U, Q = fields(N, 800)
    a1, a2 = vref.field("smooth", N), vref.field("exp", N)
    opts = dict(rtol=1e-8)
    plain = stepper(mg, N, 1.0, theta, **opts)
    want_plain, info_plain = plain.step(U, Q, steps=2)
    plain.close()
    hs = stepper(mg, N, 1.0, theta, **opts)
    try:
        assert not hs.has_coefficient
        g = mg.DeviceGrid.from_host(a1)
        hs.set_coefficient(g)
        g.free()                                   # the caller's array may be freed after the call
        junk = mg.DeviceGrid.from_host(np.full((N, N), -7.0))   # (likely the same block, recycled)
        got1, _ = hs.step(U, Q, steps=2)
        junk.free()
        hs.set_coefficient(a2)
        got2, info2 = hs.step(U, Q, steps=2)
        for a, got in ((a1, got1), (a2, got2)):
            fresh = stepper(mg, N, 1.0, theta, a, **opts)
            want, info = fresh.step(U, Q, steps=2)
            fresh.close()
            assert_bits(got, want, "a replaced coefficient steps as a fresh stepper's")
        assert info2[0]["cycles_per_step"] == info[0]["cycles_per_step"]
        assert not np.array_equal(got1, got2) and not np.array_equal(got2, want_plain)
        hs.set_coefficient(None)
        assert not hs.has_coefficient
        back, info_back = hs.step(U, Q, steps=2)
        assert_bits(back, want_plain, "set_coefficient(None) restores the constant stepper")
        assert info_back[0]["cycles_per_step"] == info_plain[0]["cycles_per_step"]
    finally:
        hs.close()


def test_refused_coefficients_leave_the_stepper_as_it_was(mg):
    N, theta = 64, 0.5
    U, Q = fields(N, 900)
    a = vref.field("smooth", N)
    big = mg.DeviceGrid.from_host(np.ones((N + 1, N)))
    for start in (None, a):
        hs = stepper(mg, N, 1.0, theta, start, rtol=1e-8)
        try:
            before, _ = hs.step(U, Q, steps=2)
            for value in (float("nan"), 0.0, -1.0, float("inf")):
                bad = a.copy()
                bad[N - 1, 3] = value              # (a rim point: the rim is part of the coefficient)
                with pytest.raises(mg.MGError, match=r"\[2\]"):
                    hs.set_coefficient(bad)
                assert hs.has_coefficient == (start is not None)
                assert_bits(hs.step(U, Q, steps=2)[0], before, f"a step after the refused value {value}")
            for shape in (np.ones((N, N + 1)), np.ones((N - 1, N - 1)), mg.DeviceGrid(32)):
                with pytest.raises(mg.MGError, match="shape"):
                    hs.set_coefficient(shape)
            with pytest.raises(mg.MGError, match=r"\[2\].*aligned"):
                hs.set_coefficient(types.SimpleNamespace(ptr=big.ptr + 8, shape=(N, N)))
            assert hs.has_coefficient == (start is not None)
            assert_bits(hs.step(U, Q, steps=2)[0], before, "a step after the refused shapes and the misaligned array")
        finally:
            hs.close()


def test_fmg_batch_and_null_are_refused(mg):
    N, theta = 64, 0.5
    U, Q = fields(N, 1000)
    U2, Q2 = fields(N, 1001)
    a = vref.field("smooth", N)
    hs = stepper(mg, N, 1.0, theta, rtol=1e-8, fmg=1)
    try:
        before, _ = hs.step(U, Q, steps=2)
        with pytest.raises(mg.MGError, match=r"\[3\].*fmg"):
            hs.set_coefficient(a)
        assert not hs.has_coefficient
        assert_bits(hs.step(U, Q, steps=2)[0], before, "the fmg stepper steps after the refusal")
    finally:
        hs.close()
    hs = stepper(mg, N, 1.0, theta, rtol=1e-8, max_batch=2)
    try:
        before, bi = hs.step(np.stack([U, U2]), np.stack([Q, Q2]), steps=2)
        with pytest.raises(mg.MGError, match=r"\[3\].*max_batch"):
            hs.set_coefficient(a)
        assert not hs.has_coefficient
        hs.set_coefficient(None)                   # (nothing to take away: accepted)
        after, ai = hs.step(np.stack([U, U2]), np.stack([Q, Q2]), steps=2)
        assert_bits(after, before, "the batched stepper steps both instances after the refusal")
        assert [i["cycles_per_step"] for i in ai] == [i["cycles_per_step"] for i in bi]
    finally:
        hs.close()
    assert mg.lib().mg_heat_stepper_set_coefficient(None, None) == 2 and mg.lib().mg_heat_stepper_has_coefficient(None) == 0
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg._check()
    with pytest.raises(TypeError):
        mg.HeatStepper(N, 1.0, coef=a)


def test_right_hand_side_refusals_leave_the_engine_usable(mg):
    N = 64
    U, Q = fields(N, 1100)
    a = vref.field("exp", N)
    ad, Ud, Qd, Fd = mg.DeviceGrid.from_host(a), mg.DeviceGrid.from_host(U), mg.DeviceGrid.from_host(Q), poisoned(mg, N)
    big = mg.DeviceGrid.from_host(np.ones((N + 1, N)))
    off = lambda g, n: types.SimpleNamespace(ptr=g.ptr + 8 * n, shape=(N, N))
    want = hvref.rhs(N, 1.0, NU, DT, 0.5, a, U, Q)
    bad = [(ad, Ud, Qd, ad), (ad, Ud, Qd, Ud), (ad, Ud, Qd, Qd),          # F overlaps a, U, Q
           (big, Ud, Qd, off(big, 2)),                                   # ... partly
           (off(big, 1), Ud, Qd, Fd), (ad, off(big, 1), Qd, Fd), (ad, Ud, off(big, 1), Fd), (ad, Ud, Qd, off(big, 1))]   # misaligned
    for av, uv, qv, fv in bad:
        with pytest.raises(mg.MGError, match=r"\[2\]"):
            mg.heat_rhs_coef(N, 1.0, NU, DT, 0.5, av, uv, qv, fv)
        assert_bits(mg.heat_rhs_coef(N, 1.0, NU, DT, 0.5, ad, Ud, Qd, Fd).to_host(), want, "after a refused call")
    for kw in (dict(theta=0.3), dict(nu=-1.0), dict(dt=float("nan"))):
        args = dict(dict(nu=NU, dt=DT, theta=0.5), **kw)
        with pytest.raises(mg.MGError, match=r"\[2\]"):
            mg.heat_rhs_coef(N, 1.0, args["nu"], args["dt"], args["theta"], ad, Ud, Qd, Fd)
    assert_bits(ad.to_host(), a, "a")
    assert_bits(Ud.to_host(), U, "U")


# ---------------------------------------------------------------- 9. torch
def test_torch_tensors_on_a_side_stream():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_heat_vc_torch_worker.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "HEAT_VC_TORCH OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
