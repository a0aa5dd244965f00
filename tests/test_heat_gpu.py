"""The heat stepper (include/mg_heat.h) on the device: the right-hand-side kernel bit for bit against the restatement
(tests/_heat_ref.py) over every form it has (one column per lane, two columns from even N = 512, non-temporal from 4096;
theta = 1 without neighbours) and inside guard bands; the stepper against its own building blocks (heat_rhs + Solver with
shift = sigma) and against the numpy restatement; the batch against single steppers; fmg, the cycle cap, the refusals, the
simple smoother and torch tensors.

Bit comparison of a step means: U bit for bit (zero_sign as in the other solve tests: the solver's folded sign flip) and the
cycles of every step equal; every case against numpy first qualifies its input (coarse margin >= 1e-10)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _guard
import _heat_ref as href
import _solve_ref as ref
from conftest import assert_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NU, DT = 0.5, 2e-4          # sigma = 1/(theta*1e-4): 1e4 (theta = 1), 2e4 (theta = 0.5)
RHS_SIZES = [6, 7, 17, 64, 100, 255, 256, 257, 511, 512, 513, 1024, 1025]
THETAS = [1.0, 0.5, 0.75]
NAN_BITS = np.uint64(0xFFFFFFFFFFFFFFFF)


def poisoned(mg, N):
    """an F no element of which the kernel may leave unwritten"""
    return mg.DeviceGrid.from_host(np.full((N, N), NAN_BITS, dtype=np.uint64).view(np.float64))


def fields(N, seed):
    Q, U = ref.random_problem(N, seed)
    return U, 40.0 * Q


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("N", RHS_SIZES)
def test_heat_rhs_bit_identical_to_restatement(mg, N):
    U, Q = fields(N, 100 + N)
    Ud, Qd, Fd = mg.DeviceGrid.from_host(U), mg.DeviceGrid.from_host(Q), poisoned(mg, N)
    nan = Fd.to_host()
    for theta in THETAS:
        for L in (1.0, 2.5):
            for q, qd in ((None, None), (Q, Qd)):
                mg.lib().mg_upload(Fd.ptr, nan.ctypes.data, nan.size)
                got = mg.heat_rhs(N, L, NU, DT, theta, Ud, qd, Fd).to_host()
                assert_bits(got, href.rhs(N, L, NU, DT, theta, U, q), f"N={N} theta={theta} L={L} Q={'yes' if q is not None else 'no'}")
    assert_bits(Ud.to_host(), U, "U")
    assert_bits(Qd.to_host(), Q, "Q")


def test_heat_rhs_non_temporal_form(mg):
    """N = 4096: two columns per lane with non-temporal accesses of F and Q; theta = 0.5 with Q and theta = 1 without."""
    N = 4096
    U, Q = fields(N, 4096)
    Ud, Qd, Fd = mg.DeviceGrid.from_host(U), mg.DeviceGrid.from_host(Q), poisoned(mg, N)
    assert_bits(mg.heat_rhs(N, 1.0, NU, DT, 0.5, Ud, Qd, Fd).to_host(), href.rhs(N, 1.0, NU, DT, 0.5, U, Q), "theta=0.5 with Q")
    assert_bits(mg.heat_rhs(N, 2.5, NU, DT, 1.0, Ud, None, Fd).to_host(), href.rhs(N, 2.5, NU, DT, 1.0, U), "theta=1 without Q")


@pytest.mark.parametrize("place", list(_guard.PLACEMENTS))
@pytest.mark.parametrize("N", [17, 256, 512, 513])
def test_heat_rhs_inside_guard_bands(mg, N, place):
    U, Q = fields(N, 300 + N)
    with _guard.block(mg, [N] * 3, place) as b:
        Uv, Qv, Fv = b.views
        Uv.upload(U)
        Qv.upload(Q)
        for theta, qv, q in ((0.5, Qv, Q), (1.0, Qv, Q), (0.75, None, None)):
            Fv.poison()
            b.expect_readonly(Uv, Qv)
            mg.heat_rhs(N, 1.0, NU, DT, theta, Uv, qv, Fv)
            assert_bits(Fv.to_host(), href.rhs(N, 1.0, NU, DT, theta, U, q), f"N={N} {place} theta={theta}")
            b.check(f"mg_heat_rhs N={N} theta={theta}")


# ---------------------------------------------------------------- the stepper
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("N", [17, 64, 257])
def test_stepper_equals_its_building_blocks(mg, N, theta):
    U, Q = fields(N, 500 + N)
    opts = dict(rtol=1e-8)
    hs = mg.HeatStepper(N, 1.0, NU, DT, theta, **opts)
    sv = mg.Solver(N, 1.0, shift=hs.sigma, **opts)
    try:
        assert hs.sigma == href.consts(N, 1.0, NU, DT, theta)[0]
        Ua, Ub, Qd, Fd = mg.DeviceGrid.from_host(U), mg.DeviceGrid.from_host(U), mg.DeviceGrid.from_host(Q), poisoned(mg, N)
        _, infos = hs.step(Ua, Qd, steps=3)
        cycles = []
        for _ in range(3):
            mg.heat_rhs(N, 1.0, NU, DT, theta, Ub, Qd, Fd)
            _, info = sv.solve(Fd, Ub)
            cycles.append(info["cycles"])
        assert_bits(Ua.to_host(), Ub.to_host(), f"N={N} theta={theta}: stepper vs heat_rhs + Solver")
        assert infos[0]["cycles_per_step"] == cycles and infos[0]["steps"] == 3 and infos[0]["cycles"] == sum(cycles)
        assert infos[0]["status"] == 0 and infos[0]["res"] == info["res"] and infos[0]["ref_norm"] == info["ref_norm"]
        assert sum(cycles) > 0
        assert_bits(Qd.to_host(), Q, "Q")
    finally:
        hs.close(); sv.close()


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("N", [17, 64, 100])
def test_stepper_bit_identical_to_restatement(mg, oracle, N, theta):
    U, Q = fields(N, 600 + N)
    margins = []
    want, cycles, conv = href.run(oracle, U, Q, steps=2, L=2.5, nu=NU, dt=DT, theta=theta, rtol=1e-8, margins=margins)
    ref.assert_qualified(margins, f"N={N} theta={theta}")
    hs = mg.HeatStepper(N, 2.5, NU, DT, theta, rtol=1e-8)
    try:
        got, infos = hs.step(U, Q, steps=2)
    finally:
        hs.close()
    assert_bits(got, want, f"N={N} theta={theta}", zero_sign=True)
    assert conv and infos[0]["converged"] and infos[0]["cycles_per_step"] == cycles and sum(cycles) > 0


def batch_fields(N):
    """three fields that need different numbers of cycles: random, a smooth mode on a random rim, and a field (zero, no
    source) whose right-hand side is zero -- its solve runs no cycle at all"""
    U0, Q0 = fields(N, 700 + N)
    U1, Q1 = fields(N, 701 + N)
    x = np.sin(np.pi * np.arange(N) / (N - 1))
    U1[1:-1, 1:-1] = np.outer(x, x)[1:-1, 1:-1]
    return [U0, U1, np.zeros((N, N))], [Q0, Q1, np.zeros((N, N))]


@pytest.mark.parametrize("N", [64, 129])
def test_batch_instances_equal_single_steppers(mg, N):
    theta, opts = 0.5, dict(rtol=1e-8)
    Us, Qs = batch_fields(N)
    single = mg.HeatStepper(N, 1.0, NU, DT, theta, **opts)
    batch = mg.HeatStepper(N, 1.0, NU, DT, theta, max_batch=3, **opts)
    try:
        assert batch.sigma == single.sigma
        own = [single.step(u, q, steps=3) for u, q in zip(Us, Qs)]
        shared = [single.step(u, Qs[0], steps=3) for u in Us]
        assert len({tuple(i[0]["cycles_per_step"]) for _, i in own}) > 1, "the instances need the same cycles in every step"
        for order in ([0, 1, 2], [2, 0, 1]):
            got, infos = batch.step(np.stack([Us[i] for i in order]), np.stack([Qs[i] for i in order]), steps=3)
            for j, i in enumerate(order):
                assert_bits(got[j], own[i][0], f"N={N} order {order} instance {i}: per-instance Q")
                for key in ("status", "steps", "cycles", "cycles_per_step", "coarse_capped", "res", "ref_norm"):
                    assert infos[j][key] == own[i][1][0][key], (order, i, key)
            got, infos = batch.step(np.stack([Us[i] for i in order]), Qs[0], steps=3)
            for j, i in enumerate(order):
                assert_bits(got[j], shared[i][0], f"N={N} order {order} instance {i}: shared Q")
                assert infos[j]["cycles_per_step"] == shared[i][1][0]["cycles_per_step"]
        # entries of Q may be NULL: that instance has no source
        Ud = [mg.DeviceGrid.from_host(u) for u in Us[:2]]
        Qd = mg.DeviceGrid.from_host(Qs[1])
        batch.step_ptrs([u.ptr for u in Ud], [None, Qd.ptr], steps=1)
        assert_bits(Ud[0].to_host(), single.step(Us[0], None, steps=1)[0], "NULL entry of Q")
        assert_bits(Ud[1].to_host(), single.step(Us[1], Qs[1], steps=1)[0], "non-NULL entry beside a NULL one")
    finally:
        single.close(); batch.close()


def test_right_hand_side_launches_do_not_grow_with_the_batch(mg):
    """one right-hand-side launch per step whatever n is (the solver's launches per cycle: test_solve_batched_gpu.py)"""
    N, steps = 64, 3
    Us, Qs = batch_fields(N)
    batch = mg.HeatStepper(N, 1.0, NU, DT, 0.5, max_batch=3, rtol=1e-8)
    try:
        counts = []
        for n in (1, 3):
            mg.profile_begin(0)
            batch.step(np.stack(Us[:n]), np.stack(Qs[:n]), steps=steps)
            counts.append(sum(e["launches"] for e in mg.profile_end() if e["name"].startswith("heat_rhs")))
        assert counts == [steps, steps]
    finally:
        batch.close()


@pytest.mark.parametrize("N", [64, 100])
def test_fmg_start_through_the_single_solver(mg, oracle, N):
    U, Q = fields(N, 800 + N)
    margins = []
    want, cycles, conv = href.run(oracle, U, Q, steps=2, nu=NU, dt=DT, theta=0.5, rtol=1e-8, fmg=1, margins=margins)
    ref.assert_qualified(margins, f"N={N} fmg")
    hs = mg.HeatStepper(N, 1.0, NU, DT, 0.5, rtol=1e-8, fmg=1)
    try:
        got, infos = hs.step(U, Q, steps=2)
    finally:
        hs.close()
    assert_bits(got, want, f"N={N} fmg=1", zero_sign=True)
    assert infos[0]["cycles_per_step"] == cycles and conv
    with pytest.raises(mg.MGError, match=r"\[2\].*mg_batch_solver_create.*fmg"):
        mg.HeatStepper(N, 1.0, NU, DT, 0.5, max_batch=2, fmg=1)


def test_a_step_that_does_not_converge_is_the_last(mg, oracle):
    N = 64
    U, Q = fields(N, 900)
    opts = dict(max_cycles=1, rtol=1e-12)
    margins = []
    want, cycles, conv = href.run(oracle, U, Q, steps=3, nu=NU, dt=DT, theta=0.5, margins=margins, **opts)
    ref.assert_qualified(margins, "capped")
    assert cycles == [1] and not conv
    for mb in (1, 2):
        hs = mg.HeatStepper(N, 1.0, NU, DT, 0.5, max_batch=mb, **opts)
        try:
            got, infos = hs.step(U, Q, steps=3)
        finally:
            hs.close()
        assert infos[0]["status"] == mg.MG_SOLVE_NOT_CONVERGED and infos[0]["steps"] == 1 and infos[0]["cycles_per_step"] == [1]
        assert_bits(got, want, f"max_batch={mb}: one capped step", zero_sign=True)


def test_refusals_leave_the_engine_usable(mg):
    N = 64
    U, Q = fields(N, 1000)
    good = dict(nu=NU, dt=DT, theta=0.5, rtol=1e-8)
    hs = mg.HeatStepper(N, 1.0, max_batch=2, **good)
    try:
        before, _ = hs.step(U, Q, steps=2)
        bad_create = [dict(nu=v) for v in (0.0, -1.0, float("nan"), float("inf"))] + \
                     [dict(dt=v) for v in (0.0, -1e-3, float("nan"), float("inf"))] + \
                     [dict(theta=v) for v in (0.49, 1.01, 0.0, float("nan"))] + [dict(shift=1.0), dict(shift=float("nan"))]
        for bad in bad_create:
            with pytest.raises(mg.MGError, match=r"\[2\]"):
                mg.HeatStepper(N, 1.0, **dict(good, **bad))
            assert_bits(hs.step(U, Q, steps=2)[0], before, f"a step after the refused creation {bad}")
        with pytest.raises(mg.MGError, match=r"\[2\]"):
            mg.HeatStepper(N, 1.0, max_batch=0, **good)
        Ud = [mg.DeviceGrid.from_host(U), mg.DeviceGrid.from_host(U)]
        Qd = mg.DeviceGrid.from_host(Q)
        big = mg.DeviceGrid((N + 1, N))
        p = [u.ptr for u in Ud]
        bad_step = [(p, None, 0), (p, None, -1),                                  # steps < 1
                    ([], None, 1), (p + [big.ptr], None, 1),                      # n outside [1, max_batch]
                    ([p[0], None], None, 1),                                      # NULL U
                    ([big.ptr + 8], None, 1), ([p[0]], [Qd.ptr + 8], 1),          # misaligned U, Q
                    ([p[0], p[0]], None, 1), ([big.ptr, big.ptr + 16], None, 1),  # U overlapping U
                    ([p[0]], [p[0]], 1), (p, [Qd.ptr, p[0]], 1)]                  # U overlapping Q
        for U_ptrs, Q_ptrs, steps in bad_step:
            with pytest.raises(mg.MGError, match=r"\[2\]"):
                hs.step_ptrs(U_ptrs, Q_ptrs, steps)
            assert_bits(Ud[0].to_host(), U, "U after a refused step")
            assert_bits(hs.step(U, Q, steps=2)[0], before, f"a step after the refused step {(len(U_ptrs), steps)}")
        for bad in (dict(theta=0.3), dict(nu=-1.0), dict(dt=float("nan"))):
            args = dict(dict(nu=NU, dt=DT, theta=0.5), **bad)
            with pytest.raises(mg.MGError, match=r"\[2\]"):
                mg.heat_rhs(N, 1.0, args["nu"], args["dt"], args["theta"], Ud[0], Qd)
        with pytest.raises(mg.MGError, match=r"\[2\]"):
            mg.heat_rhs(N, 1.0, NU, DT, 0.5, Ud[0], Qd, Ud[0])
        assert_bits(hs.step(U, Q, steps=2)[0], before, "a step after the refused heat_rhs calls")
    finally:
        hs.close()


def test_simple_smoother_gives_the_same_bits(mg):
    N = 256
    U, Q = fields(N, 1100)
    hs = mg.HeatStepper(N, 1.0, NU, DT, 0.5, rtol=1e-8)
    try:
        fused, fi = hs.step(U, Q, steps=2)
        mg.set_smoother("simple")
        try:
            simple, si = hs.step(U, Q, steps=2)
        finally:
            mg.set_smoother("stream")
    finally:
        hs.close()
    assert_bits(fused, simple, "fused vs simple", zero_sign=True)
    assert fi[0]["cycles_per_step"] == si[0]["cycles_per_step"] and sum(fi[0]["cycles_per_step"]) > 0


def test_torch_tensors():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_heat_torch_worker.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "HEAT_TORCH OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
