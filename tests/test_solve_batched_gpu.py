"""The batched residual-tolerance solver (mg_batch_solver_*, BatchSolver, solve_batched) against single Solver solves of
each instance: U, history, cycles, status, res0, ref_norm and coarse_capped bit for bit, whatever the batch around an
instance; mixed convergence, shared F, order, the operator-by-operator smoother, launch counts, argument refusals, large
sizes and torch tensors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _solve_ref as ref
from conftest import assert_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm", "history")


def _problems(N, B, seed):
    return [ref.random_problem(N, seed + 97 * i) for i in range(B)]


def _single(mg, N, F, U0, **opts):
    s = mg.Solver(N, 1.0, **opts)
    try:
        return s.solve(F, U0)
    finally:
        s.close()


def _check_against_singles(mg, N, probs, U, infos, what, **opts):
    for i, (F, U0) in enumerate(probs):
        want_U, want = _single(mg, N, F, U0, **opts)
        assert_bits(U[i], want_U, f"{what}: instance {i} U")
        for k in KEYS:
            assert infos[i][k] == want[k], f"{what}: instance {i} {k}: {infos[i][k]} != {want[k]}"


def _cases():
    out = [(N, 3, (3, 3), 0.8) for N in (17, 33, 64, 65, 100, 129, 256, 257)]
    out += [(64, 16, (1, 1), 1.0), (65, 16, (2, 1), 2.0 / 3.0), (129, 1, (3, 3), 2.0 / 3.0), (100, 3, (2, 1), 1.0),
            (257, 16, (1, 1), 0.8), (256, 3, (2, 1), 2.0 / 3.0), (33, 16, (3, 3), 1.0)]
    out += [(1000, 3, (3, 3), 0.8), (1025, 3, (2, 1), 0.8), (2048, 3, (1, 1), 2.0 / 3.0), (1025, 1, (3, 3), 1.0)]
    return out


@pytest.mark.parametrize("N,B,pp,omega", _cases())
def test_every_instance_equals_its_single_solve(mg, N, B, pp, omega):
    probs = _problems(N, B, 300 + N)
    opts = dict(pre=pp[0], post=pp[1], omega=omega, rtol=1e-9, max_cycles=4)
    F = np.stack([p[0] for p in probs])
    U0 = np.stack([p[1] for p in probs])
    U, infos = mg.solve_batched(F, U0, **opts)
    assert U.shape == (B, N, N) and len(infos) == B
    _check_against_singles(mg, N, probs, U, infos, f"N={N} B={B} V{pp} omega={omega:.4f}", **opts)


def test_mixed_convergence_in_one_batch(mg):
    """One instance converged at the start (0 cycles, U untouched), one that converges in a few cycles, one that runs
    into max_cycles -- one problem scaled by powers of two, so that each instance's history is the first one's, scaled
    exactly, against one absolute tolerance."""
    N = 129
    F, U0 = ref.random_problem(N, 1)
    s = mg.Solver(N, 1.0, rtol=0.0, atol=0.0, max_cycles=3)
    U3, info = s.solve(F, U0)
    s.close()
    atol = info["history"][-1]
    start = [U3, U0 * 1024.0, U0 / 64.0]
    Fs = [F, F * 1024.0, F / 64.0]
    opts = dict(rtol=0.0, atol=atol, max_cycles=3)
    Ud = [mg.DeviceGrid.from_host(u) for u in start]
    Fd = [mg.DeviceGrid.from_host(f) for f in Fs]
    bs = mg.BatchSolver(N, 1.0, max_batch=3, **opts)
    infos = bs.solve_ptrs([f.ptr for f in Fd], [u.ptr for u in Ud])
    bs.close()
    assert infos[0]["cycles"] == 0 and infos[0]["converged"] and infos[0]["status"] == mg.MG_SOLVE_CONVERGED
    assert_bits(Ud[0].to_host(), U3, "a converged start leaves U untouched")
    assert infos[1]["cycles"] == 3 and not infos[1]["converged"] and infos[1]["status"] == mg.MG_SOLVE_NOT_CONVERGED
    assert 0 < infos[2]["cycles"] < 3 and infos[2]["converged"]
    assert infos[0]["stats"]["status"] == mg.MG_SOLVE_NOT_CONVERGED and infos[0]["stats"]["cycles"] == 3
    for i in range(3):
        want_U, want = _single(mg, N, Fs[i], start[i], **opts)
        assert_bits(Ud[i].to_host(), want_U, f"mixed batch instance {i}")
        for k in KEYS:
            assert infos[i][k] == want[k], (i, k)


def test_coarse_cap_is_reported_per_instance(mg):
    N = 64
    probs = _problems(N, 3, 5)
    opts = dict(coarse_rtol=0.0, coarse_atol=1e-300, coarse_max_iters=3, max_cycles=1, rtol=0.0)
    U, infos = mg.solve_batched(np.stack([p[0] for p in probs]), np.stack([p[1] for p in probs]), **opts)
    assert all(i["coarse_capped"] for i in infos)
    _check_against_singles(mg, N, probs, U, infos, "coarse cap", **opts)


@pytest.mark.parametrize("N", [128, 257])
def test_shared_F_different_rims(mg, N):
    F, _ = ref.random_problem(N, 11)
    probs = [(F, ref.random_problem(N, 20 + i)[1]) for i in range(4)]
    opts = dict(rtol=1e-10, max_cycles=12)
    U, infos = mg.solve_batched(F, np.stack([p[1] for p in probs]), **opts)
    _check_against_singles(mg, N, probs, U, infos, f"shared F N={N}", **opts)


def test_order_and_repeatability(mg):
    N = 100
    probs = _problems(N, 5, 40)
    opts = dict(rtol=1e-10, max_cycles=10)
    F = np.stack([p[0] for p in probs])
    U0 = np.stack([p[1] for p in probs])
    U, infos = mg.solve_batched(F, U0, **opts)
    U_again, infos_again = mg.solve_batched(F, U0, **opts)
    assert_bits(U, U_again, "two identical calls")
    perm = [3, 0, 4, 2, 1]
    Up, infos_p = mg.solve_batched(F[perm], U0[perm], **opts)
    for j, i in enumerate(perm):
        assert_bits(Up[j], U[i], f"permuted instance {i}")
        for k in KEYS:
            assert infos_p[j][k] == infos[i][k] == infos_again[i][k]


@pytest.mark.parametrize("N", [129, 256, 1025])
def test_fused_batch_equals_simple_batch(mg, N):
    probs = _problems(N, 3, 60)
    opts = dict(rtol=0.0, max_cycles=2)
    F = np.stack([p[0] for p in probs])
    U0 = np.stack([p[1] for p in probs])
    fused, fi = mg.solve_batched(F, U0, **opts)
    mg.set_smoother("simple")
    try:
        simple, si = mg.solve_batched(F, U0, **opts)
    finally:
        mg.set_smoother("stream")
    assert_bits(fused, simple, f"N={N}: fused batch vs simple batch")
    assert [i["history"] for i in fi] == [i["history"] for i in si]


@pytest.mark.parametrize("N", [128, 257])
def test_launches_per_call_do_not_depend_on_the_batch(mg, N):
    F, U0 = ref.random_problem(N, 70)
    opts = dict(rtol=0.0, max_cycles=3)
    _, one = mg.solve_batched(F[None], U0[None], **opts)
    _, many = mg.solve_batched(np.stack([F] * 16), np.stack([U0] * 16), **opts)
    assert one[0]["stats"]["cycles"] == many[0]["stats"]["cycles"] == 3
    assert one[0]["stats"]["launches"] == many[0]["stats"]["launches"]


def test_argument_errors_leave_every_U_unchanged(mg):
    N = 64
    lib = mg.lib()
    F, U0 = ref.random_problem(N, 80)
    Fd = mg.DeviceGrid.from_host(F)
    Ud = [mg.DeviceGrid.from_host(U0) for _ in range(3)]
    big = mg.DeviceGrid((2 * N, N))
    bs = mg.BatchSolver(N, 1.0, max_batch=3)

    def call(n, F_ptrs, U_ptrs, solver=None, out=True):
        Fa = (C.c_void_p * max(len(F_ptrs), 1))(*F_ptrs)
        Ua = (C.c_void_p * max(len(U_ptrs), 1))(*U_ptrs)
        res = (mg.SolveResult * 4)()
        st = mg.BatchSolveStats()
        code = lib.mg_batch_solver_solve(bs._s if solver is None else solver, n, Fa if F_ptrs is not None else None, Ua,
                                         res if out else None, C.byref(st))
        lib.mg_clear_error()
        return code

    u = [g.ptr for g in Ud]
    f = [Fd.ptr] * 3
    assert call(0, f, u) == 2
    assert call(4, f + [Fd.ptr], u + [big.ptr]) == 2
    assert call(3, f, [u[0], None, u[2]]) == 2
    assert call(3, [Fd.ptr, None, Fd.ptr], u) == 2
    assert call(3, f, [u[0], u[1] + 8, u[2]]) == 2               # misaligned
    assert call(3, f, [u[0], u[1], u[0]]) == 2                   # the same U twice
    assert call(2, f[:2], [big.ptr, big.ptr + 8 * N * 16]) == 2  # overlapping U
    assert call(2, [Fd.ptr, u[1]], [u[0], u[1]]) == 2            # U is another instance's F
    assert call(1, [u[0]], [u[0]]) == 2                          # U is its own F
    assert call(3, f, u, out=False) == 2
    assert lib.mg_batch_solver_solve(None, 1, (C.c_void_p * 1)(Fd.ptr), (C.c_void_p * 1)(u[0]), (mg.SolveResult * 1)(),
                                     None) == 2
    lib.mg_clear_error()
    for g in Ud:
        assert_bits(g.to_host(), U0, "U after a refused call")
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg.BatchSolver(N, 1.0, max_batch=0)
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg.BatchSolver(N, 1.0, max_batch=2, omega=1.5)
    bs.close()


@pytest.mark.parametrize("N", [4096, 4097])
def test_large_sizes(mg, N):
    probs = _problems(N, 2, 90)
    opts = dict(rtol=0.0, max_cycles=2)
    Fd = [mg.DeviceGrid.from_host(p[0]) for p in probs]
    Ud = [mg.DeviceGrid.from_host(p[1]) for p in probs]
    bs = mg.BatchSolver(N, 1.0, max_batch=2, **opts)
    infos = bs.solve_ptrs([f.ptr for f in Fd], [u.ptr for u in Ud])
    bs.close()
    for i, (f, u) in enumerate(zip(Fd, Ud)):
        want = mg.DeviceGrid.from_host(probs[i][1])
        s = mg.Solver(N, 1.0, **opts)
        _, wi = s.solve(f, want)
        s.close()
        assert u.checksum() == want.checksum(), f"N={N} instance {i}"
        assert infos[i]["history"] == wi["history"]
        want.free()


def test_torch_batches_on_a_side_stream():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_solve_batched_torch_worker.py")], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "SOLVE_BATCHED_TORCH OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
