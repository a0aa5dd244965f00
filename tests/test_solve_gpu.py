"""The residual-tolerance solver (mg_solver_*) on the device against its restatement on the oracle's operators
(tests/_solve_ref.py): bit for bit per cycle, the residual history, the reference driver at omega = 1, the edge cases
of the stopping rule and the options, torch tensors on a non-default stream, and the product sizes' kernels."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _solve_ref as ref
import _synth
from conftest import assert_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWEEPS = [(1, 1), (2, 2), (3, 3), (2, 1)]
OMEGAS = [1.0, 0.8, 2.0 / 3.0]
SMALL = [17, 33, 64, 65, 100, 129, 256, 257]
LARGE = [1000, 1025, 2048, 4097]


def _cases():
    out = [(N, pp, w) for N in SMALL for pp in SWEEPS for w in OMEGAS]
    out += [(N, (3, 3), 0.8) for N in LARGE]
    out += [(N, (2, 1), 1.0) for N in LARGE]
    out += [(2048, (1, 1), 2.0 / 3.0), (1000, (2, 2), 2.0 / 3.0)]
    out += [(N, pp, 0.8) for N in (1025, 4097) for pp in ((1, 1), (2, 2))]   # odd: the one-column-per-lane forms
    return out


def _fixed_cycles(mg, N, **opts):
    return mg.Solver(N, 1.0, rtol=0.0, atol=0.0, max_cycles=1, **opts)


@pytest.mark.parametrize("N,pp,omega", _cases())
def test_cycles_bit_identical_to_restatement(mg, oracle, N, pp, omega):
    F, U0 = ref.random_problem(N, 1000 + N)
    opts = dict(pre=pp[0], post=pp[1], omega=omega)
    s = _fixed_cycles(mg, N, **opts)
    Fd, Ud = mg.DeviceGrid.from_host(F), mg.DeviceGrid.from_host(U0)
    want = U0
    for k in range(1, 4):
        _, info = s.solve(Fd, Ud)
        assert info["cycles"] == 1 and info["status"] == mg.MG_SOLVE_NOT_CONVERGED
        want = ref.cycle(oracle, F, want, **opts)
        assert_bits(Ud.to_host(), want, f"N={N} V{pp} omega={omega:.4f} after {k} cycles", zero_sign=True)
    s.close()


@pytest.mark.parametrize("N,pp,omega", [(100, (3, 3), 0.8), (129, (2, 1), 2.0 / 3.0), (256, (3, 3), 0.8), (257, (1, 1), 0.8),
                                        (1024, (4, 4), 0.8), (2048, (2, 2), 1.0), (1025, (3, 3), 0.8)])
def test_fused_path_equals_simple_smoother(mg, N, pp, omega):
    """The default cycle (fused weighted nodes of the streaming smoother) against MG_SMOOTHER=simple (one launch per
    operator): the same U after two cycles, bit for bit."""
    F, U0 = ref.random_problem(N, 50 + N)
    opts = dict(pre=pp[0], post=pp[1], omega=omega, rtol=0.0, max_cycles=2)
    fused, fi = mg.solve(F, U0, **opts)
    mg.set_smoother("simple")
    try:
        simple, si = mg.solve(F, U0, **opts)
    finally:
        mg.set_smoother("stream")
    assert_bits(fused, simple, f"N={N} V{pp} omega={omega:.4f}: fused vs simple", zero_sign=True)
    assert fi["history"] == si["history"]


@pytest.mark.parametrize("N,omega", [(129, 0.8), (257, 2.0 / 3.0), (100, 0.8)])
def test_history_matches_restatement_and_is_reproducible(mg, oracle, N, omega):
    F, U0 = ref.random_problem(N, 7 + N)
    opts = dict(omega=omega, rtol=1e-10, max_cycles=30)
    _, want_hist, want_k, want_conv = ref.solve(oracle, F, U0, **opts)
    runs = []
    for _ in range(2):
        U, info = mg.solve(F, U0, **opts)
        runs.append(info)
    a, b = runs
    assert a["history"] == b["history"], "two runs give different residual histories"
    assert a["cycles"] == want_k and a["converged"] == want_conv and len(a["history"]) == want_k + 1
    assert a["converged"] and a["status"] == mg.MG_SOLVE_CONVERGED
    np.testing.assert_allclose(a["history"], want_hist, rtol=1e-12, atol=0)
    assert a["ref_norm"] == pytest.approx(ref.ref_norm(F), rel=1e-12)
    assert a["res"] == a["history"][-1] and a["res0"] == a["history"][0]


@pytest.mark.parametrize("N", [128, 257])
def test_omega_one_is_the_reference_driver(mg, tmp_path, N):
    """omega = 1, coarse target 1e-7 absolute: one solve cycle from the one-cycle file's U is the two-cycle file."""
    plan1 = mg.CyclePlan(ref.write_vcycles(str(tmp_path / "V1.txt"), N, 8, 3, 1e-7, 1), fused=True, report=False, error=False)
    U1 = plan1.execute(fetch_U=True)["U"]
    plan1.close()
    plan2 = mg.CyclePlan(ref.write_vcycles(str(tmp_path / "V2.txt"), N, 8, 3, 1e-7, 2), fused=True, report=False, error=False)
    U2 = plan2.execute(fetch_U=True)["U"]
    plan2.close()
    F = mg.getSource(N)
    U = mg.DeviceGrid.from_host(U1)
    s = _fixed_cycles(mg, N, omega=1.0, coarse_rtol=0.0, coarse_atol=1e-7)
    s.solve(F, U)
    s.close()
    assert_bits(U.to_host(), U2, f"N={N}: solve cycle from U_1 vs the chained two-cycle file", zero_sign=True)


def test_converged_start_runs_no_cycle(mg):
    N = 65
    F, U0 = ref.random_problem(N, 3)
    Ud = mg.DeviceGrid.from_host(U0)
    _, info = mg.solve(F, Ud, atol=1e300)
    assert info["cycles"] == 0 and info["converged"] and info["history"] == [info["res0"]]
    assert_bits(Ud.to_host(), U0, "a converged start leaves U untouched")


def test_max_cycles_reports_not_converged(mg):
    N = 129
    F, U0 = ref.random_problem(N, 4)
    _, info = mg.solve(F, U0, rtol=1e-30, max_cycles=2)
    assert info["status"] == mg.MG_SOLVE_NOT_CONVERGED and not info["converged"] and info["cycles"] == 2
    assert len(info["history"]) == 3 and info["history"][2] < info["history"][0]


def test_coarse_cap_is_reported(mg):
    N = 64
    F, U0 = ref.random_problem(N, 5)
    _, info = mg.solve(F, U0, coarse_rtol=0.0, coarse_atol=1e-300, coarse_max_iters=3, max_cycles=1, rtol=0.0)
    assert info["coarse_capped"] and info["cycles"] == 1


@pytest.mark.parametrize("N,bad", [
    (64, dict(pre=0)), (64, dict(post=5)), (64, dict(N_min=2)), (64, dict(N_min=33)), (15, dict(N_min=8)),
    (64, dict(omega=0.0)), (64, dict(omega=1.5)), (64, dict(coarse_rtol=0.0, coarse_atol=0.0)),
    (64, dict(coarse_max_iters=0)), (64, dict(rtol=-1.0)), (64, dict(max_cycles=-1)), (64, dict(coarse_rtol=float("nan"))),
])
def test_bad_options_are_refused(mg, N, bad):
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg.Solver(N, 1.0, **bad)


def test_bad_length_is_refused(mg):
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg.Solver(64, -1.0)


@pytest.mark.parametrize("N", [256, 257])
def test_rim_comes_back_bit_exact(mg, N):
    F, U0 = ref.random_problem(N, 9)
    U, info = mg.solve(F, U0, rtol=0.0, max_cycles=3)
    assert info["cycles"] == 3
    for what, a, b in (("top", U[0], U0[0]), ("bottom", U[-1], U0[-1]), ("left", U[:, 0], U0[:, 0]), ("right", U[:, -1], U0[:, -1])):
        assert_bits(a, b, f"rim {what} N={N}")


def test_torch_tensors_on_a_side_stream():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_solve_torch_worker.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SOLVE_TORCH OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


def test_product_size_two_cycles(oracle):
    """8192^2 in a child process without the test suite's threshold overrides: the 16-byte non-temporal forms of the
    sweep, the norm and the transfer operators, checked by checksum against the restatement."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MG_")}
    out = subprocess.run([sys.executable, os.path.join(HERE, "_solve_big_worker.py"), "8192"], env=env, capture_output=True,
                         text=True, timeout=900)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("SOLVE_BIG ")]
    assert out.returncode == 0 and line, out.stdout[-2000:] + out.stderr[-3000:]
    child = json.loads(line[0][len("SOLVE_BIG "):])
    N = child["N"]
    F = oracle.getSource(N)
    U = np.zeros((N, N))
    hist = [ref.residual_norm(oracle, N, 1.0, U, F)]
    for _ in range(2):
        U = ref.cycle(oracle, F, U)
        hist.append(ref.residual_norm(oracle, N, 1.0, U, F))
    assert tuple(child["sum"]) == _synth.checksum(U), "2 solve cycles at 8192^2 differ from the restatement"
    np.testing.assert_allclose(child["history"], hist, rtol=1e-12, atol=0)
