"""The residual-tolerance solver across the option space that mg_solver_create accepts, bit for bit against the
restatement (tests/_solve_ref.py): every coarsest size 3..63 of the coarse solve (two-level hierarchies, even and odd),
deep hierarchies down to small and large coarsest grids, L != 1, all 16 (pre, post) pairs, small weights and the weight
just below 1, the fused cycle against the operator-by-operator one, and the residual history of a full solve.

Every bit comparison first asserts on the restatement that the input is qualified: the error of every
coarse solve of every compared cycle stays 1e-10 (relative) away from its target at the stopping iteration and the one
before, so the iteration count cannot depend on the summation order of the error."""
import numpy as np
import pytest

import _solve_ref as ref
from conftest import assert_bits

pytestmark = pytest.mark.gpu

PAIRS = [(a, b) for a in range(1, 5) for b in range(1, 5)]
PAIRS_WITH_4 = [p for p in PAIRS if 4 in p]
DEEP = [(100, 3), (96, 3), (257, 5), (256, 4), (1000, 31), (1024, 32), (1025, 17), (2048, 24), (513, 12)]
LENGTHS = [1e-3, 0.3, 2.5, 7.0, 1e3]
OMEGAS = [2.0 ** -20, 0.05, 0.5, float(np.nextafter(1.0, 0.0))]
TRUTH_CASES = [(65, 2.5, 4), (129, 0.3, 16), (100, 7.0, 3), (127, 1.0, 32), (257, 2.5, 8)]


def coarsest_cases():
    """(N, L, opts): the two-level hierarchies of every coarsest size, then the deep ones."""
    out = []
    for Nc in range(3, 64):
        for N in (2 * Nc, 2 * Nc + 1):
            out.append((N, 1.0, dict(N_min=min(Nc, 32))))
    out += [(N, 1.0, dict(N_min=N_min)) for N, N_min in DEEP]
    return out


def length_cases():
    out = [(N, L, dict(omega=0.8)) for L in LENGTHS for N in (64, 65, 100, 257, 1024, 1025)]
    out += [(N, 2.5, dict(omega=0.8, N_min=3)) for N in (100, 256)]
    return out


def sweep_cases():
    out = [(N, 1.0, dict(pre=a, post=b, omega=0.8)) for N in (100, 129, 256) for a, b in PAIRS]
    out += [(N, 1.0, dict(pre=a, post=b, omega=0.8)) for N in (1024, 1025, 2048) for a, b in PAIRS_WITH_4]
    return out


def weight_cases():
    return [(N, 1.0, dict(pre=a, post=b, omega=w)) for w in OMEGAS for N in (64, 129, 256) for a, b in ((2, 1), (3, 3))]


def fused_cases():
    """One case of each family, among them a coarsest 63 and a coarsest 3."""
    return [(126, 1.0, dict(N_min=32)), (127, 1.0, dict(N_min=32)), (6, 1.0, dict(N_min=3)), (7, 1.0, dict(N_min=3)),
            (100, 1.0, dict(N_min=3)), (1000, 1.0, dict(N_min=31)), (257, 7.0, dict(omega=0.8)), (1024, 1e-3, dict(omega=0.8)),
            (256, 2.5, dict(N_min=3)), (129, 1.0, dict(pre=1, post=4)), (2048, 1.0, dict(pre=4, post=1)),
            (256, 1.0, dict(pre=4, post=4)), (129, 1.0, dict(omega=OMEGAS[0])), (256, 1.0, dict(pre=2, post=1, omega=OMEGAS[3]))]


def case_id(case):
    N, L, opts = case
    return f"N{N}-L{L:g}-" + "-".join(f"{k}{v:.6g}" if isinstance(v, float) else f"{k}{v}" for k, v in opts.items())


def seed_of(N, L, opts):
    return 4000 + N + 7 * opts.get("N_min", 8) + 13 * opts.get("pre", 3) + 17 * opts.get("post", 3)


def restatement_cycles(oracle, N, L, opts, cycles):
    """The start, and U after each of `cycles` restatement cycles; raises when the input is not qualified."""
    F, U0 = ref.random_problem(N, seed_of(N, L, opts))
    margins, states, U = [], [], U0
    for _ in range(cycles):
        U = ref.cycle(oracle, F, U, L, margins=margins, **opts)
        states.append(U)
    ref.assert_qualified(margins, f"N={N} L={L} {opts}")
    return F, U0, states


def check_cycles(mg, oracle, N, L, opts):
    F, U0, want = restatement_cycles(oracle, N, L, opts, 3)
    s = mg.Solver(N, L, rtol=0.0, atol=0.0, max_cycles=1, **opts)
    Fd, Ud = mg.DeviceGrid.from_host(F), mg.DeviceGrid.from_host(U0)
    try:
        for k in range(3):
            _, info = s.solve(Fd, Ud)
            assert info["cycles"] == 1 and info["status"] == mg.MG_SOLVE_NOT_CONVERGED and not info["coarse_capped"]
            assert_bits(Ud.to_host(), want[k], f"N={N} L={L} {opts} after {k + 1} cycles", zero_sign=True)
    finally:
        s.close()


@pytest.mark.parametrize("case", coarsest_cases(), ids=case_id)
def test_every_coarsest_size(mg, oracle, case):
    check_cycles(mg, oracle, *case)


@pytest.mark.parametrize("case", length_cases(), ids=case_id)
def test_side_length(mg, oracle, case):
    check_cycles(mg, oracle, *case)


@pytest.mark.parametrize("case", sweep_cases(), ids=case_id)
def test_every_sweep_pair(mg, oracle, case):
    check_cycles(mg, oracle, *case)


@pytest.mark.parametrize("case", weight_cases(), ids=case_id)
def test_small_weights_and_the_weight_below_one(mg, oracle, case):
    check_cycles(mg, oracle, *case)


@pytest.mark.parametrize("case", fused_cases(), ids=case_id)
def test_fused_cycle_equals_simple(mg, case):
    N, L, opts = case
    F, U0 = ref.random_problem(N, seed_of(N, L, opts))
    opts = dict(opts, rtol=0.0, max_cycles=2)
    fused, fi = mg.solve(F, U0, L, **opts)
    mg.set_smoother("simple")
    try:
        simple, si = mg.solve(F, U0, L, **opts)
    finally:
        mg.set_smoother("stream")
    assert_bits(fused, simple, f"N={N} L={L} {opts}: fused vs simple", zero_sign=True)
    assert fi["history"] == si["history"] and len(fi["history"]) == 3
    assert not fi["coarse_capped"] and not si["coarse_capped"]


@pytest.mark.parametrize("N,L,N_min", TRUTH_CASES)
def test_history_of_a_full_solve(mg, oracle, N, L, N_min):
    F, U0 = ref.random_problem(N, 500 + N)
    opts = dict(N_min=N_min, rtol=1e-10, max_cycles=60)
    margins = []
    _, want_hist, want_k, want_conv = ref.solve(oracle, F, U0, L, margins=margins, **opts)
    ref.assert_qualified(margins, f"N={N} L={L} N_min={N_min}")
    _, info = mg.solve(F, U0, L, **opts)
    assert info["cycles"] == want_k and info["converged"] == want_conv and want_conv
    assert len(info["history"]) == want_k + 1
    np.testing.assert_allclose(info["history"], want_hist, rtol=1e-12, atol=0)
    assert info["res0"] == pytest.approx(ref.residual_norm(oracle, N, L, U0, F), rel=1e-12)
    assert info["ref_norm"] == pytest.approx(ref.ref_norm(F), rel=1e-12)
    assert info["res"] == info["history"][-1] and info["res0"] == info["history"][0]
