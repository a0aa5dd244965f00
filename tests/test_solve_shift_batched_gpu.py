"""The `shift` option through the batched solver: instance i of a BatchSolver with shift sigma is Solver(shift=sigma) on
it alone, bit for bit -- U, cycles, status, converged, coarse_capped, res0, res, ref_norm and history -- for B = 1, 3 and
16, with a shared F, with instances that leave the active set at different cycles, through the fused launches and through
MG_SMOOTHER=simple, and against the restatement (tests/_solve_shift_ref.py)."""
import numpy as np
import pytest

import _solve_ref as ref
import _solve_shift_ref as sref
from conftest import assert_bits

pytestmark = pytest.mark.gpu

KEYS = ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm", "history")


def same_as_single(mg, N, L, probs, what, **opts):
    bs = mg.BatchSolver(N, L, max_batch=len(probs), **opts)
    s = mg.Solver(N, L, **opts)
    try:
        Us, infos = bs.solve(np.stack([p[0] for p in probs]), np.stack([p[1] for p in probs]))
        for i, (F, U0) in enumerate(probs):
            want_U, want = s.solve(F, U0)
            assert_bits(Us[i], want_U, f"{what} instance {i} U")
            for k in KEYS:
                assert infos[i][k] == want[k], f"{what} instance {i} {k}: {infos[i][k]} != {want[k]}"
    finally:
        bs.close(); s.close()
    return Us, infos


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("N,L,sigma,pp,omega", [(64, 1.0, 1.0, (3, 3), 0.8), (100, 1e-3, 2.0 ** -20, (2, 1), 2.0 / 3.0),
                                                (256, 1.0, 1e4, (3, 3), 0.8), (257, 1e3, 1e8, (1, 1), 1.0),
                                                (1024, 1.0, 1e4, (2, 2), 0.8), (1025, 1.0, 1e4, (3, 3), 0.8)])
def test_batch_instance_equals_single_solve(mg, N, L, sigma, pp, omega, B):
    probs = [ref.random_problem(N, 100 * N + i) for i in range(B)]
    probs = [(F, U * min(1.0, L * L)) for F, U in probs]
    same_as_single(mg, N, L, probs, f"N={N} L={L:g} sigma={sigma:g} V{pp} B={B}", pre=pp[0], post=pp[1], omega=omega, rtol=1e-9,
                   max_cycles=4, shift=sigma)


@pytest.mark.parametrize("N,sigma", [(128, 1e4), (257, 1.0), (1024, 1e4)])
def test_shared_F(mg, N, sigma):
    """One F for every instance (the same source with different boundary values), given once."""
    F, _ = ref.random_problem(N, 17)
    Us0 = [ref.random_problem(N, 300 + i)[1] for i in range(3)]
    opts = dict(rtol=1e-9, max_cycles=5, shift=sigma)
    got, infos = mg.solve_batched(F, np.stack(Us0), **opts)
    for i, U0 in enumerate(Us0):
        want_U, want = mg.solve(F, U0, **opts)
        assert_bits(got[i], want_U, f"N={N} shared F instance {i}")
        for k in KEYS:
            assert infos[i][k] == want[k], (i, k)


@pytest.mark.parametrize("N,sigma", [(129, 1e4), (256, 1e2), (1024, 1e4)])
def test_instances_leave_the_active_set_at_different_cycles(mg, N, sigma):
    """Starts at different distances from the solution of one problem (a converged start, the solution perturbed by
    1e-9, 1e-5 and 1e-1, a random start): they meet atol after different numbers of cycles; every one equals its
    single solve."""
    F, U0 = ref.random_problem(N, 23)
    star, done = mg.solve(F, U0, rtol=1e-11, max_cycles=40, shift=sigma)
    atol = 1e-7 * done["ref_norm"]
    noise = ref.random_problem(N, 24)[1]
    noise[0] = noise[-1] = 0.0
    noise[:, 0] = noise[:, -1] = 0.0
    probs = [(F, star)] + [(F.copy(), star + e * noise) for e in (1e-9, 1e-5, 1e-1)] + [(F.copy(), U0)]
    _, infos = same_as_single(mg, N, 1.0, probs, f"N={N} sigma={sigma:g}", rtol=0.0, atol=atol, max_cycles=40, shift=sigma)
    cycles = [i["cycles"] for i in infos]
    print(f"N={N} sigma={sigma:g}: cycles per instance {cycles}")
    assert all(i["converged"] for i in infos) and cycles[0] == 0 and len(set(cycles)) >= 3, cycles


@pytest.mark.parametrize("N,sigma", [(100, 1e4), (256, 1.0), (257, 1e8), (1024, 1e4)])
def test_batched_fused_equals_simple_smoother(mg, N, sigma):
    probs = [ref.random_problem(N, 70 + N + i) for i in range(3)]
    Fs, Us = np.stack([p[0] for p in probs]), np.stack([p[1] for p in probs])
    opts = dict(rtol=0.0, max_cycles=2, shift=sigma)
    fused, fi = mg.solve_batched(Fs, Us, **opts)
    mg.set_smoother("simple")
    try:
        simple, si = mg.solve_batched(Fs, Us, **opts)
    finally:
        mg.set_smoother("stream")
    assert_bits(fused, simple, f"N={N} sigma={sigma:g}: batched fused vs simple", zero_sign=True)
    assert [i["history"] for i in fi] == [i["history"] for i in si]


@pytest.mark.parametrize("N,L,sigma", [(16, 1.0, 1.0), (100, 1e3, 1e4), (255, 1.0, 1e8), (256, 1e-3, 2.0 ** -20), (1024, 1.0, 1e4)])
def test_batch_against_restatement(mg, oracle, N, L, sigma):
    probs = [ref.random_problem(N, 900 + N + i) for i in range(3)]
    probs = [(F, U * min(1.0, L * L)) for F, U in probs]
    opts = dict(shift=sigma)
    got, infos = mg.solve_batched(np.stack([p[0] for p in probs]), np.stack([p[1] for p in probs]), L, rtol=0.0, max_cycles=2, **opts)
    for i, (F, U0) in enumerate(probs):
        margins = []
        want, hist, k, _ = sref.solve(oracle, F, U0, L, margins=margins, rtol=0.0, max_cycles=2, **opts)
        ref.assert_qualified(margins, f"N={N} instance {i}")
        assert_bits(got[i], want, f"N={N} L={L:g} sigma={sigma:g} instance {i}", zero_sign=True)
        np.testing.assert_allclose(infos[i]["history"], hist, rtol=1e-12, atol=0)
