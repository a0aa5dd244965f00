"""The full-multigrid start and the batched solver: the batched pass is not built, so mg_batch_solver_create refuses
fmg != 0 with MG_ERR_ARG -- an option is never silently ignored -- and stays what it was with fmg = 0."""
import numpy as np
import pytest

import _solve_ref as ref
from conftest import assert_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmg", [1, 2, 8, -1, 9])
def test_batched_solver_refuses_fmg_and_stays_usable(mg, fmg):
    N = 64
    F, U0 = ref.random_problem(N, 8)
    opts = dict(rtol=0.0, max_cycles=2)
    before, _ = mg.solve_batched(F[None], U0[None], **opts)
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg.BatchSolver(N, 1.0, max_batch=2, fmg=fmg)
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg.solve_batched(F[None], U0[None], fmg=fmg, **opts)
    after, _ = mg.solve_batched(F[None], U0[None], **opts)
    assert_bits(after, before, "a batched solve after a refused BatchSolver")


@pytest.mark.parametrize("N", [100, 256])
def test_batched_explicit_fmg_zero_is_the_option_left_out(mg, N):
    F, U0 = ref.random_problem(N, 60 + N)
    Fs, Us = np.stack([F, F + 1.0]), np.stack([U0, U0])
    opts = dict(rtol=1e-9, max_cycles=4)
    A, IA = mg.solve_batched(Fs, Us, **opts)
    B, IB = mg.solve_batched(Fs, Us, fmg=0, **opts)
    assert_bits(A, B, f"N={N}: batched fmg=0 vs default")
    assert IA[0]["stats"]["launches"] == IB[0]["stats"]["launches"]
    assert [i["history"] for i in IA] == [i["history"] for i in IB]
