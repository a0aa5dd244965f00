"""The batched solver across the option space: BatchSolver(N, L, ...) against single Solver solves of each instance, bit
for bit (U, history, cycles, status, res0, ref_norm, coarse_capped), at B = 3 and B = 16, over coarsest sizes 3..63, deep
hierarchies, L != 1, uneven sweep pairs and a small weight.  At coarsest 63 one launch runs 16 workgroups of 63.5 KB
LDS each: coarse_capped == 0 and the equal history show that the launch ran."""
import numpy as np
import pytest

import _solve_ref as ref
from conftest import assert_bits

pytestmark = pytest.mark.gpu

KEYS = ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm", "history")


def cases():
    out = []
    for Nc in (3, 7, 16, 33, 63):
        out += [(N, 1.0, dict(N_min=min(Nc, 32))) for N in (2 * Nc, 2 * Nc + 1)]
    out += [(100, 1.0, dict(N_min=3)), (257, 1.0, dict(N_min=5))]
    out += [(N, L, {}) for L in (0.3, 7.0) for N in (100, 256)]
    out += [(N, 1.0, dict(pre=a, post=b)) for N in (129, 256) for a, b in ((1, 4), (4, 1), (4, 4), (3, 2))]
    out += [(N, 1.0, dict(omega=0.05)) for N in (129, 256)]
    return out


def case_id(case):
    N, L, opts = case
    return f"N{N}-L{L:g}-" + "-".join(f"{k}{v}" for k, v in opts.items())


@pytest.mark.parametrize("B", [3, 16])
@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_every_instance_equals_its_single_solve(mg, case, B):
    N, L, opts = case
    opts = dict(opts, rtol=1e-9, max_cycles=4)
    probs = [ref.random_problem(N, 700 + N + 97 * i) for i in range(B)]
    Fd = [mg.DeviceGrid.from_host(p[0]) for p in probs]
    Ud = [mg.DeviceGrid.from_host(p[1]) for p in probs]
    bs = mg.BatchSolver(N, L, max_batch=B, **opts)
    try:
        infos = bs.solve_ptrs([f.ptr for f in Fd], [u.ptr for u in Ud])
    finally:
        bs.close()
    assert len(infos) == B
    s = mg.Solver(N, L, **opts)
    try:
        for i, (F, U0) in enumerate(probs):
            want_U, want = s.solve(F, U0)
            what = f"N={N} L={L} {opts} B={B} instance {i}"
            assert want["cycles"] > 0 and len(want["history"]) == want["cycles"] + 1
            assert not infos[i]["coarse_capped"], f"{what}: coarse solve capped"
            assert_bits(Ud[i].to_host(), want_U, f"{what} U")
            for k in KEYS:
                assert infos[i][k] == want[k], f"{what} {k}: {infos[i][k]} != {want[k]}"
    finally:
        s.close()
