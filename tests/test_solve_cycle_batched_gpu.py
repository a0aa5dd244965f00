"""The batched executor of the recorded cycle where fused and unfused levels meet: four levels from
N = 64 (every level fuses), 65 (level 0 does not) and 66 (level 1, 33 points, does not while level 0 does) -- the smallest
shapes with a fused level above, below and beside an unfused one -- under sweep counts of both parities of every swap and
of the final copy.  Each instance of a batch whose instances leave the active set at different cycles equals Solver on it
alone, bit for bit; the launches are those of the slowest instance alone; under guard bands nothing but each U is written.

The right-hand sides are scaled so that the instances need different numbers of cycles: measured 9 / 9-11 / 12 under V(2,1)
and V(1,2), 6 / 6-7 / 10-12 under V(3,3).  V(1,1) reduces the residual by less than 1e-6 in 12 cycles whatever the scale
(the start is never below ||F||), so there every instance runs all max_cycles and the batch stays whole: that case holds
the sweep parities on an unchanged active set, V(3,3) the same parities on a shrinking one."""
import numpy as np
import pytest

import _guard
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
KEYS = ("status", "cycles", "converged", "coarse_capped", "res0", "res", "ref_norm", "history")
B = 3
SCALES = (2.0 ** 30, 2.0 ** 12, 1.0)   # of F: the residual of the random start weighs about 1e-5, 1 and 1e4 of ||F||
OPTS = dict(rtol=1e-6, max_cycles=12)
_singles = {}


def problems(N):
    FU = [ref.random_problem(N, 4000 + N + i) for i in range(B)]
    As = [vref.field(name, N, seed=N + i) for i, name in enumerate(("smooth", "exp", "random"))]
    return As, [f * s for (f, _), s in zip(FU, SCALES)], [u for _, u in FU]


def singles(mg, N, pp, coef):
    """[(U, info)] of Solver on each instance alone (the streaming smoother): computed once per problem, shared by the variants"""
    key = (N, pp, coef)
    if key not in _singles:
        As, Fs, Us = problems(N)
        out = []
        for i in range(B):
            s = mg.Solver(N, 1.0, pre=pp[0], post=pp[1], **(dict(coef=As[i]) if coef else {}), **OPTS)
            out.append(s.solve(Fs[i], Us[i]))
            s.close()
        _singles[key] = out
    return _singles[key]


@pytest.mark.parametrize("variant", ["stream", "simple", "coef"])
@pytest.mark.parametrize("pp", [(1, 1), (2, 1), (1, 2), (3, 3)])
@pytest.mark.parametrize("N", [64, 65, 66])
def test_batch_equals_singles_where_fused_meets_unfused(mg, N, pp, variant):
    coef = variant == "coef"
    opts = dict(pre=pp[0], post=pp[1], **OPTS)
    As, Fs, Us = problems(N)
    want = singles(mg, N, pp, coef)
    cycles = [info["cycles"] for _, info in want]
    print(f"N={N} V{pp} {variant}: cycles {cycles}")
    if pp == (1, 1):   # (the docstring: the batch stays whole)
        assert cycles == [OPTS["max_cycles"]] * B
    else:
        assert len(set(cycles)) > 1, "the instances must leave the active set at different cycles"
    slowest = int(np.argmax(cycles))
    if variant == "simple":
        mg.set_smoother("simple")
    try:
        with _guard.block(mg, [N] * (3 * B), "odd16") as gb:
            ga, gF, gU = gb.views[0:B], gb.views[B:2 * B], gb.views[2 * B:3 * B]
            for views, arrays in ((ga, As), (gF, Fs), (gU, Us)):
                for v, x in zip(views, arrays):
                    v.upload(x)
            b = mg.BatchSolver(N, 1.0, max_batch=B, **opts)
            if coef:
                b.set_coefficient(ga)
            gb.expect_readonly(*ga, *gF)
            infos = b.solve_ptrs([v.ptr for v in gF], [v.ptr for v in gU])
            gb.check(f"N={N} V{pp} {variant}")
            b.close()
            got_U = [v.to_host() for v in gU]
        alone = []   # every instance through a batch solver of one
        for i in range(B):
            b1 = mg.BatchSolver(N, 1.0, max_batch=1, **opts)
            if coef:
                b1.set_coefficient(As[i])
            _, one = b1.solve(Fs[i][None], Us[i][None])
            b1.close()
            alone.append(one[0])
    finally:
        mg.set_smoother("stream")
    for i, (U, info) in enumerate(want):
        assert_bits(got_U[i], U, f"N={N} V{pp} {variant}: instance {i} U")
        for k in KEYS:
            assert infos[i][k] == info[k] == alone[i][k], (N, pp, variant, i, k, infos[i][k], info[k], alone[i][k])
    launches = infos[0]["stats"]["launches"]
    print(f"N={N} V{pp} {variant}: launches {launches}, alone {[a['stats']['launches'] for a in alone]}")
    if variant == "simple":
        # operator by operator the cycle runs instance by instance: 4 launches of the two starting norms, 2 of the norm per
        # batched cycle, and every instance's own cycles as it runs them alone
        own = [a["stats"]["launches"] - 4 - 2 * a["cycles"] for a in alone]
        assert launches == 4 + 2 * max(cycles) + sum(own)
    else:
        assert launches == alone[slowest]["stats"]["launches"]
