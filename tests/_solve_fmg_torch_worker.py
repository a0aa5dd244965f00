"""Subprocess worker: torch is imported FIRST; a solve with the full-multigrid start works in place on float64 torch CUDA
tensors on a non-default torch stream, checked bit for bit against the restatement (tests/_solve_fmg_ref.py)."""
import os
import sys

import torch  # first, on purpose

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import _oracle  # noqa: E402
import _solve_fmg_ref as fref  # noqa: E402
import _solve_ref as ref  # noqa: E402
import multigrid_poisson_solver_amd as mg  # noqa: E402

mg.init(0)
orc = _oracle.Oracle()
N = 129
F, U0 = ref.random_problem(N, 21)
tF, tU = torch.from_numpy(F).cuda(), torch.from_numpy(U0).cuda()
torch.cuda.synchronize()
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    tU.mul_(1.0)   # queued on the side stream ahead of the solve
    out, info = mg.solve(tF, tU, rtol=0.0, max_cycles=2, fmg=1)
    assert out is tU
st.synchronize()
margins = []
want, hist, k, _ = fref.solve(orc, F, U0, rtol=0.0, max_cycles=2, fmg=1, margins=margins)
ref.assert_qualified(margins, "torch worker")
got = tU.cpu().numpy() + 0.0
assert np.array_equal(got.view(np.uint64), (want + 0.0).view(np.uint64)), "FMG solve on torch tensors differs"
assert info["cycles"] == 2 and np.allclose(info["history"], hist, rtol=1e-12, atol=0)
assert mg.lib().mg_get_stream() != st.cuda_stream, "the engine stream was not restored"
mg.finalize()
print("SOLVE_FMG_TORCH OK")
