"""Subprocess worker: torch is imported FIRST, the solver works in place on float64 torch CUDA tensors on a
non-default torch stream (torch.cuda.current_stream()), checked bit for bit against the restatement."""
import os
import sys

import torch  # first, on purpose

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import _oracle  # noqa: E402
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
    out, info = mg.solve(tF, tU, rtol=0.0, max_cycles=2)
    assert out is tU
st.synchronize()
want = U0
for _ in range(2):
    want = ref.cycle(orc, F, want)
got = tU.cpu().numpy() + 0.0
assert np.array_equal(got.view(np.uint64), (want + 0.0).view(np.uint64)), "solve on torch tensors differs"
assert info["cycles"] == 2
assert mg.lib().mg_get_stream() != st.cuda_stream, "the engine stream was not restored"
mg.finalize()
print("SOLVE_TORCH OK")
