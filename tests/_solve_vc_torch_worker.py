"""Subprocess worker: torch is imported FIRST; the coefficient, F and U are float64 torch CUDA tensors, the coefficient is set
and the solve runs on a non-default torch stream (torch.cuda.current_stream()), checked bit for bit against the restatement.
The coefficient tensor is overwritten right after set_coefficient: the solver keeps a copy of its own."""
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
import _solve_vc_ref as vref  # noqa: E402
import multigrid_poisson_solver_amd as mg  # noqa: E402

mg.init(0)
orc = _oracle.Oracle()
N = 129
F, U0 = ref.random_problem(N, 21)
a = vref.field("exp", N)
tF, tU = torch.from_numpy(F).cuda(), torch.from_numpy(U0).cuda()
torch.cuda.synchronize()
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    ta = torch.from_numpy(a).cuda(non_blocking=True)
    ta.mul_(1.0)   # queued on the side stream ahead of set_coefficient
    s = mg.Solver(N, 1.0, rtol=0.0, max_cycles=2)
    s.set_coefficient(ta)
    ta.fill_(-1.0)
    out, info = s.solve(tF, tU)
    assert out is tU
st.synchronize()
levels = vref.coarsen_levels(a, 8, lambda n, m: mg.restriction_table(n, m))
margins, want = [], U0
for _ in range(2):
    want = vref.cycle(orc, levels, F, want, margins=margins)
ref.assert_qualified(margins, "torch worker")
got = tU.cpu().numpy()
assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "variable-coefficient solve on torch tensors differs"
assert info["cycles"] == 2 and s.has_coefficient
assert mg.lib().mg_get_stream() != st.cuda_stream, "the engine stream was not restored"
s.close()
mg.finalize()
print("SOLVE_VC_TORCH OK")
