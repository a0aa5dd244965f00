"""Subprocess worker: torch is imported FIRST; the coefficient, F and U are float64 torch CUDA tensors, coefficient and boundary
kinds are set and the solve runs on a non-default torch stream (torch.cuda.current_stream()), checked bit for bit against the
restatement (tests/_bc_ref.py), rim of the Neumann sides included."""
import os
import sys

import torch  # first, on purpose

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import _bc_ref as bref  # noqa: E402
import _solve_ref as ref  # noqa: E402
import _solve_vc_ref as vref  # noqa: E402
import multigrid_poisson_solver_amd as mg  # noqa: E402

mg.init(0)
N, bc = 129, "ndnn"
F, U0 = ref.random_problem(N, 21)
a = vref.field("exp", N)
tF, tU = torch.from_numpy(F).cuda(), torch.from_numpy(U0).cuda()
torch.cuda.synchronize()
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    ta = torch.from_numpy(a).cuda(non_blocking=True)
    ta.mul_(1.0)   # queued on the side stream ahead of set_coefficient
    s = mg.Solver(N, 1.0, rtol=0.0, max_cycles=2, bc=bc)
    s.set_coefficient(ta)
    ta.fill_(-1.0)
    out, info = s.solve(tF, tU)
    assert out is tU
    tg = torch.from_numpy(np.arange(4.0 * N).reshape(4, N) / N).cuda()
    ta2 = torch.from_numpy(a).cuda()
    tFe = mg.neumann_source(N, 1.0, bc, tF, tg, coef=ta2)
st.synchronize()
rt, pt = (lambda n, m: mg.restriction_table(n, m)), (lambda m, n: mg.boundary_prolongation_table(m, n))
levels = vref.coarsen_levels(a, 8, rt)
margins, want = [], U0
for _ in range(2):
    want = bref.cycle(levels, F, want, bc, margins=margins, rtable=rt, ptable=pt)
ref.assert_qualified(margins, "torch worker")
got = tU.cpu().numpy()
assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "boundary solve on torch tensors differs"
want_Fe = bref.neumann_source(N, 1.0, bc, a, F, np.arange(4.0 * N).reshape(4, N) / N)
assert np.array_equal(tFe.cpu().numpy().view(np.uint64), want_Fe.view(np.uint64)), "neumann_source on torch tensors differs"
assert info["cycles"] == 2 and s.has_coefficient and s.boundary == (1, 0, 1, 1)
assert not np.array_equal(got[0], U0[0]) and np.array_equal(got[-1], U0[-1]), "the Neumann rim is written, the Dirichlet rim kept"
assert mg.lib().mg_get_stream() != st.cuda_stream, "the engine stream was not restored"
s.close()
mg.finalize()
print("SOLVE_BC_TORCH OK")
