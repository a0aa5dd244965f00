"""Subprocess worker: torch is imported FIRST; F and U are float64 torch CUDA tensors and the accelerated solve (GCR(4) on a
variable coefficient) runs on a non-default torch stream (torch.cuda.current_stream()), checked bit for bit against the
replay of its own log (tests/_krylov_ref.py)."""
import os
import sys

import torch  # first, on purpose

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import _oracle  # noqa: E402
import _krylov_ref as kref  # noqa: E402
import _solve_ref as ref  # noqa: E402
import _solve_vc_ref as vref  # noqa: E402
import multigrid_poisson_solver_amd as mg  # noqa: E402

mg.init(0)
orc = _oracle.Oracle()
N = 129
F, U0 = ref.random_problem(N, 21)
a = vref.field("jump", N)
opts = dict(rtol=1e-9, max_cycles=10)
tF, tU = torch.from_numpy(F).cuda(), torch.from_numpy(U0).cuda()
torch.cuda.synchronize()
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    ta = torch.from_numpy(a).cuda(non_blocking=True)
    s = mg.Solver(N, 1.0, coef=ta, krylov=4, **opts)
    out, info = s.solve(tF, tU)
    assert out is tU
st.synchronize()
log = s.krylov_log()
margins = []
want = kref.solve(orc, a, F, U0, 1.0, m=4, log=log, margins=margins, table=lambda n, m: mg.restriction_table(n, m), **opts)
ref.assert_qualified(margins, "torch worker")
got = tU.cpu().numpy()
assert np.array_equal(got.view(np.uint64), want["U"].view(np.uint64)), "accelerated solve on torch tensors differs from its replay"
assert info["cycles"] == 10 == len(log) and s.krylov == 4 and not info["breakdown"]
assert info["history"][1:] == [e["rho"] for e in log]
assert [e["restarted"] for e in log] == [False, False, False, True, False, False, False, True, False, False]
assert mg.lib().mg_get_stream() != st.cuda_stream, "the engine stream was not restored"
s.close()
mg.finalize()
print("SOLVE_KRYLOV_TORCH OK")
