"""Subprocess worker: torch is imported FIRST; the coefficient, U and Q are float64 torch CUDA tensors, the coefficient is set
and the steps run on a non-default torch stream (torch.cuda.current_stream()), checked bit for bit against the restatement
(tests/_heat_vc_ref.py).  The coefficient tensor is overwritten right after set_coefficient: the stepper's solver keeps the
only copy."""
import os
import sys

import torch  # first, on purpose

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import _oracle  # noqa: E402
import _heat_vc_ref as hvref  # noqa: E402
import _solve_ref as ref  # noqa: E402
import _solve_vc_ref as vref  # noqa: E402
import multigrid_poisson_solver_amd as mg  # noqa: E402

mg.init(0)
orc = _oracle.Oracle()
N, NU, DT, THETA = 129, 0.5, 2e-4, 0.5
Q, U0 = ref.random_problem(N, 41)
Q = 40.0 * Q
a = vref.field("exp", N)
tU, tQ = torch.from_numpy(U0).cuda(), torch.from_numpy(Q).cuda()
torch.cuda.synchronize()
hs = mg.HeatStepper(N, 1.0, NU, DT, THETA, rtol=1e-8)
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    ta = torch.from_numpy(a).cuda(non_blocking=True)
    ta.mul_(1.0)   # queued on the side stream ahead of set_coefficient
    tU.mul_(1.0)
    hs.set_coefficient(ta)
    ta.fill_(-1.0)
    out, infos = hs.step(tU, tQ, steps=2)
    assert out is tU
st.synchronize()
margins = []
want, cycles, conv = hvref.run(orc, a, U0, Q, steps=2, nu=NU, dt=DT, theta=THETA, rtol=1e-8, margins=margins,
                               table=lambda n, m: mg.restriction_table(n, m))
ref.assert_qualified(margins, "torch worker")
got = tU.cpu().numpy()
assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "variable-coefficient steps on torch tensors differ"
assert infos[0]["cycles_per_step"] == cycles and conv and infos[0]["converged"] and hs.has_coefficient
assert np.array_equal(tQ.cpu().numpy().view(np.uint64), Q.view(np.uint64)), "Q changed"
assert mg.lib().mg_get_stream() != st.cuda_stream, "the engine stream was not restored"
hs.close()
mg.finalize()
print("HEAT_VC_TORCH OK")
