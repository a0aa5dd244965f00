"""Subprocess worker: torch is imported FIRST; HeatStepper steps a [B, N, N] float64 torch CUDA tensor in place on a
non-default torch stream -- N = 65 is odd, so every odd instance goes through the staging buffer -- with one shared (N, N) Q,
checked bit for bit against the restatement (tests/_heat_ref.py)."""
import os
import sys

import torch  # first, on purpose

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import _oracle  # noqa: E402
import _heat_ref as href  # noqa: E402
import _solve_ref as ref  # noqa: E402
import multigrid_poisson_solver_amd as mg  # noqa: E402

mg.init(0)
orc = _oracle.Oracle()
N, B, NU, DT, THETA = 65, 3, 0.5, 2e-4, 0.5
Q = 40.0 * ref.random_problem(N, 30)[0]
U0 = np.stack([ref.random_problem(N, 31 + i)[1] for i in range(B)])
tU, tQ = torch.from_numpy(U0).cuda(), torch.from_numpy(Q).cuda()
assert any(tU[i].data_ptr() % 16 for i in range(B)), "no instance is misaligned: the staging path is not exercised"
torch.cuda.synchronize()
hs = mg.HeatStepper(N, 1.0, NU, DT, THETA, max_batch=B, rtol=1e-8)
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    tU.mul_(1.0)   # queued on the side stream ahead of the steps
    out, infos = hs.step(tU, tQ, steps=2)
    assert out is tU
st.synchronize()
got = tU.cpu().numpy()
for i in range(B):
    margins = []
    want, cycles, conv = href.run(orc, U0[i], Q, steps=2, nu=NU, dt=DT, theta=THETA, rtol=1e-8, margins=margins)
    ref.assert_qualified(margins, f"torch worker instance {i}")
    assert np.array_equal((got[i] + 0.0).view(np.uint64), (want + 0.0).view(np.uint64)), f"instance {i} differs"
    assert infos[i]["cycles_per_step"] == cycles and conv and infos[i]["converged"]
assert np.array_equal(tQ.cpu().numpy().view(np.uint64), Q.view(np.uint64)), "Q changed"
assert mg.lib().mg_get_stream() != st.cuda_stream, "the engine stream was not restored"
hs.close()
mg.finalize()
print("HEAT_TORCH OK")
