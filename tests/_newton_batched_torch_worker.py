"""Subprocess worker: torch is imported FIRST, BatchSolver.newton_batch works in place on float64 torch CUDA tensors on a non-default
torch stream (torch.cuda.current_stream()), checked bit for bit against the numpy path of the same call.  N is odd, so the odd
instances of the contiguous [B, N, N] tensors are not 16-byte aligned and go through the staging buffers."""
import os
import sys

import torch  # first, on purpose

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import _newton_ref as nref  # noqa: E402
import multigrid_poisson_solver_amd as mg  # noqa: E402

mg.init(0)
N, B = 65, 3
F, U0 = nref.problem(N)
Fs, U0s = np.stack([F, 0.5 * F, 2.0 * F]), np.stack([U0, U0, 0.5 * U0])
ws = np.stack([nref.smooth_weight(N), 1.0 + nref.smooth_weight(N), np.ones((N, N))])
kappas = [10.0, 0.0, 30.0]
b = mg.BatchSolver(N, 1.0, max_batch=B)
want_U, want = b.newton_batch(Fs, U0s, kind="sinh", kappa=kappas, weight=ws)
tF, tU, tw = torch.from_numpy(Fs).cuda(), torch.from_numpy(U0s).cuda(), torch.from_numpy(ws).cuda()
torch.cuda.synchronize()
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    tU.mul_(1.0)   # queued on the side stream ahead of the solve
    out, infos = b.newton_batch(tF, tU, kind="sinh", kappa=kappas, weight=tw)
    assert out is tU
st.synchronize()
got = tU.cpu().numpy()
assert np.array_equal(got.view(np.uint64), want_U.view(np.uint64)), "newton on torch tensors differs"
assert list(infos) == list(want) and [i["iterations"] for i in infos] == [i["iterations"] for i in want]
assert infos[1]["iterations"] == 1 and all(i["converged"] for i in infos)
for key in ("status", "iterations", "trial_rounds", "inner_cycles", "launches"):
    assert infos.stats[key] == want.stats[key], key
assert mg.lib().mg_get_stream() != st.cuda_stream, "the engine stream was not restored"
assert not b.has_reaction
b.close()
mg.finalize()
print("NEWTON_BATCHED_TORCH OK")
