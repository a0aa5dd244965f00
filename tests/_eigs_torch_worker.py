"""Subprocess worker: torch is imported FIRST; the start vectors and the coefficient are float64 torch CUDA tensors and the
eigen-solve runs on a non-default torch stream (torch.cuda.current_stream()), in place, checked bit for bit against the same
solve on numpy arrays."""
import os
import sys

import torch  # first, on purpose

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import _solve_vc_ref as vref  # noqa: E402
import multigrid_poisson_solver_amd as mg  # noqa: E402

mg.init(0)
N, k = 33, 3   # N odd: the second vector of a contiguous [k, N, N] tensor is not 16-byte aligned and goes through staging
a = vref.field("exp", N)
X0 = np.random.default_rng(3).random((k, N, N)) - 0.5
with mg.EigenSolver(N, 1.0, k=k, coef=a) as e:
    lam_want, X_want, info_want = e.solve(X0=X0, seed=9)
assert info_want["converged"]
tX = torch.from_numpy(X0).cuda()
torch.cuda.synchronize()
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    ta = torch.from_numpy(a).cuda(non_blocking=True)
    with mg.EigenSolver(N, 1.0, k=k, coef=ta) as e:
        lam, out, info = e.solve(X0=tX, seed=9)
    assert out is tX
st.synchronize()
got = tX.cpu().numpy()
assert info["converged"] and info["iters"] == info_want["iters"]
assert np.array_equal(lam.view(np.uint64), lam_want.view(np.uint64)), "eigenvalues on torch tensors differ from the numpy solve"
assert np.array_equal(got.view(np.uint64), X_want.view(np.uint64)), "vectors on torch tensors differ from the numpy solve"
print("OK")
