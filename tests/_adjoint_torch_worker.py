"""Subprocess worker: torch is imported FIRST.  multigrid_poisson_solver_amd.autograd.DifferentiableSolver on float64 CUDA
tensors: F.grad, U0.grad and a.grad of J = sum(W*U) bit for bit against Solver.adjoint on the same data, for one (N, N)
problem and for a [3, N, N] batch; two forwards with different coefficients followed by both backwards (the stale-coefficient
counter); and a directional finite-difference check of a.grad on the device against the same quantity on the CPU.

The directional check: J = 0.5*sum((U - U_obs)^2), a fixed random direction d, eps = 1e-4,
    q = |(J(a + eps d) - J(a - eps d))/(2 eps) - <a.grad, d>|.
On the CPU (direct_solution and the restatement, the same data) q is the truncation error of the central difference:
measured q_cpu = 4.77e-09 (<g, d> = 1.70).  The device must stay within 10 q_cpu: the margin covers the solves' rtol 1e-10
against the dense solve (the numpy restatement of the solver at that rtol gives q = 1.17e-08)."""
import os
import sys

import torch  # first, on purpose

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import _adjoint_ref as aref  # noqa: E402
import _solve_vc_ref as vref  # noqa: E402
import multigrid_poisson_solver_amd as mg  # noqa: E402
from multigrid_poisson_solver_amd.autograd import DifferentiableSolver  # noqa: E402

N, L, EPS = 33, 1.0, 1e-4


def bits(x, y, what):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)), what


def data(seed, name):
    rng = np.random.default_rng(seed)
    return (40.0 * rng.standard_normal((N, N)), rng.standard_normal((N, N)), rng.standard_normal((N, N)), vref.field(name, N, L, seed=seed))


def dev(x, grad=True):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().requires_grad_(grad)


def single_reference(F, U0, W, a):
    s = mg.Solver(N, L, coef=a)
    try:
        U, fi = s.solve(F, U0)
        lam, gA, gU, ai = s.adjoint(W, U)
    finally:
        s.close()
    assert fi["converged"] and ai["converged"]
    return U, aref.zero_rim(lam), gU, gA


mg.init(0)
ds = DifferentiableSolver(N, L, max_batch=3)

# ---- one (N, N) problem, on a side stream
F, U0, W, a = data(1, "exp")
want = single_reference(F, U0, W, a)
st = torch.cuda.Stream()
torch.cuda.synchronize()
with torch.cuda.stream(st):
    tF, tU0, ta, tW = dev(F), dev(U0), dev(a), dev(W, False)
    U = ds.solve(tF, tU0, ta)
    assert U.grad_fn is not None and U.data_ptr() != tU0.data_ptr()
    U.mul(tW).sum().backward()
st.synchronize()
bits(U.detach().cpu().numpy(), want[0], "U")
bits(tF.grad.cpu().numpy(), want[1], "F.grad")
bits(tU0.grad.cpu().numpy(), want[2], "U0.grad")
bits(ta.grad.cpu().numpy(), want[3], "a.grad")
bits(tU0.detach().cpu().numpy(), U0, "U0 was written")
assert mg.lib().mg_get_stream() != st.cuda_stream, "the engine stream was not restored"

# ---- only the gradients that are required are computed
tF, tU0, ta = dev(F), dev(U0, False), dev(a, False)
ds.solve(tF, tU0, ta).mul(tW).sum().backward()
torch.cuda.synchronize()
bits(tF.grad.cpu().numpy(), want[1], "F.grad alone")
assert tU0.grad is None and ta.grad is None

# ---- a [3, N, N] batch with a coefficient per instance
sets = [data(10 + i, name) for i, name in enumerate(("smooth", "exp", "jump"))]
tF, tU0, tW, ta = (dev(np.stack([s[k] for s in sets]), k != 2) for k in range(4))
ds.solve(tF, tU0, ta).mul(tW).sum().backward()
torch.cuda.synchronize()
for i, s in enumerate(sets):
    w = single_reference(*s)
    bits(tF.grad[i].cpu().numpy(), w[1], f"batch F.grad[{i}]")
    bits(tU0.grad[i].cpu().numpy(), w[2], f"batch U0.grad[{i}]")
    bits(ta.grad[i].cpu().numpy(), w[3], f"batch a.grad[{i}]")

# ---- two forwards with different coefficients, then both backwards: each gets its own gradient
(F1, U01, W1, a1), (F2, U02, W2, a2) = data(21, "exp"), data(22, "smooth")
t1, t2 = [dev(x) for x in (F1, U01, a1)], [dev(x) for x in (F2, U02, a2)]
J1 = ds.solve(*t1).mul(dev(W1, False)).sum()
J2 = ds.solve(*t2).mul(dev(W2, False)).sum()
J1.backward()      # the solver holds a2 now: the counter makes this backward put a1 back
J2.backward()
torch.cuda.synchronize()
for t, w, what in ((t1, single_reference(F1, U01, W1, a1), "first"), (t2, single_reference(F2, U02, W2, a2), "second")):
    bits(t[0].grad.cpu().numpy(), w[1], what + " forward: F.grad")
    bits(t[1].grad.cpu().numpy(), w[2], what + " forward: U0.grad")
    bits(t[2].grad.cpu().numpy(), w[3], what + " forward: a.grad")

# ---- strict: a solve that does not converge raises
lax = DifferentiableSolver(N, L, max_cycles=1)
try:
    lax.solve(dev(F), dev(U0), dev(a))
    raise SystemExit("a forward solve that did not converge was accepted")
except mg.MGError as e:
    assert "did not converge" in str(e)
lax.close()

# ---- the directional check of a.grad
F, U0, _, a = data(31, "smooth")
rng = np.random.default_rng(32)
U_obs, d = rng.standard_normal((N, N)), rng.standard_normal((N, N))


def J_cpu(a_):
    U = vref.direct_solution(a_, F, U0, L, 0.0)
    return 0.5 * np.sum((U - np.asarray(U_obs, dtype=vref.LD)) ** 2)


U_ref = np.asarray(vref.direct_solution(a, F, U0, L, 0.0), dtype=np.float64)
lam_ref = np.asarray(aref.direct_adjoint(a, U_ref - U_obs, L, 0.0), dtype=np.float64)
g_cpu = aref.coefficient_gradient(N, L, lam_ref, U_ref)
q_cpu = abs(float((J_cpu(a + EPS * d) - J_cpu(a - EPS * d)) / (2 * EPS)) - float(np.sum(g_cpu * d)))


def J_dev(a_, grad):
    ta = dev(a_, grad)
    U = ds.solve(dev(F, False), dev(U0, False), ta)
    J = 0.5 * ((U - dev(U_obs, False)) ** 2).sum()
    if grad:
        J.backward()
    return float(J.item()), ta.grad


_, g_dev = J_dev(a, True)
q_dev = abs((J_dev(a + EPS * d, False)[0] - J_dev(a - EPS * d, False)[0]) / (2 * EPS) - float((g_dev * dev(d, False)).sum().item()))
print(f"directional check: q_cpu = {q_cpu:.3e}, q_dev = {q_dev:.3e}, <g, d> = {float(np.sum(g_cpu * d)):.3e}")
assert q_dev <= 10.0 * q_cpu, (q_dev, q_cpu)

ds.close()
mg.finalize()
print("ADJOINT_TORCH OK")
