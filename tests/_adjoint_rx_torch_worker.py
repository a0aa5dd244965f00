"""Subprocess worker: torch is imported FIRST.  DifferentiableSolver.solve_semilinear and solve_reaction on float64 CUDA tensors:
F.grad, U0.grad, a.grad, weight.grad / s.grad and kappa.grad of J = sum(W*U) bit for bit against Solver.newton_adjoint /
Solver.adjoint_reaction on the same data, for one (N, N) problem and for a [3, N, N] batch; a weight, a reaction term and a
kappa shared by the instances receive the sum over them; strict raises on an unconverged forward Newton solve."""
import os
import sys

import torch  # first, on purpose

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import _adjoint_ref as aref  # noqa: E402
import _newton_ref as nref  # noqa: E402
import _solve_vc_ref as vref  # noqa: E402
import multigrid_poisson_solver_amd as mg  # noqa: E402
from multigrid_poisson_solver_amd.autograd import DifferentiableSolver  # noqa: E402

N, L, KIND = 33, 1.0, "sinh"


def bits(x, y, what):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)), what


def data(seed, name):
    """F, U0, W, a, w, s"""
    rng = np.random.default_rng(seed)
    return (40.0 * rng.standard_normal((N, N)), rng.standard_normal((N, N)), rng.standard_normal((N, N)), vref.field(name, N, L, seed=seed),
            1.0 + rng.random((N, N)), 100.0 * rng.random((N, N)))


def dev(x, grad=True):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().requires_grad_(grad)


def newton_reference(F, U0, W, a, w, kappa):
    """(U, gF, gU0, gA, gW, gkappa) from Solver.newton and Solver.newton_adjoint"""
    s = mg.Solver(N, L, coef=a)
    try:
        U, fi = s.newton(F, U0, kind=KIND, kappa=kappa, weight=w)
        lam, gA, gU, gW, ai = s.newton_adjoint(W, U, F, kind=KIND, kappa=kappa, weight=w)
    finally:
        s.close()
    assert fi["converged"] and ai["converged"]
    return U, aref.zero_rim(lam), gU, gA, gW, ai["gkappa"]


def reaction_reference(F, U0, W, a, react):
    s = mg.Solver(N, L, coef=a, reaction=react)
    try:
        U, fi = s.solve(F, U0)
        lam, gA, gU, gS, ai = s.adjoint_reaction(W, U)
    finally:
        s.close()
    assert fi["converged"] and ai["converged"]
    return U, aref.zero_rim(lam), gU, gA, gS


mg.init(0)
ds = DifferentiableSolver(N, L, max_batch=3)

# ---- one (N, N) semilinear problem, on a side stream, kappa a 0-dim tensor that requires grad
F, U0, W, a, w, react = data(1, "exp")
want = newton_reference(F, U0, W, a, w, 0.7)
st = torch.cuda.Stream()
torch.cuda.synchronize()
with torch.cuda.stream(st):
    tF, tU0, ta, tw, tW = dev(F), dev(U0), dev(a), dev(w), dev(W, False)
    tk = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    U = ds.solve_semilinear(tF, tU0, kind=KIND, kappa=tk, weight=tw, a=ta)
    assert U.grad_fn is not None and U.data_ptr() != tU0.data_ptr()
    U.mul(tW).sum().backward()
st.synchronize()
bits(U.detach().cpu().numpy(), want[0], "U")
for t, g, what in ((tF, want[1], "F.grad"), (tU0, want[2], "U0.grad"), (ta, want[3], "a.grad"), (tw, want[4], "weight.grad")):
    bits(t.grad.cpu().numpy(), g, what)
bits(np.float64(tk.grad.item()), np.float64(want[5]), "kappa.grad")
bits(tU0.detach().cpu().numpy(), U0, "U0 was written")
assert mg.lib().mg_get_stream() != st.cuda_stream, "the engine stream was not restored"

# ---- only the gradients that are required are computed; a float kappa has no gradient
tF, tU0, tw = dev(F), dev(U0, False), dev(w, False)
ds.solve_semilinear(tF, tU0, kind=KIND, kappa=0.7, weight=tw, a=dev(a, False)).mul(tW).sum().backward()
torch.cuda.synchronize()
bits(tF.grad.cpu().numpy(), want[1], "F.grad alone")
assert tU0.grad is None and tw.grad is None

# ---- a [3, N, N] batch: a per instance, ONE weight shared by the instances, kappa per instance
sets = [data(10 + i, name) for i, name in enumerate(("smooth", "exp", "jump"))]
kap = [0.7, 1.5, 0.2]
w_shared = sets[0][4]
tF, tU0, tW, ta = (dev(np.stack([s[k] for s in sets]), k != 2) for k in range(4))
tw, tk = dev(w_shared), torch.tensor(kap, dtype=torch.float64, requires_grad=True)
ds.solve_semilinear(tF, tU0, kind=KIND, kappa=tk, weight=tw, a=ta).mul(tW).sum().backward()
torch.cuda.synchronize()
refs = [newton_reference(s[0], s[1], s[2], s[3], w_shared, kap[i]) for i, s in enumerate(sets)]
for i, r in enumerate(refs):
    bits(tF.grad[i].cpu().numpy(), r[1], f"batch F.grad[{i}]")
    bits(tU0.grad[i].cpu().numpy(), r[2], f"batch U0.grad[{i}]")
    bits(ta.grad[i].cpu().numpy(), r[3], f"batch a.grad[{i}]")
    bits(np.float64(tk.grad[i].item()), np.float64(r[5]), f"batch kappa.grad[{i}]")
bits(tw.grad.cpu().numpy(), torch.from_numpy(np.stack([r[4] for r in refs])).cuda().sum(0).cpu().numpy(), "the shared weight: the instance sum")

# ---- the same batch with a 0-dim kappa shared by the instances: the sum of the per-instance derivatives
tk = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
ds.solve_semilinear(dev(np.stack([s[0] for s in sets]), False), dev(np.stack([s[1] for s in sets]), False), kind=KIND, kappa=tk,
                    weight=dev(w_shared, False), a=dev(np.stack([s[3] for s in sets]), False)).mul(tW).sum().backward()
torch.cuda.synchronize()
gk = [newton_reference(s[0], s[1], s[2], s[3], w_shared, 0.7)[5] for s in sets]
bits(np.float64(tk.grad.item()), np.float64(torch.tensor(gk, dtype=torch.float64).sum().item()), "the shared kappa: the instance sum")

# ---- solve_reaction: one problem, then a batch with ONE reaction term shared by the instances
want = reaction_reference(F, U0, W, a, react)
tF, tU0, ta, ts = dev(F), dev(U0), dev(a), dev(react)
U = ds.solve_reaction(tF, tU0, ts, ta)
U.mul(dev(W, False)).sum().backward()
torch.cuda.synchronize()
bits(U.detach().cpu().numpy(), want[0], "reaction U")
for t, g, what in ((tF, want[1], "F.grad"), (tU0, want[2], "U0.grad"), (ta, want[3], "a.grad"), (ts, want[4], "s.grad")):
    bits(t.grad.cpu().numpy(), g, "reaction " + what)
tF, tU0, tW, ta = (dev(np.stack([s[k] for s in sets]), k != 2) for k in range(4))
ts = dev(react)
ds.solve_reaction(tF, tU0, ts, ta).mul(tW).sum().backward()
torch.cuda.synchronize()
refs = [reaction_reference(s[0], s[1], s[2], s[3], react) for s in sets]
for i, r in enumerate(refs):
    bits(tF.grad[i].cpu().numpy(), r[1], f"reaction batch F.grad[{i}]")
    bits(tU0.grad[i].cpu().numpy(), r[2], f"reaction batch U0.grad[{i}]")
    bits(ta.grad[i].cpu().numpy(), r[3], f"reaction batch a.grad[{i}]")
bits(ts.grad.cpu().numpy(), torch.from_numpy(np.stack([r[4] for r in refs])).cuda().sum(0).cpu().numpy(), "the shared s: the instance sum")
# the solvers hold no reaction afterwards: solve() gives what a fresh solver gives
plain = mg.Solver(N, L, coef=a)
try:
    bits(ds.solve(dev(F, False), dev(U0, False), dev(a, False)).cpu().numpy(), plain.solve(F, U0)[0], "solve after solve_reaction")
finally:
    plain.close()

# ---- strict: a forward Newton solve that does not converge raises
try:
    ds.solve_semilinear(dev(F), dev(U0), kind=KIND, kappa=0.7, max_iters=0)
    raise SystemExit("a forward Newton solve that did not converge was accepted")
except mg.MGError as e:
    assert "did not converge" in str(e)
lax = DifferentiableSolver(N, L, max_cycles=1)
try:
    U = lax.solve_semilinear(dev(F), dev(U0), kind=KIND, kappa=0.7, rtol=1.0)   # (the start meets rtol = 1: no inner solve)
    U.sum().backward()
    raise SystemExit("an adjoint solve that did not converge was accepted")
except mg.MGError as e:
    assert "adjoint" in str(e) and "did not converge" in str(e)
lax.close()

ds.close()
mg.finalize()
print("ADJOINT_RX_TORCH OK")
