"""One batched solve of B instances of N x N (getSource, U = 0) for a fixed number of cycles, for a kernel trace:
   rocprofv3 --kernel-trace --stats -d DIR -f csv -- python scripts/trace_solve_batched.py --B 16 --cycles 3
The dispatches per cycle are the difference of two traces with different --cycles over the cycle difference; they do not
depend on B (batched solver)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multigrid_poisson_solver_amd as mg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=257)
ap.add_argument("--B", type=int, default=1)
ap.add_argument("--cycles", type=int, default=3)
a = ap.parse_args()
mg.init(0)
F = mg.getSource(a.N)
U = [mg.DeviceGrid.zeros((a.N, a.N)) for _ in range(a.B)]
bs = mg.BatchSolver(a.N, 1.0, max_batch=a.B, rtol=0.0, atol=0.0, max_cycles=a.cycles)
infos = bs.solve_ptrs([F.ptr] * a.B, [u.ptr for u in U])
print(f"N={a.N} B={a.B} cycles={infos[0]['cycles']} launches={infos[0]['stats']['launches']}", flush=True)
bs.close()
mg.finalize()
