"""Residual-tolerance solver at N x N (default 8192), V(3,3), omega 0.8, on the getSource problem from U = 0: ms per
solve cycle in steady state next to mg_cycle_execute's V(3,3) in the same process, cycles and total ms to rtol 1e-10,
and the time of a 0-cycle solve (its two norms).  --shift SIGMA: the screened equation Laplace(U) - SIGMA*U = F instead
(mg_solve_opts.shift; the cycle-file V(3,3) beside it stays the Poisson cycle).  --fmg n: also the solve to --rtol with the
full-multigrid start (mg_solve_opts.fmg = n) against the cold start, alternating in this process, medians over --reps:
cycles, device ms of the whole solve, and the FMG pass alone (a max_cycles = 0 solve minus its two norms).  Prints one
JSON line."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multigrid_poisson_solver_amd as mg  # noqa: E402

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shift", type=float, default=0.0)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--fmg", type=int, default=0)
    a = ap.parse_args()
    N = a.N
    sh = dict(shift=a.shift) if a.shift != 0.0 else {}
    mg.init(0)
    F = mg.getSource(N)
    U = mg.DeviceGrid.zeros((N, N))
    # to convergence (the first solve also warms up)
    s = mg.Solver(N, 1.0, rtol=a.rtol, max_cycles=50, **sh)
    _, warm = s.solve(F, U)
    mg.lib().mg_fill_zero(U.ptr, N * N)
    _, conv = s.solve(F, U)
    s.close()
    # steady-state cycle: k fixed cycles minus k0 fixed cycles (the norm of U_0 and F cancel)
    def fixed(k):
        sk = mg.Solver(N, 1.0, rtol=0.0, atol=0.0, max_cycles=k, **sh)
        best = None
        for _ in range(a.reps):
            mg.lib().mg_fill_zero(U.ptr, N * N)
            _, info = sk.solve(F, U)
            best = info["device_ms"] if best is None else min(best, info["device_ms"])
        sk.close()
        return best
    t2, t6 = fixed(2), fixed(6)
    per_cycle = (t6 - t2) / 4.0
    # a max_cycles = 0 solve: the two norms (||F||, ||F - AU||) with their read-back.  The norm kernel's own time comes
    # from a kernel trace of this script (k_resnorm_pairs<true, true>, profiles/solve_norm_kernel_stats.txt)
    s0 = mg.Solver(N, 1.0, max_cycles=0, **sh)
    t0 = min(s0.solve(F, U)[1]["device_ms"] for _ in range(a.reps))
    s0.close()
    # mg_cycle_execute's V(3,3) in the same process
    path = os.path.join(tempfile.mkdtemp(), "V.txt")
    mg.write_vcycle_file(path, N, 8, 3, 1e-7)
    plan = mg.CyclePlan(path, fused=True, report=False, error=False)
    plan.execute()
    v33 = min(plan.execute()["device_ms"] for _ in range(a.reps))
    plan.close()
    out = dict(metric="solve_cycle_ms", N=N, pre=3, post=3, omega=0.8, shift=a.shift, rtol=a.rtol, solve_cycle_ms=round(per_cycle, 4),
               cycle_execute_v33_ms=round(v33, 4), cycles_to_rtol=conv["cycles"], converged=conv["converged"],
               total_ms_to_rtol=round(conv["device_ms"], 3), rel_residual=conv["res"] / conv["ref_norm"],
               rel_history=[float(f"{h / conv['ref_norm']:.3e}") for h in conv["history"]],
               zero_cycle_solve_ms=round(t0, 4))
    if a.fmg >= 1:
        import statistics
        cold = mg.Solver(N, 1.0, rtol=a.rtol, max_cycles=50, **sh)
        warm_start = mg.Solver(N, 1.0, rtol=a.rtol, max_cycles=50, fmg=a.fmg, **sh)
        pass_only = mg.Solver(N, 1.0, rtol=0.0, atol=0.0, max_cycles=0, fmg=a.fmg, **sh)
        runs = {"cold": [], "fmg": [], "pass": []}
        for rep in range(a.reps + 1):   # (the first round warms up)
            for name, sv in (("cold", cold), ("fmg", warm_start), ("pass", pass_only)):
                mg.lib().mg_fill_zero(U.ptr, N * N)
                _, info = sv.solve(F, U)
                if rep > 0:
                    runs[name].append(info)
        for sv in (cold, warm_start, pass_only):
            sv.close()
        med = lambda name: statistics.median(i["device_ms"] for i in runs[name])
        last = runs["fmg"][-1]
        out.update(fmg=a.fmg, fmg_reps=a.reps, cold_cycles=runs["cold"][-1]["cycles"], fmg_cycles=last["cycles"],
                   cold_solve_ms=round(med("cold"), 3), fmg_solve_ms=round(med("fmg"), 3),
                   fmg_pass_ms=round(med("pass") - t0, 3), fmg_converged=last["converged"],
                   fmg_rel_history=[float(f"{h / last['ref_norm']:.3e}") for h in last["history"]])
    print(json.dumps(out), flush=True)
    mg.finalize()


if __name__ == "__main__":
    main()
