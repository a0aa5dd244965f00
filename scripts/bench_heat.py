"""HeatStepper (include/mg_heat.h) against the way a caller steps without it -- torch forming F = -sigma*U, then
Solver.solve / BatchSolver.solve from U = u_old -- in one process, alternating, medians over --reps: N = 8192 with one field
and N = 257 with 64 fields, sigma = 1e4 (nu = 1, dt = 1/(theta*1e4)), theta = 1 and theta = 0.5, --steps steps after a
warm-up, rtol 1e-8, from a seeded random field.  Per case: ms per step (torch events around the call on the current
stream), cycles per step, and from a profiled run of its own the right-hand-side kernel's time and algorithmic bytes over
time (16 B per point without a source) as a share of the 8 TB/s HBM peak.  The caller's loop exists for theta = 1 only:
Crank-Nicolson needs the library's Laplacian.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multigrid_poisson_solver_amd as mg  # noqa: E402

HBM_PEAK = 8.0e12
SIGMA = 1e4
RTOL = 1e-8


def timed(fn):
    """ms of fn() on the current torch stream, by events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def case(N, B, theta, steps, warmup, reps):
    nu, dt = 1.0, 1.0 / (theta * SIGMA)
    gen = torch.Generator(device="cuda").manual_seed(1234 + N)
    U0 = torch.rand((B, N, N), dtype=torch.float64, device="cuda", generator=gen) - 0.5
    U = U0.clone()
    hs = mg.HeatStepper(N, 1.0, nu, dt, theta, max_batch=B, rtol=RTOL)
    out = dict(N=N, B=B, theta=theta, sigma=hs.sigma, steps=steps)

    def stepper():
        U.copy_(U0)
        return timed(lambda: hs.step(U, steps=steps)[1])

    runs = {"stepper": [], "caller": []}
    caller = None
    if theta == 1.0:
        F = torch.empty_like(U)
        sv = mg.Solver(N, 1.0, shift=hs.sigma, rtol=RTOL) if B == 1 else mg.BatchSolver(N, 1.0, max_batch=B, shift=hs.sigma, rtol=RTOL)

        def loop():
            cycles = []
            for _ in range(steps):
                torch.mul(U, -hs.sigma, out=F)
                if B == 1:
                    cycles.append(sv.solve(F[0], U[0])[1]["cycles"])
                else:
                    cycles.append(max(i["cycles"] for i in sv.solve(F, U)[1]))
            return cycles

        def caller():
            U.copy_(U0)
            return timed(loop)

    hs.step(U, steps=warmup)
    if caller:
        caller()
    for _ in range(reps):
        runs["stepper"].append(stepper())
        if caller:
            runs["caller"].append(caller())
    infos = runs["stepper"][-1][1]
    ms = statistics.median(t for t, _ in runs["stepper"])
    out.update(stepper_ms_per_step=round(ms / steps, 4), stepper_device_ms_per_step=round(infos[0]["device_ms"] / steps, 4),
               cycles_per_step=[max(i["cycles_per_step"][k] for i in infos) for k in range(steps)],
               converged=all(i["converged"] for i in infos))
    if caller:
        cms = statistics.median(t for t, _ in runs["caller"])
        out.update(caller_ms_per_step=round(cms / steps, 4), caller_cycles_per_step=runs["caller"][-1][1],
                   stepper_over_caller=round(ms / cms, 4))
        sv.close()
    # the right-hand-side kernel alone, from a profiled run of its own
    U.copy_(U0)
    torch.cuda.synchronize()
    mg.profile_begin(0)
    hs.step(U, steps=steps)
    rhs = [e for e in mg.profile_end() if e["name"].startswith("heat_rhs")]
    launches = sum(e["launches"] for e in rhs)
    us = 1e3 * sum(e["total_ms"] for e in rhs) / launches
    rate = rhs[0]["algo_bytes"] / (us * 1e-6)
    out.update(rhs_kernel=rhs[0]["name"], rhs_launches=launches, rhs_us=round(us, 2), rhs_bytes=rhs[0]["algo_bytes"],
               rhs_TBps=round(rate / 1e12, 3), rhs_share_of_hbm_peak=round(rate / HBM_PEAK, 3))
    hs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="8192:1,257:64", help="N:B pairs")
    a = ap.parse_args()
    mg.init(0)
    cases = []
    for pair in a.sizes.split(","):
        N, B = (int(v) for v in pair.split(":"))
        for theta in (1.0, 0.5):
            cases.append(case(N, B, theta, a.steps, a.warmup, a.reps))
    print(json.dumps(dict(metric="heat_step_ms", rtol=RTOL, sigma=SIGMA, reps=a.reps, cases=cases)), flush=True)
    mg.finalize()


if __name__ == "__main__":
    main()
