"""Adjoint sensitivities (include/mg_adjoint.h), measured in one process with the variants alternating.

  kernels   N = 8192: per repetition one launch each of the coefficient-gradient kernel (mg_coefficientGradient) and of
            k_heat_rhs<lap> with Q (mg_heat_rhs, theta = 1/2): the same 24 B per point -- two arrays read through rolling
            three-row windows, one written -- and the yardstick; and of the rim-gradient kernel (8 B per point).  Each timed by
            the engine's event pair around the launch (mg_profile_begin / mg_profile_end).  Medians over --kernel-reps with the
            spread (min, max), TB/s of algorithmic bytes, the ratio to the yardstick and the yardstick's own run-to-run spread.
  driver    N = 8192, a = 1 + 0.5 sin(2 pi x) cos(2 pi y), rtol 1e-8: Solver.adjoint_ptr (zero fill, adjoint solve, both
            gradients) against the forward-style solve of the same right-hand side from zero alone: host clock around work that
            ends in a device synchronise, medians over --reps.  Expected: 1 plus two array passes.
  batch     N = 257, B = 64, a coefficient per instance: BatchSolver.adjoint_ptrs against 64 Solver.adjoint_ptr calls.

Prints one JSON line and writes it to --out (default profiles/adjoint_bench_line.json); the kernel statistics of one
profiled adjoint call go to --stats (default profiles/adjoint_kernel_stats.csv)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multigrid_poisson_solver_amd as mg  # noqa: E402

RTOL = 1e-8
NU, SIGMA = 1.0, 1e4


def smooth_field(N, phase=0.0):
    x = np.arange(N) / float(N - 1)
    return 1.0 + 0.5 * np.sin(2 * np.pi * x + phase)[None, :] * np.cos(2 * np.pi * x)[:, None]


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def kernels(N, lam, U, Q, a, out, reps):
    theta, dt = 0.5, 1.0 / (0.5 * NU * SIGMA)
    calls = {"coef_grad": lambda: mg.coefficientGradient(N, 1.0, lam, U, out),
             "heat_rhs<lap>": lambda: mg.heat_rhs(N, 1.0, NU, dt, theta, U, Q, out),
             "rim_grad": lambda: mg.boundaryGradient(N, 1.0, a, lam, Q, out)}
    bytes_per_point = {"coef_grad": 24, "heat_rhs<lap>": 24, "rim_grad": 8}
    for f in calls.values():
        f()
    us = {k: [] for k in calls}
    for _ in range(reps):
        mg.profile_begin(0)
        for f in calls.values():
            f()
        got = {e["name"]: e for e in mg.profile_end()}
        for k in calls:
            assert got[k]["launches"] == 1 and got[k]["algo_bytes"] == bytes_per_point[k] * N * N, got[k]
            us[k].append(1e3 * got[k]["total_ms"])
    med = {k: statistics.median(v) for k, v in us.items()}
    return dict(reps=reps, us={k: spread(v) for k, v in us.items()}, bytes_per_point=bytes_per_point,
                TB_per_s={k: round(bytes_per_point[k] * N * N / (med[k] * 1e-6) / 1e12, 3) for k in calls},
                coef_grad_over_heat_rhs_lap=round(med["coef_grad"] / med["heat_rhs<lap>"], 4),
                heat_rhs_lap_spread=round((max(us["heat_rhs<lap>"]) - min(us["heat_rhs<lap>"])) / med["heat_rhs<lap>"], 4))


def driver(N, a_host, Ubar, U, lam, gA, gU, reps, stats_path):
    s = mg.Solver(N, 1.0, coef=a_host, rtol=RTOL)

    def adjoint():
        t = time.perf_counter()
        info = s.adjoint_ptr(Ubar.ptr, U.ptr, lam.ptr, gA.ptr, gU.ptr)
        mg.sync()
        return 1e3 * (time.perf_counter() - t), info

    def solve():
        mg.lib().mg_fill_zero(lam.ptr, lam.size)
        mg.sync()
        t = time.perf_counter()
        info = s.solve_ptr(Ubar.ptr, lam.ptr)
        mg.sync()
        return 1e3 * (time.perf_counter() - t), info

    adjoint()
    solve()
    runs = {"adjoint": [], "solve": []}
    for _ in range(reps):
        runs["adjoint"].append(adjoint())
        runs["solve"].append(solve())
    mg.profile_begin(0)
    adjoint()
    prof = mg.profile_end()
    s.close()
    with open(stats_path, "w") as f:
        f.write("name,N,launches,total_ms,algo_bytes\n")
        for e in sorted(prof, key=lambda e: -e["total_ms"]):
            f.write(f"{e['name']},{e['N']},{e['launches']},{e['total_ms']:.4f},{e['algo_bytes']:.0f}\n")
    ms = {k: [t for t, _ in v] for k, v in runs.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(reps=reps, rtol=RTOL, ms={k: spread(v) for k, v in ms.items()}, cycles=runs["adjoint"][-1][1]["cycles"],
                solve_cycles=runs["solve"][-1][1]["cycles"], converged=bool(runs["adjoint"][-1][1]["converged"]),
                adjoint_over_solve=round(med["adjoint"] / med["solve"], 4))


def batch(N, B, reps):
    rng = np.random.default_rng(3)
    a = [smooth_field(N, 0.1 * i) for i in range(B)]
    grids = lambda: [mg.DeviceGrid.from_host(rng.standard_normal((N, N))) for _ in range(B)]
    Ubar, U = grids(), grids()
    lam, gA, gU = ([mg.DeviceGrid((N, N)) for _ in range(B)] for _ in range(3))
    b = mg.BatchSolver(N, 1.0, max_batch=B, rtol=RTOL)
    b.set_coefficient(a)
    singles = [mg.Solver(N, 1.0, coef=a[i], rtol=RTOL) for i in range(B)]
    p = lambda gs: [g.ptr for g in gs]

    def batched():
        t = time.perf_counter()
        infos = b.adjoint_ptrs(p(Ubar), p(U), p(lam), p(gA), p(gU))
        mg.sync()
        return 1e3 * (time.perf_counter() - t), infos[0]["stats"]

    def each():
        t = time.perf_counter()
        for i in range(B):
            singles[i].adjoint_ptr(Ubar[i].ptr, U[i].ptr, lam[i].ptr, gA[i].ptr, gU[i].ptr)
        mg.sync()
        return 1e3 * (time.perf_counter() - t)

    batched()
    each()
    tb, te = [], []
    for _ in range(reps):
        tb.append(batched())
        te.append(each())
    stats = tb[-1][1]
    b.close()
    for s in singles:
        s.close()
    mb, me = statistics.median([t for t, _ in tb]), statistics.median(te)
    return dict(N=N, B=B, reps=reps, ms=dict(batched=spread([t for t, _ in tb]), singles=spread(te)), launches=stats["launches"],
                cycles=stats["cycles"], singles_over_batched=round(me / mb, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=21)
    ap.add_argument("--batch-N", type=int, default=257)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adjoint_bench_line.json"))
    ap.add_argument("--stats", default=os.path.join(ROOT, "profiles", "adjoint_kernel_stats.csv"))
    o = ap.parse_args()
    N = o.N
    mg.init(0)
    for path in (o.out, o.stats):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    a_host = smooth_field(N)
    a = mg.DeviceGrid.from_host(a_host)
    lam, U, Q = (mg.DeviceGrid.uniform((N, N), seed + N) for seed in (11, 1234, 4321))
    gA, gU = mg.DeviceGrid((N, N)), mg.DeviceGrid((N, N))
    out = dict(metric="adjoint", N=N, field="1 + 0.5 sin(2 pi x) cos(2 pi y)")
    out["kernels"] = kernels(N, lam, U, Q, a, gA, o.kernel_reps)
    out["driver"] = driver(N, a_host, Q, U, lam, gA, gU, o.reps, o.stats)
    for g in (a, lam, U, Q, gA, gU):
        g.free()
    out["batch"] = batch(o.batch_N, o.batch, o.reps)
    line = json.dumps(out)
    print(line, flush=True)
    with open(o.out, "w") as f:
        f.write(line + "\n")
    mg.finalize()


if __name__ == "__main__":
    main()
