"""The semilinear solve (include/mg_newton.h) against the reaction kernels it is layered over, in ONE process, alternating,
medians over --reps with min and max: N = 8192, a = 1 + 0.5 sin(2 pi x) cos(2 pi y), --kind sinh (cubic: the pass without exp
and division, which separates the arithmetic of g from the traffic).
  kernels   the pass, timed by the engine's own event pairs (mg_profile_begin / mg_profile_end):
              newton_residual_aw   no step, with a and w    48 B per point (U, a, w, F in; D, S out)
              newton_residual_a    no step, with a          40 B per point
              newton_step_a        the step form, with a    56 B per point (U, dlt, a, F in; V, D, S out)
              residual_rx_a        k_residual_rx on the same a, the yardstick: 40 B per point (U, a, s, F in; D out)
            byte models 48/40, 40/40 and 56/40 -- models, not thresholds.  yardstick_spread is (max - min)/median of the
            yardstick's own repetitions: a ratio above its model by more than that is an open item.
  newton    one Newton iteration (Solver.newton with max_iters = 1: the no-step pass, the coarsening of S, an inner solve of
            --cycles cycles at rtol = 0 and one step pass per trial) against one Solver(coef=a, reaction=s).solve of the same
            --cycles cycles, wall time around a synchronised call.  The model is that solve plus the passes.
Prints one JSON line and writes it to --out (default profiles/newton_bench_line.json).

Per-kernel times come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_newton.py --kernels
    python scripts/bench_newton.py --summarize DIR/.../*_kernel_trace.csv > profiles/newton_kernel_stats.txt"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multigrid_poisson_solver_amd as mg  # noqa: E402

HBM_PEAK = 8.0e12
KAPPA = 10.0


def fields(N):
    x = np.arange(N) / float(N - 1)
    w = np.sin(2 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]
    return 1.0 + 0.5 * w, 1.0 + 0.5 * w.T   # a, and a smooth weight


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def kernels(N, kind, a, w, U, dlt, F, V, D, S, reps):
    args = (N, 1.0, 0.0)
    calls = {"newton_residual_aw": (lambda: mg.nonlinear_residual(*args, a, kind, KAPPA, w, U, F, D, S), "newton_residual", 48),
             "newton_residual_a": (lambda: mg.nonlinear_residual(*args, a, kind, KAPPA, None, U, F, D, S), "newton_residual", 40),
             "newton_step_a": (lambda: mg.nonlinear_residual(*args, a, kind, KAPPA, None, U, F, D, S, dlt=dlt, t=0.5, V=V), "newton_step", 56),
             "residual_rx_a": (lambda: mg.residualReaction(*args, a, w, U, F, D), "residual_rx_a", 40)}
    for f, _, _ in calls.values():
        f()   # warm-up of every shape
    us = {k: [] for k in calls}
    for _ in range(reps):
        for k, (f, name, bpp) in calls.items():
            mg.profile_begin(0)
            f()
            got = {e["name"]: e for e in mg.profile_end()}
            assert got[name]["launches"] == 1 and got[name]["algo_bytes"] == bpp * N * N, got[name]
            us[k].append(1e3 * got[name]["total_ms"])
    med = {k: statistics.median(v) for k, v in us.items()}
    y = "residual_rx_a"
    return dict(reps=reps, us={k: spread(v) for k, v in us.items()}, bytes_per_point={k: c[2] for k, c in calls.items()},
                share_of_hbm_peak={k: round(calls[k][2] * N * N / (med[k] * 1e-6) / HBM_PEAK, 3) for k in calls},
                over_yardstick={k: round(med[k] / med[y], 4) for k in calls if k != y},
                bytes_model={k: round(calls[k][2] / 40, 4) for k in calls if k != y},
                yardstick_spread=round((max(us[y]) - min(us[y])) / med[y], 4))


def newton(N, kind, a, w, sh, F, U, n_cycles, reps, run_only=False):
    opts = dict(rtol=0.0, max_cycles=n_cycles)
    nw = mg.Solver(N, 1.0, coef=a, **opts)
    lin = mg.Solver(N, 1.0, coef=a, reaction=sh, **opts)
    info = {}

    def timed(f):
        mg.lib().mg_fill_zero(U.ptr, U.size)
        mg.sync()
        t0 = time.perf_counter()
        out = f()
        mg.sync()
        return 1e3 * (time.perf_counter() - t0), out

    runs = {"newton_iteration": lambda: nw.newton(F, U, kind=kind, kappa=KAPPA, weight=w, rtol=0.0, max_iters=1)[1],
            "reaction_solve": lambda: lin.solve(F, U)[1]}
    for f in runs.values():
        timed(f)   # warm-up of every shape (and the driver's allocations)
    ms = {k: [] for k in runs}
    for _ in range(0 if run_only else reps):
        for k, f in runs.items():
            t, info[k] = timed(f)
            ms[k].append(t)
    nw.close(), lin.close()
    if run_only:
        return None
    assert info["newton_iteration"]["inner_cycles"] == n_cycles == info["reaction_solve"]["cycles"]
    med = {k: statistics.median(v) for k, v in ms.items()}
    y = "reaction_solve"
    return dict(cycles=n_cycles, reps=reps, ms={k: spread(v) for k, v in ms.items()}, trials=info["newton_iteration"]["trials"],
                newton_over_solve=round(med["newton_iteration"] / med[y], 4), newton_minus_solve_ms=round(med["newton_iteration"] - med[y], 4),
                yardstick_spread=round((max(ms[y]) - min(ms[y])) / med[y], 4))


def summarize(path, N):
    """path: a rocprofv3 kernel_trace.csv: the pass's kernels and the yardstick, the launches with the largest grid of each"""
    by = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "k_newton_residual" not in name and "k_residual_rx" not in name:
                continue
            grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0) * int(r.get("Grid_Size_Y") or 1)
            by.setdefault(name, []).append((grid, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    print(f"{'kernel':<72} {'launches':>8} {'median us':>10} {'min us':>8} {'max us':>8}   (N={N}, the largest grid of each)")
    for name, v in sorted(by.items()):
        g = max(x for x, _ in v)
        t = sorted(us for x, us in v if x == g)
        short = name.replace("mg::k::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(f"{short:<72} {len(t):>8} {statistics.median(t):>10.1f} {t[0]:>8.1f} {t[-1]:>8.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--cycles", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kind", default="sinh", choices=sorted(mg.NEWTON_KINDS))
    ap.add_argument("--kernels", action="store_true", help="one launch of every shape alone, for a profiler run")
    ap.add_argument("--summarize", help="a rocprofv3 kernel_trace.csv")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton_bench_line.json"))
    o = ap.parse_args()
    if o.summarize:
        return summarize(o.summarize, o.N)
    N = o.N
    mg.init(0)
    ah, wh = fields(N)
    a, w = mg.DeviceGrid.from_host(ah), mg.DeviceGrid.from_host(wh)
    sh = mg.DeviceGrid.from_host(KAPPA * wh)   # the reaction of the yardstick solve: kappa*w*cosh(0)
    del ah, wh
    F = mg.getSource(N, 1.0)
    U, dlt, V, D, S = (mg.DeviceGrid.zeros((N, N)) for _ in range(5))
    k = kernels(N, o.kind, a, w, U, dlt, F, V, D, S, 1 if o.kernels else o.reps)
    if o.kernels:
        mg.finalize()
        return
    for g in (dlt, V, D, S):
        g.free()
    res = dict(metric="newton", N=N, kind=o.kind, kappa=KAPPA, field_a="1 + 0.5 sin(2 pi x) cos(2 pi y)",
               field_w="1 + 0.5 sin(2 pi y) cos(2 pi x)", kernels=k, newton=newton(N, o.kind, a, w, sh, F, U, o.cycles, o.reps))
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(line + "\n")
    mg.finalize()


if __name__ == "__main__":
    main()
