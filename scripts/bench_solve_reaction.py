"""The reaction term (include/mg_reaction.h) against the variable-coefficient kernels it is layered over, in ONE process,
alternating, medians over --reps with min and max: N = 8192, V(3,3), omega = 0.8.
  kernels   the level-0 sweep, timed by the engine's own event pairs (mg_profile_begin / mg_profile_end):
              wjacobi_rx_a   with s and a        40 B per point (U, a, s, F in, U out)
              wjacobi_rx     with s, without a   32 B per point (U, s, F in, U out): no array of ones is streamed
              wjacobi_vc     k_wjacobi_vc on the same a, the yardstick: 32 B per point
            byte models 40/32 and 32/32 -- models, not thresholds.  yardstick_spread is (max - min)/median of the yardstick's
            own repetitions: a ratio further from its model than that is an open item.
  cycles    ms per cycle (the solver's hipEvent time over --cycles cycles at rtol = 0, the two start norms inside for both) of
            Solver(coef=a, reaction=s) against Solver(coef=a, shift=sigma), the getSource problem from U = 0.
Prints one JSON line and writes it to --out (default profiles/solve_reaction_bench_line.json).

Per-kernel times come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_solve_reaction.py --kernels
    python scripts/bench_solve_reaction.py --summarize DIR/.../*_kernel_trace.csv > profiles/solve_reaction_kernel_stats.txt"""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multigrid_poisson_solver_amd as mg  # noqa: E402

HBM_PEAK = 8.0e12
SIGMA = 1.0e4
# bytes per point by kernel name; k_wjacobi_rx<ZERO_IN, PAIR, NT, HAS_A>, k_residual_rx<PAIR, HAS_A>, k_resnorm_rx<PAIR, NT, HAS_A>
BYTES_PER_POINT = {"k_wjacobi_rx<false, true, true, true>": 40, "k_wjacobi_rx<false, true, true, false>": 32,
                   "k_wjacobi_rx<true, true, true, true>": 32, "k_wjacobi_rx<true, true, true, false>": 24,
                   "k_residual_rx<true, true>": 40, "k_residual_rx<true, false>": 32,
                   "k_resnorm_rx<true, true, true>": 32, "k_resnorm_rx<true, true, false>": 24,
                   "k_wjacobi_vc<false": 32, "k_wjacobi_vc<true": 24, "k_residual_vc": 32, "k_resnorm_vc": 24}


def fields(N):
    x = np.arange(N) / float(N - 1)
    w = np.sin(2 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]
    return 1.0 + 0.5 * w, SIGMA * (1.0 + w)   # a, and s with mean sigma (the smooth field of the tests)


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def kernels(N, a, s, U, F, out, reps):
    calls = {"wjacobi_rx_a": lambda: mg.sweepReaction(N, 1.0, 0.0, 0.8, a, s, U, F, out),
             "wjacobi_rx": lambda: mg.sweepReaction(N, 1.0, 0.0, 0.8, None, s, U, F, out),
             "wjacobi_vc": lambda: mg.sweepCoefficient(N, 1.0, SIGMA, 0.8, a, U, F, out)}
    bytes_per_point = {"wjacobi_rx_a": 40, "wjacobi_rx": 32, "wjacobi_vc": 32}
    for f in calls.values():
        f()   # warm-up of every shape
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
                share_of_hbm_peak={k: round(bytes_per_point[k] * N * N / (med[k] * 1e-6) / HBM_PEAK, 3) for k in calls},
                rx_a_over_vc=round(med["wjacobi_rx_a"] / med["wjacobi_vc"], 4), rx_a_bytes_model=round(40 / 32, 4),
                rx_over_vc=round(med["wjacobi_rx"] / med["wjacobi_vc"], 4), rx_bytes_model=1.0,
                yardstick_spread=round((max(us["wjacobi_vc"]) - min(us["wjacobi_vc"])) / med["wjacobi_vc"], 4))


def cycles(N, a, s, F, U, n_cycles, reps, run_only=False):
    opts = dict(rtol=0.0, max_cycles=n_cycles)
    solvers = {"reaction": mg.Solver(N, 1.0, coef=a, reaction=s, **opts), "shift": mg.Solver(N, 1.0, coef=a, shift=SIGMA, **opts)}

    def run(name):
        mg.lib().mg_fill_zero(U.ptr, U.size)
        info = solvers[name].solve(F, U)[1]
        assert info["cycles"] == n_cycles
        return info["device_ms"] / n_cycles, info["res"] / info["ref_norm"]

    for name in solvers:
        run(name)   # warm-up of every shape
    ms, res = {k: [] for k in solvers}, {}
    for _ in range(0 if run_only else reps):
        for name in solvers:
            t, res[name] = run(name)
            ms[name].append(t)
    for sv in solvers.values():
        sv.close()
    if run_only:
        return None
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(cycles=n_cycles, reps=reps, sigma=SIGMA, ms_per_cycle={k: spread(v) for k, v in ms.items()},
                reaction_over_shift=round(med["reaction"] / med["shift"], 4),
                yardstick_spread=round((max(ms["shift"]) - min(ms["shift"])) / med["shift"], 4), res_over_ref=res)


def summarize(path, N):
    """path: a rocprofv3 kernel_trace.csv.  Per kernel the launches with the largest grid are taken: for the forms that run on
    the finest level these are the level-0 launches, whose median time gives the share of the HBM peak; the forms that only
    run on coarser levels are listed with their count and median time alone."""
    by = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            key = next((k for k in BYTES_PER_POINT if k in name), None)
            if key is None:
                continue
            grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0) * int(r.get("Grid_Size_Y") or 1)
            by.setdefault((name, key), []).append((grid, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    print(f"{'kernel':<64} {'launches':>8} {'level 0':>8} {'median us':>10} {'min us':>8} {'max us':>8} {'B/pt':>5} "
          f"share of {HBM_PEAK / 1e12:.0f} TB/s at N={N}")
    top = max(g for v in by.values() for g, _ in v)   # (the level-0 launches of the 16-byte forms)
    for (name, key), v in sorted(by.items()):
        g = max(x for x, _ in v)
        t = sorted(us for x, us in v if x == g)
        med = statistics.median(t)
        share = f"{BYTES_PER_POINT[key] * N * N / (med * 1e-6) / HBM_PEAK:8.3f}" if g == top else "   (coarser levels only)"
        short = name.replace("mg::k::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(f"{short:<64} {len(v):>8} {len(t):>8} {med:>10.1f} {t[0]:>8.1f} {t[-1]:>8.1f} {BYTES_PER_POINT[key]:>5} {share}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--cycles", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels", action="store_true", help="the warm-up launches of every shape alone, for a profiler run")
    ap.add_argument("--summarize", help="a rocprofv3 kernel_trace.csv")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_reaction_bench_line.json"))
    o = ap.parse_args()
    if o.summarize:
        return summarize(o.summarize, o.N)
    N = o.N
    mg.init(0)
    ah, sh = fields(N)
    a, s = mg.DeviceGrid.from_host(ah), mg.DeviceGrid.from_host(sh)
    del ah, sh
    F = mg.getSource(N, 1.0)
    U, out = mg.DeviceGrid.zeros((N, N)), mg.DeviceGrid((N, N))
    if o.kernels:
        cycles(N, a, s, F, U, o.cycles, 0, run_only=True)
        mg.finalize()
        return
    res = dict(metric="solve_reaction", N=N, pre=3, post=3, omega=0.8, field_a="1 + 0.5 sin(2 pi x) cos(2 pi y)",
               field_s="1e4 (1 + sin(2 pi x) cos(2 pi y))", kernels=kernels(N, a, s, U, F, out, o.reps),
               solve=cycles(N, a, s, F, U, o.cycles, o.reps))
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(line + "\n")
    mg.finalize()


if __name__ == "__main__":
    main()
