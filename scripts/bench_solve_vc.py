"""The variable-coefficient solve (include/mg_varcoef.h) against the constant-coefficient solver, in one process, alternating,
medians over --reps: N = 8192, V(3,3), omega = 0.8, the getSource problem from U = 0, --cycles cycles each (rtol = 0):
    vc_smooth   the coefficient a = 1 + 0.5 sin(2 pi x) cos(2 pi y)
    vc_one      a == 1 (the same kernels, the constant solver's bits)
    simple      the constant solver under mg_set_smoother("simple"): operator by operator, the like-for-like yardstick
    fused       the constant solver's default cycle (fused streaming nodes)
Reports ms per cycle (the solver's hipEvent time over the cycles; the two start norms are inside it for every variant alike)
and the ratios.  From bytes alone a variable sweep moves 32 B per point against 24: about 4/3 of `simple`'s sweep time -- a
model, not a threshold.  Prints one JSON line.

Per-kernel times come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_solve_vc.py --kernels
    python scripts/bench_solve_vc.py --summarize DIR/.../*_kernel_trace.csv
which prints, per kernel of the operator-by-operator cycles, the launches, the median time of the level-0 launches and their
algorithmic bytes (sweep 32 B, zero-start sweep 24 B, residual 32 B, norm 24 B per point; constant: 24 / 24 / 16, the norm of F alone 8) over that
time as a share of the 8 TB/s HBM peak."""
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
BYTES_PER_POINT = {"k_wjacobi_vc<false": 32, "k_wjacobi_vc<true": 24, "k_residual_vc": 32, "k_resnorm_vc": 24,
                   "k_wjacobi_pairs": 24, "k_wjacobi<": 24, "k_residual_pairs": 24, "k_resnorm_pairs<false": 8, "k_resnorm_pairs": 16}


def smooth_field(N):
    x = np.arange(N) / float(N - 1)
    return 1.0 + 0.5 * np.sin(2 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]


def summarize(path, N):
    """path: a rocprofv3 kernel_trace.csv.  Per kernel the launches with the largest grid are taken: for the forms that run on
    the finest level these are the level-0 launches (N x N points), whose median time gives the share of peak; the forms that
    only run on coarser levels are listed with their count and median time alone."""
    by = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            key = next((k for k in BYTES_PER_POINT if k in name), None)
            if key is None:
                continue
            grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0) * int(r.get("Grid_Size_Y") or 1)
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            by.setdefault((name, key), []).append((grid, us))
    top = max(g for v in by.values() for g, _ in v)   # (the level-0 launches of the 16-byte forms)
    print(f"{'kernel':<72} {'launches':>8} {'largest':>8} {'median us':>10} {'min us':>8} {'B/pt':>5} {'share of %.0f TB/s at N=%d' % (HBM_PEAK / 1e12, N)}")
    for (name, key), v in sorted(by.items()):
        g = max(x for x, _ in v)
        t = sorted(us for x, us in v if x == g)
        med = statistics.median(t)
        share = f"{BYTES_PER_POINT[key] * N * N / (med * 1e-6) / HBM_PEAK:8.3f}" if g == top else "   (coarser levels only)"
        short = name.replace("mg::k::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(f"{short:<72} {len(v):>8} {len(t):>8} {med:>10.1f} {t[0]:>8.1f} {BYTES_PER_POINT[key]:>5} {share}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--cycles", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels", action="store_true", help="one solve per variant, for a profiler run")
    ap.add_argument("--summarize", help="a rocprofv3 kernel_trace.csv")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.N)
    N = a.N
    mg.init(0)
    F = mg.getSource(N, 1.0)
    U = mg.DeviceGrid.zeros((N, N))
    opts = dict(rtol=0.0, max_cycles=a.cycles)
    coefs = {"vc_smooth": mg.DeviceGrid.from_host(smooth_field(N)), "vc_one": mg.DeviceGrid.from_host(np.ones((N, N)))}
    solvers = {name: mg.Solver(N, 1.0, coef=c, **opts) for name, c in coefs.items()}
    solvers["simple"] = solvers["fused"] = mg.Solver(N, 1.0, **opts)

    def run(name):
        mg.lib().mg_fill_zero(U.ptr, U.size)
        mg.set_smoother("simple" if name == "simple" else "stream")
        try:
            info = solvers[name].solve(F, U)[1]
        finally:
            mg.set_smoother("stream")
        assert info["cycles"] == a.cycles
        return info["device_ms"] / a.cycles, info["res"]

    order = ["vc_smooth", "vc_one", "simple", "fused"]
    for name in order:
        run(name)   # warm-up of every shape
    if a.kernels:
        mg.finalize()
        return
    ms = {name: [] for name in order}
    res = {}
    for _ in range(a.reps):
        for name in order:
            t, res[name] = run(name)
            ms[name].append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(metric="solve_vc_ms_per_cycle", N=N, cycles=a.cycles, reps=a.reps, pre=3, post=3, omega=0.8,
               ms_per_cycle={k: round(v, 4) for k, v in med.items()},
               spread={k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
               vc_smooth_over_simple=round(med["vc_smooth"] / med["simple"], 4),
               vc_one_over_simple=round(med["vc_one"] / med["simple"], 4),
               vc_smooth_over_fused=round(med["vc_smooth"] / med["fused"], 4),
               bytes_model_sweep_ratio=round(32 / 24, 4),
               unit_coefficient_bits_equal=res["vc_one"] == res["simple"] == res["fused"], res=res)
    print(json.dumps(out), flush=True)
    mg.finalize()


if __name__ == "__main__":
    main()
