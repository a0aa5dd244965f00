"""The pure Neumann problem (include/mg_singular.h), measured in one process at N = 8192, V(3,3), omega = 0.8,
a = 1 + 0.5 sin(2 pi x) cos(2 pi y), the getSource problem from U = 0:

  cycle     ms per cycle of the singular solve (nnnn, sigma = 0, mean 0) against nnnd at sigma = 0 on the same arrays,
            alternating: per repetition (T(k = 10) - T(k = 2)) / 8 from the solver's hipEvent time at rtol = 0, which leaves the
            start norms, the projection and the shift out.  The two cycles differ by the coarse kernel's prologue only; the
            ratio is reported with the [min, max] of the per-repetition ratios beside the nnnd leg's own spread.
  one-off   T(k = 0) of the singular solve minus T(k = 0) of nnnd: the projection of F and the shift of U (two weighted sums,
            two shifts), as ms and as a fraction of a whole singular solve to rtol 1e-9 (with the relative residual it reached
            and the one after cycles 10, 20 and 30: at this size the fp64 rounding floor may lie above 1e-9).
  kernels   the weighted sum (8 B per point, its finish launch included) and the shift (16 B per point) through mg_weightedMean
            / mg_projectMean, beside the residual norm of the boundary path (24 B per point with a coefficient) and
            k_krylov_update (48 B per point) in the same process, alternating; each timed by the engine's event pair, medians
            over --kernel-reps with [min, max], TB/s of the byte model.
  cycles    cycles to rtol 1e-9 at N = 257 and 1025, random F (not compatible) and start, a == 1 and the smooth field.

Prints one JSON line and writes it to --out (default profiles/solve_singular_bench_line.json); the kernel table goes to --stats
(default profiles/solve_singular_kernel_stats.txt)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multigrid_poisson_solver_amd as mg  # noqa: E402


def smooth_field(N):
    x = np.arange(N) / float(N - 1)
    return 1.0 + 0.5 * np.sin(2 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]


def spread(v, digits=4):
    return dict(median=round(statistics.median(v), digits), min=round(min(v), digits), max=round(max(v), digits))


def cycles_table():
    out = {}
    for N in (257, 1025):
        rng = np.random.default_rng(500 + N)
        F, U0 = rng.random((N, N)) - 0.5, rng.random((N, N)) - 0.5
        for name, a in (("one", None), ("smooth", smooth_field(N))):
            _, info = mg.solve(F, U0, 1.0, coef=a, bc="nnnn", mean=0.0, rtol=1e-9)
            out[f"N{N}_{name}"] = [info["cycles"], bool(info["converged"]), bool(info["coarse_capped"])]
    return out


def solves(N, reps):
    F = mg.getSource(N, 1.0)
    U = mg.DeviceGrid.zeros((N, N))
    a = mg.DeviceGrid.from_host(smooth_field(N))
    legs = {"nnnn": dict(bc="nnnn", mean=0.0), "nnnd": dict(bc="nnnd")}

    times = {leg: {k: [] for k in (0, 2, 10)} for leg in legs}
    whole = []
    made = {(leg, k): mg.Solver(N, 1.0, coef=a, rtol=0.0, max_cycles=k, **kw) for leg, kw in legs.items() for k in (0, 2, 10)}
    full = mg.Solver(N, 1.0, coef=a, rtol=1e-9, max_cycles=50, bc="nnnn", mean=0.0)

    def timed(s):
        mg.lib().mg_fill_zero(U.ptr, U.size)
        return s.solve(F, U)[1]

    for s in list(made.values()) + [full]:
        timed(s)   # warm-up of every shape
    info = None
    for _ in range(reps):
        for k in (0, 2, 10):
            for leg in legs:
                times[leg][k].append(timed(made[(leg, k)])["device_ms"])
        info = timed(full)
        whole.append(info["device_ms"])
    per_cycle = {leg: [(t10 - t2) / 8.0 for t10, t2 in zip(times[leg][10], times[leg][2])] for leg in legs}
    ratio = [x / y for x, y in zip(per_cycle["nnnn"], per_cycle["nnnd"])]
    one_off = [x - y for x, y in zip(times["nnnn"][0], times["nnnd"][0])]
    med_d = statistics.median(per_cycle["nnnd"])
    out = dict(N=N, reps=reps, pre=3, post=3, omega=0.8, coef="smooth",
               ms_per_cycle={leg: spread(v) for leg, v in per_cycle.items()},
               singular_over_nnnd=spread(ratio),
               nnnd_own_spread=[round(min(per_cycle["nnnd"]) / med_d, 4), round(max(per_cycle["nnnd"]) / med_d, 4)],
               one_off_ms=spread(one_off),
               whole_solve=dict(rtol=1e-9, ms=spread(whole, 2), cycles=info["cycles"], converged=bool(info["converged"]),
                                res_over_ref=info["res"] / info["ref_norm"],
                                res_over_ref_after_cycle=[round(h / info["ref_norm"], 14) for h in info["history"][10:31:10]],
                                compat_defect=info["compat_defect"], mean_before=info["mean_before"]),
               one_off_fraction_of_whole_solve=round(statistics.median(one_off) / statistics.median(whole), 5))
    for s in list(made.values()) + [full]:
        s.close()
    for g in (U, a):
        g.free()
    return out


def kernels(N, reps, stats_path):
    X, Y, Z, R = (mg.DeviceGrid.uniform((N, N), 100 + i) for i in range(4))
    a = mg.DeviceGrid.from_host(smooth_field(N))
    norm_solver = mg.Solver(N, 1.0, coef=a, bc="nnnd", rtol=0.0, max_cycles=0)
    cases = {
        "wsum": ("wsum", 8, lambda: mg.weighted_mean(X)),
        "shift": ("shift", 16, lambda: mg.project_mean(X, 0.0, out=Y)),
        "resnorm_bc": ("resnorm", 24, lambda: norm_solver.solve(X, Y)),
        "krylov_update": ("krylov_update", 48, lambda: mg.krylovUpdate(N, 1e-3, X, Y, Z, R)),
    }
    for _, _, f in cases.values():
        f()
    us = {name: [] for name in cases}
    for _ in range(reps):
        for name, (prof_name, bpp, f) in cases.items():
            mg.profile_begin(0)
            f()
            got = [x for x in mg.profile_end() if x["name"] == prof_name]
            assert len(got) == 1 and got[0]["launches"] == 1 and got[0]["algo_bytes"] == float(bpp) * N * N, (name, got)
            us[name].append(1e3 * got[0]["total_ms"])
    norm_solver.close()
    for g in (X, Y, Z, R, a):
        g.free()
    med = {name: statistics.median(v) for name, v in us.items()}
    tbs = {name: cases[name][1] * N * N / (med[name] * 1e-6) / 1e12 for name in cases}
    yard = ("resnorm_bc", "krylov_update")
    out = dict(N=N, reps=reps, us={n: spread(v, 1) for n, v in us.items()}, bytes_per_point={n: cases[n][1] for n in cases},
               TB_per_s={n: round(v, 3) for n, v in tbs.items()},
               ratio_to={y: {n: round(tbs[n] / tbs[y], 3) for n in cases if n not in yard} for y in yard},
               yardstick_spread={y: round((max(us[y]) - min(us[y])) / med[y], 4) for y in yard})
    with open(stats_path, "w") as f:
        f.write(f"N = {N}, {reps} repetitions alternating in one process; us: median [min, max]; TB/s of the byte model\n")
        f.write(f"{'kernel':16s} {'B/point':>8s} {'us':>30s} {'TB/s':>7s} {'/resnorm_bc':>12s} {'/krylov_update':>15s}\n")
        for n in cases:
            s = out["us"][n]
            f.write(f"{n:16s} {cases[n][1]:8d} {s['median']:12.1f} [{s['min']:.1f}, {s['max']:.1f}] {tbs[n]:7.3f} "
                    f"{tbs[n] / tbs[yard[0]]:12.3f} {tbs[n] / tbs[yard[1]]:15.3f}\n")
        f.write("wsum includes its one-block finish launch; resnorm_bc is the norm launch pair of a solve with a coefficient\n")
        f.write(f"yardsticks' own spread (max - min)/median: {out['yardstick_spread']}\n")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_singular_bench_line.json"))
    ap.add_argument("--stats", default=os.path.join(ROOT, "profiles", "solve_singular_kernel_stats.txt"))
    a = ap.parse_args()
    mg.init(0)
    out = dict(metric="solve_singular", solves=solves(a.N, a.reps), kernels=kernels(a.N, a.kernel_reps, a.stats),
               cycles_to_1e_9=cycles_table())
    mg.finalize()
    line = json.dumps(out)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
