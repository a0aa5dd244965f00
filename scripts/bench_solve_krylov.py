"""The Krylov acceleration (include/mg_krylov.h, Solver(krylov=m)) against the plain cycle iteration, in one process,
alternating, medians over --reps: N = 8192, V(3,3), omega = 0.8, the getSource problem from U = 0, with the coefficient
a = 1 + 0.5 sin(2 pi x) cos(2 pi y) (`smooth`) and without one (`const`, the fused cycle).

  per iteration   --iters iterations of GCR(m) (rtol = 0: k runs 0 .. m-1, then a restart) against as many plain cycles: the
                  solver's hipEvent time over the count.  From bytes alone an iteration adds 120 + 24k B per point to the
                  cycle and saves the plain loop's norm launch -- a model, not a threshold.
  to tolerance    both to rtol = 1e-9 and to rtol = 1e-8: iterations / cycles, total device time and the relative residual
                  reached.  At N = 8192 the fp64 rounding floor of the residual lies at about 1e-9 of ||F||, so
                  the first target measures the floor as much as the method; the second lies clear of it.
  jump            the same with a 10x jump of the coefficient across x = 0.37, the case the plain cycle is slow on.
  kernels         each new kernel alone at N (the test hooks; k = 0, 3, 7) under the engine's own event timing
                  (mg_profile_begin / mg_profile_end around every single call), alternating with the yardstick, the residual
                  kernel of the variable-coefficient cycle (32 B per point): algorithmic bytes over time, median and
                  min .. max.  The dots figure includes its finish launch (k blocks), the others do not.

Prints one JSON line; --stats FILE also writes the kernel table as text."""
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


def jump_field(N):
    x = np.arange(N) / float(N - 1)
    return np.where(x < 0.37, 1.0, 10.0)[None, :] + np.zeros((N, 1))


def timed(name, call):
    """(ms, algorithmic bytes) of the launches `call` enqueues under the profile scope `name`"""
    mg.profile_begin(0)
    try:
        call()
    finally:
        prof = mg.profile_end(64)
    hit = [p for p in prof if p["name"] == name]
    assert len(hit) == 1 and hit[0]["launches"] == 1, prof
    return hit[0]["total_ms"], hit[0]["algo_bytes"]


def kernel_table(N, reps, ks):
    vec = [mg.DeviceGrid.uniform((N, N), 100 + i) for i in range(4 + 2 * max(ks))]
    q, z, r, U = vec[:4]
    rest = vec[4:]
    a = mg.DeviceGrid.from_host(smooth_field(N))
    cases = [("residual_vc (yardstick)", "residual_vc", lambda: mg.residualCoefficient(N, 1.0, 0.0, a, U, r, z))]
    for k in ks:
        Q, Z = rest[:k], rest[max(ks):max(ks) + k]
        b = np.full(k, 1e-3)
        if k > 0:
            cases.append((f"krylov_dots k={k}", "krylov_dots", lambda Q=Q: mg.krylovDots(N, q, Q)))
        cases.append((f"krylov_orth k={k}", "krylov_orth", lambda Q=Q, Z=Z, b=b: mg.krylovOrth(N, b, q, z, r, Q, Z)))
    cases.append(("krylov_update", "krylov_update", lambda: mg.krylovUpdate(N, 1e-3, U, z, r, q)))
    for _, name, call in cases:
        timed(name, call)   # warm-up of every shape
    ms = {label: [] for label, _, _ in cases}
    nbytes = {}
    for _ in range(reps):
        for label, name, call in cases:
            t, nbytes[label] = timed(name, call)
            ms[label].append(t)
    rows = []
    for label, _, _ in cases:
        t = sorted(ms[label])
        rate = lambda v: nbytes[label] / (v * 1e-3) / 1e12   # noqa: E731
        rows.append(dict(kernel=label, bytes_per_point=round(nbytes[label] / (N * N), 1), ms_median=round(statistics.median(t), 4),
                         ms_min=round(t[0], 4), ms_max=round(t[-1], 4), tb_s_median=round(rate(statistics.median(t)), 3),
                         tb_s_min=round(rate(t[-1]), 3), tb_s_max=round(rate(t[0]), 3)))
    for g in vec + [a]:
        g.free()
    return rows


def table_text(N, rows):
    lines = [f"N = {N}: algorithmic bytes over the engine's event time, one call per measurement, alternating",
             f"{'kernel':<26} {'B/pt':>6} {'ms median':>10} {'ms min':>8} {'ms max':>8} {'TB/s median':>12} {'TB/s min':>9} {'TB/s max':>9}"]
    for r in rows:
        lines.append(f"{r['kernel']:<26} {r['bytes_per_point']:>6} {r['ms_median']:>10} {r['ms_min']:>8} {r['ms_max']:>8} "
                     f"{r['tb_s_median']:>12} {r['tb_s_min']:>9} {r['tb_s_max']:>9}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--m", type=int, default=8)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=9)
    ap.add_argument("--stats", help="write the kernel table to this file")
    a = ap.parse_args()
    N, m = a.N, a.m
    mg.init(0)
    rows = kernel_table(N, a.kernel_reps, (0, 3, 7))
    if a.stats:
        with open(a.stats, "w") as f:
            f.write(table_text(N, rows))
    F = mg.getSource(N, 1.0)
    U = mg.DeviceGrid.zeros((N, N))
    coef = {"smooth": lambda: mg.DeviceGrid.from_host(smooth_field(N)), "const": lambda: None,
            "jump": lambda: mg.DeviceGrid.from_host(jump_field(N))}
    out = dict(metric="solve_krylov", N=N, m=m, iters=a.iters, reps=a.reps, pre=3, post=3, omega=0.8, kernels=rows)
    for name, make in coef.items():
        c = make()
        option_sets = {"fixed": dict(rtol=0.0, max_cycles=a.iters), "to_rtol_1e9": dict(rtol=1e-9, max_cycles=50),
                       "to_rtol_1e8": dict(rtol=1e-8, max_cycles=50)}
        # (the options live in the solver: one solver per variant and option set, all alive for the alternation)
        solvers = {(which, key): mg.Solver(N, 1.0, coef=c, krylov=m if which == "krylov" else 0, **opts)
                   for which in ("plain", "krylov") for key, opts in option_sets.items()}

        def run(which, key):
            mg.lib().mg_fill_zero(U.ptr, U.size)
            return solvers[(which, key)].solve(F, U)[1]

        for which in ("plain", "krylov"):
            run(which, "fixed")   # warm-up
        per = {"plain": [], "krylov": []}
        targets = [key for key in option_sets if key != "fixed"]
        tot = {key: {"plain": [], "krylov": []} for key in targets}
        last = {key: {} for key in targets}
        for _ in range(a.reps):
            for which in ("plain", "krylov"):
                info = run(which, "fixed")
                assert info["cycles"] == a.iters
                per[which].append(info["device_ms"] / a.iters)
                for key in targets:
                    info = run(which, key)
                    tot[key][which].append(info["device_ms"])
                    last[key][which] = info
        med = {k: statistics.median(v) for k, v in per.items()}
        out[name] = dict(ms_per_iteration={k: round(v, 4) for k, v in med.items()},
                         spread={k: [round(min(v), 4), round(max(v), 4)] for k, v in per.items()},
                         krylov_over_plain=round(med["krylov"] / med["plain"], 4))
        for key in targets:
            medt = {k: statistics.median(v) for k, v in tot[key].items()}
            out[name][key] = dict(iterations={k: v["cycles"] for k, v in last[key].items()},
                                  converged={k: v["converged"] for k, v in last[key].items()},
                                  relative_residual={k: float("%.4g" % (v["res"] / v["ref_norm"])) for k, v in last[key].items()},
                                  ms={k: round(v, 3) for k, v in medt.items()},
                                  krylov_over_plain=round(medt["krylov"] / medt["plain"], 4))
        for t in solvers.values():
            t.close()
        if c is not None:
            c.free()
    print(json.dumps(out), flush=True)
    mg.finalize()


if __name__ == "__main__":
    main()
