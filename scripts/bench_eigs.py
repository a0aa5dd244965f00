"""The eigen-solver (include/mg_eigs.h), measured in one process.

  solves    N = 1025 and 8192, a == 1 and a = 1 + 0.5 sin(2 pi x) cos(2 pi y), (k, guard) = (4, 2) and (8, 4), rtol 1e-8 from
            a random start: the iterations, the total time (host clock around the synchronous call) and the time per iteration
            split into cycle, operator, Gram, rotation (the engine's event pairs, mg_profile_begin / mg_profile_end, summed
            over a solve and divided by its iterations) and the host Rayleigh-Ritz step (mg_eigsRayleighRitz timed on the host
            on matrices of the full basis size 3p): each a median over --reps solves with [min, max].
  kernels   N = 8192: k_eig_gram (m = 12, 24, 36; compulsory 16m bytes per point) and k_eig_rotate (m = 3p = 12, 24, 36;
            16m + 40p) through their test hooks, beside the two yardsticks of the parent in the same process and alternating
            with them: k_krylov_orth (k = 8: 168 B per point) and k_residual_vc (32 B per point).  Each launch timed by the
            engine's event pair; medians over --kernel-reps with [min, max], TB/s of compulsory bytes, the ratios to both
            yardsticks and the yardsticks' own run-to-run spread.  The Gram and rotation figures include their one-block
            finish launch.

Prints one JSON line and writes it to --out (default profiles/eigs_bench_line.json); the kernel table goes to --stats
(default profiles/eigs_kernel_stats.txt)."""
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


def smooth_field(N):
    x = np.arange(N) / float(N - 1)
    return 1.0 + 0.5 * np.sin(2 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]


def spread(v, digits=4):
    return dict(median=round(statistics.median(v), digits), min=round(min(v), digits), max=round(max(v), digits))


def host_step_ms(p, reps):
    m = 3 * p
    rng = np.random.default_rng(p)
    S = rng.random((400, m)) - 0.5
    B = rng.random((400, 400)) - 0.5
    G, H = S.T @ S, S.T @ (B @ B.T + 400.0 * np.eye(400)) @ S
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        mg.eigsRayleighRitz(G, H, p)
        out.append(1e3 * (time.perf_counter() - t))
    return out


def solves(N, coef, k, guard, reps):
    X = [mg.DeviceGrid((N, N)) for _ in range(k)]
    e = mg.EigenSolver(N, 1.0, k=k, guard=guard, coef=coef, rtol=RTOL)
    ptrs = [x.ptr for x in X]
    e.solve_ptrs(ptrs, False, 1)   # warm-up
    parts = {name: [] for name in ("eig_cycle", "eig_apply", "eig_gram", "eig_rotate", "eig_resnorm")}
    total, iters, conv = [], [], []
    for r in range(reps):
        mg.sync()
        mg.profile_begin(0)
        t = time.perf_counter()
        lam, info = e.solve_ptrs(ptrs, False, 1)
        total.append(1e3 * (time.perf_counter() - t))
        prof = mg.profile_end(4096)
        it = max(info["iters"], 1)
        for name in parts:
            parts[name].append(sum(x["total_ms"] for x in prof if x["name"] == name) / it)
        iters.append(info["iters"])
        conv.append(bool(info["converged"]))
    e.close()
    for x in X:
        x.free()
    host = host_step_ms(k + guard, reps)
    return dict(N=N, k=k, guard=guard, coef="one" if coef is None else "smooth", iters=iters[-1], converged=all(conv),
                lam=[float(v) for v in lam], total_ms=spread(total, 2),
                per_iteration_ms=dict(cycle=spread(parts["eig_cycle"]), operator=spread(parts["eig_apply"]), gram=spread(parts["eig_gram"]),
                                      rotation=spread(parts["eig_rotate"]), resnorm=spread(parts["eig_resnorm"]), host_step=spread(host)))


def kernels(N, reps, stats_path):
    fields = [mg.DeviceGrid.uniform((N, N), 100 + i) for i in range(72)]
    S, AS = fields[:36], fields[36:]
    a = mg.DeviceGrid.uniform((N, N), 999)          # uniform [0, 1): fine for a residual launch, which checks nothing
    b = np.full(8, 1e-3)
    rng = np.random.default_rng(0)
    cases = {}
    for m in (12, 24, 36):
        cases[f"eig_gram m={m}"] = ("eig_gram", 16 * m, lambda m=m: mg.eigsGram(N, S[:m], AS[:m]))
    for m in (12, 24, 36):
        p = m // 3
        C_ = 1e-3 * (rng.random((m, p)) - 0.5)
        theta = np.ones(p)
        cases[f"eig_rotate m={m} p={p}"] = ("eig_rotate", 16 * m + 40 * p,
                                            lambda m=m, p=p, C_=C_, theta=theta: mg.eigsRotate(N, C_, C_, theta, S[:3 * p], AS[:3 * p], AS[p:2 * p]))
    cases["krylov_orth k=8"] = ("krylov_orth", 40 + 16 * 8, lambda: mg.krylovOrth(N, b, fields[0], fields[1], fields[2], fields[3:11], fields[11:19]))
    cases["residual_vc"] = ("residual_vc", 32, lambda: mg.residualCoefficient(N, 1.0, 0.0, a, fields[0], fields[1], fields[2]))
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
    for g in fields + [a]:
        g.free()
    med = {name: statistics.median(v) for name, v in us.items()}
    tbs = {name: cases[name][1] * N * N / (med[name] * 1e-6) / 1e12 for name in cases}
    yard = ("krylov_orth k=8", "residual_vc")
    out = dict(N=N, reps=reps, us={n: spread(v, 1) for n, v in us.items()}, bytes_per_point={n: cases[n][1] for n in cases},
               TB_per_s={n: round(v, 3) for n, v in tbs.items()},
               ratio_to={y: {n: round(tbs[n] / tbs[y], 3) for n in cases if n not in yard} for y in yard},
               yardstick_spread={y: round((max(us[y]) - min(us[y])) / med[y], 4) for y in yard})
    with open(stats_path, "w") as f:
        f.write(f"N = {N}, {reps} repetitions alternating in one process; us: median [min, max]; TB/s of compulsory bytes\n")
        f.write(f"{'kernel':28s} {'B/point':>8s} {'us':>30s} {'TB/s':>7s} {'/krylov_orth':>13s} {'/residual_vc':>13s}\n")
        for n in cases:
            s = out["us"][n]
            f.write(f"{n:28s} {cases[n][1]:8d} {s['median']:12.1f} [{s['min']:.1f}, {s['max']:.1f}] {tbs[n]:7.3f} "
                    f"{tbs[n] / tbs[yard[0]]:13.3f} {tbs[n] / tbs[yard[1]]:13.3f}\n")
        f.write(f"yardsticks' own spread (max - min)/median: {out['yardstick_spread']}\n")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1025, 8192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-N", type=int, default=8192)
    ap.add_argument("--kernel-reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eigs_bench_line.json"))
    ap.add_argument("--stats", default=os.path.join(ROOT, "profiles", "eigs_kernel_stats.txt"))
    o = ap.parse_args()
    mg.init(0)
    for path in (o.out, o.stats):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    out = dict(metric="eigs", rtol=RTOL, field="1 + 0.5 sin(2 pi x) cos(2 pi y)", solves=[])
    out["kernels"] = kernels(o.kernel_N, o.kernel_reps, o.stats)
    mg.lib().mg_pool_trim()
    for N in o.sizes:
        for coef in (None, smooth_field(N)):
            for k, guard in ((4, 2), (8, 4)):
                out["solves"].append(solves(N, coef, k, guard, o.reps))
                print(json.dumps(out["solves"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line, flush=True)
    with open(o.out, "w") as f:
        f.write(line + "\n")
    mg.finalize()


if __name__ == "__main__":
    main()
