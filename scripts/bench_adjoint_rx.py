"""The adjoint of reaction and semilinear solves (include/mg_adjoint_rx.h), measured in one process with the variants alternating.

  kernels   N = 8192: per repetition one launch each of the source-gradient kernel (mg_sourceGradient) for every kind, without
            and with a weight, and of the coefficient-gradient kernel (mg_coefficientGradient) on the same lam and U -- the
            yardstick: 24 B per point like the source gradient without w (32 B with it), but through rolling three-row windows.
            Each timed by the engine's event pair around the launch (mg_profile_begin / mg_profile_end), the source gradient's
            with its finish launch inside.  Medians over --kernel-reps with the spread (min, max), TB/s of algorithmic bytes,
            the ratio to the yardstick beside the byte model (1.0, 32/24) and the yardstick's own run-to-run spread.
  driver    N = --driver-N, a = 1 + 0.5 sin(2 pi x) cos(2 pi y), w = a, sinh, kappa = 1, rtol 1e-8: Solver.newton_adjoint (pass,
            coarsening, zero fill, adjoint solve, three gradients) against the solve of the same right-hand side from zero on
            the same reaction alone -- one inner solve of a Newton iteration: host clock around work that ends in a device
            synchronise, medians over --reps.  Expected: 1 plus the pass, the coarsening and three array passes.
  batch     N = 257, B = 64, a coefficient per instance: BatchSolver.newton_adjoint_batch against 64 Solver.newton_adjoint calls.

Prints one JSON line and writes it to --out (default profiles/adjoint_rx_bench_line.json)."""
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
KINDS = ("cubic", "sinh", "exp", "linear")


def smooth_field(N, phase=0.0):
    x = np.arange(N) / float(N - 1)
    return 1.0 + 0.5 * np.sin(2 * np.pi * x + phase)[None, :] * np.cos(2 * np.pi * x)[:, None]


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def kernels(N, lam, U, w, out, reps):
    calls = {"coef_grad": ("coef_grad", 24, lambda: mg.coefficientGradient(N, 1.0, lam, U, out))}
    for kind in KINDS:
        calls[f"src_grad<{kind}>"] = ("src_grad", 24, lambda kind=kind: mg.sourceGradient(N, kind, 1.0, None, lam, U, out))
        calls[f"src_grad<{kind}, w>"] = ("src_grad_w", 32, lambda kind=kind: mg.sourceGradient(N, kind, 1.0, w, lam, U, out))
    for _, _, f in calls.values():
        f()
    us = {k: [] for k in calls}
    for _ in range(reps):
        for k, (name, bpp, f) in calls.items():
            mg.profile_begin(0)
            f()
            got = {e["name"]: e for e in mg.profile_end()}
            assert got[name]["launches"] == 1 and got[name]["algo_bytes"] == bpp * N * N, got[name]
            us[k].append(1e3 * got[name]["total_ms"])
    med = {k: statistics.median(v) for k, v in us.items()}
    return dict(reps=reps, us={k: spread(v) for k, v in us.items()}, bytes_per_point={k: c[1] for k, c in calls.items()},
                TB_per_s={k: round(calls[k][1] * N * N / (med[k] * 1e-6) / 1e12, 3) for k in calls},
                over_coef_grad={k: round(med[k] / med["coef_grad"], 4) for k in calls if k != "coef_grad"},
                byte_model={"without w": 1.0, "with w": round(32 / 24, 4)},
                coef_grad_spread=round((max(us["coef_grad"]) - min(us["coef_grad"])) / med["coef_grad"], 4))


def driver(N, reps):
    a_host = smooth_field(N)
    a, w = mg.DeviceGrid.from_host(a_host), mg.DeviceGrid.from_host(a_host)
    Ubar, U, F = (mg.DeviceGrid.uniform((N, N), seed + N) for seed in (11, 1234, 4321))
    lam, gA, gU, gW, D, S = (mg.DeviceGrid((N, N)) for _ in range(6))
    s = mg.Solver(N, 1.0, coef=a_host, rtol=RTOL)
    mg.nonlinear_residual(N, 1.0, 0.0, a, "sinh", 1.0, w, U, F, D, S)

    def adjoint():
        t = time.perf_counter()
        info = s.newton_adjoint(Ubar, U, F, kind="sinh", kappa=1.0, weight=w)[4]
        mg.sync()
        return 1e3 * (time.perf_counter() - t), info

    def solve():
        s.set_reaction(S)
        mg.lib().mg_fill_zero(lam.ptr, lam.size)
        mg.sync()
        t = time.perf_counter()
        info = s.solve_ptr(Ubar.ptr, lam.ptr)
        mg.sync()
        ms = 1e3 * (time.perf_counter() - t)
        s.set_reaction(None)
        return ms, info

    adjoint()
    solve()
    runs = {"newton_adjoint": [], "solve": []}
    for _ in range(reps):
        runs["newton_adjoint"].append(adjoint())
        runs["solve"].append(solve())
    s.close()
    for g in (a, w, Ubar, U, F, lam, gA, gU, gW, D, S):
        g.free()
    ms = {k: [t for t, _ in v] for k, v in runs.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(N=N, reps=reps, rtol=RTOL, ms={k: spread(v) for k, v in ms.items()}, cycles=runs["newton_adjoint"][-1][1]["cycles"],
                solve_cycles=runs["solve"][-1][1]["cycles"], converged=bool(runs["newton_adjoint"][-1][1]["converged"]),
                newton_adjoint_over_solve=round(med["newton_adjoint"] / med["solve"], 4))


def batch(N, B, reps):
    rng = np.random.default_rng(3)
    a = [smooth_field(N, 0.1 * i) for i in range(B)]
    grids = lambda: [mg.DeviceGrid.from_host(rng.standard_normal((N, N))) for _ in range(B)]
    Ubar, U, F = grids(), grids(), grids()
    b = mg.BatchSolver(N, 1.0, max_batch=B, rtol=RTOL)
    b.set_coefficient(a)
    singles = [mg.Solver(N, 1.0, coef=a[i], rtol=RTOL) for i in range(B)]

    def batched():
        t = time.perf_counter()
        infos = b.newton_adjoint_batch(Ubar, U, F, kind="sinh", kappa=1.0)[4]
        mg.sync()
        return 1e3 * (time.perf_counter() - t), infos[0]["stats"]

    def each():
        t = time.perf_counter()
        for i in range(B):
            singles[i].newton_adjoint(Ubar[i], U[i], F[i], kind="sinh", kappa=1.0)
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
    ap.add_argument("--driver-N", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--batch-N", type=int, default=257)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adjoint_rx_bench_line.json"))
    o = ap.parse_args()
    N = o.N
    mg.init(0)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    lam, U, w = (mg.DeviceGrid.uniform((N, N), seed + N) for seed in (11, 1234, 4321))
    G = mg.DeviceGrid((N, N))
    out = dict(metric="adjoint_rx", N=N)
    out["kernels"] = kernels(N, lam, U, w, G, o.kernel_reps)
    for g in (lam, U, w, G):
        g.free()
    out["driver"] = driver(o.driver_N, o.reps)
    out["batch"] = batch(o.batch_N, o.batch, o.reps)
    line = json.dumps(out)
    print(line, flush=True)
    with open(o.out, "w") as f:
        f.write(line + "\n")
    mg.finalize()


if __name__ == "__main__":
    main()
