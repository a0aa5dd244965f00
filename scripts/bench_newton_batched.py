"""The batched semilinear solve (include/mg_newton_batch.h) against a loop of single solves, in ONE process, alternating, medians
over --reps with min and max.  V(3,3) with inner solves to rtol 1e-8, default Newton options, sinh with a smooth weight shared
by the instances, kappa per instance (1 .. 10 over the batch), one F shared by all, U = 0 before every call; with and without
the coefficient a = 1 + 0.5 sin(2 pi x) cos(2 pi y).
  solves    one BatchSolver.newton_ptrs call over B instances against B Solver.newton_ptr calls, wall time around a synchronised
            call, for (N, B) = (257, 1 / 16 / 64), (1025, 1 / 16 / 64) and (8192, 1).  The yardstick is the loop of single
            solves; loop_spread is (max - min)/median of its own repetitions, against which a B = 1 ratio is judged.  The
            instances of the two sides are checked to agree (iterations, residuals) before anything is timed.
  step      the batched step pass at 8192^2, B = 1, with a (56 B per point), against the single pass's `newton_step` profile
            entry, both timed by the engine's own event pairs; single_spread is that entry's own (max - min)/median.
Prints one JSON line and writes it to --out (default profiles/newton_batched_bench_line.json).  --quick leaves out N = 8192."""
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

KIND = "sinh"
INNER_RTOL = 1e-8   # (the solver's default 1e-10 is below the fp64 rounding floor of a solve at N = 8192)
CASES = [(257, 1), (257, 16), (257, 64), (1025, 1), (1025, 16), (1025, 64), (8192, 1)]


def fields(N):
    x = np.arange(N) / float(N - 1)
    w = np.sin(2 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]
    F = -40.0 * np.sin(np.pi * x)[None, :] * np.sin(2 * np.pi * x)[:, None]
    return 1.0 + 0.5 * w, 1.0 + 0.5 * w.T, F   # a, a smooth weight, a right-hand side that makes |u| of order one


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def kappas(B):
    return [1.0 + 9.0 * i / max(B - 1, 1) for i in range(B)]


def solves(N, B, a, w, F, reps):
    opts = dict(pre=3, post=3, rtol=INNER_RTOL)
    kap = kappas(B)
    single = mg.Solver(N, 1.0, coef=a, **opts)
    batch = mg.BatchSolver(N, 1.0, max_batch=B, **opts)
    if a is not None:
        batch.set_coefficient(a)
    U = [mg.DeviceGrid.zeros((N, N)) for _ in range(B)]
    Fp, Up = [F.ptr] * B, [u.ptr for u in U]

    def timed(f):
        for u in U:
            mg.lib().mg_fill_zero(u.ptr, u.size)
        mg.sync()
        t0 = time.perf_counter()
        out = f()
        mg.sync()
        return 1e3 * (time.perf_counter() - t0), out

    runs = {"batched": lambda: batch.newton_ptrs(Fp, Up, kind=KIND, kappa=kap, w_ptrs=[w.ptr]),
            "loop": lambda: [single.newton_ptr(F.ptr, Up[i], kind=KIND, kappa=kap[i], w_ptr=w.ptr) for i in range(B)]}
    first = {k: timed(f)[1] for k, f in runs.items()}   # warm-up of every shape (and the drivers' allocations)
    assert list(first["batched"]) == first["loop"], "the batched call and the loop disagree"
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, f in runs.items():
            ms[k].append(timed(f)[0])
    stats = first["batched"].stats
    single.close(), batch.close()
    for u in U:
        u.free()
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(N=N, B=B, coef=a is not None, ms={k: spread(v) for k, v in ms.items()},
                loop_over_batched=round(med["loop"] / med["batched"], 3),
                loop_spread=round((max(ms["loop"]) - min(ms["loop"])) / med["loop"], 4),
                iterations=[i["iterations"] for i in first["loop"]][:4], converged=all(i["converged"] for i in first["loop"]),
                batched_stats={k: stats[k] for k in ("iterations", "trial_rounds", "inner_cycles", "launches")})


def step_pass(N, a, F, reps):
    G = mg.DeviceGrid
    U, dlt, V, D, S = (G.zeros((N, N)) for _ in range(5))
    args = (N, 1.0, 0.0)
    calls = {"newton_step": lambda: mg.nonlinear_residual(*args, a, KIND, 10.0, None, U, F, D, S, dlt=dlt, t=0.5, V=V),
             "newton_step_batch": lambda: mg.nonlinear_residual_batch(*args, a, KIND, 10.0, None, [U], [F], [D], [S], dlt=[dlt], t=0.5,
                                                                     V=[V])}
    for f in calls.values():
        f()
    us = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            mg.profile_begin(0)
            f()
            got = {e["name"]: e for e in mg.profile_end()}
            assert got[k]["launches"] == 1 and got[k]["algo_bytes"] == 56 * N * N, got[k]
            us[k].append(1e3 * got[k]["total_ms"])
    for g in (U, dlt, V, D, S):
        g.free()
    med = {k: statistics.median(v) for k, v in us.items()}
    y = "newton_step"
    return dict(N=N, B=1, bytes_per_point=56, us={k: spread(v) for k, v in us.items()},
                batched_over_single=round(med["newton_step_batch"] / med[y], 4),
                single_spread=round((max(us[y]) - min(us[y])) / med[y], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="without N = 8192")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton_batched_bench_line.json"))
    o = ap.parse_args()
    mg.init(0)
    rows, step = [], "not measured"
    for N in sorted({n for n, _ in CASES}):
        if o.quick and N > 2048:
            continue
        ah, wh, Fh = fields(N)
        a, w, F = (mg.DeviceGrid.from_host(x) for x in (ah, wh, Fh))
        del ah, wh, Fh
        for n, B in CASES:
            if n == N:
                for coef in (None, a):
                    rows.append(solves(N, B, coef, w, F, o.reps))
                    print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        if N == 8192:
            step = step_pass(N, a, F, o.reps)
        for g in (a, w, F):
            g.free()
    res = dict(metric="newton_batched", kind=KIND, cycle="V(3,3)", inner_rtol=INNER_RTOL, reps=o.reps, kappa="1 .. 10 over the batch",
               field_a="1 + 0.5 sin(2 pi x) cos(2 pi y)", field_w="1 + 0.5 sin(2 pi y) cos(2 pi x)", solves=rows, step=step)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(line + "\n")
    mg.finalize()


if __name__ == "__main__":
    main()
