"""The batched Krylov solve (BatchSolver.set_krylov(8), include/mg_krylov_batch.h) against its yardstick, a loop of B
Solver(krylov=8, coef=a_i).solve calls, in one process: V(3,3), omega 0.8, rtol 1e-9, GCR(8), the coefficients on which the
plain cycle crawls or diverges -- even instances a 10x jump across a line x = c_i, odd instances a random field of contrast
1e3 (seed i) -- and instance i solves F_i = (1 + i/B) * getSource from U = 0.  N = 257 with B in {1, 16, 64} and N = 1025 with
B in {1, 16}.  Per case --reps repetitions (at least 5), the batched call and the loop alternating within each; every solver
exists, with its coefficient and its Krylov storage, before the first timed solve.  Two times per side: the sum of the
solvers' hipEvent times (device_ms of every call) and the wall-clock time of the whole side between two device
synchronisations -- the loop's launch gaps between calls are only in the second.  Reported: medians, the ratio
loop / batched per repetition as median and [min, max], the iterations, and the launches of the batched call.  No threshold:
the numbers are the result.
Kernel byte rates (informational): one further, profiled batched solve of the case --rates (N,B; default 1025,16) gives, per
batched Krylov launch, the bytes the header counts (the dots and the orthogonalisation by each instance's k, from the logs)
over the time between the launch's events, beside the same figure for the batched residual of the restarts
(k_residual_vc_batch, 32 bytes per point) in the same process.
Writes one JSON line to profiles/solve_krylov_batched_bench_line.json (--out) and prints it."""
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

M = 8
OPTS = dict(rtol=1e-9, max_cycles=200)


def field(N, i, B):
    if i % 2:
        return 10.0 ** (3.0 * np.random.default_rng(i).random((N, N)))
    x = np.arange(N) / float(N - 1)
    return np.where(x < 0.25 + 0.5 * i / max(B, 1), 1.0, 10.0)[None, :] + np.zeros((N, 1))


def setup(N, B):
    src = mg.getSource(N).to_host()
    Fs = [mg.DeviceGrid.from_host(src * (1.0 + i / B)) for i in range(B)]
    del src
    Us = [mg.DeviceGrid.zeros((N, N)) for _ in range(B)]
    As = [mg.DeviceGrid.from_host(field(N, i, B)) for i in range(B)]
    batch = mg.BatchSolver(N, 1.0, max_batch=B, **OPTS)
    batch.set_coefficient(As)
    batch.set_krylov(M)
    return Fs, Us, As, batch


def zero(Us, N):
    for u in Us:
        mg.lib().mg_fill_zero(u.ptr, N * N)
    mg.sync()


def case(N, B, reps):
    Fs, Us, As, batch = setup(N, B)
    loop = [mg.Solver(N, 1.0, coef=a, krylov=M, **OPTS) for a in As]
    for a in As:
        a.free()
    F_ptrs, U_ptrs = [f.ptr for f in Fs], [u.ptr for u in Us]

    def run_batched():
        zero(Us, N)
        t0 = time.perf_counter()
        infos = batch.solve_ptrs(F_ptrs, U_ptrs)
        mg.sync()
        return (time.perf_counter() - t0) * 1e3, infos[0]["stats"]["device_ms"], infos

    def run_loop():
        zero(Us, N)
        t0 = time.perf_counter()
        infos = [s.solve_ptr(f, u) for s, f, u in zip(loop, F_ptrs, U_ptrs)]
        mg.sync()
        return (time.perf_counter() - t0) * 1e3, sum(i["device_ms"] for i in infos), infos

    run_batched(), run_loop()   # warm-up of every shape
    wall_b, wall_l, dev_b, dev_l = [], [], [], []
    for _ in range(reps):
        wb, db, ib = run_batched()
        wl, dl, il = run_loop()
        wall_b.append(wb), wall_l.append(wl), dev_b.append(db), dev_l.append(dl)
    same = all(x["history"] == y["history"] and x["cycles"] == y["cycles"] for x, y in zip(ib, il))
    stats = ib[0]["stats"]
    cycles = [i["cycles"] for i in ib]
    batch.close()
    for s in loop:
        s.close()
    for g in Fs + Us:
        g.free()
    med = statistics.median
    ratio_wall = [l / b for l, b in zip(wall_l, wall_b)]
    ratio_dev = [l / b for l, b in zip(dev_l, dev_b)]
    spread = lambda v: [round(min(v), 3), round(max(v), 3)]   # noqa: E731
    return dict(N=N, B=B, reps=reps, iterations=cycles[:4], iterations_min_max=[min(cycles), max(cycles)],
                converged=sum(bool(i["converged"]) for i in ib), same_history_as_loop=same, batched_launches=stats["launches"],
                batched_wall_ms=round(med(wall_b), 3), loop_wall_ms=round(med(wall_l), 3),
                batched_device_ms=round(med(dev_b), 3), loop_device_ms=round(med(dev_l), 3),
                loop_over_batched_wall=round(med(ratio_wall), 3), loop_over_batched_wall_spread=spread(ratio_wall),
                loop_over_batched_device=round(med(ratio_dev), 3), loop_over_batched_device_spread=spread(ratio_dev))


def rates(N, B):
    """GB/s per batched Krylov launch (its finish launch included, as the profiler's scope has it) of one profiled solve"""
    Fs, Us, As, batch = setup(N, B)
    for a in As:
        a.free()
    F_ptrs, U_ptrs = [f.ptr for f in Fs], [u.ptr for u in Us]
    batch.solve_ptrs(F_ptrs, U_ptrs)   # warm-up
    zero(Us, N)
    mg.profile_begin(0)
    try:
        batch.solve_ptrs(F_ptrs, U_ptrs)
    finally:
        prof = {p["name"]: p for p in mg.profile_end(1024) if p["N"] == N}
    logs = [batch.krylov_log(i) for i in range(B)]
    batch.close()
    for g in Fs + Us:
        g.free()
    pts = float(N) * N
    recs = [e for log in logs for e in log]
    total = dict(krylov_zero_batch=8.0 * len(recs), krylov_apply_batch=24.0 * len(recs),
                 krylov_dots_batch=sum(8.0 + 8.0 * e["k"] for e in recs if e["k"] > 0),
                 krylov_orth_batch=sum(40.0 + 16.0 * e["k"] if e["k"] > 0 else 16.0 for e in recs),
                 krylov_update_batch=48.0 * len(recs),
                 krylov_residual_batch=32.0 * (B + sum(e["restarted"] for e in recs)))
    out = {}
    for name, per_point in total.items():
        p = prof.get(name)
        if p and p["total_ms"] > 0:
            out[name] = dict(launches=p["launches"], total_ms=round(p["total_ms"], 3),
                             gbytes_per_s=round(per_point * pts / (p["total_ms"] * 1e-3) / 1e9, 1))
    return dict(N=N, B=B, note="krylov_residual_batch is k_residual_vc_batch on the restarting instances", kernels=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="257:1,257:16,257:64,1025:1,1025:16")
    ap.add_argument("--rates", default="1025,16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_krylov_batched_bench_line.json"))
    a = ap.parse_args()
    mg.init(0)
    rows = []
    for c in a.cases.split(","):
        if not c:
            continue
        N, B = (int(v) for v in c.split(":"))
        rows.append(case(N, B, max(a.reps, 5)))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    out = dict(metric="solve_krylov_batched", m=M, pre=3, post=3, omega=0.8, rtol=OPTS["rtol"], max_cycles=OPTS["max_cycles"],
               fields="even instances: 10x jump across x = 0.25 + 0.5*i/B; odd instances: random, contrast 1e3, seed i",
               yardstick="loop of B Solver(krylov=8, coef=a_i).solve", rows=rows)
    if a.rates:
        N, B = (int(v) for v in a.rates.split(","))
        out["byte_rates"] = rates(N, B)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    mg.finalize()


if __name__ == "__main__":
    main()
