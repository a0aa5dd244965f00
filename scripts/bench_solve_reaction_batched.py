"""The batched solve with a reaction term (BatchSolver.set_reaction, include/mg_rx_batch.h) against its yardstick, a loop of B
Solver(reaction=s_i[, coef=a_i]).solve calls, in one process: V(3,3), omega 0.8, rtol 1e-9, instance i solves
F_i = (1 + i/B) * getSource from U = 0 with its own s_i = 1e4 (1 + sin(2 pi (x + i/B)) cos(2 pi y)), without a coefficient and
with the smooth a_i = 1 + 0.5 sin(2 pi (x + i/B)) cos(2 pi y) of scripts/bench_solve_vc_batched.py.
B in {1, 16, 64} at N = 257 and N = 1025, and B = 1 at N = 8192.  Per case --reps repetitions (at least 5), the batched call
and the loop alternating within each; every solver exists, with its reaction and coefficient set, before the first timed
solve.  Two times per side: the sum of the solvers' hipEvent times (device_ms of every call) and the wall-clock time of the
whole side between two device synchronisations -- the loop's launch gaps between calls are only in the second.  Reported:
medians, the ratio loop / batched per repetition as median and [min, max], and the launches per cycle (the batched cycle's
from stats.launches; the loop enqueues B times the single cycle's).  No threshold: the numbers are the result.
Writes one JSON line to profiles/solve_reaction_batched_bench_line.json (--out) and prints it."""
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

OPTS = dict(rtol=1e-9)


def wave(N, i, B):
    x = np.arange(N) / float(N - 1)
    return np.sin(2 * np.pi * (x + i / B))[None, :] * np.cos(2 * np.pi * x)[:, None]


def case(N, B, with_a, reps):
    src = mg.getSource(N).to_host()
    Fs = [mg.DeviceGrid.from_host(src * (1.0 + i / B)) for i in range(B)]
    del src
    Us = [mg.DeviceGrid.zeros((N, N)) for _ in range(B)]
    Ss = [mg.DeviceGrid.from_host(1e4 * (1.0 + wave(N, i, B))) for i in range(B)]
    As = [mg.DeviceGrid.from_host(1.0 + 0.5 * wave(N, i, B)) for i in range(B)] if with_a else []
    batch = mg.BatchSolver(N, 1.0, max_batch=B, **OPTS)
    if with_a:
        batch.set_coefficient(As)
    batch.set_reaction(Ss)
    loop = [mg.Solver(N, 1.0, reaction=Ss[i], **(dict(coef=As[i]) if with_a else {}), **OPTS) for i in range(B)]
    for g in Ss + As:
        g.free()
    F_ptrs, U_ptrs = [f.ptr for f in Fs], [u.ptr for u in Us]

    def zero():
        for u in Us:
            mg.lib().mg_fill_zero(u.ptr, N * N)
        mg.sync()

    def run_batched():
        zero()
        t0 = time.perf_counter()
        infos = batch.solve_ptrs(F_ptrs, U_ptrs)
        mg.sync()
        return (time.perf_counter() - t0) * 1e3, infos[0]["stats"]["device_ms"], infos

    def run_loop():
        zero()
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
    per_cycle = (stats["launches"] - 4) / max(stats["cycles"], 1)   # (4: the two norms of the start)
    batch.close()
    for s in loop:
        s.close()
    for g in Fs + Us:
        g.free()
    med = statistics.median
    ratio_wall = [l / b for l, b in zip(wall_l, wall_b)]
    ratio_dev = [l / b for l, b in zip(dev_l, dev_b)]
    spread = lambda v: [round(min(v), 3), round(max(v), 3)]   # noqa: E731
    return dict(N=N, B=B, coef=bool(with_a), reps=reps, cycles=[i["cycles"] for i in ib][:4], max_cycles=stats["cycles"],
                converged=all(i["converged"] for i in ib), same_history_as_loop=same,
                batched_launches_per_cycle=round(per_cycle, 2), loop_launches_per_cycle=round(B * (per_cycle - 1), 2),
                batched_wall_ms=round(med(wall_b), 3), loop_wall_ms=round(med(wall_l), 3),
                loop_wall_ms_spread=spread(wall_l), batched_wall_ms_spread=spread(wall_b),
                batched_device_ms=round(med(dev_b), 3), loop_device_ms=round(med(dev_l), 3),
                loop_over_batched_wall=round(med(ratio_wall), 3), loop_over_batched_wall_spread=spread(ratio_wall),
                loop_over_batched_device=round(med(ratio_dev), 3), loop_over_batched_device_spread=spread(ratio_dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="257,1025")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--big", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_reaction_batched_bench_line.json"))
    a = ap.parse_args()
    mg.init(0)
    rows = []
    cases = [(int(n), int(b)) for n in a.sizes.split(",") if n for b in a.batches.split(",")] + ([(a.big, 1)] if a.big else [])
    for N, B in cases:
        for with_a in (False, True):
            rows.append(case(N, B, with_a, max(a.reps, 5)))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    out = dict(metric="solve_reaction_batched", pre=3, post=3, omega=0.8, rtol=OPTS["rtol"],
               yardstick="loop of B Solver(reaction=s_i[, coef=a_i]).solve",
               note="the loop's launch count excludes the batched cycle's final copy kernel (a memcpy in the single solve)", rows=rows)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    mg.finalize()


if __name__ == "__main__":
    main()
