"""Batched residual-tolerance solver (BatchSolver) against B sequential Solver solves in the same process: V(3,3),
omega 0.8, instance i solves F_i = (1 + i/B) * getSource from U = 0 (random F reaches a rounding floor above 1e-10 at
1025^2; getSource converges there in about 10 cycles).  For B in {1, 8, 64} at N = 257 and N = 1025: ms per batched
cycle (steady state), total ms to rtol 1e-10, the same B problems solved one after another with Solver, and the
throughput ratio; B = 1 at N = 8192 (getSource, rtol 1e-9) against Solver.  Times are hipEvent times of whole calls.
--shift SIGMA: every solver solves Laplace(U) - SIGMA*U = F (mg_solve_opts.shift), the workload of implicit time stepping.
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multigrid_poisson_solver_amd as mg  # noqa: E402


SHIFT = {}   # the options every solver of this run gets on top of its own (--shift)


def problems(N, B):
    """(F, U, reset) per instance; reset() puts U back to zero"""
    src = mg.getSource(N).to_host()
    out = []
    for i in range(B):
        U = mg.DeviceGrid.zeros((N, N))
        out.append((mg.DeviceGrid.from_host(src * (1.0 + i / B)), U, lambda U=U: mg.lib().mg_fill_zero(U.ptr, N * N)))
    return out


def reset(probs):
    for _, _, zero in probs:
        zero()


def batched_ms(N, probs, reps, **opts):
    bs = mg.BatchSolver(N, 1.0, max_batch=len(probs), **SHIFT, **opts)
    best, infos = None, None
    for _ in range(reps + 1):   # (the first call warms up)
        reset(probs)
        infos = bs.solve_ptrs([p[0].ptr for p in probs], [p[1].ptr for p in probs])
        t = infos[0]["stats"]["device_ms"]
        best = t if best is None or t < best else best
    bs.close()
    return best, infos


def sequential_ms(N, probs, reps, **opts):
    s = mg.Solver(N, 1.0, **SHIFT, **opts)
    best, cycles = None, 0
    for _ in range(reps + 1):
        reset(probs)
        tot, cycles = 0.0, 0
        for F, U, _ in probs:
            info = s.solve_ptr(F.ptr, U.ptr)
            tot += info["device_ms"]
            cycles += info["cycles"]
        best = tot if best is None or tot < best else best
    s.close()
    return best, cycles


def per_cycle(N, probs, reps):
    """steady-state ms per cycle: 6 fixed cycles minus 2, over 4"""
    t2, _ = batched_ms(N, probs, reps, rtol=0.0, atol=0.0, max_cycles=2)
    t6, _ = batched_ms(N, probs, reps, rtol=0.0, atol=0.0, max_cycles=6)
    return (t6 - t2) / 4.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="257,1025")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--big", type=int, default=8192)
    ap.add_argument("--shift", type=float, default=0.0)
    a = ap.parse_args()
    SHIFT.update(dict(shift=a.shift) if a.shift != 0.0 else {})
    mg.init(0)
    rows = []
    for N in [int(x) for x in a.sizes.split(",")]:
        for B in [int(x) for x in a.batches.split(",")]:
            probs = problems(N, B)
            cyc = per_cycle(N, probs, a.reps)
            tb, infos = batched_ms(N, probs, a.reps, rtol=1e-10)
            ts, seq_cycles = sequential_ms(N, probs, a.reps, rtol=1e-10)
            rows.append(dict(N=N, B=B, batched_cycle_ms=round(cyc, 4), batched_total_ms=round(tb, 3),
                             max_cycles=infos[0]["stats"]["cycles"], launches=infos[0]["stats"]["launches"],
                             converged=all(i["converged"] for i in infos), sequential_total_ms=round(ts, 3),
                             sequential_cycles=seq_cycles, throughput_ratio=round(ts / tb, 2)))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            for F, U, _ in probs:
                F.free()
                U.free()
    big = None
    if a.big:
        # B = 1 against Solver on the same problem: the two alternate within every repetition (min of each)
        N = a.big
        probs = problems(N, 1)
        F, U, zero = probs[0]
        cyc_b, cyc_s, tot_b, tot_s = [], [], [], []
        bs = {k: mg.BatchSolver(N, 1.0, max_batch=1, rtol=0.0, atol=0.0, max_cycles=k, **SHIFT) for k in (2, 6)}
        ss = {k: mg.Solver(N, 1.0, rtol=0.0, atol=0.0, max_cycles=k, **SHIFT) for k in (2, 6)}
        bconv, sconv = mg.BatchSolver(N, 1.0, max_batch=1, rtol=1e-9, **SHIFT), mg.Solver(N, 1.0, rtol=1e-9, **SHIFT)
        for _ in range(2 * a.reps + 1):
            t = {}
            for k in (2, 6):
                zero()
                t["b", k] = bs[k].solve_ptrs([F.ptr], [U.ptr])[0]["device_ms"]
                zero()
                t["s", k] = ss[k].solve_ptr(F.ptr, U.ptr)["device_ms"]
            cyc_b.append((t["b", 6] - t["b", 2]) / 4.0)
            cyc_s.append((t["s", 6] - t["s", 2]) / 4.0)
            zero()
            ib = bconv.solve_ptrs([F.ptr], [U.ptr])[0]
            zero()
            isv = sconv.solve_ptr(F.ptr, U.ptr)
            tot_b.append(ib["device_ms"])
            tot_s.append(isv["device_ms"])
        for x in list(bs.values()) + list(ss.values()) + [bconv, sconv]:
            x.close()
        cb, cs = float(np.median(cyc_b[1:])), float(np.median(cyc_s[1:]))
        big = dict(N=N, B=1, rtol=1e-9, batched_cycle_ms=round(cb, 4), solver_cycle_ms=round(cs, 4), cycle_ratio=round(cb / cs, 4),
                   batched_total_ms=round(min(tot_b[1:]), 3), solver_total_ms=round(min(tot_s[1:]), 3), cycles=ib["cycles"],
                   solver_cycles=isv["cycles"], converged=ib["converged"], same_history=ib["history"] == isv["history"])
    out = dict(metric="solve_batched", pre=3, post=3, omega=0.8, shift=a.shift, rows=rows, big=big)
    print(json.dumps(out), flush=True)
    mg.finalize()


if __name__ == "__main__":
    main()
