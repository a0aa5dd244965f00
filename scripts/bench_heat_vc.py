"""The heat stepper with a variable coefficient (include/mg_heat_vc.h), measured in one process with the variants alternating:
N = 8192, theta = 1/2, with a source Q, the coefficient a = 1 + 0.5 sin(2 pi x) cos(2 pi y), seeded uniform U and Q.

  kernels   per repetition one launch each of k_heat_rhs_vc (mg_heat_rhs_coef), of k_residual_vc at level 0
            (mg_residualCoefficient: the same 32 B per point -- U, a and one more array read, one written -- and the yardstick)
            and of k_heat_rhs<lap> (mg_heat_rhs, 24 B per point), each timed by the engine's event pair around the launch
            (mg_profile_begin / mg_profile_end).  Medians over --kernel-reps, the spread (min, max) beside them, the ratios,
            and algorithmic bytes over the median time as a share of the 8 TB/s HBM peak.  The new kernel may exceed the
            yardstick by no more than the spread of that comparison; the byte model puts it at 4/3 of k_heat_rhs<lap>.
  stepper   --steps steps through HeatStepper against the caller's loop of {heat_rhs_coef, Solver(shift = sigma, coef = a)
            .solve} from the same start, rtol 1e-8: host clock around work that ends in a device synchronise, medians over
            --reps with the spread, ms and cycles per step.  The stepper has to stay within 1.04 x of the loop.

Prints one JSON line and writes it to --out (default profiles/heat_vc_bench_line.json)."""
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

HBM_PEAK = 8.0e12
RTOL = 1e-8
NU, SIGMA = 1.0, 1e4


def smooth_field(N):
    x = np.arange(N) / float(N - 1)
    return 1.0 + 0.5 * np.sin(2 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def kernels(N, theta, dt, a, U, Q, F, reps):
    """us per launch of the three kernels, alternating"""
    calls = {"heat_rhs_vc": lambda: mg.heat_rhs_coef(N, 1.0, NU, dt, theta, a, U, Q, F),
             "residual_vc": lambda: mg.residualCoefficient(N, 1.0, SIGMA, a, U, Q, F, -1),
             "heat_rhs<lap>": lambda: mg.heat_rhs(N, 1.0, NU, dt, theta, U, Q, F)}
    bytes_per_point = {"heat_rhs_vc": 32, "residual_vc": 32, "heat_rhs<lap>": 24}
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
                heat_rhs_vc_over_residual_vc=round(med["heat_rhs_vc"] / med["residual_vc"], 4),
                # the spread of the comparison: how far repetitions of the yardstick alone lie from their median
                residual_vc_spread=round((max(us["residual_vc"]) - min(us["residual_vc"])) / med["residual_vc"], 4),
                heat_rhs_vc_over_heat_rhs_lap=round(med["heat_rhs_vc"] / med["heat_rhs<lap>"], 4), bytes_model_ratio=round(32 / 24, 4))


def stepping(N, theta, dt, a, U0, U, Q, F, steps, warmup, reps):
    hs = mg.HeatStepper(N, 1.0, NU, dt, theta, rtol=RTOL)
    hs.set_coefficient(a)
    sv = mg.Solver(N, 1.0, shift=hs.sigma, coef=a, rtol=RTOL)

    def reset():
        mg.lib().mg_copy(U.ptr, U0.ptr, U.size)
        mg.sync()

    def stepper(k=steps):
        reset()
        t = time.perf_counter()
        infos = hs.step(U, Q, steps=k)[1]
        mg.sync()
        return 1e3 * (time.perf_counter() - t), infos[0]["cycles_per_step"], infos[0]["converged"]

    def loop(k=steps):
        reset()
        cycles, conv = [], True
        t = time.perf_counter()
        for _ in range(k):
            mg.heat_rhs_coef(N, 1.0, NU, dt, theta, a, U, Q, F)
            info = sv.solve(F, U)[1]
            cycles.append(info["cycles"])
            conv = conv and info["converged"]
        mg.sync()
        return 1e3 * (time.perf_counter() - t), cycles, conv

    stepper(warmup)
    loop(warmup)
    runs = {"stepper": [], "loop": []}
    for _ in range(reps):
        runs["stepper"].append(stepper())
        runs["loop"].append(loop())
    bits = None
    if N <= 2048:   # (small sizes only: the two ways end on the same bits)
        stepper()
        A = U.to_host()
        loop()
        bits = bool(np.array_equal(A.view(np.uint64), U.to_host().view(np.uint64)))
    hs.close()
    sv.close()
    ms = {k: [t / steps for t, _, _ in v] for k, v in runs.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(steps=steps, reps=reps, sigma=hs.sigma, ms_per_step={k: spread(v) for k, v in ms.items()},
                cycles_per_step=runs["stepper"][-1][1], loop_cycles_per_step=runs["loop"][-1][1],
                converged=bool(runs["stepper"][-1][2] and runs["loop"][-1][2]),
                stepper_over_loop=round(med["stepper"] / med["loop"], 4), same_bits=bits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heat_vc_bench_line.json"))
    o = ap.parse_args()
    N, theta = o.N, 0.5
    dt = 1.0 / (theta * NU * SIGMA)
    mg.init(0)
    a = mg.DeviceGrid.from_host(smooth_field(N))
    U0, Q = mg.DeviceGrid.uniform((N, N), 1234 + N), mg.DeviceGrid.uniform((N, N), 4321 + N)
    U, F = U0.copy(), mg.DeviceGrid((N, N))
    out = dict(metric="heat_vc_step_ms", N=N, theta=theta, nu=NU, dt=dt, rtol=RTOL, field="1 + 0.5 sin(2 pi x) cos(2 pi y)",
               kernels=kernels(N, theta, dt, a, U, Q, F, o.kernel_reps),
               stepper=stepping(N, theta, dt, a, U0, U, Q, F, o.steps, o.warmup, o.reps))
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(line + "\n")
    mg.finalize()


if __name__ == "__main__":
    main()
