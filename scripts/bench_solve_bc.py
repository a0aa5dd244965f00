"""The solve with boundary kinds per side (include/mg_bc.h) against the variable-coefficient path with four Dirichlet sides, in
one process, alternating, medians over --reps: N = 8192, V(3,3), omega = 0.8, the getSource problem from U = 0 to rtol 1e-8:
    nnnn_one / nnnn_smooth   four Neumann sides, sigma = 1e4, a == 1 (as an array) / a = 1 + 0.5 sin(2 pi x) cos(2 pi y)
    ndnd_one / ndnd_smooth   S and W Neumann, N and E Dirichlet, sigma = 0
    nnnn_none                four Neumann sides without a coefficient (a = 1 through the same expressions, one array less)
The yardstick of each is the variable-coefficient solver (mg_varcoef.h) on the same F, coefficient and sigma with Dirichlet
sides: dddd_<sigma>_<field>.  Reports ms per cycle (the solver's hipEvent time over the cycles of the solve; the two start
norms are inside it for every variant alike), the cycles, and the ratios with the [min, max] of the per-repetition ratios.
The bytes per point are the same -- a mirrored ghost row re-reads a row the block streams anyway -- so the expectation is
parity within the `_vc` kernels' own spread.  Prints one JSON line.

    python scripts/bench_solve_bc.py --cycles-table      cycles to rtol 1e-9 at N = 257 and 1025, random F and start, for the
                                                         kinds and shifts of tests/test_solve_bc_cpu.py::test_convergence
Per-kernel times come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_solve_bc.py --kernels"""
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


def exp_field(N):
    x = np.arange(N) / float(N - 1)
    return np.exp(2.0 * np.sin(3.0 * x[None, :] + x[:, None]))


def cycles_table():
    cases = [("nnnn", 1e2), ("nnnn", 1e4), ("ddnd", 0.0), ("ndnd", 0.0), ("nndd", 0.0), ("nnnd", 0.0), ("dddd", 0.0)]
    out = {}
    for N in (257, 1025):
        rng = np.random.default_rng(500 + N)
        F, U0 = rng.random((N, N)) - 0.5, rng.random((N, N)) - 0.5
        for name, a in (("one", None), ("exp", exp_field(N))):
            for bc, shift in cases:
                _, info = mg.solve(F, U0, 1.0, coef=a, bc=bc, shift=shift, rtol=1e-9)
                out[f"N{N}_{name}_{bc}_{shift:g}"] = [info["cycles"], bool(info["converged"]), bool(info["coarse_capped"])]
    print(json.dumps(dict(metric="solve_bc_cycles_to_1e-9", cases=out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels", action="store_true", help="one solve per variant, for a profiler run")
    ap.add_argument("--cycles-table", action="store_true")
    a = ap.parse_args()
    mg.init(0)
    if a.cycles_table:
        cycles_table()
        mg.finalize()
        return
    N = a.N
    F = mg.getSource(N, 1.0)
    U = mg.DeviceGrid.zeros((N, N))
    coefs = {"one": mg.DeviceGrid.from_host(np.ones((N, N))), "smooth": mg.DeviceGrid.from_host(smooth_field(N))}
    kinds = {"nnnn": 1e4, "ndnd": 0.0}
    solvers, yard = {}, {}
    for bc, shift in kinds.items():
        for field, c in coefs.items():
            opts = dict(rtol=a.rtol, max_cycles=50, shift=shift)
            solvers[f"{bc}_{field}"] = mg.Solver(N, 1.0, coef=c, bc=bc, **opts)
            solvers[f"dddd_{shift:g}_{field}"] = mg.Solver(N, 1.0, coef=c, **opts)
            yard[f"{bc}_{field}"] = f"dddd_{shift:g}_{field}"
    solvers["nnnn_none"] = mg.Solver(N, 1.0, bc="nnnn", rtol=a.rtol, max_cycles=50, shift=kinds["nnnn"])

    def run(name):
        mg.lib().mg_fill_zero(U.ptr, U.size)
        info = solvers[name].solve(F, U)[1]
        return info["device_ms"] / max(info["cycles"], 1), info["cycles"], bool(info["converged"])

    order = sorted(solvers)
    for name in order:
        run(name)   # warm-up of every shape
    if a.kernels:
        mg.finalize()
        return
    ms = {name: [] for name in order}
    cycles, conv = {}, {}
    for _ in range(a.reps):
        for name in order:
            t, cycles[name], conv[name] = run(name)
            ms[name].append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratios = {k: [x / y for x, y in zip(ms[k], ms[y_])] for k, y_ in yard.items()}
    out = dict(metric="solve_bc_ms_per_cycle", N=N, rtol=a.rtol, reps=a.reps, pre=3, post=3, omega=0.8,
               ms_per_cycle={k: round(v, 4) for k, v in med.items()},
               spread={k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
               cycles=cycles, converged=conv,
               over_dirichlet_vc={k: round(med[k] / med[y_], 4) for k, y_ in yard.items()},
               over_dirichlet_vc_spread={k: [round(min(v), 4), round(max(v), 4)] for k, v in ratios.items()})
    print(json.dumps(out), flush=True)
    mg.finalize()


if __name__ == "__main__":
    main()
