"""Shared by tests/test_window_boundary_gpu.py and run by it as a child process: windows enqueued back to back and
collected once must report what one execute() reports, bit for bit.  TEST INFRASTRUCTURE.

As a program (argv: N n_min V|W ...) it runs check_back_to_back on each file under the environment the parent gave it
-- the register-tile kernel switched off, so that every level above the coarse tail is a streaming-kernel launch --
and prints one JSON line."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

WINDOWS = (1, 2, 7)


def write_file(mg, directory, kind, N, n_min):
    """V(3,3) or W(2,2) over N ... n_min."""
    path = os.path.join(str(directory), f"{kind}{N}_{n_min}.txt")
    if kind == "V":
        mg.write_vcycle_file(path, N, n_min, 3, 1e-7)
    else:
        mg.write_wcycle_file(path, N, n_min, 2, 1e-7)
    return path


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_window(got, want, what):
    """status 0, the same records with bit-equal errors, bit-equal U"""
    assert got["status"] == 0 and want["status"] == 0, (what, got["status"], want["status"])
    assert len(got["records"]) == len(want["records"]) > 0, what
    for i, (g, w) in enumerate(zip(got["records"], want["records"])):
        assert g[:3] == w[:3], (what, i, g, w)
        assert bits(g[3]) == bits(w[3]), f"{what}: record {i} {g[:3]} error {g[3]!r} != {w[3]!r}"
    assert np.array_equal(bits(got["U"]), bits(want["U"])), f"{what}: U differs"


def check_back_to_back(mg, path, **plan_args):
    """(a) execute() once; (b) 1, 2 and 7 windows back to back, then one collect().  Returns the number of comparisons."""
    plan = mg.CyclePlan(path, fused=True, **plan_args)
    want = plan.execute(fetch_U=True)
    assert any(r[0] != 0 and r[3] != 0.0 for r in want["records"]), "no smoothing error was reported"
    for k in WINDOWS:
        for _ in range(k):
            assert plan.enqueue() == 0
        same_window(plan.collect(fetch_U=True), want, f"{os.path.basename(path)}: {k} windows")
    plan.close()
    return len(WINDOWS)


if __name__ == "__main__":
    import tempfile
    from multigrid_poisson_solver_amd import build as b
    b.ensure_built()
    import multigrid_poisson_solver_amd as mg
    mg.init(0)
    d = tempfile.mkdtemp(prefix="mgwb_")
    n = 0
    for a in range(1, len(sys.argv), 3):
        N = int(sys.argv[a])
        path = write_file(mg, d, sys.argv[a + 2], N, int(sys.argv[a + 1]))
        n += check_back_to_back(mg, path)
        # the point of this process: the finest level runs as streaming-kernel launches (its `-1` and its `1` node)
        mg.stream_geometry_log(True)
        plan = mg.CyclePlan(path, fused=True)
        assert plan.execute()["status"] == 0
        plan.close()
        assert sum(1 for g in mg.stream_geometry_fetch() if g["N"] == N) >= 2, "no streaming launch at the finest level"
        mg.stream_geometry_log(False)
    mg.finalize()
    print(json.dumps({"ok": True, "checks": n}))
