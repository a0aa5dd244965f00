"""The window boundary of the cycle path: a window enqueued behind an unfinished one records one timing event instead
of two, and no window reduces its smoothing-error norms -- mg_cycle_collect finishes those of the last window from
partial sums kept in the plan's own pool.  None of that may change a reported bit:

  - 1, 2 and 7 windows back to back + one collect() against one execute(), for the smallest hierarchies that run all
    three kernel families (N = 132 and 256 down to 8 or 11: register-tile kernel and LDS coarse tail here, the streaming
    kernel at every level above the tail in a child process with the tile kernel switched off), V(3,3) and a W(2,2)
    file (batched schedule);
  - two plans interleaved, with operator calls and a Solver in between: nothing outside a plan reaches its partials;
  - graph replay, the mixed mode's refinement loop, close() with a window pending;
  - device_ms: positive, consistent with the wall time of a back-to-back batch, and free of a preceding idle gap."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import _window_boundary_worker as wb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

FILES = [("V", 132, 8), ("V", 132, 11), ("V", 256, 8), ("V", 256, 11), ("W", 256, 8)]


@pytest.mark.parametrize("kind,N,n_min", FILES, ids=[f"{k}{n}-{m}" for k, n, m in FILES])
def test_back_to_back_windows_report_what_execute_reports(mg, tmp_path, kind, N, n_min):
    path = wb.write_file(mg, tmp_path, kind, N, n_min)
    if kind == "W":   # (the file this case is about: independent visits merged into batched launches)
        plan = mg.CyclePlan(path, fused=True)
        assert plan.execute()["schedule_launches"] > 0
        plan.close()
    assert wb.check_back_to_back(mg, path) == len(wb.WINDOWS)


def test_back_to_back_windows_streaming_kernel_only(mg):
    """The same with MG_TILE_MAX_N=0 (read once per process, hence a child): every level above the coarse tail is a
    streaming-kernel launch, the third producer of norm partials."""
    files = [(132, 8, "V"), (256, 11, "V"), (256, 8, "W")]
    env = dict(os.environ, MG_TILE_MAX_N="0")
    out = subprocess.run([sys.executable, os.path.join(HERE, "_window_boundary_worker.py")] + [str(t) for f in files for t in f],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res == {"ok": True, "checks": len(files) * len(wb.WINDOWS)}


@pytest.mark.parametrize("between", ["nothing", "operators"])
def test_interleaved_plans_keep_their_own_partials(mg, tmp_path, between):
    """A, B, A, B, then collect B, collect A: when A is collected its last window's partial sums have lain through two
    windows and the reduction of B -- and, in the second case, an operator call that reduces a norm and a whole Solver
    run.  With the partials in an arena shared by everything on the context this is the case that breaks."""
    A = mg.CyclePlan(wb.write_file(mg, tmp_path, "V", 132, 8), fused=True)
    B = mg.CyclePlan(wb.write_file(mg, tmp_path, "V", 256, 8), fused=True)
    want_A, want_B = A.execute(fetch_U=True), B.execute(fetch_U=True)
    for plan in (A, B, A, B):
        assert plan.enqueue() == 0
    if between == "operators":
        n = 64
        rng = np.random.default_rng(5)
        F = rng.random((n, n)) - 0.5
        U_in, U_out, Fd = mg.DeviceGrid.from_host(rng.random((n, n))), mg.DeviceGrid(n), mg.DeviceGrid.from_host(F)
        assert mg.smooth_pp(n, 1.0, U_in, U_out, Fd, 3, want_error=True) > 0.0
        solver = mg.Solver(n)
        _, info = solver.solve(F)
        assert info["converged"], info
        solver.close()
    wb.same_window(B.collect(fetch_U=True), want_B, "B")
    wb.same_window(A.collect(fetch_U=True), want_A, "A")
    A.close()
    B.close()


def test_graph_replay_finishes_at_collect(mg, tmp_path):
    path = wb.write_file(mg, tmp_path, "V", 256, 8)
    eager = mg.CyclePlan(path, fused=True)
    want = eager.execute(fetch_U=True)
    eager.close()
    plan = mg.CyclePlan(path, fused=True, graph=True)
    for _ in range(5):
        assert plan.enqueue() == 0
    got = plan.collect(fetch_U=True)
    assert got["graph_replayed"]
    wb.same_window(got, want, "graph, 5 windows")
    plan.close()


def test_graph_replay_after_an_interpreted_window(mg, tmp_path):
    """A W(2,2) plan with a batched schedule, captured and replayed; then the smoother is switched away (that window runs
    node by node and builds a pending list of its own) and back: the replay that follows must reduce the list of the
    window the graph was captured from, not the interpreter's."""
    path = wb.write_file(mg, tmp_path, "W", 256, 8)
    eager = mg.CyclePlan(path, fused=True)
    want = eager.execute(fetch_U=True)
    assert want["schedule_launches"] > 0
    eager.close()
    plan = mg.CyclePlan(path, fused=True, graph=True)
    try:
        for _ in range(4):
            assert plan.enqueue() == 0
        got = plan.collect(fetch_U=True)
        assert got["graph_replayed"]
        wb.same_window(got, want, "graph, before the switch")
        mg.set_smoother("simple")
        between = plan.execute()
        assert between["status"] == 0 and not between["graph_replayed"] and between["schedule_launches"] == 0
        mg.set_smoother("stream")
        assert plan.enqueue() == 0
        got = plan.collect(fetch_U=True)
        assert got["graph_replayed"]
        wb.same_window(got, want, "graph, after the switch back")
    finally:
        mg.set_smoother("stream")
        plan.close()


def test_mixed_refinement_loop(mg, tmp_path):
    """two fp32 cycles per window: records (those of the last cycle), the fp64 iterate and the refinement error"""
    path = wb.write_file(mg, tmp_path, "V", 256, 8)
    plan = mg.CyclePlan(path, fused=True, mixed=True, refinement=2)
    want = plan.execute(fetch_U=True)
    assert len(want["refinement_errors"]) == 1 and want["refinement_errors"][0] > 0.0
    for k in wb.WINDOWS:
        for _ in range(k):
            assert plan.enqueue() == 0
        got = plan.collect(fetch_U=True)
        wb.same_window(got, want, f"mixed, {k} windows")
        assert np.array_equal(wb.bits(got["refinement_errors"]), wb.bits(want["refinement_errors"]))
    plan.close()


def test_close_with_a_window_pending(mg, tmp_path):
    path = wb.write_file(mg, tmp_path, "V", 132, 8)
    first = mg.CyclePlan(path, fused=True)
    want = first.execute(fetch_U=True)
    assert first.enqueue() == 0
    first.close()                      # its reductions are dropped with it
    mg.sync()                          # (raises if the engine recorded an error)
    again = mg.CyclePlan(path, fused=True)
    wb.same_window(again.execute(fetch_U=True), want, "the next plan")
    again.close()


def test_device_ms_of_an_execute_is_positive(mg, tmp_path):
    plan = mg.CyclePlan(wb.write_file(mg, tmp_path, "V", 256, 8), fused=True)
    for _ in range(2):
        assert plan.execute()["device_ms"] > 0.0
    plan.close()


def test_device_ms_of_a_back_to_back_window_matches_the_wall_time(mg, tmp_path):
    """K windows back to back: the last one's device_ms runs from the end of window K-1 to its own end, so K times it is
    the wall time of the batch (sanity bound 25 %; the expected ratio is about 1).  N = 4096: the smallest size at which
    a window keeps the device busy clearly longer than the host needs to enqueue its launches (measured: 0.287 ms per
    window, ratio 0.98) -- at the sizes of the other tests the stream can run dry between two windows; every such window
    records a start event of its own and the batch is bounded by the host, not by the device."""
    K = 20
    plan = mg.CyclePlan(wb.write_file(mg, tmp_path, "V", 4096, 8), fused=True, report=False, error=False)
    assert plan.execute()["status"] == 0
    for _ in range(K):                 # (clocks up, as in the timed batch)
        plan.enqueue()
    mg.sync()
    t0 = time.perf_counter()
    for _ in range(K):
        plan.enqueue()
    mg.sync()
    wall_ms = (time.perf_counter() - t0) * 1e3
    r = plan.collect()
    plan.close()
    print(f"K = {K}: wall {wall_ms:.4f} ms, last device_ms {r['device_ms']:.4f} ms, ratio {K * r['device_ms'] / wall_ms:.4f}")
    assert r["status"] == 0
    assert abs(K * r["device_ms"] - wall_ms) <= 0.25 * wall_ms


def test_device_ms_leaves_an_idle_gap_out(mg, tmp_path):
    """a window enqueued on an idle stream records its own start event: 50 ms of nothing before it are not counted"""
    plan = mg.CyclePlan(wb.write_file(mg, tmp_path, "V", 256, 8), fused=True)
    assert plan.execute()["status"] == 0
    mg.sync()
    time.sleep(0.05)
    assert plan.enqueue() == 0
    r = plan.collect()
    plan.close()
    print(f"device_ms after a 50 ms idle gap: {r['device_ms']:.4f}")
    assert 0.0 < r["device_ms"] < 10.0
