"""Any tiling, the same bits: k_jacobi_stream under forced chunk geometries.

The launcher of the streaming smoother (launch_k, csrc/mg_stream_impl.h) cuts the rows of a launch into chunks whose
height follows the device's CU count, the occupancy of the instantiation, the batch size and the slab window -- none of
them a property of the problem; the waves of a chunk recompute 2 (S + PRE + 1) halo rows at its seams.  The rest of the
suite sees only the heights a 256-CU device produces at its sizes.  Here every child process (the knobs are static per
process) forces one geometry and runs the calls that reach the kernel -- plain, zero-start, fused restriction, fused
prolongation with and without recomputed pre-sweeps, weighted, shifted, fp32 with 2 and 4 columns per lane, batches, slab
windows -- at N = 132 / 131 and 484 / 483, every output bit for bit against the oracle (tests/_stream_geometry_worker.py).
The geometry each launch really used comes back through mg_stream_geometry_log and is held to a restatement of the
launcher's arithmetic (tests/_stream_geometry.py), so a knob that is silently ignored fails the case instead of passing it."""
import json
import os
import subprocess
import sys

import pytest

import _stream_geometry as sg

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILDREN = sg.children()
CHILD_TIMEOUT = 60   # seconds; a child takes one or two, its CPU references included
_outcomes = {}       # child id -> its line, or the failure it ended in: no child is ever started twice


def run_child(c):
    """The line of child c.  It is started at most once per session: a child that failed, faulted or ran into its time
    limit is remembered as such, and whoever asks for it again (the coverage test) fails on the stored outcome."""
    cid = sg.child_id(c)
    if cid not in _outcomes:
        _outcomes[cid] = RuntimeError(f"{cid}: the child did not come to an end")   # (replaced below unless we are interrupted)
        try:
            from multigrid_poisson_solver_amd import build as b
            b.ensure_built()
            out = subprocess.run([sys.executable, os.path.join(HERE, "_stream_geometry_worker.py"), c["kind"], str(c["N"])],
                                 env=sg.child_env(c), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            assert out.returncode == 0, f"{cid}: exit status {out.returncode}\n" + out.stdout[-3000:] + out.stderr[-3000:]
            line = [l for l in out.stdout.splitlines() if l.startswith("STREAM_GEOM ")][-1]
            _outcomes[cid] = json.loads(line[len("STREAM_GEOM "):])
        except BaseException as e:
            _outcomes[cid] = e
            raise
    if isinstance(_outcomes[cid], BaseException):
        raise AssertionError(f"{cid} failed when it ran; it is not started again: {_outcomes[cid]!r:.2000}")
    return _outcomes[cid]


@pytest.mark.parametrize("c", [c for c in CHILDREN if c["kind"] == "forced"], ids=sg.child_id)
def test_forced_chunk_height_same_bits(c):
    """MG_RESIDENT_PCT=0 and MG_MAX_ROWS=r: rows_per_chunk = r plus the launcher's two roundings on any device and for any
    batch.  The child compared every output by bits; here: its count of comparisons, and every record against the
    restatement (the child asserted the same before it printed them)."""
    got = run_child(c)
    assert got["checks"] == sg.expected_checks(c) and got["r"] == c["r"]
    recs = got["records"]
    assert len(recs) >= got["checks"]
    for g in recs:
        assert (g["rows_per_chunk"], g["chunks"]) == sg.restated(g, c["r"]), g
        assert sg.last_chunk_rows(g) >= 1, g
    if c["r"]:
        # the knob took effect: no launch over more rows than the cap is one chunk
        assert all(g["chunks"] >= 2 for g in recs if g["own"] > c["r"] + 7)
        assert any(g["chunks"] >= 2 and g["own"] == c["N"] for g in recs)
    else:
        assert all(g["chunks"] == 1 for g in recs)
    if c["nt"]:   # the fused `1` nodes store U with non-temporal stores, across a seam
        assert any(g["flags"] & sg.NT and g["chunks"] == 2 and g["IN"] == sg.IN_PROLONG for g in recs)
        assert any(g["flags"] & sg.NT and g["PRE"] > 0 for g in recs) and any(g["flags"] & sg.NT and g["flags"] & sg.F32 for g in recs)
    elif int(sg.child_env(c)["MG_NT_MIN_N"]) > c["N"]:   # (the suite's threshold, 1024 unless the caller moved it)
        assert not any(g["flags"] & sg.NT for g in recs)


@pytest.mark.parametrize("c", [c for c in CHILDREN if c["kind"] == "batch"], ids=sg.child_id)
def test_batch_size_moves_the_seams_same_bits(c):
    """A small resident round and no row cap: chunks = resident / (groups * B), so the rows at which the seams fall change
    with the batch size -- and every instance still equals its single solve (asserted in the child).  Here: the finest
    level's launches of the five batch sizes really used at least three chunk heights."""
    got = run_child(c)
    assert got["checks"] == sg.expected_checks(c)
    top = [g for g in got["records"] if g["N"] == c["N"] and g["op"] == "BatchSolver"]
    assert {g["B"] for g in top} == set(sg.BATCH_SIZES)
    heights = {}
    for g in top:
        assert sg.last_chunk_rows(g) >= 1 and (g["chunks"] - 1) * g["rows_per_chunk"] < g["own"], g
        heights.setdefault(g["B"], set()).add(g["rows_per_chunk"])
    distinct = set().union(*heights.values())
    assert len(distinct) >= 3, f"rows_per_chunk per batch size: {heights}"
    assert any(g["chunks"] >= 2 for g in top if g["B"] == 1) and any(g["flags"] & sg.SH for g in top)


def test_every_geometry_class_for_every_family():
    """Over all children together: each geometry class for each kernel family, but for the pairs the launcher's arithmetic
    excludes at these sizes (test_stream_geometry_cpu.py derives them from the restatement and lists them).  A child that
    failed in its own case is not started again: this test then fails on its stored outcome."""
    from test_stream_geometry_cpu import EXCLUDED
    records = []
    for c in CHILDREN:
        records += run_child(c)["records"]
    seen = sg.pairs_seen(records)
    required = sg.ALL_PAIRS - set(EXCLUDED)
    assert len(required) >= 0.8 * len(sg.ALL_PAIRS)
    assert not required - seen, f"never recorded: {sorted(required - seen)}"
