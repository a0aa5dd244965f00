"""The case table of test_stream_geometry_gpu.py, checked on the host before anyone has a GPU: with the restatement of
the launcher's arithmetic and a model of the launches the children make (tests/_stream_geometry.py), the forced chunk
heights put every kernel family into every geometry class it can be in."""
import os

import pytest

import _stream_geometry as sg

# (class, family) pairs the children are NOT required to record: the launcher's arithmetic excludes them at these sizes,
# whatever the height.  The test below derives the same set from the restatement.
EXCLUDED = {
    # a last chunk of one row needs an odd chunk height: one column per lane, which the fused transfer stages, the fp32
    # forms met here and the (even) distributed levels of a slab plan never run
    ("last_chunk_1", "RESTRICT"), ("last_chunk_1", "IN_PROLONG"), ("last_chunk_1", "IN_PROLONG_PRE"),
    ("last_chunk_1", "F32_COLS2"), ("last_chunk_1", "F32_COLS4"), ("last_chunk_1", "SLAB"),
    # four columns per lane: strips of 240 or 248 columns, N = 484 is three of them at most -- one workgroup.  An exclusion
    # of the SIZES, not of the kernel: the four-column form with a second workgroup per chunk row (dead waves next to a
    # seam) needs N > 960 and is not compared point by point here (DESIGN 3.1 says so)
    ("groups_2", "F32_COLS4"),
}


@pytest.fixture(scope="module")
def slab_windows():
    """rows of the `-1` launches on the finest level of the children's slab plans (mg_slab_schedule, host only; the
    library's default communication-avoiding mode, which the children run with)"""
    import multigrid_poisson_solver_amd as m
    if not os.path.exists(m.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = {}
    for N, _ in sg.PAIRS:
        rows = set()
        for R in sg.SLAB_RANKS:
            assert not m.slab_partition(N, 8, R, sg.SLAB_COLLAPSE)[0][1], f"N={N} R={R}: the finest level is not distributed"
            top = m.slab_schedule(N, 8, R, sg.SLAB_COLLAPSE, sg.SLAB_STEPS, 1, 10)[0]
            assert top["N"] == N and not top["collapsed"]
            rows |= {hi - lo for lo, hi in top["dext"]}
        assert rows and all(0 < w < N for w in rows)
        out[N] = sorted(rows)
    return out


def test_restatement_on_hand_computed_launches():
    # plain rows: even for column pairs, as capped for single columns
    assert sg.restate_launch_k(132, None, 3, 0, 2, False) == (132, 1)
    assert sg.restate_launch_k(132, 130, 3, 0, 2, False) == (130, 2)
    assert sg.restate_launch_k(131, 130, 3, 0, 1, False) == (130, 2)
    assert sg.restate_launch_k(131, 65, 3, 0, 1, False) == (65, 3)
    assert sg.restate_launch_k(483, 241, 2, 0, 1, False) == (241, 3)
    assert sg.restate_launch_k(44, 6, 3, 0, 2, False) == (6, 8)
    assert sg.restate_launch_k(33, 66, 3, 0, 2, False) == (34, 1)      # an odd window: rounded past its own rows
    # the LDS ring: rows + 2 (S + PRE + 1) is a multiple of 8
    assert sg.restate_launch_k(132, 2, 1, 1, 2, True) == (2, 66)       # march 8
    assert sg.restate_launch_k(132, 2, 2, 2, 2, True) == (6, 22)       # march 12 -> 16
    assert sg.restate_launch_k(132, 2, 3, 3, 2, True) == (2, 66)       # march 16
    assert sg.restate_launch_k(484, 482, 1, 1, 2, True) == (482, 2)    # march 488
    assert sg.restate_launch_k(484, 6, 3, 3, 2, True) == (10, 49)      # march 20 -> 24
    assert sg.lds_ring(2, 1, False) and sg.lds_ring(4, 1, True) and not sg.lds_ring(4, 1, False) and not sg.lds_ring(2, 0, False)
    # strips: 64 lanes of COLS columns less two halos; four strips per workgroup
    assert (sg.halo(3, False, 2), sg.halo(3, True, 2), sg.halo(6, False, 2), sg.halo(3, False, 1), sg.halo(3, True, 4)) == (4, 6, 8, 4, 8)
    assert sg.groups_of(132, 3, 0, 2, 0) == 1 and sg.groups_of(484, 3, 0, 2, 0) == 2 and sg.groups_of(483, 3, 0, 1, 0) == 3
    assert sg.groups_of(484, 3, 0, 4, 1) == 1


def test_the_table_of_children():
    cs = sg.children()
    forced = [c for c in cs if c["kind"] == "forced"]
    assert len(forced) == 16 and len(cs) == 18 and len({sg.child_id(c) for c in cs}) == 18
    for c in forced:
        N = c["N"]
        assert N % 4 == 0 and (N, N - 1) in sg.PAIRS
        # only heights the launcher could choose by itself on some device or batch
        assert c["r"] is None or sg.min_rows(N) <= c["r"] <= N
        env = sg.child_env(c, base={"MG_LIB": "x", "MG_MIN_ROWS": "9", "MG_SMOOTHER": "simple", "HOME": "/h"})
        assert env["MG_RESIDENT_PCT"] == "0" and env.get("MG_MAX_ROWS") == (str(c["r"]) if c["r"] else None)
        assert env["MG_LIB"] == "x" and env["HOME"] == "/h" and "MG_MIN_ROWS" not in env and "MG_SMOOTHER" not in env
        assert (env["MG_TILE_MAX_N"], env["MG_TILE_SLAB_MAX_N"], env["MG_RECOMPUTE_MIN_N"], env["MG_F32_COLS4_MIN_N"]) == ("0", "0", "128", "128")
        assert env["MG_NT_MIN_N"] == ("128" if c["nt"] else "1024")
    assert sorted(c["r"] for c in forced if c["nt"]) == [66, 242]
    for N, No in sg.PAIRS:
        assert sg.forced_heights(N) == [None, sg.min_rows(N), 6, N // 2 - 2, N // 2, N // 2 + 2, N - 2] and No == N - 1
    for c in cs:
        if c["kind"] == "batch":
            env = sg.child_env(c, base={})
            assert "MG_MAX_ROWS" not in env
            # 256 CUs, 1..8 blocks per CU: at least three chunk heights over the five batch sizes on the finest level
            groups = sg.groups_of(c["N"], 3, 0, 2, 1)
            for per_cu in range(1, 9):
                resident = 256 * per_cu * int(env["MG_RESIDENT_PCT"]) // 100
                heights = set()
                for B in sg.BATCH_SIZES:
                    chunks = max(1, min(resident // (groups * B), sg.ceil_div(c["N"], sg.min_rows(c["N"]))))
                    rows = sg.ceil_div(c["N"], chunks)
                    heights.add(rows + (rows & 1))
                assert len(heights) >= 3, (c["N"], per_cu, heights)


def test_every_class_for_every_family_that_can_have_it(slab_windows):
    hit, reachable = set(), set()
    for N, _ in sg.PAIRS:
        reachable |= sg.reachable_pairs(N, slab_windows[N])
        for r in sg.forced_heights(N):
            recs = sg.model_records(N, r, slab_windows[N])
            for g in recs:   # every predicted last chunk holds at least one row
                assert 1 <= sg.last_chunk_rows(g) <= g["rows_per_chunk"] and g["chunks"] >= 1, (r, g)
            hit |= sg.pairs_seen(recs)
    assert sg.ALL_PAIRS - reachable == EXCLUDED
    assert reachable == hit
    required = sg.ALL_PAIRS - EXCLUDED
    assert required <= hit
    assert len(sg.ALL_PAIRS) == 6 * 11 and len(required) >= 0.8 * len(sg.ALL_PAIRS)
