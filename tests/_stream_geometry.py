"""The chunk geometry of the streaming smoother, restated on the host (TEST INFRASTRUCTURE): what launch_k
(csrc/mg_stream_impl.h) makes of a forced chunk height, the geometry classes and kernel families the tests of
test_stream_geometry_gpu.py must see, the table of child processes that force them, and a model of the launches those
children make -- test_stream_geometry_cpu.py checks the table against the model before anyone has a GPU, the GPU test
holds the records of the real launches (mg_stream_geometry_log) to the same restatement.

launch_k, with `resident` workgroups in one round of the device:
    chunks = clamp(resident / (groups * instances), 1, ceil(own / min_rows(N)))
    rows   = ceil(own / chunks), capped by MG_MAX_ROWS, then rounded: with the F ring in LDS (the recomputing `1` node) so
             that the march of rows + 2 (S + PRE + 1) steps is a multiple of 8, else to even when a lane holds column pairs
    chunks = ceil(own / rows)
MG_RESIDENT_PCT=0 makes resident 0, hence chunks 1 and rows = own before the cap: MG_MAX_ROWS=r then decides alone."""
import os

WAVES_PER_WG = 4
NT, WT, SH, F32 = 1, 2, 4, 8                       # flags of a record (include/mg_hip.h: MG_GEOMETRY_*)
IN_LOAD, IN_ZERO, IN_PROLONG = 0, 1, 2
FIELDS = ("N", "own", "rows_per_chunk", "chunks", "groups", "instances", "S", "COLS", "IN", "RESTRICT", "PRE", "flags")


def ceil_div(a, b):
    return -(-a // b)


def min_rows(N):
    return 2 if N <= 256 else 4 if N <= 1024 else 8


def halo(S, restrict, cols):
    """Halo<S, RESTRICT, COLS>::value: halo columns per side of a strip"""
    a = max(cols, 2)
    return (S + (2 if restrict else 1) + a - 1) // a * a


def groups_of(N, S, PRE, COLS, RESTRICT):
    ow = 64 * COLS - 2 * halo(S + PRE, RESTRICT, COLS)
    return ceil_div(ceil_div(N, ow), WAVES_PER_WG)


def lds_ring(COLS, PRE, f32):
    """LdsRing<COLS, PRE>::value"""
    return PRE > 0 and (COLS == 2 or (COLS == 4 and f32))


def restate_launch_k(own, r, S, PRE, COLS, lds_ring):
    """(rows_per_chunk, chunks) of a launch over `own` rows with MG_RESIDENT_PCT=0 and MG_MAX_ROWS=r (None: unset)"""
    rows = own if not r else min(own, r)
    if lds_ring:
        rows += (8 - (rows + 2 * (S + PRE + 1)) % 8) % 8
    elif COLS >= 2:
        rows += rows & 1
    return rows, ceil_div(own, rows)


def last_chunk_rows(rec):
    return rec["own"] - (rec["chunks"] - 1) * rec["rows_per_chunk"]


def restated(rec, r):
    """what the record of a forced-height child must hold in rows_per_chunk and chunks"""
    return restate_launch_k(rec["own"], r, rec["S"], rec["PRE"], rec["COLS"], lds_ring(rec["COLS"], rec["PRE"], bool(rec["flags"] & F32)))


# ---------------------------------------------------------------- geometry classes and kernel families of a record
CLASSES = {
    "one_chunk": lambda g: g["chunks"] == 1,
    "min_rows": lambda g: g["rows_per_chunk"] == min_rows(g["N"]),
    "shorter_than_halo": lambda g: g["rows_per_chunk"] < g["S"] + g["PRE"] + 1,
    "two_chunks_last_2": lambda g: g["chunks"] == 2 and last_chunk_rows(g) == 2,
    "last_chunk_1": lambda g: g["chunks"] >= 2 and last_chunk_rows(g) == 1 and g["COLS"] == 1,
    "groups_2": lambda g: g["groups"] >= 2,
}


def _plain(g):   # the unweighted fp64 kernel on one whole grid
    return not (g["flags"] & (WT | SH | F32)) and g["instances"] == 1 and g["own"] == g["N"]


FAMILIES = {
    "IN_LOAD": lambda g: _plain(g) and g["IN"] == IN_LOAD and not g["RESTRICT"],
    "IN_ZERO": lambda g: _plain(g) and g["IN"] == IN_ZERO and not g["RESTRICT"],
    "RESTRICT": lambda g: _plain(g) and g["RESTRICT"],
    "IN_PROLONG": lambda g: _plain(g) and g["IN"] == IN_PROLONG and g["PRE"] == 0,
    "IN_PROLONG_PRE": lambda g: _plain(g) and g["IN"] == IN_PROLONG and g["PRE"] > 0,
    "WT": lambda g: bool(g["flags"] & WT) and not g["flags"] & SH,
    "SH": lambda g: bool(g["flags"] & SH),
    "F32_COLS2": lambda g: bool(g["flags"] & F32) and g["COLS"] == 2,
    "F32_COLS4": lambda g: bool(g["flags"] & F32) and g["COLS"] == 4,
    "BATCH": lambda g: g["instances"] > 1,
    "SLAB": lambda g: g["own"] < g["N"],
}
ALL_PAIRS = {(c, f) for c in CLASSES for f in FAMILIES}


def pairs_seen(records):
    """the (class, family) pairs a list of records holds"""
    seen = set()
    for g in records:
        cs = [c for c, is_c in CLASSES.items() if is_c(g)]
        seen.update((c, f) for f, is_f in FAMILIES.items() if is_f(g) for c in cs)
    return seen


# ---------------------------------------------------------------- the table of children
PAIRS = [(132, 131), (484, 483)]    # an even size (a multiple of 4 with a fusable N -> N/2) and its odd partner N - 1
SLAB_RANKS = (2, 3)
SLAB_COLLAPSE = 64                  # (test_virtual_slabs_vcycle_vs_oracle's; an odd level is collapsed whatever it is)
SLAB_STEPS = 3
SOLVER_SWEEPS = [(3, 3), (2, 1)]
SOLVER_SHIFTS = [0.0, 1e2]
BATCH_SIZES = [1, 2, 3, 8, 32]
# MG_RESIDENT_PCT of the batch-dependent children: resident = 256 CUs * (1..8 blocks per CU) * pct / 100 workgroups, shared
# by groups * B workgroups per chunk row.  One group at N = 132, two at N = 484: with 2 and 4 per cent a single solve gets
# at least 5 chunks and B = 2 at least 2 at the lowest occupancy, B = 32 one chunk at the highest -- three heights or more
# whatever the occupancy query returns (1 per cent gives only two of them at one block per CU).
BATCH_RESIDENT_PCT = {132: 2, 484: 4}


def forced_heights(N):
    """MG_MAX_ROWS of the forced-height children of the pair (N, N - 1); N - 2 = (N - 1) - 1 leaves the odd partner a last
    chunk of one row; N / 2 - 2 does to the N / 2-row windows of a two-slab plan what N - 2 does to the whole grid"""
    return [None, min_rows(N), 6, N // 2 - 2, N // 2, N // 2 + 2, N - 2]


def children():
    out = []
    for N, _ in PAIRS:
        out += [dict(kind="forced", N=N, r=r, nt=False) for r in forced_heights(N)]
        out.append(dict(kind="forced", N=N, r=N // 2, nt=True))
    out += [dict(kind="batch", N=N, r=None, nt=False) for N, _ in PAIRS]
    return out


def child_id(c):
    return f"{c['kind']}-N{c['N']}-r{c['r'] or 'unset'}" + ("-nt" if c["nt"] else "")


def child_env(c, base=None):
    """The environment of a child: the caller's without its MG_* knobs (the library, the device and the runtime choice
    stay), then the knobs of the case."""
    base = os.environ if base is None else base
    env = {k: v for k, v in base.items() if not (k.startswith("MG_") and k not in ("MG_LIB", "MG_DEVICE", "MG_HIP_RUNTIME"))}
    env.update(MG_TILE_MAX_N="0", MG_TILE_SLAB_MAX_N="0", MG_RECOMPUTE_MIN_N="128", MG_F32_COLS4_MIN_N="128", MG_SLAB_POISON="1",
               MG_NT_MIN_N="128" if c["nt"] else base.get("MG_NT_MIN_N", "1024"))
    if c["kind"] == "forced":
        env["MG_RESIDENT_PCT"] = "0"
        if c["r"]:
            env["MG_MAX_ROWS"] = str(c["r"])
    else:
        env["MG_RESIDENT_PCT"] = str(BATCH_RESIDENT_PCT[c["N"]])
    return env


def expected_checks(c):
    """the comparisons a child counts (tests/_stream_geometry_worker.py, one per call under test)"""
    if c["kind"] == "batch":
        return len(BATCH_SIZES) * len(SOLVER_SHIFTS)
    smoothing = 2 * 6                      # both sizes, steps 1..6
    smooth_pp = 2 * 4 * 2                  # both sizes, steps 1..4, from zero and from a field
    nodes = 4 * 2 + 4                      # mg_smooth_restrict (zero, loaded), mg_prolong_smooth
    cycles = 3 + 3                         # V-cycle files of 1, 2, 3 sweeps in fp64 and on fp32 fields
    nodes_f32 = 4 * 2
    solver = 2 * len(SOLVER_SWEEPS) * len(SOLVER_SHIFTS) * 2    # both sizes; one Solver cycle, then BatchSolver with B = 3
    return smoothing + smooth_pp + nodes + cycles + nodes_f32 + solver + len(SLAB_RANKS)


# ---------------------------------------------------------------- a model of the launches of a forced-height child
def _rec(N, own, r, S, COLS, IN, RESTRICT=0, PRE=0, flags=0, instances=1):
    rows, chunks = restate_launch_k(own, r, S, PRE, COLS, lds_ring(COLS, PRE, bool(flags & F32)))
    return dict(N=N, own=own, rows_per_chunk=rows, chunks=chunks, groups=groups_of(N, S, PRE, COLS, RESTRICT), instances=instances,
                S=S, COLS=COLS, IN=IN, RESTRICT=RESTRICT, PRE=PRE, flags=flags)


def model_records(N, r, slab_windows):
    """The launches on the finest level that the calls of a forced-height child of the pair (N, N - 1) are known to make
    (a subset of what it records: coarser levels of the cycles and solvers are left out), as records with the restated
    geometry.  slab_windows: the row counts of the `-1` launches of the slab plans on level N (mg_slab_schedule: dext)."""
    out = []
    for n in (N, N - 1):
        cols = 2 if n % 2 == 0 else 1
        for S in (1, 2, 3, 4):   # mg_doSmoothing (5 and 6 sweeps: launches of 1 and 2) and mg_smooth_pp
            out.append(_rec(n, n, r, S, cols, IN_LOAD))
            out.append(_rec(n, n, r, S, cols, IN_ZERO))
        for pre, post in SOLVER_SWEEPS:
            for fl in (WT, WT | SH):
                for inst in (1, 3):
                    if cols == 2:   # the fused `-1` node from the caller's U, the fused `1` node
                        out.append(_rec(n, n, r, pre, 2, IN_LOAD, RESTRICT=1, flags=fl, instances=inst))
                        out.append(_rec(n, n, r, post, 2, IN_PROLONG, flags=fl, instances=inst))
                    else:           # the sweeps alone, the transfers operator by operator
                        out.append(_rec(n, n, r, pre, 1, IN_LOAD, flags=fl, instances=inst))
                        out.append(_rec(n, n, r, post, 1, IN_LOAD, flags=fl, instances=inst))
    for S in (1, 2, 3, 4):
        out.append(_rec(N, N, r, S, 2, IN_ZERO, RESTRICT=1))
        out.append(_rec(N, N, r, S, 2, IN_LOAD, RESTRICT=1))
        out.append(_rec(N, N, r, S, 2, IN_PROLONG))
        out.append(_rec(N, N, r, S, 4, IN_ZERO, RESTRICT=1, flags=F32))
        out.append(_rec(N, N, r, S, 4, IN_PROLONG, flags=F32))
    for S in (1, 2, 3):          # the recomputing `1` node of the V-cycle files: fp64, and fp32 fields (two columns per lane)
        out.append(_rec(N, N, r, S, 2, IN_PROLONG, PRE=S))
        out.append(_rec(N, N, r, S, 2, IN_PROLONG, PRE=S, flags=F32))
    for own in slab_windows:
        out.append(_rec(N, own, r, SLAB_STEPS, 2, IN_ZERO, RESTRICT=1))
    return out


def reachable_pairs(N, slab_windows):
    """the pairs some admissible height min_rows(N) <= r <= N (or none) gives a modelled launch of the pair (N, N - 1)"""
    seen = set()
    for r in [None] + list(range(min_rows(N), N + 1)):
        seen |= pairs_seen(model_records(N, r, slab_windows))
    return seen
