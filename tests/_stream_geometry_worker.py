"""Child process of test_stream_geometry_gpu.py: the calls that run k_jacobi_stream under ONE chunk geometry, which the
parent forced through the environment (MG_RESIDENT_PCT, MG_MAX_ROWS: static per process; the tile kernel is switched off,
so the streaming kernel runs at these small sizes).  Every output array against the oracle or the restatement of the
existing test of that call, bit for bit; every launch's record (mg_stream_geometry_log) against the restated arithmetic of
the launcher (tests/_stream_geometry.py).  Prints one line "STREAM_GEOM {json}": the number of comparisons and the
distinct records, each with the call that made it.

argv: kind (forced | batch), N."""
import json
import os
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import multigrid_poisson_solver_amd as mg

import _oracle
import _oracle_f32 as o32
import _solve_ref as ref
import _solve_shift_ref as sref
import _stream_geometry as sg
from conftest import assert_bits
from test_memory_contract_gpu import KEYS
from test_mixed_gpu import bits32
from test_parity_gpu import REL, rand_pair

kind, N = sys.argv[1], int(sys.argv[2])
No, M = N - 1, N // 2
R_FORCED = int(os.environ.get("MG_MAX_ROWS", "0")) or None
assert os.environ["MG_TILE_MAX_N"] == "0" and os.environ["MG_TILE_SLAB_MAX_N"] == "0"
assert os.environ["MG_RESIDENT_PCT"] == ("0" if kind == "forced" else str(sg.BATCH_RESIDENT_PCT[N]))

mg.init(int(os.environ.get("MG_DEVICE", "0")))
oracle = _oracle.Oracle()
G = mg.DeviceGrid
out = {"kind": kind, "N": N, "r": R_FORCED, "checks": 0, "records": []}
seen = set()


def done(op, instances=None, **tags):
    """One comparison made.  Its launches: at least one of the streaming kernel, each cut as the launcher's arithmetic says
    (forced heights: exactly, on any device); batch-dependent children: a last chunk of at least one row."""
    recs = mg.stream_geometry_fetch()
    assert recs, f"{op}: no launch of the streaming kernel was recorded"
    for g in recs:
        assert g["rows_per_chunk"] >= 1 and g["chunks"] >= 1 and g["groups"] >= 1 and sg.last_chunk_rows(g) >= 1, (op, g)
        assert (g["chunks"] - 1) * g["rows_per_chunk"] < g["own"] <= g["N"], (op, g)
        if kind == "forced":
            assert (g["rows_per_chunk"], g["chunks"]) == sg.restated(g, R_FORCED), (op, R_FORCED, g)
        if instances is not None:
            assert g["instances"] == instances, (op, g)
        key = tuple(g[f] for f in sg.FIELDS) + (op,) + tuple(sorted(tags.items()))
        if key not in seen:
            seen.add(key)
            out["records"].append(dict(g, op=op, **tags))
    out["checks"] += 1


def smoothing(n):
    """mg_doSmoothing (test_smoothing_vs_oracle) and mg_smooth_pp (test_smoothing_fused_forms)"""
    U0, F = rand_pair(n, n)
    Fd = G.from_host(F)
    for step in range(1, 7):
        U = G.from_host(U0)
        err = mg.doSmoothing(n, 1.0, U, Fd, step)
        want, werr = oracle.doSmoothing(n, 1.0, U0, F, step)
        assert_bits(U.to_host(), want, f"doSmoothing N={n} step={step} r={R_FORCED}")
        assert err == pytest.approx(werr, rel=REL), (n, step)
        done("doSmoothing")
    for step in range(1, 5):
        o, D = G.from_host(np.full((n, n), np.nan)), G.from_host(np.full((n, n), np.nan))
        err = mg.smooth_pp(n, 1.0, None, o, Fd, step, want_error=True, D_out=D, d_sign=-1)
        want, werr = oracle.doSmoothing(n, 1.0, np.zeros((n, n)), F, step)
        assert_bits(o.to_host(), want, f"zero-start smoothing N={n} step={step} r={R_FORCED}")
        assert err == pytest.approx(werr, rel=REL)
        assert_bits(D.to_host(), -oracle.getResidual(n, 1.0, want, F), f"fused -residual N={n} step={step}")
        done("smooth_pp zero")
        Uin = G.from_host(U0)
        err = mg.smooth_pp(n, 1.0, Uin, o, Fd, step, want_error=True, D_out=D, d_sign=+1)
        want, werr = oracle.doSmoothing(n, 1.0, U0, F, step)
        assert_bits(o.to_host(), want, f"out-of-place smoothing N={n} step={step} r={R_FORCED}")
        assert err == pytest.approx(werr, rel=REL)
        assert_bits(D.to_host(), oracle.getResidual(n, 1.0, want, F), f"fused +residual N={n} step={step}")
        done("smooth_pp field")


def fused_nodes():
    """mg_smooth_restrict (test_fused_smooth_restrict_vs_oracle) and mg_prolong_smooth (test_fused_prolong_smooth_vs_oracle)"""
    U0, F = rand_pair(N, 11 * N + M)
    Fd = G.from_host(F)
    for step in range(1, 5):
        for zero in (True, False):
            want_U, want_err = oracle.doSmoothing(N, 1.0, np.zeros((N, N)) if zero else U0, F, step)
            want_Fc = oracle.doRestriction(N, -oracle.getResidual(N, 1.0, want_U, F), M)
            o, Fc = G.from_host(np.full((N, N), np.nan)), G.from_host(np.full((M, M), np.nan))
            Uin = None if zero else G.from_host(U0)
            err = mg.smooth_restrict(N, 1.0, Uin, o, Fd, step, M, Fc, want_error=True)
            assert_bits(o.to_host(), want_U, f"smooth_restrict U N={N} step={step} zero={zero} r={R_FORCED}")
            assert_bits(Fc.to_host(), want_Fc, f"smooth_restrict F_coarse {N}->{M} step={step} zero={zero} r={R_FORCED}")
            assert err == pytest.approx(want_err, rel=REL)
            done("smooth_restrict")
    rng = np.random.default_rng(13 * N + M)
    Uc, Uf, F = rng.random((M, M)) - 0.5, rng.random((N, N)), rng.random((N, N)) - 0.5
    Ucd, Ufd, Fd = G.from_host(Uc), G.from_host(Uf), G.from_host(F)
    for step in range(1, 5):
        want0 = oracle.doGridAddition(N, Uf, oracle.doProlongation(M, Uc, N, fill=0.0))
        want, want_err = oracle.doSmoothing(N, 1.0, want0, F, step)
        o = G.from_host(np.full((N, N), np.nan))
        err = mg.prolong_smooth(M, Ucd, N, 1.0, Ufd, o, Fd, step, want_error=True)
        assert_bits(o.to_host(), want, f"prolong_smooth {M}->{N} step={step} r={R_FORCED}")
        assert err == pytest.approx(want_err, rel=REL)
        done("prolong_smooth")


def fused_nodes_f32():
    """mg_smooth_restrict_f32 / mg_prolong_smooth_f32 (test_fused_nodes_fp32_vs_numpy)"""
    for step in range(1, 5):
        rng = np.random.default_rng(N + step)
        F = (rng.random((N, N)) - 0.5).astype(np.float32)
        Uc = (rng.random((M, M)) - 0.5).astype(np.float32)
        Uf = rng.random((N, N)).astype(np.float32)
        U, e = o32.smooth(np.zeros((N, N), dtype=np.float32), F, step, 1.0)
        want_Fc = o32.restrict_neg_residual(mg, U, F, 1.0, M)
        Fd, Uo, Fc = mg.DeviceGrid32.from_host(F), mg.DeviceGrid32((N, N)), mg.DeviceGrid32((M, M))
        err = mg.smooth_restrict_f32(N, 1.0, Uo, Fd, step, M, Fc, want_error=True)
        assert bits32(Uo.to_host(), U), f"fp32 smoothing N={N} step={step} r={R_FORCED}"
        assert err == pytest.approx(e, rel=1e-12)
        assert bits32(Fc.to_host(), want_Fc), f"fp32 fused restriction N={N} step={step} r={R_FORCED}"
        done("smooth_restrict_f32")
        want, e = o32.smooth(o32.prolong_add(mg, Uc, Uf), F, step, 1.0)
        o = mg.DeviceGrid32((N, N))
        err = mg.prolong_smooth_f32(M, mg.DeviceGrid32.from_host(Uc), N, 1.0, mg.DeviceGrid32.from_host(Uf), o, Fd, step, want_error=True)
        assert bits32(o.to_host(), want), f"fp32 prolong+smooth {M}->{N} step={step} r={R_FORCED}"
        assert err == pytest.approx(e, rel=1e-12)
        done("prolong_smooth_f32")


def check_cycle(got, U, want, what):
    """test_slab_gpu.check / test_cycle_gpu.check_against without the report"""
    assert got["status"] == 0 and want["status"] == 0
    assert_bits(U, want["U"], what + ": final U", zero_sign=True)
    assert got["mg_error"] == pytest.approx(want["mg_error"], rel=1e-10)
    assert len(got["records"]) == len(want["records"])
    for g, w in zip(got["records"], want["records"]):
        assert tuple(g[:3]) == tuple(w[:3])
        assert g[3] == pytest.approx(w[3], rel=1e-12, abs=1e-300)


def cycle_files():
    """Generated V-cycle files of 1, 2, 3 sweeps per node through the fused driver: the recomputing pair PRE = S = steps
    with the F ring in LDS on the levels from 128 on (test_other_sweep_counts_through_the_cycle_driver); the same files on
    fp32 fields, whose recomputing `1` node holds two columns per lane (test_mixed_cycle_other_sweep_counts_vs_numpy);
    then the 3-sweep file on virtual-rank slabs (test_virtual_slabs_vcycle_vs_oracle)."""
    assert all(mg.lib().mg_recompute_pair_available(s, s) == 1 for s in (1, 2, 3))
    tmp = tempfile.mkdtemp(prefix="mg_stream_geometry_")
    paths, wants = {}, {}
    for steps in (1, 2, 3):
        path = paths[steps] = os.path.join(tmp, f"V{N}_{steps}.txt")
        mg.write_vcycle_file(path, N, 8, steps, 1e-7)
        want = wants[steps] = oracle.run_cycle_file(path, want_report=False)
        plan = mg.CyclePlan(path, fused=True)
        got = plan.execute(fetch_U=True)
        check_cycle(got, got["U"], want, f"V-cycle N={N} steps={steps} r={R_FORCED}")
        plan.close()
        done("vcycle")
    for steps in (1, 2, 3):
        path = paths[steps]
        toks = open(path).read().split()
        U32, recs = o32.run_cycle_tokens(mg, oracle, oracle.getSource(N), 1.0, steps, ref.sizes(N, 8), toks[7:])
        plan = mg.CyclePlan(path, fused=True, mixed=True)
        got = plan.execute(fetch_U=True)
        assert got["status"] == 0
        assert bits32(got["U"].astype(np.float32), U32), f"mixed V-cycle N={N} steps={steps} r={R_FORCED}: fp32 result"
        assert len(got["records"]) == len(recs)
        for g, w in zip(got["records"], recs):
            assert (g[0], g[1]) == (w[0], w[1]) and g[3] == pytest.approx(w[2], rel=1e-10, abs=1e-300)
        plan.close()
        done("vcycle_f32")
    want = wants[sg.SLAB_STEPS]
    for R in sg.SLAB_RANKS:
        levels = mg.slab_partition(N, 8, R, sg.SLAB_COLLAPSE)
        assert not levels[0][1], f"N={N} R={R}: the finest level is not distributed"
        plan = mg.SlabPlan(paths[sg.SLAB_STEPS], R, -1, sg.SLAB_COLLAPSE)
        got = plan.execute()
        check_cycle(got, plan.gather_U(N), want, f"slab V-cycle N={N} R={R} r={R_FORCED}")
        plan.close()
        done("slab", R=R)
    for path in paths.values():
        os.remove(path)
    os.rmdir(tmp)


def solver_problems(n, pp, shift, count):
    return [ref.random_problem(n, 1000 + n + 97 * i + 7 * pp[0] + (13 if shift else 0)) for i in range(count)]


def solvers(n):
    """One cycle of Solver against the restatement (test_cycles_bit_identical_to_restatement, shift:
    test_solve_shift_gpu.against_restatement), then BatchSolver with B = 3 against the single solves
    (test_batch_solver_on_one_packed_block's comparison)."""
    for pp in sg.SOLVER_SWEEPS:
        for shift in sg.SOLVER_SHIFTS:
            opts = dict(pre=pp[0], post=pp[1], omega=0.8, rtol=0.0, atol=0.0, max_cycles=1)
            if shift:
                opts["shift"] = shift
            what = f"N={n} V{pp} shift={shift:g} r={R_FORCED}"
            probs = solver_problems(n, pp, shift, 3)
            margins = []
            if shift:
                want = sref.cycle(oracle, *probs[0], 1.0, margins=margins, pre=pp[0], post=pp[1], omega=0.8, shift=shift)
            else:
                want = ref.cycle(oracle, *probs[0], 1.0, margins=margins, pre=pp[0], post=pp[1], omega=0.8)
            ref.assert_qualified(margins, what)
            s = mg.Solver(n, 1.0, **opts)
            singles = []
            for i, (F, U0) in enumerate(probs):
                U, info = s.solve(F, U0)
                assert info["cycles"] == 1 and info["status"] == mg.MG_SOLVE_NOT_CONVERGED and not info["coarse_capped"], what
                singles.append((U, info))
                if i == 0:
                    assert_bits(U, want, what + ": Solver after one cycle", zero_sign=True)
                    done("Solver", instances=1, shift=int(shift))
                else:
                    mg.stream_geometry_fetch()
            s.close()
            bs = mg.BatchSolver(n, 1.0, max_batch=3, **opts)
            Us, infos = bs.solve(np.stack([p[0] for p in probs]), np.stack([p[1] for p in probs]))
            bs.close()
            for i, (U, info) in enumerate(singles):
                assert_bits(Us[i], U, f"{what}: BatchSolver instance {i} U")
                for k in KEYS:
                    assert infos[i][k] == info[k], f"{what} instance {i} {k}: {infos[i][k]} != {info[k]}"
            done("BatchSolver", instances=3, shift=int(shift))


def batch_sizes():
    """The batch-dependent child: resident / (groups * B) chunks, so the chunk height follows B.  BatchSolver with
    B = 1, 2, 3, 8, 32 on random problems, for B >= 3 the middle instance converged at the start (as
    test_batch_solver_on_one_packed_block builds it); every instance against Solver on it alone."""
    for shift in sg.SOLVER_SHIFTS:
        opts = dict(rtol=0.0, atol=1e-2, max_cycles=2)
        if shift:
            opts["shift"] = shift
        s = mg.Solver(N, 1.0, **opts)
        single = {}   # (the problems of the batch sizes overlap: one single solve per seed)
        for B in sg.BATCH_SIZES:
            mid = B // 2 if B >= 3 else -1
            seeds = [700 + N + 97 * i for i in range(B)]
            probs = [ref.random_problem(N, seed) for seed in seeds]
            if mid >= 0:
                # F = A U + d with |d| <= 5e-4 / N: a residual norm of about 3e-4 < atol, yet one sweep would change U
                F_mid, U_mid = probs[mid]
                probs[mid] = (sref.residual(N, 1.0, U_mid, np.zeros((N, N)), shift) + F_mid * (1e-3 / N), U_mid)
            mg.stream_geometry_fetch()
            bs = mg.BatchSolver(N, 1.0, max_batch=B, **opts)
            Us, infos = bs.solve(np.stack([p[0] for p in probs]), np.stack([p[1] for p in probs]))
            bs.close()
            batch_recs = mg.stream_geometry_fetch()
            for i, (F, U0) in enumerate(probs):
                key = ("mid", i, B) if i == mid else seeds[i]
                if key not in single:
                    single[key] = s.solve(F, U0)
                want_U, want = single[key]
                what = f"N={N} B={B} shift={shift:g} instance {i}"
                assert_bits(Us[i], want_U, what + " U")
                if i == mid:
                    assert_bits(Us[i], U0, what + " U of the converged start")
                    assert infos[i]["cycles"] == 0 and infos[i]["converged"], what
                else:
                    assert infos[i]["cycles"] == 2, what
                for k in KEYS:
                    assert infos[i][k] == want[k], f"{what} {k}: {infos[i][k]} != {want[k]}"
            mg.stream_geometry_fetch()   # (the single solves)
            # the batch's own launches: the active instances (all but the converged middle one) share each of them
            active = B - (1 if mid >= 0 else 0)
            assert batch_recs and all(g["instances"] == active for g in batch_recs), (B, batch_recs[:3])
            for g in batch_recs:
                assert sg.last_chunk_rows(g) >= 1 and g["rows_per_chunk"] >= 1, g
                key = tuple(g[f] for f in sg.FIELDS) + (B, shift)
                if key not in seen:
                    seen.add(key)
                    out["records"].append(dict(g, op="BatchSolver", B=B, shift=int(shift)))
            out["checks"] += 1
        s.close()


mg.stream_geometry_log(True)
if kind == "forced":
    smoothing(N)
    smoothing(No)
    fused_nodes()
    fused_nodes_f32()
    cycle_files()
    solvers(N)
    solvers(No)
else:
    batch_sizes()
mg.stream_geometry_log(False)
assert mg.stream_geometry_fetch() == []
print("STREAM_GEOM " + json.dumps(out), flush=True)
mg.finalize()
