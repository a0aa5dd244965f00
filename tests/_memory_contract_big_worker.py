"""Child process of test_memory_contract_gpu.py::test_product_thresholds_in_guarded_blocks: the operators, the two fused
nodes (in both smoothers) and two solver cycles at N x N with the library's own thresholds (the caller removed the MG_* overrides of the test
suite), on mg_fill_uniform inputs placed in guarded blocks (tests/_guard.py; both placements).  Every call is followed by
check(): bands and read-only inputs by device checksum before / after.  Outputs that tests/golden/golden_fullsize.json
pins are printed as checksums for the parent; the others are compared here with the same call on plain mg_alloc arrays."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import multigrid_poisson_solver_amd as mg

import _guard

mg.init(0)
N = int(sys.argv[1])
M = N // 2
out = {"N": N, "checks": 0}
plain = {}


def same(key, value):
    """the first placement records, the others (and the plain arrays) must agree"""
    value = list(value)
    assert plain.setdefault(key, value) == value, f"{key}: {value} != {plain[key]}"


def on_plain_arrays():
    G = mg.DeviceGrid
    U, F, D, C = G.uniform(N, 11), G.uniform(N, 22), G(N), G(M)
    mg.doSmoothing(N, 1.0, U, F, 1, want_error=False)
    same("smooth1", U.checksum())
    F.free(); F = G.uniform(N, 7)
    mg.smooth_restrict(N, 1.0, None, U, F, 3, M, C)
    same("node_down_U", U.checksum()); same("node_down_Fc", C.checksum())
    C.free(); C = G.uniform(M, 8)
    mg.prolong_smooth(M, C, N, 1.0, U, D, F, 3)
    same("node_up", D.checksum())
    mg.lib().mg_fill_zero(U.ptr, U.size)
    s = mg.Solver(N, 1.0, rtol=0.0, atol=0.0, max_cycles=2)
    info = s.solve_ptr(F.ptr, U.ptr)
    s.close()
    same("solve_U", U.checksum()); same("solve_history", info["history"])
    for g in (U, F, D, C):
        g.free()
    mg.lib().mg_pool_trim()


on_plain_arrays()
for place in _guard.PLACEMENTS:
    b = _guard.block(mg, [N, N, N, M], place)
    assert b.big
    U, F, D, C = b.views

    def done(what):
        b.check(f"{what} N={N} ({place})")
        out["checks"] += 1

    U.fill_uniform(11); F.fill_uniform(22)
    b.expect_readonly(U, F)
    mg.getResidual(N, 1.0, U, F, D)
    same("residual", D.checksum())
    done("mg_getResidual")
    b.expect_readonly(F, D)
    mg.doSmoothing(N, 1.0, U, F, 1, want_error=False)
    same("smooth1", U.checksum())
    done("mg_doSmoothing(1)")
    U.fill_uniform(11)
    b.expect_readonly(F, D)
    err = mg.doSmoothing(N, 1.0, U, F, 3)
    same("smooth3", U.checksum())
    plain.setdefault("smooth3_err", [err])   # (a norm: the parent holds it to 1e-12 of the reference's)
    done("mg_doSmoothing(3)")
    # the same three sweeps one launch per sweep (k_jacobi_pair / k_jacobi_pair_rows on even N): the same bits
    U.fill_uniform(11)
    mg.set_smoother("simple")
    b.expect_readonly(F, D)
    mg.doSmoothing(N, 1.0, U, F, 3, want_error=False)
    mg.set_smoother("stream")
    same("smooth3", U.checksum())
    done("mg_doSmoothing(3, simple)")
    U.fill_uniform(33)
    b.expect_readonly(U, F, D)
    mg.doRestriction(N, U, M, C)
    same("restrict", C.checksum())
    done("mg_doRestriction")
    C.fill_uniform(44)
    mg.lib().mg_fill_zero(U.ptr, U.size)
    b.expect_readonly(C, F, D)
    mg.doProlongation(M, C, N, U)
    same("prolong", U.checksum())
    done("mg_doProlongation")
    # the two fused nodes and the solver, as on_plain_arrays()
    U.fill_uniform(11); F.fill_uniform(22)
    mg.doSmoothing(N, 1.0, U, F, 1, want_error=False)
    F.fill_uniform(7)
    b.expect_readonly(F, D)
    mg.smooth_restrict(N, 1.0, None, U, F, 3, M, C)
    same("node_down_U", U.checksum()); same("node_down_Fc", C.checksum())
    done("mg_smooth_restrict")
    C.fill_uniform(8)
    b.expect_readonly(C, U, F)
    mg.prolong_smooth(M, C, N, 1.0, U, D, F, 3)
    same("node_up", D.checksum())
    done("mg_prolong_smooth")
    # the two nodes operator by operator (simple smoother: k_residual_pairs on pool scratch, k_prolong_pairs)
    mg.set_smoother("simple")
    C.fill_uniform(9); D.fill_uniform(10)
    b.expect_readonly(F, D)
    mg.smooth_restrict(N, 1.0, None, U, F, 3, M, C)
    same("node_down_U", U.checksum()); same("node_down_Fc", C.checksum())
    done("mg_smooth_restrict (simple)")
    C.fill_uniform(8)
    b.expect_readonly(C, U, F)
    mg.prolong_smooth(M, C, N, 1.0, U, D, F, 3)
    mg.set_smoother("stream")
    same("node_up", D.checksum())
    done("mg_prolong_smooth (simple)")
    mg.lib().mg_fill_zero(U.ptr, U.size)
    s = mg.Solver(N, 1.0, rtol=0.0, atol=0.0, max_cycles=2)
    b.expect_readonly(F, C, D)
    info = s.solve_ptr(F.ptr, U.ptr)
    s.close()
    same("solve_U", U.checksum()); same("solve_history", info["history"])
    done("mg_solver_solve")
    b.free()
    mg.lib().mg_pool_trim()

for k in ("residual", "smooth3", "restrict", "prolong"):   # (the parent compares the ones the golden file pins)
    out[k] = plain[k]
out["smooth3_err"] = plain["smooth3_err"][0]
print("MEMORY_BIG " + json.dumps(out), flush=True)
mg.finalize()
