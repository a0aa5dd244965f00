"""multigrid_poisson_solver_amd -- Python harness over the C ABI of libmgpoisson.so.

The product is the HIP library (csrc/, built by build.py) behind include/mg_hip.h; this
module only binds it with ctypes for the tests and the benchmark.  It mirrors the
reference's operator interface (src/MG_solver_CPU.cpp:23-28: getResidual,
doGridAddition, doSmoothing, doExactSolver, doRestriction, doProlongation) on
device-resident arrays.  There is no CPU fallback: importing works anywhere, but the
first call raises if the library or a HIP device is missing.
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MG_LIB") or os.path.join(_PKG, "lib", "libmgpoisson.so")  # MG_LIB: A/B builds
EXE_PATH = os.path.join(_PKG, "bin", "MG_HIP")

MG_CYCLE_FUSED, MG_CYCLE_GRAPH, MG_CYCLE_REPORT, MG_CYCLE_ERROR, MG_CYCLE_MIXED = 1, 2, 4, 8, 16


class MGError(RuntimeError):
    pass


class NodeRecord(C.Structure):
    _fields_ = [("node", C.c_int), ("N", C.c_int), ("steps", C.c_int), ("error", C.c_double)]


class ProfileEntry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("N", C.c_int), ("launches", C.c_int), ("total_ms", C.c_double),
                ("algo_bytes", C.c_double)]


class CycleResult(C.Structure):
    _fields_ = [("status", C.c_int), ("N", C.c_int), ("U_dev", C.c_void_p), ("mg_error", C.c_double),
                ("time_ms", C.c_double), ("device_ms", C.c_double), ("n_records", C.c_int),
                ("records", C.POINTER(NodeRecord)), ("report", C.c_char_p), ("graph_replayed", C.c_int),
                ("schedule_launches", C.c_int)]


_vp, _i, _d, _sz, _u64 = C.c_void_p, C.c_int, C.c_double, C.c_size_t, C.c_uint64
_dptr = C.POINTER(C.c_double)


class SolveOpts(C.Structure):
    _fields_ = [("pre", C.c_int), ("post", C.c_int), ("N_min", C.c_int), ("omega", C.c_double), ("coarse_rtol", C.c_double),
                ("coarse_atol", C.c_double), ("coarse_max_iters", C.c_int), ("rtol", C.c_double), ("atol", C.c_double),
                ("max_cycles", C.c_int), ("fmg", C.c_int), ("shift", C.c_double)]   # (fmg fills the hole before shift)


class SolveResult(C.Structure):
    _fields_ = [("status", C.c_int), ("cycles", C.c_int), ("converged", C.c_int), ("coarse_capped", C.c_int),
                ("res0", C.c_double), ("res", C.c_double), ("ref_norm", C.c_double), ("device_ms", C.c_double),
                ("n_history", C.c_int), ("history", _dptr)]


class BatchSolveStats(C.Structure):
    _fields_ = [("cycles", C.c_int), ("launches", C.c_int), ("device_ms", C.c_double)]


class EigsOpts(C.Structure):
    _fields_ = [("cycle", SolveOpts), ("k", C.c_int), ("guard", C.c_int), ("max_iters", C.c_int), ("rtol", C.c_double),
                ("atol", C.c_double)]


class EigsResult(C.Structure):
    _fields_ = [("status", C.c_int), ("iters", C.c_int), ("converged", C.c_int), ("breakdown", C.c_int), ("restarts", C.c_int),
                ("cycles", C.c_int), ("coarse_capped", C.c_int)]


class HeatOpts(C.Structure):
    _fields_ = [("nu", C.c_double), ("dt", C.c_double), ("theta", C.c_double), ("solve", SolveOpts)]


class HeatResult(C.Structure):
    _fields_ = [("status", C.c_int), ("steps", C.c_int), ("cycles", C.c_int), ("coarse_capped", C.c_int),
                ("res", C.c_double), ("ref_norm", C.c_double), ("device_ms", C.c_double), ("n_steps", C.c_int),
                ("cycles_per_step", C.POINTER(C.c_int))]


MG_SOLVE_CONVERGED, MG_SOLVE_NOT_CONVERGED = 0, -1

# every symbol include/mg_hip.h declares: name -> (restype, argtypes)
ABI = {
    "mg_init": (_i, [_i]), "mg_finalize": (None, []), "mg_set_stream": (None, [_vp]),
    "mg_get_stream": (_vp, []), "mg_sync": (None, []), "mg_last_error": (_i, []),
    "mg_last_error_string": (C.c_char_p, []), "mg_clear_error": (None, []),
    "mg_set_abort_on_error": (None, [_i]), "mg_set_smoother": (_i, [C.c_char_p]),
    "mg_version": (C.c_char_p, []), "mg_set_source": (_i, [C.c_char_p]), "mg_source_mode": (C.c_char_p, []),
    "mg_source_is_bit_identical": (_i, []),
    "mg_alloc": (_vp, [_sz]), "mg_free": (None, [_vp]), "mg_pool_trim": (None, []),
    "mg_pool_bytes": (_sz, []), "mg_upload": (None, [_vp, _vp, _sz]), "mg_download": (None, [_vp, _vp, _sz]),
    "mg_copy": (None, [_vp, _vp, _sz]), "mg_fill_zero": (None, [_vp, _sz]), "mg_negate": (None, [_i, _vp]),
    "mg_getSource": (None, [_i, _d, _vp, _d, _d]), "mg_getAnalytic": (None, [_i, _d, _vp, _d, _d]),
    "mg_analyticError": (None, [_i, _d, _vp, _d, _d, _dptr]),
    "mg_getResidual": (None, [_i, _d, _vp, _vp, _vp]), "mg_doGridAddition": (None, [_i, _vp, _vp]),
    "mg_doSmoothing": (None, [_i, _d, _vp, _vp, _i, _dptr]),
    "mg_doExactSolver": (None, [_i, _d, _vp, _vp, _d, _i]),
    "mg_doRestriction": (None, [_i, _vp, _i, _vp]), "mg_doProlongation": (None, [_i, _vp, _i, _vp]),
    "mg_smooth_pp": (None, [_i, _d, _vp, _vp, _vp, _i, _vp, _vp, _i]),
    "mg_smooth_restrict": (None, [_i, _d, _vp, _vp, _vp, _i, _vp, _i, _vp]),
    "mg_prolong_smooth": (None, [_i, _vp, _i, _d, _vp, _vp, _vp, _i, _vp]),
    "mg_cycle_set_refinement": (_i, [_vp, _i]), "mg_cycle_refinement_errors": (_i, [_vp, _vp, _i]),
    "mg_smooth_restrict_f32": (None, [_i, _d, _vp, _vp, _vp, _i, _vp, _i, _vp]),
    "mg_prolong_smooth_f32": (None, [_i, _vp, _i, _d, _vp, _vp, _vp, _i, _vp]),
    "mg_alloc_f32": (_vp, [_sz]), "mg_free_f32": (None, [_vp]), "mg_to_f32": (None, [_vp, _vp, _sz]),
    "mg_to_f64": (None, [_vp, _vp, _sz]), "mg_upload_f32": (None, [_vp, _vp, _sz]),
    "mg_download_f32": (None, [_vp, _vp, _sz]),
    "mg_prolongAdd": (None, [_i, _vp, _i, _vp, _vp]), "mg_restrict_signed": (None, [_i, _vp, _i, _vp, _i]),
    "mg_lastExactSolverIterations": (_i, []),
    "mg_restriction_table": (None, [_i, _i, _vp, _vp]),
    "mg_prolongation_table": (None, [_i, _i, _i, _vp, _vp, _vp]),
    "mg_fill_uniform": (None, [_vp, _sz, _u64]), "mg_checksum": (None, [_vp, _sz, C.POINTER(_u64)]),
    "mg_cycle_load": (_vp, [C.c_char_p, _i]), "mg_cycle_execute": (_i, [_vp, C.POINTER(CycleResult)]),
    "mg_cycle_enqueue": (_i, [_vp]), "mg_cycle_collect": (_i, [_vp, C.POINTER(CycleResult)]),
    "mg_cycle_destroy": (None, [_vp]), "mg_cycle_main": (_i, [_i, C.POINTER(C.c_char_p)]),
    "mg_print2File": (_i, [_i, _vp, C.c_char_p]),
    "mg_comm_unique_id_bytes": (_i, []), "mg_comm_get_unique_id": (_i, [_vp]),
    "mg_comm_init_host": (_i, [_i, _i, _vp]),
    "mg_comm_init": (_i, [_i, _i, _vp]), "mg_comm_finalize": (None, []), "mg_comm_selftest": (_i, [_sz]), "mg_comm_rank": (_i, []),
    "mg_comm_size": (_i, []),
    "mg_comm_library": (C.c_char_p, []),
    "mg_slab_partition": (_i, [_i, _i, _i, _i, _vp, _vp]), "mg_slab_ghost_rows": (_i, []),
    "mg_slab_set_refinement": (_i, [_vp, _i]), "mg_slab_refinement_errors": (_i, [_vp, _vp, _i]),
    "mg_slab_schedule": (_i, [_i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "mg_slab_recompute_levels": (_i, [_i, _i, _i, _vp]), "mg_slab_recompute_levels_ranks": (_i, [_i, _i, _i, _i, _vp]),
    "mg_recompute_pair_available": (_i, [_i, _i]),
    "mg_slab_load": (_vp, [C.c_char_p, _i, _i, _i]), "mg_slab_load_flags": (_vp, [C.c_char_p, _i, _i, _i, _i]), "mg_slab_execute": (_i, [_vp, C.POINTER(CycleResult)]),
    "mg_slab_enqueue": (_i, [_vp]), "mg_slab_collect": (_i, [_vp, C.POINTER(CycleResult)]),
    "mg_slab_gather_U": (_i, [_vp, _vp]), "mg_slab_want_error": (None, [_vp, _i]), "mg_slab_destroy": (None, [_vp]),
    "mg_solve_opts_default": (None, [C.POINTER(SolveOpts)]),
    "mg_solver_create": (_vp, [_i, _d, C.POINTER(SolveOpts)]),
    "mg_solver_solve": (_i, [_vp, _vp, _vp, C.POINTER(SolveResult)]), "mg_solver_destroy": (None, [_vp]),
    "mg_batch_solver_create": (_vp, [_i, _d, _i, C.POINTER(SolveOpts)]),
    "mg_batch_solver_solve": (_i, [_vp, _i, _vp, _vp, _vp, C.POINTER(BatchSolveStats)]),
    "mg_batch_solver_destroy": (None, [_vp]),
    "mg_profile_begin": (None, [_i]), "mg_profile_sample": (None, [_i]), "mg_profile_end": (_i, [C.POINTER(ProfileEntry), _i]),
    "mg_stream_geometry_log": (None, [_i]), "mg_stream_geometry_fetch": (_i, [_vp, _i]),
}

# one record of the streaming smoother's geometry log (include/mg_hip.h: MG_STREAM_GEOMETRY_FIELDS ints, in this order)
GEOMETRY_FIELDS = ("N", "own", "rows_per_chunk", "chunks", "groups", "instances", "S", "COLS", "IN", "RESTRICT", "PRE", "flags")
MG_GEOMETRY_NT, MG_GEOMETRY_WT, MG_GEOMETRY_SH, MG_GEOMETRY_F32 = 1, 2, 4, 8

# the symbols include/mg_fmg.h declares (the full-multigrid start's building blocks); a library without them -- an older
# build named by MG_LIB for an A/B run -- still loads, cubic_table() / prolongCubic() then raise
ABI_FMG = {
    "mg_cubic_table": (None, [_i, _i, _vp, _vp]), "mg_prolongCubic": (None, [_i, _vp, _i, _vp]),
}

# the symbols include/mg_heat.h declares (theta-scheme time stepping of the heat equation over the solvers); bound like
# ABI_FMG: a library without them still loads, heat_rhs() / HeatStepper then raise
ABI_HEAT = {
    "mg_heat_opts_default": (None, [C.POINTER(HeatOpts)]),
    "mg_heat_rhs": (None, [_i, _d, _d, _d, _d, _vp, _vp, _vp]),
    "mg_heat_stepper_create": (_vp, [_i, _d, _i, C.POINTER(HeatOpts)]),
    "mg_heat_stepper_step": (_i, [_vp, _i, _vp, _vp, _i, C.POINTER(HeatResult)]),
    "mg_heat_stepper_sigma": (_d, [_vp]),
    "mg_heat_stepper_destroy": (None, [_vp]),
}

# the symbols include/mg_varcoef.h declares (the solver with a variable coefficient, div(a grad U) - sigma*U = F); bound like
# ABI_FMG: a library without them still loads, Solver.set_coefficient() / applyOperator() / ... then raise
ABI_VC = {
    "mg_solver_set_coefficient": (_i, [_vp, _vp]),
    "mg_solver_has_coefficient": (_i, [_vp]),
    "mg_applyOperator": (None, [_i, _d, _d, _vp, _vp, _vp]),
    "mg_coarsenCoefficient": (None, [_i, _vp, _i, _vp]),
    "mg_sweepCoefficient": (None, [_i, _d, _d, _d, _vp, _vp, _vp, _vp]),
    "mg_residualCoefficient": (None, [_i, _d, _d, _vp, _vp, _vp, _vp, _i]),
}

# the symbols include/mg_heat_vc.h declares (the heat stepper with a variable coefficient, u_t = nu*div(a grad u) + q); bound
# like ABI_FMG: a library without them still loads, heat_rhs_coef() / HeatStepper.set_coefficient() then raise
ABI_HEAT_VC = {
    "mg_heat_rhs_coef": (None, [_i, _d, _d, _d, _d, _vp, _vp, _vp, _vp]),
    "mg_heat_stepper_set_coefficient": (_i, [_vp, _vp]),
    "mg_heat_stepper_has_coefficient": (_i, [_vp]),
}

# the symbols include/mg_varcoef_batch.h declares (the batched solver with a coefficient per instance, or one shared); bound
# like ABI_FMG: a library without them still loads, BatchSolver.set_coefficient() / solve_batched_coef() then raise
ABI_VC_BATCH = {
    "mg_batch_solver_set_coefficient": (_i, [_vp, _i, _vp]),
    "mg_batch_solver_has_coefficient": (_i, [_vp]),
}

# the symbols include/mg_krylov.h declares (restarted GCR(m) around the cycle of Solver); bound like ABI_FMG: a library
# without them still loads, Solver(krylov=...) / Solver.set_krylov() / krylovDots() / ... then raise
ABI_KRYLOV = {
    "mg_solver_set_krylov": (_i, [_vp, _i]),
    "mg_solver_krylov": (_i, [_vp]),
    "mg_solver_krylov_breakdown": (_i, [_vp]),
    "mg_solver_krylov_log": (_i, [_vp, _vp, _i]),
    "mg_krylovDots": (None, [_i, _i, _vp, _vp, _vp]),
    "mg_krylovOrth": (None, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mg_krylovUpdate": (None, [_i, _d, _vp, _vp, _vp, _vp, _vp]),
}
MG_KRYLOV_MAX_M = 16

# the symbols include/mg_krylov_batch.h declares (GCR(m) per instance in the batched solver); bound like ABI_FMG: a library
# without them still loads, BatchSolver.set_krylov() / solve_batched_krylov() then raise
ABI_KRYLOV_BATCH = {
    "mg_batch_solver_set_krylov": (_i, [_vp, _i]),
    "mg_batch_solver_krylov": (_i, [_vp]),
    "mg_batch_solver_krylov_breakdown": (_i, [_vp, _i]),
    "mg_batch_solver_krylov_log": (_i, [_vp, _i, _vp, _i]),
}

# the symbols include/mg_adjoint.h declares (adjoint sensitivities: gradients of a solve in F, the rim data and a(x, y));
# bound like ABI_FMG: a library without them still loads, coefficientGradient() / Solver.adjoint() / ... then raise
ABI_ADJOINT = {
    "mg_coefficientGradient": (None, [_i, _d, _vp, _vp, _vp]),
    "mg_boundaryGradient": (None, [_i, _d, _vp, _vp, _vp, _vp]),
    "mg_coefficientGradient_batch": (None, [_i, _i, _d, _vp, _vp, _vp]),
    "mg_boundaryGradient_batch": (None, [_i, _i, _d, _vp, _vp, _vp, _vp]),
    "mg_solver_adjoint": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(SolveResult)]),
    "mg_batch_solver_adjoint": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(BatchSolveStats)]),
}

# the symbols include/mg_eigs.h declares (the lowest eigenmodes of -div(a grad u): multigrid-preconditioned LOBPCG); bound
# like ABI_FMG: a library without them still loads, EigenSolver / eigs() / eigsGram() / ... then raise
ABI_EIGS = {
    "mg_eigs_opts_default": (None, [C.POINTER(EigsOpts)]),
    "mg_eigs_create": (_vp, [_i, _d, C.POINTER(EigsOpts)]),
    "mg_eigs_set_coefficient": (_i, [_vp, _vp]),
    "mg_eigs_solve": (_i, [_vp, _vp, _i, _u64, _vp, _vp, C.POINTER(EigsResult)]),
    "mg_eigs_history": (_i, [_vp, _vp, _i]),
    "mg_eigs_destroy": (None, [_vp]),
    "mg_eigsGram": (_i, [_i, _i, _vp, _vp, _vp, _vp]),
    "mg_eigsRotate": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mg_eigsRayleighRitz": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp]),
}
MG_EIGS_MAX_BLOCK, MG_EIGS_DROP = 12, 1e-12

# the symbols include/mg_bc.h declares (Neumann and mixed boundary kinds per side in Solver and HeatStepper); bound like
# ABI_FMG: a library without them still loads, Solver.set_boundary() / neumann_source() / ... then raise
ABI_BC = {
    "mg_solver_set_boundary": (_i, [_vp, _vp]),
    "mg_solver_boundary": (_i, [_vp, _vp]),
    "mg_neumannSource": (None, [_i, _d, _vp, _vp, _vp, _vp, _vp]),
    "mg_applyOperatorBoundary": (None, [_i, _d, _d, _vp, _vp, _vp, _vp]),
    "mg_boundary_prolongation_table": (None, [_i, _i, _vp, _vp]),
    "mg_sweepBoundary": (None, [_i, _d, _d, _d, _vp, _vp, _vp, _vp, _vp]),
    "mg_residualBoundary": (None, [_i, _d, _d, _vp, _vp, _vp, _vp, _vp, _i]),
    "mg_restrictBoundary": (None, [_i, _vp, _vp, _i, _vp]),
    "mg_prolongAddBoundary": (None, [_i, _vp, _vp, _i, _vp, _vp]),
    "mg_heat_rhs_boundary": (None, [_i, _d, _d, _d, _d, _vp, _vp, _vp, _vp, _vp]),
    "mg_heat_stepper_set_boundary": (_i, [_vp, _vp]),
}
DIRICHLET, NEUMANN = 0, 1

# the symbols include/mg_singular.h declares (the pure Neumann problem: four flux sides at sigma = 0, the mean fixed); bound like
# ABI_FMG: a library without them still loads, Solver.set_mean() / weighted_mean() / project_mean() / ... then raise
ABI_SINGULAR = {
    "mg_solver_set_mean": (_i, [_vp, _i, _d]),
    "mg_solver_mean": (_i, [_vp, _vp]),
    "mg_solver_singular_info": (None, [_vp, _vp]),
    "mg_weightedMean": (None, [_i, _vp, _vp]),
    "mg_projectMean": (None, [_i, _vp, _d, _vp, _vp]),
    "mg_coarseSolveMean": (None, [_i, _d, _vp, _vp, _vp, _d, _d, _i, _vp, _vp]),
}

# the symbols include/mg_reaction.h declares (the solver with a variable reaction term, div(a grad U) - (sigma + s)*U = F);
# bound like ABI_FMG: a library without them still loads, Solver.set_reaction() / applyOperatorReaction() / ... then raise
ABI_REACTION = {
    "mg_solver_set_reaction": (_i, [_vp, _vp]),
    "mg_solver_has_reaction": (_i, [_vp]),
    "mg_applyOperatorReaction": (None, [_i, _d, _d, _vp, _vp, _vp, _vp]),
    "mg_sweepReaction": (None, [_i, _d, _d, _d, _vp, _vp, _vp, _vp, _vp]),
    "mg_residualReaction": (None, [_i, _d, _d, _vp, _vp, _vp, _vp, _vp, _i]),
    "mg_coarseSolveReaction": (None, [_i, _d, _d, _vp, _vp, _vp, _d, _d, _i, _vp]),
}

# the symbols include/mg_rx_batch.h declares (the batched solver with a reaction term per instance, or one shared); bound like
# ABI_VC_BATCH: a library without them still loads, BatchSolver.set_reaction() / solve_batched_reaction() then raise
ABI_RX_BATCH = {
    "mg_batch_solver_set_reaction": (_i, [_vp, _i, _vp]),
    "mg_batch_solver_has_reaction": (_i, [_vp]),
}

# the symbols include/mg_newton.h declares (the semilinear problem div(a grad U) - sigma*U - kappa*w*g(U) = F, Newton around the
# solver); bound like ABI_FMG: a library without them still loads, Solver.newton() / nonlinear_residual() / ... then raise
class NewtonOpts(C.Structure):
    _fields_ = [("rtol", C.c_double), ("atol", C.c_double), ("max_iters", C.c_int), ("max_backtracks", C.c_int)]


class NewtonResult(C.Structure):
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("converged", C.c_int), ("n_history", C.c_int),
                ("res0", C.c_double), ("res", C.c_double), ("inner_cycles", C.c_int), ("trials", C.c_int)]


class NewtonIter(C.Structure):
    _fields_ = [("res", C.c_double), ("t", C.c_double), ("backtracks", C.c_int), ("inner_cycles", C.c_int),
                ("inner_converged", C.c_int), ("inner_capped", C.c_int)]


ABI_NEWTON = {
    "mg_newton_opts_default": (None, [C.POINTER(NewtonOpts)]),
    "mg_solver_newton": (_i, [_vp, _i, _d, _vp, _vp, _vp, C.POINTER(NewtonOpts), C.POINTER(NewtonResult)]),
    "mg_solver_newton_history": (_i, [_vp, C.POINTER(NewtonIter), _i]),
    "mg_solver_newton_inner_history": (_i, [_vp, _vp, _i]),
    "mg_nonlinearResidual": (_i, [_i, _d, _d, _vp, _i, _d, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]),
}
NEWTON_KINDS = {"cubic": 0, "sinh": 1, "exp": 2}
NEWTON_CONVERGED, NEWTON_NOT_CONVERGED, NEWTON_STALLED = 0, -1, -2


# the symbols include/mg_newton_batch.h declares (the semilinear problem on the batched solver: Newton's method for many
# instances in lockstep); bound like ABI_RX_BATCH: a library without them still loads, BatchSolver.newton_batch() /
# solve_semilinear_batched() / nonlinear_residual_batch() then raise
class BatchNewtonStats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("trial_rounds", C.c_int), ("inner_cycles", C.c_int), ("launches", C.c_int),
                ("device_ms", C.c_double)]


ABI_NEWTON_BATCH = {
    "mg_batch_solver_newton": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, C.POINTER(NewtonOpts), C.POINTER(NewtonResult),
                                    C.POINTER(BatchNewtonStats)]),
    "mg_batch_solver_newton_history": (_i, [_vp, _i, C.POINTER(NewtonIter), _i]),
    "mg_batch_solver_newton_inner_history": (_i, [_vp, _i, _vp, _i]),
    "mg_nonlinearResidual_batch": (_i, [_i, _i, _d, _d, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp, _vp]),
}

# the symbols include/mg_adjoint_rx.h declares (the adjoint of reaction and semilinear solves: gradients in s, sigma, w and
# kappa); bound like ABI_ADJOINT: a library without them still loads, sourceGradient() / Solver.adjoint_reaction() / ... then raise
_dp = C.POINTER(C.c_double)
ABI_ADJOINT_RX = {
    "mg_sourceGradient": (_i, [_i, _i, _d, _vp, _vp, _vp, _vp, _dp]),
    "mg_sourceGradient_batch": (_i, [_i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "mg_solver_adjoint_reaction": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _dp, C.POINTER(SolveResult)]),
    "mg_solver_newton_adjoint": (_i, [_vp, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dp, _dp, C.POINTER(SolveResult)]),
    "mg_batch_solver_adjoint_reaction": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(BatchSolveStats)]),
    "mg_batch_solver_newton_adjoint": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                            C.POINTER(BatchSolveStats)]),
}
GRAD_KINDS = dict(NEWTON_KINDS, linear=3)   # MG_GRAD_LINEAR: g(u) = u

# the symbol include/mg_solve_cycle.h declares (the recorded V-cycle both solvers walk, as a list of its launches); bound like
# ABI_FMG: a library without it still loads, solve_cycle() then raises
ABI_SOLVE_CYCLE = {
    "mg_solve_cycle_describe": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i]),
}

_lib = None
hip_runtime = None   # which libamdhip64 the engine was bound to ("system", or the path of torch's copy)


def _bind_hip_runtime():
    """ONE HIP runtime per process.  libmgpoisson.so needs `libamdhip64.so.7`; a PyTorch wheel bundles its own
    copy (soname libamdhip64.so.7, but referenced by torch under the name `libamdhip64.so`, so the loader does
    not recognise a copy mapped earlier from /opt/rocm and maps a second one -- two runtimes on one device abort
    at exit).  The other order is fine: once torch's copy is mapped the engine's NEEDED entry matches it by
    soname.  So: when torch is installed but not imported yet, map ITS runtime first; every later import order
    then ends up with that single copy.  MG_HIP_RUNTIME=system keeps the ROCm installation's runtime (for
    processes that never import torch), MG_HIP_RUNTIME=<path> names a library explicitly."""
    global hip_runtime
    mode = os.environ.get("MG_HIP_RUNTIME", "auto")
    hip_runtime = "system"
    if mode == "system":
        return
    if mode not in ("auto", "torch"):
        C.CDLL(mode, mode=C.RTLD_GLOBAL)
        hip_runtime = mode
        return
    if "torch" in sys.modules:
        hip_runtime = "torch (imported before the engine)"
        return
    try:
        spec = importlib.util.find_spec("torch")  # locates the package without importing it
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)
        hip_runtime = cand


def load_library(path=None):
    """dlopen libmgpoisson.so and type every exported symbol.  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise MGError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc, gfx950).  There is no CPU fallback.")
    _bind_hip_runtime()
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    missing = []
    for name, (res, args) in ABI.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype, fn.argtypes = res, args
    if missing:
        raise MGError(f"{path} does not export: {missing}")
    for name, (res, args) in list(ABI_FMG.items()) + list(ABI_HEAT.items()) + list(ABI_VC.items()) + list(ABI_HEAT_VC.items()) + \
            list(ABI_VC_BATCH.items()) + list(ABI_KRYLOV.items()) + list(ABI_KRYLOV_BATCH.items()) + list(ABI_ADJOINT.items()) + \
            list(ABI_EIGS.items()) + list(ABI_BC.items()) + list(ABI_SINGULAR.items()) + list(ABI_SOLVE_CYCLE.items()) + \
            list(ABI_REACTION.items()) + list(ABI_NEWTON.items()) + list(ABI_RX_BATCH.items()) + list(ABI_NEWTON_BATCH.items()) + \
            list(ABI_ADJOINT_RX.items()):
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _check():
    code = _lib.mg_last_error()
    if code:
        msg = _lib.mg_last_error_string().decode()
        _lib.mg_clear_error()
        raise MGError(f"[{code}] {msg}")


_initialised = False


def init(device=0):
    global _initialised
    lib = load_library()
    lib.mg_set_abort_on_error(0)
    if lib.mg_init(int(device)) != 0:
        code = lib.mg_last_error()
        msg = lib.mg_last_error_string().decode()
        lib.mg_clear_error()
        raise MGError(f"mg_init({device}) failed [{code}]: {msg}")
    _initialised = True
    return lib


def lib():
    if not _initialised:
        init(int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("MG_DEVICE") is None
             else int(os.environ["MG_DEVICE"]))
    return _lib


def finalize():
    global _initialised
    if _initialised:
        _lib.mg_finalize()
        _initialised = False


def sync():
    lib().mg_sync()
    _check()


def set_smoother(name):
    lib().mg_set_smoother(name.encode())
    _check()


def set_source(mode):
    lib().mg_set_source(mode.encode())
    _check()


def source_mode():
    """'host' or 'device': where getSource is evaluated (auto mode: the device when it reproduces the host's libm)."""
    m = lib().mg_source_mode().decode()
    _check()
    return m


class DeviceGrid:
    """A device-resident fp64 array obtained from mg_alloc (the engine's replacement for
    the malloc'ed U/F/D of src/linkedlist.cpp:9-11)."""

    def __init__(self, shape):
        if isinstance(shape, int):
            shape = (shape, shape)
        self.shape = tuple(int(s) for s in shape)
        self.size = int(np.prod(self.shape))
        self.ptr = lib().mg_alloc(self.size)
        _check()
        if not self.ptr:
            raise MGError("mg_alloc returned NULL")

    @property
    def N(self):
        return self.shape[0]

    @classmethod
    def from_host(cls, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        g = cls(a.shape)
        _lib.mg_upload(g.ptr, a.ctypes.data, a.size)
        _check()
        return g

    @classmethod
    def zeros(cls, shape):
        g = cls(shape)
        _lib.mg_fill_zero(g.ptr, g.size)
        return g

    @classmethod
    def uniform(cls, shape, seed):
        g = cls(shape)
        _lib.mg_fill_uniform(g.ptr, g.size, seed)
        return g

    def to_host(self):
        out = np.empty(self.shape, dtype=np.float64)
        _lib.mg_download(out.ctypes.data, self.ptr, self.size)
        _check()
        return out

    def copy(self):
        g = DeviceGrid(self.shape)
        _lib.mg_copy(g.ptr, self.ptr, self.size)
        return g

    def checksum(self):
        out = (C.c_uint64 * 2)()
        _lib.mg_checksum(self.ptr, self.size, out)
        _check()
        return int(out[0]), int(out[1])

    def free(self):
        if self.ptr and _initialised:
            _lib.mg_free(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceGrid32:
    """fp32 device array (mixed-precision mode)."""

    def __init__(self, shape):
        if isinstance(shape, int):
            shape = (shape, shape)
        self.shape = tuple(int(s) for s in shape)
        self.size = int(np.prod(self.shape))
        self.ptr = lib().mg_alloc_f32(self.size)
        _check()

    @classmethod
    def from_host(cls, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        g = cls(a.shape)
        _lib.mg_upload_f32(g.ptr, a.ctypes.data, a.size)
        _check()
        return g

    def to_host(self):
        out = np.empty(self.shape, dtype=np.float32)
        _lib.mg_download_f32(out.ctypes.data, self.ptr, self.size)
        _check()
        return out

    def free(self):
        if self.ptr and _initialised:
            _lib.mg_free_f32(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def smooth_restrict_f32(N, L, U_out, F, step, M, F_c, want_error=False):
    err = DeviceGrid((1,)) if want_error else None
    lib().mg_smooth_restrict_f32(N, L, None, U_out.ptr, F.ptr, step, err.ptr if err else None, M, F_c.ptr)
    _check()
    if want_error:
        v = float(err.to_host()[0])
        err.free()
        return v


def prolong_smooth_f32(Nc, U_c, N, L, U_in, U_out, F, step, want_error=False):
    err = DeviceGrid((1,)) if want_error else None
    lib().mg_prolong_smooth_f32(Nc, U_c.ptr, N, L, U_in.ptr, U_out.ptr, F.ptr, step, err.ptr if err else None)
    _check()
    if want_error:
        v = float(err.to_host()[0])
        err.free()
        return v


# ---------------------------------------------------------------------------------
# the reference's operator surface (src/MG_solver_CPU.cpp:23-28) on DeviceGrid
# ---------------------------------------------------------------------------------
def getSource(N, L=1.0, min_x=0.0, min_y=0.0):
    F = DeviceGrid(N)
    _lib.mg_getSource(N, L, F.ptr, min_x, min_y)
    _check()
    return F


def getAnalytic(N, L=1.0, min_x=0.0, min_y=0.0):
    U = DeviceGrid(N)
    _lib.mg_getAnalytic(N, L, U.ptr, min_x, min_y)
    _check()
    return U


def analyticError(N, L, U, min_x=0.0, min_y=0.0):
    e = C.c_double()
    lib().mg_analyticError(N, L, U.ptr, min_x, min_y, C.byref(e))
    _check()
    return e.value


def getResidual(N, L, U, F, D):
    lib().mg_getResidual(N, L, U.ptr, F.ptr, D.ptr)
    _check()


def doGridAddition(N, U1, U2):
    lib().mg_doGridAddition(N, U1.ptr, U2.ptr)
    _check()


def doSmoothing(N, L, U, F, step, want_error=True):
    """In place, like the reference; returns the error scalar (host double)."""
    e = C.c_double()
    lib().mg_doSmoothing(N, L, U.ptr, F.ptr, step, C.byref(e) if want_error else None)
    _check()
    return e.value if want_error else None


def doExactSolver(N, L, U, F, target_error, option=1):
    lib().mg_doExactSolver(N, L, U.ptr, F.ptr, target_error, option)
    _check()


def lastExactSolverIterations():
    n = lib().mg_lastExactSolverIterations()
    _check()
    return n


def doRestriction(N, U_f, M, U_c):
    lib().mg_doRestriction(N, U_f.ptr, M, U_c.ptr)
    _check()


def doProlongation(N, U_c, M, U_f):
    lib().mg_doProlongation(N, U_c.ptr, M, U_f.ptr)
    _check()


def negate(N, D):
    lib().mg_negate(N, D.ptr)
    _check()


def smooth_pp(N, L, U_in, U_out, F, step, want_error=False, D_out=None, d_sign=1):
    """Out-of-place fused form (mg_smooth_pp).  U_in None = all-zero start."""
    err = DeviceGrid((1,)) if want_error else None
    lib().mg_smooth_pp(N, L, U_in.ptr if U_in is not None else None, U_out.ptr, F.ptr, step,
                       err.ptr if err else None, D_out.ptr if D_out is not None else None, d_sign)
    _check()
    if want_error:
        v = float(err.to_host()[0])
        err.free()
        return v
    return None


def smooth_restrict(N, L, U_in, U_out, F, step, M, F_c, want_error=False):
    err = DeviceGrid((1,)) if want_error else None
    lib().mg_smooth_restrict(N, L, U_in.ptr if U_in is not None else None, U_out.ptr, F.ptr, step,
                             err.ptr if err else None, M, F_c.ptr)
    _check()
    if want_error:
        v = float(err.to_host()[0])
        err.free()
        return v


def prolong_smooth(Nc, U_c, N, L, U_in, U_out, F, step, want_error=False):
    err = DeviceGrid((1,)) if want_error else None
    lib().mg_prolong_smooth(Nc, U_c.ptr, N, L, U_in.ptr, U_out.ptr, F.ptr, step, err.ptr if err else None)
    _check()
    if want_error:
        v = float(err.to_host()[0])
        err.free()
        return v


def prolongAdd(N, U_c, M, U_f_in, U_f_out):
    lib().mg_prolongAdd(N, U_c.ptr, M, U_f_in.ptr, U_f_out.ptr)
    _check()


def restrict_signed(N, U_f, M, U_c, sign):
    lib().mg_restrict_signed(N, U_f.ptr, M, U_c.ptr, sign)
    _check()


def restriction_table(N, M):
    lo = np.empty(M, dtype=np.int32)
    w = np.empty(M, dtype=np.float64)
    load_library().mg_restriction_table(N, M, lo.ctypes.data, w.ctypes.data)
    return lo, w


def prolongation_table(N, M, axis):
    owner = np.empty(M, dtype=np.int32)
    hi = np.empty(M)
    lo = np.empty(M)
    load_library().mg_prolongation_table(N, M, axis, owner.ctypes.data, hi.ctypes.data, lo.ctypes.data)
    return owner, hi, lo


def solve_cycle(nl, pre, post, top=0, fused=False, down_fused=None, up_fused=None, with_coef=False):
    """mg_solve_cycle_describe: the launches of one V(pre, post) cycle as both solvers walk them, one row of
    MG_SOLVE_CYCLE_RECORD ints per step (include/mg_solve_cycle.h); host only."""
    if not hasattr(load_library(), "mg_solve_cycle_describe"):
        raise MGError(f"{LIB_PATH} does not export mg_solve_cycle_describe (a build without the recorded cycle)")
    bits = [np.ascontiguousarray(b if b is not None else np.zeros(nl - 1), dtype=np.int32) for b in (down_fused, up_fused)]
    args = (nl, pre, post, top, int(fused), bits[0].ctypes.data, bits[1].ctypes.data, int(with_coef))
    n = load_library().mg_solve_cycle_describe(*args, None, 0)
    if n < 0:
        _check()
    out = np.empty((n, 16), dtype=np.int32)
    load_library().mg_solve_cycle_describe(*args, out.ctypes.data, n)
    return out


def cubic_table(N_src, N_dst):
    """mg_cubic_table: (base[N_dst], w[N_dst, 4]) of the 1-D cubic interpolation from N_src to N_dst points (the table of
    the full-multigrid start, solve_opts(fmg=...)); host only."""
    base = np.empty(N_dst, dtype=np.int32)
    w = np.empty((N_dst, 4), dtype=np.float64)
    if not hasattr(load_library(), "mg_cubic_table"):
        raise MGError(f"{LIB_PATH} does not export mg_cubic_table (a build without the fmg option)")
    load_library().mg_cubic_table(N_src, N_dst, base.ctypes.data, w.ctypes.data)
    return base, w


def prolongCubic(N_src, U_c, N_dst, U_f):
    """mg_prolongCubic on DeviceGrids: the interior of U_f = bicubic interpolation of U_c; the rim of U_f is not written."""
    if not hasattr(lib(), "mg_prolongCubic"):
        raise MGError(f"{LIB_PATH} does not export mg_prolongCubic (a build without the fmg option)")
    lib().mg_prolongCubic(N_src, U_c.ptr, N_dst, U_f.ptr)
    _check()


def _need_vc(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name} (a build without the variable-coefficient solver)")
    return getattr(_lib, name)


def applyOperator(N, L, shift, a, U, out):
    """mg_applyOperator on DeviceGrids: out = inv*b(U) of div(a grad U) - shift*U inside, +0 on the rim (include/mg_varcoef.h);
    a = None is a = 1, the constant operator."""
    _need_vc("mg_applyOperator")(N, L, shift, a.ptr if a is not None else None, U.ptr, out.ptr)
    _check()


def coarsenCoefficient(N, a_f, M, a_c):
    """mg_coarsenCoefficient on DeviceGrids: the nodal coefficient a_f (N x N) sampled at the M x M coarse points, rim included."""
    _need_vc("mg_coarsenCoefficient")(N, a_f.ptr, M, a_c.ptr)
    _check()


def sweepCoefficient(N, L, shift, omega, a, U_in, F, U_out):
    """Test hook (include/mg_varcoef.h).  mg_sweepCoefficient on DeviceGrids: one weighted Jacobi sweep of the variable-coefficient operator (U_in = None: from zero)."""
    _need_vc("mg_sweepCoefficient")(N, L, shift, omega, a.ptr, U_in.ptr if U_in is not None else None, F.ptr, U_out.ptr)
    _check()


def residualCoefficient(N, L, shift, a, U, F, D, sign=1):
    """Test hook (include/mg_varcoef.h).  mg_residualCoefficient on DeviceGrids: D = sign*(inv*b(U) - F) inside, sign*0 on the rim."""
    _need_vc("mg_residualCoefficient")(N, L, shift, a.ptr, U.ptr, F.ptr, D.ptr, sign)
    _check()


def _need_reaction(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name} (a build without the reaction term)")
    return getattr(_lib, name)


def applyOperatorReaction(N, L, shift, a, s, U, out):
    """mg_applyOperatorReaction on DeviceGrids: out = inv*b(U) of div(a grad U) - (shift + s)*U inside, +0 on the rim
    (include/mg_reaction.h); a = None is a = 1."""
    _need_reaction("mg_applyOperatorReaction")(N, L, shift, _opt(a), s.ptr, U.ptr, out.ptr)
    _check()


def sweepReaction(N, L, shift, omega, a, s, U_in, F, U_out):
    """Test hook (include/mg_reaction.h).  mg_sweepReaction on DeviceGrids: one weighted Jacobi sweep of the operator with the
    reaction term s (U_in = None: from zero; a = None: a = 1)."""
    _need_reaction("mg_sweepReaction")(N, L, shift, omega, _opt(a), s.ptr, _opt(U_in), F.ptr, U_out.ptr)
    _check()


def residualReaction(N, L, shift, a, s, U, F, D, sign=1):
    """Test hook (include/mg_reaction.h).  mg_residualReaction on DeviceGrids: D = sign*(inv*b(U) - F) inside, sign*0 on the rim."""
    _need_reaction("mg_residualReaction")(N, L, shift, _opt(a), s.ptr, U.ptr, F.ptr, D.ptr, sign)
    _check()


def coarseSolveReaction(N, L, shift, a, s, F, atol, rtol, max_iters, U_out):
    """Test hook (include/mg_reaction.h).  The coarse solve alone on DeviceGrids: U_out = the red-black solve from zero on F
    with the reaction term s, N <= 63, a = None is a = 1.  Returns the iterations."""
    _need_reaction("mg_coarseSolveReaction")(int(N), float(L), float(shift), _opt(a), s.ptr, F.ptr, float(atol), float(rtol),
                                             int(max_iters), U_out.ptr)
    _check()
    return lastExactSolverIterations()


def _need_newton(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name} (a build without the semilinear solve)")
    return getattr(_lib, name)


def _newton_kind(kind):
    if kind in NEWTON_KINDS:
        return NEWTON_KINDS[kind]
    if isinstance(kind, str):
        raise MGError(f"kind {kind!r}: expected one of {sorted(NEWTON_KINDS)}")
    return int(kind)   # (a number goes to the library, which refuses one it does not know)


def nonlinear_residual(N, L, shift, a, kind, kappa, w, U, F, D, S, dlt=None, t=1.0, V=None):
    """The pass of the semilinear solve on DeviceGrids (include/mg_newton.h: mg_nonlinearResidual), the building block of
    Solver.newton: with v = U (dlt = None) or v = U + t*dlt inside and U on the rim (written to V), S = kappa*w*g'(v) on every
    point, D = (F + kappa*w*g(v)) - A v inside and +0 on the rim, where A v = div(a grad v) - shift*v; returns
    sqrt(sum of D^2) in the order of the solver's residual norm.  a = None: a = 1; w = None: w = 1; kind: "cubic", "sinh"
    or "exp".  D is the right-hand side and S the reaction of the Newton equation, Solver(..., reaction=S).solve(D)."""
    out = C.c_double(0.0)
    status = _need_newton("mg_nonlinearResidual")(int(N), float(L), float(shift), _opt(a), _newton_kind(kind), float(kappa), _opt(w),
                                                  U.ptr, _opt(dlt), float(t), F.ptr, _opt(V), D.ptr, S.ptr, C.byref(out))
    if status:
        _check()
        raise MGError(f"mg_nonlinearResidual failed with status {status}")
    return float(out.value)


def _need_newton_batch(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name}: rebuild it (the batched semilinear solve is not in this library)")
    return getattr(_lib, name)


def _counted_pointers(arrays, n, what):
    """None, one DeviceGrid (anything with .ptr) or a sequence of 1 or n of them -> (count, pointer array or None)"""
    if arrays is None:
        return 0, None
    items = [arrays] if hasattr(arrays, "ptr") else list(arrays)
    if len(items) not in (1, n):
        raise MGError(f"[2] {what}: {len(items)} arrays for {n} instances (one shared by all, or one per instance)")
    return len(items), _pointer_array(items)


def nonlinear_residual_batch(N, L, shift, a, kind, kappa, w, U, F, D, S, dlt=None, t=1.0, V=None):
    """Test hook: nonlinear_residual for n instances in ONE launch (include/mg_newton_batch.h: mg_nonlinearResidual_batch).  U,
    F, D, S (and dlt, V in the step form): sequences of n DeviceGrids; a, w: None, one DeviceGrid shared by every instance, or
    a sequence of n; kappa: a scalar or a sequence of n.  Instance i gets the V, D, S and norm of nonlinear_residual on it
    alone, bit for bit.  Returns the list of the n norms."""
    n = len(U)
    for name, xs in (("F", F), ("D", D), ("S", S)) + ((("dlt", dlt), ("V", V)) if dlt is not None else ()):
        if xs is None or len(xs) != n:
            raise MGError(f"[2] {name}: expected {n} arrays")
    n_a, a_arr = _counted_pointers(a, n, "a")
    n_w, w_arr = _counted_pointers(w, n, "w")
    kap = np.ascontiguousarray(np.broadcast_to(np.asarray(kappa, dtype=np.float64), (n,)))
    norms = np.zeros(n)
    status = _need_newton_batch("mg_nonlinearResidual_batch")(
        n, int(N), float(L), float(shift), n_a, a_arr, _newton_kind(kind), kap.ctypes.data, n_w, w_arr, _pointer_array(U),
        None if dlt is None else _pointer_array(dlt), float(t), _pointer_array(F), None if dlt is None else _pointer_array(V),
        _pointer_array(D), _pointer_array(S), norms.ctypes.data)
    if status:
        _check()
        raise MGError(f"mg_nonlinearResidual_batch failed with status {status}")
    return [float(v) for v in norms]


def _need_bc(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name} (a build without the boundary kinds)")
    return getattr(_lib, name)


def _kinds(bc):
    """bc as a C int[4] in the order S, N, W, E (row 0, row N-1, column 0, column N-1): a 4-sequence of DIRICHLET (0) /
    NEUMANN (1), or a 4-character string of 'd' / 'n'; None: four Dirichlet sides.  The values are checked by the library."""
    if bc is None:
        bc = (0, 0, 0, 0)
    if isinstance(bc, str):
        if len(bc) != 4 or any(ch not in "dnDN" for ch in bc):
            raise MGError(f"bc = {bc!r}: expected 4 characters of 'd' / 'n' in the order S, N, W, E")
        bc = [1 if ch in "nN" else 0 for ch in bc]
    bc = list(bc)
    if len(bc) != 4:
        raise MGError(f"bc: expected 4 kinds in the order S, N, W, E, got {len(bc)}")
    return (C.c_int * 4)(*[int(v) for v in bc])


def _opt(a):
    return a.ptr if a is not None else None


def boundary_prolongation_table(M, N):
    """mg_boundary_prolongation_table: (lo[N], w[N]) of the 1-D prolongation from M coarse to N fine points of the boundary
    path (include/mg_bc.h); host only."""
    lo = np.empty(N, dtype=np.int32)
    w = np.empty(N, dtype=np.float64)
    if not hasattr(load_library(), "mg_boundary_prolongation_table"):
        raise MGError(f"{LIB_PATH} does not export mg_boundary_prolongation_table (a build without the boundary kinds)")
    load_library().mg_boundary_prolongation_table(int(M), int(N), lo.ctypes.data, w.ctypes.data)
    return lo, w


def neumann_source(N, L, bc, F, g, coef=None, out=None):
    """mg_neumannSource: out = F with the flux data dU/dn = g (outward normal) folded in, F - (2/h)*a*g at the rim unknowns of
    Neumann sides (a the NODAL coefficient; both terms at a corner of two Neumann sides), a copy elsewhere.
    bc: S, N, W, E (row 0, row N-1, column 0, column N-1).  g: shape (4, N) with the rows S, N, W, E; entries on Dirichlet
    sides are not read.  F, g, coef: numpy arrays (the result is a new numpy array), DeviceGrids (anything with .ptr and
    .shape; out = None: a new DeviceGrid) or float64 torch CUDA tensors (on torch.cuda.current_stream(); out = None: a new
    tensor), with the rules of Solver.set_coefficient.  coef = None: a = 1.  Returns out; the solver takes it as F."""
    fn = _need_bc("mg_neumannSource")
    N, kinds, keep = int(N), _kinds(bc), []
    if _is_torch(F) or _is_torch(g):
        import torch
        for name, t, shape in (("F", F, (N, N)), ("g", g, (4, N))) + ((("out", out, (N, N)),) if out is not None else ()):
            if not (_is_torch(t) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape and t.is_contiguous()
                    and t.data_ptr() % 16 == 0):
                raise MGError(f"{name}: expected a contiguous, 16-byte aligned float64 CUDA tensor of shape {shape}")
        if out is None:
            out = torch.empty_like(F)
        prev = _lib.mg_get_stream()
        _lib.mg_set_stream(torch.cuda.current_stream(F.device).cuda_stream)
        try:
            fn(N, float(L), kinds, _coefficient_address(N, coef, keep) if coef is not None else None, F.data_ptr(), g.data_ptr(),
               out.data_ptr())
        finally:
            _lib.mg_set_stream(prev)
            for k in keep:
                k.free()
        _check()
        return out

    def dev(a, shape, what):
        if hasattr(a, "ptr") and hasattr(a, "shape"):
            if tuple(a.shape) != shape:
                raise MGError(f"{what}: device array of shape {a.shape}, expected {shape}")
            return a
        a = np.asarray(a, dtype=np.float64)
        if a.shape != shape:
            raise MGError(f"{what}: array of shape {a.shape}, expected {shape}")
        keep.append(DeviceGrid.from_host(a))
        return keep[-1]

    host = not (hasattr(F, "ptr") and hasattr(F, "shape"))
    try:
        Fd, gd = dev(F, (N, N), "F"), dev(g, (4, N), "g")
        a_ptr = _coefficient_address(N, coef, keep) if coef is not None else None
        if out is None:
            out = DeviceGrid((N, N))
            if host:
                keep.append(out)
        fn(N, float(L), kinds, a_ptr, Fd.ptr, gd.ptr, out.ptr)
        _check()
        return out.to_host() if host and out in keep else out
    finally:
        for k in keep:
            k.free()


def applyOperatorBoundary(N, L, shift, bc, a, U, out):
    """mg_applyOperatorBoundary on DeviceGrids: out = inv*b(U) of div(a grad U) - shift*U at the unknowns with mirrored
    neighbours beyond Neumann sides, +0 at data points (include/mg_bc.h); bc: S, N, W, E; a = None is a = 1."""
    _need_bc("mg_applyOperatorBoundary")(int(N), float(L), float(shift), _kinds(bc), _opt(a), U.ptr, out.ptr)
    _check()


def sweepBoundary(N, L, shift, omega, bc, a, U_in, F, U_out):
    """Test hook (include/mg_bc.h).  One weighted Jacobi sweep at the unknowns (U_in = None: from zero); bc: S, N, W, E; on
    Neumann sides the rim of U is part of the guess and is written."""
    _need_bc("mg_sweepBoundary")(int(N), float(L), float(shift), float(omega), _kinds(bc), _opt(a), _opt(U_in), F.ptr, U_out.ptr)
    _check()


def residualBoundary(N, L, shift, bc, a, U, F, D, sign=1):
    """Test hook (include/mg_bc.h).  D = sign*(inv*b(U) - F) at the unknowns, sign*0 at data points; bc: S, N, W, E."""
    _need_bc("mg_residualBoundary")(int(N), float(L), float(shift), _kinds(bc), _opt(a), U.ptr, F.ptr, D.ptr, int(sign))
    _check()


def restrictBoundary(N, bc, D, M, F_c):
    """Test hook (include/mg_bc.h).  F_c (M x M) = the restriction of D (N x N) at the coarse unknowns, +0 at coarse data
    points; bc: S, N, W, E."""
    _need_bc("mg_restrictBoundary")(int(N), _kinds(bc), D.ptr, int(M), F_c.ptr)
    _check()


def prolongAddBoundary(M, bc, U_c, N, U_in, U_out):
    """Test hook (include/mg_bc.h).  U_out = U_in + P(U_c) at the fine unknowns -- the rim of Neumann sides is written --,
    U_in at fine data points; bc: S, N, W, E."""
    _need_bc("mg_prolongAddBoundary")(int(M), _kinds(bc), U_c.ptr, int(N), U_in.ptr, U_out.ptr)
    _check()


def _need_singular(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name} (a build without the pure Neumann problem)")
    return getattr(_lib, name)


def _on_array_stream(arrays, call):
    """call() with the engine on torch.cuda.current_stream() when any of `arrays` is a torch tensor, as neumann_source does"""
    ts = [t for t in arrays if _is_torch(t)]
    if not ts:
        return call()
    import torch
    prev = _lib.mg_get_stream()
    _lib.mg_set_stream(torch.cuda.current_stream(ts[0].device).cuda_stream)
    try:
        return call()
    finally:
        _lib.mg_set_stream(prev)


def _square_address(X, what, keep, N=None):
    """(N, device address) of a square fp64 field for the length of a call, by neumann_source's rules: a float64 torch CUDA
    tensor (contiguous, 16-byte aligned), a DeviceGrid (anything with .ptr and .shape), or a numpy array, which is uploaded into
    a DeviceGrid appended to `keep` (the caller frees it)."""
    shape = tuple(X.shape)
    if len(shape) != 2 or shape[0] != shape[1] or (N is not None and shape[0] != N):
        raise MGError(f"{what}: shape {shape}, expected a square array" + (f" of size {N}" if N is not None else ""))
    if _is_torch(X):
        import torch
        if not (X.is_cuda and X.dtype == torch.float64 and X.is_contiguous() and X.data_ptr() % 16 == 0):
            raise MGError(f"{what}: expected a contiguous, 16-byte aligned float64 CUDA tensor")
        return shape[0], X.data_ptr()
    if hasattr(X, "ptr"):
        return shape[0], X.ptr
    keep.append(DeviceGrid.from_host(np.asarray(X, dtype=np.float64)))
    return shape[0], keep[-1].ptr


def weighted_mean(X):
    """mg_weightedMean: the trapezoid-weighted mean of a square field, (sum of w*X)/(N-1)^2 with w = 1 inside, 1/2 on a side and
    1/4 in a corner, summed in the fixed order of include/mg_singular.h (the same bits every run).  With four Neumann sides at
    sigma = 0 it is the compatibility defect of a right-hand side and the gauge of a solution.  X: numpy array, DeviceGrid or
    float64 torch CUDA tensor (on torch.cuda.current_stream())."""
    fn = _need_singular("mg_weightedMean")
    keep, out = [], C.c_double(0.0)
    try:
        N, ptr = _square_address(X, "X", keep)
        _on_array_stream([X], lambda: fn(N, ptr, C.byref(out)))
        _check()
        return float(out.value)
    finally:
        for k in keep:
            k.free()


def project_mean(X, mean=0.0, out=None, want_removed=False):
    """mg_projectMean: out = X - (weighted_mean(X) - mean) at every point, so that weighted_mean(out) is `mean` up to rounding.
    X: numpy array (the result is a new numpy array), DeviceGrid (out = None: a new DeviceGrid) or float64 torch CUDA tensor (on
    torch.cuda.current_stream(); out = None: a new tensor); out may be X itself.  want_removed: returns (out, weighted_mean(X))."""
    fn = _need_singular("mg_projectMean")
    keep, removed = [], C.c_double(0.0)
    host = not (_is_torch(X) or hasattr(X, "ptr"))
    try:
        N, ptr = _square_address(X, "X", keep)
        if out is None:
            if _is_torch(X):
                import torch
                out = torch.empty_like(X)
            else:
                out = DeviceGrid((N, N))
                if host:
                    keep.append(out)
        elif host:
            raise MGError("out: a numpy X gives a new numpy array; pass DeviceGrids or tensors to name the output")
        _, optr = _square_address(out, "out", keep, N)
        _on_array_stream([X, out], lambda: fn(N, ptr, float(mean), optr, C.byref(removed)))
        _check()
        res = out.to_host() if host else out
        return (res, float(removed.value)) if want_removed else res
    finally:
        for k in keep:
            k.free()


def coarseSolveMean(N, L, bc, a, F, atol, rtol, max_iters, U_out):
    """Test hook (include/mg_singular.h).  The projected coarse solve alone on DeviceGrids: U_out = the red-black solve from
    zero on F minus its weighted mean, N <= 63, bc four Neumann sides, a = None is a = 1.  Returns (removed mean, iterations)."""
    removed = C.c_double(0.0)
    _need_singular("mg_coarseSolveMean")(int(N), float(L), _kinds(bc), _opt(a), F.ptr, float(atol), float(rtol), int(max_iters),
                                         U_out.ptr, C.byref(removed))
    _check()
    return float(removed.value), lastExactSolverIterations()


def _need_krylov(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name} (a build without the Krylov acceleration)")
    return getattr(_lib, name)


def _pointer_array(views):
    return (C.c_void_p * max(len(views), 1))(*[v.ptr for v in views])


def krylovDots(N, q, Q):
    """Test hook (include/mg_krylov.h).  mg_krylovDots on DeviceGrids: [<q, Q[j]>] over the interior, one pass."""
    out = np.zeros(max(len(Q), 1))
    _need_krylov("mg_krylovDots")(N, len(Q), q.ptr, _pointer_array(Q), out.ctypes.data)
    _check()
    return out[:len(Q)]


def krylovOrth(N, b, q, z, r, Q, Z):
    """Test hook (include/mg_krylov.h).  mg_krylovOrth on DeviceGrids: q -= b[j]*Q[j], z -= b[j]*Z[j] in order on the interior,
    returns (<q, q>, <r, q>) of the updated q."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    assert len(b) == len(Q) == len(Z)
    gh = np.zeros(2)
    _need_krylov("mg_krylovOrth")(N, len(Q), b.ctypes.data if len(b) else None, q.ptr, z.ptr, r.ptr, _pointer_array(Q),
                                  _pointer_array(Z), gh.ctypes.data)
    _check()
    return float(gh[0]), float(gh[1])


def krylovUpdate(N, alpha, U, z, r, q):
    """Test hook (include/mg_krylov.h).  mg_krylovUpdate on DeviceGrids: U += alpha*z, r -= alpha*q on the interior, returns
    <r, r> of the updated r."""
    rr = np.zeros(1)
    _need_krylov("mg_krylovUpdate")(N, float(alpha), U.ptr, z.ptr, r.ptr, q.ptr, rr.ctypes.data)
    _check()
    return float(rr[0])


def profile_begin(min_N=0, every=1):
    lib().mg_profile_sample(int(every))
    lib().mg_profile_begin(int(min_N))
    _check()


def profile_end(cap=256):
    buf = (ProfileEntry * cap)()
    n = lib().mg_profile_end(buf, cap)
    _check()
    return [dict(name=buf[i].name.decode(), N=buf[i].N, launches=buf[i].launches, total_ms=buf[i].total_ms,
                 algo_bytes=buf[i].algo_bytes) for i in range(n)]


def stream_geometry_log(on=True):
    """mg_stream_geometry_log: record how every launch of the streaming kernel is cut into chunks (host side, at enqueue)."""
    lib().mg_stream_geometry_log(1 if on else 0)


def stream_geometry_fetch():
    """mg_stream_geometry_fetch: the records since the last fetch, one dict with the keys GEOMETRY_FIELDS per launch."""
    out = []
    while True:
        n = lib().mg_stream_geometry_fetch(None, 0)
        if n <= 0:
            break
        buf = np.empty((n, len(GEOMETRY_FIELDS)), dtype=np.int32)
        got = _lib.mg_stream_geometry_fetch(buf.ctypes.data, n)
        _check()
        out += [dict(zip(GEOMETRY_FIELDS, (int(v) for v in row))) for row in buf[:got]]
    return out


class CyclePlan:
    """mg_cycle_load / mg_cycle_execute: the reference program's timed window
    (src/MG_solver_CPU.cpp:156..429) over a cycle structure file."""

    def __init__(self, path, fused=True, graph=False, report=True, error=True, mixed=False, refinement=1):
        flags = ((MG_CYCLE_FUSED if fused else 0) | (MG_CYCLE_GRAPH if graph else 0) |
                 (MG_CYCLE_REPORT if report else 0) | (MG_CYCLE_ERROR if error else 0) |
                 (MG_CYCLE_MIXED if mixed else 0))
        try:
            with open(path) as f:
                head = f.read().split()[:3]
        except OSError as e:
            raise MGError(f"Cannot open file {path}") from e  # src/MG_solver_CPU.cpp:65-68
        self.L, self.min_x, self.min_y = (float(t) for t in head)
        self._plan = lib().mg_cycle_load(os.fsencode(path), flags)
        _check()
        if not self._plan:
            raise MGError(f"cannot load cycle file {path}")
        self.refinement = refinement
        if refinement != 1:
            _lib.mg_cycle_set_refinement(self._plan, refinement)
            _check()

    def enqueue(self):
        """One window on the engine's stream, no host synchronisation (see collect)."""
        status = _lib.mg_cycle_enqueue(self._plan)
        _check()
        return status

    def collect(self, fetch_U=False):
        return self.execute(fetch_U=fetch_U, _collect_only=True)

    def execute(self, fetch_U=False, _collect_only=False):
        res = CycleResult()
        status = (_lib.mg_cycle_collect if _collect_only else _lib.mg_cycle_execute)(self._plan, C.byref(res))
        _check()
        out = dict(status=status, N=res.N, mg_error=res.mg_error, time_ms=res.time_ms, device_ms=res.device_ms,
                   records=[(res.records[i].node, res.records[i].N, res.records[i].steps, res.records[i].error)
                            for i in range(res.n_records)],
                   report=res.report.decode() if res.report else "", U_ptr=res.U_dev,
                   graph_replayed=bool(res.graph_replayed), schedule_launches=res.schedule_launches)
        if fetch_U:
            U = np.empty((res.N, res.N))
            _lib.mg_download(U.ctypes.data, res.U_dev, U.size)
            out["U"] = U
        if self.refinement > 1:
            e = np.zeros(self.refinement - 1)
            n = _lib.mg_cycle_refinement_errors(self._plan, e.ctypes.data, e.size)
            out["refinement_errors"] = e[:n].tolist()
        return out

    def analytic_error(self, result):
        """sum|analytic - U|/N^2 of a finished execute (src/MG_solver_CPU.cpp:434-445)."""
        e = C.c_double()
        _lib.mg_analyticError(result["N"], self.L, result["U_ptr"], self.min_x, self.min_y, C.byref(e))
        _check()
        return e.value

    def close(self):
        if self._plan and _initialised:
            _lib.mg_cycle_destroy(self._plan)
        self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def slab_partition(N_max, N_min, nranks, collapse_N):
    """Host-only: [(level N, collapsed, [(lo, hi) per rank])] of the row-slab decomposition."""
    lib_ = load_library()
    nl = lib_.mg_slab_partition(N_max, N_min, nranks, collapse_N, None, None)
    out = np.zeros((nl, nranks, 2), dtype=np.int32)
    coll = np.zeros(nl, dtype=np.int32)
    lib_.mg_slab_partition(N_max, N_min, nranks, collapse_N, out.ctypes.data, coll.ctypes.data)
    sizes, n = [], N_max
    while n >= N_min and n > 0:
        sizes.append(n)
        n //= 2
    return [(sizes[l], bool(coll[l]), [tuple(int(v) for v in out[l, r]) for r in range(nranks)]) for l in range(nl)]


def slab_schedule(N_max, N_min, nranks, collapse_N, steps, ca_mode=-1, ca_pct=-1):
    """mg_slab_schedule (host-only): per level a dict N, collapsed, halo, needF, xF, xU, pre (> 0: the level's `1`
    launch recomputes the pre-smoothed field, its `-1` launch does not store it) and, per rank, the row ranges
    own / dext / ext / fwr as (lo, hi) tuples."""
    lib_ = load_library()
    nl = lib_.mg_slab_partition(N_max, N_min, nranks, collapse_N, None, None)
    lev = np.zeros((nl, 6), dtype=np.int32)
    rk = np.zeros((nl, nranks, 8), dtype=np.int32)
    n = lib_.mg_slab_schedule(N_max, N_min, nranks, collapse_N, steps, ca_mode, ca_pct, lev.ctypes.data, rk.ctypes.data)
    if n < 0:
        lib_.mg_clear_error()
        raise MGError("mg_slab_schedule: a halo does not fit the neighbouring slab (raise collapse_N)")
    pre = np.zeros(nl, dtype=np.int32)
    lib_.mg_slab_recompute_levels_ranks(N_max, N_min, steps, nranks, pre.ctypes.data)
    out = []
    for l in range(nl):
        d = dict(N=int(lev[l, 0]), collapsed=bool(lev[l, 1]), halo=int(lev[l, 2]), needF=int(lev[l, 3]), xF=int(lev[l, 4]),
                 xU=int(lev[l, 5]), pre=0 if lev[l, 1] else int(pre[l]))
        for k, name in enumerate(("own", "dext", "ext", "fwr")):
            d[name] = [(int(rk[l, r, 2 * k]), int(rk[l, r, 2 * k + 1])) for r in range(nranks)]
        out.append(d)
    return out


def slab_ghost_rows():
    return load_library().mg_slab_ghost_rows()


def comm_init(rank, nranks, unique_id_bytes):
    buf = C.create_string_buffer(bytes(unique_id_bytes), len(unique_id_bytes))
    if lib().mg_comm_init(rank, nranks, buf) != 0:
        _check()
        raise MGError("mg_comm_init failed")
    _check()


_EXCHANGE_CB = C.CFUNCTYPE(_i, _vp, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_vp), C.POINTER(_sz))
_ALLGATHER_CB = C.CFUNCTYPE(_i, _vp, _vp, _vp, _sz)


class HostTransport(C.Structure):
    _fields_ = [("user", _vp), ("exchange", _EXCHANGE_CB), ("allgather", _ALLGATHER_CB)]


_host_transport_keepalive = []


def comm_init_host(rank, nranks, exchange, allgather):
    """mg_comm_init_host with Python callables:
    exchange(ops) with ops = [(is_send, peer, uint8 ndarray view of the host buffer), ...] must
    complete every transfer before returning; allgather(send, recv) fills recv (nranks x count)."""

    def _exchange(_user, n, is_send, peer, buf, count):
        try:
            ops = [(bool(is_send[i]), int(peer[i]),
                    np.ctypeslib.as_array(C.cast(buf[i], C.POINTER(C.c_uint8)), shape=(int(count[i]),))) for i in range(n)]
            exchange(ops)
            return 0
        except Exception as e:  # never unwind through the C frame
            print(f"host transport exchange failed: {e!r}", flush=True)
            return 1

    def _allgather(_user, send, recv, count):
        try:
            a = np.ctypeslib.as_array(C.cast(send, C.POINTER(_d)), shape=(int(count),))
            b = np.ctypeslib.as_array(C.cast(recv, C.POINTER(_d)), shape=(nranks, int(count)))
            allgather(a, b)
            return 0
        except Exception as e:
            print(f"host transport allgather failed: {e!r}", flush=True)
            return 1

    t = HostTransport(None, _EXCHANGE_CB(_exchange), _ALLGATHER_CB(_allgather))
    _host_transport_keepalive.append(t)
    if lib().mg_comm_init_host(rank, nranks, C.byref(t)) != 0:
        _check()
        raise MGError("mg_comm_init_host failed")
    _check()


def comm_unique_id():
    n = lib().mg_comm_unique_id_bytes()
    buf = C.create_string_buffer(n)
    if _lib.mg_comm_get_unique_id(buf) != 0:
        _check()
        raise MGError("mg_comm_get_unique_id failed")
    return bytes(buf.raw)


class SlabPlan:
    """The cycle-file driver on a 1-D row-slab decomposition (mg_slab_*)."""

    def __init__(self, path, nranks, rank=-1, collapse_N=512, mixed=False, refinement=1):
        self._plan = lib().mg_slab_load_flags(os.fsencode(path), nranks, rank, collapse_N, MG_CYCLE_MIXED if mixed else 0)
        _check()
        if not self._plan:
            raise MGError(f"cannot load cycle file {path} in row-slab mode")
        self.refinement = refinement
        if refinement != 1:
            _lib.mg_slab_set_refinement(self._plan, refinement)
            _check()

    def enqueue(self):
        status = _lib.mg_slab_enqueue(self._plan)
        _check()
        return status

    def collect(self):
        return self.execute(_collect_only=True)

    def execute(self, _collect_only=False):
        res = CycleResult()
        status = (_lib.mg_slab_collect if _collect_only else _lib.mg_slab_execute)(self._plan, C.byref(res))
        _check()
        out = dict(status=status, N=res.N, mg_error=res.mg_error, time_ms=res.time_ms, device_ms=res.device_ms,
                   records=[(res.records[i].node, res.records[i].N, res.records[i].steps, res.records[i].error)
                            for i in range(res.n_records)])
        if self.refinement > 1:
            e = np.zeros(self.refinement - 1)
            n = _lib.mg_slab_refinement_errors(self._plan, e.ctypes.data, e.size)
            out["refinement_errors"] = e[:n].tolist()
        return out

    def want_error(self, on):
        _lib.mg_slab_want_error(self._plan, 1 if on else 0)

    def gather_U(self, N):
        U = np.zeros((N, N))
        _lib.mg_slab_gather_U(self._plan, U.ctypes.data)
        _check()
        return U

    def close(self):
        if self._plan and _initialised:
            _lib.mg_slab_destroy(self._plan)
        self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_vcycle_file(path, N, N_min=8, steps=3, tol=1e-7, L=1.0):
    """The synthetic V-cycle of SURVEY.md section 8d: header `steps 1 / N N_min`, one -1
    per level down to the coarsest generated size, one exact solve, one 1 per level up."""
    levels = 0
    n = N
    while n >= N_min:
        levels += 1
        n //= 2
    with open(path, "w") as f:
        f.write(f"{L} 0.0 0.0\n{steps} 1\n{N} {N_min}\n")
        f.write("-1\n" * (levels - 1))
        f.write(f"0\n{tol:.10f} 1\n")
        f.write("1\n" * (levels - 1))
        f.write("2")
    return levels


def write_wcycle_file(path, N, N_min=8, steps=3, tol=1e-7, L=1.0, depth=None):
    """W-cycle with the recursion of the shipped src/Wcycle.txt (which stops after 4 of
    its 6 generated levels); depth=None takes it down to the coarsest generated size."""
    sizes = []
    n = N
    while n >= N_min:
        sizes.append(n)
        n //= 2
    if depth is not None:
        sizes = sizes[:depth]
    last = len(sizes) - 1

    def visit(level):
        if level == last:
            return ["0", f"{tol:.10f} 1"]
        return ["-1"] + visit(level + 1) + ["1"] + ["-1"] + visit(level + 1) + ["1"]

    nodes = ["-1"] + visit(1) + ["1"] if last >= 1 else visit(0)
    with open(path, "w") as f:
        f.write(f"{L} 0.0 0.0\n{steps} 1\n{N} {N_min}\n" + "\n".join(nodes) + "\n2")
    return len(sizes)


def solve_opts(**opts):
    """mg_solve_opts: the library's defaults (V(3,3), omega 0.8, N_min 8, coarse_rtol 1e-2, rtol 1e-10, 50 cycles) with
    the named fields replaced.  rtol is relative to ||F||; large grids have an fp64 rounding floor above 1e-10 (about
    8e-10 at N = 8192 on the getSource problem): there a default solve runs all max_cycles and reports not converged,
    so pass rtol=1e-9 or more at that size.
    shift (sigma, default 0, finite and >= 0) solves the screened equation  Laplace(U) - sigma*U = F  on every level
    instead (include/mg_hip.h gives the per-level constants); 0 is the Poisson solve bit for bit.  An implicit time step
    of u_t = nu*Laplace(u) is one such solve with sigma = 1/(nu*dt) and F = -u_old/(nu*dt).
    fmg (default 0 = off; 1..8) gives the solve a full-multigrid start: unless the start already meets the tolerance, the
    interior of U is first replaced by the coarsest level's solution interpolated upwards with cubic interpolation and
    fmg V-cycles per coarse level (the interior passed in is ignored, the rim is the boundary data), then the cycles
    run: 2-5 cycles to rtol 1e-9 instead of 8-11 from a cold start.  Solver only: BatchSolver refuses fmg != 0."""
    o = SolveOpts()
    lib().mg_solve_opts_default(C.byref(o))
    names = {f for f, _ in SolveOpts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise TypeError(f"unknown solver option {k!r} (have {sorted(names)})")
        setattr(o, k, v)
    return o


def _coefficient_address(N, a, keep):
    """Device address of one coefficient for the length of a call: a DeviceGrid (anything with .ptr and .shape), a float64
    torch CUDA tensor, or an N x N numpy array, which is uploaded into a DeviceGrid appended to `keep` (the caller frees it)."""
    if _is_torch(a):
        import torch
        if not (a.is_cuda and a.dtype == torch.float64 and tuple(a.shape) == (N, N) and a.is_contiguous()):
            raise MGError(f"coef: expected a contiguous float64 CUDA tensor of shape ({N}, {N})")
        if a.data_ptr() % 16 != 0:   # (odd instances of a contiguous [n, N, N] tensor with N odd; on the engine stream)
            g = DeviceGrid((N, N))
            keep.append(g)
            _lib.mg_copy(g.ptr, a.data_ptr(), N * N)
            _check()
            return g.ptr
        return a.data_ptr()
    if hasattr(a, "ptr") and hasattr(a, "shape"):
        if tuple(a.shape) != (N, N):
            raise MGError(f"coef: DeviceGrid of shape {a.shape}, expected ({N}, {N})")
        return a.ptr
    a = np.asarray(a, dtype=np.float64)
    if a.shape != (N, N):
        raise MGError(f"coef: array of shape {a.shape}, expected ({N}, {N})")
    g = DeviceGrid.from_host(a)
    keep.append(g)
    return g.ptr


def _set_coefficient(fn, handle, N, a, what="coef"):
    """The argument handling of Solver.set_coefficient, Solver.set_reaction and HeatStepper.set_coefficient (`what` names the
    array in messages): fn(handle, device address of a) with a
    an N x N numpy array (uploaded for the call), a DeviceGrid, or a float64 torch CUDA tensor (read on
    torch.cuda.current_stream()); None takes the coefficient away.  A refusal raises MGError."""
    if a is None:
        fn(handle, None)
        _check()
        return
    if _is_torch(a):
        import torch
        if not (a.is_cuda and a.dtype == torch.float64 and tuple(a.shape) == (N, N) and a.is_contiguous()):
            raise MGError(f"{what}: expected a contiguous float64 CUDA tensor of shape ({N}, {N})")
        prev = _lib.mg_get_stream()
        _lib.mg_set_stream(torch.cuda.current_stream(a.device).cuda_stream)
        try:
            status = fn(handle, a.data_ptr())
        finally:
            _lib.mg_set_stream(prev)
    elif hasattr(a, "ptr") and hasattr(a, "shape"):
        if tuple(a.shape) != (N, N):
            raise MGError(f"{what}: DeviceGrid of shape {a.shape}, expected ({N}, {N})")
        status = fn(handle, a.ptr)
    else:
        a = np.asarray(a, dtype=np.float64)
        if a.shape != (N, N):
            raise MGError(f"{what}: array of shape {a.shape}, expected ({N}, {N})")
        g = DeviceGrid.from_host(a)
        try:
            status = fn(handle, g.ptr)
        finally:
            g.free()
    if status:
        _check()
        raise MGError(f"{fn.__name__} failed with status {status}")


class Solver:
    """Residual-tolerance solver of include/mg_hip.h: V(pre, post) cycles with a weighted Jacobi smoother and a
    relative coarse target, on a caller's F and Dirichlet rim, until ||F - AU||_2 <= max(rtol*||F||_2, atol).  Every
    level array is allocated here; solve() allocates nothing on the device.  With shift=sigma > 0 the operator is
    A U = Laplace(U) - sigma*U (solve_opts); an implicit time step has sigma = 1/(nu*dt), F = -u_old/(nu*dt).
    fmg=n (1..8) starts every solve from a full-multigrid guess instead of U's interior (solve_opts).
    coef=a (or set_coefficient(a)) solves div(a grad U) - sigma*U = F, a > 0 given at the grid points:
        s = Solver(N, L, shift=sigma); s.set_coefficient(a); U, info = s.solve(F, U0); s.set_coefficient(None)
    krylov=m (or set_krylov(m), 1 <= m <= 16) wraps the cycle in restarted GCR(m) with the V-cycle from a zero start as the
    preconditioner (include/mg_krylov.h): the residual norm then cannot grow, and coefficients on which the plain cycle
    is slow or diverges (jumps, strong contrast) converge.  It costs memory, (2m + 1)*N^2 doubles allocated when it is
    switched on (8.7 GB at N = 8192 for m = 8), and 120 + 24k bytes per point and iteration.  Convergence is only stated on a
    recomputed residual, never on the recurred norm; info gains `breakdown`.  krylov=0 (the default) is the plain solver, bit for bit.
    bc=kinds (or set_boundary(kinds)) makes sides Neumann (include/mg_bc.h): four kinds in the order S, N, W, E -- row 0, row
    N-1, column 0, column N-1 -- as a sequence of DIRICHLET / NEUMANN or a string such as "ndnd".  On Neumann sides the rim of
    U is part of the guess and is written; flux data goes into F with neumann_source().
    mean=m (or set_mean(m)) opens the pure Neumann problem, bc="nnnn" at shift == 0 (include/mg_singular.h): the solve removes
    the weighted mean of F (info["compat_defect"]: what the data lacked in compatibility), runs the cycles with a projected
    coarse solve, and returns the solution whose weighted mean is m (info["mean_before"]: what it was before that shift).
    With any other boundary or shift the setting is dormant.
    reaction=s (or set_reaction(s)) solves div(a grad U) - (sigma + s)*U = F with s >= 0 given at the grid points
    (include/mg_reaction.h), with or without coef: the linearised Poisson-Boltzmann equation, a Newton step with s = g'(u), an
    absorbing region.  s == 0 everywhere is the solver without it, s == c at shift == 0 the solver with shift=c, bit for bit.
    A discontinuous or strongly varying s slows the plain cycle down; krylov=m is supported with it and is what to use then.
    Refused together with fmg, a Neumann side and adjoint().
    newton(F, U, kind=..., kappa=..., weight=w) solves the semilinear problem div(a grad U) - sigma*U - kappa*w*g(U) = F by
    Newton's method around this solver (include/mg_newton.h); it sets and removes a reaction of its own."""

    def __init__(self, N, L=1.0, coef=None, krylov=0, **opts):
        bc = opts.pop("bc", None)   # (the boundary kinds travel beside the solve options, not in mg_solve_opts)
        mean = opts.pop("mean", None)
        reaction = opts.pop("reaction", None)
        self.N, self.L = int(N), float(L)
        self.opts = solve_opts(**opts)
        self._s = lib().mg_solver_create(self.N, self.L, C.byref(self.opts))
        if not self._s:
            _check()
            raise MGError("mg_solver_create returned NULL")
        try:
            if coef is not None:
                self.set_coefficient(coef)
            if reaction is not None:
                self.set_reaction(reaction)
            if krylov:
                self.set_krylov(krylov)
            if mean is not None:
                self.set_mean(mean)
            if bc is not None:
                self.set_boundary(bc)
        except Exception:
            self.close()
            raise

    def set_mean(self, mean):
        """mean: the weighted mean (weighted_mean) the solution of a singular solve gets, which also lets set_boundary("nnnn")
        through at shift == 0 (include/mg_singular.h); None: off.  Dormant while the operator is not singular: the solver then
        enqueues what it enqueues without it.  A refusal (MGError) leaves the solver as it was: "[2]" a mean that is not
        finite; "[3]" None while four Neumann sides at shift == 0 are set."""
        fn = _need_singular("mg_solver_set_mean")
        status = fn(self._s, 0, 0.0) if mean is None else fn(self._s, 1, float(mean))
        if status:
            _check()
            raise MGError(f"mg_solver_set_mean failed with status {status}")

    @property
    def mean(self):
        """the target of set_mean, or None while it is off"""
        out = C.c_double(0.0)
        on = _need_singular("mg_solver_mean")(self._s, C.byref(out))
        return float(out.value) if on else None

    def set_krylov(self, m):
        """m = 1 .. 16: restarted GCR(m) around the cycle (include/mg_krylov.h), m directions kept between restarts; m = 0:
        the plain cycle iteration again, bit for bit.  Switching it on allocates the memory it needs, (2m + 1)*N^2 doubles
        (a later, larger m the additional slots); a solve allocates nothing.  Convergence is stated on a recomputed residual
        only.  Works with and without a coefficient and with any shift.  A refusal (MGError: m outside [0, 16], "[3]" for a
        solver created with fmg != 0, a failed allocation) leaves the solver as it was."""
        status = _need_krylov("mg_solver_set_krylov")(self._s, int(m))
        if status:
            _check()
            raise MGError(f"mg_solver_set_krylov failed with status {status}")

    @property
    def krylov(self):
        """the m of set_krylov (0: off)"""
        return int(_need_krylov("mg_solver_krylov")(self._s))

    def krylov_log(self):
        """Diagnostic and test hook (include/mg_krylov.h): one dict per iteration of the last accelerated solve with the keys
        k, d (the k dot products <q_k, q_j>), g, h, alpha, rho_rec, restarted, rho."""
        fn = _need_krylov("mg_solver_krylov_log")
        n = fn(self._s, None, 0)
        if n <= 0:
            return []
        m = self._krylov_log_m   # (the m of that solve, noted by solve_ptr: a record is m + 7 doubles)
        buf = np.zeros((n, m + 7))
        got = fn(self._s, buf.ctypes.data, n)
        return [dict(k=int(rec[0]), d=[float(v) for v in rec[1:1 + int(rec[0])]], g=float(rec[m + 1]), h=float(rec[m + 2]),
                     alpha=float(rec[m + 3]), rho_rec=float(rec[m + 4]), restarted=bool(rec[m + 5]), rho=float(rec[m + 6]))
                for rec in buf[:got]]

    def set_coefficient(self, a):
        """a: N x N values of the coefficient at the grid points, rim included, finite and > 0 (numpy array, DeviceGrid or
        float64 torch CUDA tensor, which is read on torch.cuda.current_stream()); None: back to the constant solver.
        Faces average their two nodes (aE = 0.5*(a[p] + a[p+1]), ...), coarse levels are rediscretised from the sampled a
        (include/mg_varcoef.h); a == 1 everywhere is the solver without a coefficient, bit for bit.  a is copied: it may be
        freed after the call.  A refused coefficient (MGError) leaves the solver as it was."""
        _set_coefficient(_need_vc("mg_solver_set_coefficient"), self._s, self.N, a)

    @property
    def has_coefficient(self):
        return bool(_need_vc("mg_solver_has_coefficient")(self._s))

    def set_reaction(self, s):
        """s: N x N values of the reaction term at the grid points, rim included, finite and >= 0 (numpy array, DeviceGrid or
        float64 torch CUDA tensor, which is read on torch.cuda.current_stream()); None: the solver without it, enqueueing what
        it enqueued before.  The centre of the operator becomes d = aN + aS + aE + aW + (sigma + s[p])*dx2; coarse levels sample
        s as they sample a (include/mg_reaction.h).  s is copied: it may be freed after the call.  Works with and without a
        coefficient and with krylov, in any order.  A refusal (MGError) leaves the solver as it was: "[2]" a negative or not
        finite value, a misaligned array; "[3]" a solver created with fmg != 0, a Neumann side set.  While a reaction is set,
        set_boundary with a Neumann side and adjoint() are refused."""
        _set_coefficient(_need_reaction("mg_solver_set_reaction"), self._s, self.N, s, what="reaction")

    @property
    def has_reaction(self):
        return bool(_need_reaction("mg_solver_has_reaction")(self._s))

    def set_boundary(self, bc):
        """bc: the four kinds in the order S, N, W, E (row 0, row N-1, column 0, column N-1), a sequence of DIRICHLET (0) /
        NEUMANN (1) or a string of 'd' / 'n'; None or four Dirichlet sides take the boundary away (the plain solver again, bit
        for bit).  A Neumann side is homogeneous, dU/dn = 0, discretised with a mirrored ghost point (include/mg_bc.h); flux
        data dU/dn = g goes into F with neumann_source().  On Neumann sides the rim of U is part of the guess and is written by
        the solve; points on Dirichlet sides (corners shared with a Neumann side included) stay data.  Works with and without
        a coefficient and in either order with set_coefficient.  A refusal (MGError) leaves the solver and its earlier kinds
        as they were: "[2]" a kind outside {0, 1}; "[3]" four Neumann sides with shift == 0 (the singular problem), a solver
        created with fmg != 0, krylov switched on.  While a boundary is set, set_krylov(m > 0) and adjoint() are refused."""
        status = _need_bc("mg_solver_set_boundary")(self._s, _kinds(bc))
        if status:
            _check()
            raise MGError(f"mg_solver_set_boundary failed with status {status}")

    @property
    def boundary(self):
        """the four kinds (S, N, W, E) as a tuple of DIRICHLET / NEUMANN"""
        out = (C.c_int * 4)()
        _need_bc("mg_solver_boundary")(self._s, out)
        return tuple(int(v) for v in out)

    def solve_ptr(self, F_ptr, U_ptr):
        """F_ptr, U_ptr: device addresses of N x N fp64 arrays (U in/out), on the engine stream."""
        res = SolveResult()
        status = _lib.mg_solver_solve(self._s, F_ptr, U_ptr, C.byref(res))
        if status > 0:
            _check()
            raise MGError(f"mg_solver_solve failed with status {status}")
        history = [res.history[i] for i in range(res.n_history)]
        info = dict(status=res.status, cycles=res.cycles, converged=bool(res.converged),
                    coarse_capped=bool(res.coarse_capped), res0=res.res0, res=res.res, ref_norm=res.ref_norm,
                    device_ms=res.device_ms, history=history)
        if hasattr(_lib, "mg_solver_krylov") and _lib.mg_solver_krylov(self._s):
            self._krylov_log_m = int(_lib.mg_solver_krylov(self._s))
            info["breakdown"] = bool(_lib.mg_solver_krylov_breakdown(self._s))
        if hasattr(_lib, "mg_solver_mean") and _lib.mg_solver_mean(self._s, None) and self.boundary == (1, 1, 1, 1) \
                and self.opts.shift == 0.0:   # a singular solve (include/mg_singular.h)
            three = (C.c_double * 3)()
            _lib.mg_solver_singular_info(self._s, three)
            info["compat_defect"], info["mean_before"], info["mean"] = float(three[0]), float(three[1]), float(three[2])
        return info

    def solve(self, F, U=None):
        """F, U: numpy arrays, DeviceGrid, or float64 torch CUDA tensors (worked on in place, on
        torch.cuda.current_stream()).  U = None starts from zero (zero rim).  Returns (U, info); a numpy U comes back
        as a new numpy array."""
        N = self.N
        if _is_torch(F) or _is_torch(U):
            import torch
            if U is None:
                U = torch.zeros((N, N), dtype=torch.float64, device=F.device)
            for name, t in (("F", F), ("U", U)):
                if not (_is_torch(t) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (N, N)
                        and t.is_contiguous()):
                    raise MGError(f"{name}: expected a contiguous float64 CUDA tensor of shape ({N}, {N})")
            prev = _lib.mg_get_stream()
            _lib.mg_set_stream(torch.cuda.current_stream(F.device).cuda_stream)
            try:
                info = self.solve_ptr(F.data_ptr(), U.data_ptr())
            finally:
                _lib.mg_set_stream(prev)
            return U, info
        keep = []

        def dev(a, what):
            if isinstance(a, DeviceGrid):
                if a.shape != (N, N):
                    raise MGError(f"{what}: DeviceGrid of shape {a.shape}, expected ({N}, {N})")
                return a
            a = np.asarray(a, dtype=np.float64)
            if a.shape != (N, N):
                raise MGError(f"{what}: array of shape {a.shape}, expected ({N}, {N})")
            g = DeviceGrid.from_host(a)
            keep.append(g)
            return g

        Fd = dev(F, "F")
        host_U = U is None or not isinstance(U, DeviceGrid)
        Ud = DeviceGrid.zeros((N, N)) if U is None else dev(U, "U")
        info = self.solve_ptr(Fd.ptr, Ud.ptr)
        return (Ud.to_host() if host_U else Ud), info

    def newton_ptr(self, F_ptr, U_ptr, kind="sinh", kappa=1.0, w_ptr=None, rtol=1e-8, atol=0.0, max_iters=20, max_backtracks=12):
        """mg_solver_newton on device addresses of N x N fp64 arrays (U in/out, w_ptr = None: w = 1), on the engine stream."""
        fn = _need_newton("mg_solver_newton")
        o = NewtonOpts(float(rtol), float(atol), int(max_iters), int(max_backtracks))
        res = NewtonResult()
        status = fn(self._s, _newton_kind(kind), float(kappa), w_ptr, F_ptr, U_ptr, C.byref(o), C.byref(res))
        if status > 0:
            _check()
            raise MGError(f"mg_solver_newton failed with status {status}")
        if hasattr(_lib, "mg_solver_krylov") and _lib.mg_solver_krylov(self._s):
            self._krylov_log_m = int(_lib.mg_solver_krylov(self._s))   # (krylov_log(): the last inner solve's records)
        recs = (NewtonIter * max(res.n_history, 1))()
        n = _lib.mg_solver_newton_history(self._s, recs, res.n_history)
        iters = [dict(res=r.res, t=r.t, backtracks=r.backtracks, inner_cycles=r.inner_cycles,
                      inner_converged=bool(r.inner_converged), inner_capped=bool(r.inner_capped)) for r in recs[:n]]
        return dict(status=res.status, iterations=res.iterations, converged=bool(res.converged), stalled=res.status == NEWTON_STALLED,
                    res0=res.res0, res=res.res, inner_cycles=res.inner_cycles, trials=res.trials,
                    history=[res.res0] + [r["res"] for r in iters[:res.iterations]], steps=iters,
                    last_inner_history=self._inner_history() if iters else [])

    def _inner_history(self):
        n = _lib.mg_solver_newton_inner_history(self._s, None, 0)
        buf = np.zeros(max(n, 1))
        got = _lib.mg_solver_newton_inner_history(self._s, buf.ctypes.data, n)
        return [float(v) for v in buf[:got]]

    def newton(self, F, U=None, kind="sinh", kappa=1.0, weight=None, rtol=1e-8, atol=0.0, max_iters=20, max_backtracks=12):
        """Solve the semilinear problem div(a grad U) - sigma*U - kappa*w*g(U) = F by Newton's method with a backtracking line
        search around this solver (include/mg_newton.h): g = u^3 ("cubic"), sinh u ("sinh") or e^u ("exp"), kappa >= 0,
        weight = w >= 0 at the grid points (None: w = 1), a and sigma the solver's coefficient and shift, Dirichlet values on
        the rim of U.  Every Newton step is one solve of this solver with the reaction kappa*w*g'(U), to the solver's own
        rtol / atol / max_cycles (with krylov if it is on); the outer iteration stops at ||N(U)|| <= max(atol, rtol*||N(U_0)||),
        after max_iters accepted steps, or when max_backtracks halvings of a step do not lower the norm (info["stalled"]).
        F, U, weight: numpy arrays, DeviceGrids or float64 torch CUDA tensors, as solve() takes them.  Returns (U, info);
        info["history"] holds the norms, info["steps"] one dict per iteration (res, t, backtracks, inner_cycles,
        inner_converged, inner_capped).  Refused ("[3]") while a reaction or a Neumann side is set and with fmg; the solver
        has no reaction afterwards, as before."""
        N = self.N
        opts = dict(kind=kind, kappa=kappa, rtol=rtol, atol=atol, max_iters=max_iters, max_backtracks=max_backtracks)
        if _is_torch(F) or _is_torch(U) or _is_torch(weight):
            import torch
            if U is None:
                U = torch.zeros((N, N), dtype=torch.float64, device=F.device)
            for name, t in (("F", F), ("U", U)) + ((("weight", weight),) if weight is not None else ()):
                if not (_is_torch(t) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (N, N)
                        and t.is_contiguous()):
                    raise MGError(f"{name}: expected a contiguous float64 CUDA tensor of shape ({N}, {N})")
            prev = _lib.mg_get_stream()
            _lib.mg_set_stream(torch.cuda.current_stream(F.device).cuda_stream)
            try:
                info = self.newton_ptr(F.data_ptr(), U.data_ptr(), w_ptr=None if weight is None else weight.data_ptr(), **opts)
            finally:
                _lib.mg_set_stream(prev)
            return U, info
        keep = []

        def dev(a, what):
            if isinstance(a, DeviceGrid):
                if a.shape != (N, N):
                    raise MGError(f"{what}: DeviceGrid of shape {a.shape}, expected ({N}, {N})")
                return a
            a = np.asarray(a, dtype=np.float64)
            if a.shape != (N, N):
                raise MGError(f"{what}: array of shape {a.shape}, expected ({N}, {N})")
            g = DeviceGrid.from_host(a)
            keep.append(g)
            return g

        Fd = dev(F, "F")
        wd = None if weight is None else dev(weight, "weight")
        host_U = U is None or not isinstance(U, DeviceGrid)
        Ud = DeviceGrid.zeros((N, N)) if U is None else dev(U, "U")
        info = self.newton_ptr(Fd.ptr, Ud.ptr, w_ptr=None if wd is None else wd.ptr, **opts)
        return (Ud.to_host() if host_U else Ud), info

    def adjoint_ptr(self, Ubar_ptr, U_ptr, lam_ptr, gA_ptr=None, gU_ptr=None):
        """mg_solver_adjoint on device addresses of N x N fp64 arrays, on the engine stream: lam (out) = the adjoint field of
        the right-hand side Ubar, gA (out, or None) = the gradient in the coefficient from lam and the forward solution U,
        gU (out, or None) = the gradient in the rim data.  Returns the info dict of solve_ptr for the adjoint solve."""
        res = SolveResult()
        status = _need_adjoint("mg_solver_adjoint")(self._s, Ubar_ptr, U_ptr, lam_ptr, gA_ptr, gU_ptr, C.byref(res))
        if status > 0:
            _check()
            raise MGError(f"mg_solver_adjoint failed with status {status}")
        info = _solve_info(res)
        if hasattr(_lib, "mg_solver_krylov") and _lib.mg_solver_krylov(self._s):
            self._krylov_log_m = int(_lib.mg_solver_krylov(self._s))
            info["breakdown"] = bool(_lib.mg_solver_krylov_breakdown(self._s))
        return info

    def adjoint(self, Ubar, U, want_coef=True, want_rim=True):
        """The adjoint of a solve of this solver (include/mg_adjoint.h): for a functional J(U) of the solution U of
        div(a grad U) - sigma*U = F with Ubar = dJ/dU (N x N; its rim entries are the direct dependence of J on the rim
        values), returns (lam, gA, gU, info):
          lam   the adjoint field, the solve of the same equation -- coefficient, shift, krylov, fmg as set -- with
                right-hand side Ubar from the zero field; dJ/dF is lam on the interior and 0 on the rim
          gA    dJ/da at every grid point, rim included (want_coef; None otherwise).  Without a coefficient set it is
                the sensitivity at a == 1
          gU    dJ/d(rim data) as an N x N array: 0 inside, Ubar at the corners (want_rim; None otherwise)
          info  the dict of solve() for the adjoint solve; a solve that did not converge still gives the gradients
        Ubar, U: numpy arrays (results are new numpy arrays), DeviceGrids (results are DeviceGrids) or float64 torch CUDA
        tensors (results are tensors; on torch.cuda.current_stream()), handled as solve() handles them.  Bit for bit the
        sequence {zero fill, solve, coefficientGradient, boundaryGradient} made by the caller."""
        N = self.N
        if _is_torch(Ubar) or _is_torch(U):
            import torch
            for name, t in (("Ubar", Ubar), ("U", U)):
                if not (_is_torch(t) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (N, N) and t.is_contiguous()):
                    raise MGError(f"{name}: expected a contiguous float64 CUDA tensor of shape ({N}, {N})")
            dev = Ubar.device
            (ub_ptr,), ub_buf = _staged([Ubar], False, N * N, dev)
            (u_ptr,), u_buf = _staged([U], False, N * N, dev)
            lam = torch.empty((N, N), dtype=torch.float64, device=dev)
            gA = torch.empty((N, N), dtype=torch.float64, device=dev) if want_coef else None
            gU = torch.empty((N, N), dtype=torch.float64, device=dev) if want_rim else None
            prev = _lib.mg_get_stream()
            _lib.mg_set_stream(torch.cuda.current_stream(dev).cuda_stream)
            try:
                info = self.adjoint_ptr(ub_ptr, u_ptr, lam.data_ptr(), gA.data_ptr() if want_coef else None,
                                        gU.data_ptr() if want_rim else None)
            finally:
                _lib.mg_set_stream(prev)
            del ub_buf, u_buf
            return lam, gA, gU, info
        keep = []

        def dev(a, what):
            if hasattr(a, "ptr") and hasattr(a, "shape"):
                if tuple(a.shape) != (N, N):
                    raise MGError(f"{what}: DeviceGrid of shape {a.shape}, expected ({N}, {N})")
                return a
            a = np.asarray(a, dtype=np.float64)
            if a.shape != (N, N):
                raise MGError(f"{what}: array of shape {a.shape}, expected ({N}, {N})")
            g = DeviceGrid.from_host(a)
            keep.append(g)
            return g

        host = not (hasattr(Ubar, "ptr") and hasattr(U, "ptr"))
        Ud, Ub = dev(U, "U"), dev(Ubar, "Ubar")
        lam = DeviceGrid((N, N))
        gA = DeviceGrid((N, N)) if want_coef else None
        gU = DeviceGrid((N, N)) if want_rim else None
        info = self.adjoint_ptr(Ub.ptr, Ud.ptr, lam.ptr, gA.ptr if want_coef else None, gU.ptr if want_rim else None)
        if host:
            return lam.to_host(), gA.to_host() if want_coef else None, gU.to_host() if want_rim else None, info
        return lam, gA, gU, info

    def adjoint_reaction(self, Ubar, U, want_coef=True, want_rim=True, want_reaction=True):
        """The adjoint of a solve of this solver with whatever it has set -- reaction term, coefficient, shift, krylov
        (include/mg_adjoint_rx.h): for a functional J(U) of the solution U of div(a grad U) - (sigma + s)*U = F with Ubar = dJ/dU,
        returns (lam, gA, gU, gS, info): lam, gA, gU as Solver.adjoint gives them, gS = dJ/ds = lam'*U on the interior and +0 on the
        rim (want_reaction; None otherwise; without a reaction set: the sensitivity at s = 0), info the dict of solve() for the
        adjoint solve with info["gshift"] = dJ/dsigma, the sum of gS (None without want_reaction).  Ubar, U: numpy arrays,
        DeviceGrids or float64 torch CUDA tensors, as adjoint() takes them.  Bit for bit the sequence {zero fill, solve,
        coefficientGradient, boundaryGradient, sourceGradient("linear", 1.0, None)} made by the caller; without a reaction set
        lam, gA and gU are adjoint()'s."""
        fn = _need_adjoint_rx("mg_solver_adjoint_reaction")
        io = _AdjointIO(self.N, [Ubar, U])
        ub, u = io.inp(Ubar, "Ubar"), io.inp(U, "U")
        lam, gA, gU, gS = io.out(), io.out(want_coef), io.out(want_rim), io.out(want_reaction)
        res, gshift = SolveResult(), C.c_double(0.0)
        status = io.run(lambda: fn(self._s, ub, u, io.ptr(lam), io.ptr(gA), io.ptr(gU), io.ptr(gS),
                                   C.byref(gshift) if want_reaction else None, C.byref(res)))
        if status > 0:
            _check()
            raise MGError(f"mg_solver_adjoint_reaction failed with status {status}")
        info = _solve_info(res)
        info["gshift"] = float(gshift.value) if want_reaction else None
        if hasattr(_lib, "mg_solver_krylov") and _lib.mg_solver_krylov(self._s):
            self._krylov_log_m = int(_lib.mg_solver_krylov(self._s))
            info["breakdown"] = bool(_lib.mg_solver_krylov_breakdown(self._s))
        return io.result(lam), io.result(gA), io.result(gU), io.result(gS), info

    def newton_adjoint(self, Ubar, U, F, kind="sinh", kappa=1.0, weight=None, want_coef=True, want_rim=True, want_weight=True):
        """The adjoint of a semilinear solve newton(F, U0, kind, kappa, weight) of this solver at its solution U
        (include/mg_adjoint_rx.h): for a functional J(U) with Ubar = dJ/dU, returns (lam, gA, gU, gW, info): lam the adjoint field,
        ONE solve of this solver with the reaction kappa*w*g'(U) and right-hand side Ubar from the zero field (dJ/dF is lam on the
        interior); gA, gU as Solver.adjoint gives them; gW = dJ/dw = kappa*lam'*g(U) on the interior and +0 on the rim
        (want_weight; None otherwise); info the dict of solve() for the adjoint solve with info["gkappa"] = dJ/dkappa, the sum of
        w*lam'*g(U) (None without want_weight), and info["res_forward"] = ||N(U)||, which says how converged the U is that the
        gradients are taken at.  Arrays: numpy arrays, DeviceGrids or float64 torch CUDA tensors.  Refused as newton() refuses;
        the solver has no reaction afterwards, as before."""
        fn = _need_adjoint_rx("mg_solver_newton_adjoint")
        io = _AdjointIO(self.N, [Ubar, U, F])
        ub, u, f, w = io.inp(Ubar, "Ubar"), io.inp(U, "U"), io.inp(F, "F"), io.inp(weight, "weight")
        lam, gA, gU, gW = io.out(), io.out(want_coef), io.out(want_rim), io.out(want_weight)
        res, gkappa, resf = SolveResult(), C.c_double(0.0), C.c_double(0.0)
        status = io.run(lambda: fn(self._s, _newton_kind(kind), float(kappa), w, f, u, ub, io.ptr(lam), io.ptr(gA), io.ptr(gU), io.ptr(gW),
                                   C.byref(gkappa) if want_weight else None, C.byref(resf), C.byref(res)))
        if status > 0:
            _check()
            raise MGError(f"mg_solver_newton_adjoint failed with status {status}")
        info = _solve_info(res)
        info["gkappa"] = float(gkappa.value) if want_weight else None
        info["res_forward"] = float(resf.value)
        if hasattr(_lib, "mg_solver_krylov") and _lib.mg_solver_krylov(self._s):
            self._krylov_log_m = int(_lib.mg_solver_krylov(self._s))
            info["breakdown"] = bool(_lib.mg_solver_krylov_breakdown(self._s))
        return io.result(lam), io.result(gA), io.result(gU), io.result(gW), info

    def close(self):
        if getattr(self, "_s", None) and _initialised:
            _lib.mg_solver_destroy(self._s)
        self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _is_torch(a):
    return a is not None and type(a).__module__.startswith("torch") and hasattr(a, "data_ptr")


def solve(F, U=None, L=1.0, **opts):
    """Solve the Poisson problem A U = F on the N x N grid of F (Dirichlet values on U's rim) to the residual
    tolerance; returns (U, info).  See Solver, and solve_opts for the defaults (the default rtol of 1e-10 is below the
    rounding floor of large grids: about 8e-10 at N = 8192).  shift=sigma > 0 solves Laplace(U) - sigma*U = F, the
    equation of an implicit time step: sigma = 1/(nu*dt), F = -u_old/(nu*dt).  fmg=1 starts from a full-multigrid guess
    (U then only supplies the rim).  coef=a (N x N, > 0, at the grid points) solves div(a grad U) - sigma*U = F with faces
    averaging their two nodes (Solver.set_coefficient); a == 1 everywhere is the solve without coef, bit for bit.
    krylov=m (1..16) wraps the cycle in restarted GCR(m) (Solver.set_krylov, include/mg_krylov.h): (2m + 1)*N^2 doubles of
    memory more, a residual norm that cannot grow, and convergence stated on a recomputed residual only.
    bc=kinds makes sides Neumann (Solver.set_boundary): four kinds in the order S, N, W, E (row 0, row N-1, column 0, column
    N-1), e.g. "ndnd"; on Neumann sides the rim of U is part of the guess and is written.
    bc="nnnn" with mean=m at shift == 0 is the pure Neumann problem (Solver.set_mean): F is projected onto the compatible
    right-hand sides and the solution returned has the weighted mean m.
    reaction=s (N x N, >= 0, at the grid points) solves div(a grad U) - (sigma + s)*U = F (Solver.set_reaction,
    include/mg_reaction.h), with or without coef; with a discontinuous s add krylov=m."""
    N = int(F.shape[0])
    s = Solver(N, L, **opts)
    try:
        return s.solve(F, U)
    finally:
        s.close()


def solve_semilinear(F, U=None, L=1.0, kind="sinh", kappa=1.0, weight=None, coef=None, krylov=0, rtol=1e-8, atol=0.0, max_iters=20,
                     max_backtracks=12, inner_rtol=None, inner_atol=None, **opts):
    """Solve div(a grad U) - sigma*U - kappa*w*g(U) = F on the N x N grid of F (Dirichlet values on U's rim) by Newton's method
    around the multigrid solver (Solver.newton, include/mg_newton.h); returns (U, info).  kind, kappa, weight, rtol, atol,
    max_iters and max_backtracks are the Newton iteration's; coef, krylov and **opts (shift, max_cycles, omega, ...) make the
    Solver every Newton step runs on, inner_rtol / inner_atol being that Solver's rtol / atol (the forcing term; None: the
    Solver's defaults).  With a discontinuous weight add krylov=m."""
    N = int(F.shape[0])
    for name, v in (("rtol", inner_rtol), ("atol", inner_atol)):
        if v is not None:
            opts[name] = v
    s = Solver(N, L, coef=coef, krylov=krylov, **opts)
    try:
        return s.newton(F, U, kind=kind, kappa=kappa, weight=weight, rtol=rtol, atol=atol, max_iters=max_iters,
                        max_backtracks=max_backtracks)
    finally:
        s.close()


def _instances(X, what):
    """[B, N, N] array / tensor or a list of (N, N) ones -> list of instances; a single (N, N) one -> [it] (broadcast)."""
    if isinstance(X, (list, tuple)):
        return list(X), False
    if len(X.shape) == 3:
        return [X[i] for i in range(X.shape[0])], False
    if len(X.shape) == 2:
        return [X], True
    raise MGError(f"{what}: expected [B, N, N], (N, N) or a list of (N, N) arrays, got shape {tuple(X.shape)}")


def _staged(ts, share, nn, dev):
    """device addresses of the torch tensors ts (nn doubles each), through a staging buffer of pitch nn + 1 when one of them
    is not 16-byte aligned; share: every entry of ts is the same tensor.  Returns (addresses, buffer or None)."""
    import torch
    if all(t.data_ptr() % 16 == 0 for t in ts):
        return [t.data_ptr() for t in ts], None
    if share:
        buf = torch.empty((1, nn + 1), dtype=torch.float64, device=dev)
        buf[0, :nn].copy_(ts[0].reshape(-1))
        return [buf.data_ptr()] * len(ts), buf
    buf = torch.empty((len(ts), nn + 1), dtype=torch.float64, device=dev)
    for i, t in enumerate(ts):
        buf[i, :nn].copy_(t.reshape(-1))
    return [buf[i].data_ptr() for i in range(len(ts))], buf


class BatchNewtonInfos(list):
    """The per-instance info dicts of BatchSolver.newton_batch, in the order of the instances; stats: the dict of the call's own
    figures (status, iterations, trial_rounds, inner_cycles, launches, device_ms)."""
    stats = None


class BatchSolver:
    """Batched residual-tolerance solver of include/mg_hip.h: up to max_batch problems of size N with one set of options
    (see solve_opts) in one call, every instance bit-identical to a Solver solve of it alone (U, history, cycles, status).
    An instance stops once it meets its own tolerance; one cycle is one launch per node over all active instances.
    Every level array for max_batch instances is allocated here; solve() allocates nothing on the device.  shift=sigma
    (one value for the whole batch) solves Laplace(U) - sigma*U = F: the many same-size solves of implicit time stepping,
    sigma = 1/(nu*dt), F_i = -u_old_i/(nu*dt).  fmg != 0 (the full-multigrid start of Solver) is refused here.
    set_coefficient(a) solves div(a_i grad U_i) - sigma*U_i = F_i, one coefficient per instance or one shared by all, every
    instance bit-identical to Solver(coef=a_i) on it alone (include/mg_varcoef_batch.h):
        b = BatchSolver(N, L, max_batch=B); b.set_coefficient(a); U, infos = b.solve(F, U0); b.set_coefficient(None)
    set_krylov(m) wraps the cycle of every instance in restarted GCR(m) (include/mg_krylov_batch.h), every instance
    bit-identical to Solver(krylov=m) on it alone: for coefficients on which the plain cycle crawls or diverges.
    set_reaction(s) solves div(a_i grad U_i) - (sigma + s_i)*U_i = F_i, one reaction term per instance or one shared by all,
    with or without a coefficient and with set_krylov, every instance bit-identical to Solver(reaction=s_i, coef=a_i) on it
    alone (include/mg_rx_batch.h).
    newton_batch(F, U, kind, kappa, weight) solves the semilinear problems div(a_i grad U_i) - sigma*U_i - kappa_i*w_i*g(U_i) = F_i by
    Newton's method in lockstep, every instance bit-identical to Solver.newton on it alone (include/mg_newton_batch.h)."""

    def __init__(self, N, L=1.0, max_batch=64, **opts):
        self.N, self.L, self.max_batch = int(N), float(L), int(max_batch)
        self.opts = solve_opts(**opts)
        self._s = lib().mg_batch_solver_create(self.N, self.L, self.max_batch, C.byref(self.opts))
        if not self._s:
            _check()
            raise MGError("mg_batch_solver_create returned NULL")

    def set_coefficient(self, a):
        """a of shape (N, N): one coefficient shared by every instance (one copy is stored).  a of shape (n, N, N), or a
        sequence of n (N, N) arrays, DeviceGrids or tensors, n <= max_batch: instance i of a solve uses a[i], and a solve
        then takes at most n instances.  None: back to the constant solver.  Values at the grid points, rim included, finite
        and > 0; numpy arrays, DeviceGrids or float64 torch CUDA tensors (read on torch.cuda.current_stream()), as
        Solver.set_coefficient takes them.  Every instance then solves as Solver(coef=a[i]) solves it alone, bit for bit; a == 1
        everywhere is the solver without a coefficient, bit for bit.  The arrays are copied: they may be freed after the
        call.  A refused coefficient (MGError "[2] ...": a wrong shape, more than max_batch coefficients, a bad value, whose
        instance the message names) leaves the solver as it was."""
        self._set_arrays(_need_vc_batch("mg_batch_solver_set_coefficient"), "mg_batch_solver_set_coefficient", a, "coef", "coefficient")

    def _set_arrays(self, fn, name, a, what, noun):
        """the argument handling of set_coefficient and set_reaction: fn(handle, n, the device addresses of the n arrays)"""
        if a is None:
            status = fn(self._s, 0, None)
        else:
            N = self.N
            if isinstance(a, (list, tuple)):
                items = list(a)
            elif len(a.shape) == 3:
                items = [a[i] for i in range(a.shape[0])]
            elif len(a.shape) == 2:
                items = [a]
            else:
                raise MGError(f"[2] {what}: expected (N, N), (n, N, N) or a sequence of (N, N) arrays, got shape {tuple(a.shape)}")
            if not items:
                raise MGError(f"[2] {what}: an empty sequence (None takes the {noun} away)")
            keep, prev = [], None
            torch_item = next((t for t in items if _is_torch(t)), None)
            try:
                if torch_item is not None:
                    import torch
                    prev = _lib.mg_get_stream()
                    _lib.mg_set_stream(torch.cuda.current_stream(torch_item.device).cuda_stream)
                try:
                    ptrs = [_coefficient_address(N, t, keep) for t in items]
                except MGError as e:   # (a wrong shape or type is an argument error like the library's own: code 2)
                    raise MGError("[2] " + str(e).replace("coef:", what + ":", 1)) from None
                status = fn(self._s, len(ptrs), (C.c_void_p * len(ptrs))(*ptrs))
            finally:
                if torch_item is not None:
                    _lib.mg_set_stream(prev)
                for g in keep:
                    g.free()
        if status:
            _check()
            raise MGError(f"{name} failed with status {status}")

    @property
    def has_coefficient(self):
        """True when a coefficient is set (shared or per instance)."""
        return self.n_coefficients > 0

    @property
    def n_coefficients(self):
        """0 without a coefficient, 1 with one shared by every instance, else the number of per-instance coefficients."""
        return int(_need_vc_batch("mg_batch_solver_has_coefficient")(self._s))

    def set_reaction(self, s):
        """s of shape (N, N): one reaction term shared by every instance (one copy is stored).  s of shape (n, N, N), or a
        sequence of n (N, N) arrays, DeviceGrids or tensors, n <= max_batch: instance i of a solve uses s[i], and a solve
        then takes at most n instances.  None: the solver without a reaction again, enqueueing what it enqueued before.
        Values at the grid points, rim included, finite and >= 0; numpy arrays, DeviceGrids or float64 torch CUDA tensors
        (read on torch.cuda.current_stream()), as set_coefficient takes them.  Every instance then solves
        div(a_i grad U_i) - (sigma + s_i)*U_i = F_i as Solver(reaction=s[i], coef=a_i) solves it alone, bit for bit (U,
        history, cycles, flags), with set_krylov(m) as Solver(krylov=m, reaction=s[i], coef=a_i); s == 0 everywhere is the
        solver without a reaction, s == c at shift 0 is BatchSolver(shift=c), bit for bit.  The count is independent of the
        coefficient's (a shared a with per-instance s, and so on), and set_coefficient, set_reaction and set_krylov work in
        any order.  The arrays are copied: they may be freed after the call.  A refused reaction (MGError "[2] ...": a wrong
        shape, more than max_batch terms, a negative or not finite value, whose instance the message names) leaves the solver
        as it was.  While a reaction is set, adjoint() is refused ("[3]")."""
        self._set_arrays(_need_rx_batch("mg_batch_solver_set_reaction"), "mg_batch_solver_set_reaction", s, "reaction", "reaction")

    @property
    def has_reaction(self):
        """True when a reaction term is set (shared or per instance)."""
        return self.n_reactions > 0

    @property
    def n_reactions(self):
        """0 without a reaction, 1 with one shared by every instance, else the number of per-instance reaction terms."""
        return int(_need_rx_batch("mg_batch_solver_has_reaction")(self._s))

    def set_krylov(self, m):
        """m = 1 .. 16: restarted GCR(m) around the cycle, per instance (include/mg_krylov_batch.h; the method is
        include/mg_krylov.h's), every launch over all active instances; m = 0: the plain batch solver again, bit for bit and
        launch for launch.  Contract: instance i of a solve is bit-identical to Solver(krylov=m, coef=a_i) solving F_i, U_i
        alone -- U, cycles, status, history, the breakdown flag and krylov_log(i) -- whatever the other instances are and
        wherever it sits in the batch, with per-instance coefficients, a shared one or none, any shift, any V(pre, post).
        Each instance runs with its own k, tolerance and restarts, and is stated converged on a recomputed residual only,
        never on the recurred norm.  Memory: switching it on allocates (2m + 1)*N^2*max_batch doubles (N^2 rounded up to
        32) plus small change; a later, larger m the additional slots; a solve allocates nothing.  Works before or after
        set_coefficient.  A refusal (MGError: "[2]" for m outside [0, 16], a failed allocation) leaves the solver as it was."""
        status = _need_krylov_batch("mg_batch_solver_set_krylov")(self._s, int(m))
        if status:
            _check()
            raise MGError(f"mg_batch_solver_set_krylov failed with status {status}")

    @property
    def krylov(self):
        """the m of set_krylov (0: off)"""
        return int(_need_krylov_batch("mg_batch_solver_krylov")(self._s))

    def krylov_log(self, i):
        """Diagnostic and test hook (include/mg_krylov_batch.h): the records of instance i of the last accelerated solve, one
        dict per iteration of that instance with the keys of Solver.krylov_log (k, d, g, h, alpha, rho_rec, restarted, rho);
        [] for an instance that never iterated or an i outside that solve."""
        fn = _need_krylov_batch("mg_batch_solver_krylov_log")
        n = fn(self._s, int(i), None, 0)
        if n <= 0:
            return []
        m = self._krylov_log_m   # (the m of that solve, noted by solve_ptrs: a record is m + 7 doubles)
        buf = np.zeros((n, m + 7))
        got = fn(self._s, int(i), buf.ctypes.data, n)
        return [dict(k=int(rec[0]), d=[float(v) for v in rec[1:1 + int(rec[0])]], g=float(rec[m + 1]), h=float(rec[m + 2]),
                     alpha=float(rec[m + 3]), rho_rec=float(rec[m + 4]), restarted=bool(rec[m + 5]), rho=float(rec[m + 6]))
                for rec in buf[:got]]

    def solve_ptrs(self, F_ptrs, U_ptrs):
        """F_ptrs, U_ptrs: sequences of device addresses of N x N fp64 arrays (16-byte aligned; F addresses may repeat),
        on the engine stream.  Returns one info dict per instance (the keys of Solver.solve_ptr, plus `stats` of the
        call: cycles = the most any instance ran, launches, device_ms; with set_krylov on, `breakdown` too)."""
        n = len(U_ptrs)
        if len(F_ptrs) != n:
            raise MGError(f"{len(F_ptrs)} F pointers for {n} U pointers")
        Fa = (C.c_void_p * max(n, 1))(*F_ptrs)
        Ua = (C.c_void_p * max(n, 1))(*U_ptrs)
        res = (SolveResult * max(n, 1))()
        st = BatchSolveStats()
        status = _lib.mg_batch_solver_solve(self._s, n, Fa, Ua, res, C.byref(st))
        if status > 0:
            _check()
            raise MGError(f"mg_batch_solver_solve failed with status {status}")
        stats = dict(status=status, cycles=st.cycles, launches=st.launches, device_ms=st.device_ms)
        out = []
        for r in res[:n]:
            out.append(dict(status=r.status, cycles=r.cycles, converged=bool(r.converged), coarse_capped=bool(r.coarse_capped),
                            res0=r.res0, res=r.res, ref_norm=r.ref_norm, device_ms=r.device_ms,
                            history=[r.history[i] for i in range(r.n_history)], stats=stats))
        if hasattr(_lib, "mg_batch_solver_krylov") and _lib.mg_batch_solver_krylov(self._s):
            self._krylov_log_m = int(_lib.mg_batch_solver_krylov(self._s))
            for i, info in enumerate(out):
                info["breakdown"] = bool(_lib.mg_batch_solver_krylov_breakdown(self._s, i))
        return out

    def solve(self, F, U=None):
        """F, U: numpy arrays [B, N, N], float64 torch CUDA tensors [B, N, N] (contiguous; worked on in place, on
        torch.cuda.current_stream()), or lists of B (N, N) arrays / tensors / DeviceGrids.  A single (N, N) F serves
        every instance (one shared array, no copy).  U = None starts from zero (zero rim).  Returns (U, infos); numpy
        input comes back as a new numpy array [B, N, N].  Torch instances that are not 16-byte aligned -- every odd
        instance of a contiguous [B, N, N] tensor with N odd -- go through a staging buffer whose instance pitch is
        N*N + 1 doubles (copied in and back on the same stream)."""
        if _is_torch(F if not isinstance(F, (list, tuple)) else F[0]) or \
                (U is not None and _is_torch(U if not isinstance(U, (list, tuple)) else U[0])):
            return self._solve_torch(F, U)
        return self._solve_host(F, U)

    def _solve_torch(self, F, U, run=None):
        import torch
        N = self.N
        Fs, shared = _instances(F, "F")
        if U is None:
            U = torch.zeros((1 if shared else len(Fs), N, N), dtype=torch.float64, device=Fs[0].device)
        Us, _ = _instances(U, "U")
        if shared:
            Fs = Fs * len(Us)
        if len(Fs) != len(Us):
            raise MGError(f"{len(Fs)} F instances for {len(Us)} U instances")
        for name, ts in (("F", Fs), ("U", Us)):
            for t in ts:
                if not (_is_torch(t) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (N, N)
                        and t.is_contiguous()):
                    raise MGError(f"{name}: expected contiguous float64 CUDA tensors of shape ({N}, {N})")
        dev = Us[0].device
        stream = torch.cuda.current_stream(dev)
        nn, B = N * N, len(Us)

        F_ptrs, Fbuf = _staged(Fs, shared, nn, dev)
        U_ptrs, Ubuf = _staged(Us, False, nn, dev)
        prev = _lib.mg_get_stream()
        _lib.mg_set_stream(stream.cuda_stream)
        try:
            infos = (run or self.solve_ptrs)(F_ptrs, U_ptrs)
        finally:
            _lib.mg_set_stream(prev)
        if Ubuf is not None:
            for i in range(B):
                Us[i].copy_(Ubuf[i, :nn].view(N, N))
        del Fbuf
        return U, infos

    def _solve_host(self, F, U, run=None):
        N = self.N
        keep = []

        def dev(a, what):
            if isinstance(a, DeviceGrid):
                if a.shape != (N, N):
                    raise MGError(f"{what}: DeviceGrid of shape {a.shape}, expected ({N}, {N})")
                return a
            a = np.asarray(a, dtype=np.float64)
            if a.shape != (N, N):
                raise MGError(f"{what}: array of shape {a.shape}, expected ({N}, {N})")
            g = DeviceGrid.from_host(a)
            keep.append(g)
            return g

        if isinstance(F, DeviceGrid):
            Fs, shared = [F], True
        else:
            Fs, shared = _instances(F if isinstance(F, (list, tuple)) else np.asarray(F), "F")
        Fd = [dev(f, "F") for f in Fs]
        if U is None:
            B = 1 if shared else len(Fd)
            Ud = [DeviceGrid.zeros((N, N)) for _ in range(B)]
            host_U = True
        else:
            Us = [U] if isinstance(U, DeviceGrid) else _instances(U if isinstance(U, (list, tuple)) else np.asarray(U), "U")[0]
            host_U = not all(isinstance(u, DeviceGrid) for u in Us)
            Ud = [dev(u, "U") for u in Us]
        if shared:
            Fd = Fd * len(Ud)
        if len(Fd) != len(Ud):
            raise MGError(f"{len(Fd)} F instances for {len(Ud)} U instances")
        infos = (run or self.solve_ptrs)([f.ptr for f in Fd], [u.ptr for u in Ud])
        if host_U:
            return np.stack([u.to_host() for u in Ud]), infos
        return Ud, infos

    def newton_ptrs(self, F_ptrs, U_ptrs, kind="sinh", kappa=1.0, w_ptrs=None, rtol=1e-8, atol=0.0, max_iters=20, max_backtracks=12):
        """mg_batch_solver_newton on sequences of device addresses of N x N fp64 arrays (16-byte aligned; U in/out), on the engine
        stream.  kappa: a scalar or a sequence of n; w_ptrs: None (w = 1), one address shared by every instance, or n.  Returns
        the list of the n info dicts of Solver.newton_ptr; its attribute `stats` holds the call's status, iterations (the most
        of any instance), trial_rounds, inner_cycles, launches and device_ms."""
        fn = _need_newton_batch("mg_batch_solver_newton")
        n = len(U_ptrs)
        if len(F_ptrs) != n:
            raise MGError(f"{len(F_ptrs)} F pointers for {n} U pointers")
        kap = np.asarray(kappa, dtype=np.float64)
        if kap.ndim > 1 or (kap.ndim == 1 and kap.shape[0] != n):
            raise MGError(f"[2] kappa: expected a scalar or {n} values, got shape {kap.shape}")
        kap = np.ascontiguousarray(np.broadcast_to(kap, (n,)))
        if w_ptrs is not None and not isinstance(w_ptrs, (list, tuple)):
            w_ptrs = [w_ptrs]
        n_w = 0 if w_ptrs is None else len(w_ptrs)
        arr = lambda ps: (C.c_void_p * max(len(ps), 1))(*ps)
        o = NewtonOpts(float(rtol), float(atol), int(max_iters), int(max_backtracks))
        res = (NewtonResult * max(n, 1))()
        st = BatchNewtonStats()
        status = fn(self._s, n, _newton_kind(kind), kap.ctypes.data, n_w, arr(w_ptrs) if n_w else None, arr(F_ptrs), arr(U_ptrs),
                    C.byref(o), res, C.byref(st))
        if status > 0:
            _check()
            raise MGError(f"mg_batch_solver_newton failed with status {status}")
        infos = BatchNewtonInfos()
        infos.stats = dict(status=status, iterations=st.iterations, trial_rounds=st.trial_rounds, inner_cycles=st.inner_cycles,
                           launches=st.launches, device_ms=st.device_ms)
        for i, r in enumerate(res[:n]):
            recs = (NewtonIter * max(r.n_history, 1))()
            got = _lib.mg_batch_solver_newton_history(self._s, i, recs, r.n_history)
            iters = [dict(res=x.res, t=x.t, backtracks=x.backtracks, inner_cycles=x.inner_cycles,
                          inner_converged=bool(x.inner_converged), inner_capped=bool(x.inner_capped)) for x in recs[:got]]
            infos.append(dict(status=r.status, iterations=r.iterations, converged=bool(r.converged), stalled=r.status == NEWTON_STALLED,
                              res0=r.res0, res=r.res, inner_cycles=r.inner_cycles, trials=r.trials,
                              history=[r.res0] + [x["res"] for x in iters[:r.iterations]], steps=iters,
                              last_inner_history=self._newton_inner_history(i) if iters else []))
        if hasattr(_lib, "mg_batch_solver_krylov") and _lib.mg_batch_solver_krylov(self._s):
            self._krylov_log_m = int(_lib.mg_batch_solver_krylov(self._s))   # (krylov_log(i): instance i's last inner solve)
        return infos

    def _newton_inner_history(self, i):
        n = _lib.mg_batch_solver_newton_inner_history(self._s, i, None, 0)
        buf = np.zeros(max(n, 1))
        got = _lib.mg_batch_solver_newton_inner_history(self._s, i, buf.ctypes.data, n)
        return [float(v) for v in buf[:got]]

    def newton_batch(self, F, U=None, kind="sinh", kappa=1.0, weight=None, rtol=1e-8, atol=0.0, max_iters=20, max_backtracks=12):
        """Solve B semilinear problems div(a_i grad U_i) - sigma*U_i - kappa_i*w_i*g(U_i) = F_i in one call: Solver.newton's
        Newton iteration with its backtracking line search for all instances in lockstep (include/mg_newton_batch.h).  Every
        instance is bit-identical to Solver(coef=a_i, krylov=m).newton(F_i, U_i, kind, kappa_i, w_i, ...) on it alone -- U and
        the whole info dict -- whatever the other instances are and wherever it sits in the batch.  kind ("cubic", "sinh",
        "exp"), rtol, atol, max_iters and max_backtracks are one per call, with Solver.newton's defaults; kappa is a scalar or a
        sequence of B; weight is None (w = 1), one (N, N) field shared by all, or B of them ((B, N, N) or a sequence), values
        finite and >= 0; a and GCR(m) are what set_coefficient and set_krylov have set.  F, U, weight: numpy arrays,
        DeviceGrids or float64 torch CUDA tensors, as solve() takes them (torch inputs run on torch.cuda.current_stream()).
        An instance that has converged, stalled or reached max_iters leaves the batch and is not written again; every Newton
        iteration and every line-search round is one set of launches over those that remain.  Returns (U, infos): infos[i]
        is the dict Solver.newton returns (status, iterations, converged, stalled, res0, res, inner_cycles, trials, history,
        steps, last_inner_history), infos.stats the call's status (0 when every instance converged, else -1), iterations,
        trial_rounds, inner_cycles, launches and device_ms.  Refused ("[3]") while set_reaction is on, and ("[2]") for a bad
        kappa, weight (the message names the instance), count or option, with every U untouched; the solver has no reaction
        afterwards, as before.  The first call allocates about 51*N^2*max_batch bytes; later calls allocate nothing.
        (The name is not `newton`: tests/test_newton_gpu.py pins that BatchSolver has no attribute of that name.)"""
        N = self.N
        opts = dict(kind=kind, kappa=kappa, rtol=rtol, atol=atol, max_iters=max_iters, max_backtracks=max_backtracks)
        if weight is None:
            ws = None
        elif isinstance(weight, (list, tuple)):
            ws = list(weight)
        elif len(weight.shape) == 3:
            ws = [weight[i] for i in range(weight.shape[0])]
        elif len(weight.shape) == 2:
            ws = [weight]
        else:
            raise MGError(f"[2] weight: expected (N, N), (B, N, N) or a sequence of (N, N) arrays, got shape {tuple(weight.shape)}")
        keep = []

        def run(F_ptrs, U_ptrs):   # (inside _solve_torch the engine is on the tensors' stream here)
            try:
                w_ptrs = None if ws is None else [_coefficient_address(N, w, keep) for w in ws]
            except MGError as e:
                raise MGError("[2] " + str(e).replace("coef:", "weight:", 1)) from None
            return self.newton_ptrs(F_ptrs, U_ptrs, w_ptrs=w_ptrs, **opts)

        first = lambda X: X[0] if isinstance(X, (list, tuple)) else X
        try:
            if _is_torch(first(F)) or (U is not None and _is_torch(first(U))):
                return self._solve_torch(F, U, run)
            return self._solve_host(F, U, run)
        finally:
            for g in keep:
                g.free()

    def adjoint_ptrs(self, Ubar_ptrs, U_ptrs, lam_ptrs, gA_ptrs=None, gU_ptrs=None):
        """mg_batch_solver_adjoint on sequences of device addresses (one N x N fp64 array per instance, 16-byte aligned), on the
        engine stream; gA_ptrs / gU_ptrs = None: that gradient is not wanted.  Returns one info dict per instance, as
        solve_ptrs does (stats.launches counts the two gradient launches too)."""
        n = len(lam_ptrs)
        arr = lambda ps: None if ps is None else (C.c_void_p * max(n, 1))(*ps)
        for ps in (Ubar_ptrs, U_ptrs, gA_ptrs, gU_ptrs):
            if ps is not None and len(ps) != n:
                raise MGError(f"{len(ps)} pointers for {n} instances")
        res = (SolveResult * max(n, 1))()
        st = BatchSolveStats()
        status = _need_adjoint("mg_batch_solver_adjoint")(self._s, n, arr(Ubar_ptrs), arr(U_ptrs), arr(lam_ptrs), arr(gA_ptrs),
                                                          arr(gU_ptrs), res, C.byref(st))
        if status > 0:
            _check()
            raise MGError(f"mg_batch_solver_adjoint failed with status {status}")
        stats = dict(status=status, cycles=st.cycles, launches=st.launches, device_ms=st.device_ms)
        out = [dict(_solve_info(r), stats=stats) for r in res[:n]]
        if hasattr(_lib, "mg_batch_solver_krylov") and _lib.mg_batch_solver_krylov(self._s):
            self._krylov_log_m = int(_lib.mg_batch_solver_krylov(self._s))
            for i, info in enumerate(out):
                info["breakdown"] = bool(_lib.mg_batch_solver_krylov_breakdown(self._s, i))
        return out

    def adjoint(self, Ubar, U, want_coef=True, want_rim=True):
        """Solver.adjoint for B instances in one call (include/mg_adjoint.h): returns (lam, gA, gU, infos), every instance
        bit-identical to Solver(coef=a_i).adjoint(Ubar_i, U_i) alone.  The adjoint solves run as one batched solve and each
        gradient is ONE launch over all instances, those that left the batch early included.  Ubar, U: numpy arrays
        [B, N, N] (results are numpy arrays [B, N, N]), float64 torch CUDA tensors [B, N, N] (results are tensors; on
        torch.cuda.current_stream()) or lists of B (N, N) arrays / tensors / DeviceGrids (DeviceGrids give lists of
        DeviceGrids).  With a coefficient shared by the instances gA[i] is instance i's own sensitivity; the gradient in the
        shared a is the caller's sum over i."""
        N, nn = self.N, self.N * self.N
        first = Ubar[0] if isinstance(Ubar, (list, tuple)) else Ubar
        if _is_torch(first):
            import torch
            Ubs, _ = _instances(Ubar, "Ubar")
            Us, _ = _instances(U, "U")
            if len(Ubs) != len(Us):
                raise MGError(f"{len(Ubs)} Ubar instances for {len(Us)} U instances")
            for name, ts in (("Ubar", Ubs), ("U", Us)):
                for t in ts:
                    if not (_is_torch(t) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (N, N) and t.is_contiguous()):
                        raise MGError(f"{name}: expected contiguous float64 CUDA tensors of shape ({N}, {N})")
            dev, B = Ubs[0].device, len(Ubs)
            ub_ptrs, ub_buf = _staged(Ubs, False, nn, dev)
            u_ptrs, u_buf = _staged(Us, False, nn, dev)
            pitch = nn + nn % 2   # (every instance of an output 16-byte aligned)

            def out():
                return torch.empty((B, pitch), dtype=torch.float64, device=dev)

            def ptrs(buf):
                return None if buf is None else [buf[i].data_ptr() for i in range(B)]

            def done(buf):
                return None if buf is None else buf[:, :nn].reshape(B, N, N)

            lam, gA, gU = out(), out() if want_coef else None, out() if want_rim else None
            prev = _lib.mg_get_stream()
            _lib.mg_set_stream(torch.cuda.current_stream(dev).cuda_stream)
            try:
                infos = self.adjoint_ptrs(ub_ptrs, u_ptrs, ptrs(lam), ptrs(gA), ptrs(gU))
            finally:
                _lib.mg_set_stream(prev)
            del ub_buf, u_buf
            return done(lam), done(gA), done(gU), infos
        keep = []

        def dev(a, what):
            if hasattr(a, "ptr") and hasattr(a, "shape"):
                if tuple(a.shape) != (N, N):
                    raise MGError(f"{what}: DeviceGrid of shape {a.shape}, expected ({N}, {N})")
                return a
            a = np.asarray(a, dtype=np.float64)
            if a.shape != (N, N):
                raise MGError(f"{what}: array of shape {a.shape}, expected ({N}, {N})")
            g = DeviceGrid.from_host(a)
            keep.append(g)
            return g

        def many(X, what):
            if hasattr(X, "ptr"):
                return [X]
            return _instances(X if isinstance(X, (list, tuple)) else np.asarray(X), what)[0]

        Ubs, Us = many(Ubar, "Ubar"), many(U, "U")
        if len(Ubs) != len(Us):
            raise MGError(f"{len(Ubs)} Ubar instances for {len(Us)} U instances")
        host = not all(hasattr(x, "ptr") for x in list(Ubs) + list(Us))
        Ub, Ud = [dev(x, "Ubar") for x in Ubs], [dev(x, "U") for x in Us]
        B = len(Ub)
        lam = [DeviceGrid((N, N)) for _ in range(B)]
        gA = [DeviceGrid((N, N)) for _ in range(B)] if want_coef else None
        gU = [DeviceGrid((N, N)) for _ in range(B)] if want_rim else None
        ptrs = lambda gs: None if gs is None else [g.ptr for g in gs]
        infos = self.adjoint_ptrs(ptrs(Ub), ptrs(Ud), ptrs(lam), ptrs(gA), ptrs(gU))
        if host:
            back = lambda gs: None if gs is None else np.stack([g.to_host() for g in gs])
            return back(lam), back(gA), back(gU), infos
        return lam, gA, gU, infos

    def adjoint_reaction(self, Ubar, U, want_coef=True, want_rim=True, want_reaction=True):
        """Solver.adjoint_reaction for B instances in one call (include/mg_adjoint_rx.h): returns (lam, gA, gU, gS, infos), every
        instance bit-identical to Solver(reaction=s_i, coef=a_i).adjoint_reaction(Ubar_i, U_i) alone, infos[i]["gshift"] its
        dJ/dsigma.  The adjoint solves run as one batched solve and each gradient is ONE launch over all instances.  Ubar, U:
        [B, N, N] numpy arrays or float64 torch CUDA tensors, or lists of B (N, N) arrays / tensors / DeviceGrids, as adjoint()
        takes them.  With a reaction term or a coefficient shared by the instances gS[i] and gA[i] are instance i's own
        sensitivities; the gradient in the shared field is the caller's sum over i."""
        fn = _need_adjoint_rx("mg_batch_solver_adjoint_reaction")
        io = _AdjointIO(self.N, [Ubar, U])
        ubs = io.many(Ubar, "Ubar")
        B = len(ubs)
        us = io.many(U, "U", B)
        lam, gA, gU, gS = io.out(B=B), io.out(want_coef, B), io.out(want_rim, B), io.out(want_reaction, B)
        res, st, gshift = (SolveResult * max(B, 1))(), BatchSolveStats(), np.zeros(B)
        status = io.run(lambda: fn(self._s, B, _void_array(ubs), _void_array(us), _void_array(io.ptr(lam)), _void_array(io.ptr(gA)),
                                   _void_array(io.ptr(gU)), _void_array(io.ptr(gS)), gshift.ctypes.data if want_reaction else None, res,
                                   C.byref(st)))
        if status > 0:
            _check()
            raise MGError(f"mg_batch_solver_adjoint_reaction failed with status {status}")
        infos = _batch_adjoint_infos(self, status, res, st, B)
        for i, info in enumerate(infos):
            info["gshift"] = float(gshift[i]) if want_reaction else None
        return io.result(lam, True), io.result(gA, True), io.result(gU, True), io.result(gS, True), infos

    def newton_adjoint_batch(self, Ubar, U, F, kind="sinh", kappa=1.0, weight=None, want_coef=True, want_rim=True, want_weight=True):
        """Solver.newton_adjoint for B instances in one call (include/mg_adjoint_rx.h): returns (lam, gA, gU, gW, infos), every
        instance bit-identical to Solver(coef=a_i).newton_adjoint(Ubar_i, U_i, F_i, kind, kappa_i, w_i) alone, infos[i]["gkappa"]
        and infos[i]["res_forward"] its own.  ONE pass over all instances forms the Newton matrices, one batched solve gives the
        adjoint fields, each gradient is one launch.  kappa: a scalar or a sequence of B; weight: None, one (N, N) field shared
        by all (gW[i] is then instance i's own sensitivity, the gradient in the shared w the caller's sum) or B of them.  Ubar, U,
        F: [B, N, N] numpy arrays or float64 torch CUDA tensors, or lists of B.  The solver has no reaction afterwards."""
        fn = _need_adjoint_rx("mg_batch_solver_newton_adjoint")
        io = _AdjointIO(self.N, [Ubar, U, F])
        ubs = io.many(Ubar, "Ubar")
        B = len(ubs)
        us, fs = io.many(U, "U", B), io.many(F, "F", B)
        if weight is None:
            ws = None
        elif hasattr(weight, "ptr") or (not isinstance(weight, (list, tuple)) and len(weight.shape) == 2):
            ws = [io.inp(weight, "weight")]
        else:
            ws = io.many(weight, "weight")   # (a count other than 1 or B: the library refuses it)
        kap = np.asarray(kappa, dtype=np.float64)
        if kap.ndim > 1 or (kap.ndim == 1 and kap.shape[0] != B):
            raise MGError(f"[2] kappa: expected a scalar or {B} values, got shape {kap.shape}")
        kap = np.ascontiguousarray(np.broadcast_to(kap, (B,)))
        lam, gA, gU, gW = io.out(B=B), io.out(want_coef, B), io.out(want_rim, B), io.out(want_weight, B)
        res, st, gkappa, resf = (SolveResult * max(B, 1))(), BatchSolveStats(), np.zeros(B), np.zeros(B)
        status = io.run(lambda: fn(self._s, B, _newton_kind(kind), kap.ctypes.data, 0 if ws is None else len(ws), _void_array(ws),
                                   _void_array(fs), _void_array(us), _void_array(ubs), _void_array(io.ptr(lam)), _void_array(io.ptr(gA)),
                                   _void_array(io.ptr(gU)), _void_array(io.ptr(gW)), gkappa.ctypes.data if want_weight else None,
                                   resf.ctypes.data, res, C.byref(st)))
        if status > 0:
            _check()
            raise MGError(f"mg_batch_solver_newton_adjoint failed with status {status}")
        infos = _batch_adjoint_infos(self, status, res, st, B)
        for i, info in enumerate(infos):
            info["gkappa"] = float(gkappa[i]) if want_weight else None
            info["res_forward"] = float(resf[i])
        return io.result(lam, True), io.result(gA, True), io.result(gU, True), io.result(gW, True), infos

    def close(self):
        if getattr(self, "_s", None) and _initialised:
            _lib.mg_batch_solver_destroy(self._s)
        self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve_batched(F, U=None, L=1.0, **opts):
    """Solve B Poisson problems of one size to the residual tolerance in one batched call; returns (U, infos).  F: [B, N, N]
    (or a list, or one (N, N) F shared by every instance when U gives B), U: the initial guesses with their Dirichlet rims
    (None: zero).  See BatchSolver for the accepted types and solve_opts for the defaults.  shift=sigma solves
    Laplace(U) - sigma*U = F for every instance: one implicit time step of B fields, sigma = 1/(nu*dt), F_i = -u_old_i/(nu*dt)."""
    Fs, shared = _instances(F, "F") if not isinstance(F, DeviceGrid) else ([F], True)
    if U is None:
        B = 1 if shared else len(Fs)
    else:
        B = len(U) if isinstance(U, (list, tuple)) else (1 if isinstance(U, DeviceGrid) or len(U.shape) == 2 else int(U.shape[0]))
    N = int(Fs[0].shape[-1])
    s = BatchSolver(N, L, max_batch=max(B, 1), **opts)
    try:
        return s.solve(F, U)
    finally:
        s.close()


def solve_batched_coef(F, a, U=None, L=1.0, **opts):
    """solve_batched with a variable coefficient: B problems div(a_i grad U_i) - sigma*U_i = F_i in one batched call; returns
    (U, infos).  a: (N, N), shared by every instance, or (B, N, N) / a sequence of B (N, N) ones, one per instance
    (BatchSolver.set_coefficient); F and U as solve_batched takes them.  Every instance is bit-identical to
    solve(F_i, U_i, L, coef=a_i, ...); a == 1 everywhere is solve_batched, bit for bit."""
    Fs, shared = _instances(F, "F") if not isinstance(F, DeviceGrid) else ([F], True)
    if U is None:
        B = 1 if shared else len(Fs)
    else:
        B = len(U) if isinstance(U, (list, tuple)) else (1 if isinstance(U, DeviceGrid) or len(U.shape) == 2 else int(U.shape[0]))
    n_a = len(a) if isinstance(a, (list, tuple)) else (int(a.shape[0]) if len(a.shape) == 3 else 1)
    N = int(Fs[0].shape[-1])
    s = BatchSolver(N, L, max_batch=max(B, n_a, 1), **opts)
    try:
        s.set_coefficient(a)
        return s.solve(F, U)
    finally:
        s.close()


def solve_batched_krylov(F, m, U=None, L=1.0, coef=None, **opts):
    """solve_batched with restarted GCR(m) around the cycle of every instance (BatchSolver.set_krylov, include/mg_krylov_batch.h);
    returns (U, infos), infos[i] with `breakdown`.  coef: None, or what solve_batched_coef takes as a -- (N, N) shared by every
    instance, or (B, N, N) / a sequence of B (N, N) ones; F and U as solve_batched takes them.  Every instance is
    bit-identical to solve(F_i, U_i, L, coef=a_i, krylov=m, ...) alone, and is stated converged on a recomputed residual
    only.  Allocates (2m + 1)*N^2*B doubles beside the batch solver's own arrays for the call."""
    Fs, shared = _instances(F, "F") if not isinstance(F, DeviceGrid) else ([F], True)
    if U is None:
        B = 1 if shared else len(Fs)
    else:
        B = len(U) if isinstance(U, (list, tuple)) else (1 if isinstance(U, DeviceGrid) or len(U.shape) == 2 else int(U.shape[0]))
    n_a = 0 if coef is None else len(coef) if isinstance(coef, (list, tuple)) else (int(coef.shape[0]) if len(coef.shape) == 3 else 1)
    N = int(Fs[0].shape[-1])
    s = BatchSolver(N, L, max_batch=max(B, n_a, 1), **opts)
    try:
        if coef is not None:
            s.set_coefficient(coef)
        s.set_krylov(m)
        return s.solve(F, U)
    finally:
        s.close()


def solve_batched_reaction(F, s, U=None, L=1.0, coef=None, krylov=0, **opts):
    """solve_batched with a variable reaction term: B problems div(a_i grad U_i) - (sigma + s_i)*U_i = F_i in one batched call;
    returns (U, infos).  s: (N, N), shared by every instance, or (B, N, N) / a sequence of B (N, N) ones, one per instance
    (BatchSolver.set_reaction); coef: None, or what solve_batched_coef takes as a; krylov = m > 0 wraps every instance in
    GCR(m) (BatchSolver.set_krylov); F and U as solve_batched takes them.  Every instance is bit-identical to
    solve(F_i, U_i, L, reaction=s_i, coef=a_i, krylov=m, ...) alone; s == 0 everywhere is solve_batched, bit for bit."""
    Fs, shared = _instances(F, "F") if not isinstance(F, DeviceGrid) else ([F], True)
    if U is None:
        B = 1 if shared else len(Fs)
    else:
        B = len(U) if isinstance(U, (list, tuple)) else (1 if isinstance(U, DeviceGrid) or len(U.shape) == 2 else int(U.shape[0]))
    count = lambda x: 0 if x is None else len(x) if isinstance(x, (list, tuple)) else (int(x.shape[0]) if len(x.shape) == 3 else 1)
    N = int(Fs[0].shape[-1])
    b = BatchSolver(N, L, max_batch=max(B, count(s), count(coef), 1), **opts)
    try:
        if coef is not None:
            b.set_coefficient(coef)
        b.set_reaction(s)
        if krylov:
            b.set_krylov(krylov)
        return b.solve(F, U)
    finally:
        b.close()


def solve_semilinear_batched(F, U=None, L=1.0, kind="sinh", kappa=1.0, weight=None, coef=None, krylov=0, rtol=1e-8, atol=0.0,
                             max_iters=20, max_backtracks=12, inner_rtol=None, inner_atol=None, **opts):
    """solve_semilinear for B problems in one batched call (BatchSolver.newton_batch, include/mg_newton_batch.h); returns (U, infos),
    infos.stats holding the call's figures.  F and U as solve_batched takes them; kappa: a scalar or B values; weight: None,
    (N, N) shared by every instance, or (B, N, N) / a sequence of B; coef: None, or what solve_batched_coef takes as a; krylov =
    m > 0 wraps every inner solve in GCR(m); kind, rtol, atol, max_iters and max_backtracks are the Newton iteration's, one set
    for the batch; inner_rtol / inner_atol and **opts (shift, max_cycles, omega, ...) make the BatchSolver every Newton step
    runs on.  Every instance is bit-identical to solve_semilinear(F_i, U_i, L, kind, kappa_i, w_i, coef=a_i, krylov=m, ...)."""
    Fs, shared = _instances(F, "F") if not isinstance(F, DeviceGrid) else ([F], True)
    if U is None:
        B = 1 if shared else len(Fs)
    else:
        B = len(U) if isinstance(U, (list, tuple)) else (1 if isinstance(U, DeviceGrid) or len(U.shape) == 2 else int(U.shape[0]))
    count = lambda x: 0 if x is None else len(x) if isinstance(x, (list, tuple)) else (int(x.shape[0]) if len(x.shape) == 3 else 1)
    for name, v in (("rtol", inner_rtol), ("atol", inner_atol)):
        if v is not None:
            opts[name] = v
    N = int(Fs[0].shape[-1])
    b = BatchSolver(N, L, max_batch=max(B, count(coef), 1), **opts)
    try:
        if coef is not None:
            b.set_coefficient(coef)
        if krylov:
            b.set_krylov(krylov)
        return b.newton_batch(F, U, kind=kind, kappa=kappa, weight=weight, rtol=rtol, atol=atol, max_iters=max_iters,
                        max_backtracks=max_backtracks)
    finally:
        b.close()


def _need_adjoint(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name}: rebuild it (the adjoint sensitivities are not in this library)")
    return getattr(_lib, name)


def _solve_info(res):
    """a SolveResult as the info dict of Solver.solve_ptr"""
    return dict(status=res.status, cycles=res.cycles, converged=bool(res.converged), coarse_capped=bool(res.coarse_capped),
                res0=res.res0, res=res.res, ref_norm=res.ref_norm, device_ms=res.device_ms,
                history=[res.history[i] for i in range(res.n_history)])


def coefficientGradient(N, L, lam, U, gA=None):
    """mg_coefficientGradient on DeviceGrids (include/mg_adjoint.h): gA = dJ/da at every grid point, rim included, from the
    adjoint field lam and the forward solution U,  gA_k = 0.5*inv*((((0 + tN) + tS) + tE) + tW),
    tX = (lam'_k - lam'_q)*(U_k - U_q) over the neighbours q inside the grid, lam' = lam with its rim taken as +0 (the rim
    of lam is never used).  gA = None: a new DeviceGrid.  lam and U are read only; returns gA."""
    fn = _need_adjoint("mg_coefficientGradient")
    if gA is None:
        gA = DeviceGrid((N, N))
    fn(int(N), float(L), lam.ptr, U.ptr, gA.ptr)
    _check()
    return gA


def boundaryGradient(N, L, a, lam, Ubar=None, gU=None):
    """mg_boundaryGradient on DeviceGrids (include/mg_adjoint.h): gU = dJ/d(rim data) as an N x N array -- 0 inside, Ubar at
    the corners, Ubar[b] - inv*(0.5*(a[b] + a[p])*lam[p]) at a rim point b with interior neighbour p.  a = None: a = 1;
    Ubar = None: 0.  gU = None: a new DeviceGrid.  a, lam and Ubar are read only; returns gU."""
    fn = _need_adjoint("mg_boundaryGradient")
    if gU is None:
        gU = DeviceGrid((N, N))
    fn(int(N), float(L), a.ptr if a is not None else None, lam.ptr, Ubar.ptr if Ubar is not None else None, gU.ptr)
    _check()
    return gU


def _optional_pointer_array(views, n):
    if views is None:
        return None
    return (C.c_void_p * max(n, 1))(*[v.ptr if v is not None else None for v in views])


def coefficientGradient_batch(N, L, lam, U, gA):
    """mg_coefficientGradient_batch on sequences of DeviceGrids: coefficientGradient for every instance in ONE launch, each
    bit-identical to the single call.  Returns gA."""
    n = len(gA)
    _need_adjoint("mg_coefficientGradient_batch")(n, int(N), float(L), _optional_pointer_array(lam, n), _optional_pointer_array(U, n),
                                                  _optional_pointer_array(gA, n))
    _check()
    return gA


def boundaryGradient_batch(N, L, a, lam, Ubar, gU):
    """mg_boundaryGradient_batch on sequences of DeviceGrids: boundaryGradient for every instance in ONE launch, each
    bit-identical to the single call.  a and Ubar may be None, and so may entries of them (a = 1, Ubar = 0 for that
    instance).  Returns gU."""
    n = len(gU)
    _need_adjoint("mg_boundaryGradient_batch")(n, int(N), float(L), _optional_pointer_array(a, n), _optional_pointer_array(lam, n),
                                               _optional_pointer_array(Ubar, n), _optional_pointer_array(gU, n))
    _check()
    return gU


# ---------------------------------------------------------------- the adjoint of reaction and semilinear solves
def _need_adjoint_rx(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name}: rebuild it (the adjoint of reaction and semilinear solves is not in this library)")
    return getattr(_lib, name)


def _grad_kind(kind):
    if kind in GRAD_KINDS:
        return GRAD_KINDS[kind]
    if isinstance(kind, str):
        raise MGError(f"kind {kind!r}: expected one of {sorted(GRAD_KINDS)}")
    return int(kind)   # (a number goes to the library, which refuses one it does not know)


class _AdjointIO:
    """The arrays of one adjoint call in the caller's form, as Solver.adjoint handles them: float64 torch CUDA tensors (outputs
    are tensors, the engine runs on torch.cuda.current_stream()), DeviceGrids (outputs are DeviceGrids) or numpy arrays
    (uploaded for the call; outputs come back as new numpy arrays).  `samples`: the inputs that decide the form."""

    def __init__(self, N, samples):
        flat = []
        for x in samples:
            flat += list(x) if isinstance(x, (list, tuple)) else [x]
        flat = [x for x in flat if x is not None]
        self.N, self.nn = N, N * N
        self.torch = any(_is_torch(x) for x in flat)
        self.host = not self.torch and not all(hasattr(x, "ptr") for x in flat)
        self.device = next(x.device for x in flat if _is_torch(x)) if self.torch else None
        self.keep = []

    def inp(self, x, what):
        """the device address of one N x N input (None stays None)"""
        N = self.N
        if x is None:
            return None
        if self.torch:
            import torch
            if not (_is_torch(x) and x.is_cuda and x.dtype == torch.float64 and tuple(x.shape) == (N, N) and x.is_contiguous()):
                raise MGError(f"{what}: expected a contiguous float64 CUDA tensor of shape ({N}, {N})")
            (p,), buf = _staged([x], False, self.nn, self.device)
            self.keep.append(buf)
            return p
        if hasattr(x, "ptr") and hasattr(x, "shape"):
            if tuple(x.shape) != (N, N):
                raise MGError(f"{what}: DeviceGrid of shape {x.shape}, expected ({N}, {N})")
            return x.ptr
        a = np.asarray(x, dtype=np.float64)
        if a.shape != (N, N):
            raise MGError(f"{what}: array of shape {a.shape}, expected ({N}, {N})")
        g = DeviceGrid.from_host(a)
        self.keep.append(g)
        return g.ptr

    def many(self, X, what, B=None):
        """the addresses of B inputs: [B, N, N], a list of (N, N), or one (N, N) / DeviceGrid for every instance"""
        if hasattr(X, "ptr"):
            xs, shared = [X], True
        else:
            xs, shared = _instances(X if isinstance(X, (list, tuple)) or _is_torch(X) else np.asarray(X), what)
        ps = [self.inp(x, what) for x in xs]
        if shared and B is not None:
            ps = ps * B
        if B is not None and len(ps) != B:
            raise MGError(f"{len(ps)} {what} instances for {B} instances")
        return ps

    def out(self, wanted=True, B=None):
        """one N x N output (B: a list of B), 16-byte aligned; None when it is not wanted"""
        if not wanted:
            return None
        if self.torch:
            import torch
            if B is None:
                return torch.empty((self.N, self.N), dtype=torch.float64, device=self.device)
            return torch.empty((B, self.nn + self.nn % 2), dtype=torch.float64, device=self.device)
        return DeviceGrid((self.N, self.N)) if B is None else [DeviceGrid((self.N, self.N)) for _ in range(B)]

    def ptr(self, h):
        if h is None:
            return None
        if self.torch:
            return h.data_ptr() if h.dim() == 2 and tuple(h.shape) == (self.N, self.N) else [h[i].data_ptr() for i in range(h.shape[0])]
        return [g.ptr for g in h] if isinstance(h, list) else h.ptr

    def result(self, h, batched=False):
        if h is None:
            return None
        if self.torch:
            return h[:, :self.nn].reshape(h.shape[0], self.N, self.N) if batched else h
        if self.host:
            return np.stack([g.to_host() for g in h]) if batched else h.to_host()
        return h

    def run(self, call):
        """call() with the engine on the tensors' stream"""
        if not self.torch:
            return call()
        import torch
        prev = _lib.mg_get_stream()
        _lib.mg_set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        try:
            return call()
        finally:
            _lib.mg_set_stream(prev)


def _void_array(ps):
    return None if ps is None else (C.c_void_p * max(len(ps), 1))(*ps)


def sourceGradient(N, kind, kappa, w, lam, U, G=None):
    """mg_sourceGradient (include/mg_adjoint_rx.h): G = kappa*(lam'*g(U)) on the interior and +0 on the rim, lam' = lam with its
    rim taken as +0, and sum = the sum over the interior of w*(lam'*g(U)) (w = None: of lam'*g(U)) in the order of the semilinear
    pass's norm.  kind: "cubic", "sinh", "exp" or "linear" (g(u) = u).  w, lam, U: numpy arrays, DeviceGrids or float64 torch
    CUDA tensors; G = None: a new array of the inputs' form.  Returns (G, sum)."""
    fn = _need_adjoint_rx("mg_sourceGradient")
    io = _AdjointIO(N, [lam, U])
    wp, lp, up = io.inp(w, "w"), io.inp(lam, "lam"), io.inp(U, "U")
    made = G is None
    if made:
        G = io.out()
    gp = io.ptr(G) if made else (G.data_ptr() if _is_torch(G) else G.ptr)
    s = C.c_double(0.0)
    status = io.run(lambda: fn(int(N), _grad_kind(kind), float(kappa), wp, lp, up, gp, C.byref(s)))
    if status:
        _check()
        raise MGError(f"mg_sourceGradient failed with status {status}")
    return (io.result(G) if made else G), float(s.value)


def sourceGradient_batch(N, kind, kappa, w, lam, U, G=None):
    """mg_sourceGradient_batch: sourceGradient for every instance in ONE launch, each bit-identical to the single call.  kappa: a
    scalar or a sequence of B; w: None, one (N, N) field shared by all, or B of them; lam, U: [B, N, N] or sequences of B.
    G = None: new arrays of the inputs' form, else a sequence of B DeviceGrids.  Returns (G, sums), sums a numpy array of B."""
    fn = _need_adjoint_rx("mg_sourceGradient_batch")
    io = _AdjointIO(N, [lam, U])
    lps = io.many(lam, "lam")
    B = len(lps)
    ups = io.many(U, "U", B)
    if w is None:
        wps = None
    elif hasattr(w, "ptr") or (not isinstance(w, (list, tuple)) and len(w.shape) == 2):
        wps = [io.inp(w, "w")]
    else:
        wps = io.many(w, "w")   # (a count other than 1 or B: the library refuses it)
    kap = np.asarray(kappa, dtype=np.float64)
    if kap.ndim > 1 or (kap.ndim == 1 and kap.shape[0] != B):
        raise MGError(f"[2] kappa: expected a scalar or {B} values, got shape {kap.shape}")
    kap = np.ascontiguousarray(np.broadcast_to(kap, (B,)))
    made = G is None
    if made:
        G = io.out(B=B)
    gps = io.ptr(G) if made else [g.ptr for g in G]
    sums = np.zeros(B)
    status = io.run(lambda: fn(B, int(N), _grad_kind(kind), kap.ctypes.data, 0 if wps is None else len(wps), _void_array(wps),
                               _void_array(lps), _void_array(ups), _void_array(gps), sums.ctypes.data))
    if status:
        _check()
        raise MGError(f"mg_sourceGradient_batch failed with status {status}")
    return (io.result(G, batched=True) if made else G), sums


def _batch_adjoint_infos(self, status, res, st, n):
    stats = dict(status=status, cycles=st.cycles, launches=st.launches, device_ms=st.device_ms)
    out = [dict(_solve_info(r), stats=stats) for r in res[:n]]
    if hasattr(_lib, "mg_batch_solver_krylov") and _lib.mg_batch_solver_krylov(self._s):
        self._krylov_log_m = int(_lib.mg_batch_solver_krylov(self._s))
        for i, info in enumerate(out):
            info["breakdown"] = bool(_lib.mg_batch_solver_krylov_breakdown(self._s, i))
    return out


def _need_krylov_batch(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name}: rebuild it (the batched Krylov acceleration is not in this library)")
    return getattr(_lib, name)


def _need_vc_batch(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name}: rebuild it (the batched variable-coefficient solver is not in this library)")
    return getattr(_lib, name)


def _need_rx_batch(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name}: rebuild it (the batched reaction solver is not in this library)")
    return getattr(_lib, name)


def _need_eigs(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name}: rebuild it (the eigen-solver is not in this library)")
    return getattr(_lib, name)


def eigs_default_guard(k):
    """the guard columns EigenSolver(guard=None) takes: min(max(2, k // 2), MG_EIGS_MAX_BLOCK - k)"""
    return min(max(2, int(k) // 2), MG_EIGS_MAX_BLOCK - int(k))


def eigsGram(N, S, AS):
    """Test hook (include/mg_eigs.h).  mg_eigsGram on lists of m DeviceGrids: (G, H), G[j, l] = <S[j], S[l]>,
    H[j, l] = <S[j], AS[l]> for j <= l over the interior, both mirrored; one pass, nothing on the device is written."""
    m = len(S)
    assert len(AS) == m
    G, H = np.zeros((m, m)), np.zeros((m, m))
    status = _need_eigs("mg_eigsGram")(int(N), m, _pointer_array(S), _pointer_array(AS), G.ctypes.data, H.ctypes.data)
    if status:
        _check()
        raise MGError(f"mg_eigsGram failed with status {status}")
    return G, H


def eigsRotate(N, C_, Cp, theta, S, AS, R):
    """Test hook (include/mg_eigs.h).  mg_eigsRotate on DeviceGrids, in place: C_, Cp of shape (m, p), theta of p values; S, AS:
    lists of 3p DeviceGrids of which the first m are read; written on the interior: S[i] = X'_i, AS[i] = AX'_i,
    S[2p + i] = P'_i, AS[2p + i] = AP'_i, R[i] = AX'_i - theta_i*X'_i.  Returns [<R_i, R_i>]."""
    C_ = np.ascontiguousarray(C_, dtype=np.float64)
    Cp = np.ascontiguousarray(Cp, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    m, p = C_.shape
    assert Cp.shape == (m, p) and theta.shape == (p,) and len(S) == len(AS) == 3 * p and len(R) == p
    res2 = np.zeros(p)
    status = _need_eigs("mg_eigsRotate")(int(N), m, p, C_.ctypes.data, Cp.ctypes.data, theta.ctypes.data, _pointer_array(S),
                                         _pointer_array(AS), _pointer_array(R), res2.ctypes.data)
    if status:
        _check()
        raise MGError(f"mg_eigsRotate failed with status {status}")
    return res2


def eigsRayleighRitz(G, H, p):
    """Test hook (include/mg_eigs.h).  The host Rayleigh-Ritz step on G, H (m x m): (kept, C, Cp, theta); kept < p is the
    breakdown, C, Cp, theta are then None.  Needs no device."""
    load_library()
    G = np.ascontiguousarray(G, dtype=np.float64)
    H = np.ascontiguousarray(H, dtype=np.float64)
    m = G.shape[0]
    C_, Cp, theta = np.zeros((m, p)), np.zeros((m, p)), np.zeros(p)
    if not hasattr(_lib, "mg_eigsRayleighRitz"):
        raise MGError(f"{LIB_PATH} does not export mg_eigsRayleighRitz: rebuild it (the eigen-solver is not in this library)")
    kept = _lib.mg_eigsRayleighRitz(m, int(p), G.ctypes.data, H.ctypes.data, C_.ctypes.data, Cp.ctypes.data, theta.ctypes.data)
    if kept < p:
        return kept, None, None, None
    return kept, C_, Cp, theta


class EigenSolver:
    """The k lowest eigenmodes of -div(a grad u) on the N x N vertex grid with a zero rim (include/mg_eigs.h): LOBPCG on the
    basis [X, W, P] with one V(pre, post) cycle as the preconditioner, k + guard columns in every launch.
        e = EigenSolver(N, L, k=4, coef=a); lam, X, info = e.solve(); e.close()
    lam ascending, X of shape (k, N, N) with orthonormal interiors and a zero rim.  guard=None takes
    min(max(2, k // 2), 12 - k) guard columns: a block that cuts a cluster of eigenvalues without them may not converge.
    cycle_opts are solve_opts' pre, post, omega, N_min and coarse targets; shift and fmg are refused (the eigenvalues of the
    shifted operator are lam + shift with the same vectors).  Everything is allocated here -- about 8(k + guard) fields; a
    solve allocates nothing on the device beyond the result it returns."""

    def __init__(self, N, L=1.0, k=1, guard=None, coef=None, rtol=1e-8, atol=0.0, max_iters=60, **cycle_opts):
        self.N, self.L, self.k = int(N), float(L), int(k)
        self.guard = eigs_default_guard(k) if guard is None else int(guard)
        o = EigsOpts()
        _need_eigs("mg_eigs_opts_default")(C.byref(o))
        o.cycle = solve_opts(**cycle_opts)
        o.k, o.guard, o.max_iters, o.rtol, o.atol = self.k, self.guard, int(max_iters), float(rtol), float(atol)
        self.opts = o
        self._e = _need_eigs("mg_eigs_create")(self.N, self.L, C.byref(o))
        if not self._e:
            _check()
            raise MGError("mg_eigs_create returned NULL")
        if coef is not None:
            try:
                self.set_coefficient(coef)
            except Exception:
                self.close()
                raise

    def set_coefficient(self, a):
        """a: (N, N) nodal coefficient shared by all columns (numpy array, DeviceGrid or float64 torch CUDA tensor, finite and
        > 0, copied); None: back to a = 1.  A refusal (MGError "[2] ...") leaves the earlier coefficient."""
        _set_coefficient(_need_eigs("mg_eigs_set_coefficient"), self._e, self.N, a)

    def solve_ptrs(self, X_ptrs, use_start=False, seed=0):
        """X_ptrs: k device addresses of N x N fp64 arrays (16-byte aligned), on the engine stream.  Returns (lam, info)."""
        if len(X_ptrs) != self.k:
            raise MGError(f"{len(X_ptrs)} vectors for k = {self.k}")
        lam, res = np.zeros(self.k), np.zeros(self.k)
        r = EigsResult()
        status = _lib.mg_eigs_solve(self._e, (C.c_void_p * self.k)(*X_ptrs), int(bool(use_start)), int(seed), lam.ctypes.data,
                                    res.ctypes.data, C.byref(r))
        if status > 0:
            _check()
            raise MGError(f"mg_eigs_solve failed with status {status}")
        return lam, dict(status=r.status, iters=r.iters, converged=bool(r.converged), breakdown=bool(r.breakdown),
                         restarts=r.restarts, cycles=r.cycles, coarse_capped=bool(r.coarse_capped), res=res)

    def solve(self, X0=None, seed=0):
        """X0 = None: a random start from `seed`.  X0 of shape (k, N, N) -- a numpy array, a list of k (N, N) arrays or
        DeviceGrids, or a contiguous float64 torch CUDA tensor (worked on in place, on torch.cuda.current_stream()) --: its
        interiors start the k columns (the guard columns are random).  Returns (lam, X, info): X a numpy array (k, N, N),
        the list of DeviceGrids, or the tensor."""
        N, k = self.N, self.k
        first = X0[0] if isinstance(X0, (list, tuple)) else X0
        if X0 is not None and _is_torch(first):
            import torch
            Xs, _ = _instances(X0, "X0")
            for t in Xs:
                if not (_is_torch(t) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (N, N) and t.is_contiguous()):
                    raise MGError(f"X0: expected contiguous float64 CUDA tensors of shape ({N}, {N})")
            if len(Xs) != k:
                raise MGError(f"X0: {len(Xs)} vectors for k = {k}")
            dev = Xs[0].device
            ptrs, buf = _staged(Xs, False, N * N, dev)
            prev = _lib.mg_get_stream()
            _lib.mg_set_stream(torch.cuda.current_stream(dev).cuda_stream)
            try:
                lam, info = self.solve_ptrs(ptrs, True, seed)
            finally:
                _lib.mg_set_stream(prev)
            if buf is not None:
                for i in range(k):
                    Xs[i].copy_(buf[i, :N * N].view(N, N))
            return lam, X0, info
        if X0 is None:
            Xd = [DeviceGrid.zeros((N, N)) for _ in range(k)]
            owned, host = list(Xd), True
        else:
            Xs = list(X0) if isinstance(X0, (list, tuple)) else [x for x in np.asarray(X0, dtype=np.float64)]
            if len(Xs) != k:
                raise MGError(f"X0: {len(Xs)} vectors for k = {k}")
            host = not all(isinstance(x, DeviceGrid) for x in Xs)
            Xd, owned = [], []
            for x in Xs:
                if isinstance(x, DeviceGrid):
                    if x.shape != (N, N):
                        raise MGError(f"X0: DeviceGrid of shape {x.shape}, expected ({N}, {N})")
                    Xd.append(x)
                else:
                    x = np.asarray(x, dtype=np.float64)
                    if x.shape != (N, N):
                        raise MGError(f"X0: array of shape {x.shape}, expected ({N}, {N})")
                    Xd.append(DeviceGrid.from_host(x))
                    owned.append(Xd[-1])
        try:
            lam, info = self.solve_ptrs([x.ptr for x in Xd], X0 is not None, seed)
            X = np.stack([x.to_host() for x in Xd]) if host else Xd
        finally:
            for x in owned:
                x.free()
        return lam, X, info

    def history(self):
        """the records of the last solve, one dict per Rayleigh-Ritz step: theta (k), res (k, the rotation's), kept (basis
        directions kept), restarted"""
        fn = _need_eigs("mg_eigs_history")
        n = fn(self._e, None, 0)
        if n <= 0:
            return []
        k = self.k
        buf = np.zeros((n, 2 * k + 2))
        got = fn(self._e, buf.ctypes.data, n)
        return [dict(theta=rec[:k].copy(), res=rec[k:2 * k].copy(), kept=int(rec[2 * k]), restarted=bool(rec[2 * k + 1]))
                for rec in buf[:got]]

    def close(self):
        if getattr(self, "_e", None):
            _lib.mg_eigs_destroy(self._e)
            self._e = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def eigs(N, k, L=1.0, coef=None, **opts):
    """The k lowest eigenmodes of -div(coef grad u) (coef = None: the Laplacian) on the N x N grid of side L with a zero rim:
    (lam, X, info) of one EigenSolver.solve() from a random start; opts are EigenSolver's."""
    seed = opts.pop("seed", 0)
    with EigenSolver(N, L, k=k, coef=coef, **opts) as e:
        return e.solve(seed=seed)


def _need_heat(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name} (a build without the heat stepper)")


def _need_heat_vc(name):
    if not hasattr(lib(), name):
        raise MGError(f"{LIB_PATH} does not export {name} (a build without the heat stepper's variable coefficient)")
    return getattr(_lib, name)


def heat_opts(nu=1.0, dt=1.0, theta=1.0, **opts):
    """mg_heat_opts: the scheme's nu, dt, theta and the solve options of every step (solve_opts; shift must stay 0, the
    stepper sets it to sigma = 1/(theta*nu*dt))."""
    _need_heat("mg_heat_opts_default")
    o = HeatOpts()
    lib().mg_heat_opts_default(C.byref(o))
    o.nu, o.dt, o.theta = float(nu), float(dt), float(theta)
    o.solve = solve_opts(**opts)
    return o


def heat_rhs(N, L, nu, dt, theta, U, Q=None, F=None):
    """mg_heat_rhs on DeviceGrids: F = -(sigma*U) - ((1 - theta)/theta)*Laplace_h(U) - Q/(theta*nu) on the interior,
    sigma = 1/(theta*nu*dt), +0 on the rim -- the right-hand side of one theta-scheme step of u_t = nu*Laplace(u) + q as the
    screened equation Laplace(u+) - sigma*u+ = F (include/mg_heat.h fixes the evaluation order; theta = 1 reads no
    neighbour).  Q = None: no source.  F = None: a new DeviceGrid.  U and Q are read only; returns F."""
    _need_heat("mg_heat_rhs")
    if F is None:
        F = DeviceGrid((N, N))
    _lib.mg_heat_rhs(int(N), float(L), float(nu), float(dt), float(theta), U.ptr, Q.ptr if Q is not None else None, F.ptr)
    _check()
    return F


def heat_rhs_coef(N, L, nu, dt, theta, a, U, Q=None, F=None):
    """mg_heat_rhs_coef on DeviceGrids: the right-hand side of one theta-scheme step of u_t = nu*div(a grad u) + q as the
    equation div(a grad u+) - sigma*u+ = F of Solver(shift=sigma, coef=a): F = -(sigma*U) - ((1 - theta)/theta)*A_h(U)
    - Q/(theta*nu) on the interior, A_h the operator of applyOperator at shift 0, +0 on the rim (include/mg_heat_vc.h fixes the
    evaluation order).  a = None is a = 1, exactly heat_rhs; a == 1 everywhere gives heat_rhs's bits; theta = 1 reads neither a
    neighbour nor a.  a is not checked for sign or finiteness.  Q = None: no source.  F = None: a new DeviceGrid.  a, U and Q
    are read only; returns F."""
    fn = _need_heat_vc("mg_heat_rhs_coef")
    if F is None:
        F = DeviceGrid((N, N))
    fn(int(N), float(L), float(nu), float(dt), float(theta), a.ptr if a is not None else None, U.ptr,
       Q.ptr if Q is not None else None, F.ptr)
    _check()
    return F


def heat_rhs_boundary(N, L, nu, dt, theta, bc, a, U, Q=None, F=None):
    """mg_heat_rhs_boundary on DeviceGrids: heat_rhs_coef evaluated at every unknown of the boundary kinds bc (S, N, W, E: row
    0, row N-1, column 0, column N-1) with mirrored neighbours beyond Neumann sides, +0 at data points (include/mg_bc.h);
    theta = 1 reads no neighbour and no coefficient.  a = None is a = 1.  Q = None: no source.  F = None: a new DeviceGrid.  On
    Neumann sides the rim of U is part of the field.  Returns F."""
    fn = _need_bc("mg_heat_rhs_boundary")
    if F is None:
        F = DeviceGrid((N, N))
    fn(int(N), float(L), float(nu), float(dt), float(theta), _kinds(bc), _opt(a), U.ptr, _opt(Q), F.ptr)
    _check()
    return F


class HeatStepper:
    """Time stepper of include/mg_heat.h: the theta-scheme (theta = 1 backward Euler, 0.5 Crank-Nicolson) for
    u_t = nu*Laplace(u) + q on the N x N grid of the solvers, Dirichlet values on the rim of U.  One step is one launch of
    the right-hand-side kernel (heat_rhs) over all instances and one solve of Laplace(u+) - sigma*u+ = F with
    sigma = 1/(theta*nu*dt) (the attribute .sigma), started from U itself -- u_old is the warm start.  k steps equal, bit for
    bit, k times {heat_rhs, Solver(shift=sigma).solve} on each instance.  max_batch = 1 steps through a Solver (fmg=n works
    as there), max_batch > 1 through a BatchSolver (which refuses fmg != 0).  The solve options are solve_opts's; shift is
    the stepper's own and is refused here.  Everything is allocated at creation; step() allocates nothing on the device.
    set_coefficient(a) (include/mg_heat_vc.h) steps u_t = nu*div(a grad u) + q instead, a > 0 given at the grid points: the
    solve of every step is Solver(shift=sigma, coef=a)'s and, for theta < 1, the right-hand side is heat_rhs_coef's; k steps
    equal, bit for bit, k times {heat_rhs_coef, Solver(shift=sigma, coef=a).solve}.  a == 1 everywhere is the stepper without
    a coefficient bit for bit, and with theta = 1 the right-hand side reads no coefficient at all (it stays heat_rhs).  Refused
    with [3]: a stepper with max_batch > 1 (the batched stepper passes none to its BatchSolver) and one created with fmg != 0."""

    def __init__(self, N, L=1.0, nu=1.0, dt=1.0, theta=1.0, max_batch=1, **opts):
        self.N, self.L, self.max_batch = int(N), float(L), int(max_batch)
        self.opts = heat_opts(nu, dt, theta, **opts)
        _need_heat("mg_heat_stepper_create")
        self._s = lib().mg_heat_stepper_create(self.N, self.L, self.max_batch, C.byref(self.opts))
        if not self._s:
            _check()
            raise MGError("mg_heat_stepper_create returned NULL")
        self.sigma = _lib.mg_heat_stepper_sigma(self._s)

    def set_coefficient(self, a):
        """The equation becomes u_t = nu*div(a grad u) + q.  a: what Solver.set_coefficient accepts -- N x N values at the
        grid points, rim included, finite and > 0, as a numpy array, a DeviceGrid or a float64 torch CUDA tensor (read on
        torch.cuda.current_stream()); None: back to the constant stepper, which enqueues what it always did.  The inner Solver
        checks, copies and coarsens a (the stepper keeps no second copy; a may be freed after the call).  a == 1 everywhere
        is the stepper without a coefficient, bit for bit; with theta = 1 only the solve sees a, the right-hand side stays
        heat_rhs.  Refused (MGError, the stepper stays as it was and usable): [2] a value that is not finite or not > 0, a
        wrong shape or alignment; [3] a stepper with max_batch > 1 (batch), or created with fmg != 0 (fmg)."""
        _set_coefficient(_need_heat_vc("mg_heat_stepper_set_coefficient"), self._s, self.N, a)

    @property
    def has_coefficient(self):
        """True while a coefficient is set (set_coefficient)."""
        return bool(_need_heat_vc("mg_heat_stepper_has_coefficient")(self._s))

    def set_boundary(self, bc):
        """bc: the four kinds of the walls in the order S, N, W, E (row 0, row N-1, column 0, column N-1), as
        Solver.set_boundary takes them; None or four Dirichlet sides: the stepper as it was.  Neumann walls are insulated
        (du/dn = 0); a constant wall flux enters through the source, Q_eff = Q + nu*(2/h)*a*g at the wall points
        (include/mg_bc.h).  On Neumann sides the rim of U is part of the field and is written by every step.  k steps equal,
        bit for bit, k times {heat_rhs_boundary, Solver(shift=sigma, bc=bc, coef=a).solve}.  Refused (MGError, the stepper
        stays as it was): what Solver.set_boundary refuses, and "[3]" a stepper with max_batch > 1."""
        kinds = _kinds(bc)
        status = _need_bc("mg_heat_stepper_set_boundary")(self._s, kinds)
        if status:
            _check()
            raise MGError(f"mg_heat_stepper_set_boundary failed with status {status}")
        self._bc = tuple(int(v) for v in kinds)

    @property
    def boundary(self):
        """the four kinds (S, N, W, E) as a tuple of DIRICHLET / NEUMANN"""
        return getattr(self, "_bc", (0, 0, 0, 0))

    def step_ptrs(self, U_ptrs, Q_ptrs=None, steps=1):
        """U_ptrs: device addresses of N x N fp64 arrays (16-byte aligned, stepped in place); Q_ptrs: None, or as many
        addresses (None entries: no source for that instance; addresses may repeat); on the engine stream.  Returns one
        info dict per instance: status (0 converged, -1 not), converged, steps (done), cycles (summed), cycles_per_step,
        coarse_capped, res and ref_norm of the last solve, device_ms of the call."""
        n = len(U_ptrs)
        if Q_ptrs is not None and len(Q_ptrs) != n:
            raise MGError(f"{len(Q_ptrs)} Q pointers for {n} U pointers")
        Ua = (C.c_void_p * max(n, 1))(*U_ptrs)
        Qa = (C.c_void_p * max(n, 1))(*Q_ptrs) if Q_ptrs is not None else None
        res = (HeatResult * max(n, 1))()
        status = _lib.mg_heat_stepper_step(self._s, n, Ua, Qa, int(steps), res)
        if status > 0:
            _check()
            raise MGError(f"mg_heat_stepper_step failed with status {status}")
        return [dict(status=r.status, converged=r.status == MG_SOLVE_CONVERGED, steps=r.steps, cycles=r.cycles,
                     cycles_per_step=[r.cycles_per_step[i] for i in range(r.n_steps)], coarse_capped=bool(r.coarse_capped),
                     res=r.res, ref_norm=r.ref_norm, device_ms=r.device_ms) for r in res[:n]]

    def step(self, U, Q=None, steps=1):
        """Advance U by `steps` time steps.  U: what Solver.solve / BatchSolver.solve accept -- a numpy array, a DeviceGrid
        or a float64 torch CUDA tensor (worked on in place, on torch.cuda.current_stream()), (N, N) or [B, N, N], or a list of
        B (N, N) ones.  Q (the source q, constant over the call; None: none): the same, or one (N, N) array shared by every
        instance (no copy).  Returns (U, infos) with one info dict per instance (step_ptrs); numpy input comes back as a new
        numpy array of U's shape.  Torch instances that are not 16-byte aligned -- every odd instance of a contiguous
        [B, N, N] tensor with N odd -- go through a staging buffer whose instance pitch is N*N + 1 doubles (copied in and
        back on the same stream).
        A time-dependent rim: writing the new rim into U before each steps=1 call is exact only for theta = 1, whose
        right-hand side reads no neighbour.  For theta < 1 run heat_rhs on the old field with its old rim, then set the new
        rim, then solve with Solver(shift=self.sigma) (include/mg_heat.h, mg_heat_stepper_step)."""
        first = lambda X: X[0] if isinstance(X, (list, tuple)) else X
        if _is_torch(first(U)) or (Q is not None and _is_torch(first(Q))):
            return self._step_torch(U, Q, steps)
        return self._step_host(U, Q, steps)

    def _step_torch(self, U, Q, steps):
        import torch
        N = self.N
        Us, _ = _instances(U, "U")
        Qs, shared = _instances(Q, "Q") if Q is not None else (None, False)
        if Qs is not None:
            if shared:
                Qs = Qs * len(Us)
            if len(Qs) != len(Us):
                raise MGError(f"{len(Qs)} Q instances for {len(Us)} U instances")
        for name, ts in (("U", Us), ("Q", Qs or [])):
            for t in ts:
                if not (_is_torch(t) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (N, N)
                        and t.is_contiguous()):
                    raise MGError(f"{name}: expected contiguous float64 CUDA tensors of shape ({N}, {N})")
        dev = Us[0].device
        stream = torch.cuda.current_stream(dev)
        nn = N * N
        Q_ptrs, Qbuf = _staged(Qs, shared, nn, dev) if Qs is not None else (None, None)
        U_ptrs, Ubuf = _staged(Us, False, nn, dev)
        prev = _lib.mg_get_stream()
        _lib.mg_set_stream(stream.cuda_stream)
        try:
            infos = self.step_ptrs(U_ptrs, Q_ptrs, steps)
        finally:
            _lib.mg_set_stream(prev)
        if Ubuf is not None:
            for i, u in enumerate(Us):
                u.copy_(Ubuf[i, :nn].view(N, N))
        del Qbuf
        return U, infos

    def _step_host(self, U, Q, steps):
        N = self.N
        keep = []

        def dev(a, what):
            if isinstance(a, DeviceGrid):
                if a.shape != (N, N):
                    raise MGError(f"{what}: DeviceGrid of shape {a.shape}, expected ({N}, {N})")
                return a
            a = np.asarray(a, dtype=np.float64)
            if a.shape != (N, N):
                raise MGError(f"{what}: array of shape {a.shape}, expected ({N}, {N})")
            g = DeviceGrid.from_host(a)
            keep.append(g)
            return g

        def split(X, what):
            if isinstance(X, DeviceGrid):
                return [X], True
            return _instances(X if isinstance(X, (list, tuple)) else np.asarray(X), what)

        Us, single = split(U, "U")
        host_U = not all(isinstance(u, DeviceGrid) for u in Us)
        Ud = [dev(u, "U") for u in Us]
        Q_ptrs = None
        if Q is not None:
            Qs, shared = split(Q, "Q")
            Qd = [dev(q, "Q") for q in Qs]
            if shared:
                Qd = Qd * len(Ud)
            if len(Qd) != len(Ud):
                raise MGError(f"{len(Qd)} Q instances for {len(Ud)} U instances")
            Q_ptrs = [q.ptr for q in Qd]
        infos = self.step_ptrs([u.ptr for u in Ud], Q_ptrs, steps)
        if host_U:
            out = [u.to_host() for u in Ud]
            return (out[0] if single else np.stack(out)), infos
        return U, infos

    def close(self):
        if getattr(self, "_s", None) and _initialised:
            _lib.mg_heat_stepper_destroy(self._s)
        self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
