/*
 * mg_varcoef_batch.h -- the batched residual-tolerance solver (mg_hip.h: mg_batch_solver_*) with a variable coefficient:
 *     div(a_i grad U_i) - sigma*U_i = F_i     for the instances i of one mg_batch_solver_solve call,
 * every a_i an N x N fp64 device array given AT THE GRID POINTS, rim included, every value finite and > 0; sigma =
 * mg_solve_opts.shift, one value for the batch.  Either every instance has a coefficient of its own, or all share one.
 * mg_hip.h includes this file; libmgpoisson.so exports every symbol below.  This header is the specification of the batched
 * form; the operator, the cycle and the coarsening of a are the ones of mg_varcoef.h, which it does not restate.
 *
 * The contract is bit identity with the single solver: with coefficients set, instance i of mg_batch_solver_solve gives the
 * same U, cycles, status, converged, coarse_capped, res0, res, ref_norm and history, bit for bit, as mg_solver_solve on
 * F_dev[i], U_dev[i] of a solver with the same options after mg_solver_set_coefficient(a_i) -- whatever the other instances
 * and their coefficients are, wherever the instance sits in the batch, and whether its coefficient is its own copy or the
 * shared one.  Consequently a_i == 1.0 everywhere gives the bits of the batch solver without a coefficient (mg_varcoef.h).
 *
 * How: one cycle is the variable-coefficient cycle of mg_varcoef.h -- operator by operator, the same node order and the same
 * ping-pong between the two fields of a level -- and each of its launches runs ONCE over all active instances.  A block
 * takes its instance from blockIdx (z for the sweeps, the residual, the norm's first stage and the coarsening, whose single
 * grids are (column blocks, row blocks); x for the one-workgroup coarse solve and the norm's second stage) and that
 * instance's arrays from a table in device memory; inside the instance it runs the code, the block partition and the
 * summation order of the single launch (both are compiled from one set of bodies, csrc/mg_varcoef_impl.h).  The transfer
 * operators of U and D have no coefficient in them and are the batched solver's own.  Launches per cycle,
 *     (nl - 1)*(pre + post + 3) + 1, plus one copy when pre + post is even (the result then ends in the solver's field),
 * and 2 for the norm -- independent of the number of instances.  With a coefficient set the cycle runs this way whatever
 * mg_set_smoother says, as mg_solver_solve does.  The stopping norm is the variable operator's; the reference norm ||F_i||
 * has no operator in it and stays the constant solver's launch.  Active-set handling, per-instance tolerances, results,
 * history and statistics are those of mg_batch_solver_solve without a coefficient.
 *
 * Memory contract (mg_hip.h): mg_batch_solver_set_coefficient reads the a_dev[i] and writes only storage the solver owns;
 * a solve reads F, U and solver storage and writes the U of instances that are still active, exactly as without a
 * coefficient -- an instance that met its tolerance is never written again (tests/test_solve_vc_batched_gpu.py holds every
 * array inside guard bands).  Device arrays are 16-byte aligned.
 */
#ifndef MG_VARCOEF_BATCH_H
#define MG_VARCOEF_BATCH_H

#ifdef __cplusplus
extern "C" {
#endif

/* Give the batch solver its coefficients, or take them away again.
 *   n == 1               a_dev[0] is shared by every instance of every later solve (ONE copy is stored)
 *   1 < n <= max_batch   instance i of a later solve uses a_dev[i]; such a solve takes at most n instances
 *                        (mg_batch_solver_solve refuses more with MG_ERR_ARG before anything is enqueued)
 *   n == 0, a_dev NULL   back to the constant-coefficient solver, which then enqueues exactly what it always enqueued
 * a_dev: host array of n device pointers to N x N arrays, each 16-byte aligned; two of them may be equal.  The arrays are
 * checked on the device (every value finite and > 0: one launch over the n arrays, one flag per instance, one read-back),
 * copied into level-0 storage of the solver's own (one launch) and coarsened to every level (one launch per level); they are
 * not kept and may be freed after the call.  Works on the engine stream (mg_set_stream) and returns when the coefficients
 * are in place.  The level storage (about 4/3 N^2 doubles per stored coefficient, at the solver's instance pitch) is
 * allocated by the first call and reused by later ones; it grows when a later call brings more coefficients.
 * Returns 0, or (mg_last_error; the solver keeps the state it had, coefficients included, and stays usable):
 *   MG_ERR_ARG (2)   NULL solver; n outside [0, max_batch]; n > 0 with a NULL array or a NULL entry, n == 0 with an array;
 *                    an a_dev[i] that is not 16-byte aligned; a value that is not finite or not > 0 (the message names the
 *                    first such instance: "instance <i>")
 * A HIP error (1) before the check has passed leaves the state as it was too; one after it, while the level storage is
 * being rewritten, leaves the solver WITHOUT a coefficient (mg_batch_solver_has_coefficient: 0). */
int  mg_batch_solver_set_coefficient(mg_batch_solver *s, int n, const double *const *a_dev);
/* 0 when no coefficient is set (NULL: 0), else the n it was set with (1: shared) */
int  mg_batch_solver_has_coefficient(const mg_batch_solver *s);

#ifdef __cplusplus
}
#endif
#endif /* MG_VARCOEF_BATCH_H */
