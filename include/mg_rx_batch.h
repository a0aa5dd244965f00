/*
 * mg_rx_batch.h -- the batched residual-tolerance solver (mg_hip.h: mg_batch_solver_*) with a variable reaction term:
 *     div(a_i grad U_i) - (sigma + s_i)*U_i = F_i     for the instances i of one mg_batch_solver_solve call,
 * every s_i an N x N fp64 device array given AT THE GRID POINTS, rim included, every value finite and >= 0; sigma =
 * mg_solve_opts.shift, one value for the batch; a_i as in mg_varcoef_batch.h, or absent (a = 1).  Either every instance has a
 * reaction term of its own, or all share one -- independently of how the coefficients are held: a shared a with per-instance
 * s, per-instance a with a shared s, and so on.  mg_hip.h includes this file; libmgpoisson.so exports every symbol below.  This
 * header is the specification of the batched form; the operator, the cycle and the coarsening of s are the ones of
 * mg_reaction.h, which it does not restate.
 *
 * The contract is mg_varcoef_batch.h's, bit identity with the single solver: with reactions set, instance i of
 * mg_batch_solver_solve gives the same U, cycles, status, converged, coarse_capped, res0, res, ref_norm and history, bit for
 * bit, as mg_solver_solve on F_dev[i], U_dev[i] of a solver with the same options after mg_solver_set_reaction(s_i) (and, if
 * a coefficient is set, mg_solver_set_coefficient(a_i)) -- whatever the other instances and their terms are, wherever the
 * instance sits in the batch, and whether its s is its own copy or the shared one.  Consequently, on U, history, cycles and
 * flags, with and without coefficients:
 *   s_i == 0.0 everywhere     the batch solver without a reaction
 *   s_i == c, shift == 0      the batch solver created with shift = c and no reaction
 * With no reaction set the batch solver enqueues exactly what it enqueued before it knew of one: kernels, grids, table
 * uploads and their byte counts.
 *
 * How: one cycle is the operator-by-operator cycle of mg_varcoef_batch.h -- the same recorded steps, node order and ping-pong
 * -- and each of its launches runs ONCE over all active instances through the batched forms of mg_reaction.h's kernels
 * (csrc/mg_reaction_batch_kernels.hip, compiled from the bodies of csrc/mg_reaction_impl.h that the single kernels are compiled
 * from).  A block takes its instance from blockIdx as in mg_varcoef_batch.h and that instance's arrays from the table of the
 * step; the level's s travels in a table entry that those launches leave unused, so the number of tables and the bytes of an
 * upload are what they are with a coefficient.  Within one launch either every instance has a coefficient or none has;
 * without one no array of ones is read.  Launches per cycle,
 *     (nl - 1)*(pre + post + 3) + 1, plus one copy when pre + post is even, and 2 for the norm
 * -- independent of the number of instances.  With a reaction set the cycle runs this way whatever mg_set_smoother says, with
 * or without a coefficient, as mg_solver_solve does.  The stopping norm is the reaction operator's; the reference norm
 * ||F_i|| has no operator in it and stays the constant solver's launch.  Active-set handling, per-instance tolerances,
 * results, history and statistics are those of mg_batch_solver_solve without a reaction.
 *
 * The Krylov acceleration (mg_krylov_batch.h) is supported with a reaction: the first residual, the recomputed residual and
 * A*z go through the reaction kernels, and every instance is bit-identical -- U, history, the breakdown flag and the log -- to
 * the single solver with mg_solver_set_krylov(m), mg_solver_set_reaction(s_i) and its coefficient alone.
 * mg_batch_solver_set_coefficient, mg_batch_solver_set_reaction and mg_batch_solver_set_krylov work in any order.
 *
 * Refused: mg_batch_solver_adjoint while a reaction is set (MG_ERR_UNSUPPORTED, the solver unchanged, as mg_solver_adjoint).
 * The batched Newton solve (mg_newton_batch.h) installs the Newton matrices' terms through this operator for the length of its
 * call.  Not built: a reaction in the heat stepper or the eigensolver, whose private batch
 * solvers never set one and whose launches do not change; the adjoint.
 *
 * Memory contract (mg_hip.h): mg_batch_solver_set_reaction reads the s_dev[i] and writes only storage the solver owns; a solve
 * reads F, U and solver storage and writes the U of instances that are still active -- an instance that met its tolerance is
 * never written again (tests/test_solve_reaction_batched_gpu.py holds every array inside guard bands).  Device arrays are
 * 16-byte aligned.
 */
#ifndef MG_RX_BATCH_H
#define MG_RX_BATCH_H

#ifdef __cplusplus
extern "C" {
#endif

/* Give the batch solver its reaction terms, or take them away again.  Mirrors mg_batch_solver_set_coefficient.
 *   n == 1               s_dev[0] is shared by every instance of every later solve (ONE copy is stored)
 *   1 < n <= max_batch   instance i of a later solve uses s_dev[i]; such a solve takes at most n instances
 *                        (mg_batch_solver_solve refuses more with MG_ERR_ARG before anything is enqueued)
 *   n == 0, s_dev NULL   the solver without a reaction again
 * s_dev: host array of n device pointers to N x N arrays, each 16-byte aligned; two of them may be equal.  The arrays are
 * checked on the device (every value finite and >= 0: one launch over the n arrays, one flag per instance, one read-back),
 * copied into level-0 storage of the solver's own (one launch) and coarsened to every level with mg_coarsenCoefficient's rule
 * (one launch per level); they are not kept and may be freed after the call.  Works on the engine stream (mg_set_stream) and
 * returns when the terms are in place.  The level storage (about 4/3 N^2 doubles per stored term, at the solver's instance
 * pitch) is allocated by the first call and reused by later ones; it grows when a later call brings more terms.  The count
 * is independent of the coefficient's: each count > 1 bounds the size of a solve on its own.
 * Returns 0, or (mg_last_error; the solver keeps the state it had, reaction included, and stays usable):
 *   MG_ERR_ARG (2)   NULL solver; n outside [0, max_batch]; n > 0 with a NULL array or a NULL entry, n == 0 with an array;
 *                    an s_dev[i] that is not 16-byte aligned; a value that is not finite or not >= 0 (the message names the
 *                    first such instance: "instance <i>")
 * A HIP error (1) before the check has passed leaves the state as it was too; one after it, while the level storage is
 * being rewritten, leaves the solver WITHOUT a reaction (mg_batch_solver_has_reaction: 0). */
int  mg_batch_solver_set_reaction(mg_batch_solver *s, int n, const double *const *s_dev);
/* 0 when no reaction is set (NULL: 0), else the n it was set with (1: shared) */
int  mg_batch_solver_has_reaction(const mg_batch_solver *s);

#ifdef __cplusplus
}
#endif
#endif /* MG_RX_BATCH_H */
