/*
 * mg_krylov_batch.h -- Krylov acceleration of the batched residual-tolerance solver (mg_hip.h: mg_batch_solver_*): restarted
 * GCR(m) around the cycle, PER INSTANCE, every launch over all active instances.  mg_hip.h includes this file;
 * libmgpoisson.so exports every symbol below.  This header is the specification of the batched form; the method -- every
 * operation, its order, the breakdown rule, the restart rule, the log record -- is the one of mg_krylov.h, which it does not
 * restate.
 *
 * The contract is bit identity with the single solver: after mg_batch_solver_set_krylov(s, m), instance i of
 * mg_batch_solver_solve gives the same U, cycles, status, converged, coarse_capped, res0, res, ref_norm and history, the
 * same breakdown flag and the same log (k, d_j, g, h, alpha, rho_rec, restarted, rho of every iteration), bit for bit, as
 * mg_solver_solve on F_dev[i], U_dev[i] alone of a solver with the same options after mg_solver_set_krylov(m) and, where
 * the batch has one, mg_solver_set_coefficient(a_i) -- whatever the other instances are, wherever the instance sits in the
 * batch, with a coefficient of its own, a shared one or none, with any shift and any V(pre, post), and under
 * MG_SMOOTHER=simple (where the constant batch solver runs its cycle instance by instance, as it does without the
 * acceleration: only there may the number of launches depend on the number of instances).  m == 0 is the batch solver that
 * never heard of the option: it enqueues the launches it enqueued before, bit for bit and launch for launch.
 *
 * How.  The loop of mg_krylov.h runs for every instance with ITS OWN k, tolerance and restart decisions.  One iteration over
 * the active set (the instances above their tolerance that have neither reached max_cycles nor broken down):
 *     1  z_k = 0               one launch zeroes the whole z_k of every active instance (no memset per instance)
 *     C  z_k = M(r)            the batched cycle with F0 = r_i, U0 = z_{k_i, i}: the launches of a cycle of
 *                              mg_batch_solver_solve (with a coefficient: mg_varcoef_batch.h)
 *     1  q_k = A*z_k           mg_applyOperator's launch, the coefficient nullable per instance
 *     2  d_j, b_j              the dots and their finish -- skipped while every active k is 0
 *     2  q_k, z_k, g, h, ...   the orthogonalisation and its finish (w_k, alpha, the breakdown flag, the record's head)
 *     2  U, r, rho_rec         the update and its finish (the record's tail)
 * then ONE read-back of rho_rec and the breakdown flag of all active slots (with the coarse solves' state).  The host
 * decides per instance: a restart when k_i == m or rho_rec <= tol_i.  The restarting instances get
 *     4  r, rho, the mark      the cycle's signed residual at level 0, the stopping norm (two launches) and restarted = 1,
 *                              rho = the recomputed norm in their records, over the restarting subset through its own table
 * Restarts by k_i + 1 == m are known before the read-back and enqueued in front of it; those the read-back finds
 * (rho_rec <= tol_i) cost a second round of these 4 launches and a second read-back, only when there are any.  An instance
 * that converged on a RECOMPUTED norm, reached max_cycles or broke down leaves the active set and is never written again.
 * Launches of a solve whose active instances all sit at one k in every iteration, C those of one cycle:
 *     4 (the two norms)  +  1 (the residual that starts the loop; none when no instance iterates)
 *       +  sum over the iterations of  C + 6 + (k > 0 ? 2 : 0) + (4 per restart round: k + 1 == m, or rho_rec <= tol)
 * -- independent of the number of instances (mg_batch_solve_stats.launches).  Instances at different k share every launch
 * too: a launch is compiled for the LARGEST k of the active set, each block reads its instance's own k from the table and
 * runs j = 0 .. k-1 in that order, so the count above holds with k the largest one.  `cycles` and `history` are per instance,
 * as mg_solver_solve fills them; mg_batch_solve_stats.cycles is the most iterations any instance ran.
 *
 * A block takes its instance from blockIdx (z for the streaming kernels, y or x for the one-block finish kernels and the
 * zeroing) and that instance's arrays from a table in device memory; inside the instance it runs the code, the grid, the
 * block partition, the per-block partial slots and the fixed summation order of the single launch (both are compiled from
 * one set of bodies, csrc/mg_krylov_impl.h), which is what makes every sum bit-identical.
 *
 * Memory.  The first enabling call allocates, for max_batch instances at the solver's level-0 instance pitch P (N^2 rounded
 * up to 32 doubles): r, 2m slots -- slot j holds z_j (q_j) of every instance, instance i at i*P, indexed by the instance's
 * position in the call and not by its active slot, so compacting the active set moves nothing -- the partials, the scalars
 * (b[16], w[16], alpha, the breakdown flag per instance), a log of max(max_cycles, 1) records per instance and the tables:
 * (2m + 1)*P*max_batch doubles plus small change, beside the solver's own level arrays.  A larger m later allocates the
 * additional slots only.  m == 0 keeps everything for the next enabling call; a solve allocates nothing.
 *
 * Memory contract (mg_hip.h): a solve reads F, U, the coefficients' level storage and solver storage, and writes the U of
 * instances that are still active, interior only -- an instance that met its tolerance at the start, or left the active
 * set, is never written again.  The rim of q_j, z_j, r and U is never written by the Krylov kernels and never read into a
 * result (tests/test_solve_krylov_batched_gpu.py holds F, U and the coefficients inside guard bands).  Device arrays are
 * 16-byte aligned.
 */
#ifndef MG_KRYLOV_BATCH_H
#define MG_KRYLOV_BATCH_H

#ifdef __cplusplus
extern "C" {
#endif

/* Switch the acceleration on (1 <= m <= MG_KRYLOV_MAX_M: GCR(m) per instance) or off (m == 0).  Storage is allocated here
 * (see Memory above) and kept until the solver is destroyed.  Works before or after mg_batch_solver_set_coefficient, with
 * any shift, and under MG_SMOOTHER=simple.
 * Returns 0, or (mg_last_error; the solver keeps the state it had, its m included, and stays usable):
 *   MG_ERR_ARG (2)   NULL solver, or m outside [0, MG_KRYLOV_MAX_M]
 *   MG_ERR_HIP (1)   an allocation failed: what this call had allocated is freed again */
int  mg_batch_solver_set_krylov(mg_batch_solver *s, int m);
/* the current m (0: off; NULL: 0) */
int  mg_batch_solver_krylov(const mg_batch_solver *s);
/* 1 when instance i of the last solve ended on a breakdown (mg_krylov.h), else 0 (NULL, the acceleration off, or i outside
 * the last solve: 0) */
int  mg_batch_solver_krylov_breakdown(const mg_batch_solver *s, int i);
/* TEST HOOK AND DIAGNOSTIC, as mg_solver_krylov_log: the records of instance i of the last accelerated solve, one per
 * iteration of that instance, m + 7 doubles each (m: the value at that solve), written by the device and copied back once at
 * the end of the solve.  out == NULL: returns the number of records; otherwise copies at most cap records and returns how
 * many.  NULL solver, or i outside the last solve: 0. */
int  mg_batch_solver_krylov_log(const mg_batch_solver *s, int i, double *out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* MG_KRYLOV_BATCH_H */
