/*
 * mg_newton_batch.h -- the semilinear problem on the batched residual-tolerance solver (mg_hip.h: mg_batch_solver_*):
 *     div(a_i grad U_i) - sigma*U_i - kappa_i*w_i*g(U_i) = F_i     for the instances i of one mg_batch_solver_newton call,
 * Newton's method with a backtracking line search around the batched reaction solve (mg_rx_batch.h), all instances in lockstep.
 * The kind of g, the Newton options and sigma = mg_solve_opts.shift are one per call; kappa is per instance (a HOST array);
 * w is absent (w = 1), one array shared by all, or one per instance; a is what mg_batch_solver_set_coefficient has set -- none,
 * one shared, or one per instance -- and GCR(m) runs in the inner solves when mg_batch_solver_set_krylov is on.  mg_hip.h
 * includes this file; libmgpoisson.so exports every symbol below.  This header is the specification of the batched form; the
 * pass (its expressions and their order, the kinds, exp_libm) and the driver (its steps, the acceptance test, what a record
 * holds) are mg_newton.h's, which it does not restate.
 *
 * THE CONTRACT is bit identity with the single driver.  For instance i the call gives the same U, the same mg_newton_result
 * (status, iterations, converged, n_history, res0, res, inner_cycles, trials), the same mg_newton_iter records and the same
 * inner history (and, under GCR, Krylov log) of its last inner solve, bit for bit, as mg_solver_newton on F_dev[i], U_dev[i],
 * kappa[i], w_i of an mg_solver with the same options after mg_solver_set_coefficient(a_i) and mg_solver_set_krylov(m) --
 * whatever the other instances are, wherever the instance sits in the batch, and whether its w or a is its own copy or the
 * shared one.  An instance that has converged, stalled or reached max_iters leaves the batch: nothing of it is read or written
 * by a later launch, and its U is never written again but by the copy home below.  An instance whose start meets the tolerance
 * takes 0 iterations and its U is untouched.
 *
 * THE PASS (mg_nonlinearResidual_batch; csrc/mg_newton_batch_kernels.hip): k_newton_residual of mg_newton.h for n instances in
 * ONE launch, compiled from the bodies the single kernel is compiled from.  blockIdx.z picks the instance, whose arrays and
 * kappa come from a table item of its own in device memory; grid x, y, the form (one column per lane; column pairs from the
 * pair threshold; non-temporal from the non-temporal threshold) and the summation order are the single launch's of the same N.
 * A second launch, one block per instance, finishes the n norms.  Within one launch every instance has a coefficient, a
 * weight, a step -- or none has; t is one value per launch.
 *
 * THE DRIVER (mg_batch_solver_newton) runs the iterations of mg_newton.h for all instances in lockstep:
 *   1. one no-step pass over all n: D_i, S_i, r0_i, the n norms read back in one copy.  A non-finite r0_i refuses the whole
 *      call (MG_ERR_ARG, the message names the first such instance: "instance <i>"); every U is untouched, the no-step pass
 *      writes none.  Instance i has converged when r_i <= max(atol, rtol*r0_i).
 *   2. while some instance is neither converged, stalled nor at max_iters -- over THOSE instances only:
 *        the levels of their S below level 0 are coarsened (k::coef_coarsen_batch: one launch per level);
 *        their delta are zeroed (ONE memset: the delta of all instances are one compact region);
 *        the batch solver's own solve loop runs on (D_i, delta_i) with the reaction operator of mg_rx_batch.h and GCR(m) if on:
 *        its create-time rtol / atol / max_cycles govern, it drops instances as they meet the inner tolerance, and an inner
 *        solve that ends unconverged is not an error;
 *        the line search runs in rounds: round k is ONE step-pass launch at t = 2^-k over the instances of this iteration that
 *        have not accepted yet, then one read-back of their norms.  An instance accepts when r' is finite and
 *        r' < (1 - 1e-4*t)*r, the single driver's expression; the rejection after max_backtracks earlier ones marks it stalled
 *        (its record is the extra one, t = 0, and its U stays the last accepted iterate).
 *   3. an accepted trial becomes the next iteration's (U, D, S) by swapping that instance's pointers between its two sets of
 *      (V, D, S); no field is copied.  When the loop has ended, ONE launch copies home to U_dev[i] every instance whose accepted
 *      iterate sits in solver storage (the single driver's home()).
 * Launches per Newton iteration, (levels - 1) + the inner solve's + 2 per line-search round, and every other piece of enqueued
 * work do not depend on the number of instances.  stats->launches counts kernels (the pass counts 2), not copies or memsets.
 *
 * During the call the solver holds a per-instance reaction of the driver's own, the level-0 term of instance i being whichever
 * of its two S sets holds the accepted iterate's.  On every return, errors included, mg_batch_solver_has_reaction is 0 again,
 * as before the call, and mg_batch_solver_solve enqueues what it enqueued before.
 *
 * Memory.  The FIRST call allocates, for max_batch instances at the level-0 instance pitch P (N^2 rounded up to 32 doubles):
 *     5*P*max_batch doubles                       V, D, D', S', delta -- the second set of S among them
 *     sum over the levels l of P_l*max_batch      the reaction's level storage, about (4/3)*P*max_batch doubles, only when the
 *                                                 solver holds none for max_batch instances yet (mg_batch_solver_set_reaction)
 *     max_batch*(40*(levels - 1) + 80) bytes      the tables and the norms, once in device and once in pinned host memory
 *     max_batch*4 bytes, device and pinned        the flags of the check, if no setter has allocated them
 * -- in bytes about (5 + 4/3)*8*P*max_batch, 50.7*N^2*max_batch.  Later calls allocate nothing.  A call reads F, w, U and
 * solver storage and writes U and solver storage only; device arrays are 16-byte aligned.
 *
 * Refused (the solver unchanged, every U untouched; mg_last_error):
 *   MG_ERR_UNSUPPORTED (3)  a caller's reaction is set (mg_batch_solver_set_reaction): the driver installs the Newton matrices'
 *   MG_ERR_ARG (2)          n outside [1, max_batch], or beyond a per-instance coefficient count; n_w not in {0, 1, n}; an
 *                           unknown kind; a kappa[i] negative or not finite; a value of a w negative or not finite (one batched
 *                           check launch over the n_w arrays; "instance <i>"); a NULL solver, kappa, F, U or entry, n_w > 0
 *                           with a NULL w_dev; an array that is not 16-byte aligned; two U that overlap, or a U that overlaps
 *                           an F, as mg_batch_solver_solve checks them; options out of range (mg_newton.h); a start whose
 *                           residual is not finite
 * The private batch solvers of the heat stepper and the eigensolver never call this; their launches do not change.
 * Not built: a kind or options per instance, boundary kinds, fmg, the adjoint of a semilinear solve, a semilinear heat
 * stepper, a user-supplied g.  (The adjoint is built since, beside this header: mg_adjoint_rx.h,
 * mg_batch_solver_newton_adjoint.)
 */
#ifndef MG_NEWTON_BATCH_H
#define MG_NEWTON_BATCH_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_batch_newton_stats {
    int iterations;     /* the most accepted Newton steps of any instance */
    int trial_rounds;   /* step-pass launches over the batch, all iterations together */
    int inner_cycles;   /* sum over the inner batch solves of their stats.cycles */
    int launches;       /* kernel launches the call enqueued, inner solves included */
    double device_ms;
} mg_batch_newton_stats;

/* The driver above on the engine stream.  kappa: a HOST array of n values.  n_w == 0 (w_dev NULL): w = 1; n_w == 1: w_dev[0]
 * is shared by every instance; n_w == n: instance i uses w_dev[i].  opts == NULL: mg_newton_opts_default; one set for the
 * batch.  out: n results, may be NULL; stats may be NULL.  Returns MG_NEWTON_CONVERGED when every instance converged,
 * MG_NEWTON_NOT_CONVERGED when at least one did not (out[i].status then tells _NOT_CONVERGED from _STALLED per instance), or
 * an error code > 0, which every out[i].status then holds too. */
int mg_batch_solver_newton(mg_batch_solver *s, int n, int kind, const double *kappa, int n_w, const double *const *w_dev,
                           const double *const *F_dev, double *const *U_dev, const mg_newton_opts *opts, mg_newton_result *out,
                           mg_batch_newton_stats *stats);
/* the records of instance i of the last mg_batch_solver_newton, oldest first: copies min(cap, n) of them into out (may be
 * NULL) and returns n (0 for an i outside that call) */
int mg_batch_solver_newton_history(const mg_batch_solver *s, int i, mg_newton_iter *out, int cap);
/* the residual history r_0 .. r_cycles of instance i's LAST inner solve of that call, copied like the records above (none for
 * an instance that took no iteration) */
int mg_batch_solver_newton_inner_history(const mg_batch_solver *s, int i, double *out, int cap);

/* THE PASS alone over n instances, the building block and test hook (synchronous, engine stream; N >= 3, spacing L/(N-1)), as
 * mg_nonlinearResidual.  n_a == 0 (a_dev NULL): a = 1; 1: a_dev[0] is shared; n: one per instance -- n_w, w_dev alike.
 * kappa: a HOST array of n.  dlt == NULL selects the no-step form, which reads neither t nor V (V may be NULL then); else
 * every dlt[i] and V[i] must be there.  norms: a HOST array of n (may be NULL).  The table and the partial sums live in
 * buffers the call allocates and frees.  Returns 0, MG_ERR_ARG (n < 1 or > 65535, N < 3, L or shift out of range, n_a or n_w
 * not in {0, 1, n}, an unknown kind, a kappa negative or not finite, a NULL or misaligned array) or MG_ERR_HIP; w is not
 * checked here. */
int mg_nonlinearResidual_batch(int n, int N, double L, double shift, int n_a, const double *const *a_dev, int kind, const double *kappa,
                               int n_w, const double *const *w_dev, const double *const *U, const double *const *dlt, double t,
                               const double *const *F, double *const *V, double *const *D, double *const *S, double *norms);

#ifdef __cplusplus
}
#endif
#endif /* MG_NEWTON_BATCH_H */
