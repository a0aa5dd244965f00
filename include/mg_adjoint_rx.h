/*
 * mg_adjoint_rx.h -- the adjoint of reaction and semilinear solves of the residual-tolerance solver (mg_reaction.h,
 * mg_newton.h): the gradients of a functional J(U) of a solve of
 *     (R)  div(a grad U) - (sigma + s)*U = F
 *     (N)  div(a grad U) - sigma*U - kappa*w*g(U) = F,      g one of mg_newton.h's three kinds,
 * four Dirichlet sides, in F, the rim data and a as mg_adjoint.h gives them, and in the reaction term s and the shift sigma
 * (R), in the weight w and the strength kappa (N).  mg_hip.h includes this file after mg_newton_batch.h; libmgpoisson.so
 * exports every symbol below.  This header is the specification: tests/_adjoint_rx_ref.py restates the point kernel on
 * numpy, the kernels (csrc/mg_adjoint_rx_kernels.hip, bodies in csrc/mg_adjoint_rx_impl.h) implement it, the drivers are
 * csrc/mg_adjoint_rx.cpp.  inv, b(.) and lam' (lam with its rim values replaced by +0.0) are mg_adjoint.h's.
 *
 * The linearisation of (N) at a converged U is the symmetric reaction operator of (R) with S = kappa*w*g'(U) in the place of
 * s.  Let Ubar = dJ/dU.  The adjoint field lam solves the reaction equation with right-hand side Ubar from the zero field,
 * its reaction term s for (R) and S for (N), at the forward solution U: ONE mg_solver_solve.  Then
 *   dJ/dF          = lam' (interior, 0 on the rim)                       as mg_adjoint.h
 *   dJ/da          = mg_coefficientGradient(lam, U)                      as mg_adjoint.h, the same kernel
 *   dJ/d(rim data) = mg_boundaryGradient(a, lam, Ubar)                   as mg_adjoint.h: no rim value of s, w or g(U)
 *                                                                        enters an interior equation
 *   (R)  gS[p] = lam'[p]*U[p] on the interior, +0.0 on the rim;          dJ/dsigma = gshift = sum over the interior of lam'*U
 *   (N)  gW[p] = kappa*(lam'[p]*g(U[p])) on the interior, +0.0 on the rim;
 *        dJ/dkappa = gkappa = sum over the interior of w[p]*(lam'[p]*g(U[p]))
 *
 * The source gradient, one expression for both cases.  kind: MG_NEWTON_CUBIC, MG_NEWTON_SINH, MG_NEWTON_EXP, or
 * MG_GRAD_LINEAR with g(u) = u.  At an interior point p, every operation rounded once, no fma outside exp_libm:
 *     gv = g(U[p])  by the expressions of mg_newton.h's table;   m = lam[p]*gv;   G[p] = kappa*m;
 *     term = w[p]*m,  or  m  when w == NULL.
 * On the rim G = +0.0 and term = +0.0, g is not evaluated there; the rim of lam is never used.  (R) is kind = MG_GRAD_LINEAR,
 * kappa = 1.0, w = NULL.  sum = the sum of the terms, no square root, in the block partition and the summation order of the
 * semilinear pass's norm for the same N (mg_newton.h): a lane's rows in order, x before y in a column pair, the block sum,
 * the partial of block (bx, by) at by*gx + bx, the finish's order -- deterministic, restated on numpy bit for bit.
 * Forms, with the pass's thresholds: one column per lane for any N; column pairs with 16-byte accesses for even N >= 512;
 * from N >= 4096 non-temporal loads of w and stores of G.  24 B per point, 32 B with w.
 *
 * Not built: gradients through the heat stepper; boundary kinds; fmg with a reaction; a user-supplied g; second
 * derivatives; one fused launch for gA and gW; the sum of the per-instance gradients of an a, s or w that several instances
 * of a batch share (it is the caller's sum).
 *
 * Contract of every function below, as mg_adjoint.h: synchronous, on the engine stream (mg_set_stream); N >= 3; device arrays
 * 16-byte aligned; no output overlaps an input or another output; bad arguments are refused with MG_ERR_ARG (mg_last_error)
 * before anything is enqueued, and without a device with MG_ERR_NOT_INIT and nothing written.  Memory contract (mg_hip.h):
 * each function reads its const arrays and writes its output arrays, every value of them, and nothing else.
 */
#ifndef MG_ADJOINT_RX_H
#define MG_ADJOINT_RX_H

#ifdef __cplusplus
extern "C" {
#endif

#define MG_GRAD_LINEAR 3   /* beside MG_NEWTON_CUBIC = 0, MG_NEWTON_SINH = 1, MG_NEWTON_EXP = 2: g(u) = u */

/* G and sum of the source gradient above.  w == NULL: no weight.  sum: a HOST double, may be NULL (not wanted).  kappa finite.
 * Returns MG_OK or the error code. */
int mg_sourceGradient(int N, int kind, double kappa, const double *w, const double *lam, const double *U, double *G, double *sum);
/* the same on n >= 1 instances in ONE launch (blockIdx.z picks the instance) and one finish launch, instance i bit-identical
 * to the single call on (kappa[i], w, lam[i], U[i]).  kappa: a host array of n values.  n_w: 0 (w == NULL: no weight), 1 (w[0]
 * shared by every instance) or n (w[i]).  lam, U, G: host arrays of n device pointers; sums: a host array of n doubles, may be
 * NULL.  Inputs may repeat between instances; outputs overlap nothing. */
int mg_sourceGradient_batch(int n, int N, int kind, const double *kappa, int n_w, const double *const *w, const double *const *lam,
                            const double *const *U, double *const *G, double *sums);

/* The adjoint of a solve (R) of s in one call: lam is set to zero, mg_solver_solve(s, Ubar, lam, out) runs with whatever the
 * solver has set (reaction, coefficient, shift, Krylov), then gA = mg_coefficientGradient(lam, U) when gA != NULL,
 * gU = mg_boundaryGradient(the solver's level-0 coefficient or NULL, lam, Ubar) when gU != NULL, and (gS, *gshift) =
 * mg_sourceGradient(MG_GRAD_LINEAR, 1.0, NULL, lam, U) when gS != NULL -- bit for bit the result of that sequence made by the
 * caller through the public functions.  Without a reaction set lam, gA and gU are mg_solver_adjoint's bit for bit, and gS is
 * the sensitivity at s == 0.  gshift: a host double, may be NULL; it needs gS.  U is needed for gA and gS.  Returns the
 * solve's status: a solve that does not converge still writes the gradients and returns MG_SOLVE_NOT_CONVERGED; an error
 * code (> 0) otherwise.  Refused with MG_ERR_ARG: NULL s, Ubar or lam; gA or gS without U; gshift without gS; a misaligned
 * array; an output overlapping an input or another output.  MG_ERR_UNSUPPORTED: a boundary with a Neumann side. */
int mg_solver_adjoint_reaction(mg_solver *s, const double *Ubar, const double *U, double *lam, double *gA, double *gU, double *gS,
                               double *gshift, mg_solve_result *out);

/* The adjoint of a semilinear solve (N) of s at its solution U (mg_solver_newton's kind, kappa, w and F):
 *   1. the no-step pass of mg_nonlinearResidual runs on U: it writes S = kappa*w*g'(U) into the solver's level-0 reaction
 *      storage and gives *res_forward = ||N(U)|| (a host double, may be NULL), which says how converged the U is that the
 *      gradients are taken at.  A norm that is not finite: MG_ERR_ARG.
 *   2. S is coarsened as mg_solver_newton coarsens it.
 *   3. lam is set to zero and mg_solver_solve(Ubar, lam) runs on that reaction, with the Krylov acceleration if it is on.
 *   4. gA, gU as above, and (gW, *gkappa) = mg_sourceGradient(kind, kappa, w, lam, U) when gW != NULL.
 * Bit for bit the caller's sequence {mg_nonlinearResidual -> S, mg_solver_set_reaction(S), zero fill, mg_solver_solve,
 * mg_coefficientGradient, mg_boundaryGradient, mg_sourceGradient}.  On every return the solver has no reaction, as
 * mg_solver_newton leaves it.  gkappa: a host double, may be NULL; it needs gW.  Refused as mg_solver_newton refuses (a
 * reaction or a Neumann side set, fmg: MG_ERR_UNSUPPORTED; an unknown kind, kappa or w negative or not finite: MG_ERR_ARG),
 * and as mg_solver_adjoint_reaction refuses.  Returns the adjoint solve's status, as there. */
int mg_solver_newton_adjoint(mg_solver *s, int kind, double kappa, const double *w, const double *F, const double *U,
                             const double *Ubar, double *lam, double *gA, double *gU, double *gW, double *gkappa, double *res_forward,
                             mg_solve_result *out);

/* mg_solver_adjoint_reaction over mg_batch_solver_solve for n instances, each on its own reaction term and coefficient (or the
 * shared ones, or none): the gradient launches run once over all n instances, those that left the batch early included, and do
 * not depend on n.  Every instance is bit-identical to the single call on it alone.  gA, gU, gS may be NULL (not wanted for any
 * instance); gshift: a host array of n doubles, may be NULL, needs gS.  out: n results; stats (may be NULL) counts the
 * gradient launches too.  Refused with MG_ERR_ARG: what mg_batch_solver_solve refuses, and per instance what
 * mg_solver_adjoint_reaction refuses. */
int mg_batch_solver_adjoint_reaction(mg_batch_solver *s, int n, const double *const *Ubar, const double *const *U, double *const *lam,
                                     double *const *gA, double *const *gU, double *const *gS, double *gshift, mg_solve_result *out,
                                     mg_batch_solve_stats *stats);
/* mg_solver_newton_adjoint for n instances: kappa a host array of n values, w none (n_w = 0, w == NULL), one shared (n_w = 1) or
 * one per instance (n_w = n), as mg_batch_solver_newton takes them.  ONE no-step pass over all n instances, one coarsening
 * launch per level, one batched solve and the gradient launches; no lockstep is needed.  Every instance is bit-identical to
 * mg_solver_newton_adjoint on it alone.  gkappa, res_forward: host arrays of n doubles, may be NULL; gkappa needs gW.
 * mg_batch_solver_has_reaction is 0 on every return.  Refused as mg_batch_solver_newton and mg_batch_solver_adjoint_reaction
 * refuse. */
int mg_batch_solver_newton_adjoint(mg_batch_solver *s, int n, int kind, const double *kappa, int n_w, const double *const *w,
                                   const double *const *F, const double *const *U, const double *const *Ubar, double *const *lam,
                                   double *const *gA, double *const *gU, double *const *gW, double *gkappa, double *res_forward,
                                   mg_solve_result *out, mg_batch_solve_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* MG_ADJOINT_RX_H */
