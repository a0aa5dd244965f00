/*
 * mg_adjoint.h -- adjoint sensitivities of the residual-tolerance solvers (mg_hip.h: mg_solver_*, mg_batch_solver_*):
 * the gradients of a functional J(U) of a solve
 *     div(a grad U) - sigma*U = F     on the solver's N x N vertex grid, Dirichlet values g on the rim of U,
 * in the source F, in the rim data g and in the nodal coefficient a (mg_varcoef.h).  mg_hip.h includes this file after
 * mg_krylov_batch.h; libmgpoisson.so exports every symbol below.  This header is the specification:
 * tests/_adjoint_ref.py restates the two point kernels on numpy, the kernels (csrc/mg_adjoint_kernels.hip, bodies in
 * csrc/mg_adjoint_impl.h) implement them, the drivers are csrc/mg_adjoint.cpp.
 *
 * The discrete forward problem on the interior is  inv*b(U) - F = 0,  b the bracket of mg_varcoef.h with sd = shift*dx2 and
 * the rim of U carrying g.  Its operator is symmetric on the interior -- a face value 0.5*(a_p + a_q) is shared by the two
 * points it joins -- so the adjoint equation is the SAME equation with another right-hand side, and the adjoint solve is
 * mg_solver_solve itself: shift, coefficient, Krylov acceleration, the full-multigrid start and batching apply unchanged.
 *
 * Let Ubar = dJ/dU, an N x N array whose rim entries are the direct dependence of J on the rim values.
 *   1. adjoint field   lam solves the forward equation with right-hand side Ubar (the solver ignores the rim of a
 *                      right-hand side) from the zero field, so its rim is 0.
 *   2. gradient in F   dJ/dF = lam on the interior and 0 on the rim.
 *   3. gradient in a   at EVERY grid point k, rim and corners included.  With lam' = lam whose rim values are replaced by
 *                      +0.0 (substituted, never read: the solver's prolongation may move a rim value of lam by rounding on
 *                      sizes other than 2^k and 2^k + 1), h = 0.5*inv, and for the neighbour q of k in direction X
 *                      (N: row r+1, S: row r-1, E: column c+1, W: column c-1)
 *                          tX = (lam'_k - lam'_q)*(U_k - U_q),     tX = +0.0 when q lies outside the grid,
 *                          gA_k = h*((((0.0 + tN) + tS) + tE) + tW)
 *                      every difference, product and sum rounded once, in this order, no fma.
 *   4. gradient in g   an N x N array gU.  A rim point b that is not a corner has exactly one interior neighbour p:
 *                          gU[b] = Ubar[b] - inv*(f*lam[p]),   f = 0.5*(a[b] + a[p])    (a == NULL: f = 1.0)
 *                      with Ubar[b] taken as 0.0 when Ubar == NULL.  At the four corners gU = Ubar (or +0.0): no corner
 *                      enters a solve.  On the interior gU = +0.0: the answer does not depend on the initial guess.
 * inv is the level-0 constant of the solvers, inv = 1/dx2, dx2 = (L/(N-1))^2.
 *
 * Out of scope, and not built: the derivative in shift; gradients through the heat stepper (mg_heat.h); a coefficient
 * shared by several instances of a batch (its gradient is the caller's sum of the per-instance gA); slab / multi-GPU plans.
 * (The derivative in shift, and the adjoint with a reaction term or of a semilinear solve, are mg_adjoint_rx.h's.)
 *
 * Contract of every function below: synchronous, on the engine stream (mg_set_stream); N >= 3; device arrays 16-byte
 * aligned; no output overlaps an input or another output; bad arguments are refused with MG_ERR_ARG (mg_last_error) before
 * anything is enqueued, and without a device with MG_ERR_NOT_INIT.  Memory contract (mg_hip.h): each function reads its
 * const arrays and writes its output arrays, every value of them, and nothing else.
 */
#ifndef MG_ADJOINT_H
#define MG_ADJOINT_H

#ifdef __cplusplus
extern "C" {
#endif

/* gA = the gradient in a (3. above) from the adjoint field lam and the forward solution U; the rim of lam is not read */
void mg_coefficientGradient(int N, double L, const double *lam, const double *U, double *gA);
/* gU = the gradient in the rim data (4. above); a_dev == NULL: a = 1; Ubar == NULL: 0.0 */
void mg_boundaryGradient(int N, double L, const double *a_dev, const double *lam, const double *Ubar, double *gU);
/* the same on n >= 1 instances in ONE launch each (blockIdx picks the instance), instance i bit-identical to the single
 * call on lam[i], U[i] (a_dev[i], Ubar[i]).  lam, U, gA, gU: host arrays of n device pointers.  a_dev may be NULL, and so may
 * any entry of it: a = 1 for that instance; Ubar likewise: 0.0.  Inputs may repeat between instances; outputs overlap
 * nothing. */
void mg_coefficientGradient_batch(int n, int N, double L, const double *const *lam, const double *const *U, double *const *gA);
void mg_boundaryGradient_batch(int n, int N, double L, const double *const *a_dev /* NULL, or entries NULL: a = 1 */,
                               const double *const *lam, const double *const *Ubar, double *const *gU);

/* The adjoint of a solve of s in one call: lam is set to zero, mg_solver_solve(s, Ubar, lam, out) runs with whatever the
 * solver has set (coefficient, shift, Krylov, fmg), then gA = mg_coefficientGradient(lam, U) when gA != NULL and
 * gU = mg_boundaryGradient(the solver's own level-0 coefficient or NULL, lam, Ubar) when gU != NULL -- bit for bit the
 * result of that sequence made by the caller through the public functions; the host synchronises where the solve does and
 * once at the end.  U (the forward solution) is needed for gA only.  gA may be asked for without a coefficient set: it is
 * the sensitivity at a == 1.  Ubar == 0 runs 0 cycles and gives lam = gA = gU = 0.  Returns the solve's status: a solve
 * that does not converge still writes the gradients and returns MG_SOLVE_NOT_CONVERGED; an error code (> 0) otherwise.
 * Refused with MG_ERR_ARG: NULL s, Ubar or lam; gA without U; a misaligned array; lam, gA or gU overlapping an input or one
 * another. */
int  mg_solver_adjoint(mg_solver *s, const double *Ubar, const double *U, double *lam, double *gA, double *gU, mg_solve_result *out);
/* The same over mg_batch_solver_solve for n instances, each on its own coefficient (or the shared one, or none): the two
 * gradient launches run once over all n instances, those that left the batch early included.  gA and gU may be NULL (not
 * wanted for any instance); U is needed for gA only.  out: n results; stats (may be NULL) counts the gradient launches
 * too.  Refused with MG_ERR_ARG: what mg_batch_solver_solve refuses, and per instance what mg_solver_adjoint refuses. */
int  mg_batch_solver_adjoint(mg_batch_solver *s, int n, const double *const *Ubar, const double *const *U, double *const *lam,
                             double *const *gA, double *const *gU, mg_solve_result *out, mg_batch_solve_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* MG_ADJOINT_H */
