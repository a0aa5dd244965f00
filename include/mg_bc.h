/*
 * mg_bc.h -- boundary kinds per side for the residual-tolerance solver (mg_hip.h: mg_solver_*) and the heat stepper
 * (mg_heat.h):
 *     div(a grad U) - sigma*U = F     on the solver's N x N vertex grid,
 * each of the four sides Dirichlet (U given on it) or Neumann (dU/dn given on it).  mg_hip.h includes this file after mg_eigs.h;
 * libmgpoisson.so exports every symbol below.  This header is the specification: tests/_bc_ref.py restates it on numpy, the
 * kernels (csrc/mg_bc_kernels.hip, point code in csrc/mg_bc_impl.h) implement it.
 *
 * Sides and points.  kind is a host int[4] in the order S, N, W, E: row 0, row N-1, column 0, column N-1, each
 * MG_BC_DIRICHLET (0) or MG_BC_NEUMANN (1).  A grid point is DATA when it lies on a Dirichlet side -- a corner shared with a
 * Neumann side included -- and an UNKNOWN otherwise: the interior, the rim points of Neumann sides, the corner between two
 * Neumann sides.  The unknowns form the rectangle rows [kS ? 0 : 1, kN ? N-1 : N-2] x columns [kW ? 0 : 1, kE ? N-1 : N-2].
 * On a Neumann side the rim of U is part of the guess and is written by every function below that writes U.
 *
 * Homogeneous operator.  At an unknown whose neighbour would fall outside the grid the missing neighbour is the MIRROR
 * point, for the value and for the nodal coefficient alike:
 *     U[r][-1] := U[r][1],  a[r][-1] := a[r][1],  U[r][N] := U[r][N-2],  a[r][N] := a[r][N-2],  rows likewise;
 * the corner of two Neumann sides mirrors both ways.  With that substitution the face coefficients, d, q, c, the bracket
 * b(U), the sweep, the residual inv*b(U) - F and the coarse red-black update are the expressions and orders of mg_varcoef.h,
 * unchanged (every product and every sum rounded once, no fma; dx2 = (L/(N-1))^2, inv = 1/dx2, sd = shift*dx2), evaluated at
 * every unknown instead of at the interior.  A mirrored neighbour has the colour (row + col) & 1 its ghost would have, so
 * the red-black split of the coarse solve stays consistent.  Data points keep their value in a sweep (zero start: +0) and get
 * +0 (-0 under sign < 0) in a residual and in the operator on its own.  a_dev == NULL means a = 1 through the same
 * expressions.  With four Dirichlet sides every function below is its mg_varcoef.h counterpart bit for bit.
 *
 * Flux data.  An inhomogeneous dU/dn = g (n the OUTWARD normal) enters through the right-hand side only (mg_neumannSource):
 * with h = L/(N-1) and t = 2.0/h, at a rim unknown p of a Neumann side
 *     F_eff[p] = F[p] - (t*a[p])*g[p]          (a[p] the NODAL coefficient, not a face average; a_dev == NULL: 1.0)
 * subtracted in the order S, N, W, E, so that a corner of two Neumann sides gets both sides' terms.  Every other point is
 * copied.  g is a 4 x N array with the rows S, N, W, E, indexed by the column (S, N) or the row (W, E) of p; entries on
 * Dirichlet sides are not read.  This is the half-cell finite-volume balance of the rim cell (the mirror row times h/2 on
 * the side's face), and it is second-order accurate; folding the flux in with a face-averaged coefficient is first-order
 * only (tests/test_solve_bc_cpu.py).  The solver itself only ever sees F_eff.
 *
 * Norms and stopping.  res, res0, ref_norm and the history are L2 sums over the unknowns in the block partition and
 * summation order of the mg_varcoef.h norm of the same N: with four Dirichlet sides they are that norm bit for bit.  The
 * coarse error metric and err0 divide by the number of unknowns instead of (N-2)^2.
 *
 * Transfers.  The constant solver's restriction writes the interior only and its prolongation leaves rim points alone, so
 * the boundary path has transfer operators of its own.
 *   restriction       at every coarse unknown doRestriction's expression and order
 *                         v = b*d*D[f] + a*d*D[f+1] + c*b*D[f+N] + a*c*D[f+N+1],  a = w[col], b = 1.0 - a, c = w[row],
 *                         d = 1.0 - c, f = lo[col] + lo[row]*N
 *                     on the 1-D table (lo, w) = mg_restriction_table(N, M) with the end entries replaced by (0, 0.0) and
 *                     (N-2, 1.0), exactly as mg_coarsenCoefficient replaces them; no clamp.  Coarse data points get +0.  At
 *                     interior coarse points this is doRestriction bit for bit.
 *   prolongation-add  U_out = U_in + P(U_c) at fine unknowns, fine data points are copied bit for bit.  P is a gather with
 *                     the host table mg_boundary_prolongation_table(M, N, lo, w): with h_f = 1.0/(N-1), h_c = 1.0/(M-1),
 *                         lo[k] = min((int)floor(k*h_f/h_c), M-2),  w[k] = (k*h_f - lo[k]*h_c)/h_c clamped into [0, 1],
 *                     the ends forced to (0, 0.0) and (M-2, 1.0); the value is
 *                         b*d*C[f] + a*d*C[f+1] + c*b*C[f+M] + a*c*C[f+M+1],  a = w[col], c = w[row], f = lo[col] + lo[row]*M.
 *   coefficient       the hierarchy is mg_coarsenCoefficient's, unchanged: it already covers the rim.
 * The rows that are restricted are the unscaled pointwise rows inv*b(U) - F, at the rim as inside: they approximate the
 * differential equation at every unknown, so sampling them gives the coarse equation's right-hand side.
 *
 * Cycle.  Node order, ping-pong, tolerances and result fields are those of the variable-coefficient cycle.  With a boundary
 * set the cycle runs operator by operator whatever mg_set_smoother says, as it does with a coefficient.  Setting four
 * Dirichlet sides takes the boundary away: the solver then enqueues exactly what it enqueued before.
 *
 * Heat.  mg_heat_rhs_boundary is the right-hand side of mg_heat.h / mg_heat_vc.h,
 *     F = -(sigma*u) - beta*(inv*b(u)) - gamma*q      (s = -(sigma*u); theta != 1: s = s - beta*lap; Q given: s = s - gamma*q)
 * evaluated at every unknown with the mirrored operator (sd = 0.0), +0 at data points; theta == 1 reads no neighbour and no
 * coefficient.  A stepper with a boundary runs {mg_heat_rhs_boundary, solve with shift = sigma} per step; k steps are
 * bit-identical to the caller's own loop of those two calls.  The walls of the stepper are homogeneous (insulated).  A
 * constant wall flux a*du/dn = a*g enters through the source: Q_eff = Q + nu*(2/h)*a*g at the wall points (both sides' terms
 * at a corner), which is mg_neumannSource's term carried through F = ... - gamma*q.
 *
 * Memory contract (mg_hip.h): every function below reads its const arrays and writes its output array and nothing else.
 * Device arrays are 16-byte aligned, N >= 3, no output overlaps an input.
 *
 * Not built, each refused with a message that names it: boundary kinds in the batched solver, the eigen-solver, the
 * full-multigrid start, the Krylov acceleration and the adjoint, Robin and periodic sides.  The pure Neumann problem at
 * sigma = 0 (mean fixing and the compatibility projection) is mg_singular.h's, and is refused here until it is switched on there.
 */
#ifndef MG_BC_H
#define MG_BC_H

#define MG_BC_DIRICHLET 0
#define MG_BC_NEUMANN 1

#ifdef __cplusplus
extern "C" {
#endif

/* Set the four kinds of the solver (kind: host int[4], S, N, W, E).  Four Dirichlet sides take the boundary away.  The first
 * call with a Neumann side builds the prolongation tables of the hierarchy on the device.  Returns 0, or (mg_last_error; the
 * solver keeps the state it had, the earlier kinds included, and stays usable):
 *   MG_ERR_ARG (2)          NULL solver or kind, or a kind outside {0, 1}
 *   MG_ERR_UNSUPPORTED (3)  four Neumann sides with shift == 0 (the singular problem) without mg_solver_set_mean; a solver
 *                           created with fmg != 0; the Krylov acceleration switched on
 * While a boundary is set, mg_solver_set_krylov(m > 0) and mg_solver_adjoint are refused with MG_ERR_UNSUPPORTED. */
int  mg_solver_set_boundary(mg_solver *s, const int *kind);
/* kind_out (may be NULL) = the four kinds; returns 1 when any side is Neumann, else 0 (NULL solver: 0) */
int  mg_solver_boundary(const mg_solver *s, int *kind_out);

/* the building blocks on their own (synchronous, engine stream); kind: host int[4], a_dev may be NULL (a = 1) */
/* F_out = F with the flux terms subtracted at the rim unknowns of Neumann sides, a full copy elsewhere; g: 4 x N */
void mg_neumannSource(int N, double L, const int *kind, const double *a_dev, const double *F, const double *g, double *F_out);
/* out = inv*b(U) at the unknowns, +0 at data points */
void mg_applyOperatorBoundary(int N, double L, double shift, const int *kind, const double *a_dev, const double *U, double *out);
/* the 1-D table of the prolongation from M coarse to N fine points (host arrays lo[N], w[N]); host only */
void mg_boundary_prolongation_table(int M, int N, int *lo, double *w);

/* TEST HOOKS, not part of the feature's interface: they may change with the kernels. */
/* one sweep: U_out = U_in + c*(b(U_in) - dx2*F) at the unknowns, data points copied; U_in == NULL: from the zero field */
void mg_sweepBoundary(int N, double L, double shift, double omega, const int *kind, const double *a_dev, const double *U_in,
                      const double *F, double *U_out);
/* D = inv*b(U) - F at the unknowns, +0 at data points; sign < 0: the whole array negated */
void mg_residualBoundary(int N, double L, double shift, const int *kind, const double *a_dev, const double *U, const double *F,
                         double *D, int sign);
/* F_c (M x M) = the restriction of D (N x N) at the coarse unknowns, +0 at coarse data points */
void mg_restrictBoundary(int N, const int *kind, const double *D, int M, double *F_c);
/* U_out (N x N) = U_in + P(U_c) (U_c: M x M) at the fine unknowns, U_in at fine data points */
void mg_prolongAddBoundary(int M, const int *kind, const double *U_c, int N, const double *U_in, double *U_out);

/* heat: F = rhs(a, U, Q) as defined above; Q may be NULL.  Refuses what mg_heat_rhs_coef refuses, and a bad kind. */
void mg_heat_rhs_boundary(int N, double L, double nu, double dt, double theta, const int *kind, const double *a_dev,
                          const double *U, const double *Q, double *F);
/* the kinds of the stepper's walls (insulated); goes to the inner solver's mg_solver_set_boundary, whose refusals pass
 * through.  MG_ERR_UNSUPPORTED also for a stepper created with max_batch > 1 (four Dirichlet sides ask for the state it is
 * in and return 0). */
int  mg_heat_stepper_set_boundary(mg_heat_stepper *st, const int *kind);

#ifdef __cplusplus
}
#endif
/* the pure Neumann problem (four flux sides at sigma = 0, mean fixed): mg_solver_set_mean, mg_weightedMean, mg_projectMean */
#include "mg_singular.h"
#endif /* MG_BC_H */
