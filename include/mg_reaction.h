/*
 * mg_reaction.h -- the residual-tolerance solver (mg_hip.h: mg_solver_*) with a variable reaction term:
 *     div(a grad U) - (sigma + s)*U = F     on the solver's N x N vertex grid, Dirichlet values on the rim of U,
 * sigma = mg_solve_opts.shift (>= 0), s an N x N fp64 device array given AT THE GRID POINTS, rim included, every value finite
 * and >= 0; a as in mg_varcoef.h, or absent (a = 1).  mg_hip.h includes this file; libmgpoisson.so exports every symbol
 * below.  This header is the specification: tests/_reaction_ref.py restates it on numpy, the kernels
 * (csrc/mg_reaction_kernels.hip) implement it.  Uses: the linearised Poisson-Boltzmann equation (s = kappa^2(x)), a Newton
 * step of a semilinear problem (s = g'(u)), absorbing or penalised regions, an implicit step with a varying capacity.
 *
 * Everything is the variable-coefficient cycle of mg_varcoef.h -- node order, transfers of U and D, tolerances, results,
 * read-backs, the level constants dx2, inv, sd = shift*dx2, omega -- except the centre.  Per interior point p of a level
 * with nodal reaction term s, every operation rounded once (no fma):
 *   t   = s[p]*dx2
 *   sdp = sd + t
 *   d   = (((aN + aS) + aE) + aW) + sdp,   q = 1/d (IEEE division),   c = omega*q
 * and the bracket b(U), the sweep, the residual, the red-black coarse update and the coarse stopping metric are mg_varcoef.h's
 * expressions with this d.  Without a coefficient a = 1 runs through the same expressions: every face is exactly 1 and
 * d = 4 + sdp; no array of ones is read.  The rim of s is never used by an operator; it is data for the coarsening only.
 *
 * Coarse levels take s_{l+1} = mg_coarsenCoefficient(s_l): the table, the end entries, the expression and the clamp of
 * mg_varcoef.h.  So a constant s stays that constant and s >= 0 carries to every level exactly; the host checks level 0 only.
 * Sampling keeps a discontinuous s discontinuous on every level, where the plain cycle is slow (a half plane of 1e5 at
 * N = 129 does not converge in 40 cycles): the Krylov acceleration (mg_krylov.h) is supported with a reaction for that case.
 *
 * The norms are sums of squares over the interior in the partition and order of the constant-coefficient norm of the same N;
 * the reference norm ||F|| has no operator in it and is the constant one.
 *
 * Consequences (tests/test_solve_reaction_cpu.py, tests/test_solve_reaction_gpu.py), each on U, history, cycles and flags, bit
 * for bit, with and without a coefficient:
 *   s == 0.0 everywhere     the same solver without a reaction: sd + 0.0*dx2 == sd
 *   s == c, shift == 0      the solver created with shift = c and no reaction: 0.0 + c*dx2 == shift*dx2
 *
 * What a reaction refuses (MG_ERR_UNSUPPORTED, the solver stays as it was): a solver created with fmg != 0; a boundary with
 * a Neumann side, in either order (mg_solver_set_reaction while one is set, mg_solver_set_boundary while a reaction is set) --
 * the combination would also give Robin sides and is not built; mg_solver_adjoint while a reaction is set.  The batched
 * solver takes one reaction term per instance, or one shared, through mg_rx_batch.h, every instance bit-identical to this
 * solver on it alone; the heat stepper and the eigensolver have no reaction.
 *
 * Memory contract (mg_hip.h): every function below reads its const arrays and writes its output array and nothing else.
 * Device arrays are 16-byte aligned.
 */
#ifndef MG_REACTION_H
#define MG_REACTION_H

#ifdef __cplusplus
extern "C" {
#endif

/* Give the solver the reaction term s (N x N device array), or take it away again (s_dev == NULL: the solver then enqueues
 * exactly what it enqueued before).  Behaves as mg_solver_set_coefficient: the array is checked on the device (every value
 * finite and >= 0: one launch, a flag, one read-back), copied into level-0 storage of the solver's own and coarsened to every
 * level; the caller's array is not kept.  Works on the engine stream and returns when the term is in place.  The level storage
 * (about 4/3 N^2 doubles) is allocated by the first call and reused.  With a reaction set, mg_solver_solve runs the cycle
 * operator by operator whatever mg_set_smoother says, with or without a coefficient; mg_solver_set_reaction,
 * mg_solver_set_coefficient and mg_solver_set_krylov work in any order.
 * Returns 0, or (mg_last_error; the solver keeps the state it had, reaction included, and stays usable):
 *   MG_ERR_ARG (2)          NULL solver, s_dev not 16-byte aligned, or a value of s that is negative or not finite
 *   MG_ERR_UNSUPPORTED (3)  the solver was created with fmg != 0, or a boundary with a Neumann side is set
 * A HIP error (1) before the check has passed leaves the state as it was too; one after it leaves the solver WITHOUT a
 * reaction. */
int  mg_solver_set_reaction(mg_solver *s, const double *s_dev);
/* 1 when a reaction is set, else 0 (NULL: 0) */
int  mg_solver_has_reaction(const mg_solver *s);

/* out = inv*b(U) on the interior, +0 on the rim, with the centre above (synchronous, engine stream; N >= 3, spacing L/(N-1));
 * a_dev == NULL: a = 1 */
void mg_applyOperatorReaction(int N, double L, double shift, const double *a_dev, const double *s_dev, const double *U, double *out);
/* TEST HOOKS, not part of the feature's interface: the kernels of the cycle on their own, exported so that
 * tests/test_solve_reaction_gpu.py can hold each against the restatement alone.  They may change with the kernels.
 * a_dev == NULL: a = 1 in each. */
/* one sweep: U_out = U_in + c*(b(U_in) - dx2*F), rim copied; U_in == NULL: the sweep from the zero field (rim +0) */
void mg_sweepReaction(int N, double L, double shift, double omega, const double *a_dev, const double *s_dev, const double *U_in,
                      const double *F, double *U_out);
/* D = inv*b(U) - F on the interior, +0 on the rim; sign < 0: the whole array negated */
void mg_residualReaction(int N, double L, double shift, const double *a_dev, const double *s_dev, const double *U, const double *F,
                         double *D, int sign);
/* the coarse solve alone: U_out = the red-black solve from zero on F to max(atol, rtol*err0), 1 .. max_iters iterations,
 * 3 <= N <= 63; the iterations through mg_lastExactSolverIterations() */
void mg_coarseSolveReaction(int N, double L, double shift, const double *a_dev, const double *s_dev, const double *F, double atol,
                            double rtol, int max_iters, double *U_out);

#ifdef __cplusplus
}
#endif
#endif /* MG_REACTION_H */
