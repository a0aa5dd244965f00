/*
 * mg_heat_vc.h -- the heat stepper (mg_heat.h) with a variable coefficient (mg_varcoef.h):
 *     u_t = nu * div(a grad u) + q     on the solvers' N x N vertex grid, Dirichlet values on the rim of U,
 * a an N x N fp64 device array given AT THE GRID POINTS, rim included, every value finite and > 0, frozen over a call.
 * mg_hip.h includes this file after mg_varcoef.h; libmgpoisson.so exports every symbol below.  This header is the
 * specification: tests/_heat_vc_ref.py restates it on numpy, the kernel (csrc/mg_heat_vc_kernels.hip) implements it.
 *
 * The scheme is mg_heat.h's with the operator A_h u = inv*b(u) of mg_varcoef.h (sd = 0.0) in the Laplacian's place:
 *   (u+ - u)/dt = nu*(theta*A_h u+ + (1 - theta)*A_h u) + q
 *   <=>  A_h u+ - sigma*u+ = F,   F = -sigma*u - beta*A_h u - gamma*q
 * which is the equation of mg_varcoef.h with shift = sigma: the implicit step of diffusion in a heterogeneous medium.  The
 * scheme parameters and host constants are mg_heat.h's, unchanged: alpha = theta*nu, sigma = 1.0/(alpha*dt),
 * beta = (1.0 - theta)/theta, gamma = 1.0/alpha, dx2 and inv the level-0 constants of the solvers.  Per interior point p
 * (row-major, p+N: row r+1), every product and every sum rounded once (no fma), in this order:
 *   faces (mg_varcoef.h)   aN = 0.5*(a[p] + a[p+N]),  aS = 0.5*(a[p] + a[p-N]),  aE = 0.5*(a[p] + a[p+1]),  aW = 0.5*(a[p] + a[p-1])
 *   centre                 d = ((aN + aS) + aE) + aW            (mg_varcoef.h's d with sd = 0.0, which changes no bit)
 *   bracket                b = (((aN*U[p+N] + aS*U[p-N]) + aE*U[p+1]) + aW*U[p-1]) - d*U[p]
 *                          lap = inv*b
 *                          s = -(sigma*u)
 *   theta != 1:            s = s - beta*lap
 *   q given:               s = s - gamma*q
 *   F = s;  every rim point of F is written as +0.0 (the solvers ignore the rim of F).
 * Consequences (tests/test_heat_vc_cpu.py, tests/test_heat_vc_gpu.py):
 *   theta exactly 1   the right-hand side reads neither a neighbour nor a: it is mg_heat.h's, enqueued as the very launch the
 *                     stepper without a coefficient enqueues.  The coefficient then acts through the solve alone.
 *   a == 1            every face is 1.0 and d = 4.0, the bracket is mg_heat.h's, and F equals mg_heat_rhs's bit for bit.
 *                     With the a == 1 contract of mg_varcoef.h, a stepper with this coefficient equals the stepper without
 *                     one bit for bit: U, cycles of every step, flags.
 *   k steps           equal, bit for bit, k times {mg_heat_rhs_coef, mg_solver_solve with shift = mg_heat_stepper_sigma and
 *                     the same coefficient}.
 * A time-dependent rim written into U before each steps = 1 call is exact only for theta = 1, whose right-hand side reads no
 * neighbour: for theta < 1 the right-hand side takes A_h of u_old next to the rim, and a rim already at the new time puts two
 * time levels into it (an error of first order in the rim's change, not the theta-scheme).  There the caller runs
 * mg_heat_rhs_coef on the old field with its old rim, then sets the new rim, then solves with mg_solver_solve at shift =
 * mg_heat_stepper_sigma.
 * Not built, and refused where it could be asked for: a batched stepper with a coefficient (max_batch > 1 steps through
 * mg_batch_solver and does not hand it one: mg_varcoef_batch.h), fmg with a coefficient (the inner mg_solver refuses it), a
 * heat capacity multiplying u_t.
 */
#ifndef MG_HEAT_VC_H
#define MG_HEAT_VC_H

#ifdef __cplusplus
extern "C" {
#endif

/* the building block on its own (synchronous, engine stream): F = rhs(a, U, Q) as defined above; Q may be NULL (no source);
 * a_dev == NULL: a = 1 everywhere, which is exactly mg_heat_rhs.  a, U, Q, F: N x N device arrays, 16-byte aligned, N >= 3;
 * F overlaps none of a, U and Q.  Reads a, U and Q, writes F only; no corner value of a enters F, and with theta == 1 a is
 * not read at all.  a is not checked for sign or finiteness here (as mg_applyOperator).  Refused with MG_ERR_ARG: what
 * mg_heat_rhs refuses, an a that is not 16-byte aligned, an F that overlaps a. */
void mg_heat_rhs_coef(int N, double L, double nu, double dt, double theta, const double *a_dev, const double *U, const double *Q,
                      double *F);

/* Give the stepper the coefficient a (N x N device array), or take it away again (a_dev == NULL: back to the constant
 * stepper, which then enqueues exactly what it always enqueued).  The array goes to the inner mg_solver through
 * mg_solver_set_coefficient, which checks it, copies it and coarsens it; the stepper keeps no copy of its own -- the
 * right-hand-side kernel reads the solver's level-0 array -- and the caller's array may be freed after the call.  From then on
 * a step with theta != 1 forms its right-hand side with the kernel above (one launch per step, as before), and the solve of
 * every step is the variable-coefficient solve with shift = sigma.
 * Returns 0, or (mg_last_error; the stepper keeps the state it had, coefficient included, and stays usable):
 *   MG_ERR_ARG (2)          NULL stepper, or what mg_solver_set_coefficient refuses with it (alignment, a value of a that is
 *                           not finite or not > 0); the solver's code and text pass through
 *   MG_ERR_UNSUPPORTED (3)  a stepper created with max_batch > 1 (the stepper hands its batch solver none; a_dev == NULL asks for
 *                           the state it is in and returns 0), or with solve.fmg != 0 (the solver's own refusal) */
int  mg_heat_stepper_set_coefficient(mg_heat_stepper *s, const double *a_dev);
/* 1 when a coefficient is set, else 0 (NULL: 0) */
int  mg_heat_stepper_has_coefficient(const mg_heat_stepper *s);

#ifdef __cplusplus
}
#endif
#endif /* MG_HEAT_VC_H */
