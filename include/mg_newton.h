/*
 * mg_newton.h -- the semilinear problem on the residual-tolerance solver (mg_hip.h: mg_solver_*), Newton's method around it:
 *     div(a grad U) - sigma*U - kappa*w*g(U) = F     on the solver's N x N vertex grid, Dirichlet values on the rim of U,
 * sigma = mg_solve_opts.shift (>= 0), a as in mg_varcoef.h or absent (a = 1), the scalar kappa finite and >= 0, w an optional
 * N x N fp64 device array AT THE GRID POINTS, rim included, every value finite and >= 0 (NULL: w = 1; e.g. the ion-accessible
 * region of a Poisson-Boltzmann problem), g one of three monotone kinds.  mg_hip.h includes this file; libmgpoisson.so exports
 * every symbol below.  This header is the specification: tests/_newton_ref.py restates it on numpy, the kernel
 * (csrc/mg_newton_kernels.hip) and the driver (csrc/mg_solve.cpp) implement it.
 *
 *   kind               g(u)     g'(u)    per point, every operation rounded once, no fma outside exp_libm
 *   MG_NEWTON_CUBIC    u^3      3u^2     q = u*u; g = q*u; gp = 3.0*q
 *   MG_NEWTON_SINH     sinh u   cosh u   e = exp_libm(u); f = 1.0/e; g = 0.5*(e - f); gp = 0.5*(e + f)
 *   MG_NEWTON_EXP      e^u      e^u      g = gp = exp_libm(u)
 * exp_libm (csrc/mg_exp_libm.h) is the getSource kernel's exp: libm's algorithm in its FMA form, equal to the host's exp()
 * bit for bit where mg_source_is_bit_identical() says so, on its verified path |u| < 512.  The bit-for-bit contract of this
 * header covers |v| < 512.  Beyond it exp_libm is the device library's exp(): a trial with v >= 512 is in practice rejected
 * (g^2 overflows the norm for both kinds; e = +inf above 709.78 gives g = g' = +inf), and so is one with v <= -512 for
 * MG_NEWTON_SINH, but MG_NEWTON_EXP REACHES v <= -512 IN ACCEPTED TRIALS: there g is tiny, the norm stays finite (F = +1e4 with
 * zero rim data has its solution's minimum near -737).  What is guaranteed there is the class and the size of e, not libm's
 * bits: +0 from -746 down and for -inf, NaN for NaN, otherwise a finite e >= 0, subnormal below -708.39, within 2 ulp of e^v
 * (counted in the subnormal spacing where e^v is subnormal; measured 0.4984 ulp: tests/test_newton_exp_domain_gpu.py).
 * g' >= 0 makes every Newton matrix a reaction operator the solver accepts (mg_reaction.h: s >= 0).
 *
 * THE PASS (mg_nonlinearResidual; one kernel launch and the second stage of the norm).  At every point p:
 *   v    = U[p]                     no step, and on the rim in either form
 *        = U[p] + t*dlt[p]          the step form, interior points: the product rounded, then the sum
 *   kw   = kappa                    no w
 *        = kappa*w[p]
 *   S[p] = kw*gp(v)                 on ALL N^2 points, rim included (the coarsening of s samples the rim)
 *   lin  = inv*b(v)                 mg_varcoef.h's operator expression with sd = shift*dx2, on the window of v
 *   D[p] = (F[p] + kw*g(v)) - lin   on the interior, +0 on the rim
 *   V[p] = v                        only in the step form; the rim of V is the rim of U bit for bit (a -0.0 stays -0.0)
 * and *norm = sqrt(sum of D^2 over the interior) in the partition and the order of the solver's residual norm of the same N,
 * so norms and histories compare with ==.  D = -N(v) is the right-hand side of the Newton equation (A - S) delta = D, which
 * is the equation mg_reaction.h solves with reaction S.  The rims of dlt and of F are not read into any result.  V, D and S
 * must not overlap any input or each other.
 *
 * THE DRIVER (mg_solver_newton).  r is the norm above.
 *   1. the no-step pass on U: D, S, r0 = r.  r0 not finite: MG_ERR_ARG.
 *   2. converged when r <= max(atol, rtol*r0); otherwise, while fewer than max_iters iterations have been accepted:
 *   3. S becomes the solver's reaction: the pass wrote it into the solver's own level-0 storage, the levels below are
 *      coarsened from it as mg_solver_set_reaction coarsens them.  (No check launch: a non-finite S gives a non-finite norm.)
 *   4. delta = 0, then mg_solver_solve's own loop on (D, delta): the solver's create-time rtol / atol / max_cycles govern this
 *      inner solve (its rtol is the forcing term), GCR(m) runs when mg_solver_set_krylov is on.  An inner solve that ends
 *      unconverged is not an error: its step is used and counted.
 *   5. the line search, t = 1, 1/2, 1/4, ...: the step pass on (U, delta, t) into a second set (V, D', S'); the trial is
 *      accepted when its norm r' is finite and r' < (1 - 1e-4*t)*r  (the product, the difference and the product each rounded).
 *      Accepted: the sets swap, so the accepted trial's D', S' are the next iteration's step 1, and r = r'.  Rejected:
 *      t is halved; the rejection that follows max_backtracks earlier ones in the same iteration ends the call with
 *      MG_NEWTON_STALLED and U the last accepted iterate (max_backtracks = 0: t = 1 is the only trial).
 *   6. between iterations only norms are read back.
 * On every return, errors included, the solver has no reaction, as before the call, and U holds the last accepted iterate.
 * The first call allocates the driver's level-0 arrays (5 N^2 doubles) and, if no reaction was ever set, the reaction's
 * level storage (about 4/3 N^2); later calls allocate nothing.
 *
 * What the driver refuses (the solver stays as it was, U untouched; mg_last_error):
 *   MG_ERR_UNSUPPORTED (3)  the caller has a reaction set; a boundary with a Neumann side is set; the solver was created with
 *                           fmg != 0
 *   MG_ERR_ARG (2)          an unknown kind; kappa negative or not finite; a value of w negative or not finite (one check launch
 *                           on w); a NULL solver, F or U; an array that is not 16-byte aligned; options out of range (rtol,
 *                           atol negative or not finite, max_iters or max_backtracks negative); a start whose residual is not
 *                           finite
 * The batched solver runs this driver for many instances in one call: mg_newton_batch.h.
 * Not built: the heat stepper, the adjoint of a semilinear solve, boundary kinds, a user-supplied g.  (The adjoint is built
 * since, beside this header: mg_adjoint_rx.h, mg_solver_newton_adjoint.)
 */
#ifndef MG_NEWTON_H
#define MG_NEWTON_H

#ifdef __cplusplus
extern "C" {
#endif

#define MG_NEWTON_CUBIC 0
#define MG_NEWTON_SINH  1
#define MG_NEWTON_EXP   2

#define MG_NEWTON_CONVERGED      0
#define MG_NEWTON_NOT_CONVERGED (-1)   /* max_iters iterations were accepted without meeting the tolerance */
#define MG_NEWTON_STALLED       (-2)   /* the line search ran out of trials: U is the last accepted iterate */

typedef struct mg_newton_opts {
    double rtol, atol;        /* stop when ||N(U)|| <= max(atol, rtol*||N(U_0)||) */
    int    max_iters;         /* >= 0; 0: the start's norm alone, no solve */
    int    max_backtracks;    /* >= 0: halvings of t allowed per iteration */
} mg_newton_opts;

typedef struct mg_newton_result {
    int    status;            /* MG_NEWTON_CONVERGED, _NOT_CONVERGED, _STALLED, or an error code (> 0, mg_last_error) */
    int    iterations;        /* accepted Newton steps */
    int    converged;
    int    n_history;         /* records mg_solver_newton_history has: iterations, + 1 after a stalled line search */
    double res0, res;         /* ||N(U_0)||, ||N(U)|| of the iterate returned */
    int    inner_cycles;      /* cycles (or GCR iterations) of all inner solves together */
    int    trials;            /* step passes run */
} mg_newton_result;

/* one Newton iteration: res = the norm after it (a stalled one: the norm it could not lower, t = 0) */
typedef struct mg_newton_iter {
    double res, t;
    int    backtracks;        /* rejected trials */
    int    inner_cycles;
    int    inner_converged;
    int    inner_capped;      /* the inner solve's coarse_capped */
} mg_newton_iter;

/* rtol 1e-8, atol 0, max_iters 20, max_backtracks 12 */
void mg_newton_opts_default(mg_newton_opts *o);
/* The driver above on the engine stream; w_dev == NULL: w = 1; opts == NULL: the defaults; out may be NULL.  Returns
 * out->status. */
int  mg_solver_newton(mg_solver *s, int kind, double kappa, const double *w_dev, const double *F_dev, double *U_dev,
                      const mg_newton_opts *opts, mg_newton_result *out);
/* the records of the last mg_solver_newton, oldest first: copies min(cap, n) of them into out (may be NULL) and returns n */
int  mg_solver_newton_history(const mg_solver *s, mg_newton_iter *out, int cap);
/* the residual history r_0 .. r_cycles of the solver's LAST solve -- after mg_solver_newton, of its last inner solve -- copied
 * like the records above (a test hook: kappa = 0 makes the one inner solve the linear solve of F) */
int  mg_solver_newton_inner_history(const mg_solver *s, double *out, int cap);

/* THE PASS on its own, the building block and test hook (synchronous, engine stream; N >= 3, spacing L/(N-1)).  a_dev == NULL:
 * a = 1; w_dev == NULL: w = 1; dlt == NULL selects the no-step form, which reads neither t nor V (V may be NULL then).
 * norm: a HOST double (may be NULL).  The partial sums live in a buffer the call allocates and frees.  Returns 0, or
 * MG_ERR_ARG (N < 3, L or shift out of range, an unknown kind, kappa negative or not finite, a NULL or misaligned array) or
 * MG_ERR_HIP; w is not checked here. */
int  mg_nonlinearResidual(int N, double L, double shift, const double *a_dev, int kind, double kappa, const double *w_dev,
                          const double *U, const double *dlt, double t, const double *F, double *V, double *D, double *S,
                          double *norm);

#ifdef __cplusplus
}
#endif
#endif /* MG_NEWTON_H */
