/*
 * mg_krylov.h -- Krylov acceleration of the residual-tolerance solver (mg_hip.h: mg_solver_*): restarted GCR(m) with one
 * V(pre, post) cycle from a zero start as the preconditioner.  mg_hip.h includes this file; libmgpoisson.so exports every
 * symbol below.  This header is the specification: tests/_krylov_ref.py restates it on numpy, the kernels
 * (csrc/mg_krylov_kernels.hip) and the driver (csrc/mg_solve.cpp) implement it.
 *
 * Why GCR and not CG: the cycle is no symmetric operator (doRestriction is not the transpose of doProlongation, pre may
 * differ from post) and no fixed one (the coarse solve stops on a relative target).  GCR minimises the residual over its
 * directions whatever the preconditioner is, so the recurred residual norm never grows in exact arithmetic -- on
 * coefficients on which the plain iteration U <- U + M(F - AU) is slow or diverges too.
 *
 * Notation.  A is the solver's operator at level 0: constant, shifted (mg_solve_opts.shift) or with a coefficient
 * (mg_varcoef.h); A*x is the launch of mg_applyOperator, inv*b(x) on the interior and +0 on the rim.  M(r) is one cycle
 * vcycle(F0 = r, U0 = z) on a zeroed array z, through whichever cycle mg_solver_solve runs (fused, MG_SMOOTHER=simple, or
 * the variable-coefficient one).  <x, y> is the sum of x[p]*y[p] over the INTERIOR points p, ||x|| = sqrt(<x, x>).  Every
 * elementwise operation is rounded once (no fma).  Slots z_j, q_j (N x N arrays) and w_j (scalars) run over j < m.
 * tol = max(rtol*||F||, atol), ref_norm, max_cycles, rtol, atol are those of mg_solver_solve.
 *
 *   r = -(inv*b(U) - F) (the cycle's signed residual: -0 on the rim)     rho = ||F - AU||     history[0] = rho     k = 0
 *   while !(rho <= tol) and cycles < max_cycles:
 *       z_k = 0 (the whole array);  z_k = M(r);  q_k = A*z_k
 *       d_j = <q_k, q_j>  for j < k                    (ONE launch, every d_j from the unmodified q_k)
 *       b_j = d_j * w_j
 *       for j = 0 .. k-1 in this order, per interior point:   q_k = q_k - b_j*q_j ;  z_k = z_k - b_j*z_j
 *       g = <q_k, q_k> ,  h = <r, q_k>                 (the same launch, on the updated q_k)
 *       w_k = 1/g ;  alpha = h*w_k
 *           breakdown -- g not > 0, or g or alpha not finite: alpha = 0, the flag is set, and the loop ends after this iteration
 *       per interior point:   U = U + alpha*z_k ;  r = r - alpha*q_k     (alpha == 0: U and r keep their bits)
 *       rho_rec = sqrt(<r, r>)                         (the same launch, on the updated r)
 *       cycles += 1 ;  k += 1
 *       if k == m or rho_rec <= tol:   r = -(inv*b(U) - F) ;  rho = ||F - AU||  (the launches of mg_solver_solve's residual
 *                                      and norm: recomputed from U) ;  k = 0     -- a RESTART
 *       else                           rho = rho_rec
 *       history.push(rho)
 *
 * `cycles` counts preconditioner applications.  `converged` is only ever stated on a RECOMPUTED residual: the recurred norm
 * drifts from the true one (by a small factor near 1e-9 of ||F||), so a recurred norm at or below tol only triggers the
 * recomputation; when that one is above tol the iteration goes on from k = 0.  A solve that ends on max_cycles or on a
 * breakdown between two restarts reports the recurred norm as `res` (it is history's last entry) and is not converged.
 * b_j, w_k and alpha are formed on the device and never read back; the host reads one norm per iteration, as the plain
 * loop does (and the recomputed one after it in the iteration that restarts because rho_rec <= tol).  Every sum is a
 * two-stage reduction over a fixed partition -- per-block partials, then a finish launch -- without floating-point
 * atomics: the same call twice gives the same bits.  A sum's value is specified up to its summation order: within
 * n*u/(1 - n*u) * sum|x[p]*y[p]| of the exact sum, n = (N-2)^2, u = 2^-53; everything else above is specified bit for
 * bit GIVEN the sums (tests/_krylov_ref.py replays a solve from the logged d_j, g, h).
 *
 * The rim of q_j, z_j, r and U is never written by the Krylov kernels, and never read into a result: values on the rim of
 * any of them (NaN included) show in no output and no sum.
 *
 * Memory.  The first enabling call allocates r, 2m slots and the partials: (2m + 1)*N^2 doubles -- 8.7 GB at N = 8192 for
 * m = 8 -- beside the solver's own level arrays.  A larger m later allocates the additional slots.  A solve allocates
 * nothing.  Per iteration beyond the cycle the kernels move 120 + 24k bytes per point (the zeroing of z_k 8, A*z_k 16 or
 * 24 with a coefficient, the dots 8 + 8k, the orthogonalisation 40 + 16k, the update 48) where the plain loop spends one
 * norm launch (16, or 24 with a coefficient).
 *
 * Memory contract (mg_hip.h): the test hooks below read their const arrays and write the arrays named as written, interior
 * only, and nothing else (tests/test_solve_krylov_gpu.py holds them inside guard bands).  Device arrays are 16-byte aligned.
 */
#ifndef MG_KRYLOV_H
#define MG_KRYLOV_H

#ifdef __cplusplus
extern "C" {
#endif

#define MG_KRYLOV_MAX_M 16

/* Switch the acceleration on (1 <= m <= MG_KRYLOV_MAX_M: GCR(m)) or off (m == 0: mg_solver_solve enqueues the very launches
 * it enqueued before this option existed, bit for bit).  Storage is allocated here (see Memory above) and kept until the
 * solver is destroyed; m == 0 keeps it for the next enabling call.  Works with and without a coefficient
 * (mg_solver_set_coefficient before or after this call), with any shift, and under MG_SMOOTHER=simple.
 * Returns 0, or (mg_last_error; the solver keeps the state it had, its m included, and stays usable):
 *   MG_ERR_ARG (2)          NULL solver, or m outside [0, MG_KRYLOV_MAX_M]
 *   MG_ERR_UNSUPPORTED (3)  the solver was created with fmg != 0: the full-multigrid start is not combined with the
 *                           acceleration yet, and an option is never silently ignored
 *   MG_ERR_HIP (1)          an allocation failed: what this call had allocated is freed again */
int  mg_solver_set_krylov(mg_solver *s, int m);
/* the current m (0: off; NULL: 0) */
int  mg_solver_krylov(const mg_solver *s);
/* 1 when the last solve ended on a breakdown (see above), else 0 (NULL, or the acceleration off: 0) */
int  mg_solver_krylov_breakdown(const mg_solver *s);
/* TEST HOOK AND DIAGNOSTIC, not part of the feature's interface; it may change with the kernels.  The records of the last
 * accelerated solve, one per iteration, m + 7 doubles each (m: the value at that solve):
 *     k,  d_0 ... d_{m-1} (entries j >= k: +0),  g,  h,  alpha,  rho_rec,  restarted (0 or 1),  rho
 * written by the device into a buffer sized for max_cycles records and copied back once at the end of the solve.
 * out == NULL: returns the number of records; otherwise copies at most cap records and returns how many. */
int  mg_solver_krylov_log(const mg_solver *s, double *out, int cap);

/* TEST HOOKS, not part of the feature's interface: each kernel on caller arrays (synchronous, engine stream), exported so
 * that tests/test_solve_krylov_gpu.py can hold each kernel against numpy alone.  They may change with the kernels.
 * N >= 3, 0 <= k <= MG_KRYLOV_MAX_M - 1; q, z, r, U and the entries of Q, Z: N x N device arrays, 16-byte aligned, no two
 * the same; Q, Z, b, out, gh, rr: HOST arrays (of k device pointers, k doubles, k, 2 and 1 doubles). */
/* out[j] = <q, Q[j]> for j < k; nothing on the device is written */
void mg_krylovDots(int N, int k, const double *q, const double *const *Q, double *out);
/* q = q - b[j]*Q[j], z = z - b[j]*Z[j] for j = 0 .. k-1 in this order (interior; k == 0: neither is written), then
 * gh[0] = <q, q>, gh[1] = <r, q> */
void mg_krylovOrth(int N, int k, const double *b, double *q, double *z, const double *r, const double *const *Q,
                   const double *const *Z, double *gh);
/* U = U + alpha*z, r = r - alpha*q (interior; alpha == 0: neither is written), then rr[0] = <r, r> */
void mg_krylovUpdate(int N, double alpha, double *U, const double *z, double *r, const double *q, double *rr);

#ifdef __cplusplus
}
#endif
#endif /* MG_KRYLOV_H */
