/*
 * mg_eigs.h -- the lowest eigenmodes of -div(a grad u) on the vertex grid with a zero rim: multigrid-preconditioned LOBPCG
 * (the locally optimal block preconditioned conjugate-gradient method).  mg_hip.h includes this file; libmgpoisson.so
 * exports every symbol below.  This header is the specification: tests/_eigs_ref.py restates it on numpy, the kernels
 * (csrc/mg_eigs_kernels.hip) and the driver (csrc/mg_eigs.cpp) implement it.
 *
 * The problem.  Write AA for -A at shift 0, A the operator of mg_varcoef.h: AA*x = -(inv*b(x)) on the interior with the
 * expressions and rounding of that header (the launch of mg_applyOperator with the constant -inv: negation is exact) and +0
 * on the rim; no coefficient means a = 1 through the same expressions.  AA is symmetric positive definite on the interior.
 * Wanted: the k smallest lambda_i and orthonormal x_i with AA*x_i = lambda_i*x_i, x_i = 0 on the rim.  <x, y> is the sum of
 * x[q]*y[q] over the INTERIOR points q, as in mg_krylov.h.  The eigenvalues of the shifted operator are lambda + sigma with
 * the same vectors: a shift is refused here (relative gaps collapse under it and the iteration stalls) and the caller adds it.
 *
 * Why three blocks.  Each step projects onto the basis S = [X, W, P]: X the current vectors, W the preconditioned
 * residuals, P the previous search directions.  [X, W] alone is block steepest descent: on the CPU restatement it took about
 * twice the iterations on smooth coefficients and did not converge in 60 on a random one.  The block carries
 * `guard` columns beyond the k wanted ones: convergence of column i depends on the gap to the first eigenvalue OUTSIDE the
 * block, and cutting a cluster without guard columns did not reliably converge.
 *
 * The iteration (p = k + guard; S = the basis fields, AS = AA applied to them; M(r): one V(pre, post) cycle
 * vcycle(F0 = r, U0 = z) on a zeroed array z through the batch solver's cycle -- the variable-coefficient one when a
 * coefficient is set; it approximates A^-1 = -AA^-1, and the sign of a basis vector is immaterial):
 *
 *   it = 0:  S = [X];  AX = AA*X (one operator launch over the p columns)
 *   loop:
 *     G = S^T S,  H = S^T AS          (ONE Gram launch and its finish; m(m + 1) sums, m = |S| <= 3p; read back)
 *     host: the Rayleigh-Ritz step below -> C (m x p), theta (p), and Cp = C with the rows of its X block zeroed
 *     X' = S*C, AX' = AS*C, P' = S*Cp, AP' = AS*Cp, R_i = AX'_i - theta_i*X'_i, res_i^2 = <R_i, R_i>
 *                                     (ONE rotation launch and its finish, in place: a point's outputs depend on that point only)
 *     if res_i <= max(rtol*theta_i, atol) for all i < k:
 *         recompute AX = AA*X, then R and res from X, AX and theta (the operator launch and a residual-norm launch)
 *         if it still holds: converged, done
 *         else P = none for the next step (a RESTART), and go on
 *     if it == max_iters: done, not converged
 *     W_i = M(R_i), all p columns in the batched launches;  AW = AA*W (one operator launch);  ++it
 *     S = [X, W, P]   (P absent at it = 1 and after a restart)
 *
 * Soft locking.  Column i -- guard columns included -- is LOCKED after a rotation when its res_i met max(rtol*theta_i, atol)
 * and did not decrease against the rotation before (res_i >= the previous res_i), and stays locked while res_i stays inside
 * that tolerance.  The W_i and P_i of a locked column are left OUT of the next Rayleigh-Ritz step (their rows and columns of G
 * and H are struck, their rows of C and Cp are +0); X_i stays in.  W_i of a column at its rounding floor is a cycle applied to
 * noise and P_i a difference of nearly equal vectors: with them in the basis converged columns drift away again while the
 * others still converge -- on the restatement column 0 went from 4e-14 back up to 5e-5 of theta, on the device at N = 8192 no
 * step had all of k = 4 columns inside 1e-8 at once.  A column that still converges is never locked, so the iteration counts
 * of well-behaved solves are those of plain LOBPCG.  The launches are the same whatever is locked.
 *
 * The host Rayleigh-Ritz step (deterministic, cyclic Jacobi eigen-solver for matrices up to 36 x 36, no LAPACK):
 *   d_j = 1/sqrt(G_jj);   G^ = D G D,  H^ = D H D
 *   (w, V) = eig(G^);   keep w_j > MG_EIGS_DROP*max w;   T = V_keep*diag(1/sqrt(w_keep))
 *   (theta, Y) = eig(T^T H^ T) ascending;   C = D*T*Y[:, :p]
 *   fewer than p directions kept (or a G_jj that is not finite and > 0): the breakdown flag is set and the solve ends
 *
 * The rotation, per interior point: every output is the sum over j = 0 .. m-1 in this order, started from +0; each product
 * c_ji*s_j is rounded once and each sum once (no fma); R_i = AX'_i - theta_i*X'_i from the rounded X'_i, AX'_i, product
 * rounded once, difference once.  GIVEN C, Cp and theta the rotation is specified bit for bit.  The sums in G, H and res^2
 * are specified up to their summation order: within n*u/(1 - n*u) * sum|x[q]*y[q]| of the exact sum, n = (N-2)^2, u = 2^-53.
 * Every sum is a two-stage reduction over a fixed partition -- per-block partials, then a finish launch -- without
 * floating-point atomics: the same call twice gives the same bits.  G is formed for j <= l and mirrored.  H is symmetric in
 * exact arithmetic only: its upper triangle <S_j, AS_l>, j <= l, is computed and mirrored.
 *
 * The start.  With use_start the interiors of X_dev[0 .. k) are the start of the first k columns; the guard columns, and all
 * columns otherwise, are mg_fill_uniform(seed + i) minus 0.5 on the interior (column i, all N*N values drawn, the interior
 * used).  The rim of every internal field and of the k outputs is +0; the solve writes it once.  A start of fewer than p
 * independent columns has no W yet to refill the basis from: when the first Rayleigh-Ritz step keeps fewer than p directions,
 * the dependent columns -- those a Cholesky sweep over the scaled Gram matrix, in column order, leaves with a squared residual
 * <= 1e-9 -- are replaced by mg_fill_uniform(seed + t*p + j) minus 0.5 (column j, attempt t = 1 .. 3) and the step is taken
 * again; only when that does not help is it the breakdown.
 *
 * Reported values.  "Recompute" above means everything that is reported, from X alone: AX = AA*X, then
 * theta_i = <x_i, AX_i>/<x_i, x_i> (the Gram launch on [X]), then R_i = AX_i - theta_i*x_i and res_i.  lam[i] = theta_i and
 * res[i], i < k, are always these recomputed values, never the Rayleigh-Ritz step's own: on max_iters or a breakdown the
 * recomputation is done once more for the report.  X_dev[i] receive the vectors.  A start that already is a solution -- with
 * use_start, the k start columns orthonormal within 4*n*u/(1 - n*u), n = (N-2)^2, and the residuals of their Rayleigh
 * quotients inside the tolerance, found by these same launches before the first Rayleigh-Ritz step -- is returned untouched
 * in 0 iterations, with the lam and res bits of the solve that produced it and X bit for bit what was passed (rim +0).  The
 * check looks at nothing else: ANY k orthonormal start columns whose Rayleigh-quotient residuals are inside the tolerance are
 * accepted as they stand -- eigenvectors that are not the lowest ones, or not in ascending order, included; it is the
 * caller's statement that these are the wanted modes.  No launch of a solve depends on k or p beyond
 * the instance dimension of the batched launches and uniform loop bounds.
 *
 * Memory.  create allocates everything, a solve allocates nothing: S and AS are 6p fields (R lives in AW's fields, which are
 * dead between the rotation and the next operator launch), the internal batch solver for p instances holds about 2p more
 * (the level-0 twin B, the coarse levels) and 4/3 of a field for a coefficient, and the Gram partials are
 * 72*21*ceil(N/256)*ceil(N/16) doubles at p = 12.  At p = 12 and N = 8192: 72 fields of 0.537 GB = 38.7 GB for S and AS,
 * 12.9 GB for the cycle, 0.2 GB of partials -- about 52 GB.
 *
 * Memory contract (mg_hip.h): the new kernels never write a rim, and never read one into a result.  A solve reads the
 * interiors of X_dev[0 .. k) (use_start) and writes all of X_dev[0 .. k).  The test hooks below read the arrays named as
 * read and write the arrays named as written, interior only (tests/test_eigs_gpu.py holds them inside guard bands).  Device
 * arrays are 16-byte aligned.
 */
#ifndef MG_EIGS_H
#define MG_EIGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_EIGS_MAX_BLOCK 12          /* p = k + guard */
#define MG_EIGS_DROP      1e-12       /* relative eigenvalue of the scaled Gram matrix below which a direction is dropped */

/* cycle supplies pre, post, omega, N_min and the coarse targets of the preconditioner.  Its rtol, atol and max_cycles are
 * IGNORED (the preconditioner is always exactly one cycle); its shift and fmg must be 0. */
typedef struct mg_eigs_opts {
    mg_solve_opts cycle;
    int    k, guard;           /* wanted pairs, guard columns; p = k + guard <= MG_EIGS_MAX_BLOCK */
    int    max_iters;          /* >= 0 */
    double rtol, atol;         /* column i is done when res_i <= max(rtol*theta_i, atol) */
} mg_eigs_opts;

typedef struct mg_eigs_result {
    int status;                /* 0 converged, MG_SOLVE_NOT_CONVERGED (-1), or an error code (> 0, mg_last_error) */
    int iters;                 /* Rayleigh-Ritz steps after the first (it above) */
    int converged;
    int breakdown;             /* the Rayleigh-Ritz step kept fewer than p directions */
    int restarts;
    int cycles;                /* preconditioner applications: p*iters */
    int coarse_capped;         /* 1 when some coarse solve of a preconditioner stopped at coarse_max_iters above its target */
} mg_eigs_result;

typedef struct mg_eigs mg_eigs;

/* V(3,3), omega 0.8, N_min 8 and the coarse targets of mg_solve_opts_default; k 1, guard 0, rtol 1e-8, atol 0, 60 iterations */
void mg_eigs_opts_default(mg_eigs_opts *o);
/* NULL opts: the defaults.  NULL on bad arguments (mg_last_error).  Refused with MG_ERR_ARG, never ignored: cycle.shift != 0,
 * cycle.fmg != 0, k < 1, guard < 0, k + guard > MG_EIGS_MAX_BLOCK, 3(k + guard) > (N-2)^2, max_iters < 0, a negative or
 * non-finite rtol or atol, a hierarchy of one level (N < 2*N_min), and whatever mg_batch_solver_create refuses in cycle. */
mg_eigs *mg_eigs_create(int N, double L, const mg_eigs_opts *o);
/* a_dev: N x N nodal coefficient shared by all columns; NULL: back to a = 1.  The checks, codes and texts of
 * mg_batch_solver_set_coefficient (mg_varcoef_batch.h) pass through; a refused coefficient leaves the earlier one. */
int  mg_eigs_set_coefficient(mg_eigs *e, const double *a_dev);
/* X_dev: host array of k device pointers to N x N arrays (16-byte aligned, no two overlapping); lam, res: k host doubles.
 * Returns out->status.  Works on the engine stream and is synchronous. */
int  mg_eigs_solve(mg_eigs *e, double *const *X_dev, int use_start, uint64_t seed, double *lam, double *res, mg_eigs_result *out);
/* the records of the last solve, one per Rayleigh-Ritz step (step 0 included), 2k + 2 doubles each:
 *     theta_0 .. theta_{k-1},  res_0 .. res_{k-1} (the rotation's),  directions kept,  restarted (0 or 1)
 * out == NULL: returns the number of records; otherwise copies at most cap records and returns how many. */
int  mg_eigs_history(const mg_eigs *e, double *out, int cap);
void mg_eigs_destroy(mg_eigs *e);

/* TEST HOOKS, not part of the feature's interface: each kernel on caller arrays (synchronous, engine stream), exported so
 * that tests/test_eigs_gpu.py can hold each kernel against numpy alone.  They may change with the kernels.  N >= 3. */
/* G[j*m + l] = <S[j], S[l]>, H[j*m + l] = <S[j], AS[l]> for j <= l, both mirrored; 1 <= m <= 3*MG_EIGS_MAX_BLOCK; S, AS: HOST
 * arrays of m device pointers; G, H: HOST arrays of m*m doubles; nothing on the device is written.  Returns 0 or an error code. */
int  mg_eigsGram(int N, int m, const double *const *S, const double *const *AS, double *G, double *H);
/* The rotation above, in place.  1 <= p <= MG_EIGS_MAX_BLOCK, p <= m <= 3p.  S, AS: HOST arrays of 3p device pointers each, of
 * which the first m are read; written: S[i] = X'_i, AS[i] = AX'_i, S[2p + i] = P'_i, AS[2p + i] = AP'_i, R[i] = R_i (R: HOST
 * array of p device pointers, which may be fields of AS[p .. 2p)), interior only.  C, Cp: HOST arrays, m x p row-major
 * (C[j*p + i]); theta: p doubles; res2 (HOST, p doubles) = <R_i, R_i>.  Returns 0 or an error code. */
int  mg_eigsRotate(int N, int m, int p, const double *C, const double *Cp, const double *theta, double *const *S,
                   double *const *AS, double *const *R, double *res2);
/* the host Rayleigh-Ritz step above on G, H (m x m row-major): C, Cp (m x p row-major) and theta (p); returns the number of
 * directions kept, and leaves C, Cp, theta untouched when that is below p (the breakdown) */
int  mg_eigsRayleighRitz(int m, int p, const double *G, const double *H, double *C, double *Cp, double *theta);

#ifdef __cplusplus
}
#endif
#endif /* MG_EIGS_H */
