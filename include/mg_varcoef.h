/*
 * mg_varcoef.h -- the residual-tolerance solver (mg_hip.h: mg_solver_*) with a variable coefficient:
 *     div(a grad U) - sigma*U = F     on the solver's N x N vertex grid, Dirichlet values on the rim of U,
 * sigma = mg_solve_opts.shift (>= 0), a an N x N fp64 device array given AT THE GRID POINTS, rim included, every value
 * finite and > 0.  mg_hip.h includes this file; libmgpoisson.so exports every symbol below.  This header is the
 * specification: tests/_solve_vc_ref.py restates it on numpy, the kernels (csrc/mg_varcoef_kernels.hip) implement it.
 *
 * The cycle is the V(pre, post) cycle of mg_solver_solve, operator by operator (one launch per sweep), with the same node
 * order, transfer operators of U and D, tolerances, results and read-backs.  What changes is the operator.  Per level l
 * the constants of the solver are used unchanged -- dx2 = (L/(N_l-1))^2, inv = 1/dx2, sd = shift*dx2, omega -- and, per
 * interior point p of a level with nodal coefficient a (row-major, p+N: row r+1, p-N: row r-1, p+1 / p-1: columns c+1 /
 * c-1), every product and every sum rounded once (no fma):
 *   face coefficients   aN = 0.5*(a[p] + a[p+N]),  aS = 0.5*(a[p] + a[p-N]),  aE = 0.5*(a[p] + a[p+1]),  aW = 0.5*(a[p] + a[p-1])
 *   centre              d = (((aN + aS) + aE) + aW) + sd,   q = 1/d (IEEE division),   c = omega*q
 *   bracket             b(U) = (((aN*U[p+N] + aS*U[p-N]) + aE*U[p+1]) + aW*U[p-1]) - d*U[p]
 *   sweep               U <- U + c*(b(U) - dx2*F);  from the zero field it is 0.0 + c*(0.0 - dx2*F).  Rim points keep their
 *                       value (zero start: +0).
 *   residual            inv*b(U) - F on the interior, +0 on the rim: the restricted quantity and the stopping norm.  The
 *                       cycle restricts its negative; the sign flip (sign < 0) negates the whole array, rim included (-0
 *                       there), as the constant-coefficient kernels do.
 *   coarse update       red-black Gauss-Seidel from zero, colour 0 = (row + col) even first, then colour 1:
 *                       U[p] = q*((((aW*U[p-1] + aE*U[p+1]) + aN*U[p+N]) + aS*U[p-N]) - dx2*F[p])
 *   coarse stop         error metric sum|inv*b(U) - F| / (N-2)^2 after every iteration, err0 = sum|F| / (N-2)^2; target
 *                       max(coarse_atol, coarse_rtol*err0), at least one iteration, at most coarse_max_iters; state[] as in
 *                       mg_solver_solve.
 * The norms are sums of squares over the interior in the partition and order of the constant-coefficient norm of the same N.
 *
 * Coarse levels are rediscretised from a coarsened NODAL coefficient a_{l+1}, sampled from a_l with the table (lo, w) =
 * mg_restriction_table(N_l, N_{l+1}) on both axes: an interior coarse index takes the table's (lo, w); index 0 takes
 * (0, 0.0); index M-1 takes (N-2, 1.0) -- the end points of the two grids coincide, and the table's own entry there may step
 * out of bounds.  With a = w[col], b = 1.0 - a, c = w[row], d = 1.0 - c and f = lo[col] + lo[row]*N, EVERY coarse point,
 * rim included, is
 *     v = b*d*A[f] + a*d*A[f+1] + c*b*A[f+N] + a*c*A[f+N+1]            (doRestriction's expression and order)
 *     a_c = min(max(v, m), M),  m / M = the smallest / largest of the four samples A[f], A[f+1], A[f+N], A[f+N+1].
 * In exact arithmetic v is a convex combination of the four samples and the clamp does nothing; in fp64 the four rounded
 * weights need not sum to 1 (they miss it by an ulp at about one point in ten), and the clamp puts v back where the exact
 * value lies.  So positivity and the bounds of a carry to every level exactly, a constant coefficient stays that constant
 * on every level, and the host checks level 0 only: the coarse levels are not re-checked.
 *
 * Consequence (tests/test_solve_vc_cpu.py, tests/test_solve_vc_gpu.py): with a == 1.0 everywhere every face coefficient on
 * every level is exactly 1, d, q and c are the host constants of the constant-coefficient solver (d = 4 + sd, q = 1/d,
 * c = omega*q; a centre of 4.0 at sigma = 0 gives the unshifted bits), every product aX*U is U, and the solve returns the
 * same U, history, cycles and flags as the same solver without a coefficient, bit for bit.
 *
 * Memory contract (mg_hip.h): every function below reads its const arrays and writes its output array and nothing else
 * (tests/test_solve_vc_gpu.py holds them inside guard bands).  Device arrays are 16-byte aligned.
 */
#ifndef MG_VARCOEF_H
#define MG_VARCOEF_H

#ifdef __cplusplus
extern "C" {
#endif

/* Give the solver the coefficient a (N x N device array), or take it away again (a_dev == NULL: back to the constant-
 * coefficient solver, which then enqueues exactly what it always enqueued).  The array is checked on the device (every value
 * finite and > 0: one reduction launch, a flag, one read-back), copied into level-0 storage of the solver's own and
 * coarsened to every level; the caller's array is not kept and may be freed after the call.  Works on the engine stream
 * (mg_set_stream) and returns when the coefficient is in place.  The level storage (about 4/3 N^2 doubles) is allocated by
 * the first call and reused by later ones.  With a coefficient set, mg_solver_solve runs the variable-coefficient cycle
 * operator by operator whatever mg_set_smoother says.
 * Returns 0, or (mg_last_error; the solver keeps the state it had, coefficient included, and stays usable):
 *   MG_ERR_ARG (2)          NULL solver, a_dev not 16-byte aligned, or a value of a that is not finite or not > 0
 *   MG_ERR_UNSUPPORTED (3)  the solver was created with fmg != 0: the full-multigrid pass is not built for a coefficient
 *                           yet, and an option is never silently ignored */
int  mg_solver_set_coefficient(mg_solver *s, const double *a_dev);
/* A HIP error (1) before the check has passed leaves the state as it was too; one after it, while the level
 * storage is being rewritten, leaves the solver WITHOUT a coefficient (mg_solver_has_coefficient: 0). */
/* 1 when a coefficient is set, else 0 (NULL: 0) */
int  mg_solver_has_coefficient(const mg_solver *s);

/* the building blocks on their own (synchronous, engine stream), N >= 3, spacing L/(N-1), sd = shift*dx2 as above.  No
 * output overlaps an input; a NULL array where none is allowed is refused with MG_ERR_ARG. */
/* out = inv*b(U) on the interior, +0 on the rim; a_dev == NULL: a = 1 everywhere (the constant operator through the same
 * expressions) */
void mg_applyOperator(int N, double L, double shift, const double *a_dev, const double *U, double *out);
/* a_c (M x M) = a_f (N x N) coarsened as above, 2 <= M, the restriction table N -> M must stay inside the fine grid */
void mg_coarsenCoefficient(int N, const double *a_f, int M, double *a_c);
/* TEST HOOKS, not part of the feature's interface: the sweep and the signed residual of the cycle on their own, exported so
 * that tests/test_solve_vc_gpu.py can hold each kernel against the restatement alone.  They may change with the kernels. */
/* one sweep: U_out = U_in + c*(b(U_in) - dx2*F), rim copied; U_in == NULL: the sweep from the zero field (rim +0) */
void mg_sweepCoefficient(int N, double L, double shift, double omega, const double *a_dev, const double *U_in, const double *F,
                         double *U_out);
/* D = inv*b(U) - F on the interior, +0 on the rim; sign < 0: the whole array negated */
void mg_residualCoefficient(int N, double L, double shift, const double *a_dev, const double *U, const double *F, double *D,
                            int sign);

#ifdef __cplusplus
}
#endif
#endif /* MG_VARCOEF_H */
