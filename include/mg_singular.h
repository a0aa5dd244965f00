/*
 * mg_singular.h -- the pure Neumann problem in the residual-tolerance solver (mg_hip.h: mg_solver_*):
 *     div(a grad U) = F     on the solver's N x N vertex grid, all four sides Neumann, sigma = 0.
 * mg_hip.h includes this file after mg_bc.h (through the last line of mg_bc.h); libmgpoisson.so exports every symbol below.
 * This header is the specification: tests/_singular_ref.py restates it on numpy, the kernels (csrc/mg_singular_kernels.hip,
 * point code in csrc/mg_singular_impl.h, the coarse solve beside k_gs_relative_bc in csrc/mg_bc_kernels.hip) implement it.
 *
 * The singular operator.  With four Neumann sides every grid point is an unknown, and at shift == 0 the operator A of mg_bc.h
 * has the constants as its null space.  Let
 *     w[r][c] = wr[r]*wc[c],   wr = wc = 0.5 at index 0 and N-1, 1.0 elsewhere          (the trapezoid weights)
 * Then diag(w)*A is symmetric with vanishing column sums (tests/test_bc_forms_cpu.py): w is the left null vector, A U = F
 * has a solution exactly when sum(w*F) == 0, and the solution is fixed up to a constant.  The weighted mean is
 *     mean_w(X) = (sum over all N^2 points of w*X) / sw,   sw = (double)(N-1)*(double)(N-1)  (= sum of w, exact).
 *
 * Summation order of mean_w (bit-reproducible from run to run; the products w*X are exact, w being 1, 1/2 or 1/4).
 *   partition  the blocks of the norms of the same N, resnorm_partials(N) of them: 256 lanes by 4 rows.  Block (bx, by)
 *              covers the rows 4*by .. 4*by+3 and
 *                one-column form (odd N, or N < 512):  lane t has column c = 256*bx + t
 *                column-pair form (even N >= 512):     lane t has the columns c = 2*(256*bx + t) and c + 1
 *              The form follows from N alone, by the rule of every streaming kernel of the solver.
 *   lane       acc = 0.0; for its rows r in increasing order (r < N): acc = acc + w[r][c]*X[r][c], in the pair form then
 *              acc = acc + w[r][c+1]*X[r][c+1].  A lane whose column lies beyond the grid keeps 0.0.
 *   wave       64 consecutive lanes: for o = 32, 16, 8, 4, 2, 1:  v[i] = v[i] + v[i+o]  (i < o); the wave's sum is v[0].
 *   block      s = 0.0; for the block's waves in order: s = s + (wave's sum).  partial[by*gx + bx] = s (gx blocks per row
 *              of blocks).
 *   finish     ONE block of 1024 lanes: lane t: acc = 0.0; for i = t, t + 1024, ... < resnorm_partials(N): acc = acc +
 *              partial[i]; then the wave and the block step above over its 16 waves; mean_w = s / sw.
 * The finish launch leaves {mean_w, mean_w - target} in device memory; nothing is read back to form the constant.
 *
 * Shift.  X_out[p] = X_in[p] - c at every point, c = mean_w - target as the finish launch left it (one rounding per point).
 *
 * Opt-in.  mg_solver_set_boundary with four Neumann sides at shift == 0 is refused (mg_bc.h) unless mg_solver_set_mean has
 * switched the mean fixing on.  While the operator is not singular -- any Dirichlet side, or shift != 0 -- the setting is
 * dormant: the solver enqueues exactly what it enqueues without it.
 *
 * A singular solve mg_solver_solve(s, F, U, res):
 *   1. c_F = mean_w(F); Ft = F - c_F at every point, into a solver-owned N^2 buffer (allocated when the first singular
 *      boundary is set, not before).  F is read only and is ALWAYS projected, however small c_F.  ref_norm, res0, res, the
 *      history and the stopping rule are those of the boundary path (mg_bc.h) on Ft.
 *   2. The cycles of the boundary path run on Ft: the same recorded cycle, launches, sweeps, residuals and transfers.  Only
 *      the coarse solve differs.  With M the coarsest size and Fc its right-hand side, it first forms
 *          m_c = (sum of wM*Fc) / ((double)(M-1)*(double)(M-1)),   wM the weights of the M x M grid,
 *      in this order: the one workgroup has T = min(1024, 64*ceil(M^2/64)) lanes; lane t: acc = 0.0; for j = 0 .. 3, p = t +
 *      j*T < M^2 (p = r*M + c): acc = acc + wM[r][c]*Fc[p]; then the wave and the block step above over its T/64 waves.
 *      Fc[p] - m_c replaces Fc[p] at every point (inside the workgroup: the array in memory is not written), and err0, the
 *      target and the red-black iteration of mg_bc.h work on the projected values.  Nothing is projected on the levels in
 *      between, and U is not touched between cycles.
 *   3. After the last cycle -- also when no cycle ran -- U <- U - (mean_w(U) - mean) at every point, in place, enqueued on the
 *      stream; the constant is not read back to form it.  mean is the target of mg_solver_set_mean.
 * mg_solver_singular_info gives c_F, mean_w(U) before step 3 and the target; they travel with the solve's own last wait.
 *
 * Memory contract (mg_hip.h): every function below reads its const arrays and writes its output array and nothing else.
 * Device arrays are 16-byte aligned, N >= 3.  X_out of mg_projectMean may be X_in itself; no other output overlaps an input.
 *
 * Not built: batched singular solves, the Krylov acceleration, the full-multigrid start and the adjoint with boundary kinds
 * (refused as mg_bc.h says), null spaces other than the constants, projection on the levels in between.
 */
#ifndef MG_SINGULAR_H
#define MG_SINGULAR_H

#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: fix the weighted mean of the solution of a singular solve at `mean` (finite) and accept four Neumann sides at
 * shift == 0 in mg_solver_set_boundary; on == 0: off (mean is ignored).  Returns 0, or (mg_last_error; the solver keeps the
 * state it had and stays usable):
 *   MG_ERR_ARG (2)          NULL solver, or a mean that is not finite
 *   MG_ERR_UNSUPPORTED (3)  on == 0 while four Neumann sides at shift == 0 are set (the singular problem needs it) */
int  mg_solver_set_mean(mg_solver *s, int on, double mean);
/* mean_out (may be NULL) = the target; returns 1 when the mean fixing is on, else 0 (NULL solver: 0) */
int  mg_solver_mean(const mg_solver *s, double *mean_out);
/* out[0] = c_F, the weighted mean the caller's F had (its compatibility defect), out[1] = mean_w(U) before the final shift,
 * out[2] = the target, all of the last singular solve; three zeros when the last solve was not singular */
void mg_solver_singular_info(const mg_solver *s, double *out);

/* the building blocks on their own (synchronous, engine stream) */
/* *out_host = mean_w(X) */
void mg_weightedMean(int N, const double *X_dev, double *out_host);
/* X_out = X_in - (mean_w(X_in) - mean); *removed_host (may be NULL) = mean_w(X_in).  X_out may be X_in. */
void mg_projectMean(int N, const double *X_in, double mean, double *X_out, double *removed_host);

/* TEST HOOK, not part of the feature's interface: it may change with the kernels. */
/* the projected coarse solve alone: U_out = the red-black solve from zero of the M = N problem on F - m_c, N <= 63, kind
 * four Neumann sides (anything else: MG_ERR_ARG), a_dev may be NULL (a = 1); *removed_host (may be NULL) = m_c.  The
 * iteration count is mg_lastExactSolverIterations(). */
void mg_coarseSolveMean(int N, double L, const int *kind, const double *a_dev, const double *F, double atol, double rtol,
                        int max_iters, double *U_out, double *removed_host);

#ifdef __cplusplus
}
#endif
#endif /* MG_SINGULAR_H */
