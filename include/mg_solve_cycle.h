/* mg_solve_cycle.h -- the recorded V(pre, post) cycle of the residual-tolerance solvers (mg_solver, mg_batch_solver), as a
 * list of its launches.  Host only; included by mg_hip.h. */
#ifndef MG_SOLVE_CYCLE_H
#define MG_SOLVE_CYCLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* The launches of one V(pre, post) cycle over nl levels from level `top`, in order, as both solvers walk them (host only, needs
 * no mg_init; for tests).  fused != 0: the cycle of the streaming smoother's fused nodes, whose restriction (down_fused[l]) and
 * prolongation-add (up_fused[l]), l < nl - 1, ride inside the node or run beside it; else operator by operator, with_coef != 0
 * naming the level's coefficient in the `coarse` role of sweeps, residuals and the coarse solve.  One record of
 * MG_SOLVE_CYCLE_RECORD ints per step: kind (0 node, 1 sweep, 2 residual, 3 restriction, 4 coarse solve, 5 prolongation-add,
 * 6 copy), level, sweeps and d_sign (nodes), fused_transfer, the (field, level) pairs of the roles in, F, coarse, out, Fc
 * (field: 0 none, 1 U0, 2 F0, 3 A, 4 B, 5 F, 6 coefficient), and the table slot of the batched solver (from 1; steps share
 * one exactly when their five roles are equal).  Returns the number of steps (at most cap records are written; out may be
 * NULL), -1 on bad arguments. */
#define MG_SOLVE_CYCLE_RECORD 16
int  mg_solve_cycle_describe(int nl, int pre, int post, int top, int fused, const int *down_fused, const int *up_fused,
                             int with_coef, int *out, int cap);

#ifdef __cplusplus
}
#endif

#endif
