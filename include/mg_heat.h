/*
 * mg_heat.h -- time stepping of the heat equation  u_t = nu*Laplace(u) + q  on the N x N grid of the residual-tolerance
 * solvers (mg_hip.h: spacing L/(N-1), Dirichlet values on the rim of U) with the theta-scheme: the right-hand-side kernel on
 * its own and a stepper that runs {right-hand side, solve} per step on the device.  mg_hip.h includes this file;
 * libmgpoisson.so exports every symbol below.
 *
 * The scheme, theta in [1/2, 1] (1: backward Euler, 1/2: Crank-Nicolson), q optional and constant over a call:
 *   (u+ - u)/dt = nu*(theta*Lap_h u+ + (1 - theta)*Lap_h u) + q
 *   <=>  Lap_h u+ - sigma*u+ = F,   sigma = 1/(theta*nu*dt),   F = -sigma*u - ((1 - theta)/theta)*Lap_h u - q/(theta*nu)
 * which is the screened equation of mg_solve_opts.shift with shift = sigma.  Evaluation order, every product and every sum
 * rounded once (no fma):
 *   host constants, fp64:  a = theta*nu,  sigma = 1.0/(a*dt),  beta = (1.0 - theta)/theta,  gamma = 1.0/a,
 *                          dx2 = (L/(N-1))^2,  inv = 1/dx2   (dx2, inv: the level-0 constants of the solvers)
 *   interior point (r, c): s = -(sigma*u)
 *     theta != 1:          lap = inv*((((u[r+1] + u[r-1]) + u[c+1]) + u[c-1]) - 4*u),   s = s - beta*lap
 *                          (the bracket order of b(U) in mg_hip.h; with theta exactly 1 the term is left out, not multiplied
 *                          by zero, and no neighbour is read)
 *     q given:             s = s - gamma*q
 *     F = s;  every rim point of F is written as +0.0 (the solvers ignore the rim of F).
 * Memory contract (mg_hip.h): mg_heat_rhs reads U and Q and writes F and nothing else; mg_heat_stepper_step reads Q, works
 * on U in place and writes nothing else of the caller's (tests/test_heat_gpu.py holds the kernel inside guard bands).
 */
#ifndef MG_HEAT_H
#define MG_HEAT_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_heat_opts {
    double nu, dt, theta;      /* diffusivity > 0, time step > 0, theta in [0.5, 1] */
    mg_solve_opts solve;       /* the options of the solve of every step; shift must stay 0: the stepper sets it to sigma */
} mg_heat_opts;

/* nu 1, dt 1, theta 1, solve = mg_solve_opts_default */
void mg_heat_opts_default(mg_heat_opts *o);

/* the building block on its own (synchronous, engine stream): F = rhs(U, Q) as defined above; Q may be NULL (no source).
 * U, Q, F: N x N device arrays, 16-byte aligned, N >= 3; F overlaps neither U nor Q.  Reads U and Q, writes F only. */
void mg_heat_rhs(int N, double L, double nu, double dt, double theta, const double *U, const double *Q, double *F);

typedef struct mg_heat_result {
    int    status;             /* MG_SOLVE_CONVERGED / MG_SOLVE_NOT_CONVERGED / error code > 0 */
    int    steps;              /* time steps completed (all instances advance together) */
    int    cycles;             /* V-cycles of this instance, summed over the steps */
    int    coarse_capped;      /* 1 when some coarse solve of this instance stopped at coarse_max_iters */
    double res, ref_norm;      /* of this instance's last solve */
    double device_ms;          /* hipEvent time of the whole call */
    int    n_steps;            /* entries of cycles_per_step (= steps) */
    const int *cycles_per_step;   /* owned by the stepper, valid until its next call */
} mg_heat_result;

typedef struct mg_heat_stepper mg_heat_stepper;

/* The stepper owns max_batch right-hand-side arrays (at the batch solver's 256-byte instance pitch), the tables of the
 * batched right-hand-side launch and one inner solver created with solve.shift = sigma: an mg_solver when max_batch == 1
 * (solve.fmg works as documented there), an mg_batch_solver otherwise (whose refusal of fmg != 0 is passed through).
 * NULL opts: the defaults.  Refused with MG_ERR_ARG (NULL returned, the engine stays usable): nu or dt not finite or not
 * positive, theta outside [0.5, 1], solve.shift != 0 (an option is never silently overridden), max_batch < 1, and whatever
 * the inner solver refuses. */
mg_heat_stepper *mg_heat_stepper_create(int N, double L, int max_batch, const mg_heat_opts *o);

/* `steps` time steps of the n fields U_dev[0..n) in lockstep, on the engine stream.  One step is ONE right-hand-side launch
 * over the n instances (F_i = rhs(U_i, Q_i)), then the inner solve started from U_i itself: its interior is u_old, the warm
 * start, its rim the Dirichlet data.  The rim of U is never written by the right-hand-side kernel; what the solve does to it
 * is the solver's documented behaviour.  k steps give, bit for bit, k times {mg_heat_rhs, mg_solver_solve with shift =
 * mg_heat_stepper_sigma} on each instance, whatever the others are.  Q_dev: NULL (no source), or n device pointers of which
 * any may be NULL and any may repeat.  If an instance ends a step not converged, that step still finishes for every instance
 * and the call stops there with MG_SOLVE_NOT_CONVERGED; out[i].steps tells the steps done.  A time-dependent source is
 * the caller's loop of steps = 1 calls.  A time-dependent rim written into U before each such call is exact only for
 * theta = 1, whose right-hand side reads no neighbour: for theta < 1 the right-hand side takes Lap_h of u_old next to the rim,
 * and a rim already at the new time puts two time levels into it (an error of first order in the rim's change, not the
 * theta-scheme).  There the caller runs mg_heat_rhs on the old field with its old rim, then sets the new rim, then solves
 * with mg_solver_solve at shift = mg_heat_stepper_sigma (tests/test_exact_gpu.py, test_heat_moving_rim).  Allocates nothing on the device.  Refused with MG_ERR_ARG before anything is
 * enqueued: steps < 1, n outside [1, max_batch], a NULL or not 16-byte aligned U (or non-NULL Q), a U that overlaps another
 * U or a Q.  out: n results.  Returns MG_SOLVE_CONVERGED, MG_SOLVE_NOT_CONVERGED or an error code (> 0). */
int  mg_heat_stepper_step(mg_heat_stepper *s, int n, double *const *U_dev, const double *const *Q_dev, int steps,
                          mg_heat_result *out);
/* the shift of the inner solver: sigma = 1.0/((theta*nu)*dt) */
double mg_heat_stepper_sigma(const mg_heat_stepper *s);
void mg_heat_stepper_destroy(mg_heat_stepper *s);

#ifdef __cplusplus
}
#endif
#endif /* MG_HEAT_H */
