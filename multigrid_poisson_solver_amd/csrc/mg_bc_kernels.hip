// mg_bc_kernels.hip -- fp64 kernels of the residual-tolerance solver with boundary kinds per side (include/mg_bc.h; driven by
// mg_solve.cpp: SolveOperator's members, and by mg_heat.cpp): the weighted Jacobi sweep, the residual, the operator on its own, the
// norms over the unknowns, the heat right-hand side, the red-black coarse solve, the transfers with rim and the flux source.
// Built with -ffp-contract=off like every kernel file.  The shapes are mg_varcoef_kernels.hip's: a lane walks 4 rows down its
// column (any N) or its column pair (even N from PAIR_MIN_N on, 16-byte accesses) with a rolling window of three rows of U and
// of a in registers; from NT_MIN_N on F comes in and the output leaves non-temporally, the pair residual at every size.  A
// mirrored ghost row re-reads a row the block streams anyway, so the traffic per point is the `_vc` kernels'.  The point code
// lives in mg_bc_impl.h, over mg_varcoef_impl.h.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_bc_impl.h"

namespace mg {
namespace k {

namespace {

// FORM 0: one column per lane; 1: column pairs; 2: column pairs, non-temporal
template <BcOp OP, bool HAS_A, int FORM>
__global__ __launch_bounds__(TB) void k_bc(BcArgs b)
{
    if constexpr (FORM == 0) bc_cols<OP, HAS_A>(b);
    else bc_pairs<OP, HAS_A, FORM == 2>(b);
}

__global__ __launch_bounds__(1024) void k_resnorm_finish_bc(const double *__restrict__ part, size_t n, double *__restrict__ out)
{
    resnorm_finish_body(part, n, out);
}

__global__ __launch_bounds__(1024) void k_gs_relative_bc(int N, BcGeom g, double h2, double inv, double sd,
                                                         const double *__restrict__ Ag, double *__restrict__ Ug,
                                                         const double *__restrict__ Fg, double atol, double rtol, int max_iters,
                                                         int *__restrict__ state, double *__restrict__ err_out)
{
    gs_relative_bc_body<false>(N, g, h2, inv, sd, Ag, Ug, Fg, atol, rtol, max_iters, state, err_out);
}

// its twin for the singular problem (include/mg_singular.h): the right-hand side loses its weighted mean first
__global__ __launch_bounds__(1024) void k_gs_relative_bc_mean(int N, BcGeom g, double h2, double inv, double sd,
                                                              const double *__restrict__ Ag, double *__restrict__ Ug,
                                                              const double *__restrict__ Fg, double atol, double rtol, int max_iters,
                                                              int *__restrict__ state, double *__restrict__ err_out,
                                                              double *__restrict__ mean_out)
{
    gs_relative_bc_body<true>(N, g, h2, inv, sd, Ag, Ug, Fg, atol, rtol, max_iters, state, err_out, mean_out);
}

__global__ __launch_bounds__(TB) void k_restrict_bc(int N, const double *__restrict__ D, int M, BcGeom g, double *__restrict__ Fc,
                                                    const int *__restrict__ lo, const double *__restrict__ w)
{
    restrict_bc_body(N, D, M, g, Fc, lo, w);
}

__global__ __launch_bounds__(TB) void k_prolong_add_bc(int M, const double *__restrict__ Uc, int N, BcGeom g,
                                                       const double *__restrict__ Uin, double *__restrict__ Uout,
                                                       const int *__restrict__ lo, const double *__restrict__ w)
{
    prolong_add_bc_body(M, Uc, N, g, Uin, Uout, lo, w);
}

__global__ __launch_bounds__(TB) void k_neumann_source(int N, double t, int kS, int kN, int kW, int kE, BcGeom g,
                                                       const double *__restrict__ A, const double *__restrict__ F,
                                                       const double *__restrict__ G, double *__restrict__ Fout)
{
    neumann_source_body(N, t, kS, kN, kW, kE, g, A, F, G, Fout);
}

// the form of a launch by the `_vc` launchers' rule: pairs for even N from PAIR_MIN_N on, non-temporal from NT_MIN_N on
// (always_nt: the residual, whose pair form is non-temporal at every size)
template <BcOp OP>
void launch(hipStream_t s, const BcArgs &b, bool always_nt = false)
{
    const int N = b.k.N;
    const bool has_a = b.k.A != nullptr;
    const dim3 blk(TB);
    if (!use_pairs(N)) {
        if (has_a) hipLaunchKernelGGL((k_bc<OP, true, 0>), grid_rows(N), blk, 0, s, b);
        else hipLaunchKernelGGL((k_bc<OP, false, 0>), grid_rows(N), blk, 0, s, b);
    } else if (always_nt || N >= NT_MIN_N) {
        if (has_a) hipLaunchKernelGGL((k_bc<OP, true, 2>), grid_pairs(N), blk, 0, s, b);
        else hipLaunchKernelGGL((k_bc<OP, false, 2>), grid_pairs(N), blk, 0, s, b);
    } else if constexpr (OP != BC_RESIDUAL) {
        if (has_a) hipLaunchKernelGGL((k_bc<OP, true, 1>), grid_pairs(N), blk, 0, s, b);
        else hipLaunchKernelGGL((k_bc<OP, false, 1>), grid_pairs(N), blk, 0, s, b);
    }
}

}  // namespace

// ------------------------------------------------------------------ launchers
void wjacobi_bc(hipStream_t s, int N, double dx2, double sd, double omega, const int *kind, const double *A, const double *in,
                const double *F, double *out)
{
    const BcArgs b{VcArgs{N, dx2, 0.0, sd, omega, A, in, F, out, +1}, bc_geom(N, kind), 0.0, 0.0, 0.0};
    if (in) launch<BC_SWEEP>(s, b);
    else launch<BC_SWEEP_ZERO>(s, b);
}

void residual_bc(hipStream_t s, int N, double inv, double sd, const int *kind, const double *A, const double *U, const double *F,
                 double *D, int sign)
{
    const BcArgs b{VcArgs{N, 0.0, inv, sd, 0.0, A, U, F, D, sign}, bc_geom(N, kind), 0.0, 0.0, 0.0};
    launch<BC_RESIDUAL>(s, b, true);
}

void apply_bc(hipStream_t s, int N, double inv, double sd, const int *kind, const double *A, const double *U, double *out)
{
    const BcArgs b{VcArgs{N, 0.0, inv, sd, 0.0, A, U, nullptr, out, +1}, bc_geom(N, kind), 0.0, 0.0, 0.0};
    launch<BC_APPLY>(s, b);
}

void resnorm_bc(hipStream_t s, int N, double inv, double sd, const int *kind, const double *A, const double *U, const double *F,
                double *part, double *out)
{
    const size_t np = resnorm_partials(N);   // (the same partition as the constant norm)
    const BcArgs b{VcArgs{N, 0.0, inv, sd, 0.0, U ? A : nullptr, U, F, part, +1}, bc_geom(N, kind), 0.0, 0.0, 0.0};
    if (U) launch<BC_NORM>(s, b);
    else launch<BC_NORM_F>(s, b);
    hipLaunchKernelGGL(k_resnorm_finish_bc, dim3(1), dim3(1024), 0, s, part, np, out);
}

void heat_rhs_bc(hipStream_t s, int N, const HeatConsts &c, const int *kind, const double *A, const double *U, const double *Q,
                 double *F)
{
    // (theta == 1 reads no coefficient: one instantiation serves with and without)
    const BcArgs b{VcArgs{N, 0.0, c.inv, 0.0, 0.0, c.lap ? A : nullptr, U, Q, F, +1}, bc_geom(N, kind), c.sigma, c.beta, c.gamma};
    if (c.lap) launch<BC_HEAT>(s, b);
    else launch<BC_HEAT_LOCAL>(s, b);
}

void gauss_seidel_relative_bc(hipStream_t s, int N, double h2, double inv, double sd, const int *kind, const double *A, double *U,
                              const double *F, double atol, double rtol, int max_iters, int *state, double *err_out)
{
    const size_t n = (size_t)N * N;
    const size_t lds = 2 * n * sizeof(double);   // (as gauss_seidel_relative_vc: N <= 63, inside the default 64 KiB)
    int threads = (int)((n + 63) / 64 * 64);
    if (threads > 1024) threads = 1024;          // (n <= 63^2 = 3969 <= GS_PTS * 1024)
    hipLaunchKernelGGL(k_gs_relative_bc, dim3(1), dim3(threads), lds, s, N, bc_geom(N, kind), h2, inv, sd, A, U, F, atol, rtol,
                       max_iters, state, err_out);
}

void gauss_seidel_relative_bc_mean(hipStream_t s, int N, double h2, double inv, const int *kind, const double *A, double *U,
                                   const double *F, double atol, double rtol, int max_iters, int *state, double *err_out,
                                   double *mean_out)
{
    const size_t n = (size_t)N * N;
    const size_t lds = 2 * n * sizeof(double);   // (as gauss_seidel_relative_bc)
    int threads = (int)((n + 63) / 64 * 64);
    if (threads > 1024) threads = 1024;
    hipLaunchKernelGGL(k_gs_relative_bc_mean, dim3(1), dim3(threads), lds, s, N, bc_geom(N, kind), h2, inv, 0.0, A, U, F, atol, rtol,
                       max_iters, state, err_out, mean_out);
}

void restrict_bc(hipStream_t s, int N, const int *kind, const double *D, int M, double *Fc, const RestrictTable &t)
{
    hipLaunchKernelGGL(k_restrict_bc, dim3((M + TB - 1) / TB, M), dim3(TB), 0, s, N, D, M, bc_geom(M, kind), Fc, t.lo, t.w);
}

void prolong_add_bc(hipStream_t s, int M, const int *kind, const double *Uc, int N, const double *Uin, double *Uout, const int *lo,
                    const double *w)
{
    hipLaunchKernelGGL(k_prolong_add_bc, dim3((N + TB - 1) / TB, N), dim3(TB), 0, s, M, Uc, N, bc_geom(N, kind), Uin, Uout, lo, w);
}

void neumann_source(hipStream_t s, int N, double t, const int *kind, const double *A, const double *F, const double *G, double *Fout)
{
    hipLaunchKernelGGL(k_neumann_source, dim3((N + TB - 1) / TB, N), dim3(TB), 0, s, N, t, kind[0], kind[1], kind[2], kind[3],
                       bc_geom(N, kind), A, F, G, Fout);
}

}  // namespace k
}  // namespace mg
