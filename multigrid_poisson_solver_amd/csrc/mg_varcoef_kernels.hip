// mg_varcoef_kernels.hip -- fp64 kernels of the residual-tolerance solver with a variable coefficient (include/mg_varcoef.h;
// driven by mg_solve.cpp: SolveOperator's members): the weighted Jacobi sweep, the residual, the operator on its own, the residual
// L2 norm, the red-black Gauss-Seidel coarse solve, the coarsening of the nodal coefficient and its check.
// Built with -ffp-contract=off like every kernel file: the header fixes the evaluation order (every product and every sum
// rounded once) so that numpy restates it bit for bit, and so that a == 1 gives the bits of the constant-coefficient kernels
// (mg_solve_kernels.hip, mg_kernels.hip), whose shapes these kernels copy: a lane walks 4 rows down its column (any N) or its
// column pair (even N from PAIR_MIN_N on, 16-byte accesses) with a rolling window of three rows of U AND of a in registers, so
// each value comes from memory once per block column (the east / west neighbours are the neighbouring lanes' values: L1
// hits); from NT_MIN_N on the sweep and the norm take F through non-temporal loads.  The pair form of the residual uses
// non-temporal F loads and D stores at every size it runs at (from PAIR_MIN_N on), as k_residual_pairs does: F is read once
// and D is read once, by the restriction.  Memory-bound: a sweep moves 32 B per point (U, a, F in, U out) against the
// constant sweep's 24.  d, q = 1/d and c = omega*q are formed per point in the kernel: one fp64 division per 32 B of
// traffic, instead of a fourth array to read.
// The __device__ bodies live in mg_varcoef_impl.h, which mg_varcoef_batch_kernels.hip compiles too: the kernels below hand
// them the arrays of their one instance.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_varcoef_impl.h"

namespace mg {
namespace k {

namespace {

// (the `_vc` kernels: a coefficient, no reaction term -- HAS_A = true, HAS_S = false)
template <bool ZERO_IN, bool PAIR, bool NT>
__global__ __launch_bounds__(TB) void k_wjacobi_vc(VcArgs k)
{
    if constexpr (PAIR) vc_pairs<ZERO_IN ? OP_SWEEP_ZERO : OP_SWEEP, NT, true, false>(k);
    else vc_cols<ZERO_IN ? OP_SWEEP_ZERO : OP_SWEEP, true, false>(k);
}

// (the pair form is non-temporal at every size, see vc_pairs: no NT parameter)
template <bool PAIR>
__global__ __launch_bounds__(TB) void k_residual_vc(VcArgs k)
{
    if constexpr (PAIR) vc_pairs<OP_RESIDUAL, true, true, false>(k);
    else vc_cols<OP_RESIDUAL, true, false>(k);
}

template <bool HAS_A>
__global__ __launch_bounds__(TB) void k_apply_vc(VcArgs k)
{
    vc_cols<OP_APPLY, HAS_A, false>(k);
}

template <bool PAIR, bool NT>
__global__ __launch_bounds__(TB) void k_resnorm_vc(int N, double inv, double sd, const double *__restrict__ A,
                                                   const double *__restrict__ U, const double *__restrict__ F,
                                                   double *__restrict__ part)
{
    resnorm_vc_body<PAIR, NT, true, false>(VcArgs{N, 0.0, inv, sd, 0.0, A, U, F, part, +1});
}

__global__ __launch_bounds__(1024) void k_resnorm_finish_vc(const double *__restrict__ part, size_t n, double *__restrict__ out)
{
    resnorm_finish_body(part, n, out);
}

__global__ __launch_bounds__(1024) void k_gs_relative_vc(int N, double h2, double inv, double sd, const double *__restrict__ Ag,
                                                         double *__restrict__ Ug, const double *__restrict__ Fg, double atol,
                                                         double rtol, int max_iters, int *__restrict__ state,
                                                         double *__restrict__ err_out)
{
    gs_relative_vc_body<false, false>(N, h2, inv, sd, Ag, nullptr, Ug, Fg, atol, rtol, max_iters, state, err_out);
}

__global__ __launch_bounds__(TB) void k_coef_coarsen(int N, const double *__restrict__ Af, int M, double *__restrict__ Ac,
                                                     const int *__restrict__ lo, const double *__restrict__ w)
{
    coef_coarsen_body(N, Af, M, Ac, lo, w);
}

__global__ __launch_bounds__(TB) void k_coef_check(const double *__restrict__ A, size_t n, int *__restrict__ flag)
{
    coef_check_body(A, n, flag);
}

}  // namespace

// ------------------------------------------------------------------ launchers
void wjacobi_vc(hipStream_t s, int N, double dx2, double sd, double omega, const double *A, const double *in, const double *F,
                double *out)
{
    const VcArgs k{N, dx2, 0.0, sd, omega, A, in, F, out, +1};
    dispatch_form(N, true, [&](auto pair, auto nt, auto, dim3 g) {
        if (!in) hipLaunchKernelGGL((k_wjacobi_vc<true, pair(), nt()>), g, dim3(TB), 0, s, k);
        else hipLaunchKernelGGL((k_wjacobi_vc<false, pair(), nt()>), g, dim3(TB), 0, s, k);
    });
}

void residual_vc(hipStream_t s, int N, double inv, double sd, const double *A, const double *U, const double *F, double *D, int sign)
{
    const VcArgs k{N, 0.0, inv, sd, 0.0, A, U, F, D, sign};
    dispatch_form(N, true, [&](auto pair, auto, auto, dim3 g) { hipLaunchKernelGGL(k_residual_vc<pair()>, g, dim3(TB), 0, s, k); });
}

void apply_vc(hipStream_t s, int N, double inv, double sd, const double *A, const double *U, double *out)
{
    const VcArgs k{N, 0.0, inv, sd, 0.0, A, U, nullptr, out, +1};
    if (A) hipLaunchKernelGGL(k_apply_vc<true>, grid_rows(N), dim3(TB), 0, s, k);
    else hipLaunchKernelGGL(k_apply_vc<false>, grid_rows(N), dim3(TB), 0, s, k);
}

void resnorm_vc(hipStream_t s, int N, double inv, double sd, const double *A, const double *U, const double *F, double *part,
                double *out)
{
    const size_t np = resnorm_partials(N);   // (the same partition as the constant norm)
    dispatch_form(N, true, [&](auto pair, auto nt, auto, dim3 g) {
        hipLaunchKernelGGL((k_resnorm_vc<pair(), nt()>), g, dim3(TB), 0, s, N, inv, sd, A, U, F, part);
    });
    hipLaunchKernelGGL(k_resnorm_finish_vc, dim3(1), dim3(1024), 0, s, part, np, out);
}

void gauss_seidel_relative_vc(hipStream_t s, int N, double h2, double inv, double sd, const double *A, double *U, const double *F,
                              double atol, double rtol, int max_iters, int *state, double *err_out)
{
    const size_t n = (size_t)N * N;
    const size_t lds = 2 * n * sizeof(double);   // (as gauss_seidel_relative: N <= 63, inside the default 64 KiB)
    int threads = (int)((n + 63) / 64 * 64);
    if (threads > 1024) threads = 1024;          // (n <= 63^2 = 3969 <= GS_PTS * 1024)
    hipLaunchKernelGGL(k_gs_relative_vc, dim3(1), dim3(threads), lds, s, N, h2, inv, sd, A, U, F, atol, rtol, max_iters, state, err_out);
}

void coef_coarsen(hipStream_t s, int N, const double *Af, int M, double *Ac, const RestrictTable &t)
{
    hipLaunchKernelGGL(k_coef_coarsen, dim3((M + TB - 1) / TB, M), dim3(TB), 0, s, N, Af, M, Ac, t.lo, t.w);
}

void coef_check(hipStream_t s, const double *A, size_t n, int *flag)
{
    size_t blocks = (n + TB - 1) / TB;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_coef_check, dim3((unsigned)blocks), dim3(TB), 0, s, A, n, flag);
}

}  // namespace k
}  // namespace mg
