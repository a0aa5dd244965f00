// mg_reaction_kernels.hip -- fp64 kernels of the residual-tolerance solver with a variable reaction term s(x, y)
// (include/mg_reaction.h; driven by mg_solve.cpp: SolveOperator's members): the weighted Jacobi sweep, the residual, the
// operator on its own, the residual L2 norm, the red-black Gauss-Seidel coarse solve and the check of s.
// Built with -ffp-contract=off like every kernel file.  The shapes are the `_vc` kernels' own (mg_varcoef_kernels.hip): a lane
// walks 4 rows down its column (any N) or its column pair (even N from PAIR_MIN_N on, 16-byte accesses) with a rolling window
// of three rows of U and of a in registers.  The new stream is ONE load of s per point, at the centre row only -- a 16-byte
// load in the pair forms, non-temporal where F is: s, like F, is used once per sweep.  Every streaming kernel exists with and
// without a coefficient; without one no array of ones is streamed.  Memory-bound: a sweep moves 40 B per point with a
// (U, a, s, F in, U out) and 32 B without (U, s, F in, U out).  d = (((aN + aS) + aE) + aW) + (sd + s*dx2), q = 1/d and
// c = omega*q are formed per point: one product and one sum more than k_wjacobi_vc.
// The __device__ bodies are mg_varcoef_impl.h's with HAS_S = true; mg_reaction_impl.h adds the check of s.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_reaction_impl.h"

namespace mg {
namespace k {

namespace {

template <bool ZERO_IN, bool PAIR, bool NT, bool HAS_A>
__global__ __launch_bounds__(TB) void k_wjacobi_rx(VcArgs k)
{
    if constexpr (PAIR) vc_pairs<ZERO_IN ? OP_SWEEP_ZERO : OP_SWEEP, NT, HAS_A, true>(k);
    else vc_cols<ZERO_IN ? OP_SWEEP_ZERO : OP_SWEEP, HAS_A, true>(k);
}

// (the pair form is non-temporal at every size, as k_residual_vc's: no NT parameter)
template <bool PAIR, bool HAS_A>
__global__ __launch_bounds__(TB) void k_residual_rx(VcArgs k)
{
    if constexpr (PAIR) vc_pairs<OP_RESIDUAL, true, HAS_A, true>(k);
    else vc_cols<OP_RESIDUAL, HAS_A, true>(k);
}

template <bool HAS_A>
__global__ __launch_bounds__(TB) void k_apply_rx(VcArgs k)
{
    vc_cols<OP_APPLY, HAS_A, true>(k);
}

template <bool PAIR, bool NT, bool HAS_A>
__global__ __launch_bounds__(TB) void k_resnorm_rx(VcArgs k)
{
    resnorm_vc_body<PAIR, NT, HAS_A, true>(k);
}

__global__ __launch_bounds__(1024) void k_resnorm_finish_rx(const double *__restrict__ part, size_t n, double *__restrict__ out)
{
    resnorm_finish_body(part, n, out);
}

__global__ __launch_bounds__(1024) void k_gs_relative_rx(int N, double h2, double inv, double sd, const double *__restrict__ Ag,
                                                         const double *__restrict__ Sg, double *__restrict__ Ug,
                                                         const double *__restrict__ Fg, double atol, double rtol, int max_iters,
                                                         int *__restrict__ state, double *__restrict__ err_out)
{
    gs_relative_vc_body<true, true>(N, h2, inv, sd, Ag, Sg, Ug, Fg, atol, rtol, max_iters, state, err_out);
}

__global__ __launch_bounds__(TB) void k_reaction_check(const double *__restrict__ S, size_t n, int *__restrict__ flag)
{
    rx_check_body(S, n, flag);
}

}  // namespace

// ------------------------------------------------------------------ launchers
void wjacobi_rx(hipStream_t s, int N, double dx2, double sd, double omega, const double *A, const double *S, const double *in,
                const double *F, double *out)
{
    const VcArgs k{N, dx2, 0.0, sd, omega, A, in, F, out, +1, S};
    dispatch_form(N, A != nullptr, [&](auto pair, auto nt, auto has_a, dim3 g) {
        if (!in) hipLaunchKernelGGL((k_wjacobi_rx<true, pair(), nt(), has_a()>), g, dim3(TB), 0, s, k);
        else hipLaunchKernelGGL((k_wjacobi_rx<false, pair(), nt(), has_a()>), g, dim3(TB), 0, s, k);
    });
}

void residual_rx(hipStream_t s, int N, double dx2, double inv, double sd, const double *A, const double *S, const double *U,
                 const double *F, double *D, int sign)
{
    const VcArgs k{N, dx2, inv, sd, 0.0, A, U, F, D, sign, S};
    dispatch_form(N, A != nullptr, [&](auto pair, auto, auto has_a, dim3 g) {
        hipLaunchKernelGGL((k_residual_rx<pair(), has_a()>), g, dim3(TB), 0, s, k);
    });
}

void apply_rx(hipStream_t s, int N, double dx2, double inv, double sd, const double *A, const double *S, const double *U, double *out)
{
    const VcArgs k{N, dx2, inv, sd, 0.0, A, U, nullptr, out, +1, S};
    if (A) hipLaunchKernelGGL(k_apply_rx<true>, grid_rows(N), dim3(TB), 0, s, k);
    else hipLaunchKernelGGL(k_apply_rx<false>, grid_rows(N), dim3(TB), 0, s, k);
}

void resnorm_rx(hipStream_t s, int N, double dx2, double inv, double sd, const double *A, const double *S, const double *U,
                const double *F, double *part, double *out)
{
    const size_t np = resnorm_partials(N);   // (the same partition as the constant norm)
    const VcArgs k{N, dx2, inv, sd, 0.0, A, U, F, part, +1, S};
    dispatch_form(N, A != nullptr, [&](auto pair, auto nt, auto has_a, dim3 g) {
        hipLaunchKernelGGL((k_resnorm_rx<pair(), nt(), has_a()>), g, dim3(TB), 0, s, k);
    });
    hipLaunchKernelGGL(k_resnorm_finish_rx, dim3(1), dim3(1024), 0, s, part, np, out);
}

void gauss_seidel_relative_rx(hipStream_t s, int N, double h2, double inv, double sd, const double *A, const double *S, double *U,
                              const double *F, double atol, double rtol, int max_iters, int *state, double *err_out)
{
    const size_t n = (size_t)N * N;
    const size_t lds = 2 * n * sizeof(double);   // (as gauss_seidel_relative_vc: N <= 63, inside the default 64 KiB)
    int threads = (int)((n + 63) / 64 * 64);
    if (threads > 1024) threads = 1024;          // (n <= 63^2 = 3969 <= GS_PTS * 1024)
    hipLaunchKernelGGL(k_gs_relative_rx, dim3(1), dim3(threads), lds, s, N, h2, inv, sd, A, S, U, F, atol, rtol, max_iters, state, err_out);
}

void reaction_check(hipStream_t s, const double *S, size_t n, int *flag)
{
    size_t blocks = (n + TB - 1) / TB;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_reaction_check, dim3((unsigned)blocks), dim3(TB), 0, s, S, n, flag);
}

}  // namespace k
}  // namespace mg
