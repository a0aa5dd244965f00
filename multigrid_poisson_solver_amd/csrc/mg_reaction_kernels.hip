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
// The __device__ bodies live in mg_reaction_impl.h, layered over mg_varcoef_impl.h.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_reaction_impl.h"

namespace mg {
namespace k {

namespace {

template <bool ZERO_IN, bool PAIR, bool NT, bool HAS_A>
__global__ __launch_bounds__(TB) void k_wjacobi_rx(RxArgs x)
{
    if constexpr (PAIR) rx_pairs<ZERO_IN ? OP_SWEEP_ZERO : OP_SWEEP, NT, HAS_A>(x);
    else rx_cols<ZERO_IN ? OP_SWEEP_ZERO : OP_SWEEP, HAS_A>(x);
}

// (the pair form is non-temporal at every size, as k_residual_vc's: no NT parameter)
template <bool PAIR, bool HAS_A>
__global__ __launch_bounds__(TB) void k_residual_rx(RxArgs x)
{
    if constexpr (PAIR) rx_pairs<OP_RESIDUAL, true, HAS_A>(x);
    else rx_cols<OP_RESIDUAL, HAS_A>(x);
}

template <bool HAS_A>
__global__ __launch_bounds__(TB) void k_apply_rx(RxArgs x)
{
    rx_cols<OP_APPLY, HAS_A>(x);
}

template <bool PAIR, bool NT, bool HAS_A>
__global__ __launch_bounds__(TB) void k_resnorm_rx(RxArgs x)
{
    rx_resnorm_body<PAIR, NT, HAS_A>(x);
}

__global__ __launch_bounds__(1024) void k_resnorm_finish_rx(const double *__restrict__ part, size_t n, double *__restrict__ out)
{
    resnorm_finish_vc_body(part, n, out);
}

__global__ __launch_bounds__(1024) void k_gs_relative_rx(int N, double h2, double inv, double sd, const double *__restrict__ Ag,
                                                         const double *__restrict__ Sg, double *__restrict__ Ug,
                                                         const double *__restrict__ Fg, double atol, double rtol, int max_iters,
                                                         int *__restrict__ state, double *__restrict__ err_out)
{
    rx_gs_relative_body(N, h2, inv, sd, Ag, Sg, Ug, Fg, atol, rtol, max_iters, state, err_out);
}

__global__ __launch_bounds__(TB) void k_reaction_check(const double *__restrict__ S, size_t n, int *__restrict__ flag)
{
    rx_check_body(S, n, flag);
}

// launch K<..., HAS_A> with HAS_A = (A != nullptr)
#define MG_RX_LAUNCH(KERNEL, GRID, ...)                                                                       \
    do {                                                                                                      \
        if (x.k.A) hipLaunchKernelGGL((KERNEL<__VA_ARGS__, true>), GRID, dim3(TB), 0, s, x);                  \
        else hipLaunchKernelGGL((KERNEL<__VA_ARGS__, false>), GRID, dim3(TB), 0, s, x);                       \
    } while (0)

}  // namespace

// ------------------------------------------------------------------ launchers
void wjacobi_rx(hipStream_t s, int N, double dx2, double sd, double omega, const double *A, const double *S, const double *in,
                const double *F, double *out)
{
    const RxArgs x{VcArgs{N, dx2, 0.0, sd, omega, A, in, F, out, +1}, S};
    if (use_pairs(N)) {
        const dim3 g = grid_pairs(N);
        const bool nt = N >= NT_MIN_N;
        if (!in) {
            if (nt) MG_RX_LAUNCH(k_wjacobi_rx, g, true, true, true);
            else MG_RX_LAUNCH(k_wjacobi_rx, g, true, true, false);
        } else {
            if (nt) MG_RX_LAUNCH(k_wjacobi_rx, g, false, true, true);
            else MG_RX_LAUNCH(k_wjacobi_rx, g, false, true, false);
        }
        return;
    }
    if (!in) MG_RX_LAUNCH(k_wjacobi_rx, grid_rows(N), true, false, false);
    else MG_RX_LAUNCH(k_wjacobi_rx, grid_rows(N), false, false, false);
}

void residual_rx(hipStream_t s, int N, double dx2, double inv, double sd, const double *A, const double *S, const double *U,
                 const double *F, double *D, int sign)
{
    const RxArgs x{VcArgs{N, dx2, inv, sd, 0.0, A, U, F, D, sign}, S};
    if (use_pairs(N)) MG_RX_LAUNCH(k_residual_rx, grid_pairs(N), true);
    else MG_RX_LAUNCH(k_residual_rx, grid_rows(N), false);
}

void apply_rx(hipStream_t s, int N, double dx2, double inv, double sd, const double *A, const double *S, const double *U, double *out)
{
    const RxArgs x{VcArgs{N, dx2, inv, sd, 0.0, A, U, nullptr, out, +1}, S};
    if (A) hipLaunchKernelGGL(k_apply_rx<true>, grid_rows(N), dim3(TB), 0, s, x);
    else hipLaunchKernelGGL(k_apply_rx<false>, grid_rows(N), dim3(TB), 0, s, x);
}

void resnorm_rx(hipStream_t s, int N, double dx2, double inv, double sd, const double *A, const double *S, const double *U,
                const double *F, double *part, double *out)
{
    const size_t np = resnorm_partials(N);   // (the same partition as the constant norm)
    const RxArgs x{VcArgs{N, dx2, inv, sd, 0.0, A, U, F, part, +1}, S};
    if (use_pairs(N)) {
        if (N >= NT_MIN_N) MG_RX_LAUNCH(k_resnorm_rx, grid_pairs(N), true, true);
        else MG_RX_LAUNCH(k_resnorm_rx, grid_pairs(N), true, false);
    } else {
        MG_RX_LAUNCH(k_resnorm_rx, grid_rows(N), false, false);
    }
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
