// mg_reaction_batch_kernels.hip -- batched forms of the reaction kernels (include/mg_rx_batch.h; driven by
// mg_solve_batch.cpp: run_cycle_batch): ONE launch runs a kernel of mg_reaction_kernels.hip for every active instance.  The
// __device__ bodies are the ones of mg_varcoef_impl.h (HAS_S = true), compiled here with the same flags (-ffp-contract=off): an instance
// runs the code, the block partition (grid x, y) and the summation order of its single launch, so its bits are the single
// solve's.  Which instance a block works on: blockIdx.z for the streaming kernels, whose single grids are (column blocks,
// row blocks); blockIdx.x for the one-workgroup coarse solve and the norm's finish; blockIdx.y for the check, whose single
// grid is one-dimensional (max_batch <= 65535 fits each of them) -- as mg_varcoef_batch_kernels.hip takes it.  The instance's
// arrays come from a NodeBatchItem table in device memory (mg_internal.h): the level's coefficient in the slot `coarse`, as
// the `_vc` launches carry it, the level's reaction term in the slot `Fc`, which none of these launches uses otherwise:
//   sweep            in = U (unused from the zero field), F, coarse = a, Fc = s, out
//   residual, norm   in = U, F, coarse = a, Fc = s, out = D (the norm: none; partials at part + z*resnorm_partials(N))
//   coarse solve     F, coarse = a, Fc = s, out = U; state at state + 4*instance
//   operator alone   in = U, coarse = a, Fc = s, out
//   check            in = s; flag at flags + instance
// Within one launch either every instance has a coefficient or none has: HAS_A is a template parameter chosen per launch, and
// without a coefficient the slot `coarse` is not read and no array of ones is streamed.  N, dx2, inv, sd and omega are the same
// for every instance of a launch and stay kernel arguments.  The coarsening of s is k::coef_coarsen_batch.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_reaction_impl.h"

namespace mg {
namespace k {

namespace {

template <bool HAS_A>
__device__ __forceinline__ VcArgs rx_item_args(const NodeBatchItem &it, int N, double dx2, double inv, double sd, double omega, double *out,
                                               int sign)
{
    return VcArgs{N, dx2, inv, sd, omega, HAS_A ? static_cast<const double *>(it.coarse) : nullptr,
                  static_cast<const double *>(it.in), static_cast<const double *>(it.F), out, sign,
                  static_cast<const double *>(it.Fc)};
}

template <bool ZERO_IN, bool PAIR, bool NT, bool HAS_A>
__global__ __launch_bounds__(TB) void k_wjacobi_rx_b(int N, double dx2, double sd, double omega, const NodeBatchItem *__restrict__ items)
{
    const NodeBatchItem &it = items[blockIdx.z];
    const VcArgs k = rx_item_args<HAS_A>(it, N, dx2, 0.0, sd, omega, static_cast<double *>(it.out), +1);
    if constexpr (PAIR) vc_pairs<ZERO_IN ? OP_SWEEP_ZERO : OP_SWEEP, NT, HAS_A, true>(k);
    else vc_cols<ZERO_IN ? OP_SWEEP_ZERO : OP_SWEEP, HAS_A, true>(k);
}

// (the pair form is non-temporal at every size, as k_residual_rx's)
template <bool PAIR, bool HAS_A>
__global__ __launch_bounds__(TB) void k_residual_rx_b(int N, double dx2, double inv, double sd, const NodeBatchItem *__restrict__ items,
                                                      int sign)
{
    const NodeBatchItem &it = items[blockIdx.z];
    const VcArgs k = rx_item_args<HAS_A>(it, N, dx2, inv, sd, 0.0, static_cast<double *>(it.out), sign);
    if constexpr (PAIR) vc_pairs<OP_RESIDUAL, true, HAS_A, true>(k);
    else vc_cols<OP_RESIDUAL, HAS_A, true>(k);
}

template <bool HAS_A>
__global__ __launch_bounds__(TB) void k_apply_rx_b(int N, double dx2, double inv, double sd, const NodeBatchItem *__restrict__ items)
{
    const NodeBatchItem &it = items[blockIdx.z];
    vc_cols<OP_APPLY, HAS_A, true>(rx_item_args<HAS_A>(it, N, dx2, inv, sd, 0.0, static_cast<double *>(it.out), +1));
}

// instance z's np partials at part + z*np
template <bool PAIR, bool NT, bool HAS_A>
__global__ __launch_bounds__(TB) void k_resnorm_rx_b(int N, double dx2, double inv, double sd, const NodeBatchItem *__restrict__ items,
                                                     double *__restrict__ part, size_t np)
{
    resnorm_vc_body<PAIR, NT, HAS_A, true>(rx_item_args<HAS_A>(items[blockIdx.z], N, dx2, inv, sd, 0.0, part + blockIdx.z * np, +1));
}

// out[i] = sqrt(sum of instance i's np partials): one block per instance, each the single-instance finish
__global__ __launch_bounds__(1024) void k_resnorm_finish_rx_b(const double *__restrict__ part, size_t np, double *__restrict__ out)
{
    resnorm_finish_body(part + blockIdx.x * np, np, out + blockIdx.x);
}

// one workgroup per instance: its own err0, its own stop, its state at state + 4i (no err_out)
template <bool HAS_A>
__global__ __launch_bounds__(1024) void k_gs_relative_rx_b(int N, double h2, double inv, double sd, const NodeBatchItem *__restrict__ items,
                                                           double atol, double rtol, int max_iters, int *__restrict__ state)
{
    const NodeBatchItem &it = items[blockIdx.x];
    gs_relative_vc_body<true, true>(N, h2, inv, sd, HAS_A ? static_cast<const double *>(it.coarse) : nullptr,
                                    static_cast<const double *>(it.Fc), static_cast<double *>(it.out), static_cast<const double *>(it.F), atol,
                                    rtol, max_iters, state + 4 * blockIdx.x, nullptr);
}

// flags[i] = 1 when instance i (blockIdx.y) has a value that is not finite or not >= 0 (the caller zeroes the flags)
__global__ __launch_bounds__(TB) void k_reaction_check_b(const NodeBatchItem *__restrict__ items, size_t n, int *__restrict__ flags)
{
    rx_check_body(static_cast<const double *>(items[blockIdx.y].in), n, flags + blockIdx.y);
}

}  // namespace

// ------------------------------------------------------------------ launchers (the form is chosen as the single launcher
// of the same name without `_batch` chooses it; has_a: every instance's slot `coarse` holds its coefficient)
void wjacobi_rx_batch(hipStream_t s, int n, int N, double dx2, double sd, double omega, bool zero_in, bool has_a, const NodeBatchItem *items)
{
    dispatch_form(N, has_a, [&](auto pair, auto nt, auto a, dim3 g) {
        g = with_instances(g, n);
        if (zero_in) hipLaunchKernelGGL((k_wjacobi_rx_b<true, pair(), nt(), a()>), g, dim3(TB), 0, s, N, dx2, sd, omega, items);
        else hipLaunchKernelGGL((k_wjacobi_rx_b<false, pair(), nt(), a()>), g, dim3(TB), 0, s, N, dx2, sd, omega, items);
    });
}

void residual_rx_batch(hipStream_t s, int n, int N, double dx2, double inv, double sd, bool has_a, const NodeBatchItem *items, int sign)
{
    dispatch_form(N, has_a, [&](auto pair, auto, auto a, dim3 g) {
        hipLaunchKernelGGL((k_residual_rx_b<pair(), a()>), with_instances(g, n), dim3(TB), 0, s, N, dx2, inv, sd, items, sign);
    });
}

void apply_rx_batch(hipStream_t s, int n, int N, double dx2, double inv, double sd, bool has_a, const NodeBatchItem *items)
{
    const dim3 g = with_instances(grid_rows(N), n);
    if (has_a) hipLaunchKernelGGL(k_apply_rx_b<true>, g, dim3(TB), 0, s, N, dx2, inv, sd, items);
    else hipLaunchKernelGGL(k_apply_rx_b<false>, g, dim3(TB), 0, s, N, dx2, inv, sd, items);
}

void resnorm_rx_batch(hipStream_t s, int n, int N, double dx2, double inv, double sd, bool has_a, const NodeBatchItem *items, double *part,
                      double *out)
{
    const size_t np = resnorm_partials(N);   // (the same partition as the constant norm)
    dispatch_form(N, has_a, [&](auto pair, auto nt, auto a, dim3 g) {
        hipLaunchKernelGGL((k_resnorm_rx_b<pair(), nt(), a()>), with_instances(g, n), dim3(TB), 0, s, N, dx2, inv, sd, items, part, np);
    });
    hipLaunchKernelGGL(k_resnorm_finish_rx_b, dim3(n), dim3(1024), 0, s, part, np, out);
}

void gauss_seidel_relative_rx_batch(hipStream_t s, int n, int N, double h2, double inv, double sd, bool has_a, const NodeBatchItem *items,
                                    double atol, double rtol, int max_iters, int *state)
{
    const size_t cells = (size_t)N * N;
    const size_t lds = 2 * cells * sizeof(double);   // (gauss_seidel_relative_rx's request: N <= 63, inside the default 64 KiB)
    int threads = (int)((cells + 63) / 64 * 64);
    if (threads > 1024) threads = 1024;
    if (has_a) hipLaunchKernelGGL(k_gs_relative_rx_b<true>, dim3(n), dim3(threads), lds, s, N, h2, inv, sd, items, atol, rtol, max_iters, state);
    else hipLaunchKernelGGL(k_gs_relative_rx_b<false>, dim3(n), dim3(threads), lds, s, N, h2, inv, sd, items, atol, rtol, max_iters, state);
}

void reaction_check_batch(hipStream_t s, int n, size_t count, const NodeBatchItem *items, int *flags)
{
    size_t blocks = (count + TB - 1) / TB;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_reaction_check_b, dim3((unsigned)blocks, n), dim3(TB), 0, s, items, count, flags);
}

}  // namespace k
}  // namespace mg
