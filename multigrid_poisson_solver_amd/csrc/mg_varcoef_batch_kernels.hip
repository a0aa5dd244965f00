// mg_varcoef_batch_kernels.hip -- batched forms of the variable-coefficient kernels (include/mg_varcoef_batch.h; driven by
// mg_solve_batch.cpp: run_cycle_batch): ONE launch runs a kernel of mg_varcoef_kernels.hip for every active instance.  The
// __device__ bodies are the ones of mg_varcoef_impl.h, compiled here with the same flags (-ffp-contract=off): an instance
// runs the code, the block partition (grid x, y) and the summation order of its single launch, so its bits are the single
// solve's.  Which instance a block works on: blockIdx.z for the streaming kernels, whose single grids are (column blocks,
// row blocks); blockIdx.x for the one-workgroup coarse solve and the norm's finish; blockIdx.y for the check, whose single
// grid is one-dimensional (max_batch <= 65535 fits each of them).  The instance's arrays come from a NodeBatchItem table in
// device memory (mg_internal.h), the level's coefficient in the slot `coarse`, which none of these launches uses otherwise:
//   sweep            in = U (unused from the zero field), F, coarse = a, out
//   residual, norm   in = U, F, coarse = a, out = D (the norm: none; partials at part + z*resnorm_partials(N))
//   coarse solve     F, coarse = a, out = U; state at state + 4*instance
//   coarsening       in = a_f, out = a_c          check   in = a; flag at flags + instance
//   operator alone   in = U, coarse = a (may be null for an instance: a = 1), out
// N, dx2, inv, sd and omega are the same for every instance of a launch and stay kernel arguments.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_varcoef_impl.h"

namespace mg {
namespace k {

namespace {

__device__ __forceinline__ VcArgs item_args(const NodeBatchItem &it, int N, double dx2, double inv, double sd, double omega, int sign)
{
    return VcArgs{N, dx2, inv, sd, omega, static_cast<const double *>(it.coarse), static_cast<const double *>(it.in),
                  static_cast<const double *>(it.F), static_cast<double *>(it.out), sign};
}

template <bool ZERO_IN, bool PAIR, bool NT>
__global__ __launch_bounds__(TB) void k_wjacobi_vc_b(int N, double dx2, double sd, double omega, const NodeBatchItem *__restrict__ items)
{
    const VcArgs k = item_args(items[blockIdx.z], N, dx2, 0.0, sd, omega, +1);
    if constexpr (PAIR) vc_pairs<ZERO_IN ? OP_SWEEP_ZERO : OP_SWEEP, NT, true, false>(k);
    else vc_cols<ZERO_IN ? OP_SWEEP_ZERO : OP_SWEEP, true, false>(k);
}

template <bool PAIR>
__global__ __launch_bounds__(TB) void k_residual_vc_b(int N, double inv, double sd, const NodeBatchItem *__restrict__ items, int sign)
{
    const VcArgs k = item_args(items[blockIdx.z], N, 0.0, inv, sd, 0.0, sign);
    if constexpr (PAIR) vc_pairs<OP_RESIDUAL, true, true, false>(k);
    else vc_cols<OP_RESIDUAL, true, false>(k);
}

// the operator alone (apply_vc): the coefficient may be absent PER INSTANCE (a = 1 through the same expressions, as the
// single kernel without one); the choice is the same for every lane of a block
__global__ __launch_bounds__(TB) void k_apply_vc_b(int N, double inv, double sd, const NodeBatchItem *__restrict__ items)
{
    const VcArgs k = item_args(items[blockIdx.z], N, 0.0, inv, sd, 0.0, +1);
    if (k.A) vc_cols<OP_APPLY, true, false>(k);
    else vc_cols<OP_APPLY, false, false>(k);
}

// instance z's np partials at part + z*np
template <bool PAIR, bool NT>
__global__ __launch_bounds__(TB) void k_resnorm_vc_b(int N, double inv, double sd, const NodeBatchItem *__restrict__ items,
                                                     double *__restrict__ part, size_t np)
{
    VcArgs k = item_args(items[blockIdx.z], N, 0.0, inv, sd, 0.0, +1);
    k.out = part + blockIdx.z * np;
    resnorm_vc_body<PAIR, NT, true, false>(k);
}

// out[i] = sqrt(sum of instance i's np partials): one block per instance, each the single-instance finish
__global__ __launch_bounds__(1024) void k_resnorm_finish_vc_b(const double *__restrict__ part, size_t np, double *__restrict__ out)
{
    resnorm_finish_body(part + blockIdx.x * np, np, out + blockIdx.x);
}

// one workgroup per instance: its own err0, its own stop, its state at state + 4i (no err_out)
__global__ __launch_bounds__(1024) void k_gs_relative_vc_b(int N, double h2, double inv, double sd, const NodeBatchItem *__restrict__ items,
                                                           double atol, double rtol, int max_iters, int *__restrict__ state)
{
    const NodeBatchItem &it = items[blockIdx.x];
    gs_relative_vc_body<false, false>(N, h2, inv, sd, static_cast<const double *>(it.coarse), nullptr, static_cast<double *>(it.out),
                                      static_cast<const double *>(it.F), atol, rtol, max_iters, state + 4 * blockIdx.x, nullptr);
}

__global__ __launch_bounds__(TB) void k_coef_coarsen_b(int N, int M, const NodeBatchItem *__restrict__ items, const int *__restrict__ lo,
                                                       const double *__restrict__ w)
{
    const NodeBatchItem &it = items[blockIdx.z];
    coef_coarsen_body(N, static_cast<const double *>(it.in), M, static_cast<double *>(it.out), lo, w);
}

// flags[i] = 1 when instance i (blockIdx.y) has a value that is not finite or not > 0 (the caller zeroes the flags)
__global__ __launch_bounds__(TB) void k_coef_check_b(const NodeBatchItem *__restrict__ items, size_t n, int *__restrict__ flags)
{
    coef_check_body(static_cast<const double *>(items[blockIdx.y].in), n, flags + blockIdx.y);
}

}  // namespace

// ------------------------------------------------------------------ launchers (the form is chosen as the single launcher
// of the same name without `_batch` chooses it)
void wjacobi_vc_batch(hipStream_t s, int n, int N, double dx2, double sd, double omega, bool zero_in, const NodeBatchItem *items)
{
    dispatch_form(N, true, [&](auto pair, auto nt, auto, dim3 g) {
        g = with_instances(g, n);
        if (zero_in) hipLaunchKernelGGL((k_wjacobi_vc_b<true, pair(), nt()>), g, dim3(TB), 0, s, N, dx2, sd, omega, items);
        else hipLaunchKernelGGL((k_wjacobi_vc_b<false, pair(), nt()>), g, dim3(TB), 0, s, N, dx2, sd, omega, items);
    });
}

void residual_vc_batch(hipStream_t s, int n, int N, double inv, double sd, const NodeBatchItem *items, int sign)
{
    dispatch_form(N, true, [&](auto pair, auto, auto, dim3 g) {
        hipLaunchKernelGGL(k_residual_vc_b<pair()>, with_instances(g, n), dim3(TB), 0, s, N, inv, sd, items, sign);
    });
}

void apply_vc_batch(hipStream_t s, int n, int N, double inv, double sd, const NodeBatchItem *items)
{
    hipLaunchKernelGGL(k_apply_vc_b, with_instances(grid_rows(N), n), dim3(TB), 0, s, N, inv, sd, items);
}

void resnorm_vc_batch(hipStream_t s, int n, int N, double inv, double sd, const NodeBatchItem *items, double *part, double *out)
{
    const size_t np = resnorm_partials(N);   // (the same partition as the constant norm)
    dispatch_form(N, true, [&](auto pair, auto nt, auto, dim3 g) {
        hipLaunchKernelGGL((k_resnorm_vc_b<pair(), nt()>), with_instances(g, n), dim3(TB), 0, s, N, inv, sd, items, part, np);
    });
    hipLaunchKernelGGL(k_resnorm_finish_vc_b, dim3(n), dim3(1024), 0, s, part, np, out);
}

void gauss_seidel_relative_vc_batch(hipStream_t s, int n, int N, double h2, double inv, double sd, const NodeBatchItem *items,
                                    double atol, double rtol, int max_iters, int *state)
{
    const size_t cells = (size_t)N * N;
    const size_t lds = 2 * cells * sizeof(double);   // (gauss_seidel_relative_vc's request: N <= 63, inside the default 64 KiB)
    int threads = (int)((cells + 63) / 64 * 64);
    if (threads > 1024) threads = 1024;
    hipLaunchKernelGGL(k_gs_relative_vc_b, dim3(n), dim3(threads), lds, s, N, h2, inv, sd, items, atol, rtol, max_iters, state);
}

void coef_coarsen_batch(hipStream_t s, int n, int N, int M, const NodeBatchItem *items, const RestrictTable &t)
{
    hipLaunchKernelGGL(k_coef_coarsen_b, dim3((M + TB - 1) / TB, M, n), dim3(TB), 0, s, N, M, items, t.lo, t.w);
}

void coef_check_batch(hipStream_t s, int n, size_t count, const NodeBatchItem *items, int *flags)
{
    size_t blocks = (count + TB - 1) / TB;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_coef_check_b, dim3((unsigned)blocks, n), dim3(TB), 0, s, items, count, flags);
}

}  // namespace k
}  // namespace mg
