// mg_adjoint_kernels.hip -- the contractions that turn an adjoint field into gradients (include/mg_adjoint.h; driven by
// mg_adjoint.cpp): the gradient in the nodal coefficient a from lam and U, the gradient in the rim data from lam, a and
// Ubar, and the batched twin of each, ONE launch over n instances.  The __device__ bodies are mg_adjoint_impl.h's, compiled
// here once for both forms with -ffp-contract=off like every kernel file: an instance of a batched launch runs the code and
// the block partition (grid x, y) of its single launch, so its bits are the single launch's.  Which instance a block works
// on: blockIdx.z; its arrays come from a NodeBatchItem table in device memory (mg_internal.h):
//   coefficient gradient   in = lam, F = U, out = gA
//   rim gradient           in = lam, F = Ubar (may be null: 0.0), coarse = a (may be null: a = 1), out = gU
// N, h and inv are the same for every instance of a launch and stay kernel arguments.
// The coefficient gradient takes the three forms of k_heat_rhs_vc with its thresholds (one column per lane; column pairs
// with 16-byte accesses for even N >= 512; non-temporal stores of gA from N >= 4096); the rim gradient is one pass of 8 B
// per point plus O(N) work and has the column form only.  No LDS.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_adjoint_impl.h"

namespace mg {
namespace k {

namespace {

using namespace adj;

template <bool PAIR, bool NT>
__global__ __launch_bounds__(TB) void k_coef_grad(int N, double h, const double *__restrict__ Lm, const double *__restrict__ U,
                                                  double *__restrict__ G)
{
    if constexpr (PAIR) coef_grad_pairs<NT>(N, h, Lm, U, G);
    else coef_grad_cols(N, h, Lm, U, G);
}

template <bool PAIR, bool NT>
__global__ __launch_bounds__(TB) void k_coef_grad_b(int N, double h, const NodeBatchItem *__restrict__ items)
{
    const NodeBatchItem &it = items[blockIdx.z];
    const double *Lm = static_cast<const double *>(it.in), *U = static_cast<const double *>(it.F);
    double *G = static_cast<double *>(it.out);
    if constexpr (PAIR) coef_grad_pairs<NT>(N, h, Lm, U, G);
    else coef_grad_cols(N, h, Lm, U, G);
}

__global__ __launch_bounds__(TB) void k_rim_grad(int N, double inv, const double *__restrict__ A, const double *__restrict__ Lm,
                                                 const double *__restrict__ Ubar, double *__restrict__ G)
{
    rim_grad_cols(N, inv, A, Lm, Ubar, G);
}

__global__ __launch_bounds__(TB) void k_rim_grad_b(int N, double inv, const NodeBatchItem *__restrict__ items)
{
    const NodeBatchItem &it = items[blockIdx.z];
    rim_grad_cols(N, inv, static_cast<const double *>(it.coarse), static_cast<const double *>(it.in),
                  static_cast<const double *>(it.F), static_cast<double *>(it.out));
}

inline bool use_pairs(int N) { return N % 2 == 0 && N >= PAIR_MIN_N; }
inline dim3 grid_for(int cols, int N, int n) { return dim3((cols + TB - 1) / TB, (N + HR - 1) / HR, n); }

}  // namespace

// ------------------------------------------------------------------ launchers
void coef_grad(hipStream_t s, int N, double h, const double *lam, const double *U, double *gA)
{
    const bool pairs = use_pairs(N), nt = pairs && N >= NT_MIN_N;
    const dim3 g = grid_for(pairs ? N / 2 : N, N, 1), b(TB);
    if (nt) hipLaunchKernelGGL((k_coef_grad<true, true>), g, b, 0, s, N, h, lam, U, gA);
    else if (pairs) hipLaunchKernelGGL((k_coef_grad<true, false>), g, b, 0, s, N, h, lam, U, gA);
    else hipLaunchKernelGGL((k_coef_grad<false, false>), g, b, 0, s, N, h, lam, U, gA);
}

void coef_grad_batch(hipStream_t s, int n, int N, double h, const NodeBatchItem *items)
{
    const bool pairs = use_pairs(N), nt = pairs && N >= NT_MIN_N;
    const dim3 g = grid_for(pairs ? N / 2 : N, N, n), b(TB);
    if (nt) hipLaunchKernelGGL((k_coef_grad_b<true, true>), g, b, 0, s, N, h, items);
    else if (pairs) hipLaunchKernelGGL((k_coef_grad_b<true, false>), g, b, 0, s, N, h, items);
    else hipLaunchKernelGGL((k_coef_grad_b<false, false>), g, b, 0, s, N, h, items);
}

void rim_grad(hipStream_t s, int N, double inv, const double *A, const double *lam, const double *Ubar, double *gU)
{
    hipLaunchKernelGGL(k_rim_grad, grid_for(N, N, 1), dim3(TB), 0, s, N, inv, A, lam, Ubar, gU);
}

void rim_grad_batch(hipStream_t s, int n, int N, double inv, const NodeBatchItem *items)
{
    hipLaunchKernelGGL(k_rim_grad_b, grid_for(N, N, n), dim3(TB), 0, s, N, inv, items);
}

}  // namespace k
}  // namespace mg
