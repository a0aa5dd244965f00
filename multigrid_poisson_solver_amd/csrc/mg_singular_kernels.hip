// mg_singular_kernels.hip -- fp64 kernels of the pure Neumann problem (include/mg_singular.h; driven by mg_solve.cpp): the
// trapezoid-weighted mean of a field (k_wsum into per-block partials, k_wsum_finish in a fixed order, the constant formed on the
// device) and the shift of a field by that constant (k_shift).  Built with -ffp-contract=off like every kernel file.  Both
// stream the field once: 8 bytes per point the sum, 16 the shift.  The forms are the boundary kernels': one column per lane
// for any N, column pairs with 16-byte accesses for even N from PAIR_MIN_N on, and from NT_MIN_N on the sum loads and the
// shift stores non-temporally.  The projected coarse solve is k_gs_relative_bc's twin in mg_bc_kernels.hip.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_singular_impl.h"

namespace mg {
namespace k {

namespace {

// FORM 0: one column per lane; 1: column pairs; 2: column pairs, non-temporal
template <int FORM>
__global__ __launch_bounds__(TB) void k_wsum(int N, const double *__restrict__ X, double *__restrict__ part)
{
    wsum_body<FORM != 0, FORM == 2>(N, X, part);
}

__global__ __launch_bounds__(1024) void k_wsum_finish(const double *__restrict__ part, size_t n, double sw, double target,
                                                      double *__restrict__ out)
{
    wsum_finish_body(part, n, sw, target, out);
}

template <int FORM>
__global__ __launch_bounds__(TB) void k_shift(int N, const double *Xin, const double *__restrict__ c, double *Xout)
{
    shift_body<FORM != 0, FORM == 2>(N, Xin, c, Xout);
}

// the form of a launch by the boundary launchers' rule
int form_of(int N) { return !use_pairs(N) ? 0 : (N >= NT_MIN_N ? 2 : 1); }

}  // namespace

void weighted_mean(hipStream_t s, int N, const double *X, double target, double *part, double *out)
{
    const size_t np = resnorm_partials(N);   // (the partition of the norms)
    const dim3 blk(TB);
    switch (form_of(N)) {
    case 0: hipLaunchKernelGGL(k_wsum<0>, grid_rows(N), blk, 0, s, N, X, part); break;
    case 1: hipLaunchKernelGGL(k_wsum<1>, grid_pairs(N), blk, 0, s, N, X, part); break;
    default: hipLaunchKernelGGL(k_wsum<2>, grid_pairs(N), blk, 0, s, N, X, part); break;
    }
    hipLaunchKernelGGL(k_wsum_finish, dim3(1), dim3(1024), 0, s, part, np, (double)(N - 1) * (double)(N - 1), target, out);
}

void shift_by(hipStream_t s, int N, const double *Xin, const double *c, double *Xout)
{
    const dim3 blk(TB);
    switch (form_of(N)) {
    case 0: hipLaunchKernelGGL(k_shift<0>, grid_rows(N), blk, 0, s, N, Xin, c, Xout); break;
    case 1: hipLaunchKernelGGL(k_shift<1>, grid_pairs(N), blk, 0, s, N, Xin, c, Xout); break;
    default: hipLaunchKernelGGL(k_shift<2>, grid_pairs(N), blk, 0, s, N, Xin, c, Xout); break;
    }
}

}  // namespace k
}  // namespace mg
