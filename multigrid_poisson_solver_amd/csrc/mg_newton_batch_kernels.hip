// mg_newton_batch_kernels.hip -- the batched form of the semilinear pass (include/mg_newton_batch.h; driven by
// mg_solve_batch.cpp: mg_batch_solver_newton, mg_nonlinearResidual_batch): ONE launch runs k_newton_residual of
// mg_newton_kernels.hip for every instance of the launch, and one launch finishes their norms.  The __device__ bodies are the
// ones of mg_newton_impl.h (nw_body over nw_cols / nw_pairs), compiled here with the same flags (-ffp-contract=off): an instance
// runs the code, the block partition (grid x, y) and the summation order of its single launch, so its V, D, S and norm are the
// single pass's bit for bit.  blockIdx.z picks the instance; its arrays and its kappa come from a NewtonBatchItem of its own in
// device memory (mg_internal.h), its partials go to part + z*resnorm_partials(N).  The item is uniform over the block: it is
// read once, through scalar loads, into the NwArgs the body takes by value -- no row of the walk goes back to the table.
// N, inv, sd and t are the same for every instance of a launch and stay kernel arguments (the driver's line search runs round k
// at t = 2^-k over the instances that have not accepted yet).  Within one launch either every instance has a coefficient, a
// weight, a step, or none has: HAS_A, HAS_W and HAS_STEP are template parameters chosen per launch, and a slot the form does not
// have is not read.  The forms are the single launcher's: one column per lane for any N, column pairs from PAIR_MIN_N on (even
// N), non-temporal from NT_MIN_N on.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_newton_impl.h"

namespace mg {
namespace k {

namespace {

template <int KIND, bool PAIR, bool NT, bool HAS_A, bool HAS_W, bool HAS_STEP>
__global__ __launch_bounds__(TB) void k_newton_residual_b(int N, double inv, double sd, double t, const NewtonBatchItem *__restrict__ items,
                                                          double *__restrict__ part, size_t np)
{
    const NewtonBatchItem &it = items[blockIdx.z];
    const NwArgs x{N, inv, sd, it.kappa, t, HAS_A ? it.A : nullptr, HAS_W ? it.W : nullptr, it.U, HAS_STEP ? it.dlt : nullptr, it.F,
                   HAS_STEP ? it.V : nullptr, it.D, it.S, part + blockIdx.z * np};
    nw_body<KIND, PAIR, NT, HAS_A, HAS_W, HAS_STEP>(x);
}

// out[i] = sqrt(sum of instance i's np partials): one block per instance, each the single-instance finish
__global__ __launch_bounds__(1024) void k_newton_norm_finish_b(const double *__restrict__ part, size_t np, double *__restrict__ out)
{
    resnorm_finish_body(part + blockIdx.x * np, np, out + blockIdx.x);
}

struct Launch {
    hipStream_t s;
    dim3 g;
    int N;
    double inv, sd, t;
    const NewtonBatchItem *items;
    double *part;
    size_t np;
    int sel;   // HAS_A: 4, HAS_W: 2, HAS_STEP: 1
};

template <int KIND, bool PAIR, bool NT>
void launch_form(const Launch &l)
{
#define MG_NWB_CASE(SEL, HA, HW, HS)                                                                                              \
    case SEL:                                                                                                                     \
        hipLaunchKernelGGL((k_newton_residual_b<KIND, PAIR, NT, HA, HW, HS>), l.g, dim3(TB), 0, l.s, l.N, l.inv, l.sd, l.t, l.items, \
                           l.part, l.np);                                                                                         \
        break
    switch (l.sel) {
        MG_NWB_CASE(0, false, false, false);
        MG_NWB_CASE(1, false, false, true);
        MG_NWB_CASE(2, false, true, false);
        MG_NWB_CASE(3, false, true, true);
        MG_NWB_CASE(4, true, false, false);
        MG_NWB_CASE(5, true, false, true);
        MG_NWB_CASE(6, true, true, false);
        MG_NWB_CASE(7, true, true, true);
    }
#undef MG_NWB_CASE
}

// the form newton_residual chooses for this N, its grid with the instances in z
template <int KIND>
void launch_kind(Launch l, int n)
{
    const int N = l.N;
    l.g = use_pairs(N) ? grid_pairs(N) : grid_rows(N);
    l.g.z = n;
    if (!use_pairs(N)) launch_form<KIND, false, false>(l);
    else if (N >= NT_MIN_N) launch_form<KIND, true, true>(l);
    else launch_form<KIND, true, false>(l);
}

}  // namespace

// ------------------------------------------------------------------ launcher
void newton_residual_batch(hipStream_t s, int n, int N, double inv, double sd, int kind, bool has_a, bool has_w, bool has_step, double t,
                           const NewtonBatchItem *items, double *part, double *out)
{
    const size_t np = resnorm_partials(N);   // (the grid below is the norm kernels' of this N)
    const Launch l{s, dim3(), N, inv, sd, t, items, part, np, (has_a ? 4 : 0) | (has_w ? 2 : 0) | (has_step ? 1 : 0)};
    switch (kind) {
    case NW_CUBIC: launch_kind<NW_CUBIC>(l, n); break;
    case NW_SINH: launch_kind<NW_SINH>(l, n); break;
    default: launch_kind<NW_EXP>(l, n); break;
    }
    hipLaunchKernelGGL(k_newton_norm_finish_b, dim3(n), dim3(1024), 0, s, part, np, out);
}

}  // namespace k
}  // namespace mg
