// mg_newton_kernels.hip -- the fp64 kernel of the semilinear solve div(a grad U) - sigma*U - kappa*w*g(U) = F
// (include/mg_newton.h; driven by mg_solve.cpp: mg_solver_newton): ONE streaming pass that gives the outer Newton iteration
// everything it needs -- the trial value V = U + t*dlt, the nonlinear residual D = -N(V), the sum of D^2 and the diagonal term
// S = kappa*w*g'(V) of the next Newton matrix.  Built with -ffp-contract=off like every kernel file; the only fused
// multiply-adds are the explicit ones of exp_libm.  The shapes are the reaction kernels' (mg_reaction_kernels.hip): one column
// per lane for any N, column pairs with 16-byte accesses for even N from PAIR_MIN_N on, non-temporal from NT_MIN_N on for the
// streams a pass touches once (F, w in; D, S, V out).  Templated over the kind of g, the coefficient, the weight and the step:
// without a or w no array of ones is streamed, without a step dlt and V do not exist.  Memory-bound: per point the no-step
// form moves 32 B (U, F in; D, S out) + 8 B with a + 8 B with w, the step form 16 B more (dlt in, V out) -- 56 B with a,
// in place of an axpy pass (24 B) followed by a residual pass (40 B).
// The __device__ bodies live in mg_newton_impl.h, layered over mg_varcoef_impl.h.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_newton_impl.h"

namespace mg {
namespace k {

namespace {

template <int KIND, bool PAIR, bool NT, bool HAS_A, bool HAS_W, bool HAS_STEP>
__global__ __launch_bounds__(TB) void k_newton_residual(NwArgs x)
{
    nw_body<KIND, PAIR, NT, HAS_A, HAS_W, HAS_STEP>(x);
}

__global__ __launch_bounds__(1024) void k_newton_norm_finish(const double *__restrict__ part, size_t n, double *__restrict__ out)
{
    resnorm_finish_body(part, n, out);
}

// HAS_A, HAS_W, HAS_STEP from the pointers that are there
template <int KIND, bool PAIR, bool NT>
void launch_form(hipStream_t s, dim3 g, const NwArgs &x)
{
#define MG_NW_CASE(SEL, HA, HW, HS)                                                                       \
    case SEL: hipLaunchKernelGGL((k_newton_residual<KIND, PAIR, NT, HA, HW, HS>), g, dim3(TB), 0, s, x); break
    switch ((x.A ? 4 : 0) | (x.W ? 2 : 0) | (x.dlt ? 1 : 0)) {
        MG_NW_CASE(0, false, false, false);
        MG_NW_CASE(1, false, false, true);
        MG_NW_CASE(2, false, true, false);
        MG_NW_CASE(3, false, true, true);
        MG_NW_CASE(4, true, false, false);
        MG_NW_CASE(5, true, false, true);
        MG_NW_CASE(6, true, true, false);
        MG_NW_CASE(7, true, true, true);
    }
#undef MG_NW_CASE
}

template <int KIND>
void launch_kind(hipStream_t s, const NwArgs &x)
{
    const int N = x.N;
    if (!use_pairs(N)) launch_form<KIND, false, false>(s, grid_rows(N), x);
    else if (N >= NT_MIN_N) launch_form<KIND, true, true>(s, grid_pairs(N), x);
    else launch_form<KIND, true, false>(s, grid_pairs(N), x);
}

}  // namespace

// ------------------------------------------------------------------ launcher
void newton_residual(hipStream_t s, int N, double inv, double sd, int kind, double kappa, const double *A, const double *W,
                     const double *U, const double *dlt, double t, const double *F, double *V, double *D, double *S, double *part,
                     double *out)
{
    const NwArgs x{N, inv, sd, kappa, t, A, W, U, dlt, F, V, D, S, part};
    switch (kind) {
    case NW_CUBIC: launch_kind<NW_CUBIC>(s, x); break;
    case NW_SINH: launch_kind<NW_SINH>(s, x); break;
    default: launch_kind<NW_EXP>(s, x); break;
    }
    // (the grid above is the norm kernels' of this N: resnorm_partials(N) partials)
    hipLaunchKernelGGL(k_newton_norm_finish, dim3(1), dim3(1024), 0, s, part, resnorm_partials(N), out);
}

}  // namespace k
}  // namespace mg
