// mg_adjoint_rx_kernels.hip -- the source gradient of the adjoint of reaction and semilinear solves (include/mg_adjoint_rx.h;
// driven by mg_adjoint_rx.cpp): ONE streaming launch turns the adjoint field lam and the forward solution U into
// G = kappa*(lam'*g(U)) and the partials of sum(w*(lam'*g(U))), a second one finishes the sum.  Built with -ffp-contract=off
// like every kernel file; the only fused multiply-adds are the explicit ones of exp_libm.  The forms are the semilinear
// pass's (mg_newton_kernels.hip) with its thresholds: one column per lane for any N, column pairs with 16-byte accesses for
// even N from PAIR_MIN_N on, from NT_MIN_N on non-temporal loads of w and non-temporal stores of G.  Templated over the kind
// of g and the weight: without w no array of ones is streamed.  Memory-bound: 24 B per point (lam, U in; G out), 32 B with w.
// The batched twins run the same bodies: blockIdx.z picks the instance, whose arrays and kappa come from a SrcGradItem in
// device memory (mg_internal.h) and whose partials go to part + z*resnorm_partials(N); the finish runs one block per
// instance.  Within one launch either every instance has a weight or none has.
// The __device__ bodies live in mg_adjoint_rx_impl.h, layered over mg_newton_impl.h.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_adjoint_rx_impl.h"

namespace mg {
namespace k {

namespace {

template <int KIND, bool PAIR, bool NT, bool HAS_W>
__global__ __launch_bounds__(TB) void k_src_grad(SgArgs x)
{
    sg_body<KIND, PAIR, NT, HAS_W>(x);
}

template <int KIND, bool PAIR, bool NT, bool HAS_W>
__global__ __launch_bounds__(TB) void k_src_grad_b(int N, const SrcGradItem *__restrict__ items, double *__restrict__ part, size_t np)
{
    const SrcGradItem &it = items[blockIdx.z];
    const SgArgs x{N, it.kappa, HAS_W ? it.W : nullptr, it.lam, it.U, it.G, part + blockIdx.z * np};
    sg_body<KIND, PAIR, NT, HAS_W>(x);
}

// out[i] = the sum of instance i's np partials: one block per instance, each the single-instance finish (grid 1)
__global__ __launch_bounds__(1024) void k_src_grad_finish(const double *__restrict__ part, size_t np, double *__restrict__ out)
{
    sg_finish_body(part + blockIdx.x * np, np, out + blockIdx.x);
}

// items == nullptr: the single launch on x; else the batched one (x carries N alone)
struct Launch {
    hipStream_t s;
    dim3 g;
    SgArgs x;
    const SrcGradItem *items;
    double *part;
    size_t np;
    bool has_w;
};

template <int KIND, bool PAIR, bool NT, bool HAS_W>
void launch_one(const Launch &l)
{
    if (l.items) hipLaunchKernelGGL((k_src_grad_b<KIND, PAIR, NT, HAS_W>), l.g, dim3(TB), 0, l.s, l.x.N, l.items, l.part, l.np);
    else hipLaunchKernelGGL((k_src_grad<KIND, PAIR, NT, HAS_W>), l.g, dim3(TB), 0, l.s, l.x);
}

template <int KIND, bool PAIR, bool NT>
void launch_form(const Launch &l)
{
    if (l.has_w) launch_one<KIND, PAIR, NT, true>(l);
    else launch_one<KIND, PAIR, NT, false>(l);
}

// the form newton_residual chooses for this N, its grid with the instances in z
template <int KIND>
void launch_kind(Launch l, int n)
{
    const int N = l.x.N;
    l.g = use_pairs(N) ? grid_pairs(N) : grid_rows(N);
    l.g.z = n;
    if (!use_pairs(N)) launch_form<KIND, false, false>(l);
    else if (N >= NT_MIN_N) launch_form<KIND, true, true>(l);
    else launch_form<KIND, true, false>(l);
}

void launch(const Launch &l, int kind, int n)
{
    switch (kind) {
    case NW_CUBIC: launch_kind<NW_CUBIC>(l, n); break;
    case NW_SINH: launch_kind<NW_SINH>(l, n); break;
    case NW_EXP: launch_kind<NW_EXP>(l, n); break;
    default: launch_kind<SG_LINEAR>(l, n); break;
    }
}

}  // namespace

// ------------------------------------------------------------------ launchers
void src_grad(hipStream_t s, int N, int kind, double kappa, const double *W, const double *lam, const double *U, double *G, double *part,
              double *out)
{
    const size_t np = resnorm_partials(N);   // (the grid is the norm kernels' of this N)
    launch(Launch{s, dim3(), SgArgs{N, kappa, W, lam, U, G, part}, nullptr, part, np, W != nullptr}, kind, 1);
    hipLaunchKernelGGL(k_src_grad_finish, dim3(1), dim3(1024), 0, s, part, np, out);
}

void src_grad_batch(hipStream_t s, int n, int N, int kind, bool has_w, const SrcGradItem *items, double *part, double *out)
{
    const size_t np = resnorm_partials(N);
    launch(Launch{s, dim3(), SgArgs{N, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr}, items, part, np, has_w}, kind, n);
    hipLaunchKernelGGL(k_src_grad_finish, dim3(n), dim3(1024), 0, s, part, np, out);
}

}  // namespace k
}  // namespace mg
