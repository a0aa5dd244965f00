// mg_adjoint_rx_impl.h -- the point code of the source gradient (include/mg_adjoint_rx.h; kernels and launchers:
// mg_adjoint_rx_kernels.hip).  g and exp are mg_newton_impl.h's (nw_g, exp_libm), the block sums mg_varcoef_impl.h's
// (block_sum), included, not copied.  Pointwise: per interior point gv = g(U), m = lam*gv, G = kappa*m and the term w*m (or
// m) of the sum; +0.0 for both on the rim, where g is not evaluated.  No window, no LDS beyond block_sum's, no scratch.  The
// shapes are the pass's (nw_cols / nw_pairs): a lane walks ROWS_PB rows down its column (any N) or PR rows down its column
// pair (even N from PAIR_MIN_N on, 16-byte accesses), so a block's partial lands where the pass's norm partial lands and
// the sum has the norm's partition and order.
#ifndef MG_ADJOINT_RX_IMPL_H
#define MG_ADJOINT_RX_IMPL_H

#include "mg_newton_impl.h"

namespace mg {
namespace k {

namespace {

constexpr int SG_LINEAR = 3;   // MG_GRAD_LINEAR: g(u) = u, beside NW_CUBIC / NW_SINH / NW_EXP

struct SgArgs {
    int N;
    double kappa;
    const double *W, *Lm, *U;   // W: read only by the forms that have it
    double *G, *part;
};

// g at one point: nw_g's expressions (its g' is dead code here), or u itself
template <int KIND>
__device__ __forceinline__ double sg_g(double u)
{
    if constexpr (KIND == SG_LINEAR) {
        return u;
    } else {
        double g, gp;
        nw_g<KIND>(u, &g, &gp);
        return g;
    }
}

// ---------------------------------------------------------------- one column per lane (any N)
template <int KIND, bool HAS_W>
__device__ __forceinline__ double sg_cols(const SgArgs &x)
{
    const int N = x.N;
    const int c = blockIdx.x * TB + threadIdx.x;
    double acc = 0.0;
    if (c >= N) return acc;
    const int r0 = blockIdx.y * ROWS_PB;
    const bool col_in = c > 0 && c < N - 1;
    const double *__restrict__ W = x.W;
    const double *__restrict__ Lm = x.Lm;
    const double *__restrict__ U = x.U;
#pragma unroll
    for (int i = 0; i < ROWS_PB; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        const size_t p = (size_t)r * N + c;
        const double lam = Lm[p], u = U[p];   // (the rim of lam: loaded, never used)
        double g = 0.0;
        if (col_in && r > 0 && r < N - 1) {
            const double m = lam * sg_g<KIND>(u);
            g = x.kappa * m;
            if constexpr (HAS_W) acc += W[p] * m;
            else acc += m;
        }
        x.G[p] = g;
    }
    return acc;
}

// ---------------------------------------------------------------- two columns per lane, 16-byte accesses
// (even N, 16-byte aligned arrays, as nw_pairs).  NT: w through non-temporal loads, G through non-temporal stores.
template <int KIND, bool NT, bool HAS_W>
__device__ __forceinline__ double sg_pairs(const SgArgs &x)
{
    const int N = x.N;
    const int c = 2 * (blockIdx.x * TB + threadIdx.x);
    double acc = 0.0;
    if (c >= N) return acc;
    const int r0 = blockIdx.y * PR;
    const double *__restrict__ W = x.W;
    const double *__restrict__ Lm = x.Lm;
    const double *__restrict__ U = x.U;
#pragma unroll
    for (int i = 0; i < PR; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        const size_t p = (size_t)r * N + c;
        const double2_v lam = load_f<false>(Lm + p), u = load_f<false>(U + p);
        double2_v g = {0.0, 0.0};
        if (r > 0 && r < N - 1) {
            double2_v w = {1.0, 1.0};
            if constexpr (HAS_W) w = load_f<NT>(W + p);
            if (c > 0) {
                const double m = lam.x * sg_g<KIND>(u.x);
                g.x = x.kappa * m;
                if constexpr (HAS_W) acc += w.x * m;
                else acc += m;
            }
            if (c + 1 < N - 1) {
                const double m = lam.y * sg_g<KIND>(u.y);
                g.y = x.kappa * m;
                if constexpr (HAS_W) acc += w.y * m;
                else acc += m;
            }
        }
        nw_store<NT>(x.G + p, g);
    }
    return acc;
}

// the whole launch of one block: its points, then its partial of the sum in the place and order of nw_body
template <int KIND, bool PAIR, bool NT, bool HAS_W>
__device__ __forceinline__ void sg_body(const SgArgs &x)
{
    double acc;
    if constexpr (PAIR) acc = sg_pairs<KIND, NT, HAS_W>(x);
    else acc = sg_cols<KIND, HAS_W>(x);
    const double sum = block_sum(acc);
    if (threadIdx.x == 0) x.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// second stage: resnorm_finish_body without the square root -- *out = the sum of the n partials, one block, fixed order
__device__ __forceinline__ void sg_finish_body(const double *__restrict__ part, size_t n, double *__restrict__ out)
{
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) acc += part[i];
    const double s = block_sum(acc);
    if (threadIdx.x == 0) *out = s;
}

}  // namespace

}  // namespace k
}  // namespace mg

#endif /* MG_ADJOINT_RX_IMPL_H */
