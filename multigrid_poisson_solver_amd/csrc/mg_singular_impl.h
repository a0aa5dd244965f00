// mg_singular_impl.h -- the point code of the pure Neumann problem's own kernels (include/mg_singular.h; kernels and launchers:
// mg_singular_kernels.hip): the trapezoid-weighted sum in the partition of the norms, and the shift by a constant that lives in
// device memory.  The shapes are mg_bc_impl.h's streaming bodies without their windows: a lane walks 4 rows down its column
// (any N) or its column pair (even N from PAIR_MIN_N on, 16-byte accesses).  wave_sum / block_sum are mg_varcoef_impl.h's, so
// the order of a sum here is the order of the norms; mean_weight is mg_bc_impl.h's, shared with the coarse solve's prologue.
#ifndef MG_SINGULAR_IMPL_H
#define MG_SINGULAR_IMPL_H

#include "mg_bc_impl.h"

namespace mg {
namespace k {

namespace {

// per-block partial sums of w*X (include/mg_singular.h, "Summation order"); nothing but the partials is written.
// NT: X comes in through non-temporal loads
template <bool PAIR, bool NT>
__device__ __forceinline__ void wsum_body(int N, const double *__restrict__ X, double *__restrict__ part)
{
    double acc = 0.0;
    if constexpr (!PAIR) {
        const int c = blockIdx.x * TB + threadIdx.x;
        const int r0 = blockIdx.y * ROWS_PB;
        if (c < N) {
#pragma unroll
            for (int i = 0; i < ROWS_PB; ++i) {
                const int r = r0 + i;
                if (r < N) acc = acc + mean_weight(r, c, N) * X[(size_t)r * N + c];
            }
        }
    } else {
        const int c = 2 * (blockIdx.x * TB + threadIdx.x);
        const int r0 = blockIdx.y * PR;
        if (c < N) {   // (N even: c + 1 < N too)
#pragma unroll
            for (int i = 0; i < PR; ++i) {
                const int r = r0 + i;
                if (r < N) {
                    const double2_v x = load_f<NT>(X + (size_t)r * N + c);
                    acc = acc + mean_weight(r, c, N) * x.x;
                    acc = acc + mean_weight(r, c + 1, N) * x.y;
                }
            }
        }
    }
    const double s = block_sum(acc);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// second stage: ONE block sums the n partials in a fixed order; out[0] = mean_w = sum / sw, out[1] = mean_w - target
__device__ __forceinline__ void wsum_finish_body(const double *__restrict__ part, size_t n, double sw, double target,
                                                 double *__restrict__ out)
{
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) acc = acc + part[i];
    const double s = block_sum(acc);
    if (threadIdx.x == 0) {
        const double m = s / sw;
        out[0] = m;
        out[1] = m - target;
    }
}

// Xout = Xin - *c at every point.  Xout may be Xin (no __restrict__ on the two): a lane reads a point before it writes it and
// touches no other lane's points.  NT: non-temporal stores
template <bool PAIR, bool NT>
__device__ __forceinline__ void shift_body(int N, const double *Xin, const double *__restrict__ cdev, double *Xout)
{
    const double cv = *cdev;
    if constexpr (!PAIR) {
        const int c = blockIdx.x * TB + threadIdx.x;
        const int r0 = blockIdx.y * ROWS_PB;
        if (c >= N) return;
#pragma unroll
        for (int i = 0; i < ROWS_PB; ++i) {
            const int r = r0 + i;
            if (r < N) {
                const size_t p = (size_t)r * N + c;
                Xout[p] = Xin[p] - cv;
            }
        }
    } else {
        const int c = 2 * (blockIdx.x * TB + threadIdx.x);
        const int r0 = blockIdx.y * PR;
        if (c >= N) return;
#pragma unroll
        for (int i = 0; i < PR; ++i) {
            const int r = r0 + i;
            if (r < N) {
                const size_t p = (size_t)r * N + c;
                double2_v v = *reinterpret_cast<const double2_v *>(Xin + p);
                v.x = v.x - cv;
                v.y = v.y - cv;
                if (NT) __builtin_nontemporal_store(v, reinterpret_cast<double2_v *>(Xout + p));
                else *reinterpret_cast<double2_v *>(Xout + p) = v;
            }
        }
    }
}

}  // namespace

}  // namespace k
}  // namespace mg

#endif /* MG_SINGULAR_IMPL_H */
