// mg_newton_impl.h -- the point code of the semilinear residual (include/mg_newton.h; kernels and launcher:
// mg_newton_kernels.hip).  The operator and the block sums are mg_varcoef_impl.h's (Faces, faces, bracket, block_sum,
// resnorm_finish_body), included, not copied; exp is mg_exp_libm.h's.  One streaming pass forms, per point, the trial value
// v = U + t*dlt, the Newton matrix's diagonal term S = kw*g'(v), the Newton right-hand side D = (F + kw*g(v)) - inv*b(v) and
// the partial sums of D^2, in the shapes of the reaction kernels (mg_varcoef_impl.h): a lane walks 4 rows down its column
// (any N) or its column pair (even N from PAIR_MIN_N on, 16-byte accesses) with a rolling window of three rows in registers.
// The window holds v, not U and dlt apart: a row of U and of dlt is combined as it is loaded, once, by the expression every
// other use of that point evaluates, so the step form carries one window more than the sweep's (a, v) and no third.
#ifndef MG_NEWTON_IMPL_H
#define MG_NEWTON_IMPL_H

#include "mg_exp_libm.h"
#include "mg_varcoef_impl.h"

namespace mg {
namespace k {

namespace {

enum NwKind { NW_CUBIC = 0, NW_SINH = 1, NW_EXP = 2 };   // MG_NEWTON_CUBIC / _SINH / _EXP

struct NwArgs {
    int N;
    double inv, sd, kappa, t;
    const double *A, *W, *U, *dlt, *F;   // A, W, dlt: read only by the forms that have them
    double *V, *D, *S, *part;            // V: written only by the step form
};

// g and g' at one point (include/mg_newton.h's table), every operation rounded once
template <int KIND>
__device__ __forceinline__ void nw_g(double u, double *g, double *gp)
{
    if constexpr (KIND == NW_CUBIC) {
        const double q = u * u;
        *g = q * u;
        *gp = 3.0 * q;
    } else if constexpr (KIND == NW_SINH) {
        const double e = exp_libm(u);
        const double f = 1.0 / e;
        *g = 0.5 * (e - f);
        *gp = 0.5 * (e + f);
    } else {
        const double e = exp_libm(u);
        *g = e;
        *gp = e;
    }
}

// v at (r, c), r inside the grid: U on the rim (the step never moves boundary data, and a -0.0 there stays -0.0), else
// U + t*dlt with the product rounded before the sum
template <bool HAS_STEP>
__device__ __forceinline__ double nw_value(const NwArgs &x, int r, int c)
{
    const size_t p = (size_t)r * x.N + c;
    const double u = x.U[p];
    if constexpr (HAS_STEP) {
        const double s = u + x.t * x.dlt[p];
        return rim(r, c, x.N) ? u : s;
    }
    return u;
}

// ---------------------------------------------------------------- one column per lane (any N)
template <int KIND, bool HAS_A, bool HAS_W, bool HAS_STEP>
__device__ __forceinline__ double nw_cols(const NwArgs &x)
{
    const int N = x.N;
    const int c = blockIdx.x * TB + threadIdx.x;
    double acc = 0.0;
    if (c >= N) return acc;
    const int r0 = blockIdx.y * ROWS_PB;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 1 < N ? c + 1 : N - 1;
    const bool col_in = c > 0 && c < N - 1;
    const double *__restrict__ A = x.A;
    const double *__restrict__ W = x.W;
    const double *__restrict__ F = x.F;
    auto clamp = [&](int r) { return r < 0 ? 0 : (r < N ? r : N - 1); };   // (rows beyond the grid: clamped, never used)
    double a_prv = 1.0, a_mid = 1.0;
    if constexpr (HAS_A) {
        a_prv = A[(size_t)clamp(r0 - 1) * N + c];
        a_mid = A[(size_t)clamp(r0) * N + c];
    }
    double v_prv = nw_value<HAS_STEP>(x, clamp(r0 - 1), c), v_mid = nw_value<HAS_STEP>(x, clamp(r0), c);
#pragma unroll
    for (int i = 0; i < ROWS_PB; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        double a_nxt = 1.0;
        if constexpr (HAS_A) a_nxt = A[(size_t)clamp(r + 1) * N + c];
        const double v_nxt = nw_value<HAS_STEP>(x, clamp(r + 1), c);
        const size_t line = (size_t)r * N, p = line + c;
        double kw = x.kappa;
        if constexpr (HAS_W) kw = x.kappa * W[p];
        double g, gp;
        nw_g<KIND>(v_mid, &g, &gp);
        x.S[p] = kw * gp;
        double d = 0.0;
        if (col_in && r > 0 && r < N - 1) {
            double a_east = 1.0, a_west = 1.0;
            if constexpr (HAS_A) {
                a_east = A[line + cr];
                a_west = A[line + cl];
            }
            const Faces f = faces(a_mid, a_nxt, a_prv, a_east, a_west, x.sd);
            const double lin = x.inv * bracket(f, v_mid, v_nxt, v_prv, nw_value<HAS_STEP>(x, r, cr), nw_value<HAS_STEP>(x, r, cl));
            d = (F[p] + kw * g) - lin;
            acc += d * d;
        }
        x.D[p] = d;
        if constexpr (HAS_STEP) x.V[p] = v_mid;
        a_prv = a_mid;
        a_mid = a_nxt;
        v_prv = v_mid;
        v_mid = v_nxt;
    }
    return acc;
}

// ---------------------------------------------------------------- two columns per lane, 16-byte accesses
// (even N, 16-byte aligned arrays, as vc_pairs).  NT: F and w through non-temporal loads, D, S and V through non-temporal
// stores.  U, dlt and a are windows -- every row is read by the block above and the block below as well -- and stay ordinary.
template <bool NT>
__device__ __forceinline__ void nw_store(double *p, double2_v v)
{
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<double2_v *>(p));
    else *reinterpret_cast<double2_v *>(p) = v;
}

template <int KIND, bool NT, bool HAS_A, bool HAS_W, bool HAS_STEP>
__device__ __forceinline__ double nw_pairs(const NwArgs &x)
{
    const int N = x.N;
    const int c = 2 * (blockIdx.x * TB + threadIdx.x);
    double acc = 0.0;
    if (c >= N) return acc;
    const int r0 = blockIdx.y * PR;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 2 < N ? c + 2 : N - 1;
    const double *__restrict__ A = x.A;
    const double *__restrict__ W = x.W;
    const double *__restrict__ F = x.F;
    auto clamp = [&](int r) { return r < 0 ? 0 : (r < N ? r : N - 1); };
    auto a_pair = [&](int r) { return *reinterpret_cast<const double2_v *>(A + (size_t)clamp(r) * N + c); };
    auto v_pair = [&](int r) {
        r = clamp(r);
        const size_t p = (size_t)r * N + c;
        double2_v u = *reinterpret_cast<const double2_v *>(x.U + p);
        if constexpr (HAS_STEP) {
            const double2_v dl = *reinterpret_cast<const double2_v *>(x.dlt + p);
            const bool row_rim = r == 0 || r == N - 1;
            const double sx = u.x + x.t * dl.x, sy = u.y + x.t * dl.y;
            if (!(row_rim || c == 0)) u.x = sx;
            if (!(row_rim || c + 1 == N - 1)) u.y = sy;
        }
        return u;
    };
    const double2_v ones = {1.0, 1.0};
    double2_v a_prv = ones, a_mid = ones;
    if constexpr (HAS_A) {
        a_prv = a_pair(r0 - 1);
        a_mid = a_pair(r0);
    }
    double2_v v_prv = v_pair(r0 - 1), v_mid = v_pair(r0);
#pragma unroll
    for (int i = 0; i < PR; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        double2_v a_nxt = ones;
        if constexpr (HAS_A) a_nxt = a_pair(r + 1);
        const double2_v v_nxt = v_pair(r + 1);
        const size_t line = (size_t)r * N, p = line + c;
        double kwx = x.kappa, kwy = x.kappa;
        if constexpr (HAS_W) {
            const double2_v w = load_f<NT>(W + p);
            kwx = x.kappa * w.x;
            kwy = x.kappa * w.y;
        }
        double gx, gpx, gy, gpy;
        nw_g<KIND>(v_mid.x, &gx, &gpx);
        nw_g<KIND>(v_mid.y, &gy, &gpy);
        const double2_v s = {kwx * gpx, kwy * gpy};
        nw_store<NT>(x.S + p, s);
        double2_v d = {0.0, 0.0};
        if (r > 0 && r < N - 1) {
            const double2_v f = load_f<NT>(F + p);
            if (c > 0) {
                const Faces fc = faces(a_mid.x, a_nxt.x, a_prv.x, a_mid.y, HAS_A ? A[line + cl] : 1.0, x.sd);
                const double lin = x.inv * bracket(fc, v_mid.x, v_nxt.x, v_prv.x, v_mid.y, nw_value<HAS_STEP>(x, r, cl));
                d.x = (f.x + kwx * gx) - lin;
                acc += d.x * d.x;
            }
            if (c + 1 < N - 1) {
                const Faces fc = faces(a_mid.y, a_nxt.y, a_prv.y, HAS_A ? A[line + cr] : 1.0, a_mid.x, x.sd);
                const double lin = x.inv * bracket(fc, v_mid.y, v_nxt.y, v_prv.y, nw_value<HAS_STEP>(x, r, cr), v_mid.x);
                d.y = (f.y + kwy * gy) - lin;
                acc += d.y * d.y;
            }
        }
        nw_store<NT>(x.D + p, d);
        if constexpr (HAS_STEP) nw_store<NT>(x.V + p, v_mid);
        a_prv = a_mid;
        a_mid = a_nxt;
        v_prv = v_mid;
        v_mid = v_nxt;
    }
    return acc;
}

// the whole pass of one block: its points, then its partial of the sum of D^2 in the place and order of resnorm_vc_body
template <int KIND, bool PAIR, bool NT, bool HAS_A, bool HAS_W, bool HAS_STEP>
__device__ __forceinline__ void nw_body(const NwArgs &x)
{
    double acc;
    if constexpr (PAIR) acc = nw_pairs<KIND, NT, HAS_A, HAS_W, HAS_STEP>(x);
    else acc = nw_cols<KIND, HAS_A, HAS_W, HAS_STEP>(x);
    const double sum = block_sum(acc);
    if (threadIdx.x == 0) x.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

}  // namespace

}  // namespace k
}  // namespace mg

#endif /* MG_NEWTON_IMPL_H */
