// mg_krylov_impl.h -- the point code of the Krylov kernels (include/mg_krylov.h), shared by the single-instance kernels
// (mg_krylov_kernels.hip) and their batched forms (mg_krylov_batch_kernels.hip): both translation units compile THESE bodies
// with the same flags (-ffp-contract=off), so an instance of a batched launch runs the code, the block partition, the
// per-block partial slots and the summation order of its single launch and gives the same bits.  A body takes the arrays of
// one instance as arguments and reads blockIdx.x / blockIdx.y only as (column block, row block) of that instance; which
// instance a block works on is the caller's business (blockIdx.z of the batched streaming kernels, blockIdx.x / .y of the
// one-block finish kernels).
// Shapes as in mg_varcoef_impl.h: a lane walks 4 rows down its column (any N) or its column pair (even N from PAIR_MIN_N on,
// 16-byte accesses).  Only interior points are touched: the edge lanes of the pair form load their pair and use -- and
// store -- its interior half alone (an 8-byte store), so the rim of no array is ever written and a NaN there reaches no
// result.  K is a compile-time bucket (0 .. 15) and kk <= K the number of stored directions of THIS instance: the single
// kernels pass kk = K as a constant (every guard folds away), a batched launch passes the k its block read from the
// instance's table entry -- uniform over the block, so `j < kk` is a scalar branch and every barrier stays block-uniform.
// The K accumulators are indexed by constants and live in registers either way: no scratch.  Where the stored directions
// lie: slot j of the solver's storage, a kernel argument, plus the instance's offset in the slot (0 in the single solver).
// Non-temporal loads are a compile-time property of a stream, not of N (as k_residual_pairs): in the pair form the stored
// directions Q_j, Z_j of the orthogonalisation and z_k, q_k of the update -- which the next launch does not read again --
// come through non-temporal loads; everything the next launch re-reads is loaded and stored normally.
// Everything here sits in an unnamed namespace: each translation unit has its own copy.
#ifndef MG_KRYLOV_IMPL_H
#define MG_KRYLOV_IMPL_H

#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_solver_common.h"

namespace mg {
namespace k {

namespace {

// One lane's points of a row: a double (PAIR = false) or two neighbouring columns (PAIR = true) of which mx / my tell
// which are interior.  A value outside the mask is never summed and never stored.
template <bool PAIR>
struct Pt;
template <>
struct Pt<false> {
    typedef double V;
    static __device__ __forceinline__ V ld(const double *p) { return *p; }
    static __device__ __forceinline__ V ld_nt(const double *p) { return *p; }
    static __device__ __forceinline__ void st(double *p, V v, bool, bool) { *p = v; }
    static __device__ __forceinline__ void add(double &acc, V v, bool, bool) { acc += v; }
};
template <>
struct Pt<true> {
    typedef double2_v V;
    static __device__ __forceinline__ V ld(const double *p) { return *reinterpret_cast<const double2_v *>(p); }
    static __device__ __forceinline__ V ld_nt(const double *p) { return __builtin_nontemporal_load(reinterpret_cast<const double2_v *>(p)); }
    static __device__ __forceinline__ void st(double *p, V v, bool mx, bool my)
    {
        if (mx && my) *reinterpret_cast<double2_v *>(p) = v;
        else if (mx) p[0] = v.x;
        else if (my) p[1] = v.y;
    }
    static __device__ __forceinline__ void add(double &acc, V v, bool mx, bool my)
    {
        acc += mx ? v.x : 0.0;
        acc += my ? v.y : 0.0;
    }
};

// body(p, mx, my) for every row of this lane that holds an interior point; p: the element index of the lane's first column
template <bool PAIR, typename Body>
__device__ __forceinline__ void for_rows(int N, Body body)
{
    if constexpr (!PAIR) {
        const int c = blockIdx.x * TB + threadIdx.x;
        const int r0 = blockIdx.y * ROWS_PB;
        if (c > 0 && c < N - 1) {
#pragma unroll
            for (int i = 0; i < ROWS_PB; ++i) {
                const int r = r0 + i;
                if (r > 0 && r < N - 1) body((size_t)r * N + c, true, true);
            }
        }
    } else {
        const int c = 2 * (blockIdx.x * TB + threadIdx.x);   // (N even: c + 1 <= N - 1 whenever c < N)
        const int r0 = blockIdx.y * PR;
        if (c < N) {
            const bool mx = c > 0, my = c + 1 < N - 1;
#pragma unroll
            for (int i = 0; i < PR; ++i) {
                const int r = r0 + i;
                if (r > 0 && r < N - 1) body((size_t)r * N + c, mx, my);
            }
        }
    }
}

// the slot of this block among its instance's partials, and their number per sum (gridDim.z, the instances, plays no part)
__device__ __forceinline__ size_t block_slot() { return (size_t)blockIdx.y * gridDim.x + blockIdx.x; }
__device__ __forceinline__ size_t block_count() { return (size_t)gridDim.x * gridDim.y; }

// where one instance's stored directions lie: slot j of the solver's storage (a kernel argument, indexed by constants) at the
// instance's offset in it -- 0 for the single solver, whose slots hold one instance
struct Dirs {
    const KrylovVecs &v;
    size_t off;
    __device__ __forceinline__ const double *q(int j) const { return v.q[j] + off; }
    __device__ __forceinline__ const double *z(int j) const { return v.z[j] + off; }
};

// part[j*nb + block] = this block's share of <q, Q_j>, j < kk
template <int K, bool PAIR>
__device__ __forceinline__ void krylov_dots_body(int N, int kk, const double *__restrict__ q, const Dirs &d, double *__restrict__ part)
{
    typedef Pt<PAIR> P;
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    for_rows<PAIR>(N, [&](size_t p, bool mx, bool my) {
        const typename P::V qv = P::ld(q + p);
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < kk) P::add(acc[j], qv * P::ld(d.q(j) + p), mx, my);
    });
    const size_t nb = block_count(), b = block_slot();
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < kk) {
            const double s = block_sum(acc[j]);
            if (threadIdx.x == 0) part[(size_t)j * nb + b] = s;
        }
    }
}

// q -= b_j*Q_j, z -= b_j*Z_j for j = 0 .. kk-1 in this order (kk == 0: z is not read, neither is written);
// part[block] = share of <q, q>, part[nb + block] = share of <r, q>
template <int K, bool PAIR>
__device__ __forceinline__ void krylov_orth_body(int N, int kk, double *__restrict__ q, double *__restrict__ z,
                                                 const double *__restrict__ r, const Dirs &d, const double *__restrict__ b,
                                                 double *__restrict__ part)
{
    typedef Pt<PAIR> P;
    double bj[K > 0 ? K : 1];
#pragma unroll
    for (int j = 0; j < K; ++j) bj[j] = j < kk ? b[j] : 0.0;
    double g = 0.0, h = 0.0;
    for_rows<PAIR>(N, [&](size_t p, bool mx, bool my) {
        typename P::V qv = P::ld(q + p);
        if constexpr (K > 0) {
            if (kk > 0) {
                typename P::V zv = P::ld(z + p);
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    if (j < kk) {
                        qv = qv - bj[j] * P::ld_nt(d.q(j) + p);
                        zv = zv - bj[j] * P::ld_nt(d.z(j) + p);
                    }
                }
                P::st(q + p, qv, mx, my);
                P::st(z + p, zv, mx, my);
            }
        }
        P::add(g, qv * qv, mx, my);
        P::add(h, P::ld(r + p) * qv, mx, my);
    });
    const size_t nb = block_count(), slot = block_slot();
    const double sg = block_sum(g);
    const double sh = block_sum(h);
    if (threadIdx.x == 0) {
        part[slot] = sg;
        part[nb + slot] = sh;
    }
}

// U += alpha*z, r -= alpha*q (alpha == 0: neither is written); part[block] = share of <r, r>
template <bool PAIR>
__device__ __forceinline__ void krylov_update_body(int N, const double *__restrict__ alpha_p, double *__restrict__ U,
                                                   const double *__restrict__ z, double *__restrict__ r,
                                                   const double *__restrict__ q, double *__restrict__ part)
{
    typedef Pt<PAIR> P;
    const double alpha = *alpha_p;
    const bool move = alpha != 0.0;
    double acc = 0.0;
    for_rows<PAIR>(N, [&](size_t p, bool mx, bool my) {
        typename P::V rv = P::ld(r + p);
        if (move) {
            const typename P::V uv = P::ld(U + p) + alpha * P::ld_nt(z + p);
            rv = rv - alpha * P::ld_nt(q + p);
            P::st(U + p, uv, mx, my);
            P::st(r + p, rv, mx, my);
        }
        P::add(acc, rv * rv, mx, my);
    });
    const double s = block_sum(acc);
    if (threadIdx.x == 0) part[block_slot()] = s;
}

// the sum of n partials in a fixed order (one block); valid in thread 0
__device__ __forceinline__ double finish_sum(const double *__restrict__ part, size_t n)
{
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) acc += part[i];
    return block_sum(acc);
}

// d_j = the sum of stripe j; d_out[j] = d_j, and b[j] = d_j*w[j] where w is given
__device__ __forceinline__ void krylov_dots_finish_body(int j, const double *__restrict__ part, size_t nb, const double *__restrict__ w,
                                                        double *__restrict__ b, double *__restrict__ d_out)
{
    const double d = finish_sum(part + (size_t)j * nb, nb);
    if (threadIdx.x == 0) {
        d_out[j] = d;
        if (w) b[j] = d * w[j];
    }
}

// g, h from their stripes; w_k = 1/g, alpha = h*w_k, or the breakdown (include/mg_krylov.h).  gh[0..1] = g, h.  In a solve
// (rec != nullptr) the head of the log record: rec[0] = k, the unused d entries +0, rec[m+1..m+3] = g, h, alpha.
__device__ __forceinline__ void krylov_orth_finish_body(const double *__restrict__ part, size_t nb, int k, int m,
                                                        double *__restrict__ gh, double *__restrict__ w_k,
                                                        double *__restrict__ alpha_out, double *__restrict__ brk,
                                                        double *__restrict__ rec)
{
    const double g = finish_sum(part, nb);
    const double h = finish_sum(part + nb, nb);
    if (threadIdx.x == 0) {
        gh[0] = g;
        gh[1] = h;
        if (alpha_out) {
            const double inf = __builtin_huge_val();
            const double w = 1.0 / g;
            double alpha = h * w;
            const bool bad = !(g > 0.0) || !(g < inf) || !(alpha > -inf && alpha < inf);
            if (bad) alpha = 0.0;
            *w_k = w;
            *alpha_out = alpha;
            *brk = bad ? 1.0 : 0.0;
            if (rec) {
                rec[0] = (double)k;
                for (int j = k; j < m; ++j) rec[1 + j] = 0.0;
                rec[m + 1] = g;
                rec[m + 2] = h;
                rec[m + 3] = alpha;
            }
        }
    }
}

// rho_rec = sqrt(<r, r>); in a solve the tail of the log record: rho_rec, restarted = 0, rho = rho_rec
__device__ __forceinline__ void krylov_update_finish_body(const double *__restrict__ part, size_t nb, double *__restrict__ rr,
                                                          double *__restrict__ rho_out, double *__restrict__ rec_tail)
{
    const double s = finish_sum(part, nb);
    if (threadIdx.x == 0) {
        if (rr) *rr = s;
        if (rho_out) {
            const double rho = sqrt(s);
            *rho_out = rho;
            rec_tail[0] = rho;
            rec_tail[1] = 0.0;
            rec_tail[2] = rho;
        }
    }
}

inline dim3 grid_of(int N) { return use_pairs(N) ? grid_pairs(N) : grid_rows(N); }

}  // namespace

}  // namespace k
}  // namespace mg

#endif /* MG_KRYLOV_IMPL_H */
