// mg_eigs_impl.h -- the point code of the eigen-solver's kernels (include/mg_eigs.h; launched by mg_eigs_kernels.hip): the
// block Gram matrices G = S^T S, H = S^T AS of up to 36 basis fields in one pass, the block rotation [X', AX', P', AP', R]
// of the Rayleigh-Ritz step fused with the residual norms, and the recomputed residual R = AX - theta*X with its norms.
// The lane shapes, the block sum and the finish sum are those of mg_krylov_impl.h, which this file includes instead of
// copying them: a lane owns one column (any N) or a column pair (even N from PAIR_MIN_N on, 16-byte accesses) and walks the
// rows of its block down it.  Only interior points are touched: the edge lanes of the pair form load their pair and use --
// and store -- its interior half alone, so the rim of no array is ever written and a NaN there reaches no result.
// Everything a block needs besides the fields comes from two small tables in device memory, read through uniform (scalar)
// loads: the field pointers and, for the rotation, the coefficient matrices -- nothing here depends on k or p beyond loop
// bounds that are uniform over the launch.  All per-lane arrays are indexed by constants after unrolling: no scratch.
#ifndef MG_EIGS_IMPL_H
#define MG_EIGS_IMPL_H

#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_krylov_impl.h"

namespace mg {
namespace k {

namespace {

constexpr int GRAM_ROWS = 16;    // rows per block of the Gram kernel: 72 block sums are paid once per 4096 points
constexpr int ROT_ROWS = 4;      // rows per block of the rotation and the residual kernel (as the Krylov kernels)

// body(p, mx, my) for every row of this block that holds an interior point of this lane; one row at a time (the bodies are
// large: unrolling the rows would only multiply the code)
template <bool PAIR, int ROWS, typename Body>
__device__ __forceinline__ void eig_rows(int N, Body body)
{
    const int lane_col = blockIdx.x * TB + threadIdx.x;
    const int c = PAIR ? 2 * lane_col : lane_col;   // (PAIR: N even, c + 1 <= N - 1 whenever c < N)
    const int r0 = blockIdx.y * ROWS;
    const bool mx = c > 0 && c < N - 1, my = PAIR && c + 1 < N - 1;
    if (!(mx || my) || c >= N) return;
#pragma unroll 1
    for (int i = 0; i < ROWS; ++i) {
        const int r = r0 + i;
        if (r > 0 && r < N - 1) body((size_t)r * N + c, mx, my);
    }
}

template <bool PAIR>
__device__ __forceinline__ typename Pt<PAIR>::V eig_zero()
{
    typename Pt<PAIR>::V v = {};
    return v;
}

// One tile (a, b), a <= b, of the two Gram matrices: acc[jj*T + ll] = <S_j, S_l>, acc[T*T + jj*T + ll] = <S_j, AS_l> with
// j = a*T + jj, l = b*T + ll.  DIAG (a == b): S_l is S_j, loaded once, and only jj <= ll is formed (G is symmetric; of H the
// upper triangle is computed and the host mirrors it).  part[(e*nb) + block] = this block's share of entry e.
template <bool PAIR, bool DIAG>
__device__ __forceinline__ void eig_gram_tile(int N, int m, int a, int b, const double *const *__restrict__ ptrs,
                                              double *__restrict__ part)
{
    typedef Pt<PAIR> P;
    typedef typename P::V V;
    constexpr int T = EIGS_TILE;
    const int nj = m - a * T < T ? m - a * T : T, nl = m - b * T < T ? m - b * T : T;
    const double *Sj[T], *Sl[T], *Al[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        Sj[t] = t < nj ? ptrs[a * T + t] : nullptr;
        Sl[t] = t < nl ? ptrs[b * T + t] : nullptr;
        Al[t] = t < nl ? ptrs[m + b * T + t] : nullptr;
    }
    double acc[2 * T * T];
#pragma unroll
    for (int e = 0; e < 2 * T * T; ++e) acc[e] = 0.0;
    eig_rows<PAIR, GRAM_ROWS>(N, [&](size_t p, bool mx, bool my) {
        V sj[T], sl[T], al[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            sj[t] = t < nj ? P::ld(Sj[t] + p) : eig_zero<PAIR>();
            al[t] = t < nl ? P::ld(Al[t] + p) : eig_zero<PAIR>();
            if constexpr (DIAG) sl[t] = sj[t];
            else sl[t] = t < nl ? P::ld(Sl[t] + p) : eig_zero<PAIR>();
        }
#pragma unroll
        for (int jj = 0; jj < T; ++jj)
#pragma unroll
            for (int ll = DIAG ? jj : 0; ll < T; ++ll) {
                P::add(acc[jj * T + ll], sj[jj] * sl[ll], mx, my);
                P::add(acc[T * T + jj * T + ll], sj[jj] * al[ll], mx, my);
            }
    });
    const size_t nb = block_count(), slot = block_slot();
#pragma unroll
    for (int e = 0; e < 2 * T * T; ++e) {
        const int jj = (e % (T * T)) / T, ll = e % T;
        if (DIAG && ll < jj) {   // (never formed: the host reads the mirrored entry)
            if (threadIdx.x == 0) part[(size_t)e * nb + slot] = 0.0;
            continue;
        }
        const double s = block_sum(acc[e]);
        if (threadIdx.x == 0) part[(size_t)e * nb + slot] = s;
    }
}

template <bool PAIR>
__device__ __forceinline__ void eig_gram_body(int N, int m, const double *const *__restrict__ ptrs, double *__restrict__ part)
{
    constexpr int T = EIGS_TILE;
    const int nt = (m + T - 1) / T;
    int a = 0, rem = blockIdx.z;   // tile z, row-major over a <= b
    while (rem >= nt - a) {
        rem -= nt - a;
        ++a;
    }
    const int b = a + rem;
    double *tile_part = part + (size_t)blockIdx.z * EIGS_TILE_SUMS * block_count();
    if (a == b) eig_gram_tile<PAIR, true>(N, m, a, b, ptrs, tile_part);
    else eig_gram_tile<PAIR, false>(N, m, a, b, ptrs, tile_part);
}

// The rotation of include/mg_eigs.h.  M >= m is a compile-time bucket: the values of the fields j >= m are +0 and so are
// their coefficients (the host pads every column of C and Cp with +0 up to EIGS_MAX_M), and a sum that started from +0 is
// never -0, so adding (+0)*(+0) keeps its bits: the sum over j < M equals the sum over j < m bit for bit.
template <int M, bool PAIR>
__device__ __forceinline__ void eig_rotate_body(int N, int m, int p, double *const *__restrict__ ptrs,
                                                const double *__restrict__ coef, double *__restrict__ part)
{
    typedef Pt<PAIR> P;
    typedef typename P::V V;
    constexpr int PB = MG_EIGS_MAX_BLOCK;
    double acc[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) acc[i] = 0.0;
    eig_rows<PAIR, ROT_ROWS>(N, [&](size_t pt, bool mx, bool my) {
        V s[M], as[M];
#pragma unroll
        for (int j = 0; j < M; ++j) {
            s[j] = j < m ? P::ld(ptrs[j] + pt) : eig_zero<PAIR>();
            as[j] = j < m ? P::ld(ptrs[EIGS_PTR_AS + j] + pt) : eig_zero<PAIR>();
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            if (i < p) {
                const double *__restrict__ c = coef + i * EIGS_MAX_M, *__restrict__ cp = coef + EIGS_COEF_CP + i * EIGS_MAX_M;
                V x = eig_zero<PAIR>(), ax = x, pp = x, ap = x;
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    const double cj = c[j], cpj = cp[j];
                    x = x + cj * s[j];
                    ax = ax + cj * as[j];
                    pp = pp + cpj * s[j];
                    ap = ap + cpj * as[j];
                }
                const V r = ax - coef[EIGS_COEF_THETA + i] * x;
                P::st(ptrs[i] + pt, x, mx, my);
                P::st(ptrs[EIGS_PTR_AS + i] + pt, ax, mx, my);
                P::st(ptrs[2 * p + i] + pt, pp, mx, my);
                P::st(ptrs[EIGS_PTR_AS + 2 * p + i] + pt, ap, mx, my);
                P::st(ptrs[EIGS_PTR_R + i] + pt, r, mx, my);
                P::add(acc[i], r * r, mx, my);
            }
        }
    });
    const size_t nb = block_count(), slot = block_slot();
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        if (i < p) {
            const double sum = block_sum(acc[i]);
            if (threadIdx.x == 0) part[(size_t)i * nb + slot] = sum;
        }
    }
}

// R_i = AX_i - theta_i*X_i, part[i*nb + block] = this block's share of <R_i, R_i>, i < p
template <bool PAIR>
__device__ __forceinline__ void eig_resnorm_body(int N, int p, double *const *__restrict__ ptrs, const double *__restrict__ coef,
                                                 double *__restrict__ part)
{
    typedef Pt<PAIR> P;
    typedef typename P::V V;
    constexpr int PB = MG_EIGS_MAX_BLOCK;
    double acc[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) acc[i] = 0.0;
    eig_rows<PAIR, ROT_ROWS>(N, [&](size_t pt, bool mx, bool my) {
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            if (i < p) {
                const V r = P::ld(ptrs[EIGS_PTR_AS + i] + pt) - coef[EIGS_COEF_THETA + i] * P::ld(ptrs[i] + pt);
                P::st(ptrs[EIGS_PTR_R + i] + pt, r, mx, my);
                P::add(acc[i], r * r, mx, my);
            }
        }
    });
    const size_t nb = block_count(), slot = block_slot();
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        if (i < p) {
            const double sum = block_sum(acc[i]);
            if (threadIdx.x == 0) part[(size_t)i * nb + slot] = sum;
        }
    }
}

inline dim3 eig_grid(int N, int rows)
{
    const int cols = use_pairs(N) ? N / 2 : N;
    return dim3((cols + TB - 1) / TB, (N + rows - 1) / rows);
}

}  // namespace

}  // namespace k
}  // namespace mg

#endif /* MG_EIGS_IMPL_H */
