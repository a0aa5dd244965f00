// mg_krylov_kernels.hip -- fp64 kernels of the Krylov acceleration of the residual-tolerance solver (include/mg_krylov.h;
// driven by mg_solve.cpp: krylov_iterate): the k dot products <q_k, q_j> in one pass, the orthogonalisation of q_k and z_k
// against the k stored directions fused with g = <q_k, q_k> and h = <r, q_k>, the update of U and r fused with <r, r>, and
// the one-block finish launches that turn per-block partials into d_j*w_j, w_k, alpha, rho_rec, the breakdown flag and the
// log record.  Built with -ffp-contract=off like every kernel file: the header fixes one rounding per operation, so numpy
// restates the vector updates bit for bit.
// Shapes as in mg_varcoef_impl.h: a lane walks 4 rows down its column (any N) or its column pair (even N from PAIR_MIN_N on,
// 16-byte accesses).  Only interior points are touched: the edge lanes of the pair form load their pair and use -- and
// store -- its interior half alone (an 8-byte store), so the rim of no array is ever written and a NaN there reaches no
// result.  k is a compile-time bucket (K = 0 .. 15): the pointers of the stored directions are kernel arguments indexed by
// constants, the K accumulators live in registers, no scratch.  Non-temporal loads are a compile-time property of a
// stream, not of N (as k_residual_pairs): in the pair form the stored directions Q_j, Z_j of the orthogonalisation and z_k,
// q_k of the update -- which the next launch does not read again -- come through non-temporal loads; everything the next
// launch re-reads (q_k after the dots, q_k, z_k and r after the orthogonalisation, r after the update) is loaded and stored
// normally.  Memory-bound, no stencil, no division: 8 + 8k, 40 + 16k (16 at k = 0: z_k is not read and nothing is stored)
// and 48 bytes per point.
// Every sum is per-block partials in a fixed partition (block (x, y) -> slot y*gridDim.x + x, one stripe of slots per sum)
// and a finish launch that adds them in a fixed order: no floating-point atomics, the same call twice gives the same bits.
// wave_sum / block_sum are the third private copy (mg_solve_kernels.hip, mg_varcoef_impl.h); nothing here has to match the
// other two bit for bit.
#include <hip/hip_runtime.h>

#include "mg_internal.h"

namespace mg {
namespace k {

namespace {

constexpr int TB = 256;          // threads per block
constexpr int ROWS_PB = 4;       // rows per block, one point per lane
constexpr int PR = 4;            // rows per thread of the 16-byte form
constexpr int PAIR_MIN_N = 512;
typedef double double2_v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// sum over the block in a fixed order; valid in thread 0.  Every thread of the block must call it.
__device__ __forceinline__ double block_sum(double v)
{
    __shared__ double sm[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) sm[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; ++i) r += sm[i];
    }
    return r;
}

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

__device__ __forceinline__ size_t block_slot() { return (size_t)blockIdx.y * gridDim.x + blockIdx.x; }
__device__ __forceinline__ size_t block_count() { return (size_t)gridDim.x * gridDim.y; }

// part[j*nb + block] = this block's share of <q, Q_j>, j < K
template <int K, bool PAIR>
__global__ __launch_bounds__(TB) void k_krylov_dots(int N, const double *__restrict__ q, KrylovVecs v, double *__restrict__ part)
{
    typedef Pt<PAIR> P;
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    for_rows<PAIR>(N, [&](size_t p, bool mx, bool my) {
        const typename P::V qv = P::ld(q + p);
#pragma unroll
        for (int j = 0; j < K; ++j) P::add(acc[j], qv * P::ld(v.q[j] + p), mx, my);
    });
    const size_t nb = block_count(), b = block_slot();
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double s = block_sum(acc[j]);
        if (threadIdx.x == 0) part[(size_t)j * nb + b] = s;
    }
}

// q -= b_j*Q_j, z -= b_j*Z_j for j = 0 .. K-1 in this order; part[block] = share of <q, q>, part[nb + block] = share of <r, q>
template <int K, bool PAIR>
__global__ __launch_bounds__(TB) void k_krylov_orth(int N, double *__restrict__ q, double *__restrict__ z, const double *__restrict__ r,
                                                    KrylovVecs v, const double *__restrict__ b, double *__restrict__ part)
{
    typedef Pt<PAIR> P;
    double bj[K > 0 ? K : 1];
#pragma unroll
    for (int j = 0; j < K; ++j) bj[j] = b[j];
    double g = 0.0, h = 0.0;
    for_rows<PAIR>(N, [&](size_t p, bool mx, bool my) {
        typename P::V qv = P::ld(q + p);
        if constexpr (K > 0) {
            typename P::V zv = P::ld(z + p);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                qv = qv - bj[j] * P::ld_nt(v.q[j] + p);
                zv = zv - bj[j] * P::ld_nt(v.z[j] + p);
            }
            P::st(q + p, qv, mx, my);
            P::st(z + p, zv, mx, my);
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
__global__ __launch_bounds__(TB) void k_krylov_update(int N, const double *__restrict__ alpha_p, double *__restrict__ U,
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

// block j: d_j = the sum of stripe j; d_out[j] = d_j, and b[j] = d_j*w[j] where w is given
__global__ __launch_bounds__(1024) void k_krylov_dots_finish(const double *__restrict__ part, size_t nb, const double *__restrict__ w,
                                                             double *__restrict__ b, double *__restrict__ d_out)
{
    const int j = blockIdx.x;
    const double d = finish_sum(part + (size_t)j * nb, nb);
    if (threadIdx.x == 0) {
        d_out[j] = d;
        if (w) b[j] = d * w[j];
    }
}

// g, h from their stripes; w_k = 1/g, alpha = h*w_k, or the breakdown (include/mg_krylov.h).  gh[0..1] = g, h.  In a solve
// (rec != nullptr) the head of the log record: rec[0] = k, the unused d entries +0, rec[m+1..m+3] = g, h, alpha.
__global__ __launch_bounds__(1024) void k_krylov_orth_finish(const double *__restrict__ part, size_t nb, int k, int m,
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
__global__ __launch_bounds__(1024) void k_krylov_update_finish(const double *__restrict__ part, size_t nb, double *__restrict__ rr,
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

// a restart: restarted = 1, rho = the recomputed norm
__global__ void k_krylov_log_restart(double *__restrict__ rec_tail, const double *__restrict__ rho)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        rec_tail[1] = 1.0;
        rec_tail[2] = *rho;
    }
}

inline bool use_pairs(int N) { return N % 2 == 0 && N >= PAIR_MIN_N; }
inline dim3 grid_of(int N)
{
    if (use_pairs(N)) return dim3((N / 2 + TB - 1) / TB, (N + PR - 1) / PR);
    return dim3((N + TB - 1) / TB, (N + ROWS_PB - 1) / ROWS_PB);
}

template <int K>
void launch_dots(hipStream_t s, int N, const double *q, const KrylovVecs &v, double *part)
{
    if (use_pairs(N)) hipLaunchKernelGGL((k_krylov_dots<K, true>), grid_of(N), dim3(TB), 0, s, N, q, v, part);
    else hipLaunchKernelGGL((k_krylov_dots<K, false>), grid_of(N), dim3(TB), 0, s, N, q, v, part);
}

template <int K>
void launch_orth(hipStream_t s, int N, double *q, double *z, const double *r, const KrylovVecs &v, const double *b, double *part)
{
    if (use_pairs(N)) hipLaunchKernelGGL((k_krylov_orth<K, true>), grid_of(N), dim3(TB), 0, s, N, q, z, r, v, b, part);
    else hipLaunchKernelGGL((k_krylov_orth<K, false>), grid_of(N), dim3(TB), 0, s, N, q, z, r, v, b, part);
}

}  // namespace

// ------------------------------------------------------------------ launchers
size_t krylov_blocks(int N)
{
    const dim3 g = grid_of(N);
    return (size_t)g.x * g.y;
}

#define MG_KRYLOV_BUCKETS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)

void krylov_dots(hipStream_t s, int N, int k, const double *q, const KrylovVecs &v, double *part, const double *w, double *b,
                 double *d_out)
{
    switch (k) {
#define X(K) case K: launch_dots<K>(s, N, q, v, part); break;
        MG_KRYLOV_BUCKETS(X)
#undef X
        default: return;   // (k == 0: nothing to do; the callers keep k <= KRYLOV_MAX_K)
    }
    hipLaunchKernelGGL(k_krylov_dots_finish, dim3(k), dim3(1024), 0, s, part, krylov_blocks(N), w, b, d_out);
}

void krylov_orth(hipStream_t s, int N, int k, double *q, double *z, const double *r, const KrylovVecs &v, const double *b,
                 double *part)
{
    switch (k) {
        case 0: launch_orth<0>(s, N, q, z, r, v, b, part); break;
#define X(K) case K: launch_orth<K>(s, N, q, z, r, v, b, part); break;
        MG_KRYLOV_BUCKETS(X)
#undef X
        default: return;
    }
}

void krylov_orth_finish(hipStream_t s, int N, const double *part, int k, int m, double *gh, double *w_k, double *alpha, double *brk,
                        double *rec)
{
    hipLaunchKernelGGL(k_krylov_orth_finish, dim3(1), dim3(1024), 0, s, part, krylov_blocks(N), k, m, gh, w_k, alpha, brk, rec);
}

void krylov_update(hipStream_t s, int N, const double *alpha, double *U, const double *z, double *r, const double *q, double *part)
{
    if (use_pairs(N)) hipLaunchKernelGGL(k_krylov_update<true>, grid_of(N), dim3(TB), 0, s, N, alpha, U, z, r, q, part);
    else hipLaunchKernelGGL(k_krylov_update<false>, grid_of(N), dim3(TB), 0, s, N, alpha, U, z, r, q, part);
}

void krylov_update_finish(hipStream_t s, int N, const double *part, double *rr, double *rho_out, double *rec_tail)
{
    hipLaunchKernelGGL(k_krylov_update_finish, dim3(1), dim3(1024), 0, s, part, krylov_blocks(N), rr, rho_out, rec_tail);
}

void krylov_log_restart(hipStream_t s, double *rec_tail, const double *rho)
{
    hipLaunchKernelGGL(k_krylov_log_restart, dim3(1), dim3(64), 0, s, rec_tail, rho);
}

}  // namespace k
}  // namespace mg
