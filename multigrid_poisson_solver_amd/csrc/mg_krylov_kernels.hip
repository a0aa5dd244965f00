// mg_krylov_kernels.hip -- fp64 kernels of the Krylov acceleration of the residual-tolerance solver (include/mg_krylov.h;
// driven by mg_solve.cpp: krylov_iterate): the k dot products <q_k, q_j> in one pass, the orthogonalisation of q_k and z_k
// against the k stored directions fused with g = <q_k, q_k> and h = <r, q_k>, the update of U and r fused with <r, r>, and
// the one-block finish launches that turn per-block partials into d_j*w_j, w_k, alpha, rho_rec, the breakdown flag and the
// log record.  Built with -ffp-contract=off like every kernel file: the header fixes one rounding per operation, so numpy
// restates the vector updates bit for bit.
// The __device__ bodies live in mg_krylov_impl.h, which mg_krylov_batch_kernels.hip compiles too: the kernels below hand them
// the arrays of their one instance and k = K as a constant.
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
// wave_sum / block_sum are mg_solver_common.h's, the ones of the solver's own norms.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_krylov_impl.h"

namespace mg {
namespace k {

namespace {

template <int K, bool PAIR>
__global__ __launch_bounds__(TB) void k_krylov_dots(int N, const double *__restrict__ q, KrylovVecs v, double *__restrict__ part)
{
    krylov_dots_body<K, PAIR>(N, K, q, Dirs{v, 0}, part);
}

template <int K, bool PAIR>
__global__ __launch_bounds__(TB) void k_krylov_orth(int N, double *__restrict__ q, double *__restrict__ z, const double *__restrict__ r,
                                                    KrylovVecs v, const double *__restrict__ b, double *__restrict__ part)
{
    krylov_orth_body<K, PAIR>(N, K, q, z, r, Dirs{v, 0}, b, part);
}

template <bool PAIR>
__global__ __launch_bounds__(TB) void k_krylov_update(int N, const double *__restrict__ alpha_p, double *__restrict__ U,
                                                      const double *__restrict__ z, double *__restrict__ r,
                                                      const double *__restrict__ q, double *__restrict__ part)
{
    krylov_update_body<PAIR>(N, alpha_p, U, z, r, q, part);
}

// block j: d_j = the sum of stripe j; d_out[j] = d_j, and b[j] = d_j*w[j] where w is given
__global__ __launch_bounds__(1024) void k_krylov_dots_finish(const double *__restrict__ part, size_t nb, const double *__restrict__ w,
                                                             double *__restrict__ b, double *__restrict__ d_out)
{
    krylov_dots_finish_body(blockIdx.x, part, nb, w, b, d_out);
}

__global__ __launch_bounds__(1024) void k_krylov_orth_finish(const double *__restrict__ part, size_t nb, int k, int m,
                                                             double *__restrict__ gh, double *__restrict__ w_k,
                                                             double *__restrict__ alpha_out, double *__restrict__ brk,
                                                             double *__restrict__ rec)
{
    krylov_orth_finish_body(part, nb, k, m, gh, w_k, alpha_out, brk, rec);
}

__global__ __launch_bounds__(1024) void k_krylov_update_finish(const double *__restrict__ part, size_t nb, double *__restrict__ rr,
                                                               double *__restrict__ rho_out, double *__restrict__ rec_tail)
{
    krylov_update_finish_body(part, nb, rr, rho_out, rec_tail);
}

// a restart: restarted = 1, rho = the recomputed norm
__global__ void k_krylov_log_restart(double *__restrict__ rec_tail, const double *__restrict__ rho)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        rec_tail[1] = 1.0;
        rec_tail[2] = *rho;
    }
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
