// mg_krylov_batch_kernels.hip -- batched forms of the Krylov kernels (include/mg_krylov_batch.h; driven by
// mg_solve_batch.cpp: krylov_iterate_batch): ONE launch runs a kernel of mg_krylov_kernels.hip for every active instance.
// The __device__ bodies are the ones of mg_krylov_impl.h, compiled here with the same flags (-ffp-contract=off): an instance
// runs the code, the block partition (grid x, y), the per-block partial slots and the summation order of its single launch,
// so its bits are the single solve's.  Which instance a block works on: blockIdx.z for the streaming kernels, whose single
// grids are (column blocks, row blocks); blockIdx.y for the dots' finish, whose single grid is one block per stripe;
// blockIdx.x for the one-block finish kernels, the log mark and (with blockIdx.y) the zeroing (max_batch <= 65535 fits each
// of them).  The instance's arrays come from a KrylovBatchItem table in device memory (mg_internal.h): this iteration's z_k
// and q_k, its scalars, its partials, its log record, and its offset in the slots of the stored directions -- slot j holds
// z_j (q_j) of every instance at the instance pitch, so the slots themselves are kernel arguments indexed by constants, as
// in the single kernels, and an entry carries two direction pointers, not thirty.
// Per-instance k.  K, the compile-time bucket of a launch, is the LARGEST k of the active set; a block reads its instance's
// own k <= K from the table -- the same for every lane of the block: a scalar load and scalar branches -- and runs
// j = 0 .. k-1 in this order.  An instance at k = 0 leaves the dots launch before any barrier, finish blocks of stripes
// j >= k do the same, and the orthogonalisation of such an instance neither reads z_k nor stores anything, as the K = 0
// kernel of the single solver.
// The zeroing of z_k writes every one of the N*N doubles (the memset of the single solver: the rim is +0 too), nothing of
// the instance pitch's padding behind them.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_krylov_impl.h"

namespace mg {
namespace k {

namespace {

template <int K, bool PAIR>
__global__ __launch_bounds__(TB) void k_krylov_dots_b(int N, const KrylovBatchItem *__restrict__ items, KrylovVecs v)
{
    const KrylovBatchItem &it = items[blockIdx.z];
    const int kk = it.k;
    if (kk == 0) return;   // (block-uniform, before any barrier)
    krylov_dots_body<K, PAIR>(N, kk, it.qk, Dirs{v, it.off}, it.part);
}

template <int K, bool PAIR>
__global__ __launch_bounds__(TB) void k_krylov_orth_b(int N, const KrylovBatchItem *__restrict__ items, KrylovVecs v)
{
    const KrylovBatchItem &it = items[blockIdx.z];
    krylov_orth_body<K, PAIR>(N, it.k, it.qk, it.zk, it.r, Dirs{v, it.off}, it.scal + KRYLOV_SCAL_B, it.part);
}

template <bool PAIR>
__global__ __launch_bounds__(TB) void k_krylov_update_b(int N, const KrylovBatchItem *__restrict__ items)
{
    const KrylovBatchItem &it = items[blockIdx.z];
    krylov_update_body<PAIR>(N, it.scal + KRYLOV_SCAL_ALPHA, it.U, it.zk, it.r, it.qk, it.part);
}

// block (j, instance): d_j into the record, b_j = d_j*w_j; stripes the instance does not have leave before any barrier
__global__ __launch_bounds__(1024) void k_krylov_dots_finish_b(const KrylovBatchItem *__restrict__ items, size_t nb)
{
    const KrylovBatchItem &it = items[blockIdx.y];
    const int j = blockIdx.x;
    if (j >= it.k) return;
    krylov_dots_finish_body(j, it.part, nb, it.scal + KRYLOV_SCAL_W, it.scal + KRYLOV_SCAL_B, it.rec + 1);
}

// one block per instance
__global__ __launch_bounds__(1024) void k_krylov_orth_finish_b(const KrylovBatchItem *__restrict__ items, size_t nb, int m)
{
    const KrylovBatchItem &it = items[blockIdx.x];
    krylov_orth_finish_body(it.part, nb, it.k, m, it.rec + 1 + m, it.scal + KRYLOV_SCAL_W + it.k, it.scal + KRYLOV_SCAL_ALPHA,
                            it.scal + KRYLOV_SCAL_BRK, it.rec);
}

// one block per instance; rho_rec and the breakdown flag (set by the orthogonalisation's finish) go where the host reads
// them: rb[slot], rb[stride + slot]
__global__ __launch_bounds__(1024) void k_krylov_update_finish_b(const KrylovBatchItem *__restrict__ items, size_t nb, int m,
                                                                 double *__restrict__ rb, int stride)
{
    const KrylovBatchItem &it = items[blockIdx.x];
    krylov_update_finish_body(it.part, nb, nullptr, rb + blockIdx.x, it.rec + m + 4);
    if (threadIdx.x == 0) rb[stride + blockIdx.x] = it.scal[KRYLOV_SCAL_BRK];
}

// a restart's mark in the records of the restarting instances: restarted = 1, rho = the recomputed norm norms[slot]
__global__ void k_krylov_log_restart_b(const KrylovBatchItem *__restrict__ items, int m, const double *__restrict__ norms)
{
    if (threadIdx.x == 0) {
        double *tail = items[blockIdx.x].rec + m + 4;
        tail[1] = 1.0;
        tail[2] = norms[blockIdx.x];
    }
}

// z_k = +0, all count = N*N doubles of it: 16-byte stores (the arrays are 16-byte aligned), the last double alone when
// count is odd
constexpr int ZERO_BLOCKS_MAX = 1024;
__global__ __launch_bounds__(TB) void k_krylov_zero_b(const KrylovBatchItem *__restrict__ items, size_t count)
{
    double *z = items[blockIdx.y].zk;
    const size_t pairs = count / 2;
    const double2_v zero = {0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * TB + threadIdx.x; i < pairs; i += (size_t)gridDim.x * TB)
        reinterpret_cast<double2_v *>(z)[i] = zero;
    if ((count & 1) && blockIdx.x == 0 && threadIdx.x == 0) z[count - 1] = 0.0;
}

template <int K>
void launch_dots_b(hipStream_t s, int n, int N, const KrylovBatchItem *items, const KrylovVecs &v)
{
    const dim3 g = with_instances(grid_of(N), n);
    if (use_pairs(N)) hipLaunchKernelGGL((k_krylov_dots_b<K, true>), g, dim3(TB), 0, s, N, items, v);
    else hipLaunchKernelGGL((k_krylov_dots_b<K, false>), g, dim3(TB), 0, s, N, items, v);
}

template <int K>
void launch_orth_b(hipStream_t s, int n, int N, const KrylovBatchItem *items, const KrylovVecs &v)
{
    const dim3 g = with_instances(grid_of(N), n);
    if (use_pairs(N)) hipLaunchKernelGGL((k_krylov_orth_b<K, true>), g, dim3(TB), 0, s, N, items, v);
    else hipLaunchKernelGGL((k_krylov_orth_b<K, false>), g, dim3(TB), 0, s, N, items, v);
}

size_t blocks_of(int N)
{
    const dim3 g = grid_of(N);
    return (size_t)g.x * g.y;
}

}  // namespace

// ------------------------------------------------------------------ launchers
#define MG_KRYLOV_BUCKETS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)

void krylov_zero_batch(hipStream_t s, int n, int N, const KrylovBatchItem *items)
{
    const size_t count = (size_t)N * N;
    size_t blocks = (count / 2 + TB - 1) / TB;
    if (blocks > ZERO_BLOCKS_MAX) blocks = ZERO_BLOCKS_MAX;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_krylov_zero_b, dim3((unsigned)blocks, n), dim3(TB), 0, s, items, count);
}

void krylov_dots_batch(hipStream_t s, int n, int N, int kmax, const KrylovBatchItem *items, const KrylovVecs &v)
{
    switch (kmax) {
#define X(K) case K: launch_dots_b<K>(s, n, N, items, v); break;
        MG_KRYLOV_BUCKETS(X)
#undef X
        default: return;   // (kmax == 0: nothing to do; the caller keeps kmax <= KRYLOV_MAX_K)
    }
    hipLaunchKernelGGL(k_krylov_dots_finish_b, dim3(kmax, n), dim3(1024), 0, s, items, blocks_of(N));
}

void krylov_orth_batch(hipStream_t s, int n, int N, int kmax, int m, const KrylovBatchItem *items, const KrylovVecs &v)
{
    switch (kmax) {
        case 0: launch_orth_b<0>(s, n, N, items, v); break;
#define X(K) case K: launch_orth_b<K>(s, n, N, items, v); break;
        MG_KRYLOV_BUCKETS(X)
#undef X
        default: return;
    }
    hipLaunchKernelGGL(k_krylov_orth_finish_b, dim3(n), dim3(1024), 0, s, items, blocks_of(N), m);
}

void krylov_update_batch(hipStream_t s, int n, int N, int m, const KrylovBatchItem *items, double *rb, int stride)
{
    const dim3 g = with_instances(grid_of(N), n);
    if (use_pairs(N)) hipLaunchKernelGGL(k_krylov_update_b<true>, g, dim3(TB), 0, s, N, items);
    else hipLaunchKernelGGL(k_krylov_update_b<false>, g, dim3(TB), 0, s, N, items);
    hipLaunchKernelGGL(k_krylov_update_finish_b, dim3(n), dim3(1024), 0, s, items, blocks_of(N), m, rb, stride);
}

void krylov_log_restart_batch(hipStream_t s, int n, int m, const KrylovBatchItem *items, const double *norms)
{
    hipLaunchKernelGGL(k_krylov_log_restart_b, dim3(n), dim3(64), 0, s, items, m, norms);
}

}  // namespace k
}  // namespace mg
