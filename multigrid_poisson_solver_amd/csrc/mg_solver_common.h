// mg_solver_common.h -- what the kernel families of the residual-tolerance solvers share (mg_solve_kernels.hip,
// mg_varcoef_impl.h and everything layered over it, mg_krylov_impl.h): the block shape of the streaming kernels, the block
// sums, the norm's finish and the host-side choice of a launch's form.  ONE copy: the norm of a == 1 is the constant norm bit
// for bit because both run this block_sum and this finish, and a batched launch partitions an instance as its single launch
// does because both take their grids from here.  Everything sits in an unnamed namespace: each translation unit has its own.
#ifndef MG_SOLVER_COMMON_H
#define MG_SOLVER_COMMON_H

#include <hip/hip_runtime.h>

#include <type_traits>

namespace mg {
namespace k {

namespace {

constexpr int TB = 256;          // threads per block of the streaming kernels
constexpr int ROWS_PB = 4;       // rows per block, one point per lane
constexpr int PR = 4;            // rows per thread of the 16-byte forms (rolling window of three row pairs)
constexpr int PAIR_MIN_N = 512;
constexpr int NT_MIN_N = 4096;   // from here on the arrays are far larger than the caches: non-temporal F loads
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

__device__ __forceinline__ bool rim(int r, int c, int N)
{
    return r == 0 || c == 0 || r == N - 1 || c == N - 1;
}

// second stage of every residual norm: *out = sqrt(sum of the n partials), one block in a fixed order (run-to-run
// reproducible)
__device__ __forceinline__ void resnorm_finish_body(const double *__restrict__ part, size_t n, double *__restrict__ out)
{
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) acc += part[i];
    const double s = block_sum(acc);
    if (threadIdx.x == 0) *out = sqrt(s);
}

inline dim3 grid_rows(int N) { return dim3((N + TB - 1) / TB, (N + ROWS_PB - 1) / ROWS_PB); }
inline bool use_pairs(int N) { return N % 2 == 0 && N >= PAIR_MIN_N; }
inline dim3 grid_pairs(int N) { return dim3((N / 2 + TB - 1) / TB, (N + PR - 1) / PR); }
// the grid of a batched streaming launch: instance blockIdx.z of n
inline dim3 with_instances(dim3 g, int n)
{
    g.z = n;
    return g;
}

// The form of a streaming launch on an N x N level, chosen in ONE place: one column per lane, or -- even N from PAIR_MIN_N
// on -- two columns per lane, non-temporal from NT_MIN_N on.  f(pair, nt, has_a, grid) gets the three choices as
// std::bool_constant values, to be used as template arguments (`pair()`), and the single-instance grid of that form.
// (pair, nt) is (false, false), (true, false) or (true, true): nothing else is ever instantiated.
template <class F>
void dispatch_form(int N, bool has_a, F &&f)
{
    auto with_a = [&](auto pair, auto nt, dim3 g) {
        if (has_a) f(pair, nt, std::true_type{}, g);
        else f(pair, nt, std::false_type{}, g);
    };
    if (!use_pairs(N)) with_a(std::false_type{}, std::false_type{}, grid_rows(N));
    else if (N >= NT_MIN_N) with_a(std::true_type{}, std::true_type{}, grid_pairs(N));
    else with_a(std::true_type{}, std::false_type{}, grid_pairs(N));
}

}  // namespace

}  // namespace k
}  // namespace mg

#endif /* MG_SOLVER_COMMON_H */
