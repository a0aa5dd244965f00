// mg_heat_kernels.hip -- the right-hand side of a theta-scheme time step of the heat equation (include/mg_heat.h; driven by
// mg_heat.cpp):  F = -(sigma*u) - beta*Lap_h(u) - gamma*q  on the interior, +0 on the rim.
// Built with -ffp-contract=off like every kernel file: the header fixes the evaluation order (every product and every sum
// rounded once) so that numpy restates it bit for bit.
// Memory-bound: 8 B (U) or 16 B (U and Q) read and 8 B written per point.  The shapes are those of the project's other
// streaming kernels (k_residual / k_residual_pairs, mg_kernels.hip): a lane walks HR rows down its column(s); with the
// Laplacian term it keeps a rolling window of three rows in registers, so every U value comes from memory once per block
// column (the east / west neighbours are the neighbouring lanes' values: L1 hits).  Even N from PAIR_MIN_N on: two columns per
// lane, 16-byte accesses; from NT_MIN_N on F leaves through non-temporal stores and Q comes in through non-temporal loads
// (both are far larger than the caches and touched once).  theta == 1 (LAP = false) reads no neighbour at all.
#include <hip/hip_runtime.h>

#include "mg_internal.h"

namespace mg {
namespace k {

namespace {

constexpr int TB = 256;          // threads per block
constexpr int HR = 4;            // rows per lane (as PR of mg_kernels.hip: 8 rows per thread lose there)
constexpr int PAIR_MIN_N = 512;  // even N from here on: two columns per lane, 16-byte accesses
constexpr int NT_MIN_N = 4096;   // the arrays are far larger than the caches: non-temporal accesses of F and Q
typedef double double2_h __attribute__((ext_vector_type(2)));

// one interior point in the header's order; nxt / prv: rows r+1 / r-1, east / west: columns c+1 / c-1
template <bool LAP>
__device__ __forceinline__ double heat_point(const HeatConsts &k, double u, double nxt, double prv, double east, double west,
                                             bool has_q, double q)
{
    double s = -(k.sigma * u);
    if constexpr (LAP) {
        const double lap = k.inv * ((((nxt + prv) + east) + west) - 4 * u);
        s = s - k.beta * lap;
    }
    if (has_q) s = s - k.gamma * q;
    return s;
}

// one column per lane (any N)
template <bool LAP>
__device__ __forceinline__ void heat_rhs_cols(int N, const HeatConsts &k, const double *__restrict__ U, const double *__restrict__ Q,
                                              double *__restrict__ F)
{
    const int c = blockIdx.x * TB + threadIdx.x;
    if (c >= N) return;
    const int r0 = blockIdx.y * HR;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 1 < N ? c + 1 : N - 1;
    const bool col_in = c > 0 && c < N - 1;
    const bool has_q = Q != nullptr;   // (uniform over the block)
    auto row = [&](int r) {
        r = r < 0 ? 0 : (r < N ? r : N - 1);   // (rows beyond the grid: clamped, never used)
        return U[(size_t)r * N + c];
    };
    double prv = 0.0, mid = 0.0;
    if constexpr (LAP) {
        prv = row(r0 - 1);
        mid = row(r0);
    }
#pragma unroll
    for (int i = 0; i < HR; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        double nxt = 0.0;
        if constexpr (LAP) nxt = row(r + 1);
        const size_t p = (size_t)r * N + c;
        double v = 0.0;
        if (col_in && r > 0 && r < N - 1) {
            double u, east = 0.0, west = 0.0;
            if constexpr (LAP) {
                u = mid;
                east = U[(size_t)r * N + cr];
                west = U[(size_t)r * N + cl];
            } else {
                u = U[p];
            }
            v = heat_point<LAP>(k, u, nxt, prv, east, west, has_q, has_q ? Q[p] : 0.0);
        }
        F[p] = v;
        prv = mid;
        mid = nxt;
    }
}

// two columns per lane, 16-byte accesses (even N, 16-byte aligned arrays: every pair is aligned and inside its row)
template <bool LAP, bool NT>
__device__ __forceinline__ void heat_rhs_pairs(int N, const HeatConsts &k, const double *__restrict__ U, const double *__restrict__ Q,
                                               double *__restrict__ F)
{
    const int c = 2 * (blockIdx.x * TB + threadIdx.x);
    if (c >= N) return;
    const int r0 = blockIdx.y * HR;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 2 < N ? c + 2 : N - 1;
    const bool has_q = Q != nullptr;
    auto row_pair = [&](int r) {
        r = r < 0 ? 0 : (r < N ? r : N - 1);
        return *reinterpret_cast<const double2_h *>(U + (size_t)r * N + c);
    };
    double2_h prv = {0.0, 0.0}, mid = {0.0, 0.0};
    if constexpr (LAP) {
        prv = row_pair(r0 - 1);
        mid = row_pair(r0);
    }
#pragma unroll
    for (int i = 0; i < HR; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        double2_h nxt = {0.0, 0.0};
        if constexpr (LAP) nxt = row_pair(r + 1);
        const size_t p = (size_t)r * N + c;
        double2_h v = {0.0, 0.0};
        if (r > 0 && r < N - 1) {
            double2_h u, q = {0.0, 0.0};
            double east = 0.0, west = 0.0;
            if constexpr (LAP) {
                u = mid;
                west = U[(size_t)r * N + cl];
                east = U[(size_t)r * N + cr];
            } else {
                u = *reinterpret_cast<const double2_h *>(U + p);
            }
            if (has_q) {
                if constexpr (NT) q = __builtin_nontemporal_load(reinterpret_cast<const double2_h *>(Q + p));
                else q = *reinterpret_cast<const double2_h *>(Q + p);
            }
            if (c > 0) v.x = heat_point<LAP>(k, u.x, nxt.x, prv.x, u.y, west, has_q, q.x);
            if (c + 1 < N - 1) v.y = heat_point<LAP>(k, u.y, nxt.y, prv.y, east, u.x, has_q, q.y);
        }
        if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<double2_h *>(F + p));
        else *reinterpret_cast<double2_h *>(F + p) = v;
        prv = mid;
        mid = nxt;
    }
}

template <bool LAP, bool PAIR, bool NT>
__device__ __forceinline__ void heat_rhs_body(int N, const HeatConsts &k, const double *__restrict__ U, const double *__restrict__ Q,
                                              double *__restrict__ F)
{
    if constexpr (PAIR) heat_rhs_pairs<LAP, NT>(N, k, U, Q, F);
    else heat_rhs_cols<LAP>(N, k, U, Q, F);
}

template <bool LAP, bool PAIR, bool NT>
__global__ __launch_bounds__(TB) void k_heat_rhs(int N, HeatConsts k, const double *__restrict__ U, const double *__restrict__ Q,
                                                 double *__restrict__ F)
{
    heat_rhs_body<LAP, PAIR, NT>(N, k, U, Q, F);
}

// instance blockIdx.z of items[]: in = U, coarse = Q (may be null), out = F
template <bool LAP, bool PAIR, bool NT>
__global__ __launch_bounds__(TB) void k_heat_rhs_b(int N, HeatConsts k, const NodeBatchItem *__restrict__ items)
{
    const NodeBatchItem &it = items[blockIdx.z];
    heat_rhs_body<LAP, PAIR, NT>(N, k, static_cast<const double *>(it.in), static_cast<const double *>(it.coarse),
                                 static_cast<double *>(it.out));
}

inline bool use_pairs(int N) { return N % 2 == 0 && N >= PAIR_MIN_N; }
inline dim3 heat_grid(int N, int n)
{
    const int cols = use_pairs(N) ? N / 2 : N;
    return dim3((cols + TB - 1) / TB, (N + HR - 1) / HR, n);
}

}  // namespace

// ------------------------------------------------------------------ launchers
void heat_rhs(hipStream_t s, int N, const HeatConsts &c, const double *U, const double *Q, double *F)
{
    const dim3 g = heat_grid(N, 1), b(TB);
    const bool pairs = use_pairs(N), nt = pairs && N >= NT_MIN_N;
    if (c.lap) {
        if (nt) hipLaunchKernelGGL((k_heat_rhs<true, true, true>), g, b, 0, s, N, c, U, Q, F);
        else if (pairs) hipLaunchKernelGGL((k_heat_rhs<true, true, false>), g, b, 0, s, N, c, U, Q, F);
        else hipLaunchKernelGGL((k_heat_rhs<true, false, false>), g, b, 0, s, N, c, U, Q, F);
    } else {
        if (nt) hipLaunchKernelGGL((k_heat_rhs<false, true, true>), g, b, 0, s, N, c, U, Q, F);
        else if (pairs) hipLaunchKernelGGL((k_heat_rhs<false, true, false>), g, b, 0, s, N, c, U, Q, F);
        else hipLaunchKernelGGL((k_heat_rhs<false, false, false>), g, b, 0, s, N, c, U, Q, F);
    }
}

void heat_rhs_batch(hipStream_t s, int n, int N, const HeatConsts &c, const NodeBatchItem *items)
{
    const dim3 g = heat_grid(N, n), b(TB);
    const bool pairs = use_pairs(N), nt = pairs && N >= NT_MIN_N;
    if (c.lap) {
        if (nt) hipLaunchKernelGGL((k_heat_rhs_b<true, true, true>), g, b, 0, s, N, c, items);
        else if (pairs) hipLaunchKernelGGL((k_heat_rhs_b<true, true, false>), g, b, 0, s, N, c, items);
        else hipLaunchKernelGGL((k_heat_rhs_b<true, false, false>), g, b, 0, s, N, c, items);
    } else {
        if (nt) hipLaunchKernelGGL((k_heat_rhs_b<false, true, true>), g, b, 0, s, N, c, items);
        else if (pairs) hipLaunchKernelGGL((k_heat_rhs_b<false, true, false>), g, b, 0, s, N, c, items);
        else hipLaunchKernelGGL((k_heat_rhs_b<false, false, false>), g, b, 0, s, N, c, items);
    }
}

}  // namespace k
}  // namespace mg
