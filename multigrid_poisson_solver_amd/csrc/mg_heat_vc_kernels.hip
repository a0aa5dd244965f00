// mg_heat_vc_kernels.hip -- the right-hand side of a theta-scheme time step of u_t = nu*div(a grad u) + q
// (include/mg_heat_vc.h; driven by mg_heat.cpp):  F = -(sigma*u) - beta*inv*b(u) - gamma*q  on the interior, +0 on the rim,
// b(u) the bracket of include/mg_varcoef.h with sd = 0.  Only theta != 1 comes here: with theta == 1 the right-hand side reads
// neither a neighbour nor a, and the driver launches k_heat_rhs<false, ...> (mg_heat_kernels.hip) as it always did.
// Built with -ffp-contract=off like every kernel file: the header fixes the evaluation order (every product and every sum
// rounded once) so that numpy restates it bit for bit, and so that a == 1 gives the bits of k_heat_rhs<true, ...>.
// Memory-bound: 24 B (U, a, F) or 32 B (and Q) per point, the traffic of k_residual_vc, and no division.  The shapes and
// thresholds are k_heat_rhs's: a lane walks HR rows down its column (any N) or its column pair (even N from PAIR_MIN_N on,
// 16-byte accesses) with a rolling window of three rows of U AND of a in registers, as k_residual_vc keeps it, so each value
// comes from memory once per block column (the east / west neighbours are the neighbouring lanes' values: L1 hits); from
// NT_MIN_N on F leaves through non-temporal stores and Q comes in through non-temporal loads.  No LDS.
#include <hip/hip_runtime.h>

#include "mg_internal.h"

namespace mg {
namespace k {

namespace {

constexpr int TB = 256;          // threads per block
constexpr int HR = 4;            // rows per lane
constexpr int PAIR_MIN_N = 512;  // even N from here on: two columns per lane, 16-byte accesses
constexpr int NT_MIN_N = 4096;   // the arrays are far larger than the caches: non-temporal accesses of F and Q
typedef double double2_h __attribute__((ext_vector_type(2)));

// one interior point in the header's order; nxt / prv: rows r+1 / r-1, east / west: columns c+1 / c-1
__device__ __forceinline__ double heat_point_vc(const HeatConsts &k, double a, double a_nxt, double a_prv, double a_east,
                                                double a_west, double u, double u_nxt, double u_prv, double u_east, double u_west,
                                                bool has_q, double q)
{
    const double aN = 0.5 * (a + a_nxt);
    const double aS = 0.5 * (a + a_prv);
    const double aE = 0.5 * (a + a_east);
    const double aW = 0.5 * (a + a_west);
    const double d = ((aN + aS) + aE) + aW;
    const double b = (((aN * u_nxt + aS * u_prv) + aE * u_east) + aW * u_west) - d * u;
    const double lap = k.inv * b;
    double s = -(k.sigma * u);
    s = s - k.beta * lap;
    if (has_q) s = s - k.gamma * q;
    return s;
}

// one column per lane (any N)
__device__ __forceinline__ void heat_rhs_vc_cols(int N, const HeatConsts &k, const double *__restrict__ A,
                                                 const double *__restrict__ U, const double *__restrict__ Q, double *__restrict__ F)
{
    const int c = blockIdx.x * TB + threadIdx.x;
    if (c >= N) return;
    const int r0 = blockIdx.y * HR;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 1 < N ? c + 1 : N - 1;
    const bool col_in = c > 0 && c < N - 1;
    const bool has_q = Q != nullptr;   // (uniform over the block)
    auto row = [&](const double *__restrict__ X, int r) {
        r = r < 0 ? 0 : (r < N ? r : N - 1);   // (rows beyond the grid: clamped, never used)
        return X[(size_t)r * N + c];
    };
    double a_prv = row(A, r0 - 1), a_mid = row(A, r0), u_prv = row(U, r0 - 1), u_mid = row(U, r0);
#pragma unroll
    for (int i = 0; i < HR; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        const double a_nxt = row(A, r + 1), u_nxt = row(U, r + 1);
        const size_t line = (size_t)r * N, p = line + c;
        double v = 0.0;
        if (col_in && r > 0 && r < N - 1)
            v = heat_point_vc(k, a_mid, a_nxt, a_prv, A[line + cr], A[line + cl], u_mid, u_nxt, u_prv, U[line + cr], U[line + cl],
                              has_q, has_q ? Q[p] : 0.0);
        F[p] = v;
        a_prv = a_mid;
        a_mid = a_nxt;
        u_prv = u_mid;
        u_mid = u_nxt;
    }
}

// two columns per lane, 16-byte accesses (even N, 16-byte aligned arrays: every pair is aligned and inside its row)
template <bool NT>
__device__ __forceinline__ void heat_rhs_vc_pairs(int N, const HeatConsts &k, const double *__restrict__ A,
                                                  const double *__restrict__ U, const double *__restrict__ Q, double *__restrict__ F)
{
    const int c = 2 * (blockIdx.x * TB + threadIdx.x);
    if (c >= N) return;
    const int r0 = blockIdx.y * HR;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 2 < N ? c + 2 : N - 1;
    const bool has_q = Q != nullptr;
    auto row_pair = [&](const double *__restrict__ X, int r) {
        r = r < 0 ? 0 : (r < N ? r : N - 1);
        return *reinterpret_cast<const double2_h *>(X + (size_t)r * N + c);
    };
    double2_h a_prv = row_pair(A, r0 - 1), a_mid = row_pair(A, r0), u_prv = row_pair(U, r0 - 1), u_mid = row_pair(U, r0);
#pragma unroll
    for (int i = 0; i < HR; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        const double2_h a_nxt = row_pair(A, r + 1), u_nxt = row_pair(U, r + 1);
        const size_t line = (size_t)r * N, p = line + c;
        double2_h v = {0.0, 0.0};
        if (r > 0 && r < N - 1) {
            double2_h q = {0.0, 0.0};
            if (has_q) {
                if constexpr (NT) q = __builtin_nontemporal_load(reinterpret_cast<const double2_h *>(Q + p));
                else q = *reinterpret_cast<const double2_h *>(Q + p);
            }
            if (c > 0)
                v.x = heat_point_vc(k, a_mid.x, a_nxt.x, a_prv.x, a_mid.y, A[line + cl], u_mid.x, u_nxt.x, u_prv.x, u_mid.y,
                                    U[line + cl], has_q, q.x);
            if (c + 1 < N - 1)
                v.y = heat_point_vc(k, a_mid.y, a_nxt.y, a_prv.y, A[line + cr], a_mid.x, u_mid.y, u_nxt.y, u_prv.y, U[line + cr],
                                    u_mid.x, has_q, q.y);
        }
        if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<double2_h *>(F + p));
        else *reinterpret_cast<double2_h *>(F + p) = v;
        a_prv = a_mid;
        a_mid = a_nxt;
        u_prv = u_mid;
        u_mid = u_nxt;
    }
}

template <bool PAIR, bool NT>
__global__ __launch_bounds__(TB) void k_heat_rhs_vc(int N, HeatConsts k, const double *__restrict__ A, const double *__restrict__ U,
                                                    const double *__restrict__ Q, double *__restrict__ F)
{
    if constexpr (PAIR) heat_rhs_vc_pairs<NT>(N, k, A, U, Q, F);
    else heat_rhs_vc_cols(N, k, A, U, Q, F);
}

inline bool use_pairs(int N) { return N % 2 == 0 && N >= PAIR_MIN_N; }

}  // namespace

// ------------------------------------------------------------------ launcher
void heat_rhs_vc(hipStream_t s, int N, const HeatConsts &c, const double *A, const double *U, const double *Q, double *F)
{
    const bool pairs = use_pairs(N), nt = pairs && N >= NT_MIN_N;
    const int cols = pairs ? N / 2 : N;
    const dim3 g((cols + TB - 1) / TB, (N + HR - 1) / HR), b(TB);
    if (nt) hipLaunchKernelGGL((k_heat_rhs_vc<true, true>), g, b, 0, s, N, c, A, U, Q, F);
    else if (pairs) hipLaunchKernelGGL((k_heat_rhs_vc<true, false>), g, b, 0, s, N, c, A, U, Q, F);
    else hipLaunchKernelGGL((k_heat_rhs_vc<false, false>), g, b, 0, s, N, c, A, U, Q, F);
}

}  // namespace k
}  // namespace mg
