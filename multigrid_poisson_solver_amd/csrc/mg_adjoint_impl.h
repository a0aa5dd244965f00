// mg_adjoint_impl.h -- the __device__ bodies of the adjoint-gradient kernels (include/mg_adjoint.h), shared by the single
// launches and their batched twins in mg_adjoint_kernels.hip so that an instance of a batched launch runs the code and the
// block partition of its single launch.  The header fixes the evaluation order (every difference, product and sum rounded
// once); the file is built with -ffp-contract=off like every kernel file, so numpy restates it bit for bit
// (tests/_adjoint_ref.py).
// Coefficient gradient: memory-bound, 24 B per point (lam, U read, gA written) in the access shape of k_heat_rhs_vc: a lane
// walks HR rows down its column (any N) or its column pair (even N from PAIR_MIN_N on, 16-byte accesses) with a rolling
// window of three rows of lam' AND of U in registers, so each value comes from memory once per block column (the east /
// west neighbours are the neighbouring lanes' values: L1 hits); from NT_MIN_N on gA leaves through non-temporal stores.
// lam' is lam with its rim replaced by +0.0 IN REGISTERS as the window is filled: the rim of lam in memory is loaded (the
// window is uniform) and never used.  No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>

namespace mg {
namespace k {
namespace adj {

constexpr int TB = 256;          // threads per block
constexpr int HR = 4;            // rows per lane
constexpr int PAIR_MIN_N = 512;  // even N from here on: two columns per lane, 16-byte accesses
constexpr int NT_MIN_N = 4096;   // the arrays are far larger than the caches: non-temporal stores of gA
typedef double double2_h __attribute__((ext_vector_type(2)));

// one term of the header's sum: the neighbour q of k in one direction (inside: q lies in the grid)
__device__ __forceinline__ double adj_term(bool inside, double lam_k, double lam_q, double u_k, double u_q)
{
    return inside ? (lam_k - lam_q) * (u_k - u_q) : 0.0;
}

// one grid point in the header's order; nxt / prv: rows r+1 / r-1, east / west: columns c+1 / c-1; has_*: that neighbour
// lies in the grid
__device__ __forceinline__ double coef_grad_point(double h, double l, double l_nxt, double l_prv, double l_east, double l_west, double u,
                                                  double u_nxt, double u_prv, double u_east, double u_west, bool has_nxt, bool has_prv,
                                                  bool has_east, bool has_west)
{
    const double tN = adj_term(has_nxt, l, l_nxt, u, u_nxt);
    const double tS = adj_term(has_prv, l, l_prv, u, u_prv);
    const double tE = adj_term(has_east, l, l_east, u, u_east);
    const double tW = adj_term(has_west, l, l_west, u, u_west);
    return h * ((((0.0 + tN) + tS) + tE) + tW);
}

// one column per lane (any N)
__device__ __forceinline__ void coef_grad_cols(int N, double h, const double *__restrict__ Lm, const double *__restrict__ U,
                                               double *__restrict__ G)
{
    const int c = blockIdx.x * TB + threadIdx.x;
    if (c >= N) return;
    const int r0 = blockIdx.y * HR;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 1 < N ? c + 1 : N - 1;
    const bool col_in = c > 0 && c < N - 1, cl_in = cl > 0, cr_in = cr < N - 1;   // (cl < N - 1 and cr > 0 always: N >= 3)
    auto row = [&](const double *__restrict__ X, int r) {
        r = r < 0 ? 0 : (r < N ? r : N - 1);   // (rows beyond the grid: clamped, never used)
        return X[(size_t)r * N + c];
    };
    auto row_in = [&](int r) { return r > 0 && r < N - 1; };
    // lam' of this column: +0.0 on the rim, whatever memory holds there
    auto lam_row = [&](int r) {
        const double v = row(Lm, r);
        return col_in && row_in(r) ? v : 0.0;
    };
    double l_prv = lam_row(r0 - 1), l_mid = lam_row(r0), u_prv = row(U, r0 - 1), u_mid = row(U, r0);
#pragma unroll
    for (int i = 0; i < HR; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        const double l_nxt = lam_row(r + 1), u_nxt = row(U, r + 1);
        const size_t line = (size_t)r * N;
        const bool rin = row_in(r);
        const double l_east = Lm[line + cr], l_west = Lm[line + cl];
        G[line + c] = coef_grad_point(h, l_mid, l_nxt, l_prv, rin && cr_in ? l_east : 0.0, rin && cl_in ? l_west : 0.0, u_mid, u_nxt,
                                      u_prv, U[line + cr], U[line + cl], r + 1 < N, r > 0, c + 1 < N, c > 0);
        l_prv = l_mid;
        l_mid = l_nxt;
        u_prv = u_mid;
        u_mid = u_nxt;
    }
}

// two columns per lane, 16-byte accesses (even N, 16-byte aligned arrays: every pair is aligned and inside its row)
template <bool NT>
__device__ __forceinline__ void coef_grad_pairs(int N, double h, const double *__restrict__ Lm, const double *__restrict__ U,
                                                double *__restrict__ G)
{
    const int c = 2 * (blockIdx.x * TB + threadIdx.x);
    if (c >= N) return;
    const int r0 = blockIdx.y * HR;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 2 < N ? c + 2 : N - 1;
    const bool x_in = c > 0, y_in = c + 1 < N - 1, cl_in = cl > 0, cr_in = cr < N - 1;
    auto row_pair = [&](const double *__restrict__ X, int r) {
        r = r < 0 ? 0 : (r < N ? r : N - 1);
        return *reinterpret_cast<const double2_h *>(X + (size_t)r * N + c);
    };
    auto row_in = [&](int r) { return r > 0 && r < N - 1; };
    auto lam_pair = [&](int r) {
        double2_h v = row_pair(Lm, r);
        const bool rin = row_in(r);
        v.x = rin && x_in ? v.x : 0.0;
        v.y = rin && y_in ? v.y : 0.0;
        return v;
    };
    double2_h l_prv = lam_pair(r0 - 1), l_mid = lam_pair(r0), u_prv = row_pair(U, r0 - 1), u_mid = row_pair(U, r0);
#pragma unroll
    for (int i = 0; i < HR; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        const double2_h l_nxt = lam_pair(r + 1), u_nxt = row_pair(U, r + 1);
        const size_t line = (size_t)r * N, p = line + c;
        const bool rin = row_in(r), has_nxt = r + 1 < N, has_prv = r > 0;
        const double l_east = Lm[line + cr], l_west = Lm[line + cl];
        double2_h v;
        v.x = coef_grad_point(h, l_mid.x, l_nxt.x, l_prv.x, l_mid.y, rin && cl_in ? l_west : 0.0, u_mid.x, u_nxt.x, u_prv.x, u_mid.y,
                              U[line + cl], has_nxt, has_prv, true, c > 0);
        v.y = coef_grad_point(h, l_mid.y, l_nxt.y, l_prv.y, rin && cr_in ? l_east : 0.0, l_mid.x, u_mid.y, u_nxt.y, u_prv.y,
                              U[line + cr], u_mid.x, has_nxt, has_prv, c + 2 < N, true);
        if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<double2_h *>(G + p));
        else *reinterpret_cast<double2_h *>(G + p) = v;
        l_prv = l_mid;
        l_mid = l_nxt;
        u_prv = u_mid;
        u_mid = u_nxt;
    }
}

// the gradient in the rim data: one pass over gU -- +0.0 on the interior (the zero fill), Ubar (or +0.0) at the corners, and
// O(N) work on the rest of the rim, each of whose points has ONE interior neighbour p.  One column per lane, HR rows.
// A == nullptr: f = 1.0; Ubar == nullptr: 0.0 (both uniform over the launch, or over the instance of a batched one)
__device__ __forceinline__ void rim_grad_cols(int N, double inv, const double *__restrict__ A, const double *__restrict__ Lm,
                                              const double *__restrict__ Ubar, double *__restrict__ G)
{
    const int c = blockIdx.x * TB + threadIdx.x;
    if (c >= N) return;
    const int r0 = blockIdx.y * HR;
    const bool col_in = c > 0 && c < N - 1;
#pragma unroll
    for (int i = 0; i < HR; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        const bool row_in = r > 0 && r < N - 1;
        const size_t b = (size_t)r * N + c;
        double v = 0.0;
        if (!(row_in && col_in)) {
            v = Ubar ? Ubar[b] : 0.0;
            if (row_in || col_in) {   // not a corner: the neighbour one step inside
                const int pr = row_in ? r : (r == 0 ? 1 : N - 2), pc = col_in ? c : (c == 0 ? 1 : N - 2);
                const size_t p = (size_t)pr * N + pc;
                const double f = A ? 0.5 * (A[b] + A[p]) : 1.0;
                v = v - inv * (f * Lm[p]);
            }
        }
        G[b] = v;
    }
}

}  // namespace adj
}  // namespace k
}  // namespace mg
