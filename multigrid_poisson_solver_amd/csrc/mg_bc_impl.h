// mg_bc_impl.h -- the point code of the boundary-kind kernels (include/mg_bc.h; kernels and launchers: mg_bc_kernels.hip).
// The operator, the sweep, the residual and the block sums are mg_varcoef_impl.h's (Faces, faces, bracket, swept, point,
// block_sum), included, not copied: what changes is WHERE they are evaluated (the rectangle of unknowns instead of the
// interior) and which index stands for a neighbour beyond the grid (the mirror point of a Neumann side).  Both are fixed per
// launch on the host from the four kinds (BcGeom) and travel as kernel arguments: wave-uniform scalars, so the row loops
// hold no branch on a kind -- the clamp of the streaming bodies of mg_varcoef_impl.h only gets another target.
#ifndef MG_BC_IMPL_H
#define MG_BC_IMPL_H

#include "mg_varcoef_impl.h"

namespace mg {
namespace k {

namespace {

struct BcGeom {
    int r_lo, r_hi, c_lo, c_hi;       // the unknowns: r_lo <= row <= r_hi and c_lo <= column <= c_hi
    int below, above, west, east;     // the index that stands for row -1, row N, column -1, column N
};

// kind: S, N, W, E (include/mg_bc.h).  A Dirichlet side clamps to its own rim (as mg_varcoef_impl.h does: in bounds, and
// never used by an unknown), a Neumann side to its mirror point.
inline BcGeom bc_geom(int N, const int *kind)
{
    BcGeom g;
    g.r_lo = kind[0] ? 0 : 1;
    g.r_hi = kind[1] ? N - 1 : N - 2;
    g.c_lo = kind[2] ? 0 : 1;
    g.c_hi = kind[3] ? N - 1 : N - 2;
    g.below = kind[0] ? 1 : 0;
    g.above = kind[1] ? N - 2 : N - 1;
    g.west = kind[2] ? 1 : 0;
    g.east = kind[3] ? N - 2 : N - 1;
    return g;
}

// what a streaming body does with a point.  BC_NORM / BC_NORM_F leave per-block partial sums of d^2 (d = the residual / F)
// in k.out and store nothing else; BC_HEAT / BC_HEAT_LOCAL: the heat right-hand side with / without the operator term
// (theta != 1 / theta == 1: no neighbour and no coefficient is read), k.F is the source Q and may be null
enum BcOp { BC_SWEEP, BC_SWEEP_ZERO, BC_RESIDUAL, BC_APPLY, BC_NORM, BC_NORM_F, BC_HEAT, BC_HEAT_LOCAL };

struct BcArgs {
    VcArgs k;
    BcGeom g;
    double sigma, beta, gamma;   // BC_HEAT*
};

template <BcOp OP>
__device__ __forceinline__ double bc_point(const BcArgs &b, const Faces &f, bool has_f, double F, double u, double u_nxt, double u_prv,
                                           double u_east, double u_west)
{
    if constexpr (OP == BC_SWEEP) return point<OP_SWEEP>(b.k, f, F, u, u_nxt, u_prv, u_east, u_west);
    else if constexpr (OP == BC_SWEEP_ZERO) return point<OP_SWEEP_ZERO>(b.k, f, F, u, u_nxt, u_prv, u_east, u_west);
    else if constexpr (OP == BC_RESIDUAL || OP == BC_NORM) return point<OP_RESIDUAL>(b.k, f, F, u, u_nxt, u_prv, u_east, u_west);
    else if constexpr (OP == BC_APPLY) return point<OP_APPLY>(b.k, f, F, u, u_nxt, u_prv, u_east, u_west);
    else if constexpr (OP == BC_NORM_F) return F;
    else {
        double s = -(b.sigma * u);
        if constexpr (OP == BC_HEAT) s = s - b.beta * (b.k.inv * bracket(f, u, u_nxt, u_prv, u_east, u_west));
        if (has_f) s = s - b.gamma * F;
        return s;
    }
}

template <BcOp OP>
struct BcTraits {
    static constexpr bool NORM = OP == BC_NORM || OP == BC_NORM_F;
    static constexpr bool LOCAL = OP == BC_HEAT_LOCAL || OP == BC_NORM_F;        // no neighbour, no coefficient
    static constexpr bool U_MID = OP != BC_SWEEP_ZERO && OP != BC_NORM_F;
    static constexpr bool U_NBR = U_MID && !LOCAL;
    static constexpr bool READS_F = OP != BC_APPLY;
    static constexpr bool OPT_F = OP == BC_HEAT || OP == BC_HEAT_LOCAL;          // k.F may be null
};

// ---------------------------------------------------------------- one column per lane (any N)
template <BcOp OP, bool HAS_A>
__device__ __forceinline__ void bc_cols(const BcArgs &b)
{
    typedef BcTraits<OP> T;
    constexpr bool READS_A = HAS_A && !T::LOCAL;
    const VcArgs &k = b.k;
    const int N = k.N;
    const int c = blockIdx.x * TB + threadIdx.x;
    double acc = 0.0;
    if (c < N) {
        const int r0 = blockIdx.y * ROWS_PB;
        const int cl = c > 0 ? c - 1 : b.g.west, cr = c + 1 < N ? c + 1 : b.g.east;
        const bool col_in = c >= b.g.c_lo && c <= b.g.c_hi;
        const bool has_f = T::READS_F && (!T::OPT_F || k.F != nullptr);   // (uniform over the launch)
        const double *__restrict__ A = k.A;
        const double *__restrict__ U = k.U;
        const double *__restrict__ F = k.F;
        auto row = [&](const double *__restrict__ X, int r) {
            r = r < 0 ? b.g.below : (r < N ? r : b.g.above);
            return X[(size_t)r * N + c];
        };
        double a_prv = 1.0, a_mid = 1.0, u_prv = 0.0, u_mid = 0.0;
        if constexpr (READS_A) {
            a_prv = row(A, r0 - 1);
            a_mid = row(A, r0);
        }
        if constexpr (T::U_NBR) u_prv = row(U, r0 - 1);
        if constexpr (T::U_MID) u_mid = row(U, r0);
#pragma unroll
        for (int i = 0; i < ROWS_PB; ++i) {
            const int r = r0 + i;
            if (r >= N) break;
            double a_nxt = 1.0, u_nxt = 0.0;
            if constexpr (READS_A) a_nxt = row(A, r + 1);
            if constexpr (T::U_MID) u_nxt = row(U, r + 1);   // (the next row's centre, and this row's neighbour)
            const size_t line = (size_t)r * N, p = line + c;
            double v = OP == BC_SWEEP ? u_mid : 0.0;   // a data point: a sweep keeps it, everything else writes +0
            if (col_in && r >= b.g.r_lo && r <= b.g.r_hi) {
                double a_east = 1.0, a_west = 1.0, u_east = 0.0, u_west = 0.0;
                if constexpr (READS_A) {
                    a_east = A[line + cr];
                    a_west = A[line + cl];
                }
                if constexpr (T::U_NBR) {
                    u_east = U[line + cr];
                    u_west = U[line + cl];
                }
                const Faces f = faces(a_mid, a_nxt, a_prv, a_east, a_west, k.sd);
                v = bc_point<OP>(b, f, has_f, has_f ? F[p] : 0.0, u_mid, u_nxt, u_prv, u_east, u_west);
                if constexpr (T::NORM) acc += v * v;
            }
            if constexpr (!T::NORM) {
                if (OP == BC_RESIDUAL && k.sign < 0) v = -v;
                k.out[p] = v;
            }
            a_prv = a_mid;
            a_mid = a_nxt;
            u_prv = u_mid;
            u_mid = u_nxt;
        }
    }
    if constexpr (T::NORM) {
        const double s = block_sum(acc);
        if (threadIdx.x == 0) k.out[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------- two columns per lane, 16-byte accesses
// (even N, 16-byte aligned arrays).  NT: F through non-temporal loads, the output through non-temporal stores; the residual
// stores non-temporally whatever NT, as vc_pairs does.
template <BcOp OP, bool HAS_A, bool NT>
__device__ __forceinline__ void bc_pairs(const BcArgs &b)
{
    typedef BcTraits<OP> T;
    constexpr bool READS_A = HAS_A && !T::LOCAL;
    const VcArgs &k = b.k;
    const int N = k.N;
    const int c = 2 * (blockIdx.x * TB + threadIdx.x);
    double acc = 0.0;
    if (c < N) {
        const int r0 = blockIdx.y * PR;
        const int cl = c > 0 ? c - 1 : b.g.west, cr = c + 2 < N ? c + 2 : b.g.east;
        const bool x_in = c >= b.g.c_lo, y_in = c + 1 <= b.g.c_hi;   // (c <= N - 2 <= c_hi and c + 1 >= 1 >= c_lo)
        const bool has_f = T::READS_F && (!T::OPT_F || k.F != nullptr);
        const double *__restrict__ A = k.A;
        const double *__restrict__ U = k.U;
        const double *__restrict__ F = k.F;
        auto row_pair = [&](const double *__restrict__ X, int r) {
            r = r < 0 ? b.g.below : (r < N ? r : b.g.above);
            return *reinterpret_cast<const double2_v *>(X + (size_t)r * N + c);
        };
        const double2_v one = {1.0, 1.0}, zero = {0.0, 0.0};
        double2_v a_prv = one, a_mid = one, u_prv = zero, u_mid = zero;
        if constexpr (READS_A) {
            a_prv = row_pair(A, r0 - 1);
            a_mid = row_pair(A, r0);
        }
        if constexpr (T::U_NBR) u_prv = row_pair(U, r0 - 1);
        if constexpr (T::U_MID) u_mid = row_pair(U, r0);
#pragma unroll
        for (int i = 0; i < PR; ++i) {
            const int r = r0 + i;
            if (r >= N) break;
            double2_v a_nxt = one, u_nxt = zero;
            if constexpr (READS_A) a_nxt = row_pair(A, r + 1);
            if constexpr (T::U_MID) u_nxt = row_pair(U, r + 1);
            const size_t line = (size_t)r * N, p = line + c;
            double2_v v = zero;
            if (OP == BC_SWEEP) v = u_mid;
            if (r >= b.g.r_lo && r <= b.g.r_hi) {
                double2_v f = zero;
                if (has_f) f = load_f<NT>(F + p);
                if (x_in) {
                    const Faces fc = faces(a_mid.x, a_nxt.x, a_prv.x, a_mid.y, READS_A ? A[line + cl] : 1.0, k.sd);
                    v.x = bc_point<OP>(b, fc, has_f, f.x, u_mid.x, u_nxt.x, u_prv.x, u_mid.y, T::U_NBR ? U[line + cl] : 0.0);
                    if constexpr (T::NORM) acc += v.x * v.x;
                }
                if (y_in) {
                    const Faces fc = faces(a_mid.y, a_nxt.y, a_prv.y, READS_A ? A[line + cr] : 1.0, a_mid.x, k.sd);
                    v.y = bc_point<OP>(b, fc, has_f, f.y, u_mid.y, u_nxt.y, u_prv.y, T::U_NBR ? U[line + cr] : 0.0, u_mid.x);
                    if constexpr (T::NORM) acc += v.y * v.y;
                }
            }
            if constexpr (!T::NORM) {
                if (OP == BC_RESIDUAL && k.sign < 0) v = -v;
                if (NT || OP == BC_RESIDUAL) __builtin_nontemporal_store(v, reinterpret_cast<double2_v *>(k.out + p));
                else *reinterpret_cast<double2_v *>(k.out + p) = v;
            }
            a_prv = a_mid;
            a_mid = a_nxt;
            u_prv = u_mid;
            u_mid = u_nxt;
        }
    }
    if constexpr (T::NORM) {
        const double s = block_sum(acc);
        if (threadIdx.x == 0) k.out[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------- coarse solve
// gs_relative_vc_body (mg_varcoef_impl.h) on the unknowns with mirrored neighbours: ONE workgroup, U and F in LDS, zero
// start, colour 0 = (row + col) even then colour 1, the same stopping rule and state[].  A thread keeps the LDS indices of
// its points' four neighbours beside their face coefficients; Ag == nullptr: a = 1.
// MEAN (include/mg_singular.h, four Neumann sides at shift == 0): the right-hand side first loses its weighted mean m_c, summed
// in the header's order from the values on their way into LDS; err0, the target and the iteration see the projected values,
// Fg itself is not written.  mean_out (may be null): m_c.  Without MEAN the body is what it was, statement for statement.

// the trapezoid weight of point (r, c) of an N x N grid: 1/2 on a side, 1/4 in a corner
__device__ __forceinline__ double mean_weight(int r, int c, int N)
{
    return (r == 0 || r == N - 1 ? 0.5 : 1.0) * (c == 0 || c == N - 1 ? 0.5 : 1.0);
}

template <bool MEAN>
__device__ __forceinline__ void gs_relative_bc_body(int N, BcGeom g, double h2, double inv, double sd, const double *__restrict__ Ag,
                                                    double *__restrict__ Ug, const double *__restrict__ Fg, double atol, double rtol,
                                                    int max_iters, int *__restrict__ state, double *__restrict__ err_out,
                                                    double *__restrict__ mean_out = nullptr)
{
    extern __shared__ __align__(16) double lds[];
    __shared__ double s_val;
    const int n = N * N;
    double *U = lds, *F = lds + n;
    const double denom = (double)((g.r_hi - g.r_lo + 1) * (g.c_hi - g.c_lo + 1));
    Faces fc[GS_PTS];
    double qc[GS_PTS];
    int colour_of[GS_PTS];   // 0 / 1: an unknown of that colour; -1: a data point, or beyond the grid
    int pN[GS_PTS], pS[GS_PTS], pE[GS_PTS], pW[GS_PTS];
    double acc = 0.0;
    [[maybe_unused]] double wacc = 0.0;
#pragma unroll
    for (int j = 0; j < GS_PTS; ++j) {
        const int p = threadIdx.x + j * blockDim.x;
        colour_of[j] = -1;
        fc[j] = Faces{1.0, 1.0, 1.0, 1.0, 4.0};
        qc[j] = 0.25;
        pN[j] = pS[j] = pE[j] = pW[j] = 0;
        if (p < n) {
            const double f = Fg[p];
            F[p] = f;
            U[p] = 0.0;
            const int r = p / N, c = p - r * N;
            if constexpr (MEAN) wacc = wacc + mean_weight(r, c, N) * f;
            if (r >= g.r_lo && r <= g.r_hi && c >= g.c_lo && c <= g.c_hi) {
                if constexpr (!MEAN) acc = acc + fabs(f);
                colour_of[j] = (r + c) & 1;
                pN[j] = (r + 1 < N ? r + 1 : g.above) * N + c;
                pS[j] = (r > 0 ? r - 1 : g.below) * N + c;
                pE[j] = r * N + (c + 1 < N ? c + 1 : g.east);
                pW[j] = r * N + (c > 0 ? c - 1 : g.west);
                if (Ag) fc[j] = faces(Ag[p], Ag[pN[j]], Ag[pS[j]], Ag[pE[j]], Ag[pW[j]], sd);
                else fc[j] = faces(1.0, 1.0, 1.0, 1.0, 1.0, sd);
                qc[j] = 1.0 / fc[j].d;
            }
        }
    }
    if constexpr (MEAN) {
        const double ws = block_sum(wacc);
        if (threadIdx.x == 0) {
            s_val = ws / ((double)(N - 1) * (double)(N - 1));
            if (mean_out) *mean_out = s_val;
        }
        __syncthreads();
        const double m = s_val;
        __syncthreads();   // every thread has read s_val before thread 0 writes err0 into it
#pragma unroll
        for (int j = 0; j < GS_PTS; ++j) {
            const int p = threadIdx.x + j * blockDim.x;
            if (p < n) {   // (a thread's own points, here and in every loop below)
                const double f = F[p] - m;
                F[p] = f;
                if (colour_of[j] >= 0) acc = acc + fabs(f);
            }
        }
    }
    double s = block_sum(acc);
    if (threadIdx.x == 0) s_val = s / denom;
    __syncthreads();
    const double err0 = s_val;
    const double target = rtol * err0 > atol ? rtol * err0 : atol;

    int iterations = 0;
    double err = 0.0;
    for (;;) {
        for (int colour = 0; colour < 2; ++colour) {
#pragma unroll
            for (int j = 0; j < GS_PTS; ++j) {
                const int p = threadIdx.x + j * blockDim.x;
                if (colour_of[j] == colour)
                    U[p] = qc[j] * ((((fc[j].aW * U[pW[j]] + fc[j].aE * U[pE[j]]) + fc[j].aN * U[pN[j]]) + fc[j].aS * U[pS[j]]) - h2 * F[p]);
            }
            __syncthreads();
        }
        ++iterations;
        acc = 0.0;
#pragma unroll
        for (int j = 0; j < GS_PTS; ++j) {
            const int p = threadIdx.x + j * blockDim.x;
            if (colour_of[j] >= 0) acc = acc + fabs(inv * bracket(fc[j], U[p], U[pN[j]], U[pS[j]], U[pE[j]], U[pW[j]]) - F[p]);
        }
        s = block_sum(acc);
        if (threadIdx.x == 0) s_val = s / denom;
        __syncthreads();
        err = s_val;
        __syncthreads();   // every thread has read s_val before thread 0 writes the next one
        if (!(err > target) || iterations >= max_iters) break;
    }
    for (int p = threadIdx.x; p < n; p += blockDim.x) Ug[p] = U[p];
    if (threadIdx.x == 0) {
        state[0] = 1;
        state[1] = iterations;
        state[2] = err > target ? 1 : 0;
        state[3] = 0;
        if (err_out) {
            err_out[0] = err0;
            err_out[1] = err;
        }
    }
}

// ---------------------------------------------------------------- transfers, one point per lane
// F_c = doRestriction's expression at the coarse unknowns (g: the geometry of the M x M grid), +0 at coarse data points; the
// end entries of the table are replaced as coef_coarsen_body replaces them
__device__ __forceinline__ void restrict_bc_body(int N, const double *__restrict__ D, int M, BcGeom g, double *__restrict__ Fc,
                                                 const int *__restrict__ lo, const double *__restrict__ w)
{
    const int cc = blockIdx.x * TB + threadIdx.x;
    const int rc = blockIdx.y;
    if (cc >= M) return;
    double v = 0.0;
    if (rc >= g.r_lo && rc <= g.r_hi && cc >= g.c_lo && cc <= g.c_hi) {
        auto entry = [&](int i, int *l, double *wt) {
            if (i == 0) { *l = 0; *wt = 0.0; }
            else if (i == M - 1) { *l = N - 2; *wt = 1.0; }
            else { *l = lo[i]; *wt = w[i]; }
        };
        int lc, lr;
        double a, c;
        entry(cc, &lc, &a);
        entry(rc, &lr, &c);
        const double b = 1.0 - a, d = 1.0 - c;
        const size_t f = (size_t)lc + (size_t)lr * N;
        v = b * d * D[f] + a * d * D[f + 1] + c * b * D[f + N] + a * c * D[f + N + 1];
    }
    Fc[(size_t)rc * M + cc] = v;
}

// U_out = U_in + P(U_c) at the fine unknowns (g: the geometry of the N x N grid), U_in at fine data points; (lo, w): the
// table of mg_boundary_prolongation_table(M, N), ends included
__device__ __forceinline__ void prolong_add_bc_body(int M, const double *__restrict__ Uc, int N, BcGeom g, const double *__restrict__ Uin,
                                                    double *__restrict__ Uout, const int *__restrict__ lo, const double *__restrict__ w)
{
    const int cf = blockIdx.x * TB + threadIdx.x;
    const int rf = blockIdx.y;
    if (cf >= N) return;
    const size_t p = (size_t)rf * N + cf;
    double v = Uin[p];
    if (rf >= g.r_lo && rf <= g.r_hi && cf >= g.c_lo && cf <= g.c_hi) {
        const double a = w[cf], c = w[rf];
        const double b = 1.0 - a, d = 1.0 - c;
        const size_t f = (size_t)lo[cf] + (size_t)lo[rf] * M;
        v = v + (b * d * Uc[f] + a * d * Uc[f + 1] + c * b * Uc[f + M] + a * c * Uc[f + M + 1]);
    }
    Uout[p] = v;
}

// F_out = F - (t*a)*g at the rim unknowns of Neumann sides, in the order S, N, W, E; a copy elsewhere.  kS .. kE: the kinds
__device__ __forceinline__ void neumann_source_body(int N, double t, int kS, int kN, int kW, int kE, BcGeom g,
                                                    const double *__restrict__ A, const double *__restrict__ F,
                                                    const double *__restrict__ G, double *__restrict__ Fout)
{
    const int c = blockIdx.x * TB + threadIdx.x;
    const int r = blockIdx.y;
    if (c >= N) return;
    const size_t p = (size_t)r * N + c;
    double v = F[p];
    const bool edge = r == 0 || r == N - 1 || c == 0 || c == N - 1;
    if (edge && r >= g.r_lo && r <= g.r_hi && c >= g.c_lo && c <= g.c_hi) {
        const double ta = t * (A ? A[p] : 1.0);
        if (kS && r == 0) v = v - ta * G[c];
        if (kN && r == N - 1) v = v - ta * G[(size_t)N + c];
        if (kW && c == 0) v = v - ta * G[2 * (size_t)N + r];
        if (kE && c == N - 1) v = v - ta * G[3 * (size_t)N + r];
    }
    Fout[p] = v;
}

}  // namespace

}  // namespace k
}  // namespace mg

#endif /* MG_BC_IMPL_H */
