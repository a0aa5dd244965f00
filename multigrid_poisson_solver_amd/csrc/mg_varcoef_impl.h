// mg_varcoef_impl.h -- the point code of the variable-coefficient kernels (include/mg_varcoef.h) AND of the reaction kernels
// (include/mg_reaction.h): ONE column body, ONE pair body, ONE norm body and ONE coarse solve, with two compile-time switches.
//   HAS_A   a coefficient a(x, y) is streamed (rolling window of three rows); false: no array of ones is read, a = 1 goes
//           through the same expressions (every face exactly 1)
//   HAS_S   a nodal reaction term s(x, y) is streamed: the centre gets sd + s*dx2 per point (one load at the centre row, no
//           window) instead of the level constant sd; false: k.S is not looked at
// The `_vc` kernels are <HAS_A = true, HAS_S = false> (the operator alone also without a), the `_rx` kernels <HAS_A either,
// HAS_S = true>.  A further per-point term of the centre plugs in the same way: a pointer in VcArgs, a switch, and its
// expression in centre_sd -- the row loops, the rim and the stores are not touched.
// The bodies are shared by the single-instance kernels (mg_varcoef_kernels.hip, mg_reaction_kernels.hip) and their batched
// forms (mg_varcoef_batch_kernels.hip, mg_reaction_batch_kernels.hip): all translation units compile THESE bodies with the
// same flags (-ffp-contract=off), so an instance of a batched launch runs the code, the block partition and the summation
// order of its single launch and gives the same bits.  A body takes the arrays of one instance as arguments and reads
// blockIdx.x / blockIdx.y only as (column block, row block) of that instance; which instance a block works on is the caller's
// business (blockIdx.z of the batched streaming kernels, blockIdx.x of the one-workgroup ones).  The block shape, the block
// sums and the norm's finish are mg_solver_common.h's, the ones mg_solve_kernels.hip runs: the norm of a == 1 is the constant
// norm bit for bit (test_unit_coefficient_is_the_constant_solver compares the histories with ==).
// Everything here sits in an unnamed namespace: each translation unit has its own copy.
#ifndef MG_VARCOEF_IMPL_H
#define MG_VARCOEF_IMPL_H

#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_solver_common.h"

namespace mg {
namespace k {

namespace {

template <bool NT>
__device__ __forceinline__ double2_v load_f(const double *p)
{
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const double2_v *>(p));
    return *reinterpret_cast<const double2_v *>(p);
}

// the operator at one interior point (include/mg_varcoef.h): face coefficients and centre; nxt / prv: rows r+1 / r-1
struct Faces {
    double aN, aS, aE, aW, d;
};
__device__ __forceinline__ Faces faces(double a, double a_nxt, double a_prv, double a_east, double a_west, double sd)
{
    Faces f;
    f.aN = 0.5 * (a + a_nxt);
    f.aS = 0.5 * (a + a_prv);
    f.aE = 0.5 * (a + a_east);
    f.aW = 0.5 * (a + a_west);
    f.d = (((f.aN + f.aS) + f.aE) + f.aW) + sd;
    return f;
}
__device__ __forceinline__ double bracket(const Faces &f, double u, double u_nxt, double u_prv, double u_east, double u_west)
{
    return (((f.aN * u_nxt + f.aS * u_prv) + f.aE * u_east) + f.aW * u_west) - f.d * u;
}
// the sweep's new value; ZERO_IN: from the zero field
template <bool ZERO_IN>
__device__ __forceinline__ double swept(const Faces &f, double omega, double dx2, double F, double u, double u_nxt, double u_prv,
                                        double u_east, double u_west)
{
    const double q = 1.0 / f.d;
    const double c = omega * q;
    if (ZERO_IN) return 0.0 + c * (0.0 - dx2 * F);
    return u + c * (bracket(f, u, u_nxt, u_prv, u_east, u_west) - dx2 * F);
}

// what a streaming kernel does with the bracket of a point
enum Op { OP_SWEEP, OP_SWEEP_ZERO, OP_RESIDUAL, OP_APPLY };

struct VcArgs {
    int N;
    double dx2, inv, sd, omega;
    const double *A, *U, *F;   // coefficient, field (not read by OP_SWEEP_ZERO), source (not read by OP_APPLY)
    double *out;               // (the norm: its per-block partials)
    int sign;                  // OP_RESIDUAL
    const double *S;           // HAS_S: the level's nodal reaction term (needs dx2 whatever the operation); else not read
};

// the centre's shift term of one point: the level constant, or with a reaction term (include/mg_reaction.h) t = s*dx2,
// sdp = sd + t, each rounded once
template <bool HAS_S>
__device__ __forceinline__ double centre_sd(const VcArgs &k, double s)
{
    if constexpr (HAS_S) return k.sd + s * k.dx2;
    else return k.sd;
}

template <Op OP>
__device__ __forceinline__ double point(const VcArgs &k, const Faces &f, double F, double u, double u_nxt, double u_prv,
                                        double u_east, double u_west)
{
    if constexpr (OP == OP_SWEEP) return swept<false>(f, k.omega, k.dx2, F, u, u_nxt, u_prv, u_east, u_west);
    else if constexpr (OP == OP_SWEEP_ZERO) return swept<true>(f, k.omega, k.dx2, F, 0.0, 0.0, 0.0, 0.0, 0.0);
    else if constexpr (OP == OP_RESIDUAL) return k.inv * bracket(f, u, u_nxt, u_prv, u_east, u_west) - F;
    else return k.inv * bracket(f, u, u_nxt, u_prv, u_east, u_west);
}

// ---------------------------------------------------------------- one column per lane (any N)
template <Op OP, bool HAS_A, bool HAS_S>
__device__ __forceinline__ void vc_cols(const VcArgs &k)
{
    const int N = k.N;
    const int c = blockIdx.x * TB + threadIdx.x;
    if (c >= N) return;
    const int r0 = blockIdx.y * ROWS_PB;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 1 < N ? c + 1 : N - 1;
    const bool col_in = c > 0 && c < N - 1;
    constexpr bool READS_U = OP != OP_SWEEP_ZERO, READS_F = OP != OP_APPLY;
    const double *__restrict__ A = k.A;
    const double *__restrict__ S = k.S;
    const double *__restrict__ U = k.U;
    const double *__restrict__ F = k.F;
    auto row = [&](const double *__restrict__ X, int r) {
        r = r < 0 ? 0 : (r < N ? r : N - 1);   // (rows beyond the grid: clamped, never used)
        return X[(size_t)r * N + c];
    };
    double a_prv = 1.0, a_mid = 1.0, u_prv = 0.0, u_mid = 0.0;
    if constexpr (HAS_A) {
        a_prv = row(A, r0 - 1);
        a_mid = row(A, r0);
    }
    if constexpr (READS_U) {
        u_prv = row(U, r0 - 1);
        u_mid = row(U, r0);
    }
#pragma unroll
    for (int i = 0; i < ROWS_PB; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        double a_nxt = 1.0, u_nxt = 0.0;
        if constexpr (HAS_A) a_nxt = row(A, r + 1);
        if constexpr (READS_U) u_nxt = row(U, r + 1);
        const size_t line = (size_t)r * N, p = line + c;
        double v = OP == OP_SWEEP ? u_mid : 0.0;   // the rim: a sweep keeps it, everything else writes +0
        if (col_in && r > 0 && r < N - 1) {
            double a_east = 1.0, a_west = 1.0, u_east = 0.0, u_west = 0.0;
            if constexpr (HAS_A) {
                a_east = A[line + cr];
                a_west = A[line + cl];
            }
            if constexpr (READS_U) {
                u_east = U[line + cr];
                u_west = U[line + cl];
            }
            const Faces f = faces(a_mid, a_nxt, a_prv, a_east, a_west, centre_sd<HAS_S>(k, HAS_S ? S[p] : 0.0));
            v = point<OP>(k, f, READS_F ? F[p] : 0.0, u_mid, u_nxt, u_prv, u_east, u_west);
        }
        if (OP == OP_RESIDUAL && k.sign < 0) v = -v;
        k.out[p] = v;
        a_prv = a_mid;
        a_mid = a_nxt;
        u_prv = u_mid;
        u_mid = u_nxt;
    }
}

// ---------------------------------------------------------------- two columns per lane, 16-byte accesses
// (even N, 16-byte aligned arrays: every pair is aligned and inside its row).  NT: F and s through non-temporal loads and
// the output through non-temporal stores.  The sweeps take NT from NT_MIN_N on; the residual -- whose output is read once, by
// the restriction -- is instantiated with NT = true only, whatever N, as k_residual_pairs.
template <Op OP, bool NT, bool HAS_A, bool HAS_S>
__device__ __forceinline__ void vc_pairs(const VcArgs &k)
{
    const int N = k.N;
    const int c = 2 * (blockIdx.x * TB + threadIdx.x);
    if (c >= N) return;
    const int r0 = blockIdx.y * PR;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 2 < N ? c + 2 : N - 1;
    constexpr bool READS_U = OP != OP_SWEEP_ZERO;
    const double *__restrict__ A = k.A;
    const double *__restrict__ S = k.S;
    const double *__restrict__ U = k.U;
    const double *__restrict__ F = k.F;
    auto row_pair = [&](const double *__restrict__ X, int r) {
        r = r < 0 ? 0 : (r < N ? r : N - 1);
        return *reinterpret_cast<const double2_v *>(X + (size_t)r * N + c);
    };
    const double2_v ones = {1.0, 1.0};
    double2_v a_prv = ones, a_mid = ones, u_prv = {0.0, 0.0}, u_mid = {0.0, 0.0};
    if constexpr (HAS_A) {
        a_prv = row_pair(A, r0 - 1);
        a_mid = row_pair(A, r0);
    }
    if constexpr (READS_U) {
        u_prv = row_pair(U, r0 - 1);
        u_mid = row_pair(U, r0);
    }
#pragma unroll
    for (int i = 0; i < PR; ++i) {
        const int r = r0 + i;
        if (r >= N) break;
        double2_v a_nxt = ones, u_nxt = {0.0, 0.0};
        if constexpr (HAS_A) a_nxt = row_pair(A, r + 1);
        if constexpr (READS_U) u_nxt = row_pair(U, r + 1);
        const size_t line = (size_t)r * N, p = line + c;
        double2_v v = {0.0, 0.0};
        if (OP == OP_SWEEP) v = u_mid;
        if (r > 0 && r < N - 1) {
            const double2_v f = load_f<NT>(F + p);
            double2_v s = {0.0, 0.0};
            if constexpr (HAS_S) s = load_f<NT>(S + p);
            if (c > 0) {
                const Faces fc = faces(a_mid.x, a_nxt.x, a_prv.x, a_mid.y, HAS_A ? A[line + cl] : 1.0, centre_sd<HAS_S>(k, s.x));
                v.x = point<OP>(k, fc, f.x, u_mid.x, u_nxt.x, u_prv.x, u_mid.y, READS_U ? U[line + cl] : 0.0);
            }
            if (c + 1 < N - 1) {
                const Faces fc = faces(a_mid.y, a_nxt.y, a_prv.y, HAS_A ? A[line + cr] : 1.0, a_mid.x, centre_sd<HAS_S>(k, s.y));
                v.y = point<OP>(k, fc, f.y, u_mid.y, u_nxt.y, u_prv.y, READS_U ? U[line + cr] : 0.0, u_mid.x);
            }
        }
        if (OP == OP_RESIDUAL && k.sign < 0) v = -v;
        if (NT || OP == OP_RESIDUAL) __builtin_nontemporal_store(v, reinterpret_cast<double2_v *>(k.out + p));
        else *reinterpret_cast<double2_v *>(k.out + p) = v;
        a_prv = a_mid;
        a_mid = a_nxt;
        u_prv = u_mid;
        u_mid = u_nxt;
    }
}

// ---------------------------------------------------------------- residual L2 norm
// per-block partial sums of d^2 over interior points, d = inv*b(U) - F, in the partition and the order of k_resnorm /
// k_resnorm_pairs (mg_solve_kernels.hip) for the same N; nothing but the partials (k.out) is written
template <bool PAIR, bool NT, bool HAS_A, bool HAS_S>
__device__ __forceinline__ void resnorm_vc_body(const VcArgs &k)
{
    const int N = k.N;
    const double inv = k.inv;
    const double *__restrict__ A = k.A;
    const double *__restrict__ S = k.S;
    const double *__restrict__ U = k.U;
    const double *__restrict__ F = k.F;
    double acc = 0.0;
    if constexpr (!PAIR) {
        const int c = blockIdx.x * TB + threadIdx.x;
        const int r0 = blockIdx.y * ROWS_PB;
        if (c < N) {
#pragma unroll
            for (int i = 0; i < ROWS_PB; ++i) {
                const int r = r0 + i;
                if (r < N && !rim(r, c, N)) {
                    const size_t p = (size_t)r * N + c;
                    const double sdp = centre_sd<HAS_S>(k, HAS_S ? S[p] : 0.0);
                    const Faces f = HAS_A ? faces(A[p], A[p + N], A[p - N], A[p + 1], A[p - 1], sdp) : faces(1.0, 1.0, 1.0, 1.0, 1.0, sdp);
                    const double d = inv * bracket(f, U[p], U[p + N], U[p - N], U[p + 1], U[p - 1]) - F[p];
                    acc += d * d;
                }
            }
        }
    } else {
        const int c = 2 * (blockIdx.x * TB + threadIdx.x);
        const int r0 = blockIdx.y * PR;
        if (c < N) {
            const int cl = c > 0 ? c - 1 : 0, cr = c + 2 < N ? c + 2 : N - 1;
            auto row_pair = [&](const double *__restrict__ X, int r) {
                r = r < 0 ? 0 : (r < N ? r : N - 1);
                return *reinterpret_cast<const double2_v *>(X + (size_t)r * N + c);
            };
            const double2_v ones = {1.0, 1.0};
            double2_v a_prv = ones, a_mid = ones, u_prv = row_pair(U, r0 - 1), u_mid = row_pair(U, r0);
            if constexpr (HAS_A) {
                a_prv = row_pair(A, r0 - 1);
                a_mid = row_pair(A, r0);
            }
#pragma unroll
            for (int i = 0; i < PR; ++i) {
                const int r = r0 + i;
                if (r >= N) break;
                double2_v a_nxt = ones;
                if constexpr (HAS_A) a_nxt = row_pair(A, r + 1);
                const double2_v u_nxt = row_pair(U, r + 1);
                if (r > 0 && r < N - 1) {
                    const size_t line = (size_t)r * N;
                    const double2_v f = load_f<NT>(F + line + c);
                    double2_v s = {0.0, 0.0};
                    if constexpr (HAS_S) s = load_f<NT>(S + line + c);
                    if (c > 0) {
                        const Faces fc = faces(a_mid.x, a_nxt.x, a_prv.x, a_mid.y, HAS_A ? A[line + cl] : 1.0, centre_sd<HAS_S>(k, s.x));
                        const double d = inv * bracket(fc, u_mid.x, u_nxt.x, u_prv.x, u_mid.y, U[line + cl]) - f.x;
                        acc += d * d;
                    }
                    if (c + 1 < N - 1) {
                        const Faces fc = faces(a_mid.y, a_nxt.y, a_prv.y, HAS_A ? A[line + cr] : 1.0, a_mid.x, centre_sd<HAS_S>(k, s.y));
                        const double d = inv * bracket(fc, u_mid.y, u_nxt.y, u_prv.y, U[line + cr], u_mid.x) - f.y;
                        acc += d * d;
                    }
                }
                a_prv = a_mid;
                a_mid = a_nxt;
                u_prv = u_mid;
                u_mid = u_nxt;
            }
        }
    }
    const double sum = block_sum(acc);
    if (threadIdx.x == 0) k.out[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// ---------------------------------------------------------------- coarse solve
// k_gs_relative (mg_solve_kernels.hip) with the operator of the header: ONE workgroup, U and F in LDS (the same dynamic
// request, 2 N^2 doubles), zero start, colour 0 = (row + col) even then colour 1.  N <= 63 and threads = min(1024,
// ceil64(N^2)): a thread owns at most GS_PTS = 4 points, the same ones in every loop, and keeps their four face coefficients,
// d and q in registers from before the first iteration on -- the coefficient and the reaction term are read from memory once.
// OPT_A: Ag may be null (a = 1 through the same expressions); false: Ag is read without a look at it.
constexpr int GS_PTS = 4;
template <bool OPT_A, bool HAS_S>
__device__ __forceinline__ void gs_relative_vc_body(int N, double h2, double inv, double sd, const double *__restrict__ Ag,
                                                    const double *__restrict__ Sg, double *__restrict__ Ug,
                                                    const double *__restrict__ Fg, double atol, double rtol, int max_iters,
                                                    int *__restrict__ state, double *__restrict__ err_out)
{
    extern __shared__ __align__(16) double lds[];
    __shared__ double s_val;
    const int n = N * N;
    double *U = lds, *F = lds + n;
    const double denom = (double)((N - 2) * (N - 2));
    Faces fc[GS_PTS];
    double qc[GS_PTS];
    int colour_of[GS_PTS];   // 0 / 1: an interior point of that colour; -1: rim, or beyond the grid
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < GS_PTS; ++j) {
        const int p = threadIdx.x + j * blockDim.x;
        colour_of[j] = -1;
        fc[j] = Faces{1.0, 1.0, 1.0, 1.0, 4.0};
        qc[j] = 0.25;
        if (p < n) {
            const double f = Fg[p];
            F[p] = f;
            U[p] = 0.0;
            const int r = p / N, c = p - r * N;
            if (!rim(r, c, N)) {
                acc = acc + fabs(f);
                colour_of[j] = (r + c) & 1;
                double sdp = sd;
                if constexpr (HAS_S) sdp = sd + Sg[p] * h2;
                fc[j] = !OPT_A || Ag ? faces(Ag[p], Ag[p + N], Ag[p - N], Ag[p + 1], Ag[p - 1], sdp) : faces(1.0, 1.0, 1.0, 1.0, 1.0, sdp);
                qc[j] = 1.0 / fc[j].d;
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
                    U[p] = qc[j] * ((((fc[j].aW * U[p - 1] + fc[j].aE * U[p + 1]) + fc[j].aN * U[p + N]) + fc[j].aS * U[p - N]) - h2 * F[p]);
            }
            __syncthreads();
        }
        ++iterations;
        acc = 0.0;
#pragma unroll
        for (int j = 0; j < GS_PTS; ++j) {
            const int p = threadIdx.x + j * blockDim.x;
            if (colour_of[j] >= 0) acc = acc + fabs(inv * bracket(fc[j], U[p], U[p + N], U[p - N], U[p + 1], U[p - 1]) - F[p]);
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

// ---------------------------------------------------------------- the coefficient: coarsening and check
// a_c = doRestriction's expression on every coarse point, rim included, with the end entries of the table replaced (index
// 0: (0, 0.0), index M-1: (N-2, 1.0)), clamped into the range of its four samples (include/mg_varcoef.h)
__device__ __forceinline__ void coef_coarsen_body(int N, const double *__restrict__ Af, int M, double *__restrict__ Ac,
                                                  const int *__restrict__ lo, const double *__restrict__ w)
{
    const int cc = blockIdx.x * TB + threadIdx.x;
    const int rc = blockIdx.y;
    if (cc >= M) return;
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
    const double s0 = Af[f], s1 = Af[f + 1], s2 = Af[f + N], s3 = Af[f + N + 1];
    double v = b * d * s0 + a * d * s1 + c * b * s2 + a * c * s3;
    const double mn = fmin(fmin(s0, s1), fmin(s2, s3)), mx = fmax(fmax(s0, s1), fmax(s2, s3));
    v = fmin(fmax(v, mn), mx);
    Ac[(size_t)rc * M + cc] = v;
}

// *flag = 1 when some value is not finite or not > 0 (the flag is zeroed by the caller; every offending lane stores the
// same 1)
__device__ __forceinline__ void coef_check_body(const double *__restrict__ A, size_t n, int *__restrict__ flag)
{
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * TB + threadIdx.x; i < n; i += (size_t)gridDim.x * TB) {
        const double v = A[i];
        if (!(v > 0.0) || !(v < __builtin_huge_val())) bad = true;
    }
    if (bad) *flag = 1;
}

}  // namespace

}  // namespace k
}  // namespace mg

#endif /* MG_VARCOEF_IMPL_H */
