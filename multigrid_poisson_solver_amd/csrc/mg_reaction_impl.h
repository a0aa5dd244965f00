// mg_reaction_impl.h -- the point code of the reaction kernels (include/mg_reaction.h; kernels and launchers:
// mg_reaction_kernels.hip).  The operator, the sweep, the residual and the block sums are mg_varcoef_impl.h's (Faces, faces,
// bracket, point, block_sum, resnorm_finish_vc_body), included, not copied, as mg_bc_impl.h does: what changes is the sd that
// faces() gets, sd + s[p]*dx2 per point instead of the level constant.  The streaming bodies below are vc_cols / vc_pairs /
// resnorm_vc_body with that one more stream -- s is read at the centre row only, so it needs no window -- and with the
// coefficient as a template parameter in every form: HAS_A = false streams no array of ones, a = 1 goes through the same
// expressions (every face exactly 1, d = 4 + sdp).
#ifndef MG_REACTION_IMPL_H
#define MG_REACTION_IMPL_H

#include "mg_varcoef_impl.h"

namespace mg {
namespace k {

namespace {

struct RxArgs {
    VcArgs k;          // dx2 AND inv are set whatever the operation: the centre needs dx2
    const double *S;   // the level's nodal reaction term
};

// the centre's shift term of one point (include/mg_reaction.h): t = s*dx2, sdp = sd + t, each rounded once
__device__ __forceinline__ double rx_sd(const VcArgs &k, double s) { return k.sd + s * k.dx2; }

// ---------------------------------------------------------------- one column per lane (any N)
template <Op OP, bool HAS_A>
__device__ __forceinline__ void rx_cols(const RxArgs &x)
{
    const VcArgs &k = x.k;
    const int N = k.N;
    const int c = blockIdx.x * TB + threadIdx.x;
    if (c >= N) return;
    const int r0 = blockIdx.y * ROWS_PB;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 1 < N ? c + 1 : N - 1;
    const bool col_in = c > 0 && c < N - 1;
    constexpr bool READS_U = OP != OP_SWEEP_ZERO, READS_F = OP != OP_APPLY;
    const double *__restrict__ A = k.A;
    const double *__restrict__ S = x.S;
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
            const Faces f = faces(a_mid, a_nxt, a_prv, a_east, a_west, rx_sd(k, S[p]));
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
// (even N, 16-byte aligned arrays, as vc_pairs).  NT: F and s through non-temporal loads, the output through non-temporal
// stores; the residual is instantiated with NT = true only.
template <Op OP, bool NT, bool HAS_A>
__device__ __forceinline__ void rx_pairs(const RxArgs &x)
{
    const VcArgs &k = x.k;
    const int N = k.N;
    const int c = 2 * (blockIdx.x * TB + threadIdx.x);
    if (c >= N) return;
    const int r0 = blockIdx.y * PR;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 2 < N ? c + 2 : N - 1;
    constexpr bool READS_U = OP != OP_SWEEP_ZERO;
    const double *__restrict__ A = k.A;
    const double *__restrict__ S = x.S;
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
            const double2_v f = load_f<NT>(F + p), s = load_f<NT>(S + p);
            if (c > 0) {
                const Faces fc = faces(a_mid.x, a_nxt.x, a_prv.x, a_mid.y, HAS_A ? A[line + cl] : 1.0, rx_sd(k, s.x));
                v.x = point<OP>(k, fc, f.x, u_mid.x, u_nxt.x, u_prv.x, u_mid.y, READS_U ? U[line + cl] : 0.0);
            }
            if (c + 1 < N - 1) {
                const Faces fc = faces(a_mid.y, a_nxt.y, a_prv.y, HAS_A ? A[line + cr] : 1.0, a_mid.x, rx_sd(k, s.y));
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
// resnorm_vc_body with the per-point centre: the same partition, the same order, nothing but the partials (k.out) written
template <bool PAIR, bool NT, bool HAS_A>
__device__ __forceinline__ void rx_resnorm_body(const RxArgs &x)
{
    const VcArgs &k = x.k;
    const int N = k.N;
    const double inv = k.inv;
    const double *__restrict__ A = k.A;
    const double *__restrict__ S = x.S;
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
                    const double sdp = rx_sd(k, S[p]);
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
                    const double2_v f = load_f<NT>(F + line + c), s = load_f<NT>(S + line + c);
                    if (c > 0) {
                        const Faces fc = faces(a_mid.x, a_nxt.x, a_prv.x, a_mid.y, HAS_A ? A[line + cl] : 1.0, rx_sd(k, s.x));
                        const double d = inv * bracket(fc, u_mid.x, u_nxt.x, u_prv.x, u_mid.y, U[line + cl]) - f.x;
                        acc += d * d;
                    }
                    if (c + 1 < N - 1) {
                        const Faces fc = faces(a_mid.y, a_nxt.y, a_prv.y, HAS_A ? A[line + cr] : 1.0, a_mid.x, rx_sd(k, s.y));
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
// gs_relative_vc_body with the per-point centre: ONE workgroup, U and F in LDS (the same request, 2 N^2 doubles), N <= 63.
// s, like a, is read from global memory once, into the thread's d and q registers before the first iteration; Ag == nullptr:
// a = 1 through the same expressions.
__device__ __forceinline__ void rx_gs_relative_body(int N, double h2, double inv, double sd, const double *__restrict__ Ag,
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
                const double sdp = sd + Sg[p] * h2;
                fc[j] = Ag ? faces(Ag[p], Ag[p + N], Ag[p - N], Ag[p + 1], Ag[p - 1], sdp) : faces(1.0, 1.0, 1.0, 1.0, 1.0, sdp);
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

// *flag = 1 when some value is not finite or not >= 0 (the flag is zeroed by the caller; every offending lane stores the
// same 1)
__device__ __forceinline__ void rx_check_body(const double *__restrict__ S, size_t n, int *__restrict__ flag)
{
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * TB + threadIdx.x; i < n; i += (size_t)gridDim.x * TB) {
        const double v = S[i];
        if (!(v >= 0.0) || !(v < __builtin_huge_val())) bad = true;
    }
    if (bad) *flag = 1;
}

}  // namespace

}  // namespace k
}  // namespace mg

#endif /* MG_REACTION_IMPL_H */
