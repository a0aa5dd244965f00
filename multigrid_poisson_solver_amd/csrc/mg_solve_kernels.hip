// mg_solve_kernels.hip -- fp64 kernels of the residual-tolerance solver (mg_solve.cpp): the weighted Jacobi sweep, the
// red-black Gauss-Seidel coarse solve with a target relative to its own start residual, and the residual L2 norm.
// Built with -ffp-contract=off like every kernel file: the weighted update U + c*t rounds the product and the sum
// separately, and every bracket keeps the reference's association order (src/MG_solver_CPU.cpp:590, :1020, :560).
// The sweeps here are the operator-by-operator form (MG_SMOOTHER=simple); the default cycle runs the weighted
// instantiations of the streaming smoother (mg_stream_impl.h, WT).
// The batched solver (mg_solve_batch.cpp) runs the norm, the coarse solve and the transfer operators of its non-fusable
// levels on all active instances in one launch each: the `_b` kernels below take every instance's arrays from a
// NodeBatchItem table in device memory and run, per instance, the same code as their single-instance forms.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_solver_common.h"

namespace mg {
namespace k {

namespace {

// (the block shape, wave_sum / block_sum, rim, the norm's finish and the grids: mg_solver_common.h)

// 5-point bracket in the reference's order: row+1, row-1, col+1, col-1, then -4*centre (src/MG_solver_CPU.cpp:590)
__device__ __forceinline__ double star_minus4(const double *__restrict__ A, size_t p, int N)
{
    return A[p + N] + A[p - N] + A[p + 1] + A[p - 1] - 4 * A[p];
}

// The screened operator (mg_solve_opts.shift != 0): the centre coefficient is d = 4 + shift*dx^2 instead of 4.  The
// product d*U is rounded, then subtracted (-ffp-contract=off), in the same place of the same sum.  Every kernel below is
// a shared __forceinline__ body with a template parameter SH: SH = false is the expression as it always was (d is not
// looked at), SH = true lives in kernels of their own (`_sh`), so that an unshifted solve launches what it always launched.
template <bool SH>
__device__ __forceinline__ double centre(double u, double d)
{
    if constexpr (SH) return d * u;
    else return 4 * u;
}
template <bool SH>
__device__ __forceinline__ double star_minus(const double *__restrict__ A, size_t p, int N, double d)
{
    if constexpr (SH) return A[p + N] + A[p - N] + A[p + 1] + A[p - 1] - d * A[p];
    else return star_minus4(A, p, N);
}

template <bool NT>
__device__ __forceinline__ double2_v load_f(const double *p)
{
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const double2_v *>(p));
    return *reinterpret_cast<const double2_v *>(p);
}

// ---------------------------------------------------------------- weighted Jacobi, one sweep
// U = U_old + c*t, t = star(U_old) - 4 U_old - dx^2 F, c = 0.25*omega (formed on the host).  At omega = 1 the product
// with 0.25 is exact and this is doSmoothing's sweep bit for bit.  Rim points keep their value.
template <bool ZERO_IN, bool SH>
__device__ __forceinline__ void wjacobi_body(int N, double dx2, double cw, double d, const double *__restrict__ in,
                                             const double *__restrict__ F, double *__restrict__ out)
{
    const int c = blockIdx.x * TB + threadIdx.x;
    if (c >= N) return;
    const int r0 = blockIdx.y * ROWS_PB;
#pragma unroll
    for (int k = 0; k < ROWS_PB; ++k) {
        const int r = r0 + k;
        if (r >= N) return;
        const size_t p = (size_t)r * N + c;
        double v;
        if (ZERO_IN) {
            // the bracket of an all-zero field: (0+0+0+0 - 4*0) - dx^2 F = 0 - dx^2 F
            v = rim(r, c, N) ? 0.0 : 0.0 + cw * (0.0 - dx2 * F[p]);
        } else {
            v = in[p];
            if (!rim(r, c, N)) v = v + cw * (star_minus<SH>(in, p, N, d) - dx2 * F[p]);
        }
        out[p] = v;
    }
}

template <bool ZERO_IN>
__global__ __launch_bounds__(TB) void k_wjacobi(int N, double dx2, double cw, const double *__restrict__ in,
                                                const double *__restrict__ F, double *__restrict__ out)
{
    wjacobi_body<ZERO_IN, false>(N, dx2, cw, 4.0, in, F, out);
}

template <bool ZERO_IN>
__global__ __launch_bounds__(TB) void k_wjacobi_sh(int N, double dx2, double cw, double d, const double *__restrict__ in,
                                                   const double *__restrict__ F, double *__restrict__ out)
{
    wjacobi_body<ZERO_IN, true>(N, dx2, cw, d, in, F, out);
}

// the same sweep on even N >= PAIR_MIN_N with 16 B per lane and PR rows per thread (the shape of k_jacobi_pair_rows):
// every row of `in` is read once, its outer neighbours are single doubles (L1 hits of the neighbouring lanes' pairs)
template <bool NT, bool SH>
__device__ __forceinline__ void wjacobi_pairs_body(int N, double dx2, double cw, double d, const double *__restrict__ in,
                                                   const double *__restrict__ F, double *__restrict__ out)
{
    const int c = 2 * (blockIdx.x * TB + threadIdx.x);
    const int r0 = blockIdx.y * PR;
    if (c >= N) return;
    auto row_pair = [&](int r) {
        r = r < 0 ? 0 : (r < N ? r : N - 1);   // (rows beyond the grid: clamped, never used)
        return *reinterpret_cast<const double2_v *>(in + (size_t)r * N + c);
    };
    double2_v dn = row_pair(r0 - 1), ctr = row_pair(r0);
#pragma unroll
    for (int k = 0; k < PR; ++k) {
        const int r = r0 + k;
        if (r >= N) break;
        const double2_v up = row_pair(r + 1);
        const size_t p = (size_t)r * N + c;
        double2_v o = ctr;
        if (r > 0 && r < N - 1) {
            const double2_v f = load_f<NT>(F + p);
            if (c > 0) {
                const double w = in[p - 1];
                o.x = ctr.x + cw * (up.x + dn.x + ctr.y + w - centre<SH>(ctr.x, d) - dx2 * f.x);
            }
            if (c + 1 < N - 1) {
                const double e = in[p + 2];
                o.y = ctr.y + cw * (up.y + dn.y + e + ctr.x - centre<SH>(ctr.y, d) - dx2 * f.y);
            }
        }
        if (NT) __builtin_nontemporal_store(o, reinterpret_cast<double2_v *>(out + p));
        else *reinterpret_cast<double2_v *>(out + p) = o;
        dn = ctr;
        ctr = up;
    }
}

template <bool NT>
__global__ __launch_bounds__(TB) void k_wjacobi_pairs(int N, double dx2, double cw, const double *__restrict__ in,
                                                      const double *__restrict__ F, double *__restrict__ out)
{
    wjacobi_pairs_body<NT, false>(N, dx2, cw, 4.0, in, F, out);
}

template <bool NT>
__global__ __launch_bounds__(TB) void k_wjacobi_pairs_sh(int N, double dx2, double cw, double d, const double *__restrict__ in,
                                                         const double *__restrict__ F, double *__restrict__ out)
{
    wjacobi_pairs_body<NT, true>(N, dx2, cw, d, in, F, out);
}

// ---------------------------------------------------------------- residual L2 norm
// per-block partial sums of d^2 over interior points, d = inv*(star - 4U) - F (getResidual's value, :560);
// HAS_U = false: U == 0, d = -F (the reference norm ||F||).  Nothing but the partials is written.
// (the bodies are shared with the batched forms: the same partition into partials for every instance)
template <bool HAS_U, bool SH = false>
__device__ __forceinline__ void resnorm_body(int N, double inv, const double *__restrict__ U, const double *__restrict__ F,
                                             double *__restrict__ part, double dc = 4.0)
{
    const int c = blockIdx.x * TB + threadIdx.x;
    const int r0 = blockIdx.y * ROWS_PB;
    double acc = 0.0;
    if (c < N) {
#pragma unroll
        for (int k = 0; k < ROWS_PB; ++k) {
            const int r = r0 + k;
            if (r < N && !rim(r, c, N)) {
                const size_t p = (size_t)r * N + c;
                const double d = HAS_U ? inv * star_minus<SH>(U, p, N, dc) - F[p] : F[p];
                acc += d * d;
            }
        }
    }
    const double s = block_sum(acc);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

template <bool HAS_U>
__global__ __launch_bounds__(TB) void k_resnorm(int N, double inv, const double *__restrict__ U,
                                                const double *__restrict__ F, double *__restrict__ part)
{
    resnorm_body<HAS_U>(N, inv, U, F, part);
}

// even N >= PAIR_MIN_N: 16 B per lane, PR rows per thread with a rolling window of three row pairs (every row of U read
// once), F through 16-byte (non-temporal from NT_MIN_N on) loads -- 16 B of HBM traffic per point
template <bool HAS_U, bool NT, bool SH = false>
__device__ __forceinline__ void resnorm_pairs_body(int N, double inv, const double *__restrict__ U,
                                                   const double *__restrict__ F, double *__restrict__ part, double dc = 4.0)
{
    const int c = 2 * (blockIdx.x * TB + threadIdx.x);
    const int r0 = blockIdx.y * PR;
    double acc = 0.0;
    if (c < N) {
        const int cl = c > 0 ? c - 1 : 0, cr = c + 2 < N ? c + 2 : N - 1;
        auto row_pair = [&](int r) {
            r = r < 0 ? 0 : (r < N ? r : N - 1);
            return *reinterpret_cast<const double2_v *>(U + (size_t)r * N + c);
        };
        double2_v up = {0.0, 0.0}, mid = {0.0, 0.0};
        if (HAS_U) {
            up = row_pair(r0 - 1);
            mid = row_pair(r0);
        }
#pragma unroll
        for (int k = 0; k < PR; ++k) {
            const int r = r0 + k;
            if (r >= N) break;
            double2_v down = {0.0, 0.0};
            if (HAS_U) down = row_pair(r + 1);
            if (r > 0 && r < N - 1) {
                const size_t p = (size_t)r * N + c;
                const double2_v f = load_f<NT>(F + p);
                double2_v d = f;
                if (HAS_U) {
                    const double left = U[(size_t)r * N + cl], right = U[(size_t)r * N + cr];
                    d.x = inv * (down.x + up.x + mid.y + left - centre<SH>(mid.x, dc)) - f.x;
                    d.y = inv * (down.y + up.y + right + mid.x - centre<SH>(mid.y, dc)) - f.y;
                }
                if (c > 0) acc += d.x * d.x;
                if (c + 1 < N - 1) acc += d.y * d.y;
            }
            up = mid;
            mid = down;
        }
    }
    const double s = block_sum(acc);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

template <bool HAS_U, bool NT>
__global__ __launch_bounds__(TB) void k_resnorm_pairs(int N, double inv, const double *__restrict__ U,
                                                      const double *__restrict__ F, double *__restrict__ part)
{
    resnorm_pairs_body<HAS_U, NT>(N, inv, U, F, part);
}

// the screened operator's norm (U given: the reference norm ||F|| has no operator in it)
__global__ __launch_bounds__(TB) void k_resnorm_sh(int N, double inv, double dc, const double *__restrict__ U,
                                                   const double *__restrict__ F, double *__restrict__ part)
{
    resnorm_body<true, true>(N, inv, U, F, part, dc);
}

template <bool NT>
__global__ __launch_bounds__(TB) void k_resnorm_pairs_sh(int N, double inv, double dc, const double *__restrict__ U,
                                                         const double *__restrict__ F, double *__restrict__ part)
{
    resnorm_pairs_body<true, NT, true>(N, inv, U, F, part, dc);
}

__global__ __launch_bounds__(1024) void k_resnorm_finish(const double *__restrict__ part, size_t n, double *__restrict__ out)
{
    resnorm_finish_body(part, n, out);
}

// batched forms: instance z = blockIdx.z (blockIdx.x for the finish) of items[] (in = U, F), its n partials at part + z*n
template <bool HAS_U>
__global__ __launch_bounds__(TB) void k_resnorm_b(int N, double inv, const NodeBatchItem *__restrict__ items,
                                                  double *__restrict__ part, size_t n)
{
    const NodeBatchItem &it = items[blockIdx.z];
    resnorm_body<HAS_U>(N, inv, static_cast<const double *>(it.in), static_cast<const double *>(it.F), part + blockIdx.z * n);
}

template <bool HAS_U, bool NT>
__global__ __launch_bounds__(TB) void k_resnorm_pairs_b(int N, double inv, const NodeBatchItem *__restrict__ items,
                                                        double *__restrict__ part, size_t n)
{
    const NodeBatchItem &it = items[blockIdx.z];
    resnorm_pairs_body<HAS_U, NT>(N, inv, static_cast<const double *>(it.in), static_cast<const double *>(it.F),
                                  part + blockIdx.z * n);
}

__global__ __launch_bounds__(TB) void k_resnorm_sh_b(int N, double inv, double dc, const NodeBatchItem *__restrict__ items,
                                                     double *__restrict__ part, size_t n)
{
    const NodeBatchItem &it = items[blockIdx.z];
    resnorm_body<true, true>(N, inv, static_cast<const double *>(it.in), static_cast<const double *>(it.F), part + blockIdx.z * n, dc);
}

template <bool NT>
__global__ __launch_bounds__(TB) void k_resnorm_pairs_sh_b(int N, double inv, double dc, const NodeBatchItem *__restrict__ items,
                                                           double *__restrict__ part, size_t n)
{
    const NodeBatchItem &it = items[blockIdx.z];
    resnorm_pairs_body<true, NT, true>(N, inv, static_cast<const double *>(it.in), static_cast<const double *>(it.F),
                                       part + blockIdx.z * n, dc);
}

// out[i] = sqrt(sum of instance i's n partials): one block per instance, each the single-instance finish
__global__ __launch_bounds__(1024) void k_resnorm_finish_b(const double *__restrict__ part, size_t n, double *__restrict__ out)
{
    resnorm_finish_body(part + blockIdx.x * n, n, out + blockIdx.x);
}

// ---------------------------------------------------------------- coarse solve
// red-black Gauss-Seidel of src/MG_solver_CPU.cpp:952-1066 in ONE workgroup (U and F in LDS): zero start (:993),
// colour 0 = (row+col) even then colour 1, update :1020/:1043, err :1051-1059 = sum|residual| / (N-2)^2.  The target
// is max(atol, rtol*err0) with err0 the same metric at U = 0 (sum|F| / (N-2)^2), evaluated here from F before the
// first iteration; at least one iteration, at most max_iters.  state[1] = iterations, state[2] = 1 when the cap ended
// the solve above the target, state[3] = bits of nothing (kept zero).  *err_out (when given) = err0, final err.
// SH: update q*(...) with q = 1/d, the error metric's centre term d*U (the unshifted form: 0.25 and 4)
template <bool SH = false>
__device__ __forceinline__ void gs_relative_body(int N, double h2, double inv, double *__restrict__ Ug,
                                                 const double *__restrict__ Fg, double atol, double rtol, int max_iters,
                                                 int *__restrict__ state, double *__restrict__ err_out, double dc = 4.0,
                                                 double qc = 0.25)
{
    extern __shared__ __align__(16) double lds[];
    __shared__ double s_val;
    const int n = N * N;
    double *U = lds, *F = lds + n;
    const double denom = (double)((N - 2) * (N - 2));
    double acc = 0.0;
    for (int p = threadIdx.x; p < n; p += blockDim.x) {
        const double f = Fg[p];
        F[p] = f;
        U[p] = 0.0;
        const int r = p / N, c = p - r * N;
        if (!rim(r, c, N)) acc = acc + fabs(f);
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
            for (int p = threadIdx.x; p < n; p += blockDim.x) {
                const int r = p / N, c = p - r * N;
                if (!rim(r, c, N) && ((r + c) & 1) == colour)
                    U[p] = (SH ? qc : 0.25) * (U[p - 1] + U[p + 1] + U[p + N] + U[p - N] - h2 * F[p]);
            }
            __syncthreads();
        }
        ++iterations;
        acc = 0.0;
        for (int p = threadIdx.x; p < n; p += blockDim.x) {
            const int r = p / N, c = p - r * N;
            if (!rim(r, c, N))
                acc = acc + fabs(inv * (U[p + N] + U[p - N] + U[p + 1] + U[p - 1] - centre<SH>(U[p], dc)) - F[p]);
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

__global__ __launch_bounds__(1024) void k_gs_relative(int N, double h2, double inv, double *__restrict__ Ug,
                                                      const double *__restrict__ Fg, double atol, double rtol,
                                                      int max_iters, int *__restrict__ state, double *__restrict__ err_out)
{
    gs_relative_body(N, h2, inv, Ug, Fg, atol, rtol, max_iters, state, err_out);
}

// one workgroup per instance (items[i]: out = U, F): its own err0, its own stop, its state at state + 4i
__global__ __launch_bounds__(1024) void k_gs_relative_b(int N, double h2, double inv, const NodeBatchItem *__restrict__ items,
                                                        double atol, double rtol, int max_iters, int *__restrict__ state)
{
    const NodeBatchItem &it = items[blockIdx.x];
    gs_relative_body(N, h2, inv, static_cast<double *>(it.out), static_cast<const double *>(it.F), atol, rtol, max_iters,
                     state + 4 * blockIdx.x, nullptr);
}

__global__ __launch_bounds__(1024) void k_gs_relative_sh(int N, double h2, double inv, double dc, double qc, double *__restrict__ Ug,
                                                         const double *__restrict__ Fg, double atol, double rtol,
                                                         int max_iters, int *__restrict__ state, double *__restrict__ err_out)
{
    gs_relative_body<true>(N, h2, inv, Ug, Fg, atol, rtol, max_iters, state, err_out, dc, qc);
}

__global__ __launch_bounds__(1024) void k_gs_relative_sh_b(int N, double h2, double inv, double dc, double qc,
                                                           const NodeBatchItem *__restrict__ items, double atol, double rtol,
                                                           int max_iters, int *__restrict__ state)
{
    const NodeBatchItem &it = items[blockIdx.x];
    gs_relative_body<true>(N, h2, inv, static_cast<double *>(it.out), static_cast<const double *>(it.F), atol, rtol, max_iters,
                           state + 4 * blockIdx.x, nullptr, dc, qc);
}

// ---------------------------------------------------------------- transfer operators of the non-fusable levels, batched
// The expressions of k_residual, k_restrict<double> and k_prolong<true, double> (mg_kernels.hip), one point per lane;
// instance blockIdx.z of items[].  residual: in = U, F, out = D.
template <bool SH>
__device__ __forceinline__ void residual_b_body(int N, double inv, const NodeBatchItem *__restrict__ items, int sign, double dc)
{
    const NodeBatchItem &it = items[blockIdx.z];
    const double *__restrict__ U = static_cast<const double *>(it.in);
    const double *__restrict__ F = static_cast<const double *>(it.F);
    double *__restrict__ D = static_cast<double *>(it.out);
    const int c = blockIdx.x * TB + threadIdx.x;
    if (c >= N) return;
    const int r0 = blockIdx.y * ROWS_PB;
#pragma unroll
    for (int k = 0; k < ROWS_PB; ++k) {
        const int r = r0 + k;
        if (r >= N) return;
        const size_t p = (size_t)r * N + c;
        double v = 0.0;
        if (!rim(r, c, N)) v = inv * star_minus<SH>(U, p, N, dc) - F[p];
        D[p] = sign < 0 ? -v : v;
    }
}

__global__ __launch_bounds__(TB) void k_residual_b(int N, double inv, const NodeBatchItem *__restrict__ items, int sign)
{
    residual_b_body<false>(N, inv, items, sign, 4.0);
}

__global__ __launch_bounds__(TB) void k_residual_sh_b(int N, double inv, double dc, const NodeBatchItem *__restrict__ items, int sign)
{
    residual_b_body<true>(N, inv, items, sign, dc);
}

// restriction N -> M (doRestriction, :656-678): in = fine field, out = coarse field
__global__ __launch_bounds__(TB) void k_restrict_b(int N, int M, const NodeBatchItem *__restrict__ items,
                                                   const int *__restrict__ lo, const double *__restrict__ w, int sign)
{
    const NodeBatchItem &it = items[blockIdx.z];
    const double *__restrict__ Uf = static_cast<const double *>(it.in);
    double *__restrict__ Uc = static_cast<double *>(it.out);
    const int cc = blockIdx.x * TB + threadIdx.x;
    const int rc = blockIdx.y;
    if (cc >= M) return;
    double v = 0.0;
    if (!rim(rc, cc, M)) {
        const double a = w[cc], b = 1.0 - a;
        const double c = w[rc], d = 1.0 - c;
        const size_t f = (size_t)lo[cc] + (size_t)lo[rc] * N;
        v = b * d * Uf[f] + a * d * Uf[f + 1] + c * b * Uf[f + N] + a * c * Uf[f + N + 1];
        if (sign < 0) v = -v;
    }
    Uc[(size_t)rc * M + cc] = v;
}

// out = in + doProlongation(coarse) (:354 + :368), coarse N -> fine M: coarse, in, out
__global__ __launch_bounds__(TB) void k_prolong_add_b(int N, int M, const NodeBatchItem *__restrict__ items,
                                                      const int *__restrict__ orow, const int *__restrict__ ocol,
                                                      const double *__restrict__ row_hi, const double *__restrict__ row_lo,
                                                      const double *__restrict__ col_hi, const double *__restrict__ col_lo,
                                                      double c_dx)
{
    const NodeBatchItem &it = items[blockIdx.z];
    const double *__restrict__ Uc = static_cast<const double *>(it.coarse);
    const double *__restrict__ Uf_in = static_cast<const double *>(it.in);
    double *__restrict__ Uf_out = static_cast<double *>(it.out);
    const int l = blockIdx.x * TB + threadIdx.x;
    const int kf = blockIdx.y;
    if (l >= M) return;
    const int i = orow[kf], j = ocol[l];
    const size_t q = (size_t)kf * M + l;
    if (i < 0 || j < 0) {  // no coarse cell writes this point (never for M >= N)
        Uf_out[q] = Uf_in[q];
        return;
    }
    const size_t p = (size_t)i * N + j;
    const double c1 = Uc[p], c2 = Uc[p + 1], c3 = Uc[p + N], c4 = Uc[p + N + 1];
    const double xh = col_hi[l], xl = col_lo[l], yh = row_hi[kf], yl = row_lo[kf];
    const double v = ((c1 * xh + c2 * xl) * yh + (c3 * xh + c4 * xl) * yl) / c_dx / c_dx;
    Uf_out[q] = Uf_in[q] + v;   // doGridAddition :569: U1 = U1 + U2
}

// out = in, n doubles per instance (blockIdx.y)
__global__ __launch_bounds__(TB) void k_copy_b(size_t n, const NodeBatchItem *__restrict__ items)
{
    const NodeBatchItem &it = items[blockIdx.y];
    const double *__restrict__ src = static_cast<const double *>(it.in);
    double *__restrict__ dst = static_cast<double *>(it.out);
    for (size_t i = (size_t)blockIdx.x * TB + threadIdx.x; i < n; i += (size_t)gridDim.x * TB) dst[i] = src[i];
}

}  // namespace

// ------------------------------------------------------------------ launchers
void wjacobi(hipStream_t s, int N, double dx2, double cw, const double *in, const double *F, double *out, const Shifted &sh)
{
    if (sh.on) {   // the same choice of form, the screened bracket
        const double d = sh.d;
        if (!in) hipLaunchKernelGGL(k_wjacobi_sh<true>, grid_rows(N), dim3(TB), 0, s, N, dx2, cw, d, in, F, out);
        else if (use_pairs(N) && N >= NT_MIN_N) hipLaunchKernelGGL(k_wjacobi_pairs_sh<true>, grid_pairs(N), dim3(TB), 0, s, N, dx2, cw, d, in, F, out);
        else if (use_pairs(N)) hipLaunchKernelGGL(k_wjacobi_pairs_sh<false>, grid_pairs(N), dim3(TB), 0, s, N, dx2, cw, d, in, F, out);
        else hipLaunchKernelGGL(k_wjacobi_sh<false>, grid_rows(N), dim3(TB), 0, s, N, dx2, cw, d, in, F, out);
        return;
    }
    if (!in) {
        hipLaunchKernelGGL(k_wjacobi<true>, grid_rows(N), dim3(TB), 0, s, N, dx2, cw, in, F, out);
        return;
    }
    if (use_pairs(N)) {
        if (N >= NT_MIN_N) hipLaunchKernelGGL(k_wjacobi_pairs<true>, grid_pairs(N), dim3(TB), 0, s, N, dx2, cw, in, F, out);
        else hipLaunchKernelGGL(k_wjacobi_pairs<false>, grid_pairs(N), dim3(TB), 0, s, N, dx2, cw, in, F, out);
        return;
    }
    hipLaunchKernelGGL(k_wjacobi<false>, grid_rows(N), dim3(TB), 0, s, N, dx2, cw, in, F, out);
}

size_t resnorm_partials(int N)
{
    const dim3 g = use_pairs(N) ? grid_pairs(N) : grid_rows(N);
    return (size_t)g.x * g.y;
}

void resnorm(hipStream_t s, int N, double inv, const double *U, const double *F, double *part, double *out, const Shifted &sh)
{
    const size_t np = resnorm_partials(N);
    if (sh.on && U) {
        if (use_pairs(N)) {
            if (N >= NT_MIN_N) hipLaunchKernelGGL(k_resnorm_pairs_sh<true>, grid_pairs(N), dim3(TB), 0, s, N, inv, sh.d, U, F, part);
            else hipLaunchKernelGGL(k_resnorm_pairs_sh<false>, grid_pairs(N), dim3(TB), 0, s, N, inv, sh.d, U, F, part);
        } else {
            hipLaunchKernelGGL(k_resnorm_sh, grid_rows(N), dim3(TB), 0, s, N, inv, sh.d, U, F, part);
        }
    } else if (use_pairs(N)) {
        const dim3 g = grid_pairs(N);
        const bool nt = N >= NT_MIN_N;
        if (U) {
            if (nt) hipLaunchKernelGGL((k_resnorm_pairs<true, true>), g, dim3(TB), 0, s, N, inv, U, F, part);
            else hipLaunchKernelGGL((k_resnorm_pairs<true, false>), g, dim3(TB), 0, s, N, inv, U, F, part);
        } else {
            if (nt) hipLaunchKernelGGL((k_resnorm_pairs<false, true>), g, dim3(TB), 0, s, N, inv, U, F, part);
            else hipLaunchKernelGGL((k_resnorm_pairs<false, false>), g, dim3(TB), 0, s, N, inv, U, F, part);
        }
    } else {
        if (U) hipLaunchKernelGGL(k_resnorm<true>, grid_rows(N), dim3(TB), 0, s, N, inv, U, F, part);
        else hipLaunchKernelGGL(k_resnorm<false>, grid_rows(N), dim3(TB), 0, s, N, inv, U, F, part);
    }
    hipLaunchKernelGGL(k_resnorm_finish, dim3(1), dim3(1024), 0, s, part, np, out);
}

bool gs_relative_fits(int N) { return N >= 3 && N < GS_RELATIVE_MAX_N; }

void gauss_seidel_relative(hipStream_t s, int N, double h2, double inv, double *U, const double *F, double atol,
                           double rtol, int max_iters, int *state, double *err_out, const Shifted &sh)
{
    const size_t n = (size_t)N * N;
    const size_t lds = 2 * n * sizeof(double);
    int threads = (int)((n + 63) / 64 * 64);
    if (threads > 1024) threads = 1024;
    // (N <= 63: at most 63 KiB of U and F, inside the default 64 KiB of dynamic LDS)
    if (sh.on) {
        hipLaunchKernelGGL(k_gs_relative_sh, dim3(1), dim3(threads), lds, s, N, h2, inv, sh.d, sh.q, U, F, atol, rtol, max_iters, state,
                           err_out);
        return;
    }
    hipLaunchKernelGGL(k_gs_relative, dim3(1), dim3(threads), lds, s, N, h2, inv, U, F, atol, rtol, max_iters, state, err_out);
}

// ------------------------------------------------------------------ batched launchers (mg_solve_batch.cpp)
void resnorm_batch(hipStream_t s, int n, int N, double inv, bool has_u, const NodeBatchItem *items, double *part, double *out,
                   const Shifted &sh)
{
    const size_t np = resnorm_partials(N);
    if (sh.on && has_u) {
        dim3 g = use_pairs(N) ? grid_pairs(N) : grid_rows(N);
        g.z = n;
        if (!use_pairs(N)) hipLaunchKernelGGL(k_resnorm_sh_b, g, dim3(TB), 0, s, N, inv, sh.d, items, part, np);
        else if (N >= NT_MIN_N) hipLaunchKernelGGL(k_resnorm_pairs_sh_b<true>, g, dim3(TB), 0, s, N, inv, sh.d, items, part, np);
        else hipLaunchKernelGGL(k_resnorm_pairs_sh_b<false>, g, dim3(TB), 0, s, N, inv, sh.d, items, part, np);
    } else if (use_pairs(N)) {
        dim3 g = grid_pairs(N);
        g.z = n;
        const bool nt = N >= NT_MIN_N;
        if (has_u) {
            if (nt) hipLaunchKernelGGL((k_resnorm_pairs_b<true, true>), g, dim3(TB), 0, s, N, inv, items, part, np);
            else hipLaunchKernelGGL((k_resnorm_pairs_b<true, false>), g, dim3(TB), 0, s, N, inv, items, part, np);
        } else {
            if (nt) hipLaunchKernelGGL((k_resnorm_pairs_b<false, true>), g, dim3(TB), 0, s, N, inv, items, part, np);
            else hipLaunchKernelGGL((k_resnorm_pairs_b<false, false>), g, dim3(TB), 0, s, N, inv, items, part, np);
        }
    } else {
        dim3 g = grid_rows(N);
        g.z = n;
        if (has_u) hipLaunchKernelGGL(k_resnorm_b<true>, g, dim3(TB), 0, s, N, inv, items, part, np);
        else hipLaunchKernelGGL(k_resnorm_b<false>, g, dim3(TB), 0, s, N, inv, items, part, np);
    }
    hipLaunchKernelGGL(k_resnorm_finish_b, dim3(n), dim3(1024), 0, s, part, np, out);
}

void gauss_seidel_relative_batch(hipStream_t s, int n, int N, double h2, double inv, const NodeBatchItem *items, double atol,
                                 double rtol, int max_iters, int *state, const Shifted &sh)
{
    const size_t cells = (size_t)N * N;
    int threads = (int)((cells + 63) / 64 * 64);
    if (threads > 1024) threads = 1024;
    if (sh.on) {
        hipLaunchKernelGGL(k_gs_relative_sh_b, dim3(n), dim3(threads), 2 * cells * sizeof(double), s, N, h2, inv, sh.d, sh.q, items,
                           atol, rtol, max_iters, state);
        return;
    }
    hipLaunchKernelGGL(k_gs_relative_b, dim3(n), dim3(threads), 2 * cells * sizeof(double), s, N, h2, inv, items, atol, rtol,
                       max_iters, state);
}

void residual_batch(hipStream_t s, int n, int N, double inv, const NodeBatchItem *items, int sign, const Shifted &sh)
{
    dim3 g = grid_rows(N);
    g.z = n;
    if (sh.on) {
        hipLaunchKernelGGL(k_residual_sh_b, g, dim3(TB), 0, s, N, inv, sh.d, items, sign);
        return;
    }
    hipLaunchKernelGGL(k_residual_b, g, dim3(TB), 0, s, N, inv, items, sign);
}

void restrict_batch(hipStream_t s, int n, int N, int M, const NodeBatchItem *items, const RestrictTable &t, int sign)
{
    hipLaunchKernelGGL(k_restrict_b, dim3((M + TB - 1) / TB, M, n), dim3(TB), 0, s, N, M, items, t.lo, t.w, sign);
}

void prolong_add_batch(hipStream_t s, int n, int N, int M, const NodeBatchItem *items, const ProlongTable &t)
{
    hipLaunchKernelGGL(k_prolong_add_b, dim3((M + TB - 1) / TB, M, n), dim3(TB), 0, s, N, M, items, t.owner_row, t.owner_col,
                       t.row_hi, t.row_lo, t.col_hi, t.col_lo, t.c_dx);
}

void copy_batch(hipStream_t s, int n, size_t count, const NodeBatchItem *items)
{
    size_t blocks = (count + TB - 1) / TB;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_copy_b, dim3((unsigned)blocks, n), dim3(TB), 0, s, count, items);
}

}  // namespace k
}  // namespace mg
