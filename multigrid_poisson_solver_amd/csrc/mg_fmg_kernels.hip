// mg_fmg_kernels.hip -- kernels of the full-multigrid start of the residual-tolerance solver (mg_solve.cpp: fmg_start;
// include/mg_hip.h, mg_solve_opts.fmg): the bicubic prolongation of a coarse solution into the interior of the next finer
// level, and the small rim kernels (the Dirichlet data of every level as four edges).
// Built with -ffp-contract=off like every kernel file: the header fixes the evaluation order of the interpolation
// (products and sums rounded one by one) so that numpy restates it bit for bit.
#include <hip/hip_runtime.h>

#include "mg_internal.h"

namespace mg {
namespace k {

namespace {

constexpr int TB = 256;          // threads per block
constexpr int PC_ROWS = 32;      // fine rows per block of the prolongation
constexpr int PC_SRC_ROWS = 20;  // source rows a block may need: the bases of 32 fine rows span <= 16, plus the 4 nodes
constexpr int PC_SRC_COLS = 264; // source columns: the bases of 512 fine columns span <= 256, plus 4 nodes, plus alignment
constexpr int PAIR_MIN_N = 512;  // even N from here on: two columns per lane, 16-byte accesses
constexpr int NT_MIN_N = 4096;   // the fine array is far larger than the caches: non-temporal stores
typedef double double2_s __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------- bicubic prolongation
// Fine point (r, c) = sum over the m x m source nodes at (base[r] + k, base[c] + j) with the weights w[r][k] * w[c][j],
// evaluated as the header says: first along the columns of each source row, v_k = ((w_c0 s_k0 + w_c1 s_k1) + w_c2 s_k2) +
// w_c3 s_k3, then out = ((w_r0 v_0 + w_r1 v_1) + w_r2 v_2) + w_r3 v_3 (m = 3, a 3-point source: the last term is left out).
// A block owns PC_ROWS fine rows by TB (PAIR: 2*TB) fine columns.  It copies the source window of its tile to LDS once
// (every source value is read from memory once per block, 16-byte loads where the source rows are 16-byte aligned); each
// lane then walks down its column(s) with the horizontally interpolated values of the m current source rows in
// registers: a new source row is interpolated once, when the walk reaches it, and serves every fine row that uses it.
// Only interior points are stored (PAIR: one 16-byte store per lane and row, 8 bytes next to the rim).
template <bool PAIR, bool NT>
__device__ __forceinline__ void prolong_cubic_body(int Ns, int Nd, const int *__restrict__ base, const double *__restrict__ w,
                                                   const double *__restrict__ Uc, double *__restrict__ Uf)
{
    __shared__ __align__(16) double tile[PC_SRC_ROWS * PC_SRC_COLS];
    constexpr int CPT = PAIR ? 2 : 1;
    constexpr int W = TB * CPT;
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * W, r0 = blockIdx.y * PC_ROWS;   // (the grid keeps both below Nd)
    const int m = Ns < 4 ? Ns : 4;
    const int c_last = c0 + W - 1 < Nd - 1 ? c0 + W - 1 : Nd - 1;
    const int r_last = r0 + PC_ROWS - 1 < Nd - 1 ? r0 + PC_ROWS - 1 : Nd - 1;
    const bool vec = PAIR && Ns % 2 == 0;
    int cb0 = base[c0];
    if (vec) cb0 &= ~1;
    const int rb0 = base[r0];
    const int nc = base[c_last] + m - cb0, nr = base[r_last] + m - rb0;   // <= PC_SRC_COLS, PC_SRC_ROWS: cubic_table_fits()
    if (vec) {
        // cb0 and Ns even: every pair is 16-byte aligned and inside its row (an odd nc ends before the last column)
        const int nc2 = (nc + 1) >> 1;
        for (int i = tid; i < nr * nc2; i += TB) {
            const int k = i / nc2, j = i - k * nc2;
            const double2_s v = *reinterpret_cast<const double2_s *>(Uc + (size_t)(rb0 + k) * Ns + cb0 + 2 * j);
            *reinterpret_cast<double2_s *>(tile + k * PC_SRC_COLS + 2 * j) = v;
        }
    } else {
        for (int i = tid; i < nr * nc; i += TB) {
            const int k = i / nc, j = i - k * nc;
            tile[k * PC_SRC_COLS + j] = Uc[(size_t)(rb0 + k) * Ns + cb0 + j];
        }
    }
    __syncthreads();
    const int c = c0 + tid * CPT;
    if (c >= Nd) return;
    int bc[CPT];
    double wc[CPT][4];
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
        const int cq = c + q;   // (PAIR: Nd is even, c + 1 is a column)
        bc[q] = base[cq] - cb0;
#pragma unroll
        for (int j = 0; j < 4; ++j) wc[q][j] = w[4 * (size_t)cq + j];
    }
    // the source row with tile index k, interpolated at this lane's column q
    auto hrow = [&](int k, int q) {
        const double *s = tile + k * PC_SRC_COLS + bc[q];
        double v = wc[q][0] * s[0] + wc[q][1] * s[1];
        v = v + wc[q][2] * s[2];
        if (m > 3) v = v + wc[q][3] * s[3];
        return v;
    };
    double h0[CPT], h1[CPT], h2[CPT], h3[CPT];
#pragma unroll
    for (int q = 0; q < CPT; ++q) h0[q] = h1[q] = h2[q] = h3[q] = 0.0;
    int hb = 0;
    bool have = false;
    for (int rr = 0; rr < PC_ROWS; ++rr) {
        const int r = r0 + rr;
        if (r >= Nd - 1) break;
        if (r == 0) continue;
        const int rb = base[r];   // (uniform over the block)
        if (!have || rb - hb >= m) {
#pragma unroll
            for (int q = 0; q < CPT; ++q) {
                h0[q] = hrow(rb - rb0, q);
                h1[q] = hrow(rb - rb0 + 1, q);
                h2[q] = hrow(rb - rb0 + 2, q);
                if (m > 3) h3[q] = hrow(rb - rb0 + 3, q);
            }
            hb = rb;
            have = true;
        } else {
            while (hb < rb) {
                ++hb;
#pragma unroll
                for (int q = 0; q < CPT; ++q) {
                    h0[q] = h1[q];
                    h1[q] = h2[q];
                    if (m > 3) {
                        h2[q] = h3[q];
                        h3[q] = hrow(hb - rb0 + 3, q);
                    } else {
                        h2[q] = hrow(hb - rb0 + 2, q);
                    }
                }
            }
        }
        const double wr0 = w[4 * (size_t)r], wr1 = w[4 * (size_t)r + 1], wr2 = w[4 * (size_t)r + 2], wr3 = w[4 * (size_t)r + 3];
        double o[CPT];
#pragma unroll
        for (int q = 0; q < CPT; ++q) {
            double v = wr0 * h0[q] + wr1 * h1[q];
            v = v + wr2 * h2[q];
            if (m > 3) v = v + wr3 * h3[q];
            o[q] = v;
        }
        const size_t p = (size_t)r * Nd + c;
        if constexpr (PAIR) {
            if (c == 0) {
                Uf[p + 1] = o[1];
            } else if (c + 1 == Nd - 1) {
                Uf[p] = o[0];
            } else {
                const double2_s v = {o[0], o[1]};
                if (NT) __builtin_nontemporal_store(v, reinterpret_cast<double2_s *>(Uf + p));
                else *reinterpret_cast<double2_s *>(Uf + p) = v;
            }
        } else {
            if (c > 0 && c < Nd - 1) Uf[p] = o[0];
        }
    }
}

template <bool PAIR, bool NT>
__global__ __launch_bounds__(TB) void k_prolong_cubic(int Ns, int Nd, const int *__restrict__ base, const double *__restrict__ w,
                                                      const double *__restrict__ Uc, double *__restrict__ Uf)
{
    prolong_cubic_body<PAIR, NT>(Ns, Nd, base, w, Uc, Uf);
}

inline bool use_pairs(int N) { return N % 2 == 0 && N >= PAIR_MIN_N; }

// ---------------------------------------------------------------- rim data
__global__ __launch_bounds__(TB) void k_rim_extract(int N, const double *__restrict__ U, double *__restrict__ g)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= N) return;
    g[i] = U[i];
    g[(size_t)N + i] = U[(size_t)(N - 1) * N + i];
    g[2 * (size_t)N + i] = U[(size_t)i * N];
    g[3 * (size_t)N + i] = U[(size_t)i * N + N - 1];
}

// edge blockIdx.y of the coarse rim: the 1-D interpolation of the fine edge in the header's order
__global__ __launch_bounds__(TB) void k_rim_sample(int Nf, int Nc, const int *__restrict__ base, const double *__restrict__ w,
                                                   const double *__restrict__ gf, double *__restrict__ gc)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= Nc) return;
    const int m = Nf < 4 ? Nf : 4;
    const double *s = gf + (size_t)blockIdx.y * Nf + base[i];
    const double *wi = w + 4 * (size_t)i;
    double v = wi[0] * s[0] + wi[1] * s[1];
    v = v + wi[2] * s[2];
    if (m > 3) v = v + wi[3] * s[3];
    gc[(size_t)blockIdx.y * Nc + i] = v;
}

__device__ __forceinline__ double rim_value(int r, int c, int N, const double *__restrict__ g)
{
    if (r == 0) return g[c];
    if (r == N - 1) return g[(size_t)N + c];
    if (c == 0) return g[2 * (size_t)N + r];
    return g[3 * (size_t)N + r];
}

// rim_only(g): the rim from the edges, +0 inside
__global__ __launch_bounds__(TB) void k_rim_only(int N, const double *__restrict__ g, double *__restrict__ U)
{
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p >= (size_t)N * N) return;
    const int r = (int)(p / N), c = (int)(p - (size_t)r * N);
    const bool on_rim = r == 0 || c == 0 || r == N - 1 || c == N - 1;
    U[p] = on_rim ? rim_value(r, c, N, g) : 0.0;
}

// the rim of U from the edges; nothing inside is written (the corners come from the row edges)
__global__ __launch_bounds__(TB) void k_rim_write(int N, const double *__restrict__ g, double *__restrict__ U)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= N) return;
    U[i] = g[i];
    U[(size_t)(N - 1) * N + i] = g[(size_t)N + i];
    if (i > 0 && i < N - 1) {
        U[(size_t)i * N] = g[2 * (size_t)N + i];
        U[(size_t)i * N + N - 1] = g[3 * (size_t)N + i];
    }
}

__global__ void k_flag_or(const int *__restrict__ gs_state, int *__restrict__ acc)
{
    if (threadIdx.x == 0 && gs_state[2]) *acc = 1;
}

}  // namespace

// ------------------------------------------------------------------ launchers
bool cubic_table_fits(int N_src, int N_dst, const int *base)
{
    const int m = N_src < 4 ? N_src : 4;
    const int W = use_pairs(N_dst) ? 2 * TB : TB;
    for (int c0 = 0; c0 < N_dst; c0 += W) {
        const int cl = c0 + W - 1 < N_dst - 1 ? c0 + W - 1 : N_dst - 1;
        if (base[cl] + m - (base[c0] & ~1) + 1 > PC_SRC_COLS) return false;   // (with the alignment and the rounding to pairs)
    }
    for (int r0 = 0; r0 < N_dst; r0 += PC_ROWS) {
        const int rl = r0 + PC_ROWS - 1 < N_dst - 1 ? r0 + PC_ROWS - 1 : N_dst - 1;
        if (base[rl] + m - base[r0] > PC_SRC_ROWS) return false;
    }
    return true;
}

void prolong_cubic(hipStream_t s, const CubicTable &t, const double *Uc, double *Uf)
{
    const int Ns = t.N_src, Nd = t.N_dst;
    const bool pairs = use_pairs(Nd);
    const dim3 g((Nd + (pairs ? 2 * TB : TB) - 1) / (pairs ? 2 * TB : TB), (Nd + PC_ROWS - 1) / PC_ROWS);
    if (pairs && Nd >= NT_MIN_N) hipLaunchKernelGGL((k_prolong_cubic<true, true>), g, dim3(TB), 0, s, Ns, Nd, t.base, t.w, Uc, Uf);
    else if (pairs) hipLaunchKernelGGL((k_prolong_cubic<true, false>), g, dim3(TB), 0, s, Ns, Nd, t.base, t.w, Uc, Uf);
    else hipLaunchKernelGGL((k_prolong_cubic<false, false>), g, dim3(TB), 0, s, Ns, Nd, t.base, t.w, Uc, Uf);
}

void rim_extract(hipStream_t s, int N, const double *U, double *g)
{
    hipLaunchKernelGGL(k_rim_extract, dim3((N + TB - 1) / TB), dim3(TB), 0, s, N, U, g);
}

void rim_sample(hipStream_t s, const CubicTable &t, const double *g_f, double *g_c)
{
    hipLaunchKernelGGL(k_rim_sample, dim3((t.N_dst + TB - 1) / TB, 4), dim3(TB), 0, s, t.N_src, t.N_dst, t.base, t.w, g_f, g_c);
}

void rim_fill(hipStream_t s, int N, const double *g, double *U, bool zero_interior)
{
    if (zero_interior) {
        const size_t n = (size_t)N * N;
        hipLaunchKernelGGL(k_rim_only, dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, s, N, g, U);
    } else {
        hipLaunchKernelGGL(k_rim_write, dim3((N + TB - 1) / TB), dim3(TB), 0, s, N, g, U);
    }
}

void flag_or(hipStream_t s, const int *gs_state, int *acc)
{
    hipLaunchKernelGGL(k_flag_or, dim3(1), dim3(64), 0, s, gs_state, acc);
}

}  // namespace k
}  // namespace mg
