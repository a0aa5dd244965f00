// mg_eigs_kernels.hip -- fp64 kernels of the eigen-solver (include/mg_eigs.h; driven by mg_eigs.cpp): k_eig_gram, one pass
// over the 2m basis fields that leaves both Gram matrices G = S^T S and H = S^T AS; k_eig_rotate<M>, the block rotation of
// the Rayleigh-Ritz step fused with the residuals and their norms; k_eig_resnorm, the residual recomputed from X and AX; the
// one finish kernel that adds per-block partials in a fixed order; and the start of a column.  The __device__ bodies live in
// mg_eigs_impl.h.  Built with -ffp-contract=off like every kernel file: include/mg_eigs.h fixes one rounding per product
// and per sum, so numpy restates the rotation bit for bit.
//
// k_eig_gram tiles the (j, l) pairs 6 x 6 over blockIdx.z: a tile holds 2*36 = 72 fp64 accumulators (144 VGPRs) and the 18
// (diagonal tiles: 12) values of a point.  The m(m + 1) = 1332 sums of m = 36 in one block would need 2664 VGPRs; a 12 x 12
// tile needs 576 + 72 and spills; 8 x 8 needs 256 + 48, one wave per SIMD; 6 x 6 is the largest square tile that leaves two
// (DESIGN 4.3.5 has the compiler's counts).  The price is re-reading: tile (a, b) reads its 18 fields whatever the other
// tiles read, 21 tiles at m = 36 -- 342 field reads where 72 are compulsory; blockIdx.z, the tile, is the slowest grid index,
// so the tiles of one point do not run side by side and share nothing in L2 by design of the order (see DESIGN).
// k_eig_rotate<M> holds the 2m values of a point in registers (M = 36: 144 VGPRs, one column per lane; the pair form only
// up to M = 12) and reads C, Cp and theta through scalar loads from a table the driver uploads per iteration.
// Every sum is per-block partials in a fixed partition (block (x, y) -> slot y*gridDim.x + x, one stripe of slots per sum)
// and the finish launch: no floating-point atomics, the same call twice gives the same bits.
#include <hip/hip_runtime.h>

#include "mg_internal.h"
#include "mg_eigs_impl.h"

namespace mg {
namespace k {

namespace {

template <bool PAIR>
__global__ __launch_bounds__(TB) void k_eig_gram(int N, int m, const double *const *__restrict__ ptrs, double *__restrict__ part)
{
    eig_gram_body<PAIR>(N, m, ptrs, part);
}

template <int M, bool PAIR>
__global__ __launch_bounds__(TB) void k_eig_rotate(int N, int m, int p, double *const *__restrict__ ptrs,
                                                   const double *__restrict__ coef, double *__restrict__ part)
{
    eig_rotate_body<M, PAIR>(N, m, p, ptrs, coef, part);
}

template <bool PAIR>
__global__ __launch_bounds__(TB) void k_eig_resnorm(int N, int p, double *const *__restrict__ ptrs, const double *__restrict__ coef,
                                                    double *__restrict__ part)
{
    eig_resnorm_body<PAIR>(N, p, ptrs, coef, part);
}

// block b: out[b] = the sum of stripe b
__global__ __launch_bounds__(1024) void k_eig_finish(const double *__restrict__ part, size_t nb, double *__restrict__ out)
{
    const double s = finish_sum(part + (size_t)blockIdx.x * nb, nb);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

__global__ __launch_bounds__(TB) void k_eig_start(int N, double *__restrict__ dst, const double *__restrict__ src)
{
    const int c = blockIdx.x * TB + threadIdx.x, r = blockIdx.y;
    if (c >= N) return;
    const size_t p = (size_t)r * N + c;
    const bool interior = c > 0 && c < N - 1 && r > 0 && r < N - 1;
    dst[p] = interior ? (src ? src[p] : dst[p] - 0.5) : 0.0;
}

template <int M>
void launch_rotate(hipStream_t s, int N, int m, int p, double *const *ptrs, const double *coef, double *part)
{
    if constexpr (M <= 12) {
        if (use_pairs(N)) {
            hipLaunchKernelGGL((k_eig_rotate<M, true>), eig_grid(N, ROT_ROWS), dim3(TB), 0, s, N, m, p, ptrs, coef, part);
            return;
        }
    }
    const dim3 g((N + TB - 1) / TB, (N + ROT_ROWS - 1) / ROT_ROWS);
    hipLaunchKernelGGL((k_eig_rotate<M, false>), g, dim3(TB), 0, s, N, m, p, ptrs, coef, part);
}

}  // namespace

// ------------------------------------------------------------------ launchers
size_t eigs_gram_blocks(int N)
{
    const dim3 g = eig_grid(N, GRAM_ROWS);
    return (size_t)g.x * g.y;
}

// (the larger of the two grids a rotation may take: the pair form is left at M > 12)
size_t eigs_rotate_blocks(int N)
{
    return (size_t)((N + TB - 1) / TB) * ((N + ROT_ROWS - 1) / ROT_ROWS);
}

void eigs_gram(hipStream_t s, int N, int m, const double *const *ptrs, double *part, double *out)
{
    dim3 g = eig_grid(N, GRAM_ROWS);
    const size_t nb = (size_t)g.x * g.y;
    g.z = eigs_tiles(m);
    if (use_pairs(N)) hipLaunchKernelGGL(k_eig_gram<true>, g, dim3(TB), 0, s, N, m, ptrs, part);
    else hipLaunchKernelGGL(k_eig_gram<false>, g, dim3(TB), 0, s, N, m, ptrs, part);
    hipLaunchKernelGGL(k_eig_finish, dim3(g.z * EIGS_TILE_SUMS), dim3(1024), 0, s, part, nb, out);
}

void eigs_rotate(hipStream_t s, int N, int m, int p, double *const *ptrs, const double *coef, double *part, double *res2)
{
    const bool pairs = use_pairs(N) && m <= 12;
    if (m <= 3) launch_rotate<3>(s, N, m, p, ptrs, coef, part);
    else if (m <= 6) launch_rotate<6>(s, N, m, p, ptrs, coef, part);
    else if (m <= 12) launch_rotate<12>(s, N, m, p, ptrs, coef, part);
    else if (m <= 18) launch_rotate<18>(s, N, m, p, ptrs, coef, part);
    else if (m <= 24) launch_rotate<24>(s, N, m, p, ptrs, coef, part);
    else launch_rotate<36>(s, N, m, p, ptrs, coef, part);
    const dim3 g = pairs ? eig_grid(N, ROT_ROWS) : dim3((N + TB - 1) / TB, (N + ROT_ROWS - 1) / ROT_ROWS);
    hipLaunchKernelGGL(k_eig_finish, dim3(p), dim3(1024), 0, s, part, (size_t)g.x * g.y, res2);
}

void eigs_resnorm(hipStream_t s, int N, int p, double *const *ptrs, const double *coef, double *part, double *res2)
{
    const dim3 g = eig_grid(N, ROT_ROWS);
    if (use_pairs(N)) hipLaunchKernelGGL(k_eig_resnorm<true>, g, dim3(TB), 0, s, N, p, ptrs, coef, part);
    else hipLaunchKernelGGL(k_eig_resnorm<false>, g, dim3(TB), 0, s, N, p, ptrs, coef, part);
    hipLaunchKernelGGL(k_eig_finish, dim3(p), dim3(1024), 0, s, part, (size_t)g.x * g.y, res2);
}

void eigs_start(hipStream_t s, int N, double *dst, const double *src)
{
    hipLaunchKernelGGL(k_eig_start, dim3((N + TB - 1) / TB, N), dim3(TB), 0, s, N, dst, src);
}

}  // namespace k
}  // namespace mg
