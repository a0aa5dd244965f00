// mg_reaction_impl.h -- what is the reaction kernels' own (include/mg_reaction.h; kernels and launchers:
// mg_reaction_kernels.hip, mg_reaction_batch_kernels.hip): the check of s.  The sweep, the residual, the operator, the norm and
// the coarse solve are mg_varcoef_impl.h's bodies with HAS_S = true -- the centre gets sd + s[p]*dx2 per point (centre_sd) --
// and the coefficient as a switch of its own: HAS_A = false streams no array of ones.
#ifndef MG_REACTION_IMPL_H
#define MG_REACTION_IMPL_H

#include "mg_varcoef_impl.h"

namespace mg {
namespace k {

namespace {

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
