// mg_exp_libm.h -- libm's exp() on the device, shared by the problem definition (mg_kernels.hip: k_source, k_analytic) and
// the semilinear residual (mg_newton_impl.h): both translation units compile THIS body, with its explicit fused
// multiply-adds, so -ffp-contract=off does not touch it and the two agree bit for bit.
// src/MG_solver_CPU.cpp:488 / :544 call libm's exp().  exp_libm() evaluates it with the operations of the
// algorithm glibc has used since 2.28 (exp(x) = 2^(k/128) * exp(r): a 128-entry table, a degree-5 polynomial),
// in the FMA form glibc selects on every CPU with FMA: the fused multiply-adds below are the ones that build
// performs (disassembly of libm.so.6 2.35: z + Shift, both reduction steps, every polynomial step and the final
// scale are fused).  The table comes from scripts/gen_exp_table.py (computed from its definition), the constants
// are the algorithm's published ones.  Nothing is assumed: mg_source_selfcheck() compares getSource on the device
// with the host's libm bit for bit before the device form becomes the default (mg_abi.cpp).
// The verified path is |x| < 512: there tests/test_newton_exp_domain_gpu.py holds this function, as the semilinear pass
// evaluates it in each of its kernel forms, to a longdouble reference at every k = round(x*128/ln 2) (largest error 0.5054 ulp,
// the host libm's own) and, bit for bit, to a restatement built on the C library's fma.  Beyond it exp_libm() returns the
// device library's exp(), which is not held against libm: a bit-for-bit contract built on this function covers |x| < 512
// only.  That branch IS reached: getSource never leaves the unit square, but the semilinear solve of kind MG_NEWTON_EXP
// accepts trials with v <= -512 (include/mg_newton.h).  Guaranteed there: +inf above 709.782712893384 and for +inf, +0 from
// -746 down and for -inf, NaN for NaN, otherwise a finite result >= 0 (subnormal below -708.39) within 2 ulp of e^x, an
// error in a subnormal result counted in the subnormal spacing (measured: 0.4984 ulp at the most).
#ifndef MG_EXP_LIBM_H
#define MG_EXP_LIBM_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mg_exp_table.h"

namespace mg {
namespace k {

namespace {

__device__ const uint64_t exp_tab[256] = {MG_EXP_TABLE_VALUES};
__device__ __forceinline__ double exp_libm(double x)
{
    const uint32_t abstop = (uint32_t)(__double_as_longlong(x) >> 52) & 0x7ff;
    if (abstop - 0x3c9u > 0x3eu) {
        if (abstop < 0x3c9u) return 1.0 + x;  // |x| < 2^-54
        return exp(x);                        // |x| >= 512, inf, NaN: the device library's exp (class and 2 ulp, see above)
    }
    const double InvLn2N = 0x1.71547652b82fep+7, Shift = 0x1.8p+52, NegLn2hiN = -0x1.62e42fefa0000p-8,
                 NegLn2loN = -0x1.cf79abc9e3b3ap-47, C2 = 0x1.ffffffffffdbdp-2, C3 = 0x1.555555555543cp-3,
                 C4 = 0x1.55555cf172b91p-5, C5 = 0x1.1111167a4d017p-7;
    const double kd_s = __builtin_fma(x, InvLn2N, Shift);
    const uint64_t ki = (uint64_t)__double_as_longlong(kd_s);
    const double kd = kd_s - Shift;
    double r = __builtin_fma(kd, NegLn2hiN, x);
    r = __builtin_fma(kd, NegLn2loN, r);
    const unsigned idx = 2u * (unsigned)(ki & 127u);
    const double tail = __longlong_as_double((long long)exp_tab[idx]);
    const uint64_t sbits = exp_tab[idx + 1] + (ki << 45);
    const double p23 = __builtin_fma(r, C3, C2);
    const double rt = r + tail;
    const double r2 = r * r;
    const double p45 = __builtin_fma(r, C5, C4);
    const double t = __builtin_fma(p23, r2, rt);
    const double r4 = r2 * r2;
    const double tmp = __builtin_fma(r4, p45, t);
    const double scale = __longlong_as_double((long long)sbits);
    return __builtin_fma(scale, tmp, scale);
}

}  // namespace

}  // namespace k
}  // namespace mg

#endif /* MG_EXP_LIBM_H */
