"""The case tables of tests/test_bc_forms_gpu.py and tests/test_bc_exact_gpu.py, shared with tests/test_bc_forms_cpu.py, which
checks on the CPU what the GPU cases rest on: the qualification of every seed and the teeth of the bounds.
TEST INFRASTRUCTURE."""
import numpy as np

import _bc_ref as bref
import _exact as ex
import _solve_ref as ref
import _solve_vc_ref as vref

LD = np.longdouble

# ---------------------------------------------------------------- kernels alone
# (N, kinds, operation, L, shift) of test_bc_forms_gpu.test_forms_alone; the operations are the keys of its _launches.  The
# size varies slowest (one guarded block per size).  Within a size the shift values 0 and 1e4 (and at the pair sizes three
# values of L) alternate with kind + operation, so that every operation and every kind meets both; 4098 takes the other shift
# of 4096.
FOUR = ("nnnn", "ddnd", "ndnd", "dndn")          # (test_solve_bc_gpu.FOUR)
PAIR_KINDS, PAIR_OPS = FOUR + ("nddn",), ("residual-none", "sweep0-none")
NT_KINDS = ("nnnn", "dndn", "ndnd")
NT_OPS = ("sweep", "sweep0", "sweep0-none", "residual-none", "residual", "apply", "heat-half", "heat-one")
FORM_CASES = [(N, bc, op, (1.0, 1e-3, 1e3)[(ib + io) % 3], (0.0, 1e4)[(ib + io + N // 2) % 2])
              for N in (512, 514, 1026) for ib, bc in enumerate(PAIR_KINDS) for io, op in enumerate(PAIR_OPS)]
FORM_CASES += [(N, bc, op, 1.0, (0.0, 1e4)[(ib + io + N // 2) % 2])
               for N in (4096, 4098) for ib, bc in enumerate(NT_KINDS) for io, op in enumerate(NT_OPS)]

# ---------------------------------------------------------------- whole solves against the restatement at the pair sizes
# 514 -> 257 -> 128 ... and 1026 -> 513 -> 256 ...: a pair level on top, an odd level below it
CYCLES = 2
SOLVE_SEED = {514: 3514, 1026: 4026}
SOLVE_KINDS = [("nnnd", 10.0), ("dndn", 0.0)]
SOLVE_CASES = [(N, bc, shift, name, pp) for N, pps in ((514, ((3, 3), (1, 2))), (1026, ((3, 3),))) for bc, shift in SOLVE_KINDS
               for name in (None, "exp") for pp in pps]


def restated_cycles(N, bc, shift, name, pp, rtable=None, ptable=None):
    """(F, U0, a, [U after cycle 1 .. CYCLES], [residual norm of the start and after every cycle], coarse margins) of one
    case on the numpy restatement; rtable / ptable: the library's tables in the restatement's place"""
    F, U0 = ref.random_problem(N, SOLVE_SEED[N])
    a = vref.field(name, N) if name else None
    levels = vref.coarsen_levels(a, 8, rtable) if name else None
    margins, Us, U = [], [], U0
    hist = [bref.residual_norm(N, 1.0, bc, a, U0, F, shift)]
    for _ in range(CYCLES):
        U = bref.cycle(levels, F, U, bc, 1.0, margins=margins, rtable=rtable, ptable=ptable, pre=pp[0], post=pp[1], shift=shift)
        Us.append(U)
        hist.append(bref.residual_norm(N, 1.0, bc, a, U, F, shift))
    return F, U0, a, Us, hist, margins


# ---------------------------------------------------------------- solves of exact discrete modes
# (N, L, bc, sigma, (k, l)): F = (c*lambda_kl - sigma)*U*, U* = mixed_mode(N, bc, k, l), c the constant coefficient (1 or 2),
# L as tests/test_exact_gpu.py (2.5 and 7.0), rtol 1e-10.  The bound of _exact.check_mode_solve must stay below 1e-6*max|U*|
# (teeth).  With ||U*||_2 about (N/2)*max|U*| and a residual that stops at rho*||F||, rho <= rtol, the bound is about
# rho*N*(|lambda| + sigma)/(lambda_min + sigma): what decides is how far the mode lies above the lowest one.  Measured on the
# numpy restatement (bref.solve), bound / max|U*| at 514 and 1026, the same with the coefficient 2 to the digits shown:
#   low mode (1, 2)       nnnn 1e2: 9.1e-9, 6.7e-9   dnnd / ndnd 0: 1.3e-7, 3.2e-7   dnnd / ndnd / nnnd 1e2: 1.2 .. 3.3e-8
#                         nnnd 0: 1.0e-6, 2.2e-6 -- no teeth; its lowest mode is (0, 0) with lambda_min = lambda_12 / 25.  That
#                         case takes (0, 1), lambda = 5*lambda_min: at most 1e-10*5*N whatever rho the solve stops at
#   high mode (N/3, 2)    sigma 0: 1.3e-3 .. 2.0e-2, sigma 1e2: 1.0e-5 .. 2.1e-5 for every kind -- no teeth at either shift,
#                         lambda is 1e4 .. 1e5 times lambda_min.  The high mode runs at sigma = 1e4 instead, once per kind:
#                         2.0e-8 .. 9.3e-8 at 514, 3.6e-9 .. 1.1e-7 at 1026 (the low mode there as well: at most 9.3e-8)
# The case at 4096 ("nnnd", 1e2, (1, 2)) has 1.2e-7 on the restatement (7 cycles; 104 s on the CPU, so no test repeats it).
# So each kind keeps its low mode at the shifts asked for (0 and 1e2; four Neumann sides 1e2 alone) and runs the high mode at 1e4.
MODE_RTOL = 1e-10
MODE_L = {514: 2.5, 1026: 7.0, 4096: 2.5}
MODE_COEFS = (None, 2.0)
HIGH_SIGMA = 1e4


def high(N):
    return (N // 3, 2)


def low(bc, sigma):
    return (0, 1) if (bc, sigma) == ("nnnd", 0.0) else (1, 2)


MODE_KINDS = [("nnnn", (1e2,)), ("dnnd", (0.0, 1e2)), ("ndnd", (0.0, 1e2)), ("nnnd", (0.0, 1e2))]
MODE_CASES = [(N, MODE_L[N], bc, sigma, low(bc, sigma)) for N in (514, 1026) for bc, sigmas in MODE_KINDS for sigma in sigmas]
MODE_CASES += [(N, MODE_L[N], bc, HIGH_SIGMA, high(N)) for N in (514, 1026) for bc, _ in MODE_KINDS]
MODE_CASES.append((4096, MODE_L[4096], "nnnd", 1e2, (1, 2)))


def mode_problem(N, L, bc, sigma, kl, coef=None):
    """(U* in longdouble, F in fp64, lam_min of the operator with its coefficient)"""
    c = LD(1.0 if coef is None else coef)
    star = ex.mixed_mode(N, bc, *kl)
    lam = c * ex.mixed_mode_eigenvalue(N, L, bc, *kl)
    return star, ex.r64((lam - LD(sigma)) * star), c * ex.lambda_min(N, L, bc)


# ---------------------------------------------------------------- heat steps on exact discrete modes
HEAT = dict(L=2.5, nu=0.5, dt=2e-2, rtol=1e-8, A=0.5, kl=(2, 3))
HEAT_CASES = [(514, "nnnn"), (514, "ndnd"), (1026, "nnnn")]
HEAT_STEPS = 3


def heat_problem(N, bc, theta, coef=None):
    return ex.Perturbed(N, HEAT["L"], HEAT["nu"], HEAT["dt"], theta, *HEAT["kl"], HEAT["A"], steady=False, bc=bc, coef=coef)
