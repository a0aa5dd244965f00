"""The heat stepper (include/mg_heat.h) without a GPU: the header against the binding, and what the scheme promises, asserted
on the restatement (tests/_heat_ref.py) with the oracle's transfer operators: one step multiplies a discrete eigenmode by the
theta-scheme's amplification factor to within the stopping rule, and the warm start from u_old never costs cycles."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _heat_ref as href
import _solve_ref as ref
import _solve_shift_ref as sref
from conftest import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
SYMBOLS = ("mg_heat_opts_default", "mg_heat_rhs", "mg_heat_stepper_create", "mg_heat_stepper_step", "mg_heat_stepper_sigma",
           "mg_heat_stepper_destroy")


def _header():
    return open(os.path.join(ROOT, "include", "mg_heat.h")).read()


def test_header_declares_what_the_binding_binds_and_the_library_exports():
    import multigrid_poisson_solver_amd as m
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mg_heat_[A-Za-z0-9_]+)\s*\(", text)))
    assert declared == sorted(SYMBOLS)
    lib = m.load_library()
    for name in declared:
        assert name in m.ABI_HEAT and name not in m.ABI and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == m.ABI_HEAT[name][1]
    assert sorted(m.ABI_HEAT) == declared
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert '#include "mg_heat.h"' in hip and hip.index('#include "mg_heat.h"') > hip.index('#include "mg_fmg.h"')
    # no prototype of the stepper in mg_hip.h itself
    assert not re.search(r"\bmg_heat_\w+\s*\(", re.sub(r"/\*.*?\*/", "", hip, flags=re.S))


def _fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), re.S).group(1)
    names = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [re.search(r"(\w+)$", first.strip()).group(1)] + [re.search(r"(\w+)$", x.strip()).group(1) for x in rest]
    return names


def test_structures_match_the_header():
    import multigrid_poisson_solver_amd as m
    assert [f for f, _ in m.HeatOpts._fields_] == _fields("mg_heat_opts") == ["nu", "dt", "theta", "solve"]
    assert C.sizeof(m.HeatOpts) == 3 * 8 + C.sizeof(m.SolveOpts) and m.HeatOpts.solve.offset == 24
    assert [f for f, _ in m.HeatResult._fields_] == _fields("mg_heat_result")
    # four ints, three doubles, an int padded to the pointer, the pointer
    assert C.sizeof(m.HeatResult) == 16 + 24 + 8 + 8 and m.HeatResult.cycles_per_step.offset == 48


def test_defaults():
    import multigrid_poisson_solver_amd as m
    o = m.HeatOpts()
    o.nu, o.dt, o.theta = 7.0, 7.0, 0.7
    o.solve.shift, o.solve.fmg, o.solve.pre = 3.0, 2, 1
    m.load_library().mg_heat_opts_default(C.byref(o))
    want = m.SolveOpts()
    m.load_library().mg_solve_opts_default(C.byref(want))
    assert (o.nu, o.dt, o.theta) == (1.0, 1.0, 1.0)
    for f, _ in m.SolveOpts._fields_:
        assert getattr(o.solve, f) == getattr(want, f), f
    for f in (m.heat_rhs, m.HeatStepper, m.heat_opts):
        assert "theta" in f.__doc__, f.__name__


# ---------------------------------------------------------------- the scheme, on the restatement
def mode(N, k, l):
    i = np.arange(N).astype(LD)
    pi = ref._ld_pi()
    u = np.outer(np.sin(LD(k) * pi * i / LD(N - 1)), np.sin(LD(l) * pi * i / LD(N - 1))).astype(np.float64)
    u[0, :] = u[-1, :] = 0.0
    u[:, 0] = u[:, -1] = 0.0
    return u


def eigenvalue(N, k, l):
    """lambda = (4/dx^2)(sin^2(k pi / (2(N-1))) + sin^2(l pi / (2(N-1)))), L = 1, in longdouble"""
    pi = ref._ld_pi()
    return 4 * ref._inv_ld(N, 1.0) * (np.sin(LD(k) * pi / LD(2 * (N - 1))) ** 2 + np.sin(LD(l) * pi / LD(2 * (N - 1))) ** 2)


def scheme(theta, sigma_wanted):
    """(nu, dt) with sigma = 1/(theta*nu*dt) at (or within rounding of) the wanted value; the sigma used is consts()'s"""
    return 1.0, 1.0 / (theta * sigma_wanted)


@pytest.mark.parametrize("sigma_wanted", [1e2, 1e4])
@pytest.mark.parametrize("theta", [1.0, 0.75, 0.5])
@pytest.mark.parametrize("k,l", [(1, 1), (2, 3)])
@pytest.mark.parametrize("N", [33, 65])
def test_one_step_is_the_amplification_factor(oracle, N, k, l, theta, sigma_wanted):
    """u+ = rho*u0, rho = (sigma - beta*lambda)/(sigma + lambda), to within the stopping rule over the smallest eigenvalue of
    the operator: ||u+ - rho u0|| <= (rtol*|sigma - beta*lambda|*||u0|| + R)/(sigma + lambda_min), R the rounding bound of
    the residual evaluation.  Nothing in the bound is measured."""
    rtol = 1e-8
    nu, dt = scheme(theta, sigma_wanted)
    sigma, beta, _, _ = href.consts(N, 1.0, nu, dt, theta)
    assert abs(sigma - sigma_wanted) <= 4 * np.spacing(sigma_wanted)
    u0 = mode(N, k, l)
    lam = eigenvalue(N, k, l)
    rho = (LD(sigma) - LD(beta) * lam) / (LD(sigma) + lam)
    U, hist, cycles, conv = href.step(oracle, u0, None, 1.0, nu, dt, theta, rtol=rtol)
    assert conv
    F = href.rhs(N, 1.0, nu, dt, theta, u0)
    R = sref.residual_rounding_bound(U, F, 1.0, sigma)
    err = ref.norm_ld(U.astype(LD) - rho * u0.astype(LD))
    bound = (LD(rtol) * abs(LD(sigma) - LD(beta) * lam) * ref.norm_ld(u0) + R) / (LD(sigma) + sref.lambda_11(N, 1.0))
    print(f"N={N} mode ({k},{l}) theta={theta} sigma={sigma:g}: rho {float(rho):.6f}, {cycles} cycles, "
          f"error {float(err):.3e} bound {float(bound):.3e}")
    assert err <= bound


@pytest.mark.parametrize("N", [33, 65])
def test_warm_start_costs_no_more_cycles_than_a_zero_interior(oracle, N):
    theta, rtol = 1.0, 1e-8
    nu, dt = scheme(theta, 1e4)
    sigma = href.consts(N, 1.0, nu, dt, theta)[0]
    u0 = mode(N, 1, 1)
    _, _, warm, conv_w = href.step(oracle, u0, None, 1.0, nu, dt, theta, rtol=rtol)
    F = href.rhs(N, 1.0, nu, dt, theta, u0)
    _, _, cold, conv_c = sref.solve(oracle, F, ref.rim_only(u0), 1.0, shift=sigma, rtol=rtol)
    print(f"N={N}: cycles from U = u_old {warm}, from a zero interior {cold}")
    assert conv_w and conv_c and warm <= cold


@pytest.mark.parametrize("N", [6, 17, 64])
def test_backward_euler_rhs_is_minus_sigma_u(N):
    _, U = ref.random_problem(N, 70 + N)
    nu, dt = 0.3, 1e-3
    sigma = href.consts(N, 2.5, nu, dt, 1.0)[0]
    F = href.rhs(N, 2.5, nu, dt, 1.0, U)
    assert_bits(F[1:-1, 1:-1], -(sigma * U[1:-1, 1:-1]), "interior")
    rim = np.concatenate([F[0, :], F[-1, :], F[:, 0], F[:, -1]])
    assert not np.any(rim) and not np.any(np.signbit(rim))
    # ... and with theta < 1 the rim of U enters only through the neighbours of the first interior ring
    G = href.rhs(N, 2.5, nu, dt, 0.5, U)
    rimG = np.concatenate([G[0, :], G[-1, :], G[:, 0], G[:, -1]])
    assert not np.any(rimG) and not np.any(np.signbit(rimG)) and not np.array_equal(G, F)
