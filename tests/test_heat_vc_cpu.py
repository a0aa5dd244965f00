"""The heat stepper with a variable coefficient (include/mg_heat_vc.h) without a GPU: the header against the binding, and the
restatement (tests/_heat_vc_ref.py) against what the header promises and against truth -- a == 1 is the constant right-hand
side bit for bit, one step lands on the dense direct solution of its own discrete system to within the stopping rule and the
roundings, and a perturbation of a steady state decays at least as fast as the smallest eigenvalue allows.

Measured on the restatement: one step, all 24 cases: error/bound <= 0.77, ||F - F*||/eps <= 0.06, bound/moved <= 2e-9; the
steady state, rho = 1/2: error ratios 0.352, 0.137, 0.054, 0.021 against rho^n = 0.5 ... 0.0625."""
import os
import re

import numpy as np
import pytest

import _heat_ref as href
import _heat_vc_ref as hvref
import _solve_ref as ref
from conftest import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mg_heat_rhs_coef", "mg_heat_stepper_set_coefficient", "mg_heat_stepper_has_coefficient")


def test_header_declares_what_the_binding_binds_and_the_library_exports():
    import multigrid_poisson_solver_amd as m
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mg_heat_vc.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))
    assert declared == sorted(SYMBOLS)
    lib = m.load_library()
    for name in declared:
        assert name in m.ABI_HEAT_VC and hasattr(lib, name), name
        assert not any(name in abi for abi in (m.ABI, m.ABI_FMG, m.ABI_HEAT, m.ABI_VC)), name
        assert getattr(lib, name).argtypes == m.ABI_HEAT_VC[name][1]
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(m.ABI_HEAT_VC[name][1]), name
    assert sorted(m.ABI_HEAT_VC) == declared
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    order = [hip.index('#include "%s"' % h) for h in ("mg_fmg.h", "mg_heat.h", "mg_varcoef.h", "mg_heat_vc.h")]
    assert order == sorted(order)
    assert b"0.2.2" in lib.mg_version()
    # the surface: equation, the a == 1 and theta = 1 consequences and the two refusals are in the docstrings
    for f in (m.HeatStepper, m.HeatStepper.set_coefficient):
        for word in ("div(a grad u)", "a == 1", "theta = 1", "max_batch > 1", "fmg"):
            assert word in f.__doc__, (f.__qualname__, word)
    assert "div(a grad u)" in m.heat_rhs_coef.__doc__ and "a == 1" in m.heat_rhs_coef.__doc__
    assert isinstance(m.HeatStepper.has_coefficient, property)


@pytest.mark.parametrize("with_q", [True, False])
@pytest.mark.parametrize("theta", [1.0, 0.75, 0.5])
@pytest.mark.parametrize("N", [3, 4, 5, 17, 64, 100])
def test_unit_coefficient_is_the_constant_right_hand_side(N, theta, with_q):
    rng = np.random.default_rng(1000 + N)
    U, Q = rng.standard_normal((N, N)), rng.standard_normal((N, N)) if with_q else None
    for L, nu, dt in ((2.5, 0.7, 1e-3), (1.0, 0.5, 2e-4)):
        want = href.rhs(N, L, nu, dt, theta, U, Q)
        assert_bits(hvref.rhs(N, L, nu, dt, theta, np.ones((N, N)), U, Q), want, f"N={N} theta={theta} a == 1")
        assert_bits(hvref.rhs(N, L, nu, dt, theta, None, U, Q), want, f"N={N} theta={theta} a = None")
    if theta == 1.0:   # a is not read: not even a NaN shows
        assert_bits(hvref.rhs(N, 1.0, 0.5, 2e-4, theta, np.full((N, N), np.nan), U, Q), want, "theta = 1 with a NaN coefficient")


@pytest.mark.parametrize("nu,dt", [(0.3, 1e-2), (1.0, 1e-4)])
@pytest.mark.parametrize("theta", [1.0, 0.75, 0.5])
@pytest.mark.parametrize("name", ["exp", "smooth"])
@pytest.mark.parametrize("N", [17, 33])
def test_one_step_against_the_direct_solution(oracle, N, name, theta, nu, dt):
    """_heat_vc_ref.check_one_step states the bound"""
    rtol = hvref.ONE_STEP_RTOL
    a, U0, Q = hvref.one_step_problem(N, name, 5 + N)
    F = hvref.rhs(N, 1.0, nu, dt, theta, a, U0, Q)
    U, hist, cycles, conv = hvref.step(oracle, a, U0, Q, 1.0, nu, dt, theta, rtol=rtol, max_cycles=80)
    assert conv
    hvref.check_one_step(a, U0, Q, U, F, 1.0, nu, dt, theta, rtol, f"N={N} a={name} theta={theta} nu={nu} dt={dt}, {cycles} cycles")


@pytest.mark.parametrize("N", [33, 65])
def test_perturbed_steady_state_decays(oracle, N):
    """_heat_vc_ref.Steady and check_steady state the problem and the bound"""
    p = hvref.Steady(N)
    s = hvref.STEADY
    Us, Fs = [p.U0], []
    for _ in range(s["steps"]):
        Fs.append(hvref.rhs(N, p.L, p.nu, p.dt, p.theta, p.a, Us[-1], p.Q))
        U, _, _, conv = hvref.step(oracle, p.a, Us[-1], p.Q, p.L, p.nu, p.dt, p.theta, rtol=s["rtol"])
        assert conv
        Us.append(U)
    hvref.check_steady(p, Us, Fs, s["rtol"], f"N={N}")
