"""The pure Neumann problem (include/mg_singular.h) on the GPU: the weighted mean, the shift and the projected coarse solve
alone, bit for bit against the restatement (tests/_singular_ref.py) and inside guard bands; whole singular solves against the
restatement, a bordered dense solve and the caller's own composition; dormancy on non-singular operators; refusals.  Bit
comparisons follow the qualification rule of DESIGN.md 4.3: the coarse margin of the restatement is asserted first."""
import numpy as np
import pytest

import _bc_ref as bref
import _guard
import _singular_forms_cases as cases
import _singular_ref as sref
import _solve_ref as ref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
LD = np.longdouble
U53 = ref.U53
BC = "nnnn"


def rtable(mg):
    return lambda N, M: mg.restriction_table(N, M)


def ptable(mg):
    return lambda M, N: mg.boundary_prolongation_table(M, N)


def _field(N, seed):
    """NaN-free random data with a mean well away from zero"""
    return np.random.default_rng(seed).random((N, N)) - 0.25


# ---------------------------------------------------------------- kernels alone, inside guard bands
@pytest.mark.parametrize("N", [3, 9, 33, 64, 127, 512, 514, 4096])
def test_weighted_mean_and_projection_alone(mg, N):
    """3, 9, 33: one column per lane; 64, 127: one column, even and odd N below PAIR_MIN_N; 512, 514: column pairs; 4096:
    non-temporal.  The mean and the projected field equal the restatement bit for bit, the sum lies inside its a-priori bound
    against longdouble, in place equals out of place, and only the output is written."""
    X = _field(N, 100 + N)
    want, m_want = sref.project_mean(X, 0.375)
    placement = "odd16" if N % 2 == 0 else "page"
    with _guard.block(mg, [N, N], placement) as gb:
        gX, gout = gb.views
        gX.upload(X)
        gout.poison()
        gb.expect_readonly(gX, gout)
        m = mg.weighted_mean(gX)
        gb.check(f"weighted_mean N={N}")
        m_ld = sref.weighted_mean_ld(X)
        bound = sref.gamma(N * N) * sref.weighted_mean_ld(np.abs(X)) + U53 * abs(m_ld)
        print(f"N={N}: mean {m!r}, |mean - longdouble| {float(abs(LD(m) - m_ld)):.3e} <= {float(bound):.3e}")
        assert m == sref.weighted_mean(X) == m_want
        assert abs(LD(m) - m_ld) <= bound

        gb.expect_readonly(gX)
        out, removed = mg.project_mean(gX, 0.375, out=gout, want_removed=True)
        gb.check(f"project_mean N={N}")
        assert out is gout and removed == m_want
        assert_bits(gout.to_host(), want, f"project_mean N={N}")

        gb.expect_readonly(gX)
        mg.project_mean(gout, 0.375, out=gout)               # in place, on the field that was just projected
        gb.check(f"project_mean in place N={N}")
        assert_bits(gout.to_host(), sref.project_mean(want, 0.375)[0], f"project_mean in place N={N}")
    if N <= 127:   # numpy in, numpy out
        assert_bits(mg.project_mean(X, 0.375), want, "numpy arrays")
        assert mg.weighted_mean(X) == m_want


def test_weighted_mean_and_projection_of_tensors(mg):
    torch = pytest.importorskip("torch")
    N = 514
    X = _field(N, 77)
    t = torch.from_numpy(X).cuda()
    want, m_want = sref.project_mean(X, -1.5)
    assert mg.weighted_mean(t) == m_want
    out = mg.project_mean(t, -1.5)
    torch.cuda.synchronize()
    assert_bits(out.cpu().numpy(), want, "tensor out of place")
    assert_bits(t.cpu().numpy(), X, "the input tensor")
    mg.project_mean(t, -1.5, out=t)
    torch.cuda.synchronize()
    assert_bits(t.cpu().numpy(), want, "tensor in place")


@pytest.mark.parametrize("name", [None, "smooth"])
@pytest.mark.parametrize("M", [8, 15, 16, 31, 32, 63])
def test_projected_coarse_solve_alone(mg, M, name):
    """U, the removed constant and the iteration count against the restatement, the stop qualified first; 63 fills the 1024
    lanes with 4 points each.  Then a zero right-hand side: zero in one pass."""
    L, atol, rtol, cap = 1.0, 0.0, 1e-2, 100000
    a = vref.field(name, M, L) if name else None
    F = _field(M, 300 + M)
    U_want, err0, errs, m_want = sref.rbgs_trace(M, L, a, F, atol, rtol, cap)
    ref.assert_qualified([vref.coarse_margin((U_want, err0, errs), atol, rtol)], f"M={M} a={name}")
    with _guard.block(mg, [M, M, M], "page" if M % 2 else "odd16") as gb:
        ga, gF, gout = gb.views
        ga.upload(a if name else np.ones((M, M))), gF.upload(F)
        gout.poison()
        gb.expect_readonly(ga, gF)
        removed, iters = mg.coarseSolveMean(M, L, BC, ga if name else None, gF, atol, rtol, cap, gout)
        gb.check(f"coarseSolveMean M={M} a={name}")
        print(f"M={M} a={name}: {iters} iterations, removed {removed!r}")
        assert removed == m_want and iters == len(errs)
        assert_bits(gout.to_host(), U_want, f"coarseSolveMean M={M} a={name}")
        gF.upload(np.zeros((M, M)))
        gout.poison()
        removed, iters = mg.coarseSolveMean(M, L, BC, ga if name else None, gF, atol, rtol, cap, gout)
        assert removed == 0.0 and iters == 1
        assert_bits(gout.to_host(), np.zeros((M, M)), "zero right-hand side")
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        g = mg.DeviceGrid.zeros((M, M))
        mg.coarseSolveMean(M, L, "nnnd", None, g, atol, rtol, cap, g.copy())


# ---------------------------------------------------------------- whole solves against the restatement
def _restated(mg, N, name, mean=0.0, seed=0, **opts):
    return cases.restated(N, name, mean, 8000 + N + seed, rtable(mg), ptable(mg), **opts)


def _compare(mg, case, mean=0.0, **opts):
    F, U0, a, U, hist, k, conv, info = case
    N = F.shape[0]
    gF = mg.DeviceGrid.from_host(F)
    s = mg.Solver(N, 1.0, coef=a, mean=mean, bc=BC, **opts)
    assert s.mean == mean and s.boundary == (1, 1, 1, 1)
    got, ginfo = s.solve(gF, U0)
    again, ainfo = s.solve(gF, U0)
    s.close()
    assert_bits(gF.to_host(), F, "F is read only")
    gF.free()
    print(f"N={N}: {ginfo['cycles']} cycles, compat_defect {ginfo['compat_defect']!r}, mean_before {ginfo['mean_before']!r}")
    assert ginfo["cycles"] == k and ginfo["converged"] == conv
    assert ginfo["compat_defect"] == info["compat_defect"] and ginfo["mean_before"] == info["mean_before"] and ginfo["mean"] == mean
    assert_bits(got, U, f"N={N}: U")
    np.testing.assert_allclose(ginfo["history"], hist, rtol=1e-12, atol=0.0)
    rn = bref.ref_norm(info["Ft"], BC)
    assert abs(ginfo["ref_norm"] - rn) <= 1e-12 * rn
    assert_bits(again, got, "two runs")
    assert ainfo["history"] == ginfo["history"] and ainfo["compat_defect"] == ginfo["compat_defect"]
    m_ld = sref.weighted_mean_ld(got)
    assert abs(m_ld - LD(mean)) <= sref.gamma(N * N) * sref.weighted_mean_ld(np.abs(got)) + 2 * U53 * abs(mean)
    return got, ginfo


@pytest.mark.parametrize("pp", [(3, 3), (2, 1)])
@pytest.mark.parametrize("name", ["one", "smooth"])
@pytest.mark.parametrize("N", [33, 64, 65, 257])
def test_whole_solves_bit_identical_to_restatement(mg, N, name, pp):
    opts = dict(pre=pp[0], post=pp[1], rtol=1e-9)
    _compare(mg, _restated(mg, N, name, **opts), **opts)


def test_whole_solve_with_the_largest_coarsest_level(mg):
    """N_min = 32, N = 126 -> 63: the coarse solve with every lane owning four points"""
    opts = dict(N_min=32, rtol=1e-6)
    _compare(mg, _restated(mg, 126, "smooth", **opts), **opts)


def test_whole_solve_with_a_mean(mg):
    opts = dict(rtol=1e-9)
    got, info = _compare(mg, _restated(mg, 65, "smooth", mean=2.5, **opts), mean=2.5, **opts)
    assert abs(info["mean_before"] - 2.5) > 1e-3   # (the shift did something)


def test_against_the_bordered_dense_solution(mg):
    """N = 33: max|U - X| <= ||B||_inf * (||r(U)||_inf + ||r(X)||_inf) + the two gauges' rounding, X the solution of
    [[A, 1], [w^T/sw, 0]] [X; lam] = [F; mean] assembled in longdouble, B the U-from-F block of its inverse"""
    N, L, mean = 33, 1.0, -0.5
    F, U0 = ref.random_problem(N, 8600)
    F = F + 0.25
    a = vref.field("smooth", N, L)
    U, info = mg.solve(F, U0, L, coef=a, bc=BC, mean=mean, rtol=1e-11)
    assert info["converged"], info["cycles"]
    X, lam, nB = sref.bordered_solution(a, F, L, mean)
    A, _ = bref.dense_operator(a, N, L, 0.0, BC)
    rhs = np.asarray(F, dtype=LD).reshape(-1) - lam
    rU, rX = A @ U.astype(LD).reshape(-1) - rhs, A @ X.reshape(-1) - rhs
    gauge = abs(sref.weighted_mean_ld(U) - LD(mean)) + abs(sref.weighted_mean_ld(X) - LD(mean))
    err = np.max(np.abs(U.astype(LD) - X))
    bound = (nB * (np.max(np.abs(rU)) + np.max(np.abs(rX))) + gauge) * (1 + LD(1e-6))
    print(f"{info['cycles']} cycles, |U-X| {float(err):.3e} <= {float(bound):.3e}, lam {float(lam):.6e} vs {info['compat_defect']:.6e}")
    assert err <= bound
    assert abs(LD(info["compat_defect"]) - lam) <= 1e-12 * abs(lam)


@pytest.mark.parametrize("N,k", cases.COMPOSITION_CASES)
def test_bit_identical_to_the_callers_own_composition(mg, N, k):
    """project_mean(F), then k cycles of the boundary path made of its own building blocks with the projected coarse solve, then
    project_mean(U): the solve's bits.  The cycles are composed from the hooks because a second run of the singular solver on
    the projected Ft would project it again, by a constant at rounding level, and change the last bits of small entries.
    33: one column per lane on every level; 514 and 1026: a pair level on top of an odd one; 4096: the non-temporal form, where
    the restatement takes 14 s per cycle on the host and this is the whole-solve bit check (every hook used here is held to the
    restatement alone at 4096 by test_bc_forms_gpu.py and test_weighted_mean_and_projection_alone)."""
    L, mean = 1.0, 1.25
    o = dict(sref.DEFAULTS)
    F, U0 = ref.random_problem(N, 8700)
    F = F + 0.5
    a = vref.field("smooth", N, L)
    want, info = mg.solve(F, U0, L, coef=a, bc=BC, mean=mean, rtol=0.0, max_cycles=k)
    assert info["cycles"] == k

    sz = ref.sizes(N, o["N_min"])
    nl = len(sz)
    G = lambda n: mg.DeviceGrid((n, n))
    A = [mg.DeviceGrid.from_host(a)] + [G(n) for n in sz[1:]]
    for l in range(nl - 1):
        mg.coarsenCoefficient(sz[l], A[l], sz[l + 1], A[l + 1])
    gF = mg.DeviceGrid.from_host(F)
    Fs = [mg.project_mean(gF)] + [G(n) for n in sz[1:]]
    Us, Ts, D = [G(n) for n in sz], [G(n) for n in sz], [G(n) for n in sz]
    U = gU0 = mg.DeviceGrid.from_host(U0)

    def sweeps(l, first, count):
        """count sweeps on level l starting from `first` (None: zero); returns the grid holding the result"""
        src, dst = first, (Ts[l] if first is Us[l] else Us[l])
        for _ in range(count):
            mg.sweepBoundary(sz[l], L, 0.0, o["omega"], BC, A[l], src, Fs[l], dst)
            src, dst = dst, (Us[l] if dst is Ts[l] else Ts[l])
        return src

    for _ in range(k):
        cur = [None] * nl
        for l in range(nl - 1):
            cur[l] = sweeps(l, U if l == 0 else None, o["pre"])
            mg.residualBoundary(sz[l], L, 0.0, BC, A[l], cur[l], Fs[l], D[l], -1)
            mg.restrictBoundary(sz[l], BC, D[l], sz[l + 1], Fs[l + 1])
        mg.coarseSolveMean(sz[-1], L, BC, A[-1], Fs[-1], o["coarse_atol"], o["coarse_rtol"], o["coarse_max_iters"], Us[-1])
        cur[-1] = Us[-1]
        for l in range(nl - 2, -1, -1):
            other = Ts[l] if cur[l] is Us[l] else Us[l]
            mg.prolongAddBoundary(sz[l + 1], BC, cur[l + 1], sz[l], cur[l], other)
            cur[l] = sweeps(l, other, o["post"])
        U = cur[0]
    gout = mg.project_mean(U, mean)
    got = gout.to_host()
    for g in A + Fs + Us + Ts + D + [gF, gU0, gout]:
        g.free()
    assert_bits(got, want, f"N={N}: the caller's own composition")


# ---------------------------------------------------------------- dormancy and refusals
@pytest.mark.parametrize("bc,shift", [("ndnd", 0.0), ("nnnn", 1e2)])
def test_dormant_on_a_non_singular_operator(mg, bc, shift):
    N = 100
    F, U0 = ref.random_problem(N, 8800)
    a = vref.field("smooth", N)
    opts = dict(rtol=0.0, max_cycles=3, shift=shift)
    plain = mg.Solver(N, 1.0, coef=a, bc=bc, **opts)
    want, winfo = plain.solve(F, U0)
    plain.close()
    s = mg.Solver(N, 1.0, coef=a, mean=2.0, bc=bc, **opts)
    got, ginfo = s.solve(F, U0)
    assert_bits(got, want, f"{bc} shift={shift}: dormant")
    assert ginfo["history"] == winfo["history"] and "compat_defect" not in ginfo
    s.set_mean(None)                                          # not singular: switching it off is allowed
    assert s.mean is None
    got, ginfo = s.solve(F, U0)
    assert_bits(got, want, "after set_mean(None)")
    s.close()


def test_four_dirichlet_sides_restore_the_plain_solver(mg):
    N = 64
    F, U0 = ref.random_problem(N, 8900)
    opts = dict(rtol=0.0, max_cycles=2)
    plain = mg.Solver(N, 1.0, **opts)
    want, winfo = plain.solve(F, U0)
    plain.close()
    s = mg.Solver(N, 1.0, mean=0.0, bc=BC, **opts)
    other, oinfo = s.solve(F, U0)
    assert "compat_defect" in oinfo and not np.array_equal(other, want)
    s.set_boundary("dddd")
    got, ginfo = s.solve(F, U0)
    assert_bits(got, want, "set_boundary('dddd') restores the plain solver")
    assert ginfo["history"] == winfo["history"] and "compat_defect" not in ginfo
    s.close()


def test_refusals_leave_the_solver_as_it_was(mg):
    N = 64
    F, U0 = ref.random_problem(N, 9000)
    opts = dict(rtol=0.0, max_cycles=1)

    def refused(s, code, call, match=""):
        want, winfo = s.solve(F, U0)
        kinds, mean = s.boundary, s.mean
        with pytest.raises(mg.MGError, match=r"\[%d\].*%s" % (code, match)):
            call()
        assert s.boundary == kinds and s.mean == mean
        got, ginfo = s.solve(F, U0)
        assert_bits(got, want, "the solver solves as before the refusal")
        assert ginfo["history"] == winfo["history"]

    s = mg.Solver(N, 1.0, **opts)
    refused(s, 3, lambda: s.set_boundary(BC), "singular")    # without the opt-in: as before
    refused(s, 2, lambda: s.set_mean(float("nan")))
    s.set_mean(1.0)
    s.set_boundary(BC)
    refused(s, 3, lambda: s.set_mean(None), "singular")       # switching off while singular
    refused(s, 3, lambda: s.set_krylov(4), "Krylov")
    refused(s, 3, lambda: s.adjoint(np.ones((N, N)), U0), "adjoint")
    s.set_mean(-3.0)                                          # another target stays allowed
    assert s.mean == -3.0
    s.set_boundary("ndnd")
    s.set_mean(None)
    refused(s, 3, lambda: s.set_boundary(BC), "singular")
    s.close()
    s = mg.Solver(N, 1.0, fmg=1, mean=0.0, **opts)
    refused(s, 3, lambda: s.set_boundary(BC), "fmg")
    s.close()
    s = mg.Solver(N, 1.0, krylov=4, mean=0.0, **opts)
    refused(s, 3, lambda: s.set_boundary(BC), "Krylov")
    s.close()
    assert mg.lib().mg_solver_set_mean(None, 1, 0.0) == 2
    with pytest.raises(mg.MGError, match=r"\[2\]"):
        mg._check()
    assert mg.lib().mg_solver_mean(None, None) == 0
