"""exp_libm (csrc/mg_exp_libm.h) as the semilinear pass evaluates it (csrc/mg_newton_impl.h), over its whole value domain and
in every kernel form, on the GPU.  The route: mg.nonlinear_residual in the no-step form with kind="exp", kappa = 1, no weight,
no coefficient, shift 0 and F = 0 writes S = 1.0*e at every point, rim included, so S IS exp_libm(U).  The arguments, the
longdouble reference and the ulp measure are tests/_exp_cases.py's (checked by tests/test_newton_exp_domain_cpu.py).

Sizes: 258 (one column per lane, second column block), 514 and 1026 (column pairs) and 4096 (column pairs with non-temporal
accesses: the pass takes that form from its own constant NT_MIN_N = 4096 on, not from MG_NT_MIN_N, which governs the cycle's
streaming nodes only -- so 1026 is a second pair size and 4096 is here for the third form).

(a) accuracy against the reference, never skipped; (b) bits against the host libm where the engine's self-check vouches for it,
and the forms against one another always; (c) the device library's branch |x| >= 512 by class and within 2 ulp; (d) sinh;
(e) special values with coefficient and weight present, inside guard bands; (f) the batched pass; (g) a solve whose solution
lies below -512."""
import math

import numpy as np
import pytest

import _exp_cases as xc
import _guard
import _newton_ref as nref
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
LD = np.longdouble
U53 = LD(2) ** -53                       # the unit roundoff of a double
SIZES = [258, 514, 1026]                 # the sizes of every case
FORMS = SIZES + [4096]                   # and the non-temporal form, for the cases that run exp_libm alone
MARGIN_ULP = 0.01                        # (a): the device's largest error may exceed the host libm's by this much
R3_BOUND_ULP = 2.0                       # (c): HIP documents 1 ulp for exp(double); the solver needs class and magnitude


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def exp_bits_hold(mg):
    return mg.lib().mg_source_is_bit_identical() == 1


# ---------------------------------------------------------------- the route, and what the tests share
def run_pass(mg, N, U, kind="exp"):
    """(D, S) of the no-step pass on the field U with kappa = 1, w = 1, a = 1, shift 0, F = 0, and the norm"""
    G = mg.DeviceGrid
    gU, gF, gD, gS = G.from_host(U), G.zeros((N, N)), G((N, N)), G((N, N))
    try:
        with np.errstate(all="ignore"):
            norm = mg.nonlinear_residual(N, 1.0, 0.0, None, kind, 1.0, None, gU, gF, gD, gS)
        return gD.to_host(), gS.to_host(), norm
    finally:
        for g in (gU, gF, gD, gS):
            g.free()


def through_the_pass(mg, N, values, kind="exp"):
    """S at the points that hold `values`, laid out over as many N x N fields as it takes; every repeat that pads a field must
    hold the bits of the point it repeats"""
    out = np.empty(values.size)
    for start in xc.calls(values, N):
        U, n = xc.field(values, N, start)
        S = run_pass(mg, N, U, kind)[1].reshape(-1)
        assert np.array_equal(bits(S), bits(np.resize(S[:n], N * N))), f"N={N} {kind}: a repeated argument gave other bits"
        out[start:start + n] = S[:n]
    return out


_shared = {}


def verified_path():
    """x (R2 then R1), the reference, the host libm's values and its largest error: computed once, never changed"""
    if "ref" not in _shared:
        x = np.concatenate([xc.r2(), xc.r1()])
        true = xc.exp_ref(x)
        host = xc.host_exp(x)
        err = xc.ulp_error(host, true)
        for a in (x, true, host):
            a.setflags(write=False)
        _shared["ref"] = (x, true, host, float(np.max(err)))
    return _shared["ref"]


def device_exp(mg, N):
    """exp_libm on the whole of R2 and R1 in the form of size N, once per session"""
    if ("dev", N) not in _shared:
        got = through_the_pass(mg, N, verified_path()[0])
        got.setflags(write=False)
        _shared[("dev", N)] = got
    return _shared[("dev", N)]


def error_bound_ulp():
    """what (a) holds the device to on |x| < 512, in ulp: the host libm's own largest error by the reference plus the margin.
    The sinh bounds of (d) start from it."""
    return verified_path()[3] + MARGIN_ULP


# ---------------------------------------------------------------- (a) accuracy, (b) bits
@pytest.mark.parametrize("N", FORMS)
def test_a_accuracy_against_the_longdouble_reference(mg, N):
    """R2 and R1 through the pass: the device's largest error against the longdouble reference is at most the host libm's
    largest error on the same arguments, by the same reference, plus 0.01 ulp (twenty times the reference's own error; room
    for a host whose libm is not glibc's).  Measured on an MI355X against glibc 2.35: device 0.5054 ulp, host 0.5054 ulp in
    every form."""
    x, true, host, host_max = verified_path()
    got = device_exp(mg, N)
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    err = xc.ulp_error(got, true)
    i = int(np.argmax(err))
    print(f"N={N}: {x.size} arguments, device exp_libm largest error {float(err[i]):.4f} ulp at x = {x[i]!r}; "
          f"host libm {host_max:.4f} ulp")
    assert float(err[i]) <= host_max + MARGIN_ULP, (N, float(err[i]), host_max, x[i])
    # the 1.0 + x branch: exactly 1 below 2^-54 (the sum rounds to 1, ties to even included)
    r1 = got[-xc.r1().size:]
    assert np.all(r1 == 1.0), r1


@pytest.mark.parametrize("N", FORMS)
def test_b_bits_of_the_host_libm_where_the_self_check_vouches_for_them(mg, N):
    if not exp_bits_hold(mg):
        pytest.skip("exp_libm does not reproduce this host's libm bit for bit (mg_source_is_bit_identical() != 1)")
    host = verified_path()[2]
    assert_bits(device_exp(mg, N), host, f"N={N}: exp_libm against math.exp on R2 and R1")


@pytest.mark.parametrize("N", FORMS)
def test_b_bits_of_the_restated_algorithm_on_every_host(mg, N):
    """never skipped: exp_libm restated operation by operation with the C library's fma (tests/_exp_cases.py), which does not
    go through any libm's exp().  What (a)'s 0.01 ulp cannot see -- one fused multiply-add split into a product and a sum moves
    the largest error by 0.0014 ulp at the most, the last bit of a polynomial constant by less -- changes bits here."""
    if "restated" not in _shared:
        _shared["restated"] = xc.exp_libm_restated(verified_path()[0])
        _shared["restated"].setflags(write=False)
    assert_bits(device_exp(mg, N), _shared["restated"], f"N={N}: exp_libm against its restatement on R2 and R1")


def test_b_the_three_forms_agree_bit_for_bit(mg):
    first = device_exp(mg, FORMS[0])
    for N in FORMS[1:]:
        assert_bits(device_exp(mg, N), first, f"exp_libm at N={N} against N={FORMS[0]}")


# ---------------------------------------------------------------- (c) beyond the verified path
def check_r3_classes(x, got, what):
    """+inf above the overflow threshold, +0 from -746 down, NaN for NaN; returns the mask of the finite class"""
    x, got = np.asarray(x), np.asarray(got)
    over, zero, nan = np.isin(x, xc.R3_OVER), np.isin(x, xc.R3_ZERO), np.isnan(x)
    assert np.all(got[over] == math.inf), (what, x[over], got[over])
    assert np.all(got[zero] == 0.0) and not np.any(np.signbit(got[zero])), (what, x[zero], got[zero])
    assert np.all(np.isnan(got[nan])), (what, got[nan])
    fin = ~(over | zero | nan)
    assert np.all(np.isfinite(got[fin])) and np.all(got[fin] >= 0.0) and not np.any(np.signbit(got[fin])), (what, x[fin], got[fin])
    return fin


@pytest.mark.parametrize("N", FORMS)
def test_c_the_device_librarys_branch_by_class_and_within_two_ulp(mg, N):
    """|x| >= 512, where exp_libm hands over to the device library's exp(): the classes exactly; finite results, normal and
    subnormal (an error is counted in the subnormal spacing there), within 2 ulp of the reference.  Measured on an MI355X:
    0.4984 ulp at the most (x = -745.13, result 5e-324; -745.14 gives +0, 0.4966 ulp: both correctly rounded), so below 1 ulp,
    in every form."""
    x = xc.r3()
    got = through_the_pass(mg, N, x)
    fin = check_r3_classes(x, got, f"N={N}")
    err = xc.ulp_error(got[fin], xc.exp_ref(x[fin]))
    for v, g, e in zip(x[fin], got[fin], err):
        print(f"N={N}: exp({v!r}) = {g!r}  ({float(e):.4f} ulp)")
    print(f"N={N}: largest error beyond the verified path {float(np.max(err)):.4f} ulp")
    assert float(np.max(err)) <= R3_BOUND_ULP
    sub = np.isin(x, xc.R3_SUBNORMAL)
    assert np.all(got[sub] < 2.0 ** -1022)
    assert got[x == -708.4][0] > 0.0


# ---------------------------------------------------------------- (d) sinh
def sinh_bounds(v, e_ulp):
    """The absolute bounds on g = 0.5*(e - f) against sinh v and on g' = 0.5*(e + f) against cosh v, f = 1.0/e, longdouble.

    e = e^v (1 + d1) with |d1| <= eta(v) = e_ulp * spacing(e^v) / e^v, the error (a) or (c) allows exp_libm in ulp, taken
    relative (spacing / value <= 2^-52; more where e^v is subnormal).  The division rounds once (u = 2^-53):
    f = e^-v (1 + d2)/(1 + d1), so |f - e^-v| <= (eta + u) e^-v (1 + 2 eta), plus 2^-1074 where f is subnormal.  The difference
    (the sum) rounds once more; the halving is exact, g and g' being normal numbers for |v| >= 2^-54:
        |g  - sinh v| <= 0.5 (|e - e^v| + |f - e^-v|) (1 + u) + u |sinh v| <= (eta + 2u) cosh v (1 + 4 eta) + 2^-1074
        |g' - cosh v| <= the same.
    At small |v| the two terms of the difference cancel and the bound does not shrink with sinh v: it is ABSOLUTE, about
    (2 * 0.516 + 2) * 2^-53 = 1.5 * 2^-52 times cosh v, not relative to sinh v.  The factor 1 + 2^-10 covers the reference's own
    error (longdouble sinh / cosh: 2^-63 relative to cosh v, 2^-11 of this bound)."""
    v = np.asarray(v, dtype=np.float64)
    true = xc.exp_ref(v)
    eta = LD(e_ulp) * xc.spacing(true) / true
    c = np.cosh(v.astype(LD))
    return (eta + 2 * U53) * c * (1 + 4 * eta) * (1 + LD(2) ** -10) + LD(2) ** -1074


def sinh_sample():
    """the arguments whose g is recovered from D (constant 3 x 3 patches; (258 // 3)^2 = 7396 of them fit the smallest size):
    the edges of R2, every 20th of the log-uniform magnitudes of both signs -- the small |v| where the difference cancels --
    and every 457th of the per-k arguments (457 is odd and prime to 128: every table index and both tie edges occur)"""
    x = xc.r2()
    n_k = x.size - 2 * xc.N_LOG - len(xc.R2_EDGES)
    assert n_k > 0 and np.all(x[-len(xc.R2_EDGES):] == np.array(xc.R2_EDGES))
    out = np.concatenate([np.array(xc.R2_EDGES), x[n_k:n_k + 2 * xc.N_LOG:20], x[:n_k:457]])
    assert out.size <= (SIZES[0] // 3) ** 2
    return out


@pytest.mark.parametrize("N", SIZES)
def test_d_sinh_on_the_verified_path(mg, N):
    """kind = "sinh" on all of R2.  S = g' against cosh on every argument, within sinh_bounds (the derivation is there);
    under the condition of (b), S and the interior of D are nref.residual's bit for bit.  g against sinh at sinh_sample(), where
    the field is constant over 3 x 3 patches: the stencil term of D is exactly zero there (asserted on the restated operator),
    so D = (0 + 1.0*g) - 0 = g."""
    x = xc.r2()
    bound = sinh_bounds(x, error_bound_ulp())
    worst = LD(0)
    for start in xc.calls(x, N):
        U, n = xc.field(x, N, start)
        D, S, norm = run_pass(mg, N, U, "sinh")
        err = np.abs(S.reshape(-1)[:n].astype(LD) - np.cosh(x[start:start + n].astype(LD)))
        worst = max(worst, np.max(err / bound[start:start + n]))
        assert np.all(err <= bound[start:start + n]), f"N={N}: g' = 0.5*(e + 1/e) outside its bound against cosh"
        if exp_bits_hold(mg):
            _, wD, wS, wnorm = nref.residual(N, 1.0, None, "sinh", 1.0, None, U, np.zeros((N, N)))
            assert_bits(S, wS, f"N={N} sinh, R2 from {start}: S")
            assert_bits(D, wD, f"N={N} sinh, R2 from {start}: D")
            assert norm == wnorm
    xs = sinh_sample()
    U, rows, cols = xc.patches(xs, N)
    lin = vref.apply_operator(N, 1.0, None, U, 0.0)
    assert np.all(lin[rows, cols] == 0.0), "the stencil term at the patch centres is not exactly zero"
    D, S, _ = run_pass(mg, N, U, "sinh")
    g, gp = D[rows, cols], S[rows, cols]
    b = sinh_bounds(xs, error_bound_ulp())
    eg = np.abs(g.astype(LD) - np.sinh(xs.astype(LD)))
    ep = np.abs(gp.astype(LD) - np.cosh(xs.astype(LD)))
    print(f"N={N} sinh: g' on {x.size} arguments at most {float(worst):.3f} of its bound; at the {xs.size} patch centres g "
          f"{float(np.max(eg / b)):.3f}, g' {float(np.max(ep / b)):.3f} of the bound")
    assert np.all(eg <= b) and np.all(ep <= b)
    far = np.abs(xs) >= 2.0 ** -50                 # (below, g may round to 0 inside its bound: e = f = 1.0 at |v| = 2^-54)
    assert np.all(np.sign(g[far]) == np.sign(xs[far]))


@pytest.mark.parametrize("N", SIZES)
def test_d_sinh_beyond_the_verified_path(mg, N):
    """kind = "sinh" on R3 in constant patches.  |v| >= 710: g' = +inf, and g = +-inf where the stencil term is finite (up to
    |v| = 746; at 1e308 and inf it is inf - inf and D is NaN, as in the restatement).  512 <= |v| <= 709.78...: g and g' within
    sinh_bounds at the 2 ulp of (c).  NaN gives NaN."""
    x = xc.r3()
    U, rows, cols = xc.patches(x, N)
    D, S, _ = run_pass(mg, N, U, "sinh")
    g, gp = D[rows, cols], S[rows, cols]
    with np.errstate(all="ignore"):
        _, wD, wS, _ = nref.residual(N, 1.0, None, "sinh", 1.0, None, U, np.zeros((N, N)))
    big = np.abs(x) >= 710.0
    assert np.all(gp[big] == math.inf), (x[big], gp[big])
    near = big & (np.abs(x) <= 746.0)              # 710, -745.13, -745.14 (e is 5e-324 or 0: f = 1/e = +inf either way), -746
    assert near.sum() == 4 and np.all(g[near] == np.copysign(math.inf, x[near])), (x[near], g[near])
    assert np.all(np.isnan(g[np.isnan(x)])) and np.all(np.isnan(gp[np.isnan(x)]))
    # position and class of everything that is not finite: the restatement's
    for got, want, name in ((D, wD, "D"), (S, wS, "S")):
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]) and np.array_equal(np.isinf(got), np.isinf(want)), name
    fin = np.abs(x) <= xc.EXP_MAX
    assert fin.sum() == 8
    b = sinh_bounds(x[fin], R3_BOUND_ULP)
    eg = np.abs(g[fin].astype(LD) - np.sinh(x[fin].astype(LD)))
    ep = np.abs(gp[fin].astype(LD) - np.cosh(x[fin].astype(LD)))
    print(f"N={N} sinh beyond 512: g {float(np.max(eg / b)):.3f}, g' {float(np.max(ep / b)):.3f} of the bound")
    assert np.all(eg <= b) and np.all(ep <= b)


# ---------------------------------------------------------------- (e) special values, coefficient and weight present
def special_inputs(N, which):
    """U of order one, a step of order 100 for t = 2^-9, a random coefficient, a weight over six decades with exact zeros, and
    the special values `which`: "all" -- an interior NaN, an interior 710 with w > 0, an interior 710 with w == 0 (e = inf times
    a weight of exactly 0) and a rim 710; "inf" -- the interior 710 with w > 0 alone; "rim" -- the rim 710 alone, w == 0 there"""
    rng = np.random.default_rng(90 + N)
    U = 2.0 * rng.random((N, N)) - 1.0
    dlt = 100.0 * rng.standard_normal((N, N))
    w = 10.0 ** (6.0 * rng.random((N, N)) - 3.0)
    w[::3, ::5] = 0.0
    F = 50.0 * rng.standard_normal((N, N))
    a = vref.field("random", N, seed=N)
    m = N // 2
    p_nan, p_inf, p_inf0, p_rim = (m, m - 3), (m + 2, m + 1), (N - 3, 2), (0, N - 4)     # (far enough apart: no shared neighbour)
    w[p_inf], w[p_inf0], w[p_rim] = 2.5, 0.0, 0.0
    if which == "all":
        U[p_nan], U[p_inf], U[p_inf0], U[p_rim] = math.nan, 710.0, 710.0, 710.0
        dlt[p_nan] = dlt[p_inf] = dlt[p_inf0] = 0.0                                       # (the step form leaves them in place)
    elif which == "inf":
        U[p_inf] = 710.0
        dlt[p_inf] = 0.0
    else:
        U[p_rim] = 710.0
    return U, dlt, w, F, a, dict(nan=p_nan, inf=p_inf, inf0=p_inf0, rim=p_rim)


def assert_same_classes_and_finite_bits(got, want, exact, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN at other points"
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), f"{what}: inf at other points or of other sign"
    fin = np.isfinite(want)
    if exact:
        assert np.array_equal(bits(got[fin]), bits(want[fin])), f"{what}: finite values differ by bits"
    else:
        # a host whose libm is not the device's: two correctly-ish rounded exps differ by an ulp or two of e, which enters S
        # and D linearly -- 2^-50 of the array's largest finite magnitude bounds that with room
        tol = 2.0 ** -50 * np.max(np.abs(want[fin]))
        assert np.all(np.abs(got[fin] - want[fin]) <= tol), f"{what}: finite values differ by more than {tol}"


@pytest.mark.parametrize("kind", ["sinh", "exp"])
@pytest.mark.parametrize("N", [17, 514, 1026])
def test_e_special_values_in_the_pass_with_coefficient_and_weight(mg, N, kind):
    """NaN, an overflowing 710 inside and on the rim, and 0 * inf, through both forms of the pass inside guard bands: position
    and class of every non-finite value of V, D, S are the restatement's, everything finite is the restatement's bit for bit
    (where the self-check vouches for exp's bits; to 2^-50 of the array's scale otherwise), the norm is NaN, inf or finite
    as the restatement's -- finite with the rim 710 alone, since the rim enters S only."""
    L, shift, kappa, t = 1.0, 0.0, 3.7, 2.0 ** -9
    exact = exp_bits_hold(mg)
    with _guard.block(mg, [N] * 8, "odd16" if N % 4 == 2 else "page") as gb:
        ga, gw, gU, gdlt, gF, gV, gD, gS = gb.views
        for which, steps, norm_is in (("all", (False, True), math.isnan), ("inf", (False,), math.isinf), ("rim", (False, True), math.isfinite)):
            U, dlt, w, F, a, at = special_inputs(N, which)
            ga.upload(a), gw.upload(w), gU.upload(U), gdlt.upload(dlt), gF.upload(F)
            for step in steps:
                what = f"N={N} {kind} {which} step={step}"
                gV.poison(), gD.poison(), gS.poison()
                gb.expect_readonly(*([ga, gw, gU, gdlt, gF] + ([] if step else [gV])))
                norm = mg.nonlinear_residual(N, L, shift, ga, kind, kappa, gw, gU, gF, gD, gS, dlt=gdlt if step else None, t=t,
                                             V=gV if step else None)
                gb.check(what)
                with np.errstate(all="ignore"):
                    wV, wD, wS, wnorm = nref.residual(N, L, a, kind, kappa, w, U, F, shift, dlt if step else None, t)
                D, S = gD.to_host(), gS.to_host()
                if step:
                    assert_same_classes_and_finite_bits(gV.to_host(), wV, True, what + ": V")
                assert_same_classes_and_finite_bits(D, wD, exact, what + ": D")
                assert_same_classes_and_finite_bits(S, wS, exact, what + ": S")
                assert norm_is(norm) and norm_is(wnorm), (what, norm, wnorm)
                if math.isfinite(wnorm):
                    assert norm == wnorm if exact else abs(norm - wnorm) <= 2.0 ** -50 * wnorm, (what, norm, wnorm)
                else:
                    assert norm == wnorm or (math.isnan(norm) and math.isnan(wnorm)), (what, norm, wnorm)
                # what the special points themselves must show, whatever the restatement says
                if which == "all":
                    assert math.isnan(S[at["nan"]]) and math.isnan(D[at["nan"]])
                    assert S[at["inf"]] == math.inf and D[at["inf"]] == math.inf
                    assert math.isnan(S[at["inf0"]]) and math.isnan(D[at["inf0"]])       # 0 * inf
                    assert math.isnan(S[at["rim"]]) and D[at["rim"]] == 0.0               # 0 * inf on the rim; D's rim is +0
                    assert np.isnan(S).sum() == 3 and np.isinf(S).sum() == 1
                elif which == "inf":
                    assert S[at["inf"]] == math.inf and D[at["inf"]] == math.inf and np.isinf(D).sum() == 1 and not np.isnan(D).any()
                else:
                    assert math.isnan(S[at["rim"]]) and np.isnan(S).sum() == 1 and np.all(np.isfinite(D))


# ---------------------------------------------------------------- (f) the batched twin
@pytest.mark.parametrize("kind", ["exp", "sinh"])
@pytest.mark.parametrize("N", SIZES)
def test_f_batched_pass_on_the_whole_domain_equals_the_single_pass(mg, N, kind):
    """two instances in one launch, the first slice of R2 and the R3 field, in both forms: V, D, S and the norm of each are the
    single pass's bit for bit, NaN and inf included (device against device: the same bits, payloads too)"""
    G = mg.DeviceGrid
    rng = np.random.default_rng(N)
    fields = [xc.field(xc.r2(), N)[0], xc.field(xc.r3(), N)[0]]
    dlts = [rng.standard_normal((N, N)) for _ in fields]
    gU, gdlt = [G.from_host(u) for u in fields], [G.from_host(d) for d in dlts]
    gF = [G.zeros((N, N)) for _ in fields]
    outs = [[G((N, N)) for _ in range(3)] for _ in fields]
    one = [G((N, N)) for _ in range(3)]
    t = 0.25
    try:
        for step in (False, True):
            norms = mg.nonlinear_residual_batch(N, 1.0, 0.0, None, kind, 1.0, None, gU, gF, [o[1] for o in outs], [o[2] for o in outs],
                                                dlt=gdlt if step else None, t=t, V=[o[0] for o in outs] if step else None)
            for i in range(2):
                norm = mg.nonlinear_residual(N, 1.0, 0.0, None, kind, 1.0, None, gU[i], gF[i], one[1], one[2],
                                             dlt=gdlt[i] if step else None, t=t, V=one[0] if step else None)
                what = f"N={N} {kind} step={step} instance {i}"
                assert norms[i] == norm or (math.isnan(norms[i]) and math.isnan(norm)), (what, norms[i], norm)
                for j, name in enumerate("VDS"):
                    if name != "V" or step:
                        assert_bits(outs[i][j].to_host(), one[j].to_host(), f"{what}: {name}")
            assert math.isnan(norms[1])            # (the R3 field's NaN repeats into the interior)
    finally:
        for g in gU + gdlt + gF + one + [x for o in outs for x in o]:
            g.free()


# ---------------------------------------------------------------- (g) a solve that lives beyond -512
G_SOURCE = 1e4   # Laplace(U) - e^U = +1e4 with zero rim data: U has its minimum near -1e4 * 0.0737 = -737


@pytest.mark.parametrize("N", [33, 514])
def test_g_a_solve_whose_solution_lies_below_minus_512(mg, N):
    """F == +1e4, kind = "exp", kappa = 1 from U = 0: the solution's minimum is about -737, so accepted trials evaluate exp
    through the device library's branch, into subnormal results (e^-737 = 1e-320).  The solve converges and min U < -512 (asserted:
    the case must not stop reaching the branch unnoticed).  The restatement (tests/_newton_ref.py on the CPU, N = 33) converges
    on this input with the default options in 2 iterations, no backtrack, min U = -736.147.  At N = 33 U is held against the
    dense longdouble Newton solution by max|U - X| <= ||A^-1||_inf * (||N(U)||_inf + ||N(X)||_inf)."""
    F = np.full((N, N), G_SOURCE)
    U, info = mg.solve_semilinear(F, kind="exp", kappa=1.0)
    print(f"N={N}: {info['iterations']} iterations, backtracks {[s['backtracks'] for s in info['steps']]}, min U {U.min()!r}, "
          f"history {info['history']}")
    assert info["converged"] and info["status"] == nref.CONVERGED and info["iterations"] <= 20, info["history"]
    assert np.all(np.isfinite(U)) and U.min() < -512.0
    h = info["history"]
    assert all(h[i + 1] < h[i] for i in range(len(h) - 1))
    if N == 33:
        X, nA = nref.dense_newton(None, "exp", 1.0, None, F, U, 1.0, 0.0, iters=8, chord=True)
        rU = np.max(np.abs(nref.residual_ld(None, "exp", 1.0, None, U, F, 1.0, 0.0)))
        rX = np.max(np.abs(nref.residual_ld(None, "exp", 1.0, None, X, F, 1.0, 0.0)))
        err = np.max(np.abs(U.astype(LD) - X))
        bound = nA * (rU + rX) * (1 + LD(1e-6))
        print(f"|U-X| {float(err):.3e} <= {float(bound):.3e} (N(U) {float(rU):.3e}, N(X) {float(rX):.3e}), min X {float(X.min())!r}")
        assert err <= bound and float(X.min()) < -512.0
