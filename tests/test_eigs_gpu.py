"""The eigen-solver (include/mg_eigs.h) on the GPU: the Gram and the rotation kernel alone through their test hooks -- outputs
bit for bit against numpy, sums within the a-priori bound of the longdouble sum, NaN rims, guard bands --; whole solves
against a dense eigenvalue reference that shares no code with the engine and, for a == 1, the closed form, inside Kahan's
residual bounds; starts, determinism, refusals, lifecycle, torch tensors on a side stream, and the first mode fed to the
heat stepper."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _eigs_ref as er
import _guard
import _solve_vc_ref as vref
from conftest import assert_bits

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
U53 = er.U53


def nan_rim(x):
    x[0, :] = x[-1, :] = np.nan
    x[:, 0] = x[:, -1] = np.nan
    return x


def vectors(N, count, seed):
    rng = np.random.default_rng(seed)
    return [nan_rim(rng.random((N, N)) - 0.5) for _ in range(count)]


def within(got, x, y, N):
    """a device sum against the header's bound n*u/(1 - n*u) * sum|x*y| around the exact sum.  Up to N = 129 the exact sum is the
    longdouble one.  At the sizes of the 16-byte forms (1332 sums of 2.6e5 products each) the reference is numpy's pairwise
    fp64 sum of the rounded products instead, itself within (log2(n) + 10)*u*sum|x*y| < 40*u*sum|x*y| of the exact sum: that
    much is taken OFF the bound, so the check asks no less."""
    if N <= 129:
        return abs(LD(got) - er.dot_ld(x, y)) <= er.sum_bound(N, x, y)
    prod = er.inner(x) * er.inner(y)
    abs_sum = float(np.sum(np.abs(prod)))
    n = (N - 2) * (N - 2)
    assert n < 2 ** 28
    return abs(got - float(np.sum(prod))) <= (er.gamma(n) - 40 * U53) * abs_sum


# ---------------------------------------------------------------- kernels alone, inside guard bands
# one column per lane below N = 512 and for odd N; 512 is the first size of the 16-byte form (Gram: any m; rotation: m <= 12)
SIZES = [5, 8, 9, 16, 17, 31, 33, 64, 65, 129]
BASES = [1, 2, 3, 12, 13, 24, 36]


def gram_case(mg, N, m, placements=_guard.PLACEMENTS):
    S = vectors(N, m, 1000 * N + m)
    AS = vectors(N, m, 2000 * N + m)
    for placement in placements:
        what = f"gram N={N} m={m} {placement}"
        with _guard.block(mg, [N] * (2 * m), placement) as gb:
            gS, gAS = gb.views[:m], gb.views[m:]
            for view, x in zip(gb.views, S + AS):
                view.upload(x)
            gb.expect_readonly(*gb.views)
            G, H = mg.eigsGram(N, gS, gAS)
            gb.check(what)
            gb.expect_readonly(*gb.views)
            G2, H2 = mg.eigsGram(N, gS, gAS)
            gb.check(what + " again")
        assert_bits(G, G2, what + ": G twice")
        assert_bits(H, H2, what + ": H twice")
        assert_bits(G, G.T.copy(), what + ": G mirrored")
        assert_bits(H, H.T.copy(), what + ": H mirrored")
        for j in range(m):
            for l in range(j, m):
                assert within(G[j, l], S[j], S[l], N), (what, "G", j, l, G[j, l])
                assert within(H[j, l], S[j], AS[l], N), (what, "H", j, l, H[j, l])


@pytest.mark.parametrize("m", BASES)
@pytest.mark.parametrize("N", SIZES)
def test_gram_alone(mg, N, m):
    gram_case(mg, N, m)


@pytest.mark.parametrize("N,m", [(512, 1), (512, 13), (514, 36), (513, 7)])
def test_gram_alone_at_the_sixteen_byte_form(mg, N, m):
    gram_case(mg, N, m, placements=("page",))


def rotate_case(mg, N, m, p, placements=_guard.PLACEMENTS):
    rng = np.random.default_rng(7 * N + 100 * m + p)
    S = vectors(N, 3 * p, 3000 * N + m)
    AS = vectors(N, 3 * p, 4000 * N + m)
    C = rng.random((m, p)) - 0.5
    Cp = rng.random((m, p)) - 0.5
    Cp[:min(p, m)] = 0.0
    theta = rng.random(p) * 10.0
    X, AX, P, AP, R, _ = er.rotate(C, Cp, theta, S, AS)
    for placement in placements:
        what = f"rotate N={N} m={m} p={p} {placement}"
        with _guard.block(mg, [N] * (7 * p), placement) as gb:
            gS, gAS, gR = gb.views[:3 * p], gb.views[3 * p:6 * p], gb.views[6 * p:]
            for view, x in zip(gb.views, S + AS + vectors(N, p, 5)):
                view.upload(x)
            # the W block is no output slot: S[p:2p] and AS[p:2p] are read at most
            gb.expect_readonly(*(gS[p:2 * p] + gAS[p:2 * p]))
            res2 = mg.eigsRotate(N, C, Cp, theta, gS, gAS, gR)
            gb.check(what)
            groups = dict(X=(gS[:p], X), AX=(gAS[:p], AX), P=(gS[2 * p:], P), AP=(gAS[2 * p:], AP), R=(gR, R))
            for name, (views, want) in groups.items():
                for i in range(p):
                    got = views[i].to_host()
                    assert_bits(got[1:-1, 1:-1], want[i][1:-1, 1:-1], f"{what}: {name}[{i}] interior")
                    rim = np.concatenate([got[0, :], got[-1, :], got[:, 0], got[:, -1]])
                    assert np.all(np.isnan(rim)), f"{what}: the rim of {name}[{i}] was written"
        for i in range(p):
            assert within(res2[i], R[i], R[i], N), (what, i, res2[i])


@pytest.mark.parametrize("m", BASES)
@pytest.mark.parametrize("N", SIZES)
def test_rotate_alone(mg, N, m):
    # p in {1, m/3, 12} where p <= m <= 3p holds
    ps = sorted({p for p in (1, m // 3, 12) if 1 <= p <= 12 and p <= m <= 3 * p})
    assert ps or m in (13,), (m, ps)
    if not ps:
        ps = [5]   # m = 13: p = 5 (2p < m <= 3p, the full basis with a ragged last block)
    for p in ps:
        rotate_case(mg, N, m, p, placements=_guard.PLACEMENTS if N <= 33 else ("page",))


@pytest.mark.parametrize("N,m,p", [(512, 3, 1), (512, 12, 4), (514, 13, 5), (512, 36, 12), (513, 6, 2)])
def test_rotate_alone_at_the_sixteen_byte_form(mg, N, m, p):
    rotate_case(mg, N, m, p, placements=("page",))


def test_hooks_refuse_bad_arguments(mg):
    g = mg.DeviceGrid.zeros(8)
    one = np.ones((1, 1))
    for call in (lambda: mg.eigsGram(2, [g], [g]), lambda: mg.eigsGram(8, [g] * 37, [g] * 37),
                 lambda: mg.eigsRotate(2, one, one, np.ones(1), [g] * 3, [g] * 3, [g]),
                 lambda: mg.eigsRotate(8, np.ones((4, 1)), np.ones((4, 1)), np.ones(1), [g] * 3, [g] * 3, [g])):
        with pytest.raises(mg.MGError, match=r"\[2\]"):
            call()
    g.free()


# ---------------------------------------------------------------- whole solves against truth
CASES_N = [17, 24, 33, 40, 65]
FIELDS = ["one", "exp", "jump", "random"]
BLOCKS = [(1, 0), (1, 2), (4, 2), (5, 1), (8, 4)]
CYCLES = [(3, 3), (2, 1)]


def coefficient(name, N):
    return vref.field(name, N, seed=1)


def rounding_term(N, a, L=1.0):
    """What rounding alone may put between a computed Ritz value and a dense-reference eigenvalue: each of (the dense
    eigvalsh on the fp64 matrix, the Gram sums behind theta, the deviation of X from orthonormality, the rounding of the
    operator itself) is at most n*u*||AA||, n = (N-2)^2, ||AA|| <= 8*a_max/dx^2 (Gershgorin)."""
    n = (N - 2) * (N - 2)
    dx = L / (N - 1)
    return 4.0 * n * U53 * 8.0 * float(np.max(a)) / (dx * dx)


def check_solution(N, name, a, k, lam, X, info, what, refs=None):
    """refs: the reference eigenvalues, ascending, at least k + 1 of each (the first one carries the gap of the quadratic
    bound); None: the dense reference of the field `name` and, for the field `one`, the closed form"""
    assert info["converged"] and not info["breakdown"], (what, info)
    assert info["cycles"] == (k + info["guard"]) * info["iters"], (what, info)
    # the rim of the result is +0
    for x in X:
        rim = np.concatenate([x[0, :], x[-1, :], x[:, 0], x[:, -1]])
        assert_bits(rim, np.zeros(rim.size), what + ": rim")
    # the reported residuals are true residuals
    for i in range(k):
        F = -(lam[i] * X[i])
        res_ld = vref.residual_norm_ld(a, X[i], F, 1.0, 0.0)
        bound = vref.residual_rounding_bound(a, X[i], F, 1.0, 0.0)
        print(f"{what}: res[{i}] = {info['res'][i]:.6e}, longdouble {float(res_ld):.6e}, bound {float(bound):.3e}")
        assert abs(LD(info["res"][i]) - res_ld) <= bound, (what, i, info["res"][i], res_ld, bound)
        assert info["res"][i] <= 1e-8 * lam[i], (what, i)
    # orthonormality: a Gram sum of n terms carries n*u/(1 - n*u) relative to the norms (Cauchy-Schwarz); the last
    # Rayleigh-Ritz step orthonormalises in the metric of ITS Gram sums and the check below forms its own: 2 of them, and as
    # much again for the rotation's m <= 36 roundings per point and the rounding of the scaled eigen-solve
    n = (N - 2) * (N - 2)
    XtX = np.array([[float(er.dot_ld(X[i], X[j])) for j in range(k)] for i in range(k)])
    dev = np.max(np.abs(XtX - np.eye(k)))
    print(f"{what}: |X^T X - I| = {dev:.3e}, bound {4 * er.gamma(n):.3e}")
    assert dev <= 4 * er.gamma(n), (what, dev)
    # Kahan: an orthonormal block with residual R has k eigenvalues within ||R||_F of its Ritz values
    if refs is None:
        refs = [er.dense_eigenvalues(name, N, 1.0, 1, 13)]
        if name == "one":
            refs.append(er.closed_form(N, 1.0, 13))
    RF = float(np.sqrt(np.sum(np.asarray(info["res"]) ** 2)))
    rnd = rounding_term(N, a)
    for ref in refs:
        err = np.abs(lam - ref[:k])
        print(f"{what}: max |lam - ref| = {err.max():.3e}, ||R||_F = {RF:.3e}, rounding {rnd:.3e}")
        assert np.all(err <= RF + rnd), (what, err, RF, rnd)
    gap = float(refs[0][k] - refs[0][k - 1])
    if gap > 4 * RF:
        assert np.all(np.abs(lam - refs[0][:k]) <= RF * RF / gap + rnd), (what, np.abs(lam - refs[0][:k]), RF * RF / gap, rnd)
    else:
        print(f"{what}: quadratic bound left out, gap {gap:.3e} <= 4||R||_F")


@pytest.mark.parametrize("pre,post", CYCLES)
@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("N", CASES_N)
def test_solves_meet_the_dense_reference(mg, N, name, pre, post):
    a = coefficient(name, N)
    for k, guard in BLOCKS:
        what = f"N={N} {name} k={k} guard={guard} V({pre},{post})"
        with mg.EigenSolver(N, 1.0, k=k, guard=guard, coef=None if name == "one" else a, max_iters=60, pre=pre, post=post) as e:
            lam, X, info = e.solve(seed=3)
            hist = e.history()
        info["guard"] = guard
        print(f"{what}: iters {info['iters']} restarts {info['restarts']}")
        assert len(hist) == info["iters"] + 1
        check_solution(N, name, a, k, lam, X, info, what)


def test_the_quadratic_bound_covers_more_than_half_of_the_cases():
    """The share of the table the quadratic bound can be left out of, from the dense reference alone: a converged case has
    res_i <= rtol*lam_i, so ||R||_F <= rtol*sqrt(sum lam_i^2), and every case whose k-th gap exceeds 4 times THAT is checked
    above whatever residual the solve ends on."""
    left_out = er.quadratic_bound_left_out(CASES_N, FIELDS, BLOCKS, rtol=1e-8)
    total = len(CASES_N) * len(FIELDS) * len(BLOCKS) * len(CYCLES)
    share = len(left_out) * len(CYCLES) / total
    print(f"quadratic bound: at most {len(left_out) * len(CYCLES)} of {total} cases left out ({share:.3f}): {left_out}")
    assert share < 0.5


# ---------------------------------------------------------------- starts and options
def test_a_converged_start_returns_at_once_with_the_same_eigenvalues(mg):
    N, k = 33, 4
    with mg.EigenSolver(N, 1.0, k=k, guard=2, coef=coefficient("exp", N)) as e:
        lam, X, info = e.solve(seed=1)
        lam2, X2, info2 = e.solve(X0=X, seed=1)
    assert info["converged"] and info2["converged"]
    assert info2["iters"] == 0 and info2["cycles"] == 0, info2
    print("lam first ", [float(v).hex() for v in lam])
    print("lam second", [float(v).hex() for v in lam2])
    assert_bits(lam2, lam, "lam of the restart")
    assert_bits(X2, X, "X of the restart: returned untouched")
    assert np.array_equal(info2["res"], info["res"])


def test_a_rank_deficient_start_still_converges(mg):
    """k start vectors in the span of two: the dependent columns are replaced before the first step, and directions the
    Rayleigh-Ritz step drops later are refilled by W"""
    N, k = 33, 4
    rng = np.random.default_rng(5)
    v, w = rng.random((N, N)) - 0.5, rng.random((N, N)) - 0.5
    for guard, X0 in ((0, [v, w, v + w, v - 2.0 * w]), (2, [v, w, v + w, v - 2.0 * w]),
                      (2, [v, w, v + w + 1e-7 * rng.random((N, N)), v - 2.0 * w])):
        with mg.EigenSolver(N, 1.0, k=k, guard=guard) as e:
            lam, X, info = e.solve(X0=np.stack(X0))
            kept = [h["kept"] for h in e.history()]
        print(f"rank-deficient start, guard {guard}: iters {info['iters']}, directions kept per step {kept}")
        assert info["converged"] and not info["breakdown"], info
        check_solution(N, "one", np.ones((N, N)), k, lam, X, dict(info, guard=guard), f"rank-deficient start, guard {guard}")


def test_unit_coefficient_as_an_array_and_determinism(mg):
    N, k = 40, 4
    with mg.EigenSolver(N, 1.0, k=k) as e:
        lam0, X0, info0 = e.solve(seed=2)
        lam1, X1, info1 = e.solve(seed=2)
        e.set_coefficient(np.ones((N, N)))
        lam2, X2, info2 = e.solve(seed=2)
        e.set_coefficient(None)
        lam3, X3, info3 = e.solve(seed=2)
    for lam, X, info, what in ((lam1, X1, info1, "twice"), (lam2, X2, info2, "a == 1 as an array"), (lam3, X3, info3, "coefficient taken away")):
        assert_bits(lam, lam0, what + ": lam")
        assert_bits(X, X0, what + ": X")
        assert info["iters"] == info0["iters"] and np.array_equal(info["res"], info0["res"]), what


def test_refusals_leave_a_working_solver(mg):
    """every refusal by its own text, each followed by a solve with the earlier bits"""
    N = 33
    base = dict(k=2, guard=2)
    create = lambda n, **o: (lambda: mg.EigenSolver(n, 1.0, **dict(base, **o)))
    a_bad = np.ones((N, N))
    a_bad[3, 4] = -1.0
    with mg.EigenSolver(N, 1.0, **base) as e:
        lam0, X0, _ = e.solve(seed=4)
        refusals = [
            (create(N, shift=1.0), r"\[2\] mg_eigs_create: cycle\.shift must be 0"),
            (create(N, fmg=1), r"\[2\] mg_eigs_create: cycle\.fmg must be 0"),
            (create(N, k=0), r"\[2\] mg_eigs_create: k < 1"),
            (create(N, guard=-1), r"\[2\] mg_eigs_create: guard < 0"),
            (create(N, k=8, guard=5), r"\[2\] mg_eigs_create: k \+ guard exceeds MG_EIGS_MAX_BLOCK"),
            (create(N, k=13, guard=0), r"\[2\] mg_eigs_create: k \+ guard exceeds MG_EIGS_MAX_BLOCK"),
            (create(N, max_iters=-1), r"\[2\] mg_eigs_create: max_iters < 0"),
            (create(N, rtol=-1.0), r"\[2\] mg_eigs_create: rtol and atol"),
            (create(N, atol=float("nan")), r"\[2\] mg_eigs_create: rtol and atol"),
            (create(N, pre=0), r"\[2\] mg_eigs_create: pre = 0"),
            (create(6, k=4, guard=2, N_min=3), r"\[2\] mg_eigs_create: 3\(k \+ guard\) exceeds"),   # 18 > 16 interior points, two levels
            (create(15, k=1, guard=0), r"\[2\] mg_eigs_create: .*two levels"),                      # N < 2*N_min
            (lambda: e.set_coefficient(a_bad), r"\[2\] mg_batch_solver_set_coefficient: every value of a must be finite and > 0"),
            (lambda: e.set_coefficient(np.ones((N + 1, N + 1))), r"coef: array of shape"),
            (lambda: e.solve(X0=np.zeros((3, N, N))), r"X0: 3 vectors for k = 2"),
        ]
        for call, text in refusals:
            with pytest.raises(mg.MGError, match=text):
                call()
            lam1, X1, _ = e.solve(seed=4)
            assert_bits(lam1, lam0, "lam after " + text)
            assert_bits(X1, X0, "X after " + text)


def test_one_iteration_reports_true_residuals(mg):
    N, k = 33, 2
    a = coefficient("jump", N)
    with mg.EigenSolver(N, 1.0, k=k, guard=2, coef=a, max_iters=1) as e:
        lam, X, info = e.solve(seed=6)
        hist = e.history()
    assert not info["converged"] and info["iters"] == 1 and info["cycles"] == 4 and len(hist) == 2, info
    for i in range(k):
        F = -(lam[i] * X[i])
        res_ld = vref.residual_norm_ld(a, X[i], F, 1.0, 0.0)
        assert abs(LD(info["res"][i]) - res_ld) <= vref.residual_rounding_bound(a, X[i], F, 1.0, 0.0), (i, info["res"][i], res_ld)
    with mg.EigenSolver(N, 1.0, k=k, guard=2, coef=a, max_iters=0) as e:
        lam, X, info = e.solve(seed=6)
    assert not info["converged"] and info["iters"] == 0 and info["cycles"] == 0


def test_lifecycle_and_the_one_call_form(mg):
    N = 24
    lam, X, info = mg.eigs(N, 3, seed=1)
    assert info["converged"] and X.shape == (3, N, N)
    e = mg.EigenSolver(N, 1.0, k=3)
    assert e.guard == 2 == mg.eigs_default_guard(3) and mg.eigs_default_guard(11) == 1 and mg.eigs_default_guard(8) == 4
    lam1, X1, _ = e.solve(seed=1)
    e.close()
    e.close()
    assert_bits(lam1, lam, "one-call form")
    # DeviceGrids in, DeviceGrids out, worked on in place
    grids = [mg.DeviceGrid.from_host(x) for x in X]
    with mg.EigenSolver(N, 1.0, k=3) as e:
        lam2, out, info2 = e.solve(X0=grids)
    assert out[0] is grids[0] and info2["converged"]
    for g in grids:
        g.free()


def test_torch_tensors_on_a_side_stream(mg):
    worker = os.path.join(HERE, "_eigs_torch_worker.py")
    r = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout, r.stdout + r.stderr


def test_the_first_mode_decays_in_the_heat_stepper(mg):
    """One backward-Euler step of u_t = nu*Laplace(u) from the first mode: u+ = u/(1 + nu*dt*lam_1) up to the eigen-residual and
    the stepper's stopping rule ||F - A u+|| <= rtol*||F||, which bounds the error by rtol*||F||/sigma (the shifted operator's
    smallest eigenvalue exceeds sigma = 1/(nu*dt))."""
    N, nu, dt, rtol = 65, 0.7, 1e-3, 1e-10
    lam, X, info = mg.eigs(N, 1, guard=2)
    assert info["converged"]
    st = mg.HeatStepper(N, 1.0, nu=nu, dt=dt, theta=1.0, rtol=rtol)
    U, hinfo = st.step(X[0].copy())
    st.close()
    U = np.asarray(U).reshape(N, N)
    factor = 1.0 / (1.0 + nu * dt * lam[0])
    sigma = 1.0 / (nu * dt)
    normF = sigma * float(np.sqrt(er.dot(X[0], X[0])))
    err = float(np.sqrt(er.dot(U - factor * X[0], U - factor * X[0])))
    bound = rtol * normF / sigma + info["res"][0] * nu * dt + 64 * U53
    print(f"heat: factor {factor:.6f}, |u+ - factor*u| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
