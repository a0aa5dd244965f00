"""The eigen-solver (include/mg_eigs.h) without a GPU: the header against the binding and the library's exports, the struct
sizes, the method itself on the numpy restatement (tests/_eigs_ref.py) over every case of the GPU table against a dense
reference and the closed form, the host Rayleigh-Ritz step of the library on crafted matrices, and the Jacobi routine as a
stand-alone host program compiled from the engine's own source (once more under AddressSanitizer and UBSan)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _eigs_ref as er
import _solve_vc_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mg_eigs_opts_default", "mg_eigs_create", "mg_eigs_set_coefficient", "mg_eigs_solve", "mg_eigs_history",
           "mg_eigs_destroy", "mg_eigsGram", "mg_eigsRotate", "mg_eigsRayleighRitz")
U53 = er.U53


# ---------------------------------------------------------------- header, binding, structs
def test_header_declares_what_the_binding_binds_and_the_library_exports():
    import multigrid_poisson_solver_amd as m
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mg_eigs.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))
    assert names == sorted(SYMBOLS) == sorted(m.ABI_EIGS)
    lib = m.load_library()
    for name in names:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == m.ABI_EIGS[name][1]
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(m.ABI_EIGS[name][1]), name
    assert int(re.search(r"#define MG_EIGS_MAX_BLOCK (\d+)", text).group(1)) == m.MG_EIGS_MAX_BLOCK == er.MAX_BLOCK == 12
    assert float(re.search(r"#define MG_EIGS_DROP\s+(\S+)", text).group(1)) == m.MG_EIGS_DROP == er.DROP == 1e-12


def test_mg_hip_includes_the_header_once_after_the_types_it_needs():
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert hip.count('#include "mg_eigs.h"') == 1
    assert hip.index("} mg_solve_opts;") < hip.index('#include "mg_eigs.h"')
    assert hip.index('#include "mg_varcoef_batch.h"') < hip.index('#include "mg_eigs.h"')


def test_structs_have_their_stated_sizes():
    import multigrid_poisson_solver_amd as m
    assert [f for f, _ in m.EigsOpts._fields_] == ["cycle", "k", "guard", "max_iters", "rtol", "atol"]
    assert C.sizeof(m.SolveOpts) == 80
    assert C.sizeof(m.EigsOpts) == 112 and m.EigsOpts.k.offset == 80 and m.EigsOpts.rtol.offset == 96
    assert [f for f, _ in m.EigsResult._fields_] == ["status", "iters", "converged", "breakdown", "restarts", "cycles", "coarse_capped"]
    assert C.sizeof(m.EigsResult) == 28
    o = m.EigsOpts()
    m.load_library().mg_eigs_opts_default(C.byref(o))
    assert (o.k, o.guard, o.max_iters, o.rtol, o.atol) == (1, 0, 60, 1e-8, 0.0)
    assert (o.cycle.pre, o.cycle.post, o.cycle.N_min, o.cycle.omega, o.cycle.shift, o.cycle.fmg) == (3, 3, 8, 0.8, 0.0, 0)
    assert [m.eigs_default_guard(k) for k in (1, 3, 4, 8, 10, 11, 12)] == [2, 2, 2, 4, 2, 1, 0] == \
        [er.default_guard(k) for k in (1, 3, 4, 8, 10, 11, 12)]


# ---------------------------------------------------------------- the method on the restatement
CASES_N = [17, 24, 33, 40, 65]
FIELDS = ["one", "exp", "jump", "random"]
BLOCKS = [(1, 0), (1, 2), (4, 2), (5, 1), (8, 4)]
CYCLES = [(3, 3), (2, 1)]


def rounding_term(N, a, L=1.0):
    """n*u*||AA|| for each of: the dense eigvalsh on the fp64 matrix, the Gram sums behind theta, the deviation of X from
    orthonormality, the rounding of the operator; n = (N-2)^2, ||AA|| <= 8*a_max/dx^2 (Gershgorin)"""
    n = (N - 2) * (N - 2)
    dx = L / (N - 1)
    return 4.0 * n * U53 * 8.0 * float(np.max(a)) / (dx * dx)


@pytest.mark.parametrize("pre,post", CYCLES)
@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("N", CASES_N)
def test_restatement_converges_to_the_dense_reference(oracle, N, name, pre, post):
    a = vref.field(name, N, seed=1)
    dense = er.dense_eigenvalues(name, N, 1.0, 1, 13)
    for k, guard in BLOCKS:
        what = f"N={N} {name} k={k} guard={guard} V({pre},{post})"
        lam, X, info = er.solve(oracle, None if name == "one" else a, N, 1.0, k=k, guard=guard, max_iters=60, seed=3, pre=pre, post=post)
        print(f"{what}: iters {info['iters']} restarts {info['restarts']}")
        assert info["converged"] and not info["breakdown"], (what, info["iters"])
        RF = float(np.sqrt(np.sum(info["res"] ** 2)))
        rnd = rounding_term(N, a)
        n = (N - 2) * (N - 2)
        XtX = np.array([[float(er.dot_ld(X[i], X[j])) for j in range(k)] for i in range(k)])
        assert np.max(np.abs(XtX - np.eye(k))) <= 4 * er.gamma(n), (what, np.max(np.abs(XtX - np.eye(k))))
        res_ld = er.residuals_ld(a, N, 1.0, lam, X)
        for i in range(k):
            F = -(lam[i] * X[i])
            assert abs(info["res"][i] - res_ld[i]) <= vref.residual_rounding_bound(a, X[i], F, 1.0, 0.0), (what, i)
        for ref in [dense] + ([er.closed_form(N, 1.0, 13)] if name == "one" else []):
            err = np.abs(lam - ref[:k])
            assert np.all(err <= RF + rnd), (what, err, RF, rnd)
        gap = float(dense[k] - dense[k - 1])
        if gap > 4 * RF:
            assert np.all(np.abs(lam - dense[:k]) <= RF * RF / gap + rnd), (what, np.abs(lam - dense[:k]), RF * RF / gap, rnd)
        else:
            print(f"{what}: quadratic bound left out, gap {gap:.3e} <= 4||R||_F")


def test_the_quadratic_bound_covers_more_than_half_of_the_cases():
    """The share of the table the quadratic bound can be left out of, from the dense reference alone: a converged case has
    res_i <= rtol*lam_i, so ||R||_F <= rtol*sqrt(sum lam_i^2), and every case whose k-th gap exceeds 4 times THAT is checked
    above whatever residual the solve ends on."""
    left_out = er.quadratic_bound_left_out(CASES_N, FIELDS, BLOCKS, rtol=1e-8)
    total = len(CASES_N) * len(FIELDS) * len(BLOCKS) * len(CYCLES)
    share = len(left_out) * len(CYCLES) / total
    print(f"quadratic bound: at most {len(left_out) * len(CYCLES)} of {total} cases left out ({share:.3f}): {left_out}")
    assert share < 0.5


def test_the_dense_reference_meets_the_closed_form():
    for N in (17, 24, 40):
        dense, closed = er.dense_eigenvalues(None, N, 1.0, 0, 13), er.closed_form(N, 1.0, 13)
        n = (N - 2) * (N - 2)
        assert np.all(np.abs(dense - closed) <= n * U53 * 8.0 * (N - 1) ** 2), N
        assert closed[1] == closed[2] or abs(closed[1] - closed[2]) <= 4 * U53 * closed[1]   # lambda_12 = lambda_21


def test_two_blocks_are_slower_than_three(oracle):
    N, k, guard = 33, 4, 2
    a = vref.field("exp", N, seed=1)
    three = er.solve(oracle, a, N, k=k, guard=guard, seed=3)[2]
    two = er.solve(oracle, a, N, k=k, guard=guard, seed=3, blocks=2)[2]
    print(f"[X, W, P]: {three['iters']} iterations; [X, W]: {two['iters']} (converged: {two['converged']})")
    assert three["converged"] and (not two["converged"] or two["iters"] > three["iters"])


# ---------------------------------------------------------------- the library's host Rayleigh-Ritz step
def crafted(m, seed):
    """G, H of m random vectors of length 200 and a random symmetric positive definite operator"""
    rng = np.random.default_rng(seed)
    S = rng.random((200, m)) - 0.5
    B = rng.random((200, 200)) - 0.5
    A = B @ B.T + 200.0 * np.eye(200)
    return S, A, S.T @ S, S.T @ A @ S


@pytest.mark.parametrize("m,p", [(1, 1), (2, 1), (6, 2), (12, 12), (18, 6), (36, 12)])
def test_rayleigh_ritz_of_the_library_meets_the_restatement(m, p):
    import multigrid_poisson_solver_amd as mg
    S, A, G, H = crafted(m, 10 * m + p)
    kept, Cm, Cp, theta = mg.eigsRayleighRitz(G, H, p)
    kept_ref, C_ref, Cp_ref, theta_ref = er.rayleigh_ritz(G, H, p)
    assert kept == kept_ref == m
    scale = np.linalg.norm(A, 2)
    assert np.all(np.abs(theta - theta_ref) <= 64 * m * U53 * scale), (theta, theta_ref)
    X = S @ Cm
    assert np.max(np.abs(X.T @ X - np.eye(p))) <= 1e-12                      # orthonormal in the metric of G
    assert np.max(np.abs(X.T @ A @ X - np.diag(theta))) <= 1e-12 * scale     # and H is diagonal on it
    assert np.all(np.diff(theta) >= 0)
    assert np.array_equal(Cp[:p], np.zeros((p, p))) and np.array_equal(Cp[p:], Cm[p:])


def test_rayleigh_ritz_drops_a_duplicated_column_and_reports_a_breakdown():
    import multigrid_poisson_solver_amd as mg
    S, A, _, _ = crafted(6, 3)
    S[:, 4] = S[:, 1]                          # a duplicated column: rank 5
    G, H = S.T @ S, S.T @ A @ S
    kept, Cm, Cp, theta = mg.eigsRayleighRitz(G, H, 3)
    assert kept == 5 and theta.shape == (3,)
    X = S @ Cm
    assert np.max(np.abs(X.T @ X - np.eye(3))) <= 1e-10
    Q = np.linalg.svd(S, full_matrices=False)[0][:, :5]   # an orthonormal basis of the 5-dimensional span
    ritz = np.linalg.eigvalsh(Q.T @ A @ Q)[:3]
    assert np.all(np.abs(theta - ritz) <= 1e-9 * np.linalg.norm(A, 2)), (theta, ritz)
    S[:, 2] = S[:, 0] - S[:, 1]
    S[:, 3] = 2.0 * S[:, 0]
    S[:, 5] = S[:, 1]                          # rank 2 < p = 3
    kept, Cm, Cp, theta = mg.eigsRayleighRitz(S.T @ S, S.T @ A @ S, 3)
    assert kept == 2 and Cm is None
    G = np.eye(3)
    G[1, 1] = 0.0
    assert mg.eigsRayleighRitz(G, np.eye(3), 1)[0] == 0       # a zero column
    H = np.eye(3)
    H[0, 2] = H[2, 0] = np.nan
    assert mg.eigsRayleighRitz(np.eye(3), H, 1)[0] == 0       # a matrix that is not finite: the breakdown, not a rotation


# ---------------------------------------------------------------- the Jacobi routine as a stand-alone host program
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
#include "mg_eigs_rr.h"
// reads n and the n*n entries of a symmetric matrix from stdin; prints sweeps, w, V
int main()
{
    int n = 0;
    if (std::scanf("%d", &n) != 1 || n < 1 || n > 64) return 2;
    std::vector<double> A((size_t)n * n), w(n), V((size_t)n * n);
    for (double &x : A)
        if (std::scanf("%lf", &x) != 1) return 2;
    const int sweeps = mg::eigs_rr::jacobi_eig(n, A.data(), w.data(), V.data());
    std::printf("%d\n", sweeps);
    for (double x : w) std::printf("%.17g\n", x);
    for (double x : V) std::printf("%.17g\n", x);
    return 0;
}
"""


def symmetric_cases():
    rng = np.random.default_rng(11)
    out = [("1x1", np.array([[-3.5]])), ("2x2", np.array([[2.0, 1.0], [1.0, 2.0]]))]
    for n in (12, 36):
        B = rng.random((n, n)) - 0.5
        out.append((f"{n}x{n}", B + B.T))
    Q, _ = np.linalg.qr(rng.random((12, 12)))
    out.append(("repeated", Q @ np.diag([1.0, 1.0, 1.0, 2.0, 2.0, 3.0, 4.0, 5.0, 5.0, 5.0, 5.0, 9.0]) @ Q.T))
    out.append(("diagonal", np.diag([3.0, 1.0, 2.0])))
    return out


def run_jacobi(exe, A):
    n = A.shape[0]
    text = f"{n}\n" + "\n".join(f"{float(x).hex()}" for x in A.reshape(-1)) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    vals = r.stdout.split()
    return int(vals[0]), np.array(vals[1:1 + n], dtype=float), np.array(vals[1 + n:], dtype=float).reshape(n, n), r.stderr


@pytest.mark.parametrize("sanitize", [False, True])
def test_jacobi_routine_as_a_stand_alone_program(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "jacobi_main.cpp", tmp_path / "jacobi_main"
    src.write_text(PROGRAM)
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "multigrid_poisson_solver_amd", "csrc"), str(src), "-o", str(exe)]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if sanitize:   # (a host compiler without the sanitizers' runtime cannot link even an empty program with them)
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        linked = subprocess.run([cxx, "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")],
                                capture_output=True, text=True)
        if linked.returncode != 0:
            pytest.skip("this host compiler has no sanitizer runtime: " + linked.stderr[-200:])
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    for what, A in symmetric_cases():
        n = A.shape[0]
        sweeps, w, V, err = run_jacobi(str(exe), A)
        assert "runtime error" not in err and "AddressSanitizer" not in err, err
        scale = max(np.linalg.norm(A, 2), 1e-300)
        assert 0 <= sweeps <= 20, (what, sweeps)
        assert np.all(np.diff(w) >= 0), what
        assert np.all(np.abs(w - np.linalg.eigvalsh(A)) <= 64 * n * U53 * scale), (what, w)
        assert np.max(np.abs(V.T @ V - np.eye(n))) <= 64 * n * U53, what
        assert np.max(np.abs(A @ V - V * w[None, :])) <= 64 * n * U53 * scale, what
