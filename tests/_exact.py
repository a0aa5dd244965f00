"""Exact problems for the shifted solve, the heat stepper and the variable-coefficient solve: fields of the CONTINUOUS
equations whose discrete solutions are known in closed form, built in np.longdouble from the formulas below and from nothing
the engine, its header or a restatement defines.  Every fp64 array is its longdouble original rounded once.

The grid is ref.cubic_problem's: x = x0 + col*dx, y = y0 + row*dx, dx = L/(N-1), (x0, y0) = ORIGIN unless a problem says
otherwise.

  vc_polynomial   a linear, U quadratic, F = div(a grad U) - sigma*U.  The face mean of a linear a is its midpoint value,
                  U[p+1] - U[p] = h*U_x(midpoint) for a quadratic, and the centred difference of the quadratic a*U_x is exact:
                  U is the discrete solution on its own rim at every N and L.
  vc_smooth       a = exp(0.6 sin(2x) cos(y)), U = sin(1.3x + 0.4) exp(0.7y), origin (0, 0), L = 1.5, sigma = 25: nothing is
                  exact, the discrete solution is second-order accurate.
  shifted_cubic   U = ref.CUBIC, F = Laplace(U) - sigma*U: the 5-point stencil is exact on cubics.
  Perturbed       heat: u_0 = P + A*m with P = ref.CUBIC held steady by Q = -nu*Laplace(P) and m the discrete sine mode
                  (k, l).  The stencil is exact on P and m is its eigenvector, so the theta-scheme gives
                  u_n = P + A*rho^n*m, rho = (sigma - beta*lambda_kl)/(sigma + lambda_kl).
  mixed_mode      boundary kinds per side (include/mg_bc.h): the eigenvectors of the 5-point Laplacian with a mirrored ghost
                  point beyond every Neumann side, one sine or cosine factor per axis, for all 16 kinds; check_mode_solve holds
                  a solve against one, and Perturbed(steady=False, bc=...) a heat stepper (pure decay, u_n = rho^n*u_0).
  MovingRim       heat: u = P + t*R, R = ref.HARMONIC, Q = R - nu*Laplace(P): linear in time, so every theta-scheme
                  reproduces it exactly -- when the right-hand side is formed on the old rim and the solve runs on the new one.

The scheme's constants are restated here from the equation, (u+ - u)/dt = nu*(theta*Lap u+ + (1 - theta)*Lap u) + q divided by
theta*nu: sigma = 1/(theta*nu*dt), beta = (1 - theta)/theta, gamma = 1/(theta*nu).  TEST INFRASTRUCTURE."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _solve_ref as ref
import _solve_shift_ref as sref

LD = ref.LD
U53 = ref.U53
ORIGIN = (0.25, -0.5)


def r64(A):
    return np.asarray(A, dtype=LD).astype(np.float64)


def together(*thunks):
    """The results of the thunks, evaluated side by side on up to four threads: numpy's longdouble loops release the
    interpreter lock, and at N = 4096 one residual in longdouble takes seconds."""
    with ThreadPoolExecutor(max_workers=min(4, len(thunks))) as pool:
        return [f.result() for f in [pool.submit(t) for t in thunks]]


def grid(N, L, origin=ORIGIN):
    """(x, y) in longdouble: x along columns (1 x N), y along rows (N x 1)."""
    k = np.arange(N).astype(LD)
    h = LD(L) / LD(N - 1)
    return (LD(origin[0]) + k * h)[None, :], (LD(origin[1]) + k * h)[:, None]


def poly(coeffs, x, y):
    """(P, Laplace(P)) of P = sum coeffs[i, j] x^i y^j in longdouble."""
    P = np.zeros((y.shape[0], x.shape[1]), dtype=LD)
    lap = np.zeros_like(P)
    for (i, j), c in coeffs.items():
        c = LD(c)
        P = P + (c * x ** i) * y ** j
        if i >= 2:
            lap = lap + (c * (i * (i - 1)) * x ** (i - 2)) * y ** j
        if j >= 2:
            lap = lap + (c * (j * (j - 1)) * x ** i) * y ** (j - 2)
    return P, lap


@functools.lru_cache(maxsize=2)
def cubic(N, L):
    """(P, Laplace(P)) of ref.CUBIC on the grid, in longdouble; shared by the cases of one size (treat as read-only)."""
    return poly(ref.CUBIC, *grid(N, L))


def with_rim(U, E):
    """A copy of U carrying E's rim."""
    out = np.array(U, copy=True)
    out[0, :], out[-1, :], out[:, 0], out[:, -1] = E[0, :], E[-1, :], E[:, 0], E[:, -1]
    return out


# ---------------------------------------------------------------- variable coefficient
def vc_polynomial(N, L, sigma):
    """a = 2 + 0.5x - 0.25y, U = 0.5 + x - 2y + xy + 0.75x^2 - 1.25y^2,
    F = a_x U_x + a_y U_y + a*(U_xx + U_yy) - sigma*U = 0.5 U_x - 0.25 U_y + a*(1.5 - 2.5) - sigma*U.
    Returns (a, U in longdouble, F, a_min): a_min at the corner (x0, y0 + L), 1.625 at L = 2.5 and 0.5 at L = 7."""
    x, y = grid(N, L)
    a = LD(2) + LD(0.5) * x - LD(0.25) * y
    U = LD(0.5) + x - 2 * y + x * y + LD(0.75) * x * x - LD(1.25) * y * y
    Ux = 1 + y + LD(1.5) * x
    Uy = -2 + x - LD(2.5) * y
    F = LD(0.5) * Ux - LD(0.25) * Uy + a * (LD(1.5) - LD(2.5)) - LD(sigma) * U
    a_min = LD(2) + LD(0.5) * LD(ORIGIN[0]) - LD(0.25) * (LD(ORIGIN[1]) + LD(L))
    return r64(a), U, r64(F), a_min


VC_SMOOTH_L, VC_SMOOTH_SIGMA = 1.5, 25.0


def vc_smooth(N):
    """Returns (a, U in longdouble, F) on [0, 1.5]^2 with sigma = 25; F = a_x U_x + a_y U_y + a*Laplace(U) - 25 U."""
    x, y = grid(N, VC_SMOOTH_L, (0.0, 0.0))
    a = np.exp(LD(0.6) * np.sin(2 * x) * np.cos(y))
    ax = a * LD(0.6) * 2 * np.cos(2 * x) * np.cos(y)
    ay = -a * LD(0.6) * np.sin(2 * x) * np.sin(y)
    U = np.sin(LD(1.3) * x + LD(0.4)) * np.exp(LD(0.7) * y)
    Ux = LD(1.3) * np.cos(LD(1.3) * x + LD(0.4)) * np.exp(LD(0.7) * y)
    Uy = LD(0.7) * U
    lap = (LD(0.7) ** 2 - LD(1.3) ** 2) * U
    F = ax * Ux + ay * Uy + a * lap - LD(VC_SMOOTH_SIGMA) * U
    return r64(a), U, r64(F)


def max_error(U, exact):
    """Interior max-norm of U - exact, in longdouble."""
    return np.max(np.abs(np.asarray(U, dtype=LD) - exact)[1:-1, 1:-1])


# ---------------------------------------------------------------- shift
def shifted_cubic(N, L, sigma):
    """(F, U) in fp64: U = ref.CUBIC, F = Laplace(U) - sigma*U formed in longdouble from the longdouble U."""
    U, lap = cubic(N, L)
    return r64(lap - LD(sigma) * U), r64(U)


# ---------------------------------------------------------------- heat
def heat_consts(nu, dt, theta):
    """(sigma, beta, gamma) in longdouble from the fp64 values of nu, dt and theta."""
    nu, dt, theta = LD(float(nu)), LD(float(dt)), LD(float(theta))
    return 1 / (theta * nu * dt), (1 - theta) / theta, 1 / (theta * nu)


def sine_mode(N, k, l):
    """sin(k pi col/(N-1)) sin(l pi row/(N-1)) with an exactly zero rim, in longdouble."""
    i = np.arange(N).astype(LD)
    pi = ref._ld_pi()
    m = np.sin(pi * LD(l) * i / LD(N - 1))[:, None] * np.sin(pi * LD(k) * i / LD(N - 1))[None, :]
    return with_rim(m, np.zeros((N, N), dtype=LD))


def mode_eigenvalue(N, L, k, l):
    """lambda_kl of -Laplace_h: (4/dx^2)(sin^2(k pi/(2(N-1))) + sin^2(l pi/(2(N-1))))."""
    pi = ref._ld_pi()
    return 4 * ref._inv_ld(N, L) * (np.sin(pi * LD(k) / LD(2 * (N - 1))) ** 2 + np.sin(pi * LD(l) / LD(2 * (N - 1))) ** 2)


# ---------------------------------------------------------------- boundary kinds: the modes of the mirrored operator
def _axis_kinds(bc):
    """((low end, high end) of the column axis, of the row axis) as booleans `Neumann`, from the kinds S, N, W, E (row 0, row
    N-1, column 0, column N-1) given as a string of 'd' / 'n' or four 0 / 1"""
    kS, kN, kW, kE = [(ch in "nN") if isinstance(ch, str) else bool(ch) for ch in bc]
    return (kW, kE), (kS, kN)


def _axis_range(N, lo, hi):
    """the admissible indices of one axis, one per unknown: d-d 1 .. N-2, n-n 0 .. N-1, mixed 0 .. N-2"""
    if lo and hi:
        return 0, N - 1
    return (0, N - 2) if lo or hi else (1, N - 2)


def _axis_factor(N, lo, hi, m):
    """The factor of one axis (table in the docstring of mixed_mode) in longdouble.  theta*i = pi*(2m + delta)*i / (2(N-1))
    with delta = 1 for unlike ends; the product is reduced in integers (period 4(N-1)) before it meets pi.  A Dirichlet end
    is forced to an exact zero, as with_rim does for the sine mode: sin(pi) and cos(pi/2) round to 1e-20, not to 0."""
    first, last = _axis_range(N, lo, hi)
    assert first <= m <= last, f"index {m} outside {first} .. {last}"
    i = np.arange(N, dtype=np.int64)
    num = ((2 * m + (1 if lo != hi else 0)) * i) % (4 * (N - 1))
    angle = ref._ld_pi() * num.astype(LD) / LD(2 * (N - 1))
    f = np.cos(angle) if lo else np.sin(angle)
    if not lo:
        f[0] = 0
    if not hi:
        f[-1] = 0
    return f


def _axis_theta(N, lo, hi, m):
    return ref._ld_pi() * (LD(2 * m + 1) / 2 if lo != hi else LD(m)) / LD(N - 1)


def mixed_mode(N, bc, k, l):
    """The eigenvector (k, l) of the 5-point Laplacian with a mirrored ghost point beyond every Neumann side, in longdouble:
    one factor per axis, index k along the columns (kinds W, E), l along the rows (kinds S, N), i the index along the axis:

        low end, high end    factor         theta
        d, d                 sin(theta i)   k pi/(N-1), k >= 1
        n, n                 cos(theta i)   k pi/(N-1), k >= 0
        d, n                 sin(theta i)   (k + 1/2) pi/(N-1)
        n, d                 cos(theta i)   (k + 1/2) pi/(N-1)

    sin vanishes at a Dirichlet low end and cos is even about a Neumann one; theta is what makes the high end do the same.
    Points on Dirichlet sides are exact zeros."""
    (kW, kE), (kS, kN) = _axis_kinds(bc)
    return _axis_factor(N, kS, kN, l)[:, None] * _axis_factor(N, kW, kE, k)[None, :]


def mixed_mode_eigenvalue(N, L, bc, k, l):
    """lambda of the discrete Laplacian on mixed_mode(N, bc, k, l): -(4/h^2)(sin^2(theta_x/2) + sin^2(theta_y/2)) <= 0."""
    (kW, kE), (kS, kN) = _axis_kinds(bc)
    return -4 * ref._inv_ld(N, L) * (np.sin(_axis_theta(N, kW, kE, k) / 2) ** 2 + np.sin(_axis_theta(N, kS, kN, l) / 2) ** 2)


def lambda_min(N, L, bc):
    """The smallest |lambda| over the admissible (k, l): the lowest index of each axis.  0 for four Neumann sides."""
    (kW, kE), (kS, kN) = _axis_kinds(bc)
    return -mixed_mode_eigenvalue(N, L, bc, _axis_range(N, kW, kE)[0], _axis_range(N, kS, kN)[0])


def check_mode_solve(U, info, star, F, L, sigma, bc, lam_min, what, coef=None):
    """A solve of (c*Laplace_h - sigma)U = F whose exact discrete solution is the longdouble `star` (a mixed_mode; c the
    constant coefficient, None: 1; lam_min = c*lambda_min), in the shape of test_solve_bc_gpu.test_against_the_direct_solution.
    diag(w)*A is symmetric for the trapezoid weights w, 1/4 <= w <= 1 on the unknowns, so ||(A - sigma)^-1|| <=
    1/(lam_min + sigma) in the w-norm and ||x||_w <= ||x||_2 <= 2||x||_w:

        max|U - U*| <= 2*(||r(U)||_2 + ||r(fp64(U*))||_2) / (lam_min + sigma)

    with both residuals in longdouble against F (_bc_ref.residual_ld_stencil: the dense matrix's expressions); the reported
    res within _bc_ref.residual_rounding_bound of ||r(U)||_2; and teeth: the bound is at most 1e-6*max|U*|.  info = None (the
    restatement): the line on res is left out.  Returns (error, bound), relative to max|U*|."""
    import _bc_ref as bref
    X = r64(star)
    rU, rX = together(lambda: bref.residual_ld_stencil(coef, U, F, L, sigma, bc), lambda: bref.residual_ld_stencil(coef, X, F, L, sigma, bc))
    nU, nX = np.sqrt(np.sum(rU ** 2)), np.sqrt(np.sum(rX ** 2))
    err = np.max(np.abs(np.asarray(U, dtype=LD) - X.astype(LD)))      # (against the fp64 array U* rounds to, as check_vc_truth)
    bound = 2 * (nU + nX) / (LD(lam_min) + LD(sigma))
    top = np.max(np.abs(star))
    print(f"{what}: |U - U*| {float(err):.3e} <= {float(bound):.3e} (relative {float(err / top):.2e} <= {float(bound / top):.2e}), "
          f"r(U) {float(nU):.3e}, r(U*) {float(nX):.3e}")
    assert err <= bound, f"{what}: max|U - U*| = {float(err):.6e} above {float(bound):.6e}"
    assert bound <= LD(1e-6) * top, f"{what}: no teeth: bound {float(bound):.3e} against max|U*| = {float(top):.3e}"
    if info is not None:
        a = None if coef is None else np.full(F.shape, float(coef))
        R = bref.residual_rounding_bound(a, U, F, L, sigma, bc, r=rU)
        print(f"{what}: {info['cycles']} cycles, res {info['res']:.6e} vs {float(nU):.6e} (bound {float(R):.3e})")
        assert info["converged"], f"{what}: not converged after {info['cycles']} cycles"
        assert abs(LD(info["res"]) - nU) <= R, f"{what}: res {info['res']!r} is not the residual of U, {float(nU)!r}"
    return float(err / top), float(bound / top)


def check_singular_mode_solve(U, info, star, F, L, d, mean, lam_plus, what, coef=None, teeth=1e-6):
    """A singular solve (four Neumann sides, sigma = 0, include/mg_singular.h) of c*Laplace_h U = F with F = fp64(c*lambda*U*) + d,
    `star` a mixed_mode of "nnnn" other than (0, 0) in longdouble: its weighted mean vanishes, so the answer with the target
    `mean` is X = fp64(U*) + mean whatever the incompatibility d.  check_mode_solve cannot serve, its lam_min is 0 for this
    kind.  diag(w)*A is symmetric, so A is self-adjoint in the w-inner product, and on the w-orthogonal complement of the
    constants ||A^-1||_w <= 1/lam_plus, lam_plus the smallest non-zero eigenvalue of -A (c times that of mode (0, 1));
    ||x||_w <= ||x||_2 <= 2||x||_w as in check_mode_solve, and the component of U - X along the constants is the difference
    of the two weighted means:

        max|U - X| <= 2*(||r(U)||_2 + ||r(X)||_2) / lam_plus + |mean_w(U) - mean_w(X)|

    both residuals in longdouble against Ft = F - mean_w(F), the fp64 array the solver itself works on
    (_singular_ref.project_mean), the means in longdouble.  Also: compat_defect is the restatement's mean_w(F), bit for bit,
    and within gamma(N^2)*mean_w(|F|) of d; teeth: the bound is at most teeth*max|U*|; converged; the reported res within
    _bc_ref.residual_rounding_bound of ||r(U)||_2; mean_w(U) within gamma(N^2)*mean_w(|U|) + 2u|mean| of the target.
    info: the solver's, or for the restatement dict(compat_defect, converged, cycles) without res (that line is left out).
    Returns (error, bound), relative to max|U*|."""
    import _bc_ref as bref
    import _singular_ref as sing
    bc = "nnnn"
    n = F.shape[0] * F.shape[0]
    Ft, c_F = sing.project_mean(F)
    X = r64(star) + float(mean)
    rU, rX, mU, mX, mF = together(lambda: bref.residual_ld_stencil(coef, U, Ft, L, 0.0, bc), lambda: bref.residual_ld_stencil(coef, X, Ft, L, 0.0, bc),
                                  lambda: (sing.weighted_mean_ld(U), sing.weighted_mean_ld(np.abs(U))), lambda: sing.weighted_mean_ld(X),
                                  lambda: sing.weighted_mean_ld(np.abs(F)))
    mU, mabsU = mU
    print(f"{what}: compat_defect {info['compat_defect']!r} for d = {d!r}, |difference| {abs(info['compat_defect'] - d):.3e} <= {float(sing.gamma(n) * mF):.3e}")
    assert info["compat_defect"] == c_F, f"{what}: compat_defect {info['compat_defect']!r} is not the restatement's mean_w(F) = {c_F!r}"
    assert abs(LD(info["compat_defect"]) - LD(d)) <= sing.gamma(n) * mF, f"{what}: compat_defect {info['compat_defect']!r} for d = {d!r}"
    nU, nX = np.sqrt(np.sum(rU ** 2)), np.sqrt(np.sum(rX ** 2))
    err = np.max(np.abs(np.asarray(U, dtype=LD) - X.astype(LD)))
    gauge = abs(mU - mX)
    bound = 2 * (nU + nX) / LD(lam_plus) + gauge
    top = np.max(np.abs(star))
    print(f"{what}: |U - X| {float(err):.3e} <= {float(bound):.3e} (relative {float(err / top):.2e} <= {float(bound / top):.2e}), "
          f"r(U) {float(nU):.3e}, r(X) {float(nX):.3e}, gauge term {float(gauge):.3e}, {info['cycles']} cycles")
    assert err <= bound, f"{what}: max|U - X| = {float(err):.6e} above {float(bound):.6e}"
    assert bound <= LD(teeth) * top, f"{what}: no teeth: bound {float(bound):.3e} against max|U*| = {float(top):.3e}"
    assert info["converged"], f"{what}: not converged after {info['cycles']} cycles"
    if "res" in info:
        a = None if coef is None else np.full(F.shape, float(coef))
        R = bref.residual_rounding_bound(a, U, Ft, L, 0.0, bc, r=rU)
        print(f"{what}: res {info['res']:.6e} vs {float(nU):.6e} (bound {float(R):.3e})")
        assert abs(LD(info["res"]) - nU) <= R, f"{what}: res {info['res']!r} is not the residual of U, {float(nU)!r}"
    slack = sing.gamma(n) * mabsU + 2 * U53 * abs(LD(mean))
    print(f"{what}: |mean_w(U) - mean| {float(abs(mU - LD(mean))):.3e} <= {float(slack):.3e}")
    assert abs(mU - LD(mean)) <= slack, f"{what}: mean_w(U) = {float(mU)!r} for the target {mean!r}"
    return float(err / top), float(bound / top)


class Perturbed:
    """u_0 = P + A*m, Q = -nu*Laplace(P) (steady=False: P = 0 and no Q, pure decay).  .U0 and .Q are the fp64 arrays a stepper
    is given (.Q None without P); exact(n) is u_n in longdouble; bound(n, rtol) is the a-priori bound on ||U_n - u_n||_2 of
    a theta >= 1/2 stepper whose solves stop at rtol:

        sum_{k=1..n} (rtol*||F*_k|| + R_k + eps_k) / (sigma + lambda_min)

    The step operator (sigma - beta*A_h)/(sigma + A_h), A_h = -Laplace_h, has norm <= 1 for theta >= 1/2, so what the earlier
    steps left is not amplified and each step adds its own solve error: the stopping rule rtol*||F|| plus the rounding R_k of
    the norm it is tested on (sref.residual_rounding_bound, on the exact u_k rounded to fp64 and F*_k) plus the rounding of
    the right-hand-side kernel, eps_k = 8*2^-53*|| sigma|u| + 8 beta inv |u| + gamma|Q| ||, all over the smallest eigenvalue
    of sigma + A_h.  F*_k is the right-hand side formed in longdouble from the exact u_{k-1}, with
    Laplace_h u = Laplace(P) - lambda_kl*A*rho^{k-1}*m.  Nothing in it comes from a run."""

    def __init__(self, N, L, nu, dt, theta, k, l, A, steady=True, bc=None, coef=None):
        self.N, self.L, self.bc, self.coef = N, L, bc, coef
        if steady:
            self.P, self.lapP = cubic(N, L)
        else:
            self.P, self.lapP = np.zeros((N, N), dtype=LD), np.zeros((N, N), dtype=LD)
        if bc is None:
            assert coef is None
            self.Am = LD(A) * sine_mode(N, k, l)
            self.lam = mode_eigenvalue(N, L, k, l)
            self.lam_min = ref.lambda_min(N, L)
        else:
            assert not steady, "the cubic is no solution under a Neumann side"
            c = LD(1.0 if coef is None else float(coef))
            self.Am = LD(A) * mixed_mode(N, bc, k, l)
            self.lam = -c * mixed_mode_eigenvalue(N, L, bc, k, l)
            self.lam_min = c * lambda_min(N, L, bc)
        self.sigma, self.beta, self.gamma = heat_consts(nu, dt, theta)
        self.rho = (self.sigma - self.beta * self.lam) / (self.sigma + self.lam)
        self.q = -LD(float(nu)) * self.lapP
        self.Q = r64(self.q) if steady else None
        self.U0 = r64(self.exact(0))

    def exact(self, n):
        return self.P + self.rho ** n * self.Am

    def rhs_star(self, k):
        """F*_k: the right-hand side of step k from the exact u_{k-1}."""
        lap_h = self.lapP - self.lam * self.rho ** (k - 1) * self.Am
        return -self.sigma * self.exact(k - 1) - self.beta * lap_h - self.gamma * self.q

    def norm(self, X):
        """the 2-norm the bound is stated in: over the interior, or over every unknown of the boundary kinds (the data points
        of every field here are zero, so that is the whole grid)"""
        return ref.norm_ld(X) if self.bc is None else np.sqrt(np.sum(np.asarray(X, dtype=LD) ** 2))

    def _bound_bc(self, n, rtol):
        """bound() under boundary kinds: A_h is symmetric in the inner product of the trapezoid weights w, 1/4 <= w <= 1
        on the unknowns, so the step operator has norm <= 1 and ||(A_h + sigma)^-1|| <= 1/(sigma + lam_min) in the w-norm, and
        ||x||_w <= ||x||_2 <= 2||x||_w: the sum of bound(), every term in the 2-norm, times 2.  R_k is
        _bc_ref.residual_rounding_bound; eps_k counts 16 roundings on sigma|u| + beta*inv*c*(sum|neighbours| + 4|u|), the
        neighbours through the mirror; the rounding of u_0 to fp64 is carried along."""
        import _bc_ref as bref
        inv = ref._inv_ld(self.N, self.L)
        c = LD(1.0 if self.coef is None else float(self.coef))
        a = None if self.coef is None else np.full((self.N, self.N), float(self.coef))

        def delta(k):
            Fs, uk = self.rhs_star(k), r64(self.exact(k))
            P = bref.pad(np.abs(self.exact(k - 1)), self.bc)
            nbr = P[2:, 1:-1] + P[:-2, 1:-1] + P[1:-1, 2:] + P[1:-1, :-2] + 4 * P[1:-1, 1:-1]
            r = bref.residual_ld_stencil(self.coef, uk, r64(Fs), self.L, float(self.sigma), self.bc)
            R = bref.residual_rounding_bound(a, uk, r64(Fs), self.L, float(self.sigma), self.bc, r=r)
            eps = 16 * U53 * self.norm(self.sigma * P[1:-1, 1:-1] + self.beta * inv * c * nbr)
            return (LD(rtol) * self.norm(Fs) + R + eps) / (self.sigma + self.lam_min)

        return 2 * (sum(together(*[lambda k=k: delta(k) for k in range(1, n + 1)]), LD(0)) + U53 * self.norm(self.exact(0)))

    def bound(self, n, rtol):
        if self.bc is not None:
            return self._bound_bc(n, rtol)
        inv = ref._inv_ld(self.N, self.L)

        def delta(k):
            Fs = self.rhs_star(k)
            prev = np.abs(self.exact(k - 1))
            R = sref.residual_rounding_bound(r64(self.exact(k)), r64(Fs), self.L, float(self.sigma))
            eps = 8 * U53 * ref.norm_ld(self.sigma * prev + 8 * self.beta * inv * prev + self.gamma * np.abs(self.q))
            return (LD(rtol) * ref.norm_ld(Fs) + R + eps) / (self.sigma + ref.lambda_min(self.N, self.L))

        return sum(together(*[lambda k=k: delta(k) for k in range(1, n + 1)]), LD(0))

    def moved(self, n):
        """||u_n - u_0||_2: what the steps did to the field."""
        return self.norm(self.exact(n) - self.exact(0))


class MovingRim:
    """u(t) = P + t*R with R = 1 + x - 2y + xy + x^2 - y^2 harmonic and Q = R - nu*Laplace(P).  (u+ - u)/dt = R and
    nu*Laplace_h(u) + Q = R at every time level (the stencil is exact on P and on R), so u_n = P + n*dt*R satisfies the
    theta-scheme exactly for every theta.  .Q is fp64, exact(n) longdouble."""

    def __init__(self, N, L, nu, dt, theta):
        self.N, self.L = N, L
        self.P, lapP = cubic(N, L)
        self.R, lapR = poly(ref.HARMONIC, *grid(N, L))
        assert not np.any(lapR)
        self.dt = LD(float(dt))
        self.q = self.R - LD(float(nu)) * lapP
        self.Q = r64(self.q)
        self.sigma, self.beta, self.gamma = heat_consts(nu, dt, theta)

    def exact(self, n):
        return self.P + LD(n) * self.dt * self.R

    def start_bound(self):
        """||fp64(u_0) - u_0||_2"""
        return U53 * ref.norm_ld(self.exact(0))

    def exact_residual_bound(self, n, prev):
        """A-priori bound on r(u_n as fp64) against the F that step n used, given ||U_{n-1} - u_{n-1}|| <= prev.  u_n solves the
        scheme exactly for F*_n, the right-hand side of the exact u_{n-1}, so the residual is the distance of F from F*_n plus
        the rounding of u_n to fp64 through the operator:
            ||(sigma - beta*A_h)(U_{n-1} - u_{n-1})|| <= (sigma + 8 beta inv)*prev
            + eps_n = 8*2^-53*|| sigma|u| + 8 beta inv |u| + gamma|Q| ||            (the roundings of the right-hand-side kernel)
            + 2^-53*(sigma + 8 inv)*||u_n||.
        sigma, beta and gamma are heat_consts's, from the equation.  This is what gives check_moving_rim_step its teeth: its
        error bound takes both residuals against the F the step used, so an F formed with a wrong constant would widen
        r(u_n), and the bound with it, unnoticed."""
        inv = ref._inv_ld(self.N, self.L)
        u = np.abs(self.exact(n - 1))
        eps = 8 * U53 * ref.norm_ld(self.sigma * u + 8 * self.beta * inv * u + self.gamma * np.abs(self.q))
        return (self.sigma + 8 * self.beta * inv) * prev + eps + U53 * (self.sigma + 8 * inv) * ref.norm_ld(self.exact(n))


def vc_exact_residual_bound(a, exact, F, L, sigma):
    """A-priori bound on the longdouble flux-form residual of the analytic U of vc_polynomial, rounded to fp64.  In exact
    arithmetic on exact data the residual is zero.  What is left, per point and then in the 2-norm:
      a and F were rounded to fp64: 2^-53*(inv*a_max*sum|U_nb - u| + |F|);
      U was rounded to fp64 and goes through the operator: 2^-53*(inv*a_max*(sum|U_nb| + 4|u|) + sigma|u|);
      the longdouble evaluation itself, 16 roundings of 2^-64 on the magnitude of the terms.
    Gives check_vc_truth its teeth: its error bound is built on r(exact), which a face mean that is not the midpoint value of
    the linear a would widen."""
    N = F.shape[0]
    inv, amax = ref._inv_ld(N, L), LD(float(np.max(a)))
    A = np.abs(exact)
    c = exact[1:-1, 1:-1]
    nb = (exact[2:, 1:-1], exact[:-2, 1:-1], exact[1:-1, 2:], exact[1:-1, :-2])
    diff = sum(np.abs(n - c) for n in nb)
    Fa = np.abs(np.asarray(F, dtype=LD))[1:-1, 1:-1]
    mag = inv * amax * (A[2:, 1:-1] + A[:-2, 1:-1] + A[1:-1, 2:] + A[1:-1, :-2] + 4 * A[1:-1, 1:-1]) + LD(sigma) * A[1:-1, 1:-1]
    data = U53 * np.sqrt(np.sum((inv * amax * diff + Fa) ** 2))
    return data + (U53 + 16 * LD(2.0) ** -64) * np.sqrt(np.sum((mag + Fa) ** 2))


# ---------------------------------------------------------------- the assertions the CPU and GPU modules share
def check_vc_truth(a, U, exact, F, L, sigma, rtol, a_min, what, info=None, U0=None):
    """test_solve_vc_gpu.test_against_the_direct_solution with the analytic U (longdouble `exact`, compared as the fp64 array it
    rounds to: the bound below is a statement about two fp64 arrays on one rim) in the dense solve's place:
    r(U) <= rtol*||F|| + R, which keeps the next line from being vacuous; ||U - exact|| <= (r(U) + r(exact as fp64)) /
    (a_min*lambda_min + sigma); r(exact as fp64) <= vc_exact_residual_bound, which pins the operator the other two
    lines measure with; and, given the solver's info and start, res and res0 within R of the longdouble residuals."""
    import _solve_vc_ref as vref
    N = F.shape[0]
    X = r64(exact)
    todo = [lambda: vref.residual_norm_ld(a, U, F, L, sigma), lambda: vref.residual_norm_ld(a, X, F, L, sigma),
            lambda: vref.residual_rounding_bound(a, U, F, L, sigma)]
    if info is not None:
        todo += [lambda: vref.residual_norm_ld(a, U0, F, L, sigma), lambda: vref.residual_rounding_bound(a, U0, F, L, sigma)]
    todo.append(lambda: vc_exact_residual_bound(a, exact, F, L, sigma))
    rU, rX, R, *start, pin = together(*todo)
    err = ref.norm_ld(np.asarray(U, dtype=LD) - X.astype(LD))
    bound = (rU + rX) / (LD(a_min) * ref.lambda_min(N, L) + LD(sigma))
    tol = LD(rtol) * ref.norm_ld(F)
    print(f"{what}: r(U) {float(rU):.3e} (tol {float(tol):.3e} + R {float(R):.3e}), r(exact) {float(rX):.3e} <= {float(pin):.3e}, "
          f"|U - exact| {float(err):.3e} <= {float(bound):.3e}, relative {float(err / ref.norm_ld(exact)):.2e}")
    assert rX <= pin, f"{what}: the analytic U leaves a residual of {float(rX):.6e}, above its rounding {float(pin):.6e}"
    assert rU <= tol + R, f"{what}: residual {float(rU):.6e} above {float(tol):.6e} + {float(R):.6e}"
    assert err <= bound, f"{what}: ||U - exact|| = {float(err):.6e} above {float(bound):.6e}"
    if info is not None:
        assert info["converged"], f"{what}: not converged after {info['cycles']} cycles"
        assert abs(LD(info["res"]) - rU) <= R, f"{what}: res {info['res']!r} is not the residual of U, {float(rU)!r}"
        r0, R0 = start
        assert abs(LD(info["res0"]) - r0) <= R0, f"{what}: res0 {info['res0']!r} is not the residual of the start, {float(r0)!r}"
    return float(err), float(bound)


def check_perturbed(p, U, n, rtol, what):
    """||U_n - u_n|| <= p.bound(n, rtol), and the teeth condition bound <= 1e-4*||u_n - u_0||: a wrong sign or factor in the
    scheme moves the field differently by a fraction of ||u_n - u_0||, four orders above the bound."""
    err = p.norm(np.asarray(U, dtype=LD) - p.exact(n))
    bound, moved = p.bound(n, rtol), p.moved(n)
    print(f"{what}: rho^n {float(p.rho ** n):.5f}, error {float(err):.3e} bound {float(bound):.3e} "
          f"moved {float(moved):.3e} bound/moved {float(bound / moved):.1e}")
    assert bound <= LD(1e-4) * moved, f"{what}: no teeth: bound {float(bound):.3e}, field moved by {float(moved):.3e}"
    assert err <= bound, f"{what}: ||U_n - u_n|| = {float(err):.6e} above the a-priori bound {float(bound):.6e}"
    return float(err), float(bound)


def moving_rim_error_and_bound(U, exact, F, L, sigma):
    """(||U - exact||, (r(U) + r(exact as fp64)) / (sigma + lambda_min), r(U), r(exact as fp64)): both residuals in longdouble
    against the F the step used; the error against the fp64 array the exact field rounds to."""
    N = F.shape[0]
    X = r64(exact)
    rU = sref.residual_norm_ld(U, F, L, sigma)
    rX = sref.residual_norm_ld(X, F, L, sigma)
    err = ref.norm_ld(np.asarray(U, dtype=LD) - X.astype(LD))
    return err, (rU + rX) / (LD(sigma) + ref.lambda_min(N, L)), rU, rX


def check_moving_rim_step(m, n, U, F, sigma, rtol, prev, what):
    """Step n of the MovingRim m in the correct order, U_n solved against F: r(U_n) <= rtol*||F|| + R;
    ||U_n - u_n|| <= (r(U_n) + r(u_n as fp64)) / (sigma + lambda_min); and r(u_n as fp64) <= m.exact_residual_bound(n, prev)
    with prev the bound on ||U_{n-1} - u_{n-1}|| that the step before returned (m.start_bound() for the first).  Returns
    (error, the bound on ||U_n - u_n|| for the next step)."""
    exact = m.exact(n)
    err, bound, rU, rX = moving_rim_error_and_bound(U, exact, F, m.L, sigma)
    tol, R = LD(rtol) * ref.norm_ld(F), sref.residual_rounding_bound(U, F, m.L, sigma)
    pin = m.exact_residual_bound(n, prev)
    print(f"{what}: r(U) {float(rU):.3e} (tol {float(tol):.3e} + R {float(R):.3e}), r(exact) {float(rX):.3e} <= {float(pin):.3e}, "
          f"error {float(err):.3e} bound {float(bound):.3e}, relative {float(err / ref.norm_ld(exact)):.2e}")
    assert abs(LD(sigma) - m.sigma) <= 4 * U53 * m.sigma, f"{what}: sigma {sigma!r} is not 1/(theta*nu*dt) = {float(m.sigma)!r}"
    assert rX <= pin, f"{what}: the exact u_n leaves a residual of {float(rX):.6e} against the step's F, above {float(pin):.6e}"
    assert rU <= tol + R, f"{what}: residual {float(rU):.6e} above {float(tol):.6e} + {float(R):.6e}"
    assert err <= bound, f"{what}: ||U_n - u_n|| = {float(err):.6e} above {float(bound):.6e}"
    return float(err), bound + U53 * ref.norm_ld(exact)
