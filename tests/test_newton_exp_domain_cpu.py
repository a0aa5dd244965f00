"""What the GPU cases of tests/test_newton_exp_domain_gpu.py rest on, checked without a GPU: the argument set of
tests/_exp_cases.py covers every table index of exp_libm at every exponent, both signs and every listed edge; the longdouble
reference agrees with mpmath at 200 bits to 2^-10 ulp of a double; the host libm's largest error on the verified path, by that
reference (printed: about 0.506 ulp with glibc); the restatement's exp returns libm's classes beyond the verified path."""
import math

import numpy as np
import pytest

import _exp_cases as xc
import _newton_ref as nref

LD = np.longdouble


def test_r2_covers_every_table_index_at_every_exponent_and_both_signs():
    x = xc.r2()
    assert np.all(np.abs(x) >= xc.TINY) and np.all(np.abs(x) < xc.BIG) and np.all(np.isfinite(x))
    k = xc.k_of(x)
    ks = xc.k_range()
    K = int(ks[-1])
    assert K == 94548 and ks[0] == -K
    count = np.bincount(k + K, minlength=2 * K + 1)
    assert np.all(count >= 1), "a k with no argument"
    inner = np.abs(ks) < K
    assert np.all(count[inner] >= 3), "a k without its three arguments"
    # the two tie edges of every k: fractional parts of x*128/ln 2 beyond +-0.499 on both sides
    frac = (x.astype(LD) * xc.K_PER_UNIT - k.astype(LD)).astype(np.float64)
    assert np.all(np.abs(frac) < 0.5)
    lo = np.bincount((k + K)[frac < -0.4999], minlength=2 * K + 1)
    hi = np.bincount((k + K)[frac > 0.4999], minlength=2 * K + 1)
    assert np.all(lo[inner] >= 1) and np.all(hi[inner] >= 1)
    # every (exponent k >> 7, table index k & 127) pair that |x| < 512 reaches
    pairs = set(zip((ks >> 7).tolist(), (ks & 127).tolist()))
    assert set(zip((k >> 7).tolist(), (k & 127).tolist())) == pairs
    exps = sorted({e for e, _ in pairs})
    assert exps[0] == -739 and exps[-1] == 738 and len(exps) == 1478
    per_exp = np.bincount(np.array([e for e, _ in pairs]) - exps[0])
    assert np.all(per_exp[1:-1] == 128) and per_exp[0] >= 1 and per_exp[-1] >= 1
    assert np.any(x > 0) and np.any(x < 0)
    # the log-uniform part reaches every binade from 2^-54 to 2^8 on both signs
    for s in (1.0, -1.0):
        e = np.frexp(x[s * x > 0])[1]
        assert set(range(-53, 10)) <= set(e.tolist())
    for v in xc.R2_EDGES:
        assert np.any(x == v), v
    print(f"R2: {x.size} arguments, k = -{K} .. {K}, {len(exps)} exponents x 128 table entries")


def test_r1_and_r3_hold_each_listed_edge():
    r1, r3 = xc.r1(), xc.r3()
    assert np.all(np.abs(r1) < xc.TINY) and r1.size == 8
    assert sum(1 for v in r1 if v == 0.0 and math.copysign(1.0, v) < 0) == 1 and sum(1 for v in r1 if v == 0.0) == 2
    for v in (5e-324, 1e-300, math.nextafter(2.0 ** -54, 0.0)):
        assert v in r1 and -v in r1
    assert np.all((np.abs(r3) >= xc.BIG) | np.isnan(r3))
    for v in (512.0, 600.0, 700.0):
        assert v in r3 and -v in r3
    below, above = xc.EXP_MAX, math.nextafter(xc.EXP_MAX, math.inf)
    assert below in r3 and above in r3 and math.isfinite(math.exp(below))
    with pytest.raises(OverflowError):
        math.exp(above)
    for v in (710.0, 1e308, -708.4, -745.13, -745.14, -746.0, -1e308, math.inf, -math.inf):
        assert v in r3
    assert np.isnan(r3).sum() == 1
    # the classes the lists claim, by the reference
    ref = xc.exp_ref(np.array(xc.R3_FINITE))
    assert np.all(ref > 0) and np.all(ref <= xc.DBL_MAX)
    sub = xc.exp_ref(np.array(xc.R3_SUBNORMAL))
    assert np.all(sub < xc.MIN_NORMAL) and np.all(sub > 0)
    # exp(-745.13) lies just above half the smallest subnormal, exp(-745.14) just below: the last non-zero result lies between
    assert sub[1] > xc.SUB_SPACING / 2 > sub[2]
    assert np.all(xc.exp_ref(np.array([v for v in xc.R3_OVER if math.isfinite(v)])) > xc.DBL_MAX)
    assert np.all(xc.exp_ref(np.array([v for v in xc.R3_ZERO if math.isfinite(v)])) < xc.SUB_SPACING / 2)


def test_field_layouts():
    v = np.arange(1.0, 30.0)
    U, n = xc.field(v, 4, start=3)
    assert n == 16 and np.array_equal(U.reshape(-1), v[3:19])
    U, n = xc.field(v, 4, start=16)
    assert n == 13 and np.array_equal(U.reshape(-1)[:13], v[16:]) and np.array_equal(U.reshape(-1)[13:], v[16:19])
    assert xc.calls(v, 4) == [0, 16]
    U, r, c = xc.patches(v[:9], 10)
    for dr, dc in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
        assert np.array_equal(U[r + dr, c + dc], v[:9])
    assert r.min() >= 1 and r.max() <= 8 and c.min() >= 1 and c.max() <= 8


def test_ulp_measure():
    one = LD(1)
    assert xc.spacing(one) == LD(2) ** -52 and xc.spacing(LD(2) - LD(2) ** -60) == LD(2) ** -52
    assert xc.spacing(LD(0.75)) == LD(2) ** -53
    assert xc.spacing(LD(2) ** -1022) == LD(2) ** -1074 and xc.spacing(LD(2) ** -1030) == LD(2) ** -1074
    assert xc.spacing(LD(2) ** -1021) == LD(2) ** -1073
    assert xc.ulp_error(np.array([1.0 + 2.0 ** -52]), np.array([one])) == 1
    assert xc.ulp_error(np.array([5e-324]), np.array([LD(2) ** -1074 * LD(1.25)])) == LD(0.25)


def test_longdouble_reference_against_mpmath_at_200_bits():
    import mpmath
    assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit mantissa here: the reference would be no better than the host libm"
    x2 = xc.r2()
    pick = np.random.default_rng(7).choice(x2.size, 3000, replace=False)
    finite3 = np.array(xc.R3_FINITE)
    x = np.concatenate([x2[pick], np.array(xc.R2_EDGES), xc.r1(), finite3])
    ref = xc.exp_ref(x)
    worst = 0.0
    with mpmath.workprec(200):
        for v, r in zip(x.tolist(), ref):
            true = mpmath.exp(mpmath.mpf(v))
            m, e = np.frexp(r)                                     # r = m * 2^e exactly, m of 64 bits: two exact halves
            hi = float(np.ldexp(m, 32).astype(np.int64))           # (m*2^32 truncated, exact in a double)
            lo = float(np.ldexp(m, 64) - np.ldexp(LD(hi), 32))
            got = (mpmath.mpf(hi) * 2 ** 32 + mpmath.mpf(lo)) * mpmath.mpf(2) ** (int(e) - 64)
            sp = mpmath.mpf(2) ** -1074 if true < mpmath.mpf(2) ** -1022 else mpmath.mpf(2) ** (mpmath.floor(mpmath.log(true, 2)) - 52)
            worst = max(worst, float(abs(got - true) / sp))
    print(f"longdouble exp against mpmath (200 bits) on {x.size} arguments: largest error {worst:.3e} ulp of a double "
          f"(bound 2^-10 = {2.0 ** -10:.3e})")
    assert worst <= 2.0 ** -10
    # the classes beyond the finite range, by mpmath as well
    with mpmath.workprec(200):
        for v in xc.R3_OVER:
            if math.isfinite(v):
                assert mpmath.exp(mpmath.mpf(v)) > mpmath.mpf(np.finfo(np.float64).max)
        for v in xc.R3_ZERO:
            if math.isfinite(v):
                assert mpmath.exp(mpmath.mpf(v)) < mpmath.mpf(2) ** -1075


def test_host_libm_largest_error_on_the_verified_path():
    """measured, printed, and held only to what any libm worth comparing with delivers (1 ulp); glibc 2.28+: 0.506"""
    x = np.concatenate([xc.r2(), xc.r1()])
    err = xc.ulp_error(xc.host_exp(x), xc.exp_ref(x))
    i = int(np.argmax(err))
    print(f"host libm exp on {x.size} arguments of R1 and R2: largest error {float(err[i]):.4f} ulp at x = {x[i]!r}")
    assert float(err[i]) < 1.0


def test_restatement_exp_gives_libms_classes_beyond_the_verified_path():
    r3 = xc.r3()
    with np.errstate(all="ignore"):
        e = nref._exp(r3)
    for v, got in zip(r3.tolist(), e.tolist()):
        if math.isnan(v):
            assert math.isnan(got)
        elif v in xc.R3_OVER:
            assert got == math.inf, v
        elif v in xc.R3_ZERO:
            assert got == 0.0 and not math.copysign(1.0, got) < 0, v
        else:
            assert math.isfinite(got) and got >= 0.0 and not math.copysign(1.0, got) < 0, v
            assert got == math.exp(v)
            assert (got < 2.0 ** -1022) == (v in xc.R3_SUBNORMAL), v
            assert float(xc.ulp_error(np.array([got]), xc.exp_ref(np.array([v])))[0]) <= 1.0, v
    # sinh's classes at |v| >= 710 in the restatement: g = +-inf, g' = +inf
    with np.errstate(all="ignore"):
        g, gp = nref.g_gp("sinh", np.array([710.0, -710.0, 1e308, -1e308, math.inf, -math.inf]))
    assert np.array_equal(g, [math.inf, -math.inf] * 3) and np.all(gp == math.inf)


def test_restated_exp_libm_is_the_algorithm_of_the_header():
    """tests/_exp_cases.py restates csrc/mg_exp_libm.h with the C library's fma and no exp(): its table, computed from the
    definition, is csrc/mg_exp_table.h's; its constants are the header's; its largest error by the reference stays inside the
    0.511 ulp its authors give for the algorithm (0.509 with fma); how many arguments it and this host's exp() disagree on is
    printed (0 on glibc >= 2.28, which runs this algorithm)."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multigrid_poisson_solver_amd", "csrc")
    with open(os.path.join(csrc, "mg_exp_table.h")) as f:
        vals = np.array([int(v, 16) for v in re.findall(r"0x([0-9a-f]{16})ull", f.read())], dtype=np.uint64)
    assert vals.size == 256 and np.array_equal(vals, xc.exp_table())
    with open(os.path.join(csrc, "mg_exp_libm.h")) as f:
        body = f.read()
    with open(xc.__file__) as f:
        mine = f.read()
    consts = re.findall(r"-?0x1\.[0-9a-f]+p[+-]\d+", body)
    assert len(consts) == 8 and all(c in mine for c in consts), consts
    x = np.concatenate([xc.r2(), xc.r1()])
    y = xc.exp_libm_restated(x)
    err = float(np.max(xc.ulp_error(y, xc.exp_ref(x))))
    differ = int(np.sum(y.view(np.uint64) != xc.host_exp(x).view(np.uint64)))
    print(f"exp_libm restated on {x.size} arguments: largest error {err:.4f} ulp; differs from this host's exp() on {differ}")
    assert err <= 0.511
    assert np.all(y[-xc.r1().size:] == 1.0)
