"""The argument set that holds exp_libm (csrc/mg_exp_libm.h) to a reference over its whole domain, built regime by regime and
deterministic, with the reference exp in longdouble (64-bit mantissa) and an ulp measure on the double grid.  Shared by
tests/test_newton_exp_domain_cpu.py and tests/test_newton_exp_domain_gpu.py.  TEST INFRASTRUCTURE.

exp_libm(x) = 2^(k/128) * exp(r) with k = round(x*128/ln 2), r = x - k*ln2/128: k mod 128 selects the table entry, k >> 7 the
exponent.
  R2  2^-54 <= |x| < 512   the verified path: every k at three points of its reduction interval, log-uniform magnitudes, edges
  R1  |x| < 2^-54          the 1.0 + x branch
  R3  |x| >= 512           the device library's exp(): overflow, underflow, subnormal results, inf, NaN"""
import math

import numpy as np

LD = np.longdouble
LN2_LD = np.log(LD(2))
K_PER_UNIT = LD(128) / LN2_LD          # k = round(x * 128/ln 2)
TINY = 2.0 ** -54                      # below it exp_libm returns 1.0 + x
BIG = 512.0                            # from it on exp_libm returns the device library's exp()
EXP_MAX = 709.782712893384             # the largest double whose exp is finite (tests/_newton_ref.py)
N_LOG = 60000                          # log-uniform magnitudes per sign
TIE = LD("0.4999999")                  # just inside the tie edges of a reduction interval

R1_VALUES = (0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, math.nextafter(TINY, 0.0), -math.nextafter(TINY, 0.0))
R2_EDGES = (TINY, -TINY, math.nextafter(BIG, 0.0), -math.nextafter(BIG, 0.0))
R3_OVER = (math.nextafter(EXP_MAX, math.inf), 710.0, 1e308, math.inf)                 # exp = +inf
R3_ZERO = (-746.0, -1e308, -math.inf)                                                 # exp = +0
R3_FINITE = (512.0, -512.0, 600.0, -600.0, 700.0, -700.0, EXP_MAX, -708.4, -745.13, -745.14)   # finite and not zero
R3_SUBNORMAL = (-708.4, -745.13, -745.14)                                             # of those: subnormal results
R3_VALUES = R3_FINITE + R3_OVER + R3_ZERO + (math.nan,)


def k_of(x):
    """round(x*128/ln 2) as exp_libm forms it (ties aside, which the set stays clear of), int64"""
    return np.rint(np.asarray(x, dtype=LD) * K_PER_UNIT).astype(np.int64)


def k_range():
    """every k an |x| < 512 reaches: -K .. K"""
    K = int(k_of(math.nextafter(BIG, 0.0)))
    return np.arange(-K, K + 1, dtype=np.int64)


_cache = {}


def r2():
    """the R2 arguments, float64, in a fixed order: per k (one random point, the low tie edge, the high tie edge), then the
    log-uniform magnitudes of both signs, then the edges.  Read-only, built once."""
    if "r2" not in _cache:
        rng = np.random.default_rng(20240)
        ks = k_range().astype(LD)
        per_k = []
        for off in (LD(1) * (rng.random(ks.size).astype(LD) - LD(0.5)) * LD(0.999), -TIE, TIE):
            per_k.append(((ks + off) / K_PER_UNIT).astype(np.float64))
        x = np.stack(per_k, axis=1).reshape(-1)
        x = x[(np.abs(x) >= TINY) & (np.abs(x) < BIG)]       # (k = 0's low-magnitude points and the last k's far edge may fall out)
        mag = np.exp2(rng.uniform(-54.0, 9.0, N_LOG))
        mag = mag[(mag >= TINY) & (mag < BIG)]
        out = np.concatenate([x, mag, -mag, np.array(R2_EDGES)])
        out.setflags(write=False)
        _cache["r2"] = out
    return _cache["r2"]


def r1():
    return np.array(R1_VALUES)


def r3():
    return np.array(R3_VALUES)


def field(values, N, start=0):
    """(U, n): the N x N field, rim included, that holds values[start:start + n] row by row, n = min(N*N, what is left), the rest
    filled with repeats of that slice; point p < n of U.reshape(-1) is values[start + p]"""
    values = np.asarray(values, dtype=np.float64)
    n = min(N * N, values.size - start)
    assert n > 0
    return np.resize(values[start:start + n], N * N).reshape(N, N).copy(), n


def calls(values, N):
    """the start offsets that carry all of values through N x N fields"""
    return list(range(0, len(values), N * N))


def patches(values, N):
    """(U, rows, cols): values laid out in constant 3 x 3 patches, so that at a patch's centre the point and its four neighbours
    are equal and a constant-coefficient five-point stencil with shift 0 gives exactly zero; rows, cols index the centres, in
    the order of values.  Points no patch covers hold 0.  Needs (N // 3)^2 >= len(values)."""
    values = np.asarray(values, dtype=np.float64)
    m = N // 3
    assert m * m >= values.size, (N, values.size)
    idx = np.arange(values.size)
    rows, cols = 3 * (idx // m) + 1, 3 * (idx % m) + 1
    U = np.zeros((N, N))
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            U[rows + dr, cols + dc] = values
    return U, rows, cols


# ---------------------------------------------------------------- the reference and the ulp measure
MIN_NORMAL = LD(2) ** -1022
SUB_SPACING = LD(2) ** -1074
DBL_MAX = LD(np.finfo(np.float64).max)


def exp_ref(x):
    """exp in longdouble (64-bit mantissa) of float64 arguments: error below 2^-10 ulp of a double
    (test_newton_exp_domain_cpu.py holds it against mpmath at 200 bits)"""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.asarray(x, dtype=np.float64).astype(LD))


def spacing(true):
    """the spacing of the double grid at the true value `true` (longdouble, positive and finite): 2^(e-52) in the binade
    2^e <= true < 2^(e+1), 2^-1074 where the result is subnormal"""
    true = np.asarray(true, dtype=LD)
    _, e = np.frexp(np.maximum(true, MIN_NORMAL))         # true = m * 2^e, 0.5 <= m < 1
    return np.where(true < MIN_NORMAL, SUB_SPACING, np.ldexp(LD(1), e - 1 - 52))


def ulp_error(got, true):
    """|got - true| in units of spacing(true), longdouble; got float64, true longdouble, both finite"""
    return np.abs(np.asarray(got, dtype=np.float64).astype(LD) - true) / spacing(true)


def host_exp(x):
    """math.exp per element: the host libm, +inf instead of OverflowError"""
    def one(v):
        try:
            return math.exp(v)
        except OverflowError:
            return math.inf
    x = np.asarray(x, dtype=np.float64)
    return np.fromiter(map(one, x.reshape(-1).tolist()), dtype=np.float64, count=x.size).reshape(x.shape)


# ---------------------------------------------------------------- exp_libm restated, libm's exp() not in it
def exp_table():
    """the 128 x 2 table of csrc/mg_exp_table.h from its definition (scripts/gen_exp_table.py): for k = 0..127, H = RN(2^(k/128)),
    T = RN((2^(k/128) - H)/H); entry 2k = bits(T), entry 2k + 1 = bits(H) - (k << 52)/128.  uint64[256]"""
    from decimal import Decimal, getcontext
    import struct
    getcontext().prec = 80
    tab = []
    for k in range(128):
        v = Decimal(2) ** (Decimal(k) / Decimal(128))
        H = float(v)
        T = float((v - Decimal(H)) / Decimal(H))
        tab += [struct.unpack("<Q", struct.pack("<d", T))[0], struct.unpack("<Q", struct.pack("<d", H))[0] - ((k << 52) // 128)]
    return np.array(tab, dtype=np.uint64)


def _fma():
    """fma(a, b, c) per element with ONE rounding: the C library's fma(), which C99 and IEEE 754 define exactly (unlike exp(),
    whose last bit is each libm's own), so the restatement below gives the same bits on every host"""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    assert libm.fma(2.0 ** 27 + 1.0, 2.0 ** 27 + 1.0, -(2.0 ** 54)) == 2.0 ** 28 + 1.0    # (a product of 55 bits, kept whole)
    return np.frompyfunc(libm.fma, 3, 1)


def exp_libm_restated(x):
    """csrc/mg_exp_libm.h operation by operation on 2^-54 <= |x| < 512 (R2) and 1.0 + x below: numpy for the operations that
    round once by themselves, the C library's fma for the fused ones.  A reference for exp_libm's BITS that does not depend on
    the host's exp()."""
    x = np.asarray(x, dtype=np.float64)
    assert np.all(np.abs(x) < BIG)
    fma = lambda a, b, c: _fma()(a, b, c).astype(np.float64)
    f = float.fromhex
    InvLn2N, Shift, NegLn2hiN, NegLn2loN = f("0x1.71547652b82fep+7"), f("0x1.8p+52"), f("-0x1.62e42fefa0000p-8"), f("-0x1.cf79abc9e3b3ap-47")
    C2, C3, C4, C5 = f("0x1.ffffffffffdbdp-2"), f("0x1.555555555543cp-3"), f("0x1.55555cf172b91p-5"), f("0x1.1111167a4d017p-7")
    tab = exp_table()
    kd_s = fma(x, InvLn2N, Shift)
    ki = kd_s.view(np.uint64)
    kd = kd_s - Shift
    r = fma(kd, NegLn2hiN, x)
    r = fma(kd, NegLn2loN, r)
    idx = 2 * (ki & np.uint64(127)).astype(np.int64)
    tail = tab[idx].view(np.float64)
    sbits = tab[idx + 1] + (ki << np.uint64(45))          # (uint64: wraps as the device's does)
    p23 = fma(r, C3, C2)
    rt = r + tail
    r2 = r * r
    p45 = fma(r, C5, C4)
    t = fma(p23, r2, rt)
    r4 = r2 * r2
    tmp = fma(r4, p45, t)
    scale = sbits.view(np.float64)
    out = fma(scale, tmp, scale)
    return np.where(np.abs(x) < TINY, 1.0 + x, out)
