"""The exact side of the device math tests and their inputs (test_device_math.py checks this module, test_gpu_device_math.py uses it).
It never imports the library.

Reference: numpy.longdouble (x86 80-bit, 64-bit significand): sinl / cosl / atanl / asinl of the argument taken as the exact double it is.
Eleven extra bits resolve an f64 error to about 0.001 unit; the tests compare in tenths.  The degree forms reduce exactly first
(deg - 90 n is exact for |deg| < 2^53 in f64 and in long double; beyond, deg is an integer and Python's integers reduce it), multiply the
remainder by pi/180 in long double and set exact multiples of 90 to exact 0 and +-1 with the signs MATLAB's reduction gives them
(oracle em_sincosd; tests/golden/matlab/trig_table.csv).  round500 and 1/d are numpy f64 (IEEE, correctly rounded).

Error measures: `units` = |got - exact| in units of 2^-53 (absolute: every sine and cosine); `ulps` = |got - exact| in ulps of the EXACT
result, the f64 spacing at its magnitude (atan, asin, 1/d and sincos_small's sine, which owe relative accuracy near 0)."""
import os
from fractions import Fraction

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant == 63, "the reference needs the x86 80-bit long double"

# emgpu_debug_device_math's fn by number (EMGPU_MATH_*, include/emgpu.h)
FUNCTIONS = ("sincos_small", "sincos_small_sk", "sincosd_small", "t_sincosd", "f_sincosd", "ut_sincos", "ut_sincos_sk", "ut_atan",
             "ut_atan_sk", "ut_asin_small", "ut_asin_small_sk", "ut_rcp", "round500")
PAIRS = FUNCTIONS[:7]                      # the functions with two results (sine, cosine)
TWINS = (("sincos_small", "sincos_small_sk"), ("ut_sincos", "ut_sincos_sk"), ("ut_atan", "ut_atan_sk"), ("ut_asin_small", "ut_asin_small_sk"))
# the input set each function is run on
FAMILY = {"sincos_small": "sincos_small", "sincos_small_sk": "sincos_small", "sincosd_small": "sincosd", "t_sincosd": "sincosd",
          "f_sincosd": "sincosd", "ut_sincos": "ut_sincos", "ut_sincos_sk": "ut_sincos", "ut_atan": "ut_atan", "ut_atan_sk": "ut_atan",
          "ut_asin_small": "ut_asin_small", "ut_asin_small_sk": "ut_asin_small", "ut_rcp": "ut_rcp", "round500": "round500"}
FAMILIES = ("sincos_small", "sincosd", "ut_sincos", "ut_atan", "ut_asin_small", "ut_rcp", "round500")

DBL_MIN, DBL_MAX, DENORM_MIN = 2.0 ** -1022, float(np.finfo(np.float64).max), 5e-324
SPECIALS = np.array([0.0, -0.0, DENORM_MIN, 1e-310, DBL_MIN, -DBL_MIN, np.nan, np.inf, -np.inf, DBL_MAX, -DBL_MAX])
N_RANDOM = 1 << 17
PI_LD = LD(4) * np.arctan(LD(1))
PI4 = float(np.pi / 4)
K_MAX = 63661                              # every k with |k pi/2| < 1e5
TRIG_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matlab", "trig_table.csv")

_cache = {}


def neighbours(x, k):
    """x with its k neighbours on each side, in order: 2k + 1 doubles per element, [len(x), 2k + 1]"""
    x = np.asarray(x, dtype=np.float64)
    cols = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cols = [lo] + cols + [hi]
    return np.stack(cols, axis=-1)


def both_signs(x):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return np.concatenate([x, -x])


def trig_table():
    """tests/golden/matlab/trig_table.csv: [rows, 3] = angle in degrees, the oracle's sind, cosd (the signs of its zeros kept)"""
    if "csv" not in _cache:
        t = np.loadtxt(TRIG_TABLE, delimiter=",", comments="%")
        t.setflags(write=False)
        _cache["csv"] = t
    return _cache["csv"]


def _parts(family):
    """the named pieces of a family's input set, in order (the CPU test counts them)"""
    rs = np.random.RandomState(20261021 + FAMILIES.index(family))
    sign = lambda n: np.where(rs.randint(0, 2, n) == 0, -1.0, 1.0)          # noqa: E731
    P = [("specials", SPECIALS)]
    if family == "sincos_small":
        P += [("pi/4", neighbours(both_signs([PI4]), 1)),
              ("tiny", both_signs(2.0 ** -np.array([27.0, 28, 30, 40, 100, 500, 1000]))),      # s = x and c = 1 exactly
              ("random", rs.uniform(-PI4, PI4, N_RANDOM))]
    elif family == "ut_sincos":
        k = np.arange(-K_MAX, K_MAX + 1)
        centre = (k.astype(LD) * (PI_LD / 2)).astype(np.float64)
        P += [("k pi/2", neighbours(centre, 2)),
              ("1e5", neighbours(both_signs([1.0e5]), 2)),
              ("fallback", both_signs(np.concatenate([10.0 ** np.arange(5, 23), [2.0 ** 1023]]))),
              ("fallback random", sign(4096) * 10.0 ** rs.uniform(5.0, 22.0, 4096)),
              ("random", rs.uniform(-1.0e5, 1.0e5, N_RANDOM))]
    elif family == "sincosd":
        j = np.arange(0, 44)                                                 # 360 * 2^43 + 90 < 2^52
        P += [("k 45", neighbours(45.0 * np.arange(-4000, 4001), 2)),
              ("csv", trig_table()[:, 0]),
              ("360 2^j +- 90", both_signs(np.concatenate([360.0 * 2.0 ** j + 90.0, 360.0 * 2.0 ** j - 90.0]))),
              ("beyond 2^53", both_signs([2.0 ** 53, 2.0 ** 53 + 2.0, 1.0e17, 2.0 ** 60, 90.0 * 2.0 ** 62])),
              ("beyond 90 2^63", both_signs([90.0 * 2.0 ** 63, 1.0e21, 1.0e22, 2.0 ** 80, 1.0e300])),
              ("random", np.concatenate([rs.uniform(-1080.0, 1080.0, N_RANDOM // 2),
                                         sign(N_RANDOM // 2) * 2.0 ** rs.uniform(0.0, 53.0, N_RANDOM // 2)]))]
    elif family == "ut_atan":
        P += [("breakpoints", both_signs(neighbours([7.0 / 16, 11.0 / 16, 19.0 / 16, 39.0 / 16], 3))),
              ("powers of two", both_signs(2.0 ** np.arange(-1070.0, 1024.0))),
              ("random", np.concatenate([rs.uniform(-4.0, 4.0, N_RANDOM // 2), sign(N_RANDOM // 2) * 2.0 ** rs.uniform(-40.0, 40.0, N_RANDOM // 2)]))]
    elif family == "ut_asin_small":
        P += [("0.5", both_signs(neighbours([0.5], 3)[:, :4])),             # 0.5 (the first value outside) and three neighbours inside
              ("powers of two", both_signs(2.0 ** -np.arange(2.0, 1075.0))),
              ("random", rs.uniform(-0.5, 0.5, N_RANDOM))]
    elif family == "ut_rcp":
        P += [("powers of two", both_signs(2.0 ** np.arange(-1074.0, 1024.0))),
              ("random", sign(N_RANDOM) * np.ldexp(1.0 + rs.uniform(0.0, 1.0, N_RANDOM), rs.randint(-1021, 1022, N_RANDOM))),
              ("subnormal", sign(256) * rs.randint(1, 1 << 52, 256).astype(np.float64) * DENORM_MIN),
              ("subnormal reciprocal", sign(256) * (2.0 ** 1022 * (1.0 + rs.uniform(2.0 ** -40, 1.0, 256))))]
    elif family == "round500":
        P += [("multiples of 250", neighbours(250.0 * np.arange(-40, 41), 1)),
              ("1e15", neighbours([1.0e15], 1)),
              ("random", rs.uniform(-60000.0, 60000.0, N_RANDOM))]
    else:
        raise KeyError(family)
    return [(name, np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))) for name, v in P]


def parts(family):
    key = ("parts", family)
    if key not in _cache:
        _cache[key] = _parts(family)
        for _, v in _cache[key]:
            v.setflags(write=False)
    return _cache[key]


def inputs(family):
    """the family's whole input set, built once and shared read-only"""
    key = ("inputs", family)
    if key not in _cache:
        x = np.concatenate([v for _, v in parts(family)])
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def in_domain(family, x):
    """the arguments the function's header comment promises its accuracy for"""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    with np.errstate(invalid="ignore"):
        if family == "sincos_small":
            return fin & (np.abs(x) <= np.nextafter(PI4, 1.0))              # pi/4 and the ulp beyond it that a reduction's rounding leaves
        if family == "sincosd":
            return fin & (np.abs(x) < 2.0 ** 53)
        if family == "ut_asin_small":
            return fin & (np.abs(x) < 0.5)
        if family == "ut_rcp":
            return fin & (np.abs(x) >= DBL_MIN) & (np.abs(x) <= 2.0 ** 1022)     # normal, with a normal reciprocal
        return fin                                                          # ut_sincos, ut_atan, round500: every finite x


def round_half_away(q):
    """C's round() on f64"""
    q = np.asarray(q, dtype=np.float64)
    a = np.abs(q)
    f = np.floor(a)
    return np.copysign(f + (a - f >= 0.5), q)


def sincosd_exact(deg):
    """(sin, cos) of deg degrees as long doubles; NaN for a non-finite argument"""
    deg = np.asarray(deg, dtype=np.float64)
    r = np.full(deg.shape, np.nan, dtype=LD)
    m = np.zeros(deg.shape, dtype=np.int64)
    fin = np.isfinite(deg)
    small = fin & (np.abs(deg) < 2.0 ** 53)
    n = round_half_away(deg[small] / 90.0)
    r[small] = deg[small].astype(LD) - LD(90) * n.astype(LD)                # exact: both are multiples of ulp(deg) below 2^64
    m[small] = n.astype(np.int64) & 3
    for i in np.flatnonzero(fin & ~small):                                  # an integer: reduced in Python's integers
        D = int(deg[i])
        q = (2 * D + 90) // 180
        r[i], m[i] = LD(D - 90 * q), q & 3
    with np.errstate(invalid="ignore"):
        x = r * (PI_LD / LD(180))
        sx, cx = np.sin(x), np.cos(x)
    zero = r == 0
    sx[zero], cx[zero] = LD(0), LD(1)                                       # exact at every multiple of 90
    s = np.where(m == 0, sx, np.where(m == 1, cx, np.where(m == 2, -sx, -cx)))
    c = np.where(m == 0, cx, np.where(m == 1, -sx, np.where(m == 2, -cx, sx)))
    return s, c


def sincosd_quotients(deg):
    """the two reduction quotients in f64 as the device forms them (IEEE multiply, divide and round): round(deg * (1/90)) of sincosd_small and
    t_sincosd, round(deg / 90) of f_sincosd and the oracle"""
    deg = np.asarray(deg, dtype=np.float64)
    return round_half_away(deg * (1.0 / 90.0)), round_half_away(deg / 90.0)


def round500(num):
    """UncorEncounterModel.m:196: round500 = @(num) 500 * (floor(num / 500) + (mod(num, 500) > 250)), MATLAB's mod being the floored one"""
    num = np.asarray(num, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return 500.0 * (np.floor(num / 500.0) + (np.mod(num, 500.0) > 250.0))


def exact(family, x):
    """the exact results for x as a tuple of arrays: (sin, cos) long doubles for the pairs, (value,) otherwise (f64 for ut_rcp, round500)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if family in ("sincos_small", "ut_sincos"):
            return np.sin(x.astype(LD)), np.cos(x.astype(LD))
        if family == "sincosd":
            return sincosd_exact(x)
        if family == "ut_atan":
            return (np.arctan(x.astype(LD)),)
        if family == "ut_asin_small":
            return (np.arcsin(x.astype(LD)),)
        if family == "ut_rcp":
            return (1.0 / x,)
        if family == "round500":
            return (round500(x),)
    raise KeyError(family)


def reference(family):
    """exact(family, inputs(family)), computed once and shared read-only"""
    key = ("exact", family)
    if key not in _cache:
        out = exact(family, inputs(family))
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def units(got, want):
    """|got - want| in units of 2^-53 (long double); nan where either is"""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(got).astype(LD) - np.asarray(want).astype(LD)) * LD(2.0 ** 53)


def ulp_of(want):
    """the f64 spacing at the magnitude of the exact result (2^-1074 in the subnormal range and at 0)"""
    w = np.abs(np.asarray(want).astype(LD))
    with np.errstate(invalid="ignore"):
        _, e = np.frexp(np.where(np.isfinite(w) & (w > 0), w, LD(1)))       # |w| = m 2^e, m in [0.5, 1)
    e = np.where(w > 0, e.astype(np.int64), -10000)
    return np.ldexp(LD(1), np.maximum(e - 53, -1074).astype(np.int32))


def ulps(got, want):
    """|got - want| in ulps of want"""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(got).astype(LD) - np.asarray(want).astype(LD)) / ulp_of(want)


def worst(err, x, mask):
    """(the largest error over the masked elements, its argument); a NaN among them counts as infinite"""
    e = np.where(np.isnan(err), np.inf, err).astype(np.float64)
    e = np.where(mask, e, -1.0)
    i = int(np.argmax(e))
    return float(e[i]), float(x[i])


def same_bits(a, b):
    """a == b bit for bit, any NaN equal to any NaN; returns the indices that differ"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.flatnonzero((na != nb) | (~na & ~nb & (a.view(np.int64) != b.view(np.int64))))


def mp_exact(family, x):
    """the exact results at 60 digits (mpmath), one tuple per argument; the degree forms reduce in exact rationals first"""
    import mpmath as mp
    mp.mp.dps = 60
    out = []
    for v in np.asarray(x, dtype=np.float64):
        v = float(v)
        if family in ("sincos_small", "ut_sincos"):
            out.append((mp.sin(mp.mpf(v)), mp.cos(mp.mpf(v))))
        elif family == "sincosd":
            f = Fraction(v) % 360
            a = mp.mpf(f.numerator) / mp.mpf(f.denominator) * mp.pi / 180
            out.append((mp.sin(a), mp.cos(a)))
        elif family == "ut_atan":
            out.append((mp.atan(mp.mpf(v)),))
        elif family == "ut_asin_small":
            out.append((mp.asin(mp.mpf(v)),))
        elif family == "ut_rcp":
            out.append((1 / mp.mpf(v),))
        else:
            raise KeyError(family)
    return out


def to_mp(v):
    """a long double as an mpmath number, exactly"""
    import mpmath as mp
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(LD(v) - LD(hi)))
