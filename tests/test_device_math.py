"""CPU: the yardstick of test_gpu_device_math.py (device_math_ref.py) checked on its own -- the input sets hold what they are meant to,
the long-double reference agrees with mpmath at 60 digits and reproduces the oracle's trig_table.csv -- and every refusal of
emgpu_debug_device_math, all of which come before any device work.  Nothing here evaluates a device function."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import device_math_ref as R
from em_model_manned_bayes_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the pieces of every input set and their sizes, written out: a piece that loses or gains an element fails here
SIZES = {
    "sincos_small": {"specials": 11, "pi/4": 6, "tiny": 14, "random": 1 << 17},
    "ut_sincos": {"specials": 11, "k pi/2": 5 * (2 * 63661 + 1), "1e5": 10, "fallback": 38, "fallback random": 4096, "random": 1 << 17},
    "sincosd": {"specials": 11, "k 45": 5 * 8001, "csv": 350, "360 2^j +- 90": 176, "beyond 2^53": 10, "beyond 90 2^63": 10, "random": 1 << 17},
    "ut_atan": {"specials": 11, "breakpoints": 56, "powers of two": 2 * 2094, "random": 1 << 17},
    "ut_asin_small": {"specials": 11, "0.5": 8, "powers of two": 2 * 1073, "random": 1 << 17},
    "ut_rcp": {"specials": 11, "powers of two": 2 * 2098, "random": 1 << 17, "subnormal": 256, "subnormal reciprocal": 256},
    "round500": {"specials": 11, "multiples of 250": 3 * 81, "1e15": 3, "random": 1 << 17},
}


def _has(x, v):
    """v is among x, by its bits (-0.0 is not 0.0; a NaN is any NaN)"""
    return bool(len(x)) and len(R.same_bits(x, np.full(len(x), v))) < len(x)


def test_the_function_numbers_are_the_headers_and_the_librarys():
    hdr = open(os.path.join(ROOT, "include", "emgpu.h")).read()
    numbers = {name.lower(): int(num) for name, num in re.findall(r"#define EMGPU_MATH_([A-Z0-9_]+) (\d+)", hdr)}
    assert numbers == {name: i for i, name in enumerate(R.FUNCTIONS)}
    assert tuple(L.MATH_FUNCTIONS) == R.FUNCTIONS
    assert set(R.FAMILY) == set(R.FUNCTIONS) and set(R.FAMILY.values()) == set(R.FAMILIES)
    assert all(a in R.FUNCTIONS and b in R.FUNCTIONS and R.FAMILY[a] == R.FAMILY[b] for a, b in R.TWINS)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_the_input_sets_hold_what_they_list(family):
    parts = dict(R.parts(family))
    assert {name: len(v) for name, v in parts.items()} == SIZES[family]
    x = R.inputs(family)
    assert len(x) == sum(SIZES[family].values()) and R.inputs(family) is x and not x.flags.writeable
    for v in R.SPECIALS:                                          # every special, -0.0 apart from 0.0
        assert _has(parts["specials"], v), v
    for name, v in parts.items():                                 # no piece repeats a value (a piece built twice, a neighbour that did not move)
        if name != "specials":
            assert len(np.unique(v.view(np.int64))) == len(v), name
    dom = R.in_domain(family, parts["random"])
    assert dom.all(), "the random arguments are drawn over the documented domain"
    if family == "sincos_small":
        p4 = float(np.pi / 4)
        for v in (p4, -p4, np.nextafter(p4, 0), np.nextafter(p4, 1), np.nextafter(-p4, 0), np.nextafter(-p4, -1), 2.0 ** -27, -2.0 ** -1000):
            assert _has(x, v), v
    if family == "ut_sincos":
        kp = parts["k pi/2"].reshape(-1, 5)
        assert (np.diff(kp, axis=1) > 0).all() and (np.abs(kp) < 1.0e5).all()
        k = np.arange(-R.K_MAX, R.K_MAX + 1)
        assert (np.abs(kp[:, 2].astype(R.LD) - k * (R.PI_LD / 2)) <= np.spacing(np.abs(kp[:, 2])) / 2).all()      # the nearest double
        assert (R.K_MAX + 1) * np.pi / 2 > 1.0e5                  # ... of every k below 1e5
        assert kp[R.K_MAX, 2] == 0.0 and kp[R.K_MAX, 3] == R.DENORM_MIN
        for v in (1.0e5, np.nextafter(1.0e5, 0), np.nextafter(1.0e5, np.inf), -1.0e5, np.nextafter(-1.0e5, 0), 1.0e22, -1.0e22, 2.0 ** 1023):
            assert _has(x, v), v
        assert (np.abs(parts["fallback random"]) >= 1.0e5).all()
    if family == "sincosd":
        k45 = parts["k 45"].reshape(-1, 5)
        assert np.array_equal(k45[:, 2], 45.0 * np.arange(-4000, 4001)) and (np.diff(k45, axis=1) > 0).all()
        for v in R.trig_table()[:, 0]:
            assert _has(parts["csv"], v)
        for v in (450.0, 270.0, 360.0 * 2.0 ** 43 + 90.0, -(360.0 * 2.0 ** 43 - 90.0), 2.0 ** 53, 90.0 * 2.0 ** 63, -1.0e300):
            assert _has(x, v), v
        assert 360.0 * 2.0 ** 43 + 90.0 < 2.0 ** 52 < 360.0 * 2.0 ** 44
        assert R.in_domain(family, parts["360 2^j +- 90"]).all() and not R.in_domain(family, parts["beyond 2^53"]).any()
        assert (np.abs(parts["beyond 90 2^63"]) >= 90.0 * 2.0 ** 63).all()
    if family == "ut_atan":
        bp = parts["breakpoints"].reshape(2, 4, 7)
        assert np.array_equal(bp[0, :, 3], [0.4375, 0.6875, 1.1875, 2.4375]) and np.array_equal(bp[1], -bp[0]) and (np.diff(bp[0], axis=1) > 0).all()
        assert _has(x, 2.0 ** -1070) and _has(x, 2.0 ** 1023) and _has(x, -2.0 ** 1023)
    if family == "ut_asin_small":
        assert np.array_equal(np.sort(np.abs(parts["0.5"]))[-2:], [0.5, 0.5])
        assert R.in_domain(family, parts["0.5"]).sum() == 6 and _has(x, np.nextafter(0.5, 0)) and _has(x, -np.nextafter(0.5, 0))
    if family == "ut_rcp":
        assert _has(x, 2.0 ** -1074) and _has(x, 2.0 ** 1023) and _has(x, 2.0 ** 1022) and _has(x, 2.0 ** -1022)
        assert (np.abs(parts["subnormal"]) < R.DBL_MIN).all() and (parts["subnormal"] != 0).all()
        with np.errstate(under="ignore"):
            assert (np.abs(1.0 / parts["subnormal reciprocal"]) < R.DBL_MIN).all()
        e = np.frexp(parts["random"])[1] - 1
        assert e.min() == -1021 and e.max() == 1021
    if family == "round500":
        m = parts["multiples of 250"].reshape(-1, 3)
        assert np.array_equal(m[:, 1], 250.0 * np.arange(-40, 41)) and _has(x, 1.0e15) and (parts["random"] < 0).any()


def _subset(family, n=2000):
    """n arguments of the family's set: every structured piece strided, the rest from the random piece; the finite ones"""
    parts = R.parts(family)
    fixed = np.concatenate([v for name, v in parts if name not in ("random", "k pi/2", "k 45")])
    big = [v for name, v in parts if name in ("k pi/2", "k 45")]
    pick = [fixed[:: max(1, len(fixed) // 700)]] + [v[:: len(v) // 600] for v in big]
    have = sum(len(v) for v in pick)
    pick.append(dict(parts)["random"][: n - have])
    x = np.concatenate(pick)
    assert len(x) == n
    return x


@pytest.mark.parametrize("family", [f for f in R.FAMILIES if f != "round500"])      # (round500's reference is exact IEEE arithmetic: nothing to resolve)
def test_the_long_double_reference_agrees_with_mpmath(family):
    """The yardstick, not the library: |long double - mpmath at 60 digits| <= 0.01 of the unit the GPU test measures in (1/d is numpy's f64
    quotient: correctly rounded, at most half an ulp)."""
    pytest.importorskip("mpmath")
    x = _subset(family)
    want = R.exact(family, x)
    fin = np.isfinite(x) & ((np.abs(x) <= 1) | (family != "ut_asin_small"))      # where the function exists
    if family == "ut_rcp":
        fin &= np.abs(x) >= 2.0 ** -1024                          # ... and its value is finite in f64
    assert fin.sum() >= 1900
    for a in want:
        if family != "ut_rcp":
            assert np.isnan(np.asarray(a, dtype=np.float64)[~fin]).all()
    xs = x[fin]
    mp = R.mp_exact(family, xs)
    worst = 0.0
    for j, v in enumerate(xs):
        for r in range(len(want)):
            w = want[r][fin][j]
            exact = mp[j][r]
            diff = abs(R.to_mp(w) - exact)
            if family == "ut_rcp":
                err, bound = diff / R.to_mp(R.ulp_of(np.array([float(exact)]))[0]), 0.5
            elif family in ("ut_atan", "ut_asin_small") or (family == "sincos_small" and r == 0):
                err, bound = diff / R.to_mp(R.ulp_of(np.array([w]))[0]), 0.01
            else:
                err, bound = diff * 2 ** 53, 0.01
            worst = max(worst, float(err))
            assert err <= bound, (family, float(v).hex(), r, float(err))
    print("%s: long double against mpmath, worst %.5f" % (family, worst))


def test_the_reference_reproduces_the_oracles_trig_table():
    """At the multiples of 90 exactly, the signs of the zeros included; elsewhere to one unit of 2^-53 (the golden is the host libm's)."""
    t = R.trig_table()
    s, c = R.sincosd_exact(t[:, 0])
    at90 = np.fmod(t[:, 0], 90.0) == 0
    assert at90.sum() == 17 and len(t) == 350
    assert not len(R.same_bits(s[at90].astype(np.float64), t[at90, 1])) and not len(R.same_bits(c[at90].astype(np.float64), t[at90, 2]))
    assert np.signbit(t[t[:, 0] == 90.0, 2]).all() and np.signbit(t[t[:, 0] == 180.0, 1]).all()      # `90,1,-0` and `180,-0,-1`
    assert R.units(t[:, 1], s).max() <= 1.0 and R.units(t[:, 2], c).max() <= 1.0


def test_the_two_reduction_quotients_differ_only_at_ties():
    """round(deg * (1/90)) (sincosd_small, t_sincosd) against round(deg / 90) (f_sincosd, the oracle) over the in-domain degree set: they
    differ on some k * 90 + 45, where both remainders (+45 and -45 of neighbouring quadrants) name the same angle, and nowhere else."""
    x = R.inputs("sincosd")
    x = x[R.in_domain("sincosd", x)]
    n_mul, n_div = R.sincosd_quotients(x)
    diff = n_mul != n_div
    assert diff.any()
    assert (np.abs(np.abs(x[diff] - 90.0 * n_div[diff]) - 45.0) <= np.spacing(np.abs(x[diff]))).all()      # a tie, or the double next to one
    assert (np.abs(n_mul - n_div)[diff] == 1).all()
    print("sincosd: %d of %d angles reduce to different quadrants (%d of them exact ties k * 90 + 45)"
          % (diff.sum(), len(x), (np.abs(x[diff] - 90.0 * n_div[diff]) == 45.0).sum()))


def test_round500_restates_the_floored_mod():
    assert np.array_equal(R.round500([0.0, 249.0, 250.0, 250.5, 500.0, 749.0, 751.0, -100.0, -250.0, -251.0, -500.0]),
                          [0.0, 0.0, 0.0, 500.0, 500.0, 500.0, 1000.0, 0.0, -500.0, -500.0, -500.0])


def _call(fn, n, x, out0, out1):
    lib = L.lib()
    rc = lib.emgpu_debug_device_math(None, fn, n, x, out0, out1)
    return rc, lib.emgpu_last_error()


def test_every_refusal_comes_before_any_device_work():
    """An unknown fn, a negative n, a null x or out0 and a pointer off an 8-byte boundary are EMGPU_ERR_ARG; n == 0 is EMGPU_OK without a
    launch (the pointers are host memory here: nothing may touch them)."""
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    assert _call(0, 0, p, p + 8, p + 16)[0] == L.OK and _call(12, 0, p, p + 8, None)[0] == L.OK
    for fn in (-1, 13, 1 << 30):
        assert _call(fn, 1, p, p + 8, p + 16) == (L.ERR_ARG, b"no such function: fn outside 0..12")
    assert _call(0, -1, p, p + 8, p + 16) == (L.ERR_ARG, b"n outside 0..2^32")
    assert _call(0, (1 << 32) + 1, p, p + 8, p + 16) == (L.ERR_ARG, b"n outside 0..2^32")
    assert _call(0, 1, None, p + 8, p + 16) == (L.ERR_ARG, b"null argument: x")
    assert _call(0, 1, p, None, p + 16) == (L.ERR_ARG, b"null argument: out0")
    for args in ((p + 4, p + 8, p + 16), (p, p + 12, p + 16), (p, p + 8, p + 17), (p + 1, p + 8, None)):
        assert _call(0, 1, *args) == (L.ERR_ARG, b"x, out0 and out1 must be 8-byte aligned")
        assert _call(0, 0, *args)[0] == L.ERR_ARG                 # ... also where there is nothing to do
    assert list(buf) == [0.0] * 8
