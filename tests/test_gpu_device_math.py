"""-m gpu: the track kernels' hand-written device math (sincos_small, sincosd_small, t_sincosd, f_sincosd, ut_sincos, ut_atan,
ut_asin_small, ut_rcp, round500), each evaluated on the device by emgpu_debug_device_math -- the very functions the product kernels
call -- and compared with the exact value of the exact argument (device_math_ref.py: long double, checked against mpmath by
test_device_math.py), never with another run of the code under test.

Measures: every sine and cosine as |got - exact| in units of 2^-53 (absolute); atan, asin, 1/d and sincos_small's sine in ulps of the exact
result.  BOUNDS are the figures the functions' header comments state; the measured worst errors and their arguments are DESIGN.md
section 39's table.  Every function runs once on its family's whole input set (the results are shared by the tests, read-only), into
output buffers between guard bytes."""
import numpy as np
import pytest

import device_math_ref as R
import pair_cases as PC
from em_model_manned_bayes_amd import _lib as L

pytestmark = pytest.mark.gpu

# fn: the bound on (out0, out1), in the measure of MEASURE
BOUNDS = {
    "sincos_small": (2.0, 2.0), "sincos_small_sk": (2.0, 2.0),
    "sincosd_small": (2.0, 2.0), "t_sincosd": (2.0, 2.0), "f_sincosd": (2.0, 2.0),
    "ut_sincos": (2.0, 2.0), "ut_sincos_sk": (2.0, 2.0),
    "ut_atan": (2.0,), "ut_atan_sk": (2.0,), "ut_asin_small": (2.0,), "ut_asin_small_sk": (2.0,),
    "ut_rcp": (1.0,),
}
MEASURE = {fn: ((R.ulps if fn.startswith("sincos_small") else R.units), R.units) if fn in R.PAIRS else (R.ulps,) for fn in BOUNDS}
NAME = {R.units: "units of 2^-53", R.ulps: "ulp"}
DEGREES = ("sincosd_small", "t_sincosd", "f_sincosd")

_results = {}


def probe(fn, x, out1=True, n=None):
    """emgpu_debug_device_math on x[:n]: (out0, out1 or None) as numpy arrays, the guard bytes checked.  A one-result function given an
    out1 must leave it as it was."""
    import torch
    dev = torch.device("cuda", 0)
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x) if n is None else n
    d_x = torch.from_numpy(x).to(dev)
    sizes = {"out0": 8 * n}
    if out1:
        sizes["out1"] = 8 * n
    bufs = PC.guarded(sizes, dev)
    L.check(L.lib().emgpu_debug_device_math(None, R.FUNCTIONS.index(fn), n, d_x.data_ptr(), bufs["out0"].data_ptr() + PC.GUARD,
                                            bufs["out1"].data_ptr() + PC.GUARD if out1 else None))
    torch.cuda.synchronize()
    got = {name: raw.view(np.float64) for name, raw in PC.payloads(bufs, sizes).items()}
    if out1 and fn not in R.PAIRS:
        assert (got["out1"].view(np.uint8) == PC.FILL).all(), "a one-result function wrote out1"
    return got["out0"], got.get("out1") if fn in R.PAIRS else None


def results(fn):
    """fn on its family's whole input set, run once"""
    if fn not in _results:
        out = tuple(a for a in probe(fn, R.inputs(R.FAMILY[fn])) if a is not None)
        for a in out:
            a.setflags(write=False)
        _results[fn] = out
    return _results[fn]


# ---- 1. the probe itself
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 100003])
def test_the_probe_writes_every_element_and_nothing_else(n):
    """Every size around a wave and a workgroup and one of many workgroups: each element holds its function's value (the buffers start as a
    pattern that is no result), the guard bytes stay, a NULL out1 is accepted and a one-result function leaves its out1 alone."""
    for fn in ("ut_sincos", "ut_atan"):
        x = R.inputs(R.FAMILY[fn])[11:11 + n]                                     # behind the specials: every result is a number
        assert len(x) == n and np.isfinite(x).all()
        whole = results(fn)
        got = probe(fn, x)
        for g, w in zip(got, whole):
            assert not len(R.same_bits(g, w[11:11 + n]))
        assert not len(R.same_bits(probe(fn, x, out1=False)[0], whole[0][11:11 + n]))
    longer = R.inputs("ut_atan")[11:11 + n + 300]                                 # n of a longer input: nothing behind n is computed
    assert not len(R.same_bits(probe("ut_atan", longer, n=n)[0], results("ut_atan")[0][11:11 + n]))


def test_the_probe_refuses_bad_arguments_with_device_pointers():
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.zeros(64, dtype=torch.float64, device=dev)
    p, lib = buf.data_ptr(), L.lib()
    for args, msg in (((13, 1, p, p + 64, p + 128), b"no such function: fn outside 0..12"), ((-1, 1, p, p + 64, p + 128), b"no such function: fn outside 0..12"),
                      ((0, -1, p, p + 64, p + 128), b"n outside 0..2^32"), ((0, 1, None, p + 64, p + 128), b"null argument: x"),
                      ((0, 1, p, None, p + 128), b"null argument: out0"), ((0, 1, p + 4, p + 64, p + 128), b"x, out0 and out1 must be 8-byte aligned"),
                      ((0, 1, p, p + 68, None), b"x, out0 and out1 must be 8-byte aligned"), ((7, 1, p, p + 64, p + 130), b"x, out0 and out1 must be 8-byte aligned")):
        assert lib.emgpu_debug_device_math(None, *args) == L.ERR_ARG and lib.emgpu_last_error() == msg, args
    assert lib.emgpu_debug_device_math(None, 0, 0, p, p + 64, p + 128) == L.OK
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()


# ---- 2. accuracy
def _errors(fn):
    """per result: (the errors in the result's measure over the whole set, the in-domain mask)"""
    fam = R.FAMILY[fn]
    x, want = R.inputs(fam), R.reference(fam)
    dom = R.in_domain(fam, x)
    return [(MEASURE[fn][r](results(fn)[r], want[r]), dom) for r in range(len(want))]


@pytest.mark.parametrize("fn", sorted(BOUNDS))
def test_the_worst_error_over_the_whole_input_set_is_within_the_stated_bound(fn):
    """Over the arguments of the documented domain (device_math_ref.in_domain).  ut_asin_small's is |x| < 0.5, the guard of both its call
    sites in k_uncor_track: `fabs(st) < 0.5 ? ut_asin_small<true>(st) : asin(st)` and `if (fabs(sn) < 0.5) as = ut_asin_small(sn); else as =
    asin(sn);`.  ut_rcp's is a normal d with a normal reciprocal.  A failure names the argument in hex and the error."""
    x = R.inputs(R.FAMILY[fn])
    found = []
    for r, (err, dom) in enumerate(_errors(fn)):
        worst, at = R.worst(err, x, dom)
        which = ("sin", "cos")[r] if fn in R.PAIRS else "value"
        print("%-16s %-5s worst %.3f %s at x = %s (%r), bound %.1f, %d arguments" % (fn, which, worst, NAME[MEASURE[fn][r]], at.hex(), at, BOUNDS[fn][r], dom.sum()))
        found.append((which, worst, at, BOUNDS[fn][r]))
    for which, worst, at, bound in found:
        assert worst <= bound, "%s %s: %.3f %s at x = %s, bound %.1f" % (fn, which, worst, NAME[MEASURE[fn][0 if which != "cos" else 1]], at.hex(), bound)


def test_the_relative_error_of_the_small_component_near_a_multiple_of_half_pi_is_recorded():
    """Not asserted (the absolute measure is the claim): ut_sincos reduces with pi/2 in two pieces, and next to k pi/2 the component that
    vanishes there keeps the reduction's absolute error, which is many ulps of the component itself."""
    x, (ws, wc) = R.inputs("ut_sincos"), R.reference("ut_sincos")
    s, c = results("ut_sincos")
    near = np.zeros(len(x), dtype=bool)
    near[11:11 + 5 * (2 * R.K_MAX + 1)] = True
    near &= x != 0
    small_is_sin = np.abs(ws) < np.abs(wc)
    rel = np.where(small_is_sin, R.ulps(s, ws), R.ulps(c, wc))
    absolute = np.where(small_is_sin, R.units(s, ws), R.units(c, wc))
    worst, at = R.worst(rel, x, near)
    print("ut_sincos: the small component next to k pi/2: worst %.3g ulps of itself at x = %s (%r); absolute %.3g units of 2^-53"
          % (worst, at.hex(), at, R.worst(absolute, x, near)[0]))
    assert R.worst(absolute, x, near)[0] <= 2.0


# ---- 3. exactness
def test_the_degree_forms_are_exact_at_every_multiple_of_90_with_the_goldens_signs():
    x = R.inputs("sincosd")
    at90 = R.in_domain("sincosd", x) & (np.fmod(x, 90.0) == 0)
    assert at90.sum() >= 4001 + 17 + 176
    ws, wc = (a.astype(np.float64) for a in R.reference("sincosd"))
    assert set(np.unique(np.abs(ws[at90]))) | set(np.unique(np.abs(wc[at90]))) == {0.0, 1.0}
    t = R.trig_table()
    csv = slice(11 + 5 * 8001, 11 + 5 * 8001 + len(t))
    assert np.array_equal(x[csv], t[:, 0])
    t90 = np.fmod(t[:, 0], 90.0) == 0
    for fn in DEGREES:
        s, c = results(fn)
        bad = np.union1d(R.same_bits(s[at90], ws[at90]), R.same_bits(c[at90], wc[at90]))
        assert not len(bad), "%s at %s degrees: (%r, %r), exact (%r, %r)" % (fn, x[at90][bad[0]], s[at90][bad[0]], c[at90][bad[0]], ws[at90][bad[0]], wc[at90][bad[0]])
        assert not len(R.same_bits(s[csv][t90], t[t90, 1])) and not len(R.same_bits(c[csv][t90], t[t90, 2]))      # the golden itself, `90,1,-0` included


def test_signed_zeros_go_through():
    for fn in ("sincos_small", "sincos_small_sk", "ut_sincos", "ut_sincos_sk"):
        s, c = probe(fn, [0.0, -0.0])
        assert not len(R.same_bits(s, [0.0, -0.0])) and not len(R.same_bits(c, [1.0, 1.0])), fn
    for fn in ("ut_asin_small", "ut_asin_small_sk"):
        assert not len(R.same_bits(probe(fn, [0.0, -0.0])[0], [0.0, -0.0])), fn
    tiny = 2.0 ** -np.array([27.0, 28, 30, 40, 100, 500, 1000, 1074])             # 2^-27 and below: s = x and c = 1 exactly
    tiny = np.concatenate([tiny, -tiny])
    for fn in ("sincos_small", "sincos_small_sk"):
        s, c = probe(fn, tiny)
        assert not len(R.same_bits(s, tiny)) and (c == 1.0).all(), fn


def test_ut_atan_returns_its_tabulated_constants_where_the_reduced_argument_vanishes():
    """At 0.5, 1 and 1.5 the reduced argument (2x - 1) / (2 + x), (x - 1) / (x + 1), (x - 1.5) / (1 + 1.5 x) is exactly 0, and from 2^54 up
    -1 / x is below half an ulp of pi/2: the result is the branch's constant alone, which must be the double nearest atan(0.5), atan(1),
    atan(1.5) and pi/2 -- half an ulp, by reasoning, not the two of the function at large (a constant off in its 17th digit fails here)."""
    x = np.array([0.5, 1.0, 1.5, 2.0 ** 54, R.DBL_MAX, -0.5, -1.0, -1.5, -2.0 ** 54, -R.DBL_MAX])
    want, = R.exact("ut_atan", x)
    for fn in ("ut_atan", "ut_atan_sk"):
        got = probe(fn, x)[0]
        err = R.ulps(got, want)
        print("%s at the constants: %s ulp" % (fn, np.round(err.astype(np.float64), 3)))
        assert (err <= 0.5).all(), (fn, got, err)


# ---- 4. "the same bits"
def test_t_sincosd_is_sincosd_small_bit_for_bit():
    a, b = results("sincosd_small"), results("t_sincosd")
    x = R.inputs("sincosd")
    for r in range(2):
        bad = R.same_bits(a[r], b[r])
        assert not len(bad), "%d differ, the first at %s degrees: %r against %r" % (len(bad), float(x[bad[0]]).hex(), a[r][bad[0]], b[r][bad[0]])


@pytest.mark.parametrize("plain,sk", R.TWINS)
def test_the_scalar_operand_variant_is_its_twin_bit_for_bit(plain, sk):
    x = R.inputs(R.FAMILY[plain])
    for a, b in zip(results(plain), results(sk)):
        bad = R.same_bits(a, b)
        assert not len(bad), "%d differ, the first at x = %s: %r against %r" % (len(bad), float(x[bad[0]]).hex(), a[bad[0]], b[bad[0]])


# ---- 5. non-finite arguments and arguments outside the documented domain
def test_not_a_number_and_the_infinities():
    """NaN and +-inf give NaN in both results of every sine / cosine form that reduces its argument; nothing traps (the launches complete and
    every other element of the same launch is right: the accuracy tests read these very results).  sincos_small reduces nothing: NaN gives
    NaN, and an infinite argument is outside |x| <= pi/4 like any other large one (its header comment: the sine NaN, the cosine -inf)."""
    bad = np.array([np.nan, np.inf, -np.inf])
    for fn in DEGREES + ("ut_sincos", "ut_sincos_sk"):
        s, c = probe(fn, bad)
        assert np.isnan(s).all() and np.isnan(c).all(), (fn, s, c)
    for fn in ("sincos_small", "sincos_small_sk"):
        s, c = probe(fn, bad)
        assert np.isnan(s).all() and np.isnan(c[0]) and (c[1:] == -np.inf).all(), (fn, s, c)
    for fn in ("ut_atan", "ut_atan_sk", "ut_asin_small", "ut_asin_small_sk", "ut_rcp"):
        assert np.isnan(probe(fn, [np.nan])[0]).all(), fn


def test_ut_atan_outside_and_at_the_edge_of_its_domain():
    """Its domain is finite x.  +-inf gives NaN, not +-pi/2 (ut_rcp(inf) = 0 and fma(-inf, 0, 1) is NaN): no infinite argument reaches it from
    k_uncor_track.  atan(-0.0) is +0.0.  The largest finite arguments are inside: +-pi/2."""
    for fn in ("ut_atan", "ut_atan_sk"):
        got = probe(fn, [np.inf, -np.inf, -0.0, 0.0, R.DBL_MAX, -R.DBL_MAX])[0]
        assert np.isnan(got[:2]).all(), (fn, got)
        assert not len(R.same_bits(got[2:], [0.0, 0.0, np.pi / 2, -np.pi / 2])), (fn, got)


def test_degrees_beyond_2_to_the_53_are_unspecified_and_do_not_trap():
    """|deg| >= 2^53 is outside the degree forms' domain: n * 90 is no longer exact (and from 90 * 2^63 on the quotient is outside the integer
    conversion), so the results are not the sine and cosine of deg -- any value, the infinities and NaN included.  What holds: the launch
    completes, the elements beside them are untouched by it (exactness and accuracy read the same launch), and the results are recorded."""
    x = R.inputs("sincosd")
    out = np.isfinite(x) & ~R.in_domain("sincosd", x)
    assert out.sum() == 22                                                       # +-DBL_MAX and the two pieces beyond 2^53
    ws, wc = R.reference("sincosd")
    for fn in DEGREES:
        s, c = results(fn)
        for i in np.flatnonzero(out):
            print("%-14s deg = %-24r -> (%r, %r); exact (%.17g, %.17g)" % (fn, x[i], s[i], c[i], float(ws[i]), float(wc[i])))


def test_what_ut_rcp_and_ut_asin_small_do_outside_their_domains_is_recorded():
    """Recorded, not asserted: v_rcp_f64 on subnormals and on arguments whose reciprocal is subnormal is whatever the hardware does; the
    rational kernel of ut_asin_small at and beyond 0.5 simply loses accuracy."""
    x, (want,) = R.inputs("ut_rcp"), R.reference("ut_rcp")
    got, = results("ut_rcp")
    err = R.ulps(got, want)
    fin = np.isfinite(x)
    for name, mask in (("subnormal d", fin & (np.abs(x) < R.DBL_MIN) & (x != 0)), ("subnormal 1/d", fin & (np.abs(x) > 2.0 ** 1022))):
        worst, at = R.worst(err, x, mask)
        print("ut_rcp, %s: %d arguments, %d exact, %d infinite, %d zero, worst %.3g ulp at d = %s -> %r (1/d = %r)"
              % (name, mask.sum(), (err[mask] == 0).sum(), np.isinf(got[mask]).sum(), (got[mask] == 0).sum(), worst, at.hex(),
                 got[np.flatnonzero(x == at)[0]], 1.0 / at))
    z = probe("ut_rcp", [0.0, -0.0, np.inf, -np.inf])[0]
    print("ut_rcp(+-0, +-inf) = %r" % (z,))
    a = probe("ut_asin_small", [0.5, -0.5, 0.75, 1.0, R.DBL_MAX])[0]
    print("ut_asin_small(0.5, -0.5, 0.75, 1, DBL_MAX) = %r; asin = %r" % (a, np.arcsin([0.5, -0.5, 0.75, 1.0])))


# ---- 6. round500
def test_round500_is_the_references_line_bit_for_bit():
    """UncorEncounterModel.m:196 restated in numpy (device_math_ref.round500: MATLAB's mod is numpy's mod, the floored one) on multiples of 250
    and 500 with their neighbours, negatives, +-0, 1e15, the specials (NaN against NaN) and 2^17 random altitudes of both signs."""
    x, (want,) = R.inputs("round500"), R.reference("round500")
    got, = results("round500")
    bad = R.same_bits(got, want)
    assert not len(bad), "%d differ, the first: round500(%r) = %r, the reference's line gives %r" % (len(bad), x[bad[0]], got[bad[0]], want[bad[0]])
    assert np.signbit(want[1]) == np.signbit(got[1])                              # -0.0


# ---- 7. the quadrant choice
def test_both_reduction_quotients_give_the_exact_value_where_they_differ():
    """sincosd_small / t_sincosd form round(deg * (1/90)), f_sincosd and the oracle round(deg / 90); where the two differ (k * 90 + 45 and the
    doubles next to it) each form must still be within its bound of the exact value."""
    x = R.inputs("sincosd")
    dom = R.in_domain("sincosd", x)
    n_mul, n_div = R.sincosd_quotients(x)
    with np.errstate(invalid="ignore"):
        diff = dom & (n_mul != n_div)
    assert diff.sum() > 0
    want = R.reference("sincosd")
    for fn in DEGREES:
        for r in range(2):
            worst, at = R.worst(R.units(results(fn)[r], want[r]), x, diff)
            print("%-14s %s over the %d angles the two quotients reduce differently: worst %.3f units at %r" % (fn, ("sin", "cos")[r], diff.sum(), worst, at))
            assert worst <= BOUNDS[fn][r], (fn, r, worst, at)
