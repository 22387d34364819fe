"""The scaled boundary table of the cooperative dediscretize (emgpu_coop.h: BndScaled): a worker computes a + d32 * (x' + 0.5) with
d32 = (b - a) * 2^-32 where dediscretize.m:39 -- and the oracle -- compute a + (b - a) * ((x' + 0.5) * 2^-32).  The two round the same
real number, hence agree to the bit, whenever the scaling by 2^-32 is exact: b == a, |b - a| >= 2^-990 (the scaled width stays normal),
or a width that is not finite.  Checked here in numpy float64 (IEEE, no contraction) on every boundary pair of every shipped model and
on hand-made extremes; the plan compiler refuses a model that breaks the condition (dedisc_scalable in emgpu_model.cpp), which is
checked through a host-only hook that compiles the plan."""
import ctypes as C
import os

import numpy as np
import pytest

from em_model_manned_bayes_amd import em_io, native, _lib as L
from util import shaped_model

ALL_MODELS = sorted(f[:-4] for f in os.listdir(em_io.MODELS_DIR) if f.endswith(".npz"))
TWO_M32 = 2.0 ** -32
X_FIXED = np.array([0, 1, 2 ** 31, 0xFFFFFFFE], dtype=np.uint64)
X_DRAWS = np.random.RandomState(0x5CA1ED).randint(0, 0xFFFFFFFF, 10 ** 4).astype(np.uint64)   # x' <= 0xFFFFFFFE (clamp32)
XS = np.concatenate([X_FIXED, X_DRAWS]).astype(np.float64)                                     # exact: x' < 2^32

# (a, b): equal boundaries, the smallest gap the condition admits, infinities, magnitudes of 1e+-300 (a width that overflows among them)
EXTREMES = [(0.0, 0.0), (-37.5, -37.5), (0.0, 2.0 ** -989), (1.0, 1.0 + 2.0 ** -52), (2.0 ** -989, 2.0 ** -988), (-2.0 ** -990, 0.0),
            (-np.inf, 0.0), (0.0, np.inf), (-np.inf, np.inf), (1e300, 1.5e300), (-1e300, 1e300), (-1.7e308, 1.7e308),
            (1e-300, 1e-297), (-1e-300, 1e-298), (1e-300, 1.0), (1e-300, 1e300), (5.0, -3.0)]
# 2^-990 is 9.6e-299: pairs of magnitude 1e-300 that lie closer than that break the condition and must be refused
REFUSED = [(1e-300, 2e-300), (-1e-300, 1e-300), (0.0, 1e-300), (0.0, 2.0 ** -1000), (2.0 ** -991, 2.0 ** -990), (0.0, 5e-324)]


def scalable(a, b):
    """dedisc_scalable of emgpu_model.cpp"""
    with np.errstate(invalid="ignore", over="ignore"):
        dd = np.float64(b) - np.float64(a)
    return bool(dd == 0.0 or not (abs(dd) < 2.0 ** -990))


def both_forms(a, b):
    """(oracle's expression, the scaled table's) for every x' of XS, as float64 arrays"""
    a, b = np.float64(a), np.float64(b)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        dd = b - a
        oracle = a + dd * ((XS + 0.5) * TWO_M32)
        scaled = a + (dd * TWO_M32) * (XS + 0.5)
    return oracle, scaled


def assert_bit_equal(a, b):
    oracle, scaled = both_forms(a, b)
    assert np.array_equal(oracle.view(np.uint64), scaled.view(np.uint64)), (a, b)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        assert np.array_equal(oracle.astype(np.float32).view(np.uint32), scaled.astype(np.float32).view(np.uint32)), (a, b)


def shipped_pairs(name):
    p = em_io.load_npz(os.path.join(em_io.MODELS_DIR, name + ".npz"))
    return [(float(b[q]), float(b[q + 1])) for b in p["boundaries"] for q in range(len(b) - 1)]


@pytest.mark.parametrize("name", ALL_MODELS)
def test_every_boundary_pair_of_a_shipped_model(name):
    pairs = shipped_pairs(name)
    assert pairs
    for a, b in pairs:
        assert scalable(a, b), (name, a, b)
        assert_bit_equal(a, b)


@pytest.mark.parametrize("a,b", EXTREMES)
def test_extremes(a, b):
    assert scalable(a, b)
    assert_bit_equal(a, b)


@pytest.mark.parametrize("a,b", REFUSED)
def test_pairs_closer_than_the_condition_are_not_eligible(a, b):
    assert not scalable(a, b)


def test_the_condition_is_needed():
    """Below 2^-990 the scaled width is subnormal and loses bits: the two forms part for some x', which is why such a model is refused."""
    rs = np.random.RandomState(7)
    parted = 0
    for _ in range(64):
        gap = np.float64(rs.uniform(1.0, 2.0)) * 2.0 ** -1000
        assert not scalable(0.0, gap)
        with np.errstate(under="ignore"):
            o = gap * ((XS + 0.5) * TWO_M32)
            s = (gap * TWO_M32) * (XS + 0.5)
        parted += int(not np.array_equal(o.view(np.uint64), s.view(np.uint64)))
    assert parted >= 32, parted


def _compiles(p, path):
    """Loads the model and has its plan compiled on the host (a debug hook that needs the plan); -> the error code, 0 for none."""
    em_io.em_write(p, path)
    nm = native.NativeModel.load_txt(path)
    cm, nw = C.c_uint32(), C.c_uint32()
    return int(L.lib().emgpu_debug_parent_masks(nm._h, C.byref(cm), C.byref(nw)))


@pytest.mark.parametrize("name", ALL_MODELS)
def test_the_plan_compiler_accepts_every_shipped_model(name, model_dir):
    nm = native.NativeModel.load_txt(em_io.materialize_model(name, model_dir))
    cm, nw = C.c_uint32(), C.c_uint32()
    assert L.lib().emgpu_debug_parent_masks(nm._h, C.byref(cm), C.byref(nw)) == L.OK


def test_the_plan_compiler_refuses_a_gap_below_the_condition(tmp_path):
    p = shaped_model(np.random.RandomState(26), 7, (2, 4, 2))
    assert _compiles(p, str(tmp_path / "ok.txt")) == L.OK
    for v, gap, want in ((1, 2.0 ** -1000, L.ERR_UNSUPPORTED), (5, 2.0 ** -1000, L.ERR_UNSUPPORTED), (1, 2.0 ** -989, L.OK), (1, 0.0, L.OK)):
        q = dict(p)
        q["boundaries"] = [np.array(b, dtype=np.float64) for b in p["boundaries"]]
        if len(q["boundaries"][v]) < 2:
            q["boundaries"][v] = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0])[: int(p["r_initial"][v]) + 1]
        b = q["boundaries"][v]
        b[0] = 0.0
        b[1] = gap                       # written with repr(): the text carries the exact double
        b[2:] = np.arange(1, len(b) - 1)
        rc = _compiles(q, str(tmp_path / ("v%d_%g.txt" % (v, gap))))
        assert rc == want, (v, gap, rc)
        if want != L.OK:
            assert b"2^-990" in L.lib().emgpu_last_error()
