"""CPU: the miss distance between the seconds without a device -- the numpy restatement (miss_seg_ref) against answers worked out by hand
and against dense sampling of the piecewise-linear tracks, the conditions on the inputs that the GPU comparison relies on, every refusal
of emgpu_miss_segments_device (all of them come before any device work), and the binding against the header."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import miss_ref
import miss_seg_ref as R
from em_model_manned_bayes_amd import _lib as L, native
from em_model_manned_bayes_amd import encounter_model as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
assert (L.MISS_CPA_BETWEEN, L.MISS_NMAC_BETWEEN) == (R.CPA_BETWEEN, R.NMAC_BETWEEN)          # the restatement's bits are the library's
SHAPES = [(n, P) for n in (257, 1000) for P in (2, 3, 5, 64)]          # the GPU test's crossing cases of 257 pairs and more


# ---- the restatement against hand-computed answers
@pytest.mark.parametrize("case", R.HAND, ids=[c[0] for c in R.HAND])
def test_hand_computed(case):
    _, (a, b), (h, v), hmd, vmd, t, flags = case
    got = R.miss_segments(R.planar(a), R.planar(b), 1, 1, 1, nmac_h_ft=h, nmac_v_ft=v)
    want = {"hmd": np.array([hmd]), "vmd": np.array([vmd]), "t_cpa_s": np.array([t]), "flags": np.array([flags], dtype=np.uint8)}
    R.pair_cases.same(got, want, ("hmd", "vmd", "t_cpa_s", "flags"))
    ok = 0 if flags & R.BAD_INDEX else 1
    between = 1 if flags & R.NMAC_BETWEEN else 0
    assert got["totals"].tolist() == [ok, flags & 1, (flags >> 1) & 1, (flags >> 2) & 1, 1 - ok, ok, flags & 1, (flags >> 1) & 1, between, between]


def test_the_hand_cases_cover_what_the_per_second_call_misses():
    """the head-on passes are NMACs that emgpu_miss_distance_device's definition does not see, and weights reach totals[9]"""
    for name in ("head-on, ts = 0.5, ez = 0", "head-on, ts = 0.25", "a NaN point and a later pass"):
        (a, b), (h, v) = next((c[1], c[2]) for c in R.HAND if c[0] == name)
        assert miss_ref.miss(R.planar(a), R.planar(b), 1, 1, 1, nmac_h_ft=h, nmac_v_ft=v)["flags"].tolist() == [0]
        got = R.miss_segments(R.planar(a), R.planar(b), 1, 1, 1, nmac_h_ft=h, nmac_v_ft=v, weights=[7], totals=np.arange(10))
        assert got["totals"].tolist() == [1, 2, 3, 3, 4, 12, 13, 14, 9, 16]
    a, b = R.crossing(3, 4, 1)
    got = R.miss_segments(R.planar(a), R.planar(b), 3, 3, 3, idx_a=[0, 3, 1], idx_b=[-1, 0, 1])
    assert got["flags"][:2].tolist() == [R.BAD_INDEX] * 2 and got["t_cpa_s"][:2].tolist() == [-1.0, -1.0] and np.isnan(got["hmd"][:2]).all()
    assert got["totals"][[0, 4]].tolist() == [1, 2]


# ---- the restatement against dense sampling
def test_the_reference_against_dense_sampling():
    """4 000 crossing pairs x 12 points against K = 2 000 sub-steps per second.  The closed form never lies above a sample (to the
    rounding of two different expressions of one distance), and a sample never lies below it by more than max|e| / (2K): distance is
    1-Lipschitz in position and the nearest sample is within 1 / (2K) of a segment's length from the foot."""
    n, P, K = 4000, 12, 2000
    a, b = R.crossing(n, P, 1)
    ref = R.miss_segments(R.planar(a), R.planar(b), n, n, n)
    hmd, hit, e_max = R.brute(a, b, K)
    print("largest hmd_ref / hmd_brute - 1: %.3g; largest hmd_brute - hmd_ref: %.3g ft of %.3g allowed" %
          ((ref["hmd"] / hmd - 1.0).max(), (hmd - ref["hmd"]).max(), e_max / (2 * K)))
    assert (ref["hmd"] <= hmd * (1.0 + 1e-12)).all()
    assert (hmd - ref["hmd"] <= e_max / (2 * K)).all()
    ref_any = (ref["flags"] & R.NMAC_ANY) != 0
    assert not (hit & ~ref_any).any()                    # every brute-force NMAC is a reference NMAC
    grazing = int((ref_any & ~hit).sum())
    print("reference NMACs the brute force lacks: %d of %d pairs" % (grazing, n))
    assert grazing <= n // 100
    assert hit.sum() > n // 4                            # (the case holds NMACs)


@pytest.mark.parametrize("n,P", SHAPES)
def test_the_crossing_cases_exercise_the_new_paths(n, P):
    """without these the GPU comparison would prove nothing about the interior candidate and the between test"""
    for a, b, pose in (R.crossing(n, P, 1) + (None,), R.posed_crossing(n, P, 1)):
        flags = R.miss_segments(R.planar(a), R.planar(b), n, n, n, pose_b=pose)["flags"]
        assert ((flags & R.NMAC_BETWEEN) != 0).sum() >= 0.03 * n
        assert ((flags & R.CPA_BETWEEN) != 0).sum() >= 0.30 * n


def test_against_the_per_second_definition():
    n, P = 1000, 5
    a, b, pose = R.posed_crossing(n, P, 1)
    seg = R.miss_segments(R.planar(a), R.planar(b), n, n, n, pose_b=pose)
    sec = miss_ref.miss(R.planar(a), R.planar(b), n, n, n, pose_b=pose)
    at_point = (seg["flags"] & R.CPA_BETWEEN) == 0
    assert (seg["hmd"] <= sec["hmd"]).all() and np.array_equal(seg["hmd"][at_point], sec["hmd"][at_point])
    assert np.array_equal(seg["t_cpa_s"][at_point], sec["t_cpa"][at_point].astype(np.float64))
    assert np.array_equal(((seg["flags"] & R.NMAC_ANY) != 0) & ((seg["flags"] & R.NMAC_BETWEEN) == 0), (sec["flags"] & R.NMAC_ANY) != 0)
    assert np.array_equal(seg["totals"][[0, 3, 4, 5]], sec["totals"][[0, 3, 4, 5]])


# ---- every refusal, through the library: none needs a device
def _call(p, xyz_a=True, xyz_b=True, idx_a=False, idx_b=False, outs=(True,) * 5, entry="emgpu_miss_segments_device", shift=None):
    buf = np.zeros(64)
    at = lambda yes, by=0: C.c_void_p(buf.ctypes.data + by) if yes else None          # noqa: E731
    lib = L.lib()
    args = [at(xyz_a), at(xyz_b), at(idx_a), at(idx_b), None, None] + [at(o) for o in outs]
    if shift is not None:
        args[shift[0]] = at(True, shift[1])
    rc = getattr(lib, entry)(None, C.byref(p) if p is not None else None, *args)
    return rc, lib.emgpu_last_error().decode()


def _refused(words, *a, **kw):
    rc, msg = _call(*a, **kw)
    assert rc == L.ERR_ARG and words in msg, (rc, msg)


def test_every_refusal_names_its_argument():
    ok = lambda **kw: native.miss_params(**{**dict(n_pairs=4, n_a=4, n_b=4, points=3), **kw})          # noqa: E731
    _refused("null argument: p", None)
    _refused("null argument: xyz_a", ok(), xyz_a=False)
    _refused("null argument: xyz_b", ok(), xyz_b=False)
    _refused("null hmd, vmd, t_cpa_s, flags and totals: nothing to write", ok(), outs=(False,) * 5)
    _refused("points outside 1..65537", ok(points=0))
    _refused("points outside 1..65537", ok(points=65538))
    _refused("n_pairs", ok(n_pairs=-1))
    _refused("n_pairs", ok(n_pairs=2**32 + 1, n_a=1, n_b=1))
    _refused("n_a", ok(n_a=0))
    _refused("n_b", ok(n_b=0))
    _refused("ld_a", ok(ld_a=3))
    _refused("ld_b", ok(ld_b=3))
    _refused("idx_a", ok(n_pairs=5, n_b=5))
    _refused("idx_b", ok(n_pairs=5, n_a=5))
    _refused("idx_b", ok(n_pairs=5, n_a=1))
    _refused("nmac_h_ft", ok(nmac_h_ft=-1.0))
    _refused("nmac_h_ft", ok(nmac_h_ft=float("nan")))
    _refused("nmac_v_ft", ok(nmac_v_ft=-0.5))
    _refused("nmac_v_ft", ok(nmac_v_ft=float("nan")))
    # alignment: t_cpa_s is a double here (argument 8 behind p), the weights stay 4-byte
    _refused("t_cpa_s and totals must be 8-byte aligned", ok(), shift=(8, 4))
    _refused("8-byte aligned", ok(), shift=(0, 4))
    _refused("weights must be 4-byte aligned", ok(), shift=(5, 2))


def test_the_shared_refusals_carry_the_per_second_calls_messages():
    for fault in (dict(no_p=True), dict(xyz_a=False), dict(xyz_b=False), dict(n_pairs=-1), dict(n_pairs=2**32 + 1, n_a=1, n_b=1), dict(n_a=0),
                  dict(n_b=0), dict(ld_a=3), dict(ld_b=3), dict(n_pairs=5, n_b=5), dict(n_pairs=5, n_a=5), dict(n_pairs=5, n_a=1),
                  dict(points=0), dict(points=65538), dict(nmac_h_ft=-1.0), dict(nmac_v_ft=float("nan"))):
        fault = dict(fault)
        no_p, xyz_a, xyz_b = fault.pop("no_p", False), fault.pop("xyz_a", True), fault.pop("xyz_b", True)
        p = None if no_p else native.miss_params(**{**dict(n_pairs=4, n_a=4, n_b=4, points=3), **fault})
        seg = _call(p, xyz_a, xyz_b)
        sec = _call(p, xyz_a, xyz_b, entry="emgpu_miss_distance_device")
        assert seg == sec and seg[0] == L.ERR_ARG and seg[1], (fault, seg, sec)
    seg, sec = _call(native.miss_params(4, 4, 4, 3), outs=(False,) * 5), _call(native.miss_params(4, 4, 4, 3), outs=(False,) * 5,
                                                                             entry="emgpu_miss_distance_device")
    assert seg[1] != sec[1] and seg[1].endswith(": nothing to write") and sec[1].endswith(": nothing to write")


def test_no_pairs_succeed_without_a_launch_and_the_limits_themselves_pass_the_checks():
    assert _call(native.miss_params(0, 4, 4, 3))[0] == L.OK
    assert _call(native.miss_params(0, 1, 1, 65537, nmac_h_ft=0.0, nmac_v_ft=0.0, ld_a=1, ld_b=9))[0] == L.OK
    for k in range(5):                                   # each output alone is enough
        assert _call(native.miss_params(0, 4, 4, 1), outs=tuple(j == k for j in range(5)))[0] == L.OK
    assert _call(native.miss_params(0, 1, 1, 1), idx_a=True, idx_b=True)[0] == L.OK


def test_weights_outside_uint32_are_refused_before_the_library_is_called():
    xyz = np.zeros((2, 3, 3))
    for w in ([1, -1], [1, 2**32], [1.0, 2.0], [1]):
        with pytest.raises(ValueError):
            native.miss_segments(xyz, xyz, weights=w)
    with pytest.raises(ValueError):
        native.miss_segments(xyz, xyz, pose_b=np.zeros((5, 3)))


# ---- the binding against the header
def test_the_header_declares_the_entry_point_the_binding_mirrors():
    hdr = open(os.path.join(ROOT, "include", "emgpu.h")).read()
    assert "emgpu_miss_segments_device" in L.SYMBOLS and hasattr(L.lib(), "emgpu_miss_segments_device")
    decl = re.search(r"int emgpu_miss_segments_device\(([^)]*)\);", hdr).group(1)
    params = [re.sub(r"/\*.*?\*/", "", s).strip() for s in decl.split(",")]
    assert len(params) == 13 == len(L.lib().emgpu_miss_segments_device.argtypes)
    assert params[0] == "void *hip_stream" and params[1] == "const emgpu_miss_params *p" and params[10] == "double *t_cpa_s"
    assert "emgpu_ctx" not in decl and "emgpu_model" not in decl                   # the entry point takes no handle
    old = [s.strip() for s in re.search(r"int emgpu_miss_distance_device\(([^)]*)\);", hdr).group(1).split(",")]
    assert [p for k, p in enumerate(params) if k != 10] == [p for k, p in enumerate(old) if k != 10]
    assert C.sizeof(L.MissParams) == 5 * 8 + 2 * 4 + 2 * 8                         # the struct is the per-second call's, unchanged


def test_the_two_new_flags():
    hdr = open(os.path.join(ROOT, "include", "emgpu.h")).read()
    for name, bit in (("CPA_BETWEEN", 16), ("NMAC_BETWEEN", 32)):
        value = int(re.search(r"#define EMGPU_MISS_%s (\d+)u" % name, hdr).group(1))
        assert getattr(L, "MISS_" + name) == value == getattr(R, name) == bit
    for name in ("NMAC_CPA", "NMAC_ANY", "NO_CPA", "BAD_INDEX"):
        assert getattr(L, "MISS_" + name) == getattr(R, name) == getattr(miss_ref, name)


def test_the_python_surface():
    sig = lambda f: str(inspect.signature(f))          # noqa: E731
    assert sig(native.miss_segments) == sig(native.miss_distance)
    assert sig(native.encounter_miss_segments) == sig(native.encounter_miss)
    assert sig(native.miss_segments_device) == sig(native.miss_distance_device).replace("t_cpa=0", "t_cpa_s=0")
    assert sig(native._miss_segments_tensors) == sig(native._miss_tensors)
    assert sig(native._miss_segments_dict) == "(hmd, vmd, t_cpa_s, flags, totals)"
    for method in (E.UncorEncounterModel.pair, E.UncorEncounterModel.encounter):
        assert inspect.signature(method).parameters["between"].default is False
