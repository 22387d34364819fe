"""CPU: the miss-distance feature without a device -- the numpy restatement (miss_ref) against answers worked out by hand, every refusal of
emgpu_miss_distance_device (all of them come before any device work), make_pose, and the binding against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import miss_ref as R
from em_model_manned_bayes_amd import _lib as L, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against hand-computed answers
def test_two_tracks_crossing_at_right_angles():
    """A flies east along y = 0 at 100 ft/s and passes x = 0 at second 5; B flies north along x = 0 and passes y = 0 at second 3, 50 ft above.
    d^2 = (100 p - 500)^2 + (100 p - 300)^2: 40000 at p = 3 and p = 5, 20000 at p = 4."""
    p = np.arange(11.0)
    a = np.stack([100.0 * p - 500.0, 0.0 * p, 0.0 * p + 1000.0], axis=1)[None]
    b = np.stack([0.0 * p, 100.0 * p - 300.0, 0.0 * p + 1050.0], axis=1)[None]
    got = R.miss(R.planar(a), R.planar(b), 1, 1, 1)
    assert got["t_cpa"].tolist() == [4] and got["hmd"][0] == np.sqrt(20000.0) and got["vmd"][0] == 50.0
    assert got["flags"].tolist() == [R.NMAC_CPA | R.NMAC_ANY]
    assert got["totals"].tolist() == [1, 1, 1, 0, 0, 1, 1, 1]
    # 150 ft above instead: no NMAC anywhere, whatever the horizontal distance
    b[..., 2] += 100.0
    got = R.miss(R.planar(a), R.planar(b), 1, 1, 1, weights=[7])
    assert got["vmd"][0] == 150.0 and got["flags"].tolist() == [0] and got["totals"].tolist() == [1, 0, 0, 0, 0, 7, 0, 0]
    # the pose that turns B's track by 90 degrees and moves it: B' flies west along y = 400 -> x' = -y, y' = x + 400
    got = R.miss(R.planar(a), R.planar(b), 1, 1, 1, pose_b=[[0.0], [1.0], [0.0], [400.0], [-150.0]])
    # dx = (100 p - 500) - (300 - 100 p) = 200 p - 800, dy = -400: closest at p = 4, d = 400, dz = 0
    assert got["t_cpa"].tolist() == [4] and got["hmd"][0] == 400.0 and got["vmd"][0] == 0.0 and got["flags"].tolist() == [3]


def test_the_first_of_two_equal_minima_is_the_cpa_and_a_nan_second_is_skipped():
    a = np.zeros((1, 5, 3))
    b = np.zeros((1, 5, 3))
    b[0, :, 0] = [5.0, 3.0, 4.0, 3.0, 6.0]
    b[0, :, 2] = [0.0, 10.0, 20.0, 30.0, 40.0]
    got = R.miss(R.planar(a), R.planar(b), 1, 1, 1)
    assert got["t_cpa"].tolist() == [1] and got["hmd"][0] == 3.0 and got["vmd"][0] == 10.0
    b[0, 1, 0] = np.nan
    got = R.miss(R.planar(a), R.planar(b), 1, 1, 1)
    assert got["t_cpa"].tolist() == [3] and got["vmd"][0] == 30.0
    b[0, :, 0] = np.nan
    got = R.miss(R.planar(a), R.planar(b), 1, 1, 1)
    assert got["t_cpa"].tolist() == [-1] and np.isnan(got["hmd"][0]) and got["flags"].tolist() == [R.NO_CPA]
    assert got["totals"].tolist() == [1, 0, 0, 1, 0, 1, 0, 0]
    got = R.miss(R.planar(a), R.planar(b), 1, 1, 3, idx_a=[0, -1, 0], idx_b=[0, 0, 1])
    assert got["flags"].tolist() == [R.NO_CPA, R.BAD_INDEX, R.BAD_INDEX] and got["totals"].tolist() == [1, 0, 0, 1, 2, 1, 0, 0]


def test_two_squares_that_round_to_one_root():
    """The pair of the GPU test's case 2: the minimum is over the roots, so the earlier second wins although its square is larger."""
    dx, dy = 2607.925961031258, 4757.272111997083
    dx1 = np.nextafter(dx, 0.0)
    q0, q1 = dx * dx + dy * dy, dx1 * dx1 + dy * dy
    assert q0.hex() == "0x1.c11c53c40bdc9p+24" and q1.hex() == "0x1.c11c53c40bdc8p+24"
    assert np.sqrt(q0) == np.sqrt(q1) and float(np.sqrt(q0)).hex() == "0x1.531360c60e4d8p+12"
    a = np.zeros((1, 2, 3))
    a[0, :, 0], a[0, :, 1] = [dx, dx1], dy
    got = R.miss(R.planar(a), R.planar(np.zeros((1, 2, 3))), 1, 1, 1)
    assert got["t_cpa"].tolist() == [0]


# ---- every refusal, through the library: none needs a device
def _call(p, xyz_a=True, xyz_b=True, idx_a=False, idx_b=False, outs=(True, True, True, True, True)):
    buf = np.zeros(64)
    at = lambda yes: buf.ctypes.data_as(C.c_void_p) if yes else None          # noqa: E731
    lib = L.lib()
    rc = lib.emgpu_miss_distance_device(None, C.byref(p) if p is not None else None, at(xyz_a), at(xyz_b), at(idx_a), at(idx_b), None, None,
                                        *(at(o) for o in outs))
    return rc, lib.emgpu_last_error().decode()


def _refused(words, *a, **kw):
    rc, msg = _call(*a, **kw)
    assert rc == L.ERR_ARG and words in msg, (rc, msg)


def test_every_refusal_names_its_argument():
    ok = lambda **kw: native.miss_params(**{**dict(n_pairs=4, n_a=4, n_b=4, points=3), **kw})          # noqa: E731
    _refused("null argument: p", None)
    _refused("null argument: xyz_a", ok(), xyz_a=False)
    _refused("null argument: xyz_b", ok(), xyz_b=False)
    _refused("nothing to write", ok(), outs=(False,) * 5)
    _refused("points", ok(points=0))
    _refused("points", ok(points=65538))
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


def test_both_entry_points_say_the_same_about_a_faulty_pairing():
    """emgpu_miss_distance_device and emgpu_encounter_pose_device check a pairing in one place: the same fault, the same message; only the
    outputs named where there is nothing to write and the lower bound of `points` (1 and 2) are each call's own"""
    def both(xyz_a=True, xyz_b=True, no_p=False, outs=True, **kw):
        kw = {**dict(n_pairs=4, n_a=4, n_b=4, points=3), **kw}
        rc, miss = _call(None if no_p else native.miss_params(**kw), xyz_a, xyz_b, outs=(outs,) * 5)
        buf = np.zeros(64)
        at = lambda yes: buf.ctypes.data_as(C.c_void_p) if yes else None          # noqa: E731
        pe = native.encounter_params(radius_ft=1.0, half_height_ft=1.0, seed=0, **kw)
        rc_e = L.lib().emgpu_encounter_pose_device(None, None if no_p else C.byref(pe), at(xyz_a), at(xyz_b), None, None, None, *(at(outs),) * 4)
        assert rc == rc_e == L.ERR_ARG
        return miss, L.lib().emgpu_last_error().decode()
    for fault in (dict(no_p=True), dict(xyz_a=False), dict(xyz_b=False), dict(n_pairs=-1), dict(n_pairs=2**32 + 1, n_a=1, n_b=1), dict(n_a=0),
                  dict(n_b=0), dict(ld_a=3), dict(ld_b=3), dict(n_pairs=5, n_b=5), dict(n_pairs=5, n_a=5), dict(n_pairs=5, n_a=1)):
        miss, enc = both(**fault)
        assert miss == enc and miss, (fault, miss, enc)
    for fault in (dict(points=0), dict(points=65538), dict(points=0, n_a=0)):       # (two faults: the first check's message)
        miss, enc = both(**fault)
        assert miss == "points outside 1..65537" and enc == "points outside 2..65537"
    miss, enc = both(outs=False, points=0)
    assert miss != enc and miss.endswith(": nothing to write") and enc.endswith(": nothing to write")


def test_no_pairs_succeed_without_a_launch_and_the_limits_themselves_pass_the_checks():
    assert _call(native.miss_params(0, 4, 4, 3))[0] == L.OK
    assert _call(native.miss_params(0, 1, 1, 65537, nmac_h_ft=0.0, nmac_v_ft=0.0, ld_a=1, ld_b=9))[0] == L.OK
    # each output alone is enough
    for k in range(5):
        assert _call(native.miss_params(0, 4, 4, 1), outs=tuple(j == k for j in range(5)))[0] == L.OK
    # with index arrays n_pairs may exceed both sets
    assert _call(native.miss_params(0, 1, 1, 1), idx_a=True, idx_b=True)[0] == L.OK


def test_weights_outside_uint32_are_refused_before_the_library_is_called():
    xyz = np.zeros((2, 3, 3))
    for w in ([1, -1], [1, 2**32], [1.0, 2.0], [1]):
        with pytest.raises(ValueError):
            native.miss_distance(xyz, xyz, weights=w)


# ---- make_pose
def test_make_pose_is_exact_at_the_quarter_turns():
    got = native.make_pose([0.0, 90.0, 180.0, 270.0, -90.0, 360.0], 1.5, [2.0, 3.0, 4.0, 5.0, 6.0, 7.0], -8.0)
    assert got.shape == (5, 6) and got.dtype == np.float64 and got.flags["C_CONTIGUOUS"]
    assert got[0].tolist() == [1.0, 0.0, -1.0, 0.0, 0.0, 1.0] and got[1].tolist() == [0.0, 1.0, 0.0, -1.0, -1.0, 0.0]
    assert not np.signbit(got[:2]).any() or (got[:2][np.signbit(got[:2])] != 0.0).all()      # no negative zero
    assert got[2].tolist() == [1.5] * 6 and got[3].tolist() == [2.0, 3.0, 4.0, 5.0, 6.0, 7.0] and got[4].tolist() == [-8.0] * 6
    one = native.make_pose(30.0)
    assert one.shape == (5, 1) and abs(one[1, 0] - 0.5) < 1e-15 and abs(one[0, 0] - np.sqrt(0.75)) < 1e-15 and one[2:].tolist() == [[0.0]] * 3


# ---- the binding against the header
def test_the_header_declares_the_entry_point_and_the_struct_the_binding_mirrors():
    hdr = open(os.path.join(ROOT, "include", "emgpu.h")).read()
    assert "emgpu_miss_distance_device" in L.SYMBOLS and hasattr(L.lib(), "emgpu_miss_distance_device")
    decl = re.search(r"int emgpu_miss_distance_device\(([^)]*)\);", hdr).group(1)
    params = [s.strip() for s in decl.split(",")]
    assert len(params) == 13 == len(L.lib().emgpu_miss_distance_device.argtypes)
    assert params[0] == "void *hip_stream" and params[1] == "const emgpu_miss_params *p"
    assert "emgpu_ctx" not in decl and "emgpu_model" not in decl                   # the entry point takes no handle
    body = re.search(r"typedef struct \{([^}]*)\} emgpu_miss_params;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    fields = [(nm.strip(), ctype[ty]) for ty, names in re.findall(r"(int64_t|int32_t|double)\s+([^;]+);", body) for nm in names.split(",")]
    assert fields == list(L.MissParams._fields_)
    assert C.sizeof(L.MissParams) == 5 * 8 + 2 * 4 + 2 * 8
    for name in ("NMAC_CPA", "NMAC_ANY", "NO_CPA", "BAD_INDEX"):
        value = int(re.search(r"#define EMGPU_MISS_%s (\d+)u" % name, hdr).group(1))
        assert getattr(L, "MISS_" + name) == value == getattr(R, name)


def test_a_context_remembers_the_stream_it_was_given():
    """Context.stream without a device: the attribute is set by set_stream alone (creating a Context needs a GPU)."""
    class Fake(native.Context):
        def __init__(self):
            self._h = None
            self.stream = None
    seen = []
    c = Fake()
    assert c.stream is None
    real = L.lib().emgpu_ctx_set_stream
    try:
        L.lib().emgpu_ctx_set_stream = lambda h, s: seen.append(s.value) or 0
        c.set_stream(0x1000)
        assert c.stream == 0x1000 and seen == [0x1000]
        c.set_stream(None)
        assert c.stream == 0 and seen[-1] in (0, None)
    finally:
        L.lib().emgpu_ctx_set_stream = real
