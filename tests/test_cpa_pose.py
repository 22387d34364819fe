"""CPU: the placement at a drawn closest approach without a device -- the numpy restatement (cpa_pose_ref) against the geometry and the
statistics its definition promises, every refusal of emgpu_cpa_pose_device (all of them come before any device work), and the binding
against the header."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cpa_pose_ref as R
import encounter_ref
import miss_ref
import miss_seg_ref
import pair_cases as PC
from em_model_manned_bayes_amd import _lib as L, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, P, T_LO, T_HI, HM, VM, SEED = 200_000, 41, 5, 30, 1000.0, 200.0, 0x37C0FFEE
_cache = {}


def _level(n, seed, lo, hi):
    """n level straight tracks of P points, PLANAR [P, 3, n]: starts within 8000 ft of the origin, speeds of lo .. hi ft/s on random
    courses, so that every coordinate stays below 2^15 ft"""
    rs = np.random.RandomState(seed)
    start = np.stack([rs.uniform(-8000.0, 8000.0, n), rs.uniform(-8000.0, 8000.0, n), rs.uniform(500.0, 9000.0, n)])
    speed, course = rs.uniform(lo, hi, n), rs.uniform(-np.pi, np.pi, n)
    vel = np.stack([speed * np.cos(course), speed * np.sin(course), np.zeros(n)])
    return np.ascontiguousarray(start[None] + vel[None] * np.arange(P, dtype=np.float64)[:, None, None])


def _big():
    """N level straight pairs, A at 50 .. 100 ft/s and B at 300 .. 400 ft/s (g >= 200 ft/s); the restatement on them and miss_ref.miss on
    the posed pairs; computed once and shared (read-only)"""
    if "big" not in _cache:
        a, b = _level(N, 1, 50.0, 100.0), _level(N, 2, 300.0, 400.0)
        got = R.cpa_pose(a, b, N, N, N, HM, VM, SEED, T_LO, T_HI)
        miss = miss_ref.miss(a, b, N, N, N, pose_b=got["pose"])
        for v in list(got.values()) + list(miss.values()):
            v.setflags(write=False)
        _cache["big"] = (a, b, got, miss)
    return _cache["big"]


# ---- the restatement: geometry
def test_the_offset_is_perpendicular_to_the_relative_velocity_and_inside_the_miss_plane():
    n, points, t_lo, t_hi = 600, 9, 2, 6
    a, b = PC.planar(PC.tracks(n, points, 1), n + 3), PC.planar(PC.tracks(n, points, 2), n + 9)
    got = R.cpa_pose(a, b, n, n, n, HM, VM, 5, t_lo, t_hi)
    assert not got["flags"].any()
    relx, rely, dz = got["rel"]
    ex, ey = got["e"]
    eps = 2.0 ** -53
    assert np.abs(relx * ex + rely * ey).max() <= 8.0 * eps * HM           # two products of |l| <= Hm and |e| <= 1, one sum
    assert np.abs(np.hypot(relx, rely) - np.abs(got["l"])).max() <= 16.0 * eps * HM
    assert (np.abs(got["l"]) <= HM).all() and (np.abs(dz) <= VM).all()
    assert np.abs(got["l"]).max() > 0.95 * HM and np.abs(dz).max() > 0.95 * VM                      # (the plane is filled)
    assert sorted(set(got["tc"].tolist())) == list(range(t_lo, t_hi + 1))                          # every second and nothing else
    assert np.array_equal(got["t_cpa"], got["tc"])
    # the pose puts B's point tc where the offsets say, turned by a unit vector
    c, s, ox, oy, oz = got["pose"]
    assert np.abs(c * c + s * s - 1.0).max() < 1e-15
    i, tc = np.arange(n), got["tc"]
    bx, by, bz = b[tc, 0, i], b[tc, 1, i], b[tc, 2, i]
    there = np.stack([(c * bx - s * by) + ox, (s * bx + c * by) + oy, bz + oz])
    assert np.abs(there - (np.stack([a[tc, 0, i], a[tc, 1, i], a[tc, 2, i]]) + got["rel"])).max() < 1e-10 * 40000.0
    assert np.array_equal(got["rate"], (4.0 * HM) * VM * got["g"])
    one = R.cpa_pose(a, b, n, n, n, HM, VM, 5, 7)                          # t_hi = None: that second, here the last legal one
    assert (one["t_cpa"] == 7).all()
    assert np.array_equal(one["pose"][:2], got["pose"][:2])                # the heading does not depend on the second


# ---- the restatement: the pass happens where it was put
def test_the_pass_happens_at_the_drawn_second_with_the_drawn_miss():
    """Level straight pairs: hmd is |l| and vmd is dz, to 1e-9 ft (coordinates below 2^15 ft, a few dozen operations: each rounds within
    2^-53 * 2^15 = 3.6e-12 ft), at the drawn second (a second earlier or later the pair is g >= 200 ft further along)."""
    _, _, got, miss = _big()
    assert not got["flags"].any() and (got["g"] >= 200.0).all()
    assert np.array_equal(miss["t_cpa"], got["t_cpa"])
    assert sorted(set(got["t_cpa"].tolist())) == list(range(T_LO, T_HI + 1))
    dh, dv = np.abs(miss["hmd"] - np.abs(got["l"])).max(), np.abs(miss["vmd"] - got["rel"][2]).max()
    print("largest |hmd - |l|| %.3g ft, |vmd - dz| %.3g ft" % (dh, dv))
    assert dh <= 1e-9 and dv <= 1e-9


# ---- the restatement: the rate is the flux
def test_the_rate_is_the_flux_through_the_miss_plane():
    a, b, got, miss = _big()
    nmac = (miss["flags"] & miss_ref.NMAC_CPA) != 0
    share = nmac.mean()
    print("NMAC share %.4f" % share)
    assert abs(share - 0.25) <= 5.0 * np.sqrt(0.25 * 0.75 / N)             # (500 / 1000) * (100 / 200); 5 binomial standard errors: 0.0049
    x = got["rate"] * nmac
    est, se = x.mean(), x.std() / np.sqrt(N)
    # the cylinder placement on the same pairs: R 2000, H 400, the NMAC at any time of the segment miss distance
    enc = encounter_ref.encounter(a, b, N, N, N, 2000.0, 400.0, SEED)
    seg = miss_seg_ref.miss_segments(a, b, N, N, N, pose_b=enc["pose"])
    y = enc["rate"] * ((seg["flags"] & miss_seg_ref.NMAC_ANY) != 0)
    est_cyl, se_cyl = y.mean(), y.std() / np.sqrt(N)
    exact = 4.0 * 500.0 * 100.0 * got["g"].mean()
    d = (abs(est - est_cyl) / np.hypot(se, se_cyl), abs(est - exact) / se, abs(est_cyl - exact) / se_cyl)
    print("E[rate NMAC]: CPA %.4e +- %.2e, cylinder %.4e +- %.2e, exact %.4e; differences in standard errors %.2f %.2f %.2f"
          % (est, se, est_cyl, se_cyl, exact, *d))
    assert max(d) <= 5.0, d
    assert se < se_cyl                                                     # what the placement is for


# ---- draws, bad indices, weights
def test_first_index_shifts_the_draws_and_a_bad_index_and_standing_still_have_their_own_rows():
    n, points, k = 50, 6, 20
    a, b = PC.planar(PC.tracks(n, points, 3)), PC.planar(PC.tracks(n, points, 4))
    whole = R.cpa_pose(a, b, n, n, n, HM, VM, 9, 1, 4)
    part = R.cpa_pose(a[:, :, k:], b[:, :, k:], n - k, n - k, n - k, HM, VM, 9, 1, 4, first_index=k)
    for name in ("pose", "rate", "t_cpa", "flags", "weights"):
        assert np.array_equal(whole[name][..., k:], part[name]), name
    a2, b2 = a.copy(), b.copy()
    a2[1:, :, 7], b2[1:, :, 7] = a2[0, :, 7], b2[0, :, 7]                  # pair 7: both stand still
    got = R.cpa_pose(a2, b2, n, n, n, HM, VM, 9, 1, 4, idx_b=np.r_[np.arange(n - 1), n], weights_in=np.full(n, 3), rate_scale=1e7)
    assert got["flags"][7] == R.NO_PASS and got["rate"][7] == 0.0 and got["weights"][7] == 0 and got["t_cpa"][7] == whole["t_cpa"][7]
    assert np.isnan(got["pose"][2:, 7]).all() and np.array_equal(got["pose"][:2, 7], whole["pose"][:2, 7])
    assert got["flags"][49] == R.BAD_INDEX and np.isnan(got["pose"][:, 49]).all() and got["rate"][49] == 0.0 and got["weights"][49] == 0
    assert got["t_cpa"][49] == -1
    ok = np.ones(n, dtype=bool)
    ok[[7, 49]] = False
    assert np.array_equal(got["weights"][ok], np.floor(3.0 * (got["rate"][ok] / 1e7) + 0.5).astype(np.uint32)) and got["weights"][ok].max() > 3
    top = R.cpa_pose(a, b, n, n, n, HM, VM, 9, 1, 4, weights_in=np.full(n, 2**32 - 1), rate_scale=1.0)
    assert (top["weights"] == 2**32 - 1).all() and (top["flags"] & R.SATURATED).all()
    _, _, fb = encounter_ref.disc_point(np.arange(1000, dtype=np.uint64), 9, 3, 1)
    one = R.cpa_pose(a[:, :, :1], b[:, :, :1], 1, 1, 1000, HM, VM, 9, 1, 4, max_attempts=1)
    assert 0.15 <= fb.mean() <= 0.28 and np.array_equal((one["flags"] & R.FALLBACK) != 0, fb)          # 1 - pi / 4 = 0.215
    assert (one["pose"][0, fb] == 1.0).all() and (one["pose"][1, fb] == 0.0).all()


# ---- every refusal, through the library: none needs a device
def _call(p, xyz_a=True, xyz_b=True, idx_a=False, idx_b=False, weights_in=False, outs=(True,) * 5):
    buf = np.zeros(64)
    at = lambda yes: buf.ctypes.data_as(C.c_void_p) if yes else None          # noqa: E731
    lib = L.lib()
    rc = lib.emgpu_cpa_pose_device(None, C.byref(p) if p is not None else None, at(xyz_a), at(xyz_b), at(idx_a), at(idx_b), at(weights_in),
                                   *(at(o) for o in outs))
    return rc, lib.emgpu_last_error().decode()


def _refused(words, *a, **kw):
    rc, msg = _call(*a, **kw)
    assert rc == L.ERR_ARG and words in msg, (rc, msg)


def _ok(**kw):
    return native.cpa_pose_params(**{**dict(n_pairs=4, n_a=4, n_b=4, points=5, hmd_max_ft=1000.0, vmd_max_ft=200.0, seed=1, t_lo=1, t_hi=3), **kw})


def test_every_refusal_names_its_argument():
    _refused("null argument: p", None)
    _refused("null argument: xyz_a", _ok(), xyz_a=False)
    _refused("null argument: xyz_b", _ok(), xyz_b=False)
    _refused("nothing to write", _ok(), outs=(False,) * 5)
    _refused("points", _ok(points=1, t_lo=0, t_hi=0))
    _refused("points", _ok(points=0, t_lo=0, t_hi=0))
    _refused("points", _ok(points=65538))
    _refused("n_pairs", _ok(n_pairs=-1))
    _refused("n_pairs", _ok(n_pairs=2**32 + 1, n_a=1, n_b=1))
    _refused("n_a", _ok(n_a=0))
    _refused("n_b", _ok(n_b=0))
    _refused("ld_a", _ok(ld_a=3))
    _refused("ld_b", _ok(ld_b=3))
    _refused("idx_a", _ok(n_pairs=5, n_b=5))
    _refused("idx_b", _ok(n_pairs=5, n_a=5))
    _refused("idx_b", _ok(n_pairs=5, n_a=1))
    for name in ("hmd_max_ft", "vmd_max_ft", "rate_scale"):
        for value in (0.0, -1.0, float("nan"), float("inf")):
            _refused(name, _ok(**{name: value}))
    _refused("max_attempts", _ok(max_attempts=0))
    _refused("max_attempts", _ok(max_attempts=17))
    _refused("t_lo", _ok(t_lo=-1))
    _refused("t_hi < t_lo", _ok(t_lo=3, t_hi=2))
    _refused("t_hi > points - 2", _ok(t_hi=4))
    _refused("t_hi > points - 2", _ok(points=2, t_lo=1, t_hi=1))
    _refused("weights_in without weights_out", _ok(), weights_in=True, outs=(True, True, True, True, False))


def test_no_pairs_succeed_without_a_launch_and_the_limits_themselves_pass_the_checks():
    assert _call(_ok(n_pairs=0))[0] == L.OK
    assert _call(_ok(n_pairs=0, n_a=1, n_b=1, points=65537, t_lo=0, t_hi=65535, ld_a=1, ld_b=9, max_attempts=1, first_index=2**64 - 1,
                     seed=2**64 - 1))[0] == L.OK
    assert _call(_ok(n_pairs=0, points=2, t_lo=0, t_hi=0, max_attempts=16), weights_in=True)[0] == L.OK
    assert _call(_ok(n_pairs=0, t_lo=3, t_hi=3))[0] == L.OK                  # the last legal second
    for k in range(5):                                                      # each output alone is enough
        assert _call(_ok(n_pairs=0), outs=tuple(j == k for j in range(5)))[0] == L.OK
    assert _call(_ok(n_pairs=0, n_a=1, n_b=1), idx_a=True, idx_b=True)[0] == L.OK
    assert native.cpa_pose_params(1, 1, 1, 9, 1.0, 1.0, 0, 4).t_hi == 4      # t_hi = None is t_lo


def test_weights_without_a_rate_scale_are_refused_before_the_library_is_called():
    xyz = np.zeros((2, 3, 3))
    for fn in (native.cpa_pose, native.cpa_miss, native.cpa_miss_segments):
        with pytest.raises(ValueError, match="rate_scale"):
            fn(xyz, xyz, 1000.0, 200.0, 1, 0, weights=[1, 2])
        with pytest.raises(ValueError, match="rate_scale"):
            fn(xyz, xyz, 1000.0, 200.0, 1, 0, weights=True)
        with pytest.raises(ValueError):
            fn(xyz, xyz, 1000.0, 200.0, 1, 0, weights=[1, -1], rate_scale=1.0)
        with pytest.raises(ValueError):
            fn(xyz, xyz, 1000.0, 200.0, 1, 0, weights=[1, 2**32], rate_scale=1.0)


# ---- the binding against the header
def test_the_header_declares_the_entry_point_and_the_struct_the_binding_mirrors():
    hdr = open(os.path.join(ROOT, "include", "emgpu.h")).read()
    assert "emgpu_cpa_pose_device" in L.SYMBOLS and hasattr(L.lib(), "emgpu_cpa_pose_device")
    decl = re.search(r"int emgpu_cpa_pose_device\(([^)]*)\);", hdr).group(1)
    params = [s.strip() for s in decl.split(",")]
    assert len(params) == 12 == len(L.lib().emgpu_cpa_pose_device.argtypes)
    assert params[0] == "void *hip_stream" and params[1] == "const emgpu_cpa_pose_params *p"
    assert "emgpu_ctx" not in decl and "emgpu_model" not in decl                   # the entry point takes no handle
    body = re.search(r"typedef struct \{([^}]*)\} emgpu_cpa_pose_params;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "int32_t": C.c_int32, "double": C.c_double}
    fields = [(nm.strip(), ctype[ty]) for ty, names in re.findall(r"\b(int64_t|uint64_t|int32_t|double)\s+([^;]+);", body) for nm in names.split(",")]
    assert fields == list(L.CpaPoseParams._fields_)
    assert C.sizeof(L.CpaPoseParams) == 5 * 8 + 2 * 4 + 2 * 8 + 2 * 4 + 3 * 8
    for name in ("FALLBACK", "NO_PASS", "SATURATED", "BAD_INDEX"):
        value = int(re.search(r"#define EMGPU_CPA_%s (\d+)u" % name, hdr).group(1))
        assert getattr(L, "CPA_" + name) == value == getattr(R, name)
    assert (L.CPA_FALLBACK, L.CPA_NO_PASS, L.CPA_SATURATED, L.CPA_BAD_INDEX) == (L.ENC_FALLBACK, L.ENC_NO_ENTRY, L.ENC_SATURATED, L.ENC_BAD_INDEX)
    assert int(L.lib().emgpu_slot_map_revision()) == 2                              # two new streams of section 13: no existing draw moved


def test_the_python_surface():
    sig = lambda f: str(inspect.signature(f))          # noqa: E731
    assert sig(native.cpa_pose_params) == ("(n_pairs, n_a, n_b, points, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi=None, first_index=0, "
                                           "max_attempts=16, rate_scale=1.0, ld_a=0, ld_b=0)")
    assert sig(native.cpa_pose_device) == ("(params, xyz_a, xyz_b, idx_a=0, idx_b=0, weights_in=0, pose=0, rate=0, t_cpa=0, flags=0, "
                                           "weights_out=0, stream=None)")
    assert sig(native.cpa_miss) == sig(native.cpa_miss_segments)
    assert sig(native.cpa_pose).startswith("(xyz_a, xyz_b, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi=None, ")
    from em_model_manned_bayes_amd.encounter_model import UncorEncounterModel
    assert sig(UncorEncounterModel.encounter_cpa).startswith(
        "(self, own_xyz, intruder_xyz, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi=None, weights=None, rate_scale=None, between=False, ")
