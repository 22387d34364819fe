"""CPU: the encounter-cylinder placement without a device -- the numpy restatement (encounter_ref) against the geometry and the statistics
its definition promises, every refusal of emgpu_encounter_pose_device (all of them come before any device work), and the binding against
the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import encounter_ref as R
from em_model_manned_bayes_amd import _lib as L, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, RADIUS, HALF_HEIGHT, SEED = 200_000, 6000.0, 800.0, 0x33C0FFEE
_cache = {}


def _straight(n, seed):
    """n straight tracks of two points, PLANAR [2, 3, n]: random starts, horizontal speeds of 40 .. 300 ft/s on random courses, climbs of
    -40 .. 40 ft/s"""
    rs = np.random.RandomState(seed)
    start = np.stack([rs.uniform(-20000.0, 20000.0, n), rs.uniform(-20000.0, 20000.0, n), rs.uniform(500.0, 9000.0, n)])
    speed, course = rs.uniform(40.0, 300.0, n), rs.uniform(-np.pi, np.pi, n)
    vel = np.stack([speed * np.cos(course), speed * np.sin(course), rs.uniform(-40.0, 40.0, n)])
    return np.ascontiguousarray(np.stack([start, start + vel]))


def _big(max_attempts=16):
    """the restatement on N pairs of straight tracks, computed once per max_attempts and shared (read-only)"""
    if max_attempts not in _cache:
        a, b = _straight(N, 1), _straight(N, 2)
        got = R.encounter(a, b, N, N, N, RADIUS, HALF_HEIGHT, SEED, max_attempts=max_attempts)
        for v in got.values():
            v.setflags(write=False)
        _cache[max_attempts] = (a, b, got)
    return _cache[max_attempts]


# ---- the restatement: geometry
def test_side_entries_lie_on_the_cylinder_facing_the_relative_velocity():
    _, _, got = _big()
    side = (got["flags"] & (R.END | R.NO_ENTRY | R.BAD_INDEX)) == 0
    assert 0.2 * N < side.sum() < 0.8 * N                                  # (the case holds plenty of both kinds)
    relx, rely, dz = got["rel"][:, side]
    rx, ry = got["rxy"][:, side]
    assert np.abs(np.hypot(relx, rely) - RADIUS).max() <= 1e-9 * RADIUS
    assert (relx * rx + rely * ry < 0.0).all()
    assert (np.abs(dz) <= HALF_HEIGHT).all()


def test_end_entries_lie_on_the_cap_the_intruder_flies_into():
    a, b, got = _big()
    end = (got["flags"] & R.END) != 0
    assert 0.2 * N < end.sum() < 0.8 * N and not (got["flags"] & (R.NO_ENTRY | R.BAD_INDEX)).any()
    relx, rely, dz = got["rel"][:, end]
    wr = ((b[1, 2] - b[0, 2]) - (a[1, 2] - a[0, 2]))[end]
    assert (np.abs(dz) == HALF_HEIGHT).all() and (dz[wr < 0.0] == HALF_HEIGHT).all() and (dz[wr >= 0.0] == -HALF_HEIGHT).all()
    # p' * p' + q' * q' <= 1 as rounded; R * p' and R * q' round once each and the hypotenuse once more: a few parts in 2^53
    assert (np.hypot(relx, rely) <= RADIUS * (1.0 + 1e-15 * 8)).all()
    assert np.hypot(relx, rely).max() > 0.99 * RADIUS and np.hypot(relx, rely).min() < 0.05 * RADIUS      # (the disc is filled)


def test_the_pose_puts_the_intruders_first_point_at_the_entry_point_and_turns_it_by_a_unit_vector():
    a, b, got = _big()
    c, s, ox, oy, oz = got["pose"]
    assert np.abs(c * c + s * s - 1.0).max() < 1e-15                       # (root, quotient, square, sum: each rounds within 2^-53)
    x = (c * b[0, 0] - s * b[0, 1]) + ox
    y = (s * b[0, 0] + c * b[0, 1]) + oy
    z = b[0, 2] + oz
    want = a[0] + got["rel"]
    assert np.abs(np.stack([x, y, z]) - want).max() < 1e-10 * 40000.0      # (coordinates of up to 4e4 ft, a handful of roundings)
    assert np.array_equal(got["rate"], got["Qs"] + (np.pi * RADIUS) * RADIUS * np.abs((b[1, 2] - b[0, 2]) - (a[1, 2] - a[0, 2])))


# ---- the restatement: statistics
def test_the_share_of_side_entries_is_the_sides_share_of_the_swept_volume():
    _, _, got = _big()
    side = (got["flags"] & R.END) == 0
    share = got["Qs"] / got["rate"]
    se = np.sqrt((share * (1.0 - share)).sum()) / N
    assert abs(side.mean() - share.mean()) <= 4.0 * se, (side.mean(), share.mean(), se)


def test_the_lateral_offset_is_centred():
    _, _, got = _big()
    side = (got["flags"] & R.END) == 0
    m = got["m"][side]
    se = (1.0 / np.sqrt(3.0)) / np.sqrt(side.sum())                        # m is uniform on (-1, 1)
    assert abs(m.mean()) <= 4.0 * se, (m.mean(), se)
    assert abs(m.var() - 1.0 / 3.0) < 0.01


def test_sixteen_attempts_never_fall_back_and_one_attempt_does_at_the_rate_of_the_corners():
    _, _, got = _big(16)
    assert not (got["flags"] & R.FALLBACK).any()
    gidx = np.arange(N, dtype=np.uint64)
    _, _, fb = R.disc_point(gidx, SEED, 0, 1)
    assert 0.15 <= fb.mean() <= 0.28, fb.mean()                            # 1 - pi / 4 = 0.215
    _, _, one = _big(1)
    heading_fell_back = (one["flags"] & R.FALLBACK) != 0
    assert (heading_fell_back | ~fb).all()                                 # the flag holds the heading's fallback (and an end cap's)
    side = (one["flags"] & R.END) == 0
    assert np.array_equal(heading_fell_back[side], fb[side])
    c, s = one["pose"][:2]
    assert (c[fb] == 1.0).all() and (s[fb] == 0.0).all()


def test_first_index_shifts_the_draws_and_a_bad_index_and_standing_still_have_their_own_rows():
    a, b = _straight(50, 3), _straight(50, 4)
    whole = R.encounter(a, b, 50, 50, 50, RADIUS, HALF_HEIGHT, 9)
    part = R.encounter(a[:, :, 20:], b[:, :, 20:], 30, 30, 30, RADIUS, HALF_HEIGHT, 9, first_index=20)
    assert np.array_equal(whole["pose"][:, 20:], part["pose"]) and np.array_equal(whole["flags"][20:], part["flags"])
    b2 = b.copy()
    b2[1, :, 7], a2 = b2[0, :, 7], a.copy()
    a2[1, :, 7] = a2[0, :, 7]                                              # pair 7: both stand still
    got = R.encounter(a2, b2, 50, 50, 50, RADIUS, HALF_HEIGHT, 9, idx_b=np.r_[np.arange(49), 50], weights_in=np.full(50, 3), rate_scale=1e9)
    assert got["flags"][7] == R.NO_ENTRY and got["rate"][7] == 0.0 and got["weights"][7] == 0
    assert np.isnan(got["pose"][2:, 7]).all() and np.array_equal(got["pose"][:2, 7], whole["pose"][:2, 7])
    assert got["flags"][49] == R.BAD_INDEX and np.isnan(got["pose"][:, 49]).all() and got["rate"][49] == 0.0 and got["weights"][49] == 0
    ok = np.ones(50, dtype=bool)
    ok[[7, 49]] = False
    assert np.array_equal(got["weights"][ok], np.floor(3.0 * (got["rate"][ok] / 1e9) + 0.5).astype(np.uint32))
    top = R.encounter(a, b, 50, 50, 50, RADIUS, HALF_HEIGHT, 9, weights_in=np.full(50, 2**32 - 1), rate_scale=1.0)
    assert (top["weights"] == 2**32 - 1).all() and (top["flags"] & R.SATURATED).all()


# ---- every refusal, through the library: none needs a device
def _call(p, xyz_a=True, xyz_b=True, idx_a=False, idx_b=False, weights_in=False, outs=(True, True, True, True)):
    buf = np.zeros(64)
    at = lambda yes: buf.ctypes.data_as(C.c_void_p) if yes else None          # noqa: E731
    lib = L.lib()
    rc = lib.emgpu_encounter_pose_device(None, C.byref(p) if p is not None else None, at(xyz_a), at(xyz_b), at(idx_a), at(idx_b), at(weights_in),
                                         *(at(o) for o in outs))
    return rc, lib.emgpu_last_error().decode()


def _refused(words, *a, **kw):
    rc, msg = _call(*a, **kw)
    assert rc == L.ERR_ARG and words in msg, (rc, msg)


def _ok(**kw):
    return native.encounter_params(**{**dict(n_pairs=4, n_a=4, n_b=4, points=3, radius_ft=6000.0, half_height_ft=800.0, seed=1), **kw})


def test_every_refusal_names_its_argument():
    _refused("null argument: p", None)
    _refused("null argument: xyz_a", _ok(), xyz_a=False)
    _refused("null argument: xyz_b", _ok(), xyz_b=False)
    _refused("nothing to write", _ok(), outs=(False,) * 4)
    _refused("points", _ok(points=1))
    _refused("points", _ok(points=0))
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
    for name in ("radius_ft", "half_height_ft", "rate_scale"):
        for value in (0.0, -1.0, float("nan"), float("inf")):
            _refused(name, _ok(**{name: value}))
    _refused("max_attempts", _ok(max_attempts=0))
    _refused("max_attempts", _ok(max_attempts=17))
    _refused("weights_in without weights_out", _ok(), weights_in=True, outs=(True, True, True, False))


def test_no_pairs_succeed_without_a_launch_and_the_limits_themselves_pass_the_checks():
    assert _call(_ok(n_pairs=0))[0] == L.OK
    assert _call(_ok(n_pairs=0, n_a=1, n_b=1, points=65537, ld_a=1, ld_b=9, max_attempts=1, first_index=2**64 - 1, seed=2**64 - 1))[0] == L.OK
    assert _call(_ok(n_pairs=0, points=2, max_attempts=16), weights_in=True)[0] == L.OK
    for k in range(4):                                                      # each output alone is enough
        assert _call(_ok(n_pairs=0), outs=tuple(j == k for j in range(4)))[0] == L.OK
    assert _call(_ok(n_pairs=0, n_a=1, n_b=1), idx_a=True, idx_b=True)[0] == L.OK


def test_weights_without_a_rate_scale_are_refused_before_the_library_is_called():
    xyz = np.zeros((2, 3, 3))
    for fn in (native.encounter_pose, native.encounter_miss):
        with pytest.raises(ValueError, match="rate_scale"):
            fn(xyz, xyz, 6000.0, 800.0, 1, weights=[1, 2])
        with pytest.raises(ValueError, match="rate_scale"):
            fn(xyz, xyz, 6000.0, 800.0, 1, weights=True)
        with pytest.raises(ValueError):
            fn(xyz, xyz, 6000.0, 800.0, 1, weights=[1, -1], rate_scale=1.0)


# ---- the binding against the header
def test_the_header_declares_the_entry_point_and_the_struct_the_binding_mirrors():
    hdr = open(os.path.join(ROOT, "include", "emgpu.h")).read()
    assert "emgpu_encounter_pose_device" in L.SYMBOLS and hasattr(L.lib(), "emgpu_encounter_pose_device")
    decl = re.search(r"int emgpu_encounter_pose_device\(([^)]*)\);", hdr).group(1)
    params = [s.strip() for s in decl.split(",")]
    assert len(params) == 11 == len(L.lib().emgpu_encounter_pose_device.argtypes)
    assert params[0] == "void *hip_stream" and params[1] == "const emgpu_encounter_params *p"
    assert "emgpu_ctx" not in decl and "emgpu_model" not in decl                   # the entry point takes no handle
    body = re.search(r"typedef struct \{([^}]*)\} emgpu_encounter_params;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "int32_t": C.c_int32, "double": C.c_double}
    fields = [(nm.strip(), ctype[ty]) for ty, names in re.findall(r"\b(int64_t|uint64_t|int32_t|double)\s+([^;]+);", body) for nm in names.split(",")]
    assert fields == list(L.EncounterParams._fields_)
    assert C.sizeof(L.EncounterParams) == 5 * 8 + 2 * 4 + 2 * 8 + 3 * 8
    for name in ("END", "FALLBACK", "NO_ENTRY", "SATURATED", "BAD_INDEX"):
        value = int(re.search(r"#define EMGPU_ENC_%s (\d+)u" % name, hdr).group(1))
        assert getattr(L, "ENC_" + name) == value == getattr(R, name)
    assert int(L.lib().emgpu_slot_map_revision()) == 2                              # section 13 is new: no existing draw moved
