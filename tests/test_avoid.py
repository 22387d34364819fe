"""CPU: the ownship's vertical avoidance without a device -- the numpy restatement (avoid_ref) against answers worked out by hand, the
conditions on the inputs that the GPU comparison relies on, every refusal of emgpu_avoid_device (all of them come before any device
work), and the binding against the header."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import avoid_ref as R
from em_model_manned_bayes_amd import _lib as L, native
from em_model_manned_bayes_amd import encounter_model as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_NAMES = ("ALERTED", "CLIMB", "NMAC_UNMIT", "NMAC_MIT", "LATE", "NO_CPA", "BAD_INDEX")
FLAGS = {name: getattr(L, "AVOID_" + name) for name in FLAG_NAMES}          # (a library without the entry point: nothing here is collected)
OUTS = ("hmd", "vmd", "vmd_mit", "t_cpa", "t_alert", "flags", "totals")
PARAMS = ("alert_tau_s=60.0, alert_dmod_ft=4000.0, alert_hmd_ft=4000.0, alert_h_ft=700.0, nmac_h_ft=500.0, nmac_v_ft=100.0, delay_s=5, "
          "rate_fps=25.0, accel_fps2=8.0, dz_max_ft=inf")


# ---- the restatement against hand-computed answers
@pytest.mark.parametrize("case", R.HAND, ids=[c[0] for c in R.HAND])
def test_hand_computed(case):
    _, (a, b), par = case[:3]
    got = R.avoid(R.planar(a), R.planar(b), 1, 1, 1, **par)
    R.pair_cases.same(got, R.hand_want(case), OUTS)


def test_the_hand_cases_cover_what_they_must():
    flags = [c[8] for c in R.HAND]
    induced = [f for f in flags if f & R.NMAC_MIT and not f & R.NMAC_UNMIT]
    resolved = [f for f in flags if f & R.NMAC_UNMIT and not f & R.NMAC_MIT]
    assert induced and resolved and any(f & R.LATE for f in flags) and any(f == 0 for f in flags) and any(f == R.NO_CPA for f in flags)
    assert any(f & R.CLIMB for f in resolved) and any(not f & R.CLIMB for f in resolved)                    # both senses resolve one
    assert any(f & R.NMAC_UNMIT and f & R.NMAC_MIT for f in flags)                                           # an unresolved one
    assert any(c[1][0].shape[1] == 1 for c in R.HAND)                                                        # P = 1
    assert sorted(c[5] for c in R.HAND if c[2]["accel_fps2"] == 8.0) == [-60.9375, -50.0, -36.0, -36.0, -16.0, -4.0]


def test_weights_totals_and_bad_indices_in_the_restatement():
    name, (a, b), par = R.HAND[0][:3]
    got = R.avoid(R.planar(a), R.planar(b), 1, 1, 1, weights=[7], totals=np.arange(12), **par)
    assert got["totals"].tolist() == [1, 2, 3, 3, 4, 5, 6, 14, 15, 16, 10, 11]                               # alerted, unmitigated NMAC
    a, b = R.encounters(3, 4, 1)
    got = R.avoid(R.planar(a), R.planar(b), 3, 3, 3, idx_a=[0, 3, 1], idx_b=[-1, 0, 1])
    assert got["flags"][:2].tolist() == [R.BAD_INDEX] * 2 and got["t_cpa"][:2].tolist() == [-1, -1] and got["t_alert"][:2].tolist() == [-1, -1]
    assert np.isnan(got["hmd"][:2]).all() and np.isnan(got["vmd"][:2]).all() and np.isnan(got["vmd_mit"][:2]).all()
    assert got["totals"][[0, 6, 7]].tolist() == [1, 2, 1]


def test_a_zero_rate_changes_nothing_in_the_restatement():
    a, b = R.encounters(257, 32, 2)
    got = R.avoid(R.planar(a), R.planar(b), 257, 257, 257, **dict(R.DEFAULTS, rate_fps=0.0))
    R.pair_cases.same({"vmd_mit": got["vmd_mit"]}, {"vmd_mit": got["vmd"]}, ("vmd_mit",))
    fl = got["flags"]
    assert np.array_equal((fl & R.NMAC_MIT) != 0, (fl & R.NMAC_UNMIT) != 0) and got["totals"][4] == 0 and got["totals"][2] > 0


# ---- the conditions on the generator's pairs
@pytest.mark.parametrize("P", [32, 64])
@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_encounters_take_every_outcome(n, P, seed):
    """conditions on the inputs, not on the kernel: without these the GPU comparison would leave an outcome unexercised"""
    a, b = R.encounters(n, P, seed)
    share = R.check_floors(R.avoid(R.planar(a), R.planar(b), n, n, n, **R.DEFAULTS), n, P, R.DEFAULTS)
    print(n, P, seed, {k: round(float(v), 3) for k, v in share.items()})
    for name in R.FLOORS:
        assert share[name] >= R.FLOOR, (name, share[name])
    rows_a, rows_b, pose = R.posed_encounters(n, P, seed)                       # the same pairs through a pose keep their outcomes, to rounding
    R.check_floors(R.avoid(R.planar(rows_a), R.planar(rows_b), n, n, n, pose_b=pose, **R.DEFAULTS), n, P, R.DEFAULTS)


@pytest.mark.parametrize("P", [3, 5])
@pytest.mark.parametrize("n", [257, 1000])
def test_short_tracks_are_late_and_a_prompt_response_still_resolves_some(n, P):
    a, b = R.encounters(n, P, 1)
    share = R.check_floors(R.avoid(R.planar(a), R.planar(b), n, n, n, **R.DEFAULTS), n, P, R.DEFAULTS)
    assert share["late"] >= R.LATE_FLOOR
    prompt = R.check_floors(R.avoid(R.planar(a), R.planar(b), n, n, n, **R.PROMPT), n, P, R.PROMPT)
    print(n, P, round(float(share["late"]), 3), round(float(prompt["resolved"]), 4))
    assert prompt["resolved"] > 0.0


# ---- every refusal, through the library: none needs a device
def _call(p, xyz_a=True, xyz_b=True, idx_a=False, idx_b=False, outs=(True,) * 7, shift=None):
    buf = np.zeros(64)
    at = lambda yes, by=0: C.c_void_p(buf.ctypes.data + by) if yes else None          # noqa: E731
    lib = L.lib()
    # behind p: xyz_a, xyz_b, idx_a, idx_b, pose_b, weights, hmd, vmd, vmd_mit, t_cpa, t_alert, flags, totals
    args = [at(xyz_a), at(xyz_b), at(idx_a), at(idx_b), None, None] + [at(o) for o in outs]
    if shift is not None:
        args[shift[0]] = at(True, shift[1])
    rc = lib.emgpu_avoid_device(None, C.byref(p) if p is not None else None, *args)
    return rc, lib.emgpu_last_error().decode()


def _refused(words, *a, **kw):
    rc, msg = _call(*a, **kw)
    assert rc == L.ERR_ARG and words in msg, (rc, msg)


def test_every_refusal_names_its_argument():
    ok = lambda **kw: native.avoid_params(**{**dict(n_pairs=4, n_a=4, n_b=4, points=3), **kw})          # noqa: E731
    _refused("null argument: p", None)
    _refused("null argument: xyz_a", ok(), xyz_a=False)
    _refused("null argument: xyz_b", ok(), xyz_b=False)
    _refused("null hmd, vmd, vmd_mit, t_cpa, t_alert, flags and totals: nothing to write", ok(), outs=(False,) * 7)
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
    for name in ("alert_tau_s", "alert_dmod_ft", "alert_hmd_ft", "alert_h_ft", "nmac_h_ft", "nmac_v_ft", "dz_max_ft"):
        _refused(name + " is negative or NaN", ok(**{name: -1.0}))
        _refused(name + " is negative or NaN", ok(**{name: float("nan")}))
    _refused("delay_s is negative", ok(delay_s=-1))
    for bad in (-1.0, float("nan"), float("inf")):
        _refused("rate_fps is negative, NaN or infinite", ok(rate_fps=bad))
    for bad in (0.0, -8.0, float("nan")):
        _refused("accel_fps2 is not positive or NaN", ok(accel_fps2=bad))
    # alignment: doubles, indices and totals 8 bytes; weights, t_cpa and t_alert 4
    for k in (0, 1, 2, 3, 4, 6, 7, 8, 12):
        _refused("must be 8-byte aligned", ok(), shift=(k, 4))
    for k in (5, 9, 10):
        _refused("weights, t_cpa and t_alert must be 4-byte aligned", ok(), shift=(k, 2))
    assert _call(ok(n_pairs=0), shift=(11, 1))[0] == L.OK                                                   # the byte array


def test_the_shared_refusals_carry_the_miss_calls_messages():
    def miss(p, xyz_a, xyz_b):
        buf = np.zeros(64)
        at = lambda yes: C.c_void_p(buf.ctypes.data) if yes else None          # noqa: E731
        lib = L.lib()
        rc = lib.emgpu_miss_distance_device(None, C.byref(p) if p is not None else None, at(xyz_a), at(xyz_b), None, None, None, None,
                                            *[at(True)] * 5)
        return rc, lib.emgpu_last_error().decode()
    for fault in (dict(no_p=True), dict(xyz_a=False), dict(xyz_b=False), dict(n_pairs=-1), dict(n_pairs=2**32 + 1, n_a=1, n_b=1), dict(n_a=0),
                  dict(n_b=0), dict(ld_a=3), dict(ld_b=3), dict(n_pairs=5, n_b=5), dict(n_pairs=5, n_a=5), dict(n_pairs=5, n_a=1),
                  dict(points=0), dict(points=65538)):
        fault = dict(fault)
        no_p, xyz_a, xyz_b = fault.pop("no_p", False), fault.pop("xyz_a", True), fault.pop("xyz_b", True)
        dims = {**dict(n_pairs=4, n_a=4, n_b=4, points=3), **fault}
        av = _call(None if no_p else native.avoid_params(**dims), xyz_a, xyz_b)
        sec = miss(None if no_p else native.miss_params(**dims), xyz_a, xyz_b)
        assert av == sec and av[0] == L.ERR_ARG and av[1], (fault, av, sec)


def test_no_pairs_succeed_without_a_launch_and_the_limits_themselves_pass_the_checks():
    assert _call(native.avoid_params(0, 4, 4, 3))[0] == L.OK
    zero = dict(alert_tau_s=0.0, alert_dmod_ft=0.0, alert_hmd_ft=0.0, alert_h_ft=0.0, nmac_h_ft=0.0, nmac_v_ft=0.0, delay_s=0, rate_fps=0.0,
                dz_max_ft=0.0)
    assert _call(native.avoid_params(0, 1, 1, 65537, ld_a=1, ld_b=9, **zero))[0] == L.OK
    inf = {k: np.inf for k in ("alert_tau_s", "alert_dmod_ft", "alert_hmd_ft", "alert_h_ft", "nmac_h_ft", "nmac_v_ft", "accel_fps2", "dz_max_ft")}
    assert _call(native.avoid_params(0, 1, 1, 1, delay_s=2**31 - 1, **inf))[0] == L.OK
    for k in range(7):                                   # each output alone is enough
        assert _call(native.avoid_params(0, 4, 4, 1), outs=tuple(j == k for j in range(7)))[0] == L.OK
    assert _call(native.avoid_params(0, 1, 1, 1), idx_a=True, idx_b=True)[0] == L.OK


def test_bad_python_arguments_are_refused_before_the_library_is_called():
    xyz = np.zeros((2, 3, 3))
    for w in ([1, -1], [1, 2**32], [1.0, 2.0], [1]):
        with pytest.raises(ValueError):
            native.avoid(xyz, xyz, weights=w)
    with pytest.raises(ValueError):
        native.avoid(xyz, xyz, pose_b=np.zeros((5, 3)))
    with pytest.raises(ValueError):
        native.cpa_avoid(xyz, xyz, 1000.0, 300.0, 1, 0, weights=True)          # weights need a rate_scale


# ---- the binding against the header
def test_the_header_declares_the_entry_point_the_binding_mirrors():
    hdr = open(os.path.join(ROOT, "include", "emgpu.h")).read()
    assert "emgpu_avoid_device" in L.SYMBOLS and hasattr(L.lib(), "emgpu_avoid_device")
    decl = re.search(r"int emgpu_avoid_device\(([^)]*)\);", hdr).group(1)
    params = [re.sub(r"/\*.*?\*/", "", s).strip() for s in decl.split(",")]
    assert len(params) == 15 == len(L.lib().emgpu_avoid_device.argtypes)
    assert params[0] == "void *hip_stream" and params[1] == "const emgpu_avoid_params *p"
    assert params[8:] == ["double *hmd", "double *vmd", "double *vmd_mit", "int32_t *t_cpa", "int32_t *t_alert", "uint8_t *flags", "uint64_t *totals"]
    assert "emgpu_ctx" not in decl and "emgpu_model" not in decl                   # the entry point takes no handle
    old = [s.strip() for s in re.search(r"int emgpu_miss_distance_device\(([^)]*)\);", hdr).group(1).split(",")]
    assert params[2:8] == old[2:8]                                                 # the inputs are the miss call's
    body = re.search(r"typedef struct \{([^}]*)\} emgpu_avoid_params;", hdr).group(1)
    fields = [f for decl in re.sub(r"/\*.*?\*/", "", body).split(";") for f in re.sub(r"^\s*\w+\s", "", decl.strip()).replace(" ", "").split(",") if f]
    assert fields == [f for f, _ in L.AvoidParams._fields_]
    assert fields[:6] == [f for f, _ in L.MissParams._fields_][:6] and fields[6] == "delay_s"          # the six pairing fields in emgpu_miss_params' order
    assert all(t is C.c_double for _, t in L.AvoidParams._fields_[7:]) and L.AvoidParams._fields_[6][1] is C.c_int32
    assert C.sizeof(L.AvoidParams) == 5 * 8 + 2 * 4 + 9 * 8 == 120


def test_the_seven_flags():
    hdr = open(os.path.join(ROOT, "include", "emgpu.h")).read()
    for k, name in enumerate(FLAG_NAMES):
        value = int(re.search(r"#define EMGPU_AVOID_%s (\d+)u" % name, hdr).group(1))
        assert FLAGS[name] == value == getattr(R, name) == 1 << k
    assert L.AVOID_NMAC_UNMIT != L.MISS_NMAC_ANY          # the bit moves: compare the events, not the bytes


def test_the_python_surface():
    sig = lambda f: str(inspect.signature(f))          # noqa: E731
    assert sig(native.avoid_params) == "(n_pairs, n_a, n_b, points, %s, ld_a=0, ld_b=0)" % PARAMS
    assert sig(native.avoid_device) == ("(params, xyz_a, xyz_b, idx_a=0, idx_b=0, pose_b=0, weights=0, hmd=0, vmd=0, vmd_mit=0, t_cpa=0, t_alert=0, "
                                        "flags=0, totals=0, stream=None)")
    assert sig(native.avoid) == "(xyz_a, xyz_b, idx_a=None, idx_b=None, pose_b=None, weights=None, %s, layout='rows', ctx=None, stream=None)" % PARAMS
    nmac = "nmac_h_ft=500.0, nmac_v_ft=100.0"
    assert sig(native.encounter_avoid) == sig(native.encounter_miss).replace(nmac, PARAMS)
    assert sig(native.cpa_avoid) == sig(native.cpa_miss).replace(nmac, PARAMS)
    assert sig(E.UncorEncounterModel.avoid) == ("(self, own_xyz, intruder_xyz, pose=None, weights=None, idx_own=None, idx_intruder=None, %s, "
                                                "layout='rows', ctx=None)" % PARAMS)
    assert callable(native._avoid_tensors) and callable(native._avoid_dict)
    p = native.avoid_params(7, 5, 6, 9, delay_s=3, rate_fps=30.0, ld_a=8)
    assert (p.n_pairs, p.n_a, p.n_b, p.ld_a, p.ld_b, p.points, p.delay_s) == (7, 5, 6, 8, 0, 9, 3)
    assert (p.alert_tau_s, p.alert_dmod_ft, p.alert_hmd_ft, p.alert_h_ft, p.nmac_h_ft, p.nmac_v_ft) == (60.0, 4000.0, 4000.0, 700.0, 500.0, 100.0)
    assert (p.rate_fps, p.accel_fps2, p.dz_max_ft) == (30.0, 8.0, np.inf)
