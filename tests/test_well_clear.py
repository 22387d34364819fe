"""CPU: loss of DAA well clear without a device -- the numpy restatement (well_clear_ref) against answers worked out by hand, the
conditions on the inputs that the GPU comparison relies on, every refusal of emgpu_well_clear_device (all of them come before any device
work), and the binding against the header."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import well_clear_ref as R
from em_model_manned_bayes_amd import _lib as L, native
from em_model_manned_bayes_amd import encounter_model as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(n, P) for n in (257, 1000) for P in (2, 3, 5, 64)]          # the GPU test's cases of 257 pairs and more, with a velocity
FLAG_NAMES = ("LOST", "AT_START", "NO_DATA", "BAD_INDEX", "INSIDE_DMOD", "BY_TAU")


# ---- the restatement against hand-computed answers
@pytest.mark.parametrize("case", R.HAND, ids=[c[0] for c in R.HAND])
def test_hand_computed(case):
    _, (a, b), thr, t_first, n_lost, tau_min, flags, wide = case
    got = R.well_clear(R.planar(a), R.planar(b), 1, 1, 1, **thr)
    want = {"t_first": np.array([t_first], dtype=np.int32), "n_lost": np.array([n_lost], dtype=np.int32), "tau_min": np.array([tau_min]),
            "flags": np.array([flags], dtype=np.uint8), "wide": np.array([wide])}
    R.pair_cases.same(got, want, ("t_first", "n_lost", "tau_min", "flags", "wide"))
    lost, start, none = flags & 1, (flags >> 1) & 1, (flags >> 2) & 1
    assert got["totals"].tolist() == [1, lost, start, none, 0, 1, lost, start, 0, 0]


def test_weights_miss_flags_and_bad_indices_in_the_restatement():
    (a, b), thr = R.HAND[0][1], R.HAND[0][2]
    got = R.well_clear(R.planar(a), R.planar(b), 1, 1, 1, weights=[7], miss_flags=[R.MISS_NMAC_ANY], totals=np.arange(10), **thr)
    assert got["totals"].tolist() == [1, 2, 3, 3, 4, 12, 13, 14, 9, 16]
    got = R.well_clear(R.planar(a), R.planar(b), 1, 1, 1, weights=[7], miss_flags=[1 | 4], **thr)          # no NMAC_ANY among the miss flags
    assert got["totals"].tolist() == [1, 1, 1, 0, 0, 7, 7, 7, 0, 0]
    a, b = R.approaching(3, 4, 1)
    got = R.well_clear(R.planar(a), R.planar(b), 3, 3, 3, idx_a=[0, 3, 1], idx_b=[-1, 0, 1], miss_flags=[2, 2, 2])
    assert got["flags"][:2].tolist() == [R.BAD_INDEX] * 2 and got["t_first"][:2].tolist() == [-1, -1] and got["n_lost"][:2].tolist() == [0, 0]
    assert np.isnan(got["tau_min"][:2]).all() and got["totals"][[0, 4]].tolist() == [1, 2]


@pytest.mark.parametrize("n,P", SHAPES)
def test_the_approaching_cases_take_every_branch(n, P):
    """conditions on the inputs, not on the kernel: without these the GPU comparison would leave a branch of the predicate unexercised"""
    a, b = R.approaching(n, P, 1)
    share = R.shares(R.well_clear(R.planar(a), R.planar(b), n, n, n), n)
    print(n, P, {k: round(float(v), 3) for k, v in share.items()})
    for name, floor in R.FLOORS.items():
        assert share[name] >= floor, (name, share[name])
    if P == 64:
        assert share["later"] >= 0.05


# ---- every refusal, through the library: none needs a device
def _call(p, xyz_a=True, xyz_b=True, idx_a=False, idx_b=False, outs=(True,) * 5, shift=None):
    buf = np.zeros(64)
    at = lambda yes, by=0: C.c_void_p(buf.ctypes.data + by) if yes else None          # noqa: E731
    lib = L.lib()
    # behind p: xyz_a, xyz_b, idx_a, idx_b, pose_b, weights, miss_flags, t_first, n_lost, tau_min, flags, totals
    args = [at(xyz_a), at(xyz_b), at(idx_a), at(idx_b), None, None, None] + [at(o) for o in outs]
    if shift is not None:
        args[shift[0]] = at(True, shift[1])
    rc = lib.emgpu_well_clear_device(None, C.byref(p) if p is not None else None, *args)
    return rc, lib.emgpu_last_error().decode()


def _refused(words, *a, **kw):
    rc, msg = _call(*a, **kw)
    assert rc == L.ERR_ARG and words in msg, (rc, msg)


def test_every_refusal_names_its_argument():
    ok = lambda **kw: native.well_clear_params(**{**dict(n_pairs=4, n_a=4, n_b=4, points=3), **kw})          # noqa: E731
    _refused("null argument: p", None)
    _refused("null argument: xyz_a", ok(), xyz_a=False)
    _refused("null argument: xyz_b", ok(), xyz_b=False)
    _refused("null t_first, n_lost, tau_min, flags and totals: nothing to write", ok(), outs=(False,) * 5)
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
    for name in ("tau_s", "dmod_ft", "hmd_ft", "h_ft"):
        _refused(name + " is negative or NaN", ok(**{name: -1.0}))
        _refused(name + " is negative or NaN", ok(**{name: float("nan")}))
    # alignment: doubles, indices and totals 8 bytes; weights, t_first and n_lost 4
    for k in (0, 1, 2, 3, 4, 9, 11):
        _refused("must be 8-byte aligned", ok(), shift=(k, 4))
    for k in (5, 7, 8):
        _refused("weights, t_first and n_lost must be 4-byte aligned", ok(), shift=(k, 2))
    assert _call(ok(n_pairs=0), shift=(6, 1))[0] == L.OK and _call(ok(n_pairs=0), shift=(10, 1))[0] == L.OK          # the two byte arrays


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
        wc = _call(None if no_p else native.well_clear_params(**dims), xyz_a, xyz_b)
        sec = miss(None if no_p else native.miss_params(**dims), xyz_a, xyz_b)
        assert wc == sec and wc[0] == L.ERR_ARG and wc[1], (fault, wc, sec)


def test_no_pairs_succeed_without_a_launch_and_the_limits_themselves_pass_the_checks():
    assert _call(native.well_clear_params(0, 4, 4, 3))[0] == L.OK
    assert _call(native.well_clear_params(0, 1, 1, 65537, tau_s=0.0, dmod_ft=0.0, hmd_ft=0.0, h_ft=0.0, ld_a=1, ld_b=9))[0] == L.OK
    assert _call(native.well_clear_params(0, 1, 1, 1, tau_s=np.inf, dmod_ft=np.inf, hmd_ft=np.inf, h_ft=np.inf))[0] == L.OK
    for k in range(5):                                   # each output alone is enough
        assert _call(native.well_clear_params(0, 4, 4, 1), outs=tuple(j == k for j in range(5)))[0] == L.OK
    assert _call(native.well_clear_params(0, 1, 1, 1), idx_a=True, idx_b=True)[0] == L.OK


def test_bad_python_arguments_are_refused_before_the_library_is_called():
    xyz = np.zeros((2, 3, 3))
    for w in ([1, -1], [1, 2**32], [1.0, 2.0], [1]):
        with pytest.raises(ValueError):
            native.well_clear(xyz, xyz, weights=w)
    with pytest.raises(ValueError):
        native.well_clear(xyz, xyz, pose_b=np.zeros((5, 3)))
    for mf in (np.zeros(3, dtype=np.uint8), np.zeros(2, dtype=np.int32), np.zeros((2, 1), dtype=np.uint8)):
        with pytest.raises(ValueError):
            native.well_clear(xyz, xyz, miss_flags=mf)


# ---- the binding against the header
def test_the_header_declares_the_entry_point_the_binding_mirrors():
    hdr = open(os.path.join(ROOT, "include", "emgpu.h")).read()
    assert "emgpu_well_clear_device" in L.SYMBOLS and hasattr(L.lib(), "emgpu_well_clear_device")
    decl = re.search(r"int emgpu_well_clear_device\(([^)]*)\);", hdr).group(1)
    params = [re.sub(r"/\*.*?\*/", "", s).strip() for s in decl.split(",")]
    assert len(params) == 14 == len(L.lib().emgpu_well_clear_device.argtypes)
    assert params[0] == "void *hip_stream" and params[1] == "const emgpu_well_clear_params *p"
    assert params[8:] == ["const uint8_t *miss_flags", "int32_t *t_first", "int32_t *n_lost", "double *tau_min", "uint8_t *flags", "uint64_t *totals"]
    assert "emgpu_ctx" not in decl and "emgpu_model" not in decl                   # the entry point takes no handle
    old = [s.strip() for s in re.search(r"int emgpu_miss_distance_device\(([^)]*)\);", hdr).group(1).split(",")]
    assert params[2:8] == old[2:8]                                                 # the inputs are the miss call's
    body = re.search(r"typedef struct \{([^}]*)\} emgpu_well_clear_params;", hdr).group(1)
    fields = [f for decl in re.sub(r"/\*.*?\*/", "", body).split(";") for f in re.sub(r"^\s*\w+\s", "", decl.strip()).replace(" ", "").split(",") if f]
    assert fields == [f for f, _ in L.WellClearParams._fields_]
    assert fields[:7] == [f for f, _ in L.MissParams._fields_][:7]                 # the six pairing fields in emgpu_miss_params' order, reserved
    assert C.sizeof(L.WellClearParams) == 5 * 8 + 2 * 4 + 4 * 8 == 80


def test_the_six_flags():
    hdr = open(os.path.join(ROOT, "include", "emgpu.h")).read()
    for k, name in enumerate(FLAG_NAMES):
        value = int(re.search(r"#define EMGPU_WC_%s (\d+)u" % name, hdr).group(1))
        assert getattr(L, "WC_" + name) == value == getattr(R, name) == 1 << k
    assert L.WC_BAD_INDEX == L.MISS_BAD_INDEX and R.MISS_NMAC_ANY == L.MISS_NMAC_ANY


def test_the_python_surface():
    sig = lambda f: str(inspect.signature(f))          # noqa: E731
    thr = "tau_s=35.0, dmod_ft=4000.0, hmd_ft=4000.0, h_ft=450.0"
    assert sig(native.well_clear_params) == "(n_pairs, n_a, n_b, points, %s, ld_a=0, ld_b=0)" % thr
    assert sig(native.well_clear_device) == ("(params, xyz_a, xyz_b, idx_a=0, idx_b=0, pose_b=0, weights=0, miss_flags=0, t_first=0, n_lost=0, "
                                             "tau_min=0, flags=0, totals=0, stream=None)")
    assert sig(native.well_clear) == ("(xyz_a, xyz_b, idx_a=None, idx_b=None, pose_b=None, weights=None, miss_flags=None, %s, layout='rows', "
                                      "ctx=None, stream=None)" % thr)
    assert sig(native.encounter_well_clear) == sig(native.encounter_miss).replace("layout=", "between=False, %s, layout=" % thr)
    assert sig(native.cpa_well_clear) == sig(native.cpa_miss).replace("layout=", "between=False, %s, layout=" % thr)
    assert sig(E.UncorEncounterModel.well_clear) == ("(self, own_xyz, intruder_xyz, pose=None, weights=None, idx_own=None, idx_intruder=None, "
                                                     "miss_flags=None, %s, layout='rows', ctx=None)" % thr)
    assert callable(native._well_clear_tensors) and callable(native._well_clear_dict)
    # the methods beside it keep their signatures
    assert list(inspect.signature(E.UncorEncounterModel.pair).parameters)[-1] == "between"
    assert inspect.signature(E.UncorEncounterModel.encounter).parameters["between"].default is False
    assert inspect.signature(E.UncorEncounterModel.encounter_cpa).parameters["between"].default is False
