"""CPU: the hand-made terminal-filter cases are what they claim to be, before a device sees them (test_gpu_terminal_filter.py), and the two
entry points that hand them to the device refuse bad arguments before any device work.

A case is a pair of encounters around one accepted base encounter (terminal_filter_cases.py).  Here: the two restatements of the filters,
em_oracle.c and pyref.py, agree on every side in decision and in the bits of meta; exactly one side of every case is accepted; the filter
the case names, computed on its own by pyref's function for it, flips between the sides while every other filter passes on both -- so no
filter hides behind another; and the packer writes blocks from which the rows come back."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import pyref as P
import terminal_filter_cases as K
import terminal_filter_ref as R
from em_model_manned_bayes_amd import _lib as L, native

IDS = [c["name"] for c in K.CASES]


def test_the_case_list_covers_every_family_and_every_filter():
    assert set(K.FAMILIES) == {"cpa", "enc_time", "proximity", "vertical", "heading", "limits", "cum_turn", "void"}
    assert {c["filter"] for c in K.CASES} == set(K.FILTERS)
    assert len(IDS) == len(set(IDS)) >= 60


@pytest.mark.parametrize("c", K.CASES, ids=IDS)
def test_the_restatements_agree_and_one_side_is_accepted(c):
    goods = []
    for s in c["sides"]:
        good, meta = R.oracle(s)
        if not s["void"]:
            good_p, meta_p = R.pyref(s)
            assert good == good_p and np.array_equal(meta.view(np.int64), meta_p.view(np.int64)), (c["name"], good, good_p, meta, meta_p)
        goods.append(good)
    assert goods == [True, False], c["name"]             # the accepted side is written first


@pytest.mark.parametrize("c", K.CASES, ids=IDS)
def test_one_filter_decides_each_case(c):
    a, b = (R.named_filters(s) for s in c["sides"])
    assert all(a.values()), (c["name"], [k for k, v in a.items() if not v])
    assert [k for k, v in b.items() if not v] == [c["filter"]], c["name"]


def test_the_base_encounter_is_the_issue_s():
    own, intr = K.BASE["own"], K.BASE["intr"]
    assert (own[0, 0], own[-1, 0], intr[0, 0], intr[-1, 0]) == (-20, 20, -15, 25) and K.BASE["intents"] == (1, 3)
    assert own[20, 3] == 900 and np.all(np.diff(own[:, 3]) == -8) and np.all(own[:, 4] == 90) and np.all(own[:, 5] == 190)
    assert np.all(intr[:, 3] == 2500) and np.all(intr[:, 4] == 200) and np.all(intr[:, 5] == 95)
    good, meta = R.oracle(K.BASE)
    assert good and meta[0] == 0 and meta[2] == 1600 and meta[3] == 36 and meta[1] == np.sqrt(0.375 * 0.375 + 1.0) * 6076.1154855643


def test_two_tracks_without_a_common_second_are_rejected_by_both_restatements():
    own, intr = K.NO_COMMON
    o = K.DEFAULT
    good, meta = O.terminal_filters(own, intr, 1, 3, o["dl"], o["cum"], o["pitch"])
    good_p, meta_p = P.terminal_filters([R.as_dict(own), R.as_dict(intr)], 1, 3, R.dl_dicts(o), o["cum"], o["pitch"])
    assert not good and not good_p and np.array_equal(meta, np.zeros(4)) and np.array_equal(np.array(meta_p), np.zeros(4))


def test_check_cum_turn_known_answers():
    """CheckCumTurn (CorTerminalModel.m:135-185) on hand-made headings, in both restatements: a steady 3 deg/s turn through 210 deg is
    rejected at 180, the same amount split into a left and a right turn is not.  The device sees the same headings in the cases
    steady_zigzag and steady_limit_inf_180 (test_gpu_terminal_filter.py)."""
    for ref in (O, P):
        assert ref.check_cum_turn(K.STEADY, 180.0) and not ref.check_cum_turn(K.ZIGZAG, 180.0) and not ref.check_cum_turn(K.STEADY, np.inf)
    used = {id(s["intr"]) for c in K.CASES if c["name"] in ("steady_zigzag", "steady_limit_inf_180") for s in c["sides"]}
    assert len(used) >= 3
    for c in K.CASES:
        if c["name"] == "steady_zigzag":
            assert np.array_equal(c["sides"][0]["intr"][:, 4], K.ZIGZAG) and np.array_equal(c["sides"][1]["intr"][:, 4], K.STEADY)


def test_the_packer_round_trips():
    for opts, sides in K.batches(K.sides_of()):
        cap = opts["cap"]
        geo, tracks, rows = K.pack(sides, cap)
        assert tracks.dtype == np.float32 and tracks.shape == (2 * len(sides), 2 * K.t0_row(cap), 5) and rows.shape == (4 * len(sides),)
        back = K.unpack(tracks, rows, cap)
        live = np.zeros(tracks.shape[:2], dtype=bool)
        for e, (s, pair) in enumerate(zip(sides, back)):
            assert (geo[e, 5], geo[e, 11]) == s["intents"]
            for a, want in enumerate((s["own"], s["intr"])):
                if s["void"] and s["void"][0] // 2 == a:
                    assert pair[a] is None
                else:
                    assert np.array_equal(pair[a], want)
                lo = K.t0_row(cap) + int(want[0, 0])
                live[2 * e + a, lo: lo + want.shape[0]] = True
        assert np.isnan(tracks[~live]).all() and not np.isnan(tracks[live]).any()     # every row outside a span is poison
        assert rows.max() <= cap


def test_the_smooth_blocks_are_inexact_and_asymmetric():
    tracks, rows = K.smooth_block(((8, 8), (0, 3)), 8, 1)
    z = tracks[0, 1:16, 2].astype(np.float64)
    assert not np.array_equal(z, z[::-1]) and np.float32(z[:5].sum()) != z[:5].sum()
    assert not np.isnan(tracks[1]).any() and np.isnan(tracks[0, 0]).all()
    want = R.smoothed(tracks, rows, 8)
    assert np.array_equal(want[1], tracks[1]) and not np.array_equal(want[0, 1:16, 2], tracks[0, 1:16, 2])
    assert np.array_equal(want[0, 1:16, [0, 1, 3]], tracks[0, 1:16, [0, 1, 3]])
    assert want[0, 1, 2] == tracks[0, 1, 2] and want[0, 15, 4] == tracks[0, 15, 4]          # a window of one row at either end


# ---- the entry points' refusals: all before any device work, so they are seen without a device
def _filter(p, geo=64, tracks=64, rows=64, accepted=64, meta=0, ln=0, traj=0):
    ptr = lambda a: C.c_void_p(a or None)          # noqa: E731  (never dereferenced: the call is refused first, or n == 0)
    rc = L.lib().emgpu_filter_terminal_device(None, None if p is None else C.byref(p), ptr(geo), ptr(tracks), ptr(rows), ptr(accepted), ptr(meta), ptr(ln), ptr(traj))
    return rc, L.lib().emgpu_last_error().decode()


def _params(n=1, cap=48, cap2=0):
    o = K.DEFAULT
    return native.terminal_filter_params(n, cap, o["dl"], o["cum"], o["pitch"], cap2=cap2)


def test_filter_entry_refuses_bad_arguments_before_any_device_work():
    assert _filter(None) == (L.ERR_ARG, "null argument: p")
    for name in ("geo", "tracks", "rows", "accepted"):
        assert _filter(_params(), **{name: 0}) == (L.ERR_ARG, "null argument: " + name)
    assert _filter(_params(n=-1)) == (L.ERR_ARG, "n outside 0..2^29-1")
    assert _filter(_params(n=1 << 29)) == (L.ERR_ARG, "n outside 0..2^29-1")
    # the status emgpu_track_terminal_host has for tmax_s > 122: CheckCumTurn's 248 heading differences per lane
    for cap in (1, 126, 0, -5, 1 << 20):
        assert _filter(_params(cap=cap)) == (L.ERR_UNSUPPORTED, "cap outside 2..125")
    assert _filter(_params(cap2=0), traj=64) == (L.ERR_ARG, "traj with cap2 < 1")
    assert _filter(_params(), geo=68)[0] == L.ERR_ARG and _filter(_params(), meta=68)[0] == L.ERR_ARG and _filter(_params(), rows=66)[0] == L.ERR_ARG
    # n == 0 is fine and launches nothing, at either end of the caps the entry accepts
    for cap in (2, 125):
        assert _filter(_params(n=0, cap=cap))[0] == L.OK
    with pytest.raises(L.EmgpuError) as ei:
        native.filter_terminal_device(_params(cap=126), 64, 64, 64, 64, stream=0)
    assert ei.value.code == L.ERR_UNSUPPORTED


def test_smooth_entry_refuses_bad_arguments_before_any_device_work():
    def smooth(n2=1, cap=48, tracks=64, rows=64):
        rc = L.lib().emgpu_smooth_terminal_device(None, n2, cap, C.c_void_p(tracks or None), C.c_void_p(rows or None))
        return rc, L.lib().emgpu_last_error().decode()
    assert smooth(tracks=0) == (L.ERR_ARG, "null argument: tracks") and smooth(rows=0) == (L.ERR_ARG, "null argument: rows")
    assert smooth(n2=-1) == (L.ERR_ARG, "n2 outside 0..2^30-1") and smooth(cap=1) == (L.ERR_ARG, "cap < 2")
    assert smooth(cap=129) == (L.ERR_UNSUPPORTED, "cap above 128")          # 272 block rows: more than the kernel's tile of 256
    assert smooth(tracks=66)[0] == L.ERR_ARG
    for cap in (2, 125, 128):
        assert smooth(n2=0, cap=cap)[0] == L.OK
    with pytest.raises(L.EmgpuError) as ei:
        native.smooth_terminal_device(1, 129, 64, 64, stream=0)
    assert ei.value.code == L.ERR_UNSUPPORTED


def test_the_header_declares_the_two_entry_points_in_the_paired_tracks_form():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "emgpu.h")).read()
    for name, second in (("emgpu_filter_terminal_device", "const emgpu_tfilter_params *p"), ("emgpu_smooth_terminal_device", "int64_t n2")):
        params = [q.strip() for q in re.search(r"int %s\(([^)]*)\);" % name, hdr).group(1).split(",")]
        assert params[0] == "void *hip_stream" and " ".join(params[1].split()) == second
        assert not any("emgpu_ctx" in q or "emgpu_model" in q for q in params)
    assert C.sizeof(L.TFilterParams) == 8 + 4 + 4 + 8 * (10 + 2 + 2 + 4)
