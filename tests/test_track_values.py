"""Values of a trace from 1 Hz tracks, the parts that need no GPU: the numpy restatement track_values_ref on the CPU oracle's own sample and
track (it gives the sampled bins back), on hand-written tracks against a plain-Python loop over the definition, the argument checks of
emgpu_track_values_* (made before any device work: there is no context on this box to do any), and the Python surface."""
import ctypes as C
import math

import numpy as np
import pytest

import discretize_ref as DR
import oracle as O
import track_values_ref as R
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native
from em_model_manned_bayes_amd import encounter_model as E

UR = ((1852.0 / 0.3048) / 3600.0, 1.0 / 60.0, 1.0)
TURN_TOL = 2.0 ** -40          # degrees: two atan2 of the same arguments from different libraries (test_gpu_track_values.py derives it)


def model_rows(parms):
    """(the 0-based variable ids of L, v, \\dot h, \\dot v, \\dot \\psi; the temporal-map rows of \\dot h, \\dot v, \\dot \\psi)"""
    labs = parms["labels_initial"]
    ids = [labs.index('"%s"' % s) for s in ("L", "v", "\\dot h", "\\dot v", "\\dot \\psi")]
    tm = [int(r[0]) - 1 for r in np.asarray(parms["temporal_map"]).reshape(-1, 2)]
    return ids, [tm.index(v) for v in ids[2:]]


def oracle_round_trip(name, model_dir, n=777, T=61, seed=0xD15C):
    """oracle sample (values as f32) -> oracle sample2track -> restatement; returns (g, ids, slots, flags, original init / dyn values,
    recovered init / dyn values of T - 1 seconds)"""
    path = em_io.materialize_model(name, model_dir)
    parms, pp = em_io.em_read(path), O.parse_model_txt(path)
    ids, slots = model_rows(parms)
    ref = O.uncor_sample(O.OracleModel(pp), n, T, seed, want_events=False)
    iv = ref["init_val"].astype(np.float32).astype(np.float64)
    dv = ref["dense_val"].astype(np.float32).astype(np.float64)
    b_v = np.asarray(parms["boundaries"][ids[1]], dtype=np.float64)
    xyz, flags, _ = O.sample2track(iv[:, ids[0]], iv[:, ids[1]], dv[:, :, slots], *UR, float(b_v[0]), float(b_v[-1]))
    init, dyn = R.values(xyz, *UR)
    iv2, dv2 = iv.copy(), dv[:, :T - 1].copy()
    iv2[:, ids] = init
    dv2[:, :, slots] = dyn
    return DR.info(parms), ids, slots, flags, iv, dv[:, :T - 1], iv2, dv2


def compare_bins(g, ids, slots, keep, want, got, what=""):
    """(cells compared, cells off) of the rows the tracks give, over the tracks `keep`; every cell that is off is printed"""
    (wi, wd), (gi, gd) = want, got
    wi, gi, wd, gd = wi[keep][:, ids], gi[keep][:, ids], wd[keep][:, :, slots], gd[keep][:, :, slots]
    off = int((wi != gi).sum() + (wd != gd).sum())
    for i, c in zip(*np.nonzero(wi != gi)):
        print("%s init track %d variable %d: bin %d, sampled %d" % (what, i, ids[c], gi[i, c], wi[i, c]))
    for i, t, c in zip(*np.nonzero(wd != gd)):
        print("%s dyn track %d second %d slot %d: bin %d, sampled %d" % (what, i, t, slots[c], gd[i, t, c], wd[i, t, c]))
    return wi.size + wd.size, off


def test_the_oracles_own_tracks_give_the_sampled_bins_back(model_dir):
    g, ids, slots, flags, iv, dv, iv2, dv2 = oracle_round_trip("uncor_1200code_v2p1", model_dir)
    keep = flags == 0
    assert keep.mean() >= 0.90
    want = DR.discretize(g, iv[keep], dv[keep], 4)
    got = DR.discretize(g, iv2[keep], dv2[keep], 4)
    all_rows = np.ones(int(keep.sum()), dtype=bool)
    cells, off = compare_bins(g, ids, slots, all_rows, want[:2], got[:2])
    print("accepted %.2f %%, %d cells, %d off" % (100 * keep.mean(), cells, off))
    assert off <= 1e-4 * cells
    assert np.array_equal(want[2], got[2]) and np.array_equal(want[3], got[3])
    assert want[4] == 0 and got[4] == 0


def loop_values(xyz, ur_speed, ur_vertrate, ur_heading):
    """the definition, one track, one second and one value at a time: (init [5], dyn [T][3])"""
    P = len(xyz)
    s, h, dz = [], [], []
    for t in range(P - 1):
        dx, dy = xyz[t + 1][0] - xyz[t][0], xyz[t + 1][1] - xyz[t][1]
        dz.append(xyz[t + 1][2] - xyz[t][2])
        s.append(math.sqrt(dx * dx + dy * dy))
        if s[t] == 0.0:
            h.append(h[t - 1] if t > 0 else 0.0)
        else:
            h.append(math.atan2(dy, dx) * 57.29577951308232)
    dyn = []
    for t in range(P - 2):
        d = h[t + 1] - h[t]
        w = d - 360.0 * math.floor((d + 180.0) / 360.0)
        dyn.append([dz[t] / ur_vertrate, (s[t + 1] - s[t]) / ur_speed, w / ur_heading])
    return [xyz[0][2], s[0] / ur_speed] + dyn[0], dyn


EXPECT_TURN = {"right angle": [90], "across 180": [2, -2, 2, -2], "more than a circle": [100, 100, 100, 100], "reversal": [-180],
               "stands in the middle": [0, 90, 0, 0], "stands first": [90], "never moves": [0, 0, 0, 0], "dx -0.0 climbing north": [0],
               "dx -0.0 standing": [0]}


@pytest.mark.parametrize("ur", [(1.0, 1.0, 1.0), UR, (0.5, -2.0, 3.0)])
def test_hand_written_tracks(ur):
    tracks = R.hand_tracks()
    assert set(tracks) == set(EXPECT_TURN) and {len(v) for v in tracks.values()} == {3, 6}
    for name, xyz in tracks.items():
        init, dyn = R.values(xyz[None], *ur)
        li, ld = loop_values(xyz.tolist(), *ur)
        li, ld = np.array(li), np.array(ld)
        # sums, products, quotients and square roots are the same IEEE operations; only atan2 may come from another library
        assert np.array_equal(init[0, :4], li[:4]) and np.array_equal(dyn[0, :, :2], ld[:, :2]), name
        assert np.all(np.abs(dyn[0, :, 2] - ld[:, 2]) <= TURN_TOL / abs(ur[2])) and abs(init[0, 4] - li[4]) <= TURN_TOL / abs(ur[2]), name
        assert np.all(np.abs(dyn[0, :, 2] * ur[2] - EXPECT_TURN[name]) <= 1e-9), (name, dyn[0, :, 2])
        w = dyn[0, :, 2] * ur[2]
        assert np.all((w >= -180.0 - 1e-12) & (w < 180.0))
    one = lambda name: R.values(tracks[name][None], 1.0, 1.0, 1.0)   # noqa: E731
    assert one("reversal")[1][0, 0, 2] == -180.0                                   # exactly
    assert one("right angle")[0][0].tolist() == [0.0, 1.0, 10.0, 0.0, 90.0] and one("right angle")[1][0, 0].tolist() == [10.0, 0.0, 90.0]
    init, dyn = one("stands in the middle")
    assert dyn[0, :, 1].tolist() == [-1.0, 1.0, 0.0, -1.0] and dyn[0, :, 2].tolist() == [0.0, 90.0, 0.0, 0.0]
    assert one("stands first")[0][0].tolist() == [7.0, 0.0, 0.0, 1.0, 90.0]
    init, dyn = one("never moves")
    assert init[0].tolist() == [100.0, 0.0, -10.0, 0.0, 0.0] and np.all(dyn[0] == [-10.0, 0.0, 0.0])
    assert one("dx -0.0 standing")[1][0, 0].tolist() == [0.0, 1.0, 0.0]            # without the hold the turn would be -180
    assert np.array_equal(one("across 180")[1][0, :, 0], [5.0] * 4)


def test_what_a_bad_point_touches_in_the_restatement():
    rs = np.random.RandomState(7)
    P = 9
    clean = R._polyline(rs.uniform(-170, 170, P - 1), rs.uniform(50, 200, P - 1), np.cumsum(rs.uniform(-20, 20, P)))
    ci, cd = R.values(clean[None], *UR)
    for k in (0, 4, P - 1):
        for coord in (0, 1, 2):
            for bad in (np.nan, np.inf):
                xyz = clean.copy()
                xyz[k, coord] = bad
                bi, bd = R.values(xyz[None], *UR)
                init, dyn = R.touched(P, k, coord)
                rest_i = [c for c in range(5) if c not in init]
                assert np.array_equal(bd[0][~dyn], cd[0][~dyn]) and np.array_equal(bi[0, rest_i], ci[0, rest_i]), (k, coord, bad)
                if np.isnan(bad):
                    assert not np.isfinite(bd[0][dyn]).any() and not np.isfinite(bi[0, init]).any()
                else:                                   # atan2 of an infinite displacement is a multiple of 90 degrees: finite turn rates
                    d2 = dyn.copy()
                    d2[:, 2] = False
                    assert not np.isfinite(bd[0][d2]).any() and np.isfinite(bd[0][:, 2]).all()
                    assert not np.isfinite(bi[0, [c for c in init if c != R.TURNRATE]]).any()


def test_track_values_entry_points_check_their_arguments_before_any_device_work():
    lib = L.lib()
    xyz = np.zeros((64, 7, 3))
    iv, dv = np.full((7, 64), 9, np.float32), np.full((2, 3, 64, 4), 9, np.float32)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    kw = dict(n_initial=7, nd=3, rows=(2, 3, 5, 4, 6), slots=(1, 0, 2))
    for f in (lib.emgpu_track_values_device, lib.emgpu_track_values_host):
        def call(p, a=xyz, b=iv, c=dv):
            return f(None, None if p is None else C.byref(p), P(a), P(b), P(c))

        def bad(what, p=None, **half):
            rc = call(p if p is not None else native.track_values_params(64, 7, *UR, **kw), **half)
            assert rc == L.ERR_ARG and what in lib.emgpu_last_error(), (what, lib.emgpu_last_error())
        par = lambda n=64, points=7, ur=UR, **over: native.track_values_params(n, points, *ur, **{**kw, **over})   # noqa: E731
        assert call(None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
        bad(b"null", a=None)
        bad(b"nothing to write", b=None, c=None)
        for points in (2, 0, -1, 65538):
            bad(b"points", par(points=points))
        bad(b"n < 0", par(n=-1))
        bad(b"col_offset + n exceeds ld", par(ld=100, col_offset=37))
        bad(b"col_offset + n exceeds ld", par(col_offset=1))
        bad(b"value_type", par(value_type=2))
        bad(b"layout", par(layout=2))
        for ur in ((0.0, 1.0, 1.0), (1.0, np.nan, 1.0), (1.0, 1.0, np.inf), (1.0, -0.0, 1.0)):
            bad(b"unit ratio", par(ur=ur))
        bad(b"n_initial", par(n_initial=0))
        bad(b"initial row outside", par(rows=(2, 3, 5, 4, 7)))
        bad(b"initial row outside", par(rows=(-2, 3, 5, 4, 6)))
        bad(b"same initial row", par(rows=(2, 3, 5, 3, 6)))
        bad(b"nd outside", par(nd=2, slots=(0, 1, 1)))
        bad(b"dynamic slot outside", par(slots=(1, 0, 3)))
        bad(b"dynamic slot outside", par(slots=(-1, 0, 2)))
        bad(b"same dynamic slot", par(slots=(1, 1, 2)))
        if f is lib.emgpu_track_values_host:
            bad(b"rows", par(layout=L.TRACKS_PLANAR))
        # nothing left to object to but the missing context
        rows_layout = dict(layout=L.TRACKS_ROWS)
        for p, half in ((par(**rows_layout), {}), (par(points=3, **rows_layout), {}), (par(points=65537, **rows_layout), {}),
                        (par(rows=(-1, -1, -1, -1, -1), **rows_layout), {}), (par(value_type=L.VALUE_F64, **rows_layout), {}),
                        (par(rows=(9, 9, 9, 9, 9), **rows_layout), {"b": None}),      # a half that is not there is not looked at
                        (par(slots=(9, 9, 9), **rows_layout), {"c": None}), (par(n=0, **rows_layout), {})):
            assert call(p, **half) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx", lib.emgpu_last_error()
    assert np.all(iv == 9) and np.all(dv == 9)


def test_the_track_values_surface(model_dir):
    for s in ("emgpu_track_values_device", "emgpu_track_values_host"):
        assert s in L.SYMBOLS and hasattr(L.lib(), s)
    for f in ("track_values_params", "track_values_device", "track_values_host", "track_count_host", "track_rows"):
        assert callable(getattr(native, f))
    assert callable(E.UncorEncounterModel.count_tracks)
    p = native.track_values_params(10, 7, 2.0, 3.0, 4.0, n_initial=7, nd=4, rows=(2, 3, 5, 4, -1), slots=(1, 0, 3), value_type=L.VALUE_F64,
                                   layout=L.TRACKS_PLANAR, ld=16, col_offset=2)
    assert (p.n, p.points, p.value_type, p.ld, p.col_offset, p.n_initial, p.nd, p.layout) == (10, 7, 1, 16, 2, 7, 4, 0)
    assert (p.row_alt, p.row_speed, p.row_vertrate, p.row_acc, p.row_turnrate) == (2, 3, 5, 4, -1)
    assert (p.slot_vertrate, p.slot_acc, p.slot_turnrate, p.ur_speed, p.ur_vertrate, p.ur_heading) == (1, 0, 3, 2.0, 3.0, 4.0)
    assert C.sizeof(L.TrackValuesParams) == 104
    xyz = np.zeros((5, 6, 3))
    with pytest.raises(ValueError):
        native.track_values_host(None, np.zeros((5, 6, 2)), *UR)
    with pytest.raises(ValueError):                 # static may only fill what the tracks leave
        native.track_values_host(None, xyz, *UR, n_initial=7, rows=(2, 3, 5, 4, 6), static={3: 1.0})
    with pytest.raises(ValueError):
        native.track_values_host(None, xyz, *UR, n_initial=7, rows=(2, 3, 5, 4, 6), static={8: 1.0})
    with pytest.raises(L.EmgpuError) as ei:         # shaped and filled by the Python layer, refused by the library for want of a context
        native.track_values_host(None, xyz, *UR, n_initial=7, rows=(2, 3, 5, 4, 6), static={1: 2.0, 2: np.arange(5)})
    assert ei.value.code == L.ERR_ARG and "null ctx" in str(ei.value)
    iv = np.zeros((7, 5), np.float32)
    native._fill_static(iv, {1: 2.0, 2: np.arange(5)}, [2, 3, 4, 5, 6])
    assert iv[0].tolist() == [2.0] * 5 and iv[1].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and not iv[2:].any()
    # the rows of a model, by label and temporal map
    path = em_io.materialize_model("uncor_1200code_v2p1", model_dir)
    m = E.UncorEncounterModel(parameters_filename=path)
    ids, slots = model_rows(em_io.em_read(path))
    idxL, idxV, idxDV, idxDH, idxDPsi = m._track_variables()
    assert native.track_rows(m.native, (idxL, idxV, idxDH, idxDV, idxDPsi)) == (tuple(ids), tuple(slots))
    with pytest.raises(L.EmgpuError) as ei:         # UncorEncounterModel.m:231-234: raised before anything touches a device
        E.UncorEncounterModel(parameters_filename=em_io.materialize_model("balloon_v1", model_dir)).count_tracks(xyz)
    assert ei.value.identifier == "dynvar:empty"
