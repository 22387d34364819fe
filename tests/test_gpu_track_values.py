"""-m gpu: k_track_values against the numpy restatement of its definition (track_values_ref.values) on the very same xyz.

The comparison rule.  Altitude, speed, vertical rate and acceleration are sums, products, quotients and square roots of doubles, the same
IEEE operations on both sides: they are BIT-EQUAL as f64 and equal to float32(ref) as f32.  The turn rate passes through atan2: both sides
feed it bit-equal dx, dy; the device library documents 2 ulp, the host's is below 1 ulp, of a value <= pi (ulp 4.4e-16), times 57.3 is
7.6e-14 deg per heading, two headings, then one multiply and two subtractions of values <= 360 (half an ulp of 360 = 2.8e-14 each, and
the floor term is exact): about 3.5e-13 deg.  The bound is 2^-40 = 9.1e-13 deg (a factor 2.6), divided by |ur_heading|; as f32 that or one
f32 step of float32(ref), whichever is larger.  Every test prints the largest turn-rate difference it saw.

Outputs go into device buffers pre-filled with a pattern and followed by guard words that must stay; rows and slots not named keep the
pattern."""
import numpy as np
import pytest

import discretize_ref as DR
import track_values_ref as R
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native
from em_model_manned_bayes_amd import encounter_model as E

pytestmark = pytest.mark.gpu

UR = ((1852.0 / 0.3048) / 3600.0, 1.0 / 60.0, 1.0)
TURN_TOL = 2.0 ** -40
FILL, GUARD = -12345.5, 16
N, T_SAMPLE, SEED = 777, 61, 0xD15C
_cache = {}
_seen = {"turn": 0.0}


def _tracks(n, P, seed=1):
    """n random tracks of P points, drawn once per shape and shared (read-only): random headings and speeds, climbs and descents, and in
    every eighth second a standing aircraft (speed exactly 0: the point repeats), in some tracks from the first second on"""
    key = ("tracks", n, P, seed)
    if key not in _cache:
        rs = np.random.RandomState(seed * 1000003 + n * 131 + P)
        hd = rs.uniform(-180.0, 180.0, (n, P - 1))
        hd[:, 1::3] = hd[:, 0::3][:, : hd[:, 1::3].shape[1]] + rs.uniform(-3.0, 3.0, hd[:, 1::3].shape)      # gentle turns as well
        sp = rs.uniform(50.0, 300.0, (n, P - 1))
        sp[rs.uniform(size=sp.shape) < 0.125] = 0.0
        sp[::5, 0] = 0.0
        x = np.concatenate([np.zeros((n, 1)), np.cumsum(sp * np.cos(np.radians(hd)), axis=1)], axis=1)
        y = np.concatenate([np.zeros((n, 1)), np.cumsum(sp * np.sin(np.radians(hd)), axis=1)], axis=1)
        z = 3000.0 + np.cumsum(rs.uniform(-30.0, 30.0, (n, P)), axis=1)
        xyz = np.ascontiguousarray(np.stack([x, y, z], axis=2))
        xyz.setflags(write=False)
        _cache[key] = xyz
    return _cache[key]


def _ref(xyz, ur=UR):
    key = ("ref", id(xyz), ur)
    if key not in _cache:
        _cache[key] = (xyz,) + R.values(xyz, *ur)          # (the array is kept: its id stays its own)
    return _cache[key][1:]


def _expected(xyz, ni, nd, rows, slots, ld, col, init, dyn, ur=UR):
    """what the buffers must hold, as doubles: ((init_val [ni, width], its turn-rate cells), (dyn_val [G4, nd, width, 4], its turn-rate cells))"""
    n, P, _ = xyz.shape
    T, width = P - 2, ld or n
    G4 = (T + 3) // 4
    want_i, want_d = _ref(xyz, ur)
    iv, dv = np.full((ni, width), FILL), np.full((G4, nd, width, 4), FILL)
    ti, td = np.zeros(iv.shape, bool), np.zeros(dv.shape, bool)
    if init:
        for a, r in enumerate(rows):
            if r >= 0:
                iv[r, col:col + n] = want_i[:, a]
                ti[r, col:col + n] = a == R.TURNRATE
    if dyn:
        packed = native.pack_dyn_val(want_d)               # [G4, 3, n, 4], the padding 0
        for k, s in enumerate(slots):
            dv[:, s, col:col + n, :] = packed[:, k]
            td[:, s, col:col + n, :] = k == 2
    return (iv, ti), (dv, td)


def _same(got, want, dt):
    """bit-equal to want rounded once to dt; a NaN equals a NaN of any sign and payload"""
    w = want.astype(dt)
    u = np.uint64 if dt == np.float64 else np.uint32
    return (got.view(u) == w.view(u)) | (np.isnan(got) & np.isnan(w))


def _assert_rule(got, want, turn, dt, ur=UR, what=""):
    ok = _same(got, want, dt)
    assert ok[~turn].all(), (what, np.argwhere(~ok & ~turn)[:5])
    if turn.any():
        g, w = got[turn].astype(np.float64), want[turn].astype(dt).astype(np.float64)
        tol = np.full(g.shape, TURN_TOL / abs(ur[2]))
        if dt == np.float32:
            tol = np.maximum(tol, np.spacing(np.abs(want[turn].astype(np.float32))).astype(np.float64))
        diff = np.abs(g - w)
        both_nan = np.isnan(g) & np.isnan(w)
        if dt == np.float64 and (~both_nan).any():
            _seen["turn"] = max(_seen["turn"], float(diff[~both_nan].max()) * abs(ur[2]))
        assert (both_nan | (diff <= tol)).all(), (what, float(np.nanmax(diff)), float(tol.min()))


def _device(ctx, xyz, layout, dt, ni=5, nd=3, rows=(0, 1, 2, 3, 4), slots=(0, 1, 2), ld=0, col=0, init=True, dyn=True, ur=UR):
    """emgpu_track_values_device over a device copy of xyz (given as rows; transposed here for PLANAR).  Both outputs are filled with FILL
    and followed by GUARD elements of it, which must stay.  Returns (init_val [ni, width], dyn_val [G4, nd, width, 4], kernel)."""
    import torch
    dev = torch.device("cuda", 0)
    n, P, _ = xyz.shape
    T, width = P - 2, ld or n
    G4 = (T + 3) // 4
    src = xyz if layout == L.TRACKS_ROWS else xyz.transpose(1, 2, 0)
    d_xyz = torch.from_numpy(np.array(src, order="C")).to(dev)
    h_iv, h_dv = np.full(ni * width + GUARD, FILL, dtype=dt), np.full(G4 * nd * width * 4 + GUARD, FILL, dtype=dt)
    d_iv, d_dv = torch.from_numpy(h_iv).to(dev), torch.from_numpy(h_dv).to(dev)
    torch.cuda.synchronize()
    vt = L.VALUE_F64 if dt == np.float64 else L.VALUE_F32
    p = native.track_values_params(n, P, *ur, n_initial=ni, nd=nd, rows=rows, slots=slots, value_type=vt, layout=layout, ld=ld, col_offset=col)
    native.track_values_device(ctx, p, d_xyz.data_ptr(), d_iv.data_ptr() if init else 0, d_dv.data_ptr() if dyn else 0)
    kernel = ctx.last_kernel()
    assert ctx.last_launches() == 1
    ctx.sync()
    torch.cuda.synchronize()
    iv, dv = d_iv.cpu().numpy(), d_dv.cpu().numpy()
    assert np.all(iv[ni * width:] == FILL) and np.all(dv[G4 * nd * width * 4:] == FILL)
    return iv[:ni * width].reshape(ni, width).copy(), dv[:G4 * nd * width * 4].reshape(G4, nd, width, 4).copy(), kernel


def _check(ctx, xyz, ur=UR, **kw):
    """both layouts and both value types against the rule; PLANAR and ROWS bit-equal to each other.  Returns the f64 ROWS outputs."""
    n, P, _ = xyz.shape
    geo = dict(ni=5, nd=3, rows=(0, 1, 2, 3, 4), slots=(0, 1, 2), ld=0, col=0, init=True, dyn=True)
    geo.update(kw)
    (wi, ti), (wd, td) = _expected(xyz, ur=ur, **geo)
    out = None
    for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
        res = {}
        for layout, name in ((L.TRACKS_PLANAR, "PLANAR"), (L.TRACKS_ROWS, "ROWS")):
            iv, dv, kernel = _device(ctx, xyz, layout, dt, ur=ur, **geo)
            assert kernel == "k_track_values[%s,%s]" % (name, tag)
            _assert_rule(iv, wi, ti, dt, ur, (n, P, name, tag, "init"))
            _assert_rule(dv, wd, td, dt, ur, (n, P, name, tag, "dyn"))
            res[name] = (iv, dv)
        u = np.uint64 if dt == np.float64 else np.uint32
        for a, b in zip(res["PLANAR"], res["ROWS"]):
            assert np.array_equal(a.view(u), b.view(u)), (n, P, tag)
        out = res["ROWS"]
    return out


# ---- 1. shapes
@pytest.mark.parametrize("P", [3, 4, 5, 6, 7, 10, 62])
def test_points_and_batch_sizes(gpu_ctx, P):
    """T = P - 2 covers T = 1 and every residue of the group of four; P = 10 and 62 are no multiples of the LDS tile's 8 points, and of the
    batch sizes only 256 is a multiple of its 256 tracks"""
    for n in (1, 63, 64, 65, 256, 257, 777):
        iv, dv = _check(gpu_ctx, _tracks(n, P))
        T = P - 2
        if T % 4:
            assert not dv[-1, :, :, T % 4:].any()            # the last group's padding is 0
    print("largest turn-rate difference so far: %.3g deg (bound %.3g)" % (_seen["turn"], TURN_TOL))


# ---- 2. surroundings
def test_rows_and_slots_not_named_keep_the_pattern(gpu_ctx):
    xyz = _tracks(257, 7)
    geo = dict(ni=7, nd=4, rows=(2, 3, 5, 4, 6), slots=(3, 0, 2))
    iv, dv = _check(gpu_ctx, xyz, **geo)
    assert np.all(iv[[0, 1]] == FILL) and np.all(dv[:, 1] == FILL)
    # one row_* at -1, each in turn
    for a in range(5):
        rows = list(geo["rows"])
        rows[a] = -1
        iv, _ = _check(gpu_ctx, xyz, ni=7, nd=4, rows=tuple(rows), slots=geo["slots"])
        assert np.all(iv[geo["rows"][a]] == FILL)
    # either half absent: the other buffer keeps the pattern altogether
    iv, dv = _check(gpu_ctx, xyz, init=False, **geo)
    assert np.all(iv == FILL) and not np.all(dv == FILL)
    iv, dv = _check(gpu_ctx, xyz, dyn=False, **geo)
    assert np.all(dv == FILL) and not np.all(iv == FILL)


@pytest.mark.parametrize("P", [3, 7, 62])
def test_a_window_between_poisoned_neighbours(gpu_ctx, P):
    iv, dv = _check(gpu_ctx, _tracks(777, P), ld=1024, col=100)
    assert np.all(iv[:, :100] == FILL) and np.all(iv[:, 877:] == FILL) and np.all(dv[:, :, :100] == FILL) and np.all(dv[:, :, 877:] == FILL)
    _check(gpu_ctx, _tracks(65, P), ld=1024, col=959, ni=7, nd=4, rows=(6, 5, 4, 3, 2), slots=(2, 3, 1))


def test_other_unit_ratios(gpu_ctx):
    for ur in ((1.0, 1.0, 1.0), (0.5, -2.0, 3.0), (1e-3, 1e3, 0.25)):
        _check(gpu_ctx, _tracks(130, 10), ur=ur)


# ---- 3. hand-built geometry
def test_hand_written_tracks(gpu_ctx):
    tracks = R.hand_tracks()
    for P in (3, 6):
        names = [k for k, v in tracks.items() if len(v) == P]
        xyz = np.ascontiguousarray(np.stack([tracks[k] for k in names]))
        iv, dv = _check(gpu_ctx, xyz, ur=(1.0, 1.0, 1.0))
        turn = native.unpack_dyn_val(dv, P - 2)[:, :, 2]
        for i, k in enumerate(names):
            print(k, turn[i].tolist())
        if P == 3:
            assert turn[names.index("reversal"), 0] == -180.0
            assert turn[names.index("dx -0.0 standing"), 0] == 0.0 and turn[names.index("dx -0.0 climbing north"), 0] == 0.0
            assert turn[names.index("stands first"), 0] == 90.0 and iv[1, names.index("stands first")] == 0.0
        else:
            assert turn[names.index("stands in the middle")].tolist() == [0.0, 90.0, 0.0, 0.0]
            assert not turn[names.index("never moves")].any()
            assert np.all(np.abs(turn[names.index("across 180")] - [2, -2, 2, -2]) < 1e-9)
            assert np.all(np.abs(turn[names.index("more than a circle")] - 100) < 1e-9)


def test_axes_and_diagonals_at_speeds_from_a_thousandth_to_a_thousand(gpu_ctx):
    """three seconds along one of the eight directions, then three along another that is not its opposite: turns of 45, 90 and 135 degrees
    either way (a difference of headings of up to 315 is wrapped), at 1e-3 .. 1e3 ft/s"""
    dirs = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
    rows, want = [], []
    for v in (1e-3, 1e-2, 0.1, 1.0, 7.0, 10.0, 100.0, 1e3):
        for a in range(8):
            for b in range(8):
                if (b - a) % 8 == 4:
                    continue
                steps = np.array([dirs[a]] * 3 + [dirs[b]] * 3, dtype=np.float64) * v
                xy = np.concatenate([np.zeros((1, 2)), np.cumsum(steps, axis=0)])
                rows.append(np.concatenate([xy, np.linspace(500.0, 560.0, 7)[:, None]], axis=1))
                turn = ((b - a) * 45 + 180) % 360 - 180
                want.append([0, 0, turn, 0, 0])
    xyz = np.ascontiguousarray(np.stack(rows))
    iv, dv = _check(gpu_ctx, xyz)
    turn = native.unpack_dyn_val(dv, 5)[:, :, 2]
    assert np.all(np.abs(turn - np.array(want)) < 1e-9)
    assert np.all(native.unpack_dyn_val(dv, 5)[:, :, 0] == 10.0 / UR[1])


def test_a_bad_point_touches_what_the_definition_names(gpu_ctx):
    rs = np.random.RandomState(7)
    P = 9
    clean = R._polyline(rs.uniform(-170, 170, P - 1), rs.uniform(50, 200, P - 1), np.cumsum(rs.uniform(-20, 20, P)))
    plants = [(k, c, bad) for k in (0, 4, P - 1) for c in (0, 1, 2) for bad in (np.nan, np.inf, -np.inf)]
    xyz = np.repeat(clean[None], 1 + len(plants), axis=0)
    for i, (k, c, bad) in enumerate(plants):
        xyz[1 + i, k, c] = bad
    for dt in (np.float32, np.float64):
        u = np.uint64 if dt == np.float64 else np.uint32
        for layout in (L.TRACKS_PLANAR, L.TRACKS_ROWS):
            iv, dv, _ = _device(gpu_ctx, xyz, layout, dt)
            init, dyn = iv.T, native.unpack_dyn_val(dv, P - 2)          # [n, 5], [n, T, 3]
            (wi, _), (wd, _) = _expected(xyz, 5, 3, (0, 1, 2, 3, 4), (0, 1, 2), 0, 0, True, True)
            want_i, want_d = wi.T, native.unpack_dyn_val(wd, P - 2)
            assert np.isfinite(init[0]).all() and np.isfinite(dyn[0]).all()
            for i, (k, c, bad) in enumerate(plants):
                ti, td = R.touched(P, k, c)
                rest = [a for a in range(5) if a not in ti]
                # every other value is the clean track's, bit for bit
                assert np.array_equal(dyn[1 + i][~td].view(u), dyn[0][~td].view(u)) and np.array_equal(init[1 + i, rest].view(u), init[0, rest].view(u)), (k, c, bad)
                # the touched values but the turn rates follow the exact half of the rule; the turn rates: NaN from a NaN, finite from an inf
                t2 = td.copy()
                t2[:, 2] = False
                assert _same(dyn[1 + i][t2], want_d[1 + i][t2], dt).all() and not np.isfinite(dyn[1 + i][t2]).any(), (k, c, bad)
                ti2 = [a for a in ti if a != R.TURNRATE]
                assert _same(init[1 + i, ti2], want_i[1 + i, ti2], dt).all() and not np.isfinite(init[1 + i, ti2]).any(), (k, c, bad)
                turns = dyn[1 + i][:, 2][td[:, 2]]
                assert np.isnan(turns).all() if np.isnan(bad) else np.isfinite(turns).all(), (k, c, bad)


# ---- 4. the host entry point
def test_the_host_entry_point_and_its_chunks(gpu_ctx, monkeypatch):
    n, P = 20011, 62
    xyz = _tracks(n, P)
    geo = dict(n_initial=7, nd=4, rows=(2, 3, 5, 4, 6), slots=(1, 0, 3))
    want = _expected(xyz, 7, 4, geo["rows"], geo["slots"], 0, 0, True, True)
    for vt, dt in ((L.VALUE_F32, np.float32), (L.VALUE_F64, np.float64)):
        monkeypatch.delenv("EMGPU_HOST_CHUNK_MB", raising=False)
        one = native.track_values_host(gpu_ctx, xyz, *UR, value_type=vt, raw=True, static={1: 2.0, 2: np.arange(n) % 4 + 1}, **geo)
        assert gpu_ctx.last_launches() == 1 and one["kernel"] == "k_track_values[ROWS,%s]" % ("f64" if vt else "f32") and one["T"] == 60
        monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", "1")
        many = native.track_values_host(gpu_ctx, xyz, *UR, value_type=vt, raw=True, static={1: 2.0, 2: np.arange(n) % 4 + 1}, **geo)
        assert gpu_ctx.last_launches() >= 8
        u = np.uint64 if dt == np.float64 else np.uint32
        for k in ("init_val", "dyn_val"):
            assert one[k].dtype == dt and np.array_equal(one[k].view(u), many[k].view(u))
        # the rows the kernel leaves: static's values, else the zeros the arrays started with
        iv, dv = one["init_val"].copy(), one["dyn_val"].copy()
        assert np.all(iv[0] == 2.0) and np.array_equal(iv[1], (np.arange(n) % 4 + 1).astype(dt)) and not dv[:, 2].any()
        iv[[0, 1]] = FILL
        dv[:, 2] = FILL
        _assert_rule(iv, want[0][0], want[0][1], dt, UR, "host init")
        _assert_rule(dv, want[1][0], want[1][1], dt, UR, "host dyn")
    monkeypatch.delenv("EMGPU_HOST_CHUNK_MB", raising=False)
    # user-facing shapes, either half alone
    got = native.track_values_host(gpu_ctx, xyz[:65], *UR, value_type=L.VALUE_F64)
    assert got["init_val"].shape == (65, 5) and got["dyn_val"].shape == (65, 60, 3)
    wi, wd = R.values(xyz[:65], *UR)
    assert np.array_equal(got["init_val"][:, :4], wi[:, :4]) and np.array_equal(got["dyn_val"][:, :, :2], wd[:, :, :2])
    assert np.all(np.abs(got["dyn_val"][:, :, 2] - wd[:, :, 2]) <= TURN_TOL)
    assert native.track_values_host(gpu_ctx, xyz[:65], *UR, want_dyn=False)["dyn_val"] is None
    assert native.track_values_host(gpu_ctx, xyz[:65], *UR, want_init=False)["init_val"] is None
    print("largest turn-rate difference so far: %.3g deg (bound %.3g)" % (_seen["turn"], TURN_TOL))


# ---- 5. round trip on the device
def _model(name, model_dir):
    key = ("model", name)
    if key not in _cache:
        path = em_io.materialize_model(name, model_dir)
        parms = em_io.em_read(path)
        labs = parms["labels_initial"]
        ids = [labs.index('"%s"' % s) for s in ("L", "v", "\\dot h", "\\dot v", "\\dot \\psi")]
        tm = [int(r[0]) - 1 for r in np.asarray(parms["temporal_map"]).reshape(-1, 2)]
        _cache[key] = (path, parms["native"], parms, DR.info(parms), ids, [tm.index(v) for v in ids[2:]])
    return _cache[key]


@pytest.mark.parametrize("name", ["uncor_1200code_v2p1", "uncor_1200only_fwse_v1p2"])
def test_round_trip_of_the_sampled_bins_on_the_device(gpu_ctx, model_dir, name):
    """sampler -> k_sample2track<dense> -> k_track_values<PLANAR> -> k_discretize_dbn, all on the device block: the bins of L, v and the
    three rates and the dynamic bins of seconds 0 .. T-2 are the sampler's own, on the tracks sample2track accepts.  Conditions, not
    measurements: at least 90 % of the tracks accepted, at most 1e-4 of the cells off (the CPU oracle's own pipeline: 0)."""
    import torch
    dev = torch.device("cuda", 0)
    path, nm, parms, g, ids, slots = _model(name, model_dir)
    n, T, ni, nd = N, T_SAMPLE, nm.n_initial, nm.n_dyn
    s = native.sample_dbn_host(gpu_ctx, nm, n, T, SEED, raw=True, pinned=False)
    ib, db = s["init_bin"], native.unpack_dyn_bin(s["dyn_bin"], T)
    d_iv, d_dv = torch.from_numpy(s["init_val"].copy()).to(dev), torch.from_numpy(s["dyn_val"].copy()).to(dev)
    d_xyz = torch.zeros((T + 1, 3, n), dtype=torch.float64, device=dev)
    d_fl = torch.zeros(n, dtype=torch.uint8, device=dev)
    b_v = np.asarray(parms["boundaries"][ids[1]], dtype=np.float64)
    torch.cuda.synchronize()
    tp = native.track_params(n, T, *UR, float(b_v[0]), float(b_v[-1]), nd=nd, slot_vertrate=slots[0], slot_acc=slots[1], slot_turnrate=slots[2])
    native.sample2track_device(gpu_ctx, tp, d_iv[ids[0]].data_ptr(), d_iv[ids[1]].data_ptr(), d_dv.data_ptr(), d_xyz.data_ptr(), d_fl.data_ptr())
    gpu_ctx.sync()
    keep = d_fl.cpu().numpy() == 0
    print("%s: accepted %.2f %%" % (name, 100 * keep.mean()))
    assert keep.mean() >= 0.90
    T2 = T - 1
    G2 = (T2 + 3) // 4
    for vt, tdt, dt in ((L.VALUE_F32, torch.float32, np.float32), (L.VALUE_F64, torch.float64, np.float64)):
        d_iv2 = d_iv.to(tdt).clone()                              # G and A stay; the five rows are overwritten
        d_dv2 = torch.zeros((G2, nd, n, 4), dtype=tdt, device=dev)
        d_ib2 = torch.zeros((ni, n), dtype=torch.uint8, device=dev)
        d_db2 = torch.zeros((G2, nd, n), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        p = native.track_values_params(n, T + 1, *UR, n_initial=ni, nd=nd, rows=ids, slots=slots, value_type=vt, layout=L.TRACKS_PLANAR)
        native.track_values_device(gpu_ctx, p, d_xyz.data_ptr(), d_iv2.data_ptr(), d_dv2.data_ptr())
        assert gpu_ctx.last_kernel() == "k_track_values[PLANAR,%s]" % ("f64" if vt else "f32")
        native.discretize_dbn_device(gpu_ctx, nm, native.discretize_params(n, T2, 0, vt), d_iv2.data_ptr(), d_dv2.data_ptr(), d_ib2.data_ptr(),
                                     d_db2.data_ptr())
        gpu_ctx.sync()
        torch.cuda.synchronize()
        ib2, db2 = d_ib2.cpu().numpy(), native.unpack_dyn_bin(d_db2.cpu().numpy().view(np.uint32), T2)
        iv2, dv2 = d_iv2.cpu().numpy(), native.unpack_dyn_val(d_dv2.cpu().numpy(), T2)
        off_i = (ib2[ids] != ib[ids]) & keep[None, :]
        off_d = (db2[:, :, slots] != db[:, :T2, slots]) & keep[:, None, None]
        cells = int(keep.sum()) * (len(ids) + T2 * len(slots))
        for a, i in zip(*np.nonzero(off_i)):
            b = g["bnd"][ids[a]]
            print("init track %d variable %d: value %.17g, bin %d, sampled %d, nearest cut %.17g" % (i, ids[a] + 1, iv2[ids[a], i], ib2[ids[a], i], ib[ids[a], i], b[np.argmin(np.abs(b - iv2[ids[a], i]))]))
        for i, t, k in zip(*np.nonzero(off_d)):
            b = g["bnd"][g["dvar"][slots[k]]]
            print("dyn track %d second %d slot %d: value %.17g, bin %d, sampled %d, nearest cut %.17g" % (i, t, slots[k], dv2[i, t, slots[k]], db2[i, t, slots[k]], db[i, t, slots[k]], b[np.argmin(np.abs(b - dv2[i, t, slots[k]]))]))
        off = int(off_i.sum() + off_d.sum())
        print("%s %s: %d cells, %d off" % (name, dt.__name__, cells, off))
        assert off <= 1e-4 * cells


# ---- 6. composition
def test_track_count_host_equals_values_then_discretize_count(gpu_ctx, model_dir):
    path, nm, parms, g, ids, slots = _model("uncor_1200code_v2p1", model_dir)
    ni, nd = nm.n_initial, nm.n_dyn
    s = native.sample_dbn_host(gpu_ctx, nm, N, T_SAMPLE, SEED, pinned=False)
    iv, dv = s["init_val"].astype(np.float64), s["dyn_val"].astype(np.float64)
    b_v = np.asarray(parms["boundaries"][ids[1]], dtype=np.float64)
    xyz, flags, _ = native.sample2track_host(gpu_ctx, iv[:, ids[0]], iv[:, ids[1]], dv[:, :, slots], *UR, float(b_v[0]), float(b_v[-1]))
    keep = flags == 0
    xyz = np.ascontiguousarray(xyz[keep])
    n = xyz.shape[0]
    assert n >= 0.9 * N
    static = {v + 1: iv[keep, v] for v in range(ni) if v not in ids}
    assert sorted(static) == [1, 2]
    rows1 = tuple(i + 1 for i in ids)
    for vt in (L.VALUE_F32, L.VALUE_F64):
        got = native.track_count_host(gpu_ctx, nm, xyz, rows1, static, n_fine=4, value_type=vt)
        vals = native.track_values_host(gpu_ctx, xyz, *UR, n_initial=ni, nd=nd, rows=ids, slots=slots, value_type=vt, static=static)
        assert vals["init_val"].shape == (n, ni) and vals["dyn_val"].shape == (n, T_SAMPLE - 1, nd)
        want = native.discretize_count_host(gpu_ctx, nm, vals["init_val"], vals["dyn_val"], n_fine=4)
        assert got["values_kernel"] == vals["kernel"] and got["kernel"] == want["kernel"] and got["count_kernel"] == want["count_kernel"]
        assert np.array_equal(got["raw"][0], want["raw"][0]) and np.array_equal(got["raw"][1], want["raw"][1])
        assert np.array_equal(got["raw_pairs"][0], want["raw_pairs"][0]) and np.array_equal(got["raw_pairs"][1], want["raw_pairs"][1])
        assert int(got["raw"][1].sum()) == n * (T_SAMPLE - 2) * nd
    # the class layer: the rows by label, the result in setParameters' order; it sets finite resample rates for the three rates
    m = E.UncorEncounterModel(parameters_filename=path)
    Ni, Nt, rep, chg = m.count_tracks(xyz, static, ctx=gpu_ctx)
    assert rep.shape == chg.shape == (ni, 1) and np.array_equal(rep[:, 0], got["repeat"]) and np.array_equal(chg[:, 0], got["change"])
    assert sum(float(a.sum()) for a in Ni) == n * ni
    with np.errstate(invalid="ignore"):
        m.setParameters(Ni, Nt, rep, chg)
    rates = np.asarray(m.resample_rates).reshape(-1)
    for v in ids[2:]:
        assert np.isfinite(rates[v]) and 0 < rates[v] < 1 and rates[v] == chg[v, 0] / (rep[v, 0] + chg[v, 0])
