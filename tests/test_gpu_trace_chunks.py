"""-m gpu: the chunk driver the four trace _host entry points share (csrc/emgpu_tracechunk.hpp), where only the combination can go wrong:
chunks x a window of a wider array, chunks x one half alone, chunks x the bad-value word, chunks x accumulation.  Every many-chunk call
runs under EMGPU_HOST_CHUNK_MB=1, is compared with the same call as one chunk, and must make ceil(n / c) launches for the c of its own
per-lane bytes: n is 2 c + 89 (of its own c, or of a neighbour's where two calls share a trace): at least three chunks, the last one
short and no multiple of 64 lanes.  Traces, helpers and references are those of test_gpu_score / _count / _discretize / _track_values
(score_ref, count_ref, discretize_ref, track_values_ref)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_count as TC
import test_gpu_discretize as TD
import test_gpu_score as TS
import test_gpu_track_values as TV
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import native

pytestmark = pytest.mark.gpu

MODEL, AUTO = "uncor_1200code_v2p1", L.TRANSITION_REFERENCE_AUTO
NI, ND = 7, 3                     # its variables (asserted where a model is loaded)
T, P = 61, 62                     # seconds of the traces, points of the tracks
COL, MARGIN = 333, 91             # the window: an odd first column, no multiple of 256, and columns behind it
_cache = {}


def _g4(t):
    return (t + 3) // 4


def _c(per_lane):
    """lanes per chunk under EMGPU_HOST_CHUNK_MB=1"""
    return max((1 << 20) // per_lane // 256 * 256, 256)


def _n(per_lane):
    return 2 * _c(per_lane) + 89


def _launches(n, per_lane):
    c = min((n + 255) // 256 * 256, _c(per_lane))
    return (n + c - 1) // c


PER_LANE = {
    "score": lambda t, dyn=True: NI + 4 * (_g4(t) * ND if dyn and t > 1 else 0) + 16,
    "count": lambda t, dyn=True: NI + 4 * (_g4(t) * ND if dyn and t > 1 else 0),
    "discretize": lambda t, es=4, init=True, dyn=True: (NI * (es + 1) if init else 0) + (_g4(t) * ND * (4 * es + 4) if dyn else 0),
    "track": lambda es=8, init=True, dyn=True: 24 * P + (5 * es if init else 0) + (3 * _g4(P - 2) * 4 * es if dyn else 0),
}


class Chunks:
    """one call under EMGPU_HOST_CHUNK_MB=1 (so many launches, counted) and once more as a single chunk"""

    def __init__(self, ctx, monkeypatch):
        self.ctx, self.mp = ctx, monkeypatch

    def both(self, call, n, per_lane):
        self.mp.setenv("EMGPU_HOST_CHUNK_MB", "1")
        try:
            many = call()
        finally:
            self.mp.delenv("EMGPU_HOST_CHUNK_MB", raising=False)
        want = _launches(n, per_lane)
        assert want >= 3 and (n % _c(per_lane)) % 64 != 0
        assert self.ctx.last_launches() == want, (self.ctx.last_launches(), want)
        one = call()
        assert self.ctx.last_launches() == 1
        return many, one

    def many(self, call, n, per_lane):
        self.mp.setenv("EMGPU_HOST_CHUNK_MB", "1")
        try:
            return call()
        finally:
            self.mp.delenv("EMGPU_HOST_CHUNK_MB", raising=False)
            assert self.ctx.last_launches() == _launches(n, per_lane) >= 3


@pytest.fixture
def chunks(gpu_ctx, monkeypatch):
    return Chunks(gpu_ctx, monkeypatch)


def _bins(ctx, model_dir, n, t):
    nm, parms, g, ib, db = TC._trace(ctx, MODEL, model_dir, n, t, AUTO)
    assert (nm.n_initial, nm.n_dyn) == (NI, ND)
    return nm, g, ib, db


def _values(ctx, model_dir, n, t):
    nm, g, iv, dv, _, _ = TD._trace(ctx, MODEL, model_dir, n, t)
    assert (nm.n_initial, nm.n_dyn) == (NI, ND)
    return nm, g, iv, dv


def _wide(a, axis, poison):
    """a, its lanes on `axis`, as columns COL .. COL + n of a wider array of `poison`"""
    shape = list(a.shape)
    shape[axis] += COL + MARGIN
    big = np.full(shape, poison, dtype=a.dtype)
    big[(slice(None),) * axis + (slice(COL, COL + a.shape[axis]),)] = a
    return big


def _score_want(nm, g, ib, db, t):
    key = ("score", id(ib), t)
    if key not in _cache:
        _cache[key] = (ib,) + tuple(TS.R.score(TS.R.lib_tables(nm), g, ib.T, None if db is None else native.unpack_dyn_bin(db, t), AUTO))
    return _cache[key][1:]


def _same_bits(a, b):
    return all(TS.R.same_bits(a[k], b[k]) for k in ("log_lik", "initial"))


def _same_raw(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a["raw"], b["raw"]))


# ---- 1. a window x chunks
def test_score_window(gpu_ctx, model_dir, chunks):
    per_lane = PER_LANE["score"](T)
    n = _n(PER_LANE["count"](T))                          # (the counting test's trace: 3 chunks of either c)
    nm, g, ib, db = _bins(gpu_ctx, model_dir, n, T)
    want, want_ini = _score_want(nm, g, ib, db, T)
    big_ib, big_db = _wide(ib, 1, 255), _wide(db, 2, 0xFFFFFFFF)
    many, one = chunks.both(lambda: native.score_dbn_host(gpu_ctx, nm, big_ib, big_db, T, AUTO, raw=True, n=n, col_offset=COL), n, per_lane)
    assert many["log_lik"].shape == (n,) and _same_bits(many, one)
    assert TS.R.same_bits(many["log_lik"], want) and TS.R.same_bits(many["initial"], want_ini) and np.isfinite(want).any()


def test_count_window(gpu_ctx, model_dir, chunks):
    per_lane = PER_LANE["count"](T)
    n = _n(per_lane)
    nm, g, ib, db = _bins(gpu_ctx, model_dir, n, T)
    want_i, want_t, _ = TC._ref((MODEL, n, T, AUTO), g, ib, db, T, AUTO, nm.n_transition)
    big_ib, big_db = _wide(ib, 1, 255), _wide(db, 2, 0xFFFFFFFF)
    pat = lambda a, k: (np.arange(a.size, dtype=np.uint64) * np.uint64(k) + np.uint64(5))      # the tables the call adds to
    call = lambda: native.count_dbn_host(gpu_ctx, nm, big_ib, big_db, T, AUTO, raw=True, n=n, col_offset=COL,
                                         counts=(pat(want_i, 3), pat(want_t, 7)))
    many, one = chunks.both(call, n, per_lane)
    assert _same_raw(many, one)
    assert np.array_equal(many["raw"][0], want_i + pat(want_i, 3)) and np.array_equal(many["raw"][1], want_t + pat(want_t, 7))


def _discretize_into(ctx, nm, iv, dv, t, n_fine, n, ld, col, start):
    """emgpu_discretize_dbn_host itself: bins into arrays of the values' extent pre-filled with 0xEE, vectors into copies of `start`"""
    ib = None if iv is None else np.full(iv.shape, TD.FILL8, dtype=np.uint8)
    db = None if dv is None else np.full(dv.shape[:3], TD.FILL32, dtype=np.uint32)
    rep, chg = start[0].copy(), start[1].copy()
    f64 = (iv if iv is not None else dv).dtype == np.float64
    p = native.discretize_params(n, t, n_fine, L.VALUE_F64 if f64 else L.VALUE_F32, None, ld, col)
    L.check(L.lib().emgpu_discretize_dbn_host(ctx._h, nm._h, C.byref(p), native._p(iv), native._p(dv), native._p(ib), native._p(db),
                                              native._p(rep), native._p(chg)))
    return ib, db, rep, chg


@pytest.mark.parametrize("dt,es", [(np.float32, 4), (np.float64, 8)])
def test_discretize_window(gpu_ctx, model_dir, chunks, dt, es):
    n = _n(PER_LANE["discretize"](T, 4))                  # 2137: 3 chunks as f32, 5 as f64, the last of 89 lanes in both
    per_lane = PER_LANE["discretize"](T, es)
    nm, g, iv, dv = _values(gpu_ctx, model_dir, n, T)
    want_ib, want_db, rep, chg, bad = TD._want(g, iv, dv, n, T, 4)
    assert bad == 0
    big_iv, big_dv = _wide(iv.astype(dt), 1, np.nan), _wide(dv.astype(dt), 2, np.nan)
    start = (np.arange(NI, dtype=np.uint64) + np.uint64(2 ** 32 - 3), np.arange(NI, dtype=np.uint64) * np.uint64(11))
    many, one = chunks.both(lambda: _discretize_into(gpu_ctx, nm, big_iv, big_dv, T, 4, n, big_iv.shape[1], COL, start), n, per_lane)
    assert all(np.array_equal(a, b) for a, b in zip(many, one))
    full_ib, full_db = _wide(want_ib, 1, TD.FILL8), _wide(want_db, 2, TD.FILL32)              # untouched outside the window
    assert np.array_equal(many[0], full_ib) and np.array_equal(many[1], full_db)
    assert np.array_equal(many[2], rep + start[0]) and np.array_equal(many[3], chg + start[1])


def _track_into(ctx, xyz, dt, ld, col, rows=(0, 1, 2, 3, 4), init=True, dyn=True):
    """emgpu_track_values_host itself, into arrays of ld columns pre-filled with FILL"""
    n = xyz.shape[0]
    iv = np.full((5, ld), TV.FILL, dtype=dt) if init else None
    dv = np.full((_g4(P - 2), 3, ld, 4), TV.FILL, dtype=dt) if dyn else None
    p = native.track_values_params(n, P, *TV.UR, rows=rows, value_type=L.VALUE_F64 if dt == np.float64 else L.VALUE_F32, ld=ld, col_offset=col)
    L.check(L.lib().emgpu_track_values_host(ctx._h, C.byref(p), native._p(xyz), native._p(iv), native._p(dv)))
    return iv, dv


def _bits(a, b):
    return (a is None and b is None) or np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("dt,es", [(np.float32, 4), (np.float64, 8)])
def test_track_values_window(gpu_ctx, chunks, dt, es):
    per_lane = PER_LANE["track"](es)
    n = _n(per_lane)                                      # 601 tracks of 62 points
    xyz = TV._tracks(n, P)
    ld = COL + n + MARGIN
    many, one = chunks.both(lambda: _track_into(gpu_ctx, xyz, dt, ld, COL), n, per_lane)
    assert _bits(many[0], one[0]) and _bits(many[1], one[1])
    (wi, ti), (wd, td) = TV._expected(xyz, 5, 3, (0, 1, 2, 3, 4), (0, 1, 2), ld, COL, True, True)   # FILL outside the window
    TV._assert_rule(many[0], wi, ti, dt, TV.UR, "chunked window, init")
    TV._assert_rule(many[1], wd, td, dt, TV.UR, "chunked window, dyn")


# ---- 2. one half alone x chunks
N_BIG, T_BIG = _n(NI), 5          # 299 609 lanes of 5 seconds: three chunks even of the initial bins alone (7 bytes per lane)


@pytest.mark.parametrize("half", ["init", "dyn"])
def test_discretize_one_half(gpu_ctx, model_dir, chunks, half):
    init = half == "init"
    t = T_BIG if init else T
    per_lane = PER_LANE["discretize"](t, 4, init=init, dyn=not init)
    n = _n(per_lane)                                      # init: 59 993 lanes of the large trace; dyn: 2137
    nm, g, iv, dv = _values(gpu_ctx, model_dir, N_BIG if init else n, t)
    full = chunks.many(lambda: native.discretize_dbn_host(gpu_ctx, nm, iv, dv, t, 4, raw=True, n=n), n, PER_LANE["discretize"](t, 4))
    many, one = chunks.both(lambda: native.discretize_dbn_host(gpu_ctx, nm, iv if init else None, None if init else dv, t, 4, raw=True, n=n),
                            n, per_lane)
    key, none = ("init_bin", "dyn_bin") if init else ("dyn_bin", "init_bin")
    assert many[none] is None and one[none] is None
    assert np.array_equal(many[key], one[key]) and np.array_equal(many[key], full[key]) and many[key][..., :n].any()
    assert _same_raw(many, one)
    if init:                                              # the pairs are the dynamic half's
        assert not many["raw"][0].any() and not many["raw"][1].any()
    else:
        assert _same_raw(many, full) and many["raw"][0].any()


@pytest.mark.parametrize("what", ["no init", "no dyn", "a row at -1"])
def test_track_values_one_half(gpu_ctx, chunks, what):
    init, dyn = what != "no init", what != "no dyn"
    rows = (0, 1, -1, 3, 4) if what == "a row at -1" else (0, 1, 2, 3, 4)
    per_lane = PER_LANE["track"](8, init, dyn)
    n = _n(per_lane)                                      # 601, or 1113 where the dynamic half is away
    xyz = TV._tracks(n, P)
    full = _track_into(gpu_ctx, xyz, np.float64, n, 0)
    many, one = chunks.both(lambda: _track_into(gpu_ctx, xyz, np.float64, n, 0, rows, init, dyn), n, per_lane)
    assert _bits(many[0], one[0]) and _bits(many[1], one[1])
    assert (many[0] is None) == (not init) and (many[1] is None) == (not dyn)
    if dyn:
        assert _bits(many[1], full[1])
    if init:
        keep = [r for r in rows if r >= 0]
        assert _bits(many[0][keep], full[0][keep])
        if len(keep) < 5:
            assert np.all(many[0][2] == TV.FILL) and not np.all(full[0][2] == TV.FILL)


def test_count_the_initial_network_alone(gpu_ctx, model_dir, chunks):
    per_lane, n = PER_LANE["count"](T_BIG, dyn=False), N_BIG
    nm, g, ib, db = _bins(gpu_ctx, model_dir, n, T_BIG)
    full = chunks.many(lambda: native.count_dbn_host(gpu_ctx, nm, ib, db, T_BIG, AUTO, raw=True), n, PER_LANE["count"](T_BIG))
    many, one = chunks.both(lambda: native.count_dbn_host(gpu_ctx, nm, ib, None, T_BIG, AUTO, raw=True), n, per_lane)
    assert _same_raw(many, one)
    assert np.array_equal(many["raw"][0], full["raw"][0]) and int(many["raw"][0].sum()) == n * NI
    assert not many["raw"][1].any() and full["raw"][1].any()
    assert np.array_equal(many["raw"][0], TC._ref(None, g, ib, None, 1, AUTO, nm.n_transition)[0])


def test_score_one_second(gpu_ctx, model_dir, chunks):
    per_lane = PER_LANE["score"](1)
    n = _n(per_lane)                                      # 91 225 lanes of the large trace
    nm, g, ib, db = _bins(gpu_ctx, model_dir, N_BIG, T_BIG)
    full = chunks.many(lambda: native.score_dbn_host(gpu_ctx, nm, ib, db, T_BIG, AUTO, raw=True, n=n), n, PER_LANE["score"](T_BIG))
    for dyn_bin in (db[:1], None):                        # T = 1 reads no transition, given or not
        many, one = chunks.both(lambda: native.score_dbn_host(gpu_ctx, nm, ib, dyn_bin, 1, AUTO, raw=True, n=n), n, per_lane)
        assert _same_bits(many, one)
        assert TS.R.same_bits(many["log_lik"], full["initial"]) and TS.R.same_bits(many["initial"], full["initial"])
    assert not TS.R.same_bits(full["log_lik"], full["initial"])


# ---- 3. the report word across chunks
def _pending(ctx):
    """the pending _device report comes with this sync, once"""
    with pytest.raises(L.EmgpuError) as ei:
        ctx.sync()
    assert ei.value.code == L.ERR_ARG and "outside 1..r" in str(ei.value)
    ctx.sync()


def test_score_report_word(gpu_ctx, model_dir, chunks):
    gpu_ctx.sync()
    per_lane = PER_LANE["score"](T)
    n = _n(PER_LANE["count"](T))
    nm, g, ib, db = _bins(gpu_ctx, model_dir, n, T)
    want, want_ini = _score_want(nm, g, ib, db, T)
    _, _, _, sib, sdb = TS._trace(gpu_ctx, MODEL, model_dir, TS.N, 5, AUTO)
    bad_small = sib.copy()
    bad_small[0, 9] = 0
    ll = TS._device(gpu_ctx, nm, bad_small, sdb, TS.N, 5, AUTO, sync=False)[0]                # a report nobody has synchronized on
    assert np.flatnonzero(np.isnan(ll)).tolist() == [9]
    clean = chunks.many(lambda: native.score_dbn_host(gpu_ctx, nm, ib, db, T, AUTO, raw=True), n, per_lane)
    assert TS.R.same_bits(clean["log_lik"], want) and TS.R.same_bits(clean["initial"], want_ini)
    bad_ib = ib.copy()
    bad_ib[3, n - 5] = 0                                  # in the last, short chunk
    with pytest.raises(L.EmgpuError) as ei:
        chunks.many(lambda: native.score_dbn_host(gpu_ctx, nm, bad_ib, db, T, AUTO, raw=True), n, per_lane)
    assert ei.value.code == L.ERR_ARG and "outside 1..r" in str(ei.value)
    keep = np.arange(n) != n - 5
    for got, ref in ((ei.value.log_lik, want), (ei.value.initial, want_ini)):
        assert np.flatnonzero(np.isnan(got)).tolist() == [n - 5] and TS.R.same_bits(got[keep], ref[keep])
    _pending(gpu_ctx)


def test_count_report_word(gpu_ctx, model_dir, chunks):
    gpu_ctx.sync()
    per_lane = PER_LANE["count"](T)
    n = _n(per_lane)
    nm, g, ib, db = _bins(gpu_ctx, model_dir, n, T)
    want_i, want_t, _ = TC._ref((MODEL, n, T, AUTO), g, ib, db, T, AUTO, nm.n_transition)
    _, _, _, sib, sdb = TC._trace(gpu_ctx, MODEL, model_dir, TC.N, 5, AUTO)
    bad_small = sib.copy()
    bad_small[0, 9] = 0
    TC._device(gpu_ctx, nm, bad_small, sdb, TC.N, 5, AUTO, sync=False)
    clean = chunks.many(lambda: native.count_dbn_host(gpu_ctx, nm, ib, db, T, AUTO, raw=True), n, per_lane)
    assert np.array_equal(clean["raw"][0], want_i) and np.array_equal(clean["raw"][1], want_t)
    bad_ib = ib.copy()
    bad_ib[0, n - 5] = 0                                  # a root, in the last, short chunk
    bad_i, bad_t, skipped = TC._ref(None, g, bad_ib, db, T, AUTO, nm.n_transition)
    assert skipped > 0
    with pytest.raises(L.EmgpuError) as ei:
        chunks.many(lambda: native.count_dbn_host(gpu_ctx, nm, bad_ib, db, T, AUTO, raw=True), n, per_lane)
    assert ei.value.code == L.ERR_ARG and "count: a bin outside 1..r" in str(ei.value)
    assert np.array_equal(ei.value.counts["raw"][0], bad_i) and np.array_equal(ei.value.counts["raw"][1], bad_t)
    _pending(gpu_ctx)


def test_discretize_report_word(gpu_ctx, model_dir, chunks):
    gpu_ctx.sync()
    per_lane = PER_LANE["discretize"](T, 4)
    n = _n(per_lane)
    nm, g, iv, dv = _values(gpu_ctx, model_dir, n, T)
    want = TD._want(g, iv, dv, n, T, 4)
    _, _, siv, sdv, _, _ = TD._trace(gpu_ctx, MODEL, model_dir, 130, 12)
    bad_small = siv.copy()
    bad_small[3, 7] = np.nan
    TD._device(gpu_ctx, nm, bad_small, sdv, 130, 6, 4, sync=False)
    clean = chunks.many(lambda: native.discretize_dbn_host(gpu_ctx, nm, iv, dv, T, 4, raw=True), n, per_lane)
    assert np.array_equal(clean["init_bin"], want[0]) and np.array_equal(clean["dyn_bin"], want[1])
    assert np.array_equal(clean["raw"][0], want[2]) and np.array_equal(clean["raw"][1], want[3])
    bad_dv = dv.copy()
    bad_dv[7, 1, n - 5, 2] = np.nan                       # second 30 of a lane of the last, short chunk
    bad = TD._want(g, iv, bad_dv, n, T, 4)
    assert bad[4] == 1
    with pytest.raises(L.EmgpuError) as ei:
        chunks.many(lambda: native.discretize_dbn_host(gpu_ctx, nm, iv, bad_dv, T, 4, raw=True), n, per_lane)
    assert ei.value.code == L.ERR_ARG and "discretize: a NaN" in str(ei.value)
    got = ei.value.bins
    assert np.array_equal(got["init_bin"], bad[0]) and np.array_equal(got["dyn_bin"], bad[1]) and int((got["dyn_bin"] != want[1]).sum()) == 1
    assert np.array_equal(got["raw"][0], bad[2]) and np.array_equal(got["raw"][1], bad[3])
    _pending(gpu_ctx)


# ---- 4. accumulation x chunks
def test_count_accumulates_over_chunked_windows(gpu_ctx, model_dir, chunks):
    per_lane, n = PER_LANE["count"](T_BIG), N_BIG
    h = n // 2 + 3                                        # two windows of five chunks each
    nm, g, ib, db = _bins(gpu_ctx, model_dir, n, T_BIG)
    whole = chunks.many(lambda: native.count_dbn_host(gpu_ctx, nm, ib, db, T_BIG, AUTO, raw=True), n, per_lane)
    first = chunks.many(lambda: native.count_dbn_host(gpu_ctx, nm, ib, db, T_BIG, AUTO, raw=True, n=h, col_offset=0), h, per_lane)
    assert not np.array_equal(first["raw"][1], whole["raw"][1])
    both = chunks.many(lambda: native.count_dbn_host(gpu_ctx, nm, ib, db, T_BIG, AUTO, raw=True, n=n - h, col_offset=h, counts=first["raw"]),
                       n - h, per_lane)
    assert both["raw"][0] is first["raw"][0] and both["raw"][1] is first["raw"][1]
    assert _same_raw(both, whole) and int(whole["raw"][0].sum()) == n * NI


def test_discretize_accumulates_over_chunked_windows(gpu_ctx, model_dir, chunks):
    per_lane = PER_LANE["discretize"](T_BIG, 4)
    n = _n(PER_LANE["discretize"](T_BIG, 4, dyn=False))   # 59 993 lanes of the large trace: ten chunks
    h = n // 2 + 3
    nm, g, iv, dv = _values(gpu_ctx, model_dir, N_BIG, T_BIG)
    whole = chunks.many(lambda: native.discretize_dbn_host(gpu_ctx, nm, iv, dv, T_BIG, 4, raw=True, n=n), n, per_lane)
    first = chunks.many(lambda: native.discretize_dbn_host(gpu_ctx, nm, iv, dv, T_BIG, 4, raw=True, n=h, col_offset=0), h, per_lane)
    assert not np.array_equal(first["raw"][0], whole["raw"][0])
    both = chunks.many(lambda: native.discretize_dbn_host(gpu_ctx, nm, iv, dv, T_BIG, 4, raw=True, n=n - h, col_offset=h, counts=first["raw"]),
                       n - h, per_lane)
    assert both["raw"][0] is first["raw"][0] and both["raw"][1] is first["raw"][1]
    assert _same_raw(both, whole) and whole["raw"][0].any() and whole["raw"][1].any()
    assert np.array_equal(first["init_bin"] + both["init_bin"], whole["init_bin"])            # (each call's other columns are 0)
    assert np.array_equal(first["dyn_bin"] + both["dyn_bin"], whole["dyn_bin"])
