"""The sampling calls: emgpu_sample_dbn_* with raw device pointers or numpy arrays, the uncorrelated model's arrays, the static network,
the start grid's weights and the terminal model's draw."""
import ctypes as C

import numpy as np

from .. import _lib as L
from .base import EVENT_DTYPE, _array_factory, _device_call, _event_cap_error, _p, make_params
from .layout import TraceLayout, split_rows, unpack_dyn_bin, unpack_dyn_val


def _sample_out(init_bin=0, init_val=0, dyn_bin=0, dyn_val=0, ev_count=0, events=0, attempts=0, ld=0, col_offset=0, log_weight=0):
    o = L.SampleOut()
    o.init_bin, o.init_val, o.dyn_bin, o.dyn_val = init_bin or None, init_val or None, dyn_bin or None, dyn_val or None
    o.ev_count, o.events, o.attempts, o.log_weight = ev_count or None, events or None, attempts or None, log_weight or None
    o.ld, o.col_offset = int(ld), int(col_offset)
    return o


def sample_dbn_device(ctx, model, params, init_bin=0, init_val=0, dyn_bin=0, dyn_val=0, ev_count=0, events=0, attempts=0,
                      ld=0, col_offset=0, log_weight=0):
    """Asynchronous launch with raw device pointers (ints, 0 = skip).  ld / col_offset: write this call's
    trajectories into columns [col_offset, col_offset + n) of buffers dimensioned for ld trajectories.  log_weight: [n] f64, not
    offset by col_offset (a start grid goes in through make_params(start=device pointer))."""
    o = _sample_out(init_bin, init_val, dyn_bin, dyn_val, ev_count, events, attempts, ld, col_offset, log_weight)
    L.check(L.lib().emgpu_sample_dbn_device(ctx._h, model._h, C.byref(params), C.byref(o)))


def mixed_blocks(n_total, n_models, lo=0, hi=None):
    """emgpu_mixed_blocks: [(model, first_index, count)] of the equal-contiguous-block assignment inside [lo, hi)."""
    hi = n_total if hi is None else hi
    buf = (L.Block * max(1, int(n_models)))()
    k = L.check(L.lib().emgpu_mixed_blocks(int(n_total), int(n_models), int(lo), int(hi), buf))
    return [(int(buf[i].model), int(buf[i].first_index), int(buf[i].n)) for i in range(k)]


def sample_dbn_blocks_device(ctx, models, params, blocks, **ptrs):
    """emgpu_sample_dbn_blocks_device: one shared trace (device pointers in ptrs, as for sample_dbn_device) filled by
    blocks = [(model index, first_index, count)]; params.n / params.first_index describe the range the trace covers."""
    o = _sample_out(**ptrs)
    handles = (C.c_void_p * len(models))(*[m._h for m in models])
    arr = (L.Block * max(1, len(blocks)))()
    for i, (m, f, c) in enumerate(blocks):
        arr[i].model, arr[i].first_index, arr[i].n = int(m), int(f), int(c)
    L.check(L.lib().emgpu_sample_dbn_blocks_device(ctx._h, handles, len(models), C.byref(params), arr, len(blocks), C.byref(o)))


def sample_dbn_multi_device(ctxs, model, params, outs):
    """emgpu_sample_dbn_multi_device: outs = one dict of device pointers (sample_dbn_device keywords) per ctx, each
    holding that ctx's shard (native.shard_range(params.n, d, len(ctxs))).  Asynchronous: sync every ctx afterwards."""
    hs = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    arr = (L.SampleOut * len(ctxs))(*[_sample_out(**kw) for kw in outs])
    L.check(L.lib().emgpu_sample_dbn_multi_device(hs, len(ctxs), model._h, C.byref(params), arr))


def sample_dbn_host(ctx, model, n, sample_time, seed, want_dense=True, want_events=False, event_cap=None, want_log_weight=False, pinned=True,
                    raw=False, **kw):
    """Synchronous host-buffer call.  Returns a dict of numpy arrays in user-facing shapes:
    init_bin [n, n_i] u8, init_val [n, n_i] f32, dyn_bin [n, T, n_d] u8, dyn_val [n, T, n_d] f32,
    events: list of structured arrays (EVENT_DTYPE), attempts [n].
    ctx may be a list of Contexts (one per device): the batch is then split over them inside ONE library call
    (emgpu_sample_dbn_multi_host: one host thread + one stream per device) with identical results.
    pinned: the library's arrays come from the context's pinned pool (the copy engine writes straight into them); False: pageable numpy
    arrays, which the library fills through its own staging buffers -- what a caller's own arrays (MATLAB's, a C host's) get.
    raw: return the arrays in the library's layout (init_* [n_i, n], dyn_bin [G4, n_d, n] u32, dyn_val [G4, n_d, n, 4]) without the
    transposing copies; `host_stats` = emgpu_host_stats of the call either way.
    """
    ni, nd, T = model.n_initial, model.n_dyn, int(sample_time)
    if want_events and event_cap is None:
        event_cap = min((ni + nd + 1) * T + 2, 4096)
    p, keep = make_params(n, T, seed, event_cap=event_cap or 0, **kw)
    lay = TraceLayout(ni, nd, n, T)
    ctx0 = ctx[0] if isinstance(ctx, (list, tuple)) else ctx
    empty = _array_factory(ctx0, pinned, np.zeros)
    o = L.SampleOut()
    ib = lay.make("init_bin", empty)
    iv = lay.make("init_val", empty)
    att = empty((n,), np.int32)
    o.init_bin, o.init_val, o.attempts = _p(ib), _p(iv), _p(att)
    if want_dense and nd > 0:
        db = lay.make("dyn_bin", empty)
        dv = lay.make("dyn_val", empty)
        o.dyn_bin, o.dyn_val = _p(db), _p(dv)
    if want_events:
        ec = empty((n,), np.uint32)
        ev = empty((n, event_cap), EVENT_DTYPE)
        o.ev_count, o.events = _p(ec), _p(ev)
    if want_log_weight:
        lw = np.zeros(n, dtype=np.float64)
        o.log_weight = _p(lw)
    if isinstance(ctx, (list, tuple)):
        hs = (C.c_void_p * len(ctx))(*[c._h for c in ctx])
        L.check(L.lib().emgpu_sample_dbn_multi_host(hs, len(ctx), model._h, C.byref(p), C.byref(o)))
    else:
        L.check(L.lib().emgpu_sample_dbn_host(ctx._h, model._h, C.byref(p), C.byref(o)))
    ctx = ctx0
    out = {"attempts": np.array(att), "kernel": ctx.last_kernel(), "host_stats": ctx.host_stats()}
    if raw:
        out["init_bin"], out["init_val"] = ib, iv
    else:
        out["init_bin"], out["init_val"] = ib.T.copy(), iv.T.copy()
    if want_log_weight:
        out["log_weight"] = lw
    if want_dense and nd > 0:
        out["dyn_bin"] = db if raw else unpack_dyn_bin(db, T)
        out["dyn_val"] = dv if raw else unpack_dyn_val(dv, T)
    if want_events:
        ec = np.array(ec)
        flat = ev[np.arange(ev.shape[1], dtype=np.uint32)[None, :] < ec[:, None]]   # all rows in order, one array (no per-sample concatenation; a copy)
        out["ev_count"] = ec
        out["events_flat"] = flat
        ends = np.cumsum(ec.astype(np.int64))
        out["events"] = split_rows(flat, ends)
    return out


def sample_uncor_host(ctx, model, n, sample_time, seed, ctrl_var, event_cap=256, events_cap=None, controls_cap=None, want_samples=True,
                      pinned=True, **kw):
    """emgpu_sample_uncor_host: UncorEncounterModel.sample's arrays built on the device.  Returns a dict:
    inits [n, n_i] f64, ev_count [n] u32, events [rows] EVENT_DTYPE (list after list), ctrl_count [n] u32, controls [rows, 4] f64
    (trajectory after trajectory), samples [n, n_i, T] f64 (None unless want_samples), attempts [n] i32, kernel, host_stats.
    ctrl_var: the 1-based ids of "\\dot h", "\\dot \\psi", "\\dot v".
    pinned: the per-trajectory arrays come from the context's pinned pool (the copy engine writes straight into them); False: pageable
    numpy arrays, filled through the library's staging buffers.  The packed rows go into arrays of events_cap / controls_cap rows (default
    n * event_cap: pinned when `pinned` and a capacity is given, else pageable, whose untouched pages cost nothing) and are returned trimmed.
    A list longer than event_cap, or rows beyond a capacity, raise EmgpuError(ERR_EVENT_CAP) with `.totals` (the rows needed, see emgpu.h)
    and `.ev_count` set: a retry with that much room gives the same draws.
    start= (make_params): a start grid [n, n_initial]; the weights of its rows: start_grid_log_weight."""
    ni, T, n = model.n_initial, int(sample_time), int(n)
    p, keep = make_params(n, T, seed, event_cap=int(event_cap), **kw)
    empty = _array_factory(ctx, pinned, np.empty)
    rows_empty = lambda cap_, shape, dt: (empty if cap_ is not None else _array_factory(ctx, False, np.empty))(shape, dt)
    ev_cap = int(events_cap) if events_cap is not None else n * int(event_cap)
    ct_cap = int(controls_cap) if controls_cap is not None else n * int(event_cap)
    o = L.UncorOut()
    inits, ec, cc, att = empty((n, ni), np.float64), empty((n,), np.uint32), empty((n,), np.uint32), empty((n,), np.int32)
    ev = rows_empty(events_cap, (max(ev_cap, 1),), EVENT_DTYPE)
    ctl = rows_empty(controls_cap, (max(ct_cap, 1), 4), np.float64)
    smp = empty((n, ni, T), np.float64) if want_samples else None
    totals = np.zeros(2, dtype=np.int64)
    o.inits, o.ev_count, o.ctrl_count, o.attempts, o.events, o.controls = _p(inits), _p(ec), _p(cc), _p(att), _p(ev), _p(ctl)
    o.events_cap, o.controls_cap, o.samples, o.totals = ev_cap, ct_cap, _p(smp), _p(totals)
    o.ctrl_var[:] = [int(v) for v in ctrl_var]
    rc = L.lib().emgpu_sample_uncor_host(ctx._h, model._h, C.byref(p), C.byref(o))
    if rc == L.ERR_EVENT_CAP:
        raise _event_cap_error(rc, (int(totals[0]), int(totals[1])), ev_count=ec)
    L.check(rc)
    return {"inits": inits, "ev_count": ec, "events": ev[: int(totals[0])], "ctrl_count": cc, "controls": ctl[: int(totals[1])],
            "samples": smp, "attempts": att, "kernel": ctx.last_kernel(), "host_stats": ctx.host_stats()}


def _same_shape(a, b):
    tm_a, tm_b = a.get_i32(L.F_TEMPORAL_MAP).reshape(-1, 2), b.get_i32(L.F_TEMPORAL_MAP).reshape(-1, 2)
    if a.n_initial != b.n_initial or not np.array_equal(a.get_i32(L.F_R_INITIAL), b.get_i32(L.F_R_INITIAL)):
        return False
    if not np.array_equal(tm_a, tm_b):
        return False
    return bool(np.array_equal(a.get_i32(L.F_R_TRANSITION)[tm_a[:, 1] - 1], b.get_i32(L.F_R_TRANSITION)[tm_b[:, 1] - 1])) if len(tm_a) else True


def sample_bn_host(ctx, model, n, seed, first_index=0, dediscretize=False, max_attempts=100000, bounds_sample=None,
                   idx_own_speed=0, idx_int_speed=0, lim1=(0.0, np.inf), lim2=(0.0, np.inf), start=None, want_log_weight=False):
    """bn_sample.m (dediscretize=False) or the CorTerminalModel geometry draw (sample.m:29-77).  start: a start grid [n, n_initial]
    (0 = unset) -- one row of presets per sample, ONE launch; want_log_weight: also return the per-sample log-weights (4th value)."""
    p = L.BnParams()
    p.seed, p.first_index, p.n = int(seed) & (2**64 - 1), int(first_index), int(n)
    p.flags = 0 if dediscretize else L.FLAG_NO_DEDISC
    p.max_attempts = int(max_attempts)
    bs = None
    if bounds_sample is not None:
        bs = np.ascontiguousarray(np.asarray(bounds_sample, dtype=np.float64).reshape(model.n_initial, 2))
        p.bounds_sample = _p(bs)
    p.idx_own_speed, p.idx_int_speed = int(idx_own_speed), int(idx_int_speed)
    p.min_vel1, p.max_vel1, p.min_vel2, p.max_vel2 = float(lim1[0]), float(lim1[1]), float(lim2[0]), float(lim2[1])
    ob = np.zeros((model.n_initial, n), dtype=np.uint8)
    ov = np.zeros((model.n_initial, n), dtype=np.float32)
    att = np.zeros(n, dtype=np.int32)
    st = lw = None
    if start is not None:
        st = np.ascontiguousarray(start, dtype=np.int32)
        assert st.shape == (n, model.n_initial)
        p.start = _p(st)
    if want_log_weight:
        lw = np.zeros(n, dtype=np.float64)
        p.log_weight = _p(lw)
    L.check(L.lib().emgpu_sample_bn_host(ctx._h, model._h, C.byref(p), _p(ob), _p(ov), _p(att)))
    if want_log_weight:
        return ob.T.copy(), ov.T.copy(), att, lw
    return ob.T.copy(), ov.T.copy(), att


def start_grid_log_weight(model, grid):
    """emgpu_start_grid_log_weight (host only, no GPU needed): log P(presets of row i) for every row of a start grid [n, n_initial]
    (0 = unset: the model's own start) -- bit for bit the log_weight a sampling call returns for that row.  EmgpuError(ERR_PRESET) names the
    first row that presets a node without its parents or to a bin outside 1..r."""
    g = np.ascontiguousarray(grid, dtype=np.int32)
    if g.ndim != 2 or g.shape[1] != model.n_initial:
        raise ValueError("a start grid has n_initial columns")
    out = np.zeros(g.shape[0], dtype=np.float64)
    L.check(L.lib().emgpu_start_grid_log_weight(model._h, _p(g), g.shape[0], _p(out)))
    return out


TERMINAL_GEO_FIELDS = ("distance", "bearing", "alt", "speed", "heading", "intent")


def _fill_terminal(p, geom_model, n, seed, first_index, tmax_s, dyn_limits, bounds_sample, max_attempts, max_resample, local_smooth):
    """The fields emgpu_tsample_params and emgpu_ttrack_params share, into either; returns the keep-alive of bounds_sample."""
    labels = [s.strip('"') for s in geom_model.get_labels(L.F_LABELS_INITIAL)]
    p.seed, p.first_index, p.n, p.tmax_s = int(seed) & (2**64 - 1), int(first_index), int(n), float(tmax_s)
    p.max_resample, p.max_attempts = int(max_resample), int(max_attempts)
    p.flags = L.FLAG_LOCAL_SMOOTH if local_smooth else 0
    p.dyn_limits[:] = np.asarray(dyn_limits, dtype=np.float64).reshape(10).tolist()
    bs = None
    if bounds_sample is not None:
        bs = np.ascontiguousarray(np.asarray(bounds_sample, dtype=np.float64).reshape(geom_model.n_initial, 2))
        p.bounds_sample = _p(bs)
    for a, pre in enumerate(("own", "int")):
        for k, f in enumerate(TERMINAL_GEO_FIELDS):
            p.idx[6 * a + k] = labels.index(pre + "_" + f) + 1
    return bs


def terminal_sample_params(geom_model, n, seed, dyn_limits, first_index=0, tmax_s=120.0, cap=None, bounds_sample=None,
                           max_attempts=100000, max_resample=100000, local_smooth=False):
    """emgpu_tsample_params for emgpu_sample_terminal_device; returns (params, keep-alive) -- the variable ids are looked up by label like
    @CorTerminalModel/sample.m:56-62 / createEncounter.m:45-49."""
    p = L.TSampleParams()
    p.cap = int(cap or (int(tmax_s) + 3))
    return p, _fill_terminal(p, geom_model, n, seed, first_index, tmax_s, dyn_limits, bounds_sample, max_attempts, max_resample, local_smooth)


def sample_terminal_device(ctx, geom_model, traj_models, p, geom_val, geo, model_of, traj, rows, geom_bin=0, attempts=0):
    """emgpu_sample_terminal_device: geometry draw + createEncounter inputs + PropagateTrajectory x 4, device pointers (integers)."""
    if len(traj_models) != 10:
        raise ValueError("traj_models: the 10 trajectory models in CorTerminalModel.m:84-100 order")
    handles = (C.c_void_p * 10)(*[m._h for m in traj_models])
    _device_call("sample_terminal_device", (ctx, geom_model, handles, 10), p, geom_bin, geom_val, geo, model_of, traj, rows, attempts)
