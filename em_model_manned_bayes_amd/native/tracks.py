"""Tracks: the uncorrelated model's point-mass tracks, the terminal model's propagated and accepted encounters, sample2track from values
or from the transition file's text."""
import ctypes as C

import numpy as np

from .. import _lib as L
from .base import _device_call, _event_cap_error, _p, _stream_handle
from .layout import split_rows
from .sampling import _fill_terminal
from .text import _buffer_address, _parse_error


def terminal_t0_row(cap):
    """EMGPU_TERMINAL_T0_ROW: the row of t = 0 in an aircraft's block of 2 * terminal_t0_row(cap) rows."""
    return (int(cap) + 7) & ~7


def propagate_terminal_joined_host(ctx, models, geo, model_of, seed, first_index=0, tmax_s=120.0, dyn_limits=None,
                                   max_resample=100000, cap=None, local_smooth=False):
    """emgpu_propagate_terminal_host: PropagateTrajectory for 4 tracks per encounter (createEncounter.m:52-72) in the library's
    own layout.  models: list of NativeModel (stay prior already applied); geo [n, 12]; model_of [n, 4].
    Returns (traj [2n, 2 C, 5] f32, C = terminal_t0_row(cap): the joined track of aircraft 2e + a, row C + t = second t, fields x_nm y_nm z_ft
    heading_deg v_ft_s; rows [4n]: rows of track 4e + 2a + backward, < 0 = failed).  Rows outside a track's span are 0."""
    geo = np.ascontiguousarray(np.asarray(geo, dtype=np.float64).reshape(-1, 12))
    n = geo.shape[0]
    model_of = np.ascontiguousarray(np.asarray(model_of, dtype=np.int32).reshape(-1))
    assert model_of.size == 4 * n
    cap = int(cap or (int(tmax_s) + 3))
    p = L.TermParams()
    p.seed, p.first_index, p.n, p.tmax_s = int(seed) & (2**64 - 1), int(first_index), n, float(tmax_s)
    p.max_resample, p.cap = int(max_resample), cap
    p.flags = L.FLAG_LOCAL_SMOOTH if local_smooth else 0
    p.dyn_limits[:] = np.asarray(dyn_limits, dtype=np.float64).reshape(10).tolist()
    handles = (C.c_void_p * len(models))(*[m._h for m in models])
    traj = np.zeros((2 * n, 2 * terminal_t0_row(cap), 5), dtype=np.float32)
    rows = np.zeros(4 * n, dtype=np.int32)
    L.check(L.lib().emgpu_propagate_terminal_host(ctx._h, handles, len(models), C.byref(p), _p(geo), _p(model_of), _p(traj), _p(rows)))
    return traj, rows


def split_joined_tracks(traj, rows, cap):
    """The four PropagateTrajectory results of every encounter, as the reference's function returns them one by one
    (createEncounter.m:96, 162-167), cut out of the joined tracks: out [4n, cap, 6] f32 = t_s x_nm y_nm z_ft heading_deg v_ft_s of
    track 4e + 2a + backward, row r = second +-r (rows beyond rows[l] are 0)."""
    n4 = rows.size
    out = np.zeros((n4, cap, 6), dtype=np.float32)
    c0 = terminal_t0_row(cap)
    r = np.arange(cap)
    for d, sign in ((0, 1), (1, -1)):
        src = traj[:, c0 + sign * r, :]                      # [2n, cap, 5]
        lanes = np.arange(d, n4, 2)                            # lane 4e + 2a + d  <->  aircraft 2e + a
        keep = r[None, :] < np.abs(np.where(rows[lanes] < 0, -rows[lanes] - 1, rows[lanes]))[:, None]
        out[lanes, :, 1:] = np.where(keep[:, :, None], src, 0)
        out[lanes, :, 0] = np.where(keep, sign * r[None, :], 0)
    return out


def propagate_terminal_host(ctx, models, geo, model_of, seed, first_index=0, tmax_s=120.0, dyn_limits=None,
                            max_resample=100000, cap=None, local_smooth=False):
    """propagate_terminal_joined_host, returned per PropagateTrajectory call like the reference does:
    (out [4n, cap, 6] f32 as t_s x_nm y_nm z_ft heading_deg v_ft_s, rows [4n])."""
    cap = int(cap or (int(tmax_s) + 3))
    traj, rows = propagate_terminal_joined_host(ctx, models, geo, model_of, seed, first_index, tmax_s, dyn_limits, max_resample, cap, local_smooth)
    return split_joined_tracks(traj, rows, cap), rows


def utrack_params(model, n, sample_time, seed, first_index=0, is_quantize500=False, is_rotorcraft=False,
                  max_track_attempts=200, max_attempts=1000, record_stride=1):
    """emgpu_utrack_params with the variable ids looked up by label like UncorEncounterModel.m:385-391."""
    labels = model.get_labels(L.F_LABELS_INITIAL)

    def lab(name):
        q = '"%s"' % name
        return labels.index(q) + 1 if q in labels else 0
    p = L.UTrackParams()
    p.seed, p.first_index, p.n, p.sample_time = int(seed) & (2**64 - 1), int(first_index), int(n), int(sample_time)
    p.flags = L.FLAG_QUANTIZE500 if is_quantize500 else 0
    p.max_track_attempts, p.max_attempts, p.record_stride = int(max_track_attempts), int(max_attempts), int(record_stride)
    p.idx_G, p.idx_A, p.idx_L, p.idx_v = lab("G"), lab("A"), lab("L"), lab("v")
    p.idx_dv, p.idx_dh, p.idx_dpsi = lab("\\dot v"), lab("\\dot h"), lab("\\dot \\psi")
    p.is_rotorcraft = int(bool(is_rotorcraft))
    return p


def track_uncor_host(ctx, model, n, sample_time, seed, want_tracks=True, start=None, **kw):
    """emgpu_track_uncor_host: UncorEncounterModel.track on the GPU (sample -> point-mass dynamics -> rejection rounds).
    Returns dict: tracks [n, S, 8] (time north east up speed phi theta psi), limits [n, 3], attempts [n], kernel.
    start: a start grid [n, n_initial] of preset bins (0 = unset), every attempt of track i drawn under row i (emgpu_track_uncor_grid_host)."""
    p = utrack_params(model, n, sample_time, seed, **kw)
    S = 10 * int(sample_time) // p.record_stride + 1
    tracks = np.zeros((n, S, 8)) if want_tracks else None
    limits = np.zeros((n, 3))
    attempts = np.zeros(n, dtype=np.int32)
    if start is not None:
        st = np.ascontiguousarray(start, dtype=np.int32)
        assert st.shape == (int(n), model.n_initial)
        L.check(L.lib().emgpu_track_uncor_grid_host(ctx._h, model._h, C.byref(p), _p(st), _p(tracks), _p(limits), _p(attempts)))
    else:
        L.check(L.lib().emgpu_track_uncor_host(ctx._h, model._h, C.byref(p), _p(tracks), _p(limits), _p(attempts)))
    return {"tracks": tracks, "limits": limits, "attempts": attempts, "kernel": ctx.last_kernel()}


def track_uncor_device(ctx, model, n, sample_time, seed, tracks=0, limits=0, attempts=0, start=0, **kw):
    """emgpu_track_uncor_device: track_uncor_host into the caller's device buffers (raw pointers, ints, 0 = skip): tracks [n, S, 8] f64,
    limits [n, 3] f64, attempts [n] i32, in the layouts of track_uncor_host; start: a start grid [n, n_initial] i32 on the device
    (emgpu_track_uncor_grid_device).  Returns the kernel names."""
    _device_call("track_uncor_grid_device", (ctx, model), utrack_params(model, n, sample_time, seed, **kw), start, tracks, limits, attempts)
    return ctx.last_kernel()


def uncor_dynamic_limits(model, initial, up_min, up_max, speed_min, speed_max, is_rotorcraft=False):
    """emgpu_uncor_dynamic_limits: getDynamicLimits.m for one trajectory (host only, no GPU needed)."""
    p = utrack_params(model, 1, 1, 0, is_rotorcraft=is_rotorcraft)
    iv = np.ascontiguousarray(initial, dtype=np.float64)
    out = np.zeros(3)
    L.check(L.lib().emgpu_uncor_dynamic_limits(model._h, C.byref(p), _p(iv), float(up_min), float(up_max), float(speed_min), float(speed_max), _p(out)))
    return out


def track_terminal_host(ctx, geom_model, traj_models, n, seed, dyn_limits, max_cum_turn_deg, pitch_deg, first_index=0, tmax_s=120.0,
                        min_enc_time_s=30.0, thres_dist_ft=2.5 * 6076, thres_alt_low_ft=750.0, thres_vertrate_ft_s=300.0 / 60.0,
                        bounds_sample=None, max_track_attempts=500, max_attempts=100000, max_resample=100000, allow_cap=False, local_smooth=True,
                        want_traj=True):
    """emgpu_track_terminal_host: CorTerminalModel.track (track.m:45-150) on the GPU.  Returns dict: sample [n, n_i], traj [n, 2, cap2, 6]
    (t_s x_nm y_nm z_ft heading_deg v_ft_s, time-ordered), len [n, 2], meta [n, 4] (tcpa_s hmd_ft vmd_ft enc_time_s), attempts [n].
    want_traj=False: traj is None and the library gets no track buffer (it is 2 * cap2 * 48 bytes per encounter).
    local_smooth -- ONE rule for every Python layer: a function smooths by default exactly when the reference function it mirrors does.
    track.m calls createEncounter, whose lines 88-89 smooth speed and altitude, so this helper, CorTerminalModel.track and
    CorTerminalModel.createEncounter default to True; PropagateTrajectory (createEncounter.m:93-265) does not smooth, so
    propagate_terminal_host / _joined_host default to False.  The C ABI has no defaults (a zeroed `flags` field is off: set
    EMGPU_FLAG_LOCAL_SMOOTH).  The smoother itself is the library's documented stand-in for em-core's un-vendored local_smooth: UNPINNED."""
    p = L.TTrackParams()
    bs = _fill_terminal(p, geom_model, n, seed, first_index, tmax_s, dyn_limits, bounds_sample, max_attempts, max_resample, local_smooth)   # (bs: alive through the call)
    p.max_track_attempts = int(max_track_attempts)
    for a in range(2):
        p.max_cum_turn_deg[a], p.pitch_deg[a] = float(max_cum_turn_deg[a]), float(pitch_deg[a])
    p.min_enc_time_s, p.thres_dist_ft, p.thres_alt_low_ft, p.thres_vertrate_ft_s = float(min_enc_time_s), float(thres_dist_ft), float(thres_alt_low_ft), float(thres_vertrate_ft_s)
    ni, cap2 = geom_model.n_initial, 2 * (int(tmax_s) + 3)
    sample = np.zeros((n, ni)); traj = np.zeros((n, 2, cap2, 6)) if want_traj else None; ln = np.zeros((n, 2), dtype=np.int32)
    meta = np.zeros((n, 4)); att = np.zeros(n, dtype=np.int32)
    if len(traj_models) != 10:
        raise ValueError("traj_models: the 10 trajectory models in CorTerminalModel.m:84-100 order")
    handles = (C.c_void_p * len(traj_models))(*[m._h for m in traj_models])
    rc = L.lib().emgpu_track_terminal_host(ctx._h, geom_model._h, handles, len(traj_models), C.byref(p), _p(sample), _p(traj), cap2, _p(ln), _p(meta), _p(att))
    if not (allow_cap and rc == L.ERR_REJECT_CAP):   # the outputs of the encounters that were accepted are delivered either way (attempts -1 marks the rest)
        L.check(rc)
    return {"sample": sample, "traj": traj, "len": ln, "meta": meta, "attempts": att, "kernel": ctx.last_kernel()}


def terminal_filter_params(n, cap, dyn_limits, max_cum_turn_deg, pitch_deg, cap2=0, min_enc_time_s=30.0, thres_dist_ft=2.5 * 6076,
                           thres_alt_low_ft=750.0, thres_vertrate_ft_s=300.0 / 60.0):
    """emgpu_tfilter_params: n encounters in blocks of 2 * terminal_t0_row(cap) rows, the limits and thresholds of track_terminal_host,
    cap2 rows per track of the traj output."""
    p = L.TFilterParams()
    p.n, p.cap, p.cap2 = int(n), int(cap), int(cap2)
    p.dyn_limits[:] = np.asarray(dyn_limits, dtype=np.float64).reshape(10).tolist()
    for a in range(2):
        p.max_cum_turn_deg[a], p.pitch_deg[a] = float(max_cum_turn_deg[a]), float(pitch_deg[a])
    p.min_enc_time_s, p.thres_dist_ft, p.thres_alt_low_ft, p.thres_vertrate_ft_s = float(min_enc_time_s), float(thres_dist_ft), float(thres_alt_low_ft), float(thres_vertrate_ft_s)
    return p


def filter_terminal_device(params, geo, tracks, rows, accepted, meta=0, len=0, traj=0, stream=None):
    """emgpu_filter_terminal_device: k_terminal_filter once on the caller's track blocks (raw device pointers, ints, 0 = skip an output;
    params: terminal_filter_params).  geo [n, 12] f64, tracks [2n, 2 C, 5] f32 and rows [4n] i32 in propagate_terminal_joined_host's
    layout; accepted [n] u8, meta [n, 4] f64, len [n, 2] i32, traj [n, 2, cap2, 6] f64, the last three written for accepted encounters
    only.  No context: the current device and `stream` (a raw hipStream_t; 0: the HIP default stream; None: torch's current stream).
    Asynchronous."""
    _device_call("filter_terminal_device", (_stream_handle(stream),), params, geo, tracks, rows, accepted, meta, len, traj)


def smooth_terminal_device(n2, cap, tracks, rows, stream=None):
    """emgpu_smooth_terminal_device: k_terminal_smooth on n2 joined tracks [n2, 2 C, 5] f32 (rows [2 n2] i32), speed and altitude smoothed
    in place.  Raw device pointers; the stream as filter_terminal_device's.  Asynchronous."""
    L.check(L.lib().emgpu_smooth_terminal_device(_stream_handle(stream), int(n2), int(cap), C.c_void_p(int(tracks or 0) or None),
                                                 C.c_void_p(int(rows or 0) or None)))


def track_params(n, T, ur_speed, ur_vertrate, ur_heading, min_speed, max_speed, nd=0, slot_vertrate=0, slot_acc=0, slot_turnrate=0):
    p = L.TrackParams()
    p.n, p.T, p.nd = int(n), int(T), int(nd)
    p.slot_vertrate, p.slot_acc, p.slot_turnrate = int(slot_vertrate), int(slot_acc), int(slot_turnrate)
    p.ur_speed, p.ur_vertrate, p.ur_heading = float(ur_speed), float(ur_vertrate), float(ur_heading)
    p.min_speed, p.max_speed = float(min_speed), float(max_speed)
    return p


def sample2track_host(ctx, alt0, speed0, updates, ur_speed, ur_vertrate, ur_heading, min_speed, max_speed):
    """emgpu_sample2track_host: sample2track.m:183-243 on the GPU for values parsed from the em_sample files.
    alt0, speed0 [n]; updates [n, T, 3] = vertical rate, acceleration, turn rate (model units).
    Returns (xyz [n, T+1, 3] f64 feet, flags [n] u8 (bit 0 CFIT, bit 1 speed), speed_minmax [n, 2])."""
    alt0 = np.ascontiguousarray(alt0, dtype=np.float64).reshape(-1)
    speed0 = np.ascontiguousarray(speed0, dtype=np.float64).reshape(-1)
    updates = np.ascontiguousarray(updates, dtype=np.float64)
    n, T = updates.shape[0], updates.shape[1]
    assert updates.shape == (n, T, 3) and alt0.size == n and speed0.size == n
    p = track_params(n, T, ur_speed, ur_vertrate, ur_heading, min_speed, max_speed)
    xyz = np.zeros((n, T + 1, 3))
    flags = np.zeros(n, dtype=np.uint8)
    vmm = np.zeros((n, 2))
    L.check(L.lib().emgpu_sample2track_host(ctx._h, C.byref(p), _p(alt0), _p(speed0), _p(updates), _p(xyz), _p(flags), _p(vmm)))
    return xyz, flags, vmm


def sample2track_device(ctx, params, alt0, speed0, dyn_val, xyz=0, flags=0, speed_minmax=0):
    """emgpu_sample2track_device with raw device pointers (ints, 0 = skip an output): consumes the sampler's
    device output in place (alt0 / speed0 = rows of init_val, dyn_val = the dense trace).  Asynchronous."""
    _device_call("sample2track_device", (ctx,), params, alt0, speed0, dyn_val, xyz, flags, speed_minmax)


def tracks_text_host(ctx, text, ncol, cols, ids, alt0, speed0, ur_speed, ur_vertrate, ur_heading, min_speed, max_speed, want_csv=True,
                     csv=None, csv_cap=None, want_xyz=False, header_lines=1):
    """emgpu_tracks_text_host: the transition table `text` (bytes-like or uint8 array; pinned: no staging) parsed on the device, the tracks of
    the wanted ids integrated from it and their CSV files formatted there.  cols: the 0-based columns of vertical rate, acceleration, turn rate.
    Returns a dict: flags [n] u8, speed_minmax [n, 2], lengths [n] i32, offsets [n + 1] u64 and csv (uint8: file i is csv[offsets[i]:
    offsets[i + 1]]; None unless want_csv), totals {"csv_bytes", "rows", "hard_tokens", "host_formatted", "noncontiguous"}, xyz (list of
    [lengths[i] + 1, 3] views, when want_xyz), phase_ms, kernel, host_stats.  csv: a uint8 buffer of the caller's (default: a pinned one of
    csv_cap bytes, or measured by a first call that writes nothing).  A buffer that is too small raises EmgpuError(ERR_EVENT_CAP) with
    `.totals`.  A malformed line raises ValueError (its line counted with header_lines in front)."""
    addr, nbytes, keep = _buffer_address(text)
    ids = np.ascontiguousarray(ids, dtype=np.float64).reshape(-1)
    alt0 = np.ascontiguousarray(alt0, dtype=np.float64).reshape(-1)
    speed0 = np.ascontiguousarray(speed0, dtype=np.float64).reshape(-1)
    n = ids.size
    assert alt0.size == n and speed0.size == n
    p = track_params(n, 1, ur_speed, ur_vertrate, ur_heading, min_speed, max_speed)
    i = L.TracksTextIn()
    i.text, i.nbytes, i.ncol = addr, nbytes, int(ncol)
    i.col_vertrate, i.col_acc, i.col_turnrate = (int(c) for c in cols)
    i.id, i.alt0, i.speed0 = _p(ids), _p(alt0), _p(speed0)
    flags, vmm, lengths = np.zeros(n, dtype=np.uint8), np.zeros((n, 2)), np.zeros(n, dtype=np.int32)
    offsets, totals, phase = np.zeros(n + 1, dtype=np.uint64), np.zeros(5, dtype=np.int64), np.zeros(6)

    def call(csv_buf, cap, xyz_buf=None):
        o = L.TracksTextOut()
        o.flags, o.speed_minmax, o.lengths, o.totals, o.phase_ms = _p(flags), _p(vmm), _p(lengths), _p(totals), _p(phase)
        if want_csv:
            o.offsets = _p(offsets)
            if csv_buf is not None:
                o.csv, o.csv_cap = _p(csv_buf), int(cap)
        if xyz_buf is not None:
            o.xyz, o.xyz_cap = _p(xyz_buf), xyz_buf.shape[0]
        rc = L.lib().emgpu_tracks_text_host(ctx._h, C.byref(p), C.byref(i), C.byref(o))
        if rc == L.ERR_PARSE:
            raise _parse_error(rc, int(header_lines), "tracks_text_host")
        if rc == L.ERR_EVENT_CAP:
            raise _event_cap_error(rc, totals.copy())
        L.check(rc)

    xyz_buf = None
    if want_csv and csv is None and csv_cap is None:
        call(None, 0)                                      # measured first: the buffer is sized from the totals
        csv_cap = int(totals[0])
    if want_csv and csv is None:
        csv = ctx.pinned_empty((max(int(csv_cap), 1),), np.uint8)
    if want_csv:
        csv_cap = csv.size if csv_cap is None else int(csv_cap)
    call(csv, csv_cap)
    if want_xyz:
        xyz_buf = np.empty((int(lengths.astype(np.int64).sum()) + n, 3))
        call(csv, csv_cap, xyz_buf)
    del keep
    out = {"flags": flags, "speed_minmax": vmm, "lengths": lengths, "offsets": offsets if want_csv else None,
           "csv": csv[: int(totals[0])] if want_csv else None,
           "totals": dict(zip(("csv_bytes", "rows", "hard_tokens", "host_formatted", "noncontiguous"), (int(v) for v in totals))),
           "phase_ms": dict(zip(("h2d", "parse", "track", "csv", "d2h", "host"), (float(v) for v in phase))),
           "kernel": ctx.last_kernel(), "host_stats": ctx.host_stats(), "xyz": None}
    if want_xyz:
        ends = np.cumsum(lengths.astype(np.int64) + 1)
        out["xyz"] = split_rows(xyz_buf, ends)
    return out
