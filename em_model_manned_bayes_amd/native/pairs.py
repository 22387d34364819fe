"""Paired tracks: the one pairing, and on it the miss distance, the loss of well clear, the ownship's vertical avoidance manoeuvre and the
two placements of the intruder, on the encounter cylinder and at a drawn closest approach.  Torch does the plumbing here."""
import contextlib
import types

import numpy as np

from .. import _lib as L
from .base import _device_call, _stream_handle, _weights_array


def _pairing(p, n_pairs, n_a, n_b, points, ld_a, ld_b):
    """p, one of L's *Params, with its pairing filled in"""
    p.n_pairs, p.n_a, p.n_b, p.ld_a, p.ld_b, p.points = int(n_pairs), int(n_a), int(n_b), int(ld_a), int(ld_b), int(points)
    return p


def miss_params(n_pairs, n_a, n_b, points, nmac_h_ft=500.0, nmac_v_ft=100.0, ld_a=0, ld_b=0):
    """emgpu_miss_params: n_pairs pairs of a column of set A (n_a columns, pitch ld_a, 0 = n_a) and a column of set B, `points` seconds each;
    the NMAC thresholds of track.m:175 in feet."""
    p = _pairing(L.MissParams(), n_pairs, n_a, n_b, points, ld_a, ld_b)
    p.nmac_h_ft, p.nmac_v_ft = float(nmac_h_ft), float(nmac_v_ft)
    return p


def miss_distance_device(params, xyz_a, xyz_b, idx_a=0, idx_b=0, pose_b=0, weights=0, hmd=0, vmd=0, t_cpa=0, flags=0, totals=0, stream=None):
    """emgpu_miss_distance_device: asynchronous, raw device pointers (ints, 0 = none; params: miss_params).  xyz_a / xyz_b f64 PLANAR
    [P, 3, ld], idx_a / idx_b int64 [n_pairs], pose_b f64 [5, n_pairs] (make_pose), weights uint32 [n_pairs]; hmd / vmd f64, t_cpa int32,
    flags uint8 [n_pairs] each, totals uint64 [8], ADDED to.  The call takes no context: it runs on the current device and on `stream`, a
    raw hipStream_t (0: the HIP default stream; None: torch's current stream).  To stay ordered behind a sampler, pass the stream its
    Context was given (Context.stream)."""
    _device_call("miss_distance_device", (_stream_handle(stream),), params, xyz_a, xyz_b, idx_a, idx_b, pose_b, weights, hmd, vmd, t_cpa, flags,
                 totals)


def miss_segments_device(params, xyz_a, xyz_b, idx_a=0, idx_b=0, pose_b=0, weights=0, hmd=0, vmd=0, t_cpa_s=0, flags=0, totals=0, stream=None):
    """emgpu_miss_segments_device: miss_distance_device on the segments between the seconds, the tracks read as piecewise linear.  The
    arguments are miss_distance_device's but t_cpa_s f64 [n_pairs], the real-valued time of closest approach, and totals uint64 [10],
    ADDED to; flags may carry L.MISS_CPA_BETWEEN and L.MISS_NMAC_BETWEEN."""
    _device_call("miss_segments_device", (_stream_handle(stream),), params, xyz_a, xyz_b, idx_a, idx_b, pose_b, weights, hmd, vmd, t_cpa_s, flags,
                 totals)


def make_pose(heading_deg, ox=0.0, oy=0.0, oz=0.0):
    """The pose_b of miss_distance: [5, n] float64 on the host, rows cos, sin of heading_deg (counter-clockwise, MATLAB's cosd / sind: the
    reduction in degrees of CorTerminalModel._sincosd, so that multiples of 90 give exact 0 and +-1), then the offsets ox, oy, oz in feet.
    Track B is turned about its own origin by the heading, then moved by the offset.  The arguments broadcast against each other."""
    from ..encounter_model import CorTerminalModel
    h, ox, oy, oz = np.broadcast_arrays(*(np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (heading_deg, ox, oy, oz)))
    s, c = CorTerminalModel._sincosd(h)
    return np.ascontiguousarray(np.stack([c, s, ox, oy, oz]) + 0.0)   # (+ 0.0: -0.0 becomes 0.0)


def _planar_tracks(xyz, layout, dev):
    """xyz as a contiguous float64 PLANAR [P, 3, n] tensor on dev: numpy [n, P, 3] (layout "rows") or [P, 3, n] ("planar"), or a torch
    tensor in either layout, uploaded and transposed by torch"""
    import torch
    if layout not in ("rows", "planar"):
        raise ValueError("layout must be 'rows' or 'planar'")
    if not isinstance(xyz, torch.Tensor):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        xyz = xyz if xyz.flags.writeable else xyz.copy()      # (torch takes no read-only array; the tensor is only read)
    t = xyz if isinstance(xyz, torch.Tensor) else torch.from_numpy(xyz)
    if t.dim() != 3 or t.shape[2 if layout == "rows" else 1] != 3:
        raise ValueError("xyz must be [n, points, 3] (layout 'rows') or [points, 3, n] ('planar')")
    t = t.to(device=dev, dtype=torch.float64)
    return (t.permute(1, 2, 0) if layout == "rows" else t).contiguous()


def _pair_columns(xyz_a, xyz_b, idx_a, idx_b, layout):
    """(n_a, n_b, [idx_a, idx_b] as int64 vectors or None, n_pairs) of a pairing of two sets of tracks, as miss_distance reads its arguments"""
    import torch
    n_of = lambda t: int(t.shape[0 if layout == "rows" else 2])          # noqa: E731
    for t in (xyz_a, xyz_b):
        if getattr(t, "ndim", 0) != 3:
            raise ValueError("xyz must be [n, points, 3] (layout 'rows') or [points, 3, n] ('planar')")
    n_a, n_b = n_of(xyz_a), n_of(xyz_b)
    idx = [None if i is None else np.ascontiguousarray(i, dtype=np.int64).reshape(-1) if not isinstance(i, torch.Tensor) else i
           for i in (idx_a, idx_b)]
    return n_a, n_b, idx, max([len(i) for i in idx if i is not None] + [n for n, i in zip((n_a, n_b), idx) if i is None])


@contextlib.contextmanager
def _paired(xyz_a, xyz_b, columns, w, pose_b, layout, ctx, stream):
    """The pairing step of miss_distance, encounter_pose and encounter_miss: what a launch on paired tracks needs, as a namespace of
    dev, stream (resolved; None: torch's current stream), the PLANAR device tensors a / b, n_a, n_b, n_pairs, sizes (what every *_params
    opens with: n_pairs, n_a, n_b, points), and d_ia, d_ib (int64), d_w (uint32 held as int32) and d_pose on the device or None.
    columns = _pair_columns(...), w = _weights_array(...) or None: the caller has them before torch.cuda is touched.  The body runs on dev
    with the uploads complete for its stream; leaving it waits for that stream."""
    import torch
    n_a, n_b, idx, n_pairs = columns
    dev = xyz_a.device if isinstance(xyz_a, torch.Tensor) and xyz_a.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if ctx is not None and stream is None:
        stream = ctx.stream
        if stream is None:
            ctx.sync()
    with torch.cuda.device(dev):
        a, b = _planar_tracks(xyz_a, layout, dev), _planar_tracks(xyz_b, layout, dev)
        if a.shape[0] != b.shape[0]:
            raise ValueError("both sets of tracks must hold the same number of points")
        up = lambda x, dt: None if x is None else (x if isinstance(x, torch.Tensor) else torch.from_numpy(x)).to(device=dev, dtype=dt).contiguous()  # noqa: E731
        pr = types.SimpleNamespace(dev=dev, stream=stream, a=a, b=b, n_a=n_a, n_b=n_b, n_pairs=n_pairs, sizes=(n_pairs, n_a, n_b, a.shape[0]),
                                   d_ia=up(idx[0], torch.int64), d_ib=up(idx[1], torch.int64), d_pose=up(pose_b, torch.float64),
                                   d_w=None if w is None else torch.from_numpy(w.view(np.int32)).to(dev))
        # torch.cuda.synchronize brackets the launches only when they do not run on torch's stream, where the uploads ran
        pr.guard = (lambda: None) if stream is None else (lambda: torch.cuda.synchronize(dev))
        pr.guard()
        yield pr
        pr.guard()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _launch(pr, device_call, params, inputs, outputs, n_totals=0):
    """One kernel on the pairing pr: device_call(params, the pairing's four addresses, *inputs, *outputs[, totals]) on pr.stream, not waited
    for.  inputs: device tensors or None.  outputs: {name: dtype, [n_pairs]; or (dtype, 5), [5, n_pairs]; or None, not wanted} in the
    entry point's order, allocated here; n_totals: the width of the int64 totals behind them, zeroed, or 0 for none.  Returns the outputs
    as a tuple of device tensors."""
    import torch
    def empty(dtype, *rows):
        return torch.empty((*rows, pr.n_pairs), dtype=getattr(torch, dtype), device=pr.dev)
    out = [None if d is None else empty(*d) if isinstance(d, tuple) else empty(d) for d in outputs.values()]
    if n_totals:
        out.append(torch.zeros(n_totals, dtype=torch.int64, device=pr.dev))
        pr.guard()      # totals was zeroed on torch's stream
    device_call(params, *(_ptr(t) for t in (pr.a, pr.b, pr.d_ia, pr.d_ib, *inputs, *out)), stream=pr.stream)
    return tuple(out)


def _host(*tensors):
    """device tensors as numpy arrays; None stays None"""
    return [None if t is None else t.cpu().numpy() for t in tensors]


def _miss_tensors(pr, d_pose, d_w, nmac_h_ft, nmac_v_ft):
    """k_miss_distance on the pairing pr with the device tensors d_pose and d_w (or None): the device tensors (hmd, vmd, t_cpa, flags,
    totals), launched on pr.stream and not waited for"""
    return _launch(pr, miss_distance_device, miss_params(*pr.sizes, nmac_h_ft, nmac_v_ft), (d_pose, d_w),
                   {"hmd": "float64", "vmd": "float64", "t_cpa": "int32", "flags": "uint8"}, 8)


def _miss_dict(hmd, vmd, t_cpa, flags, totals):
    """miss_distance's dict from _miss_tensors' device tensors"""
    hmd, vmd, t_cpa, fl, tot = _host(hmd, vmd, t_cpa, flags, totals)
    return {"hmd_ft": hmd, "vmd_ft": vmd, "t_cpa": t_cpa, "flags": fl, "nmac": (fl & L.MISS_NMAC_CPA) != 0, "totals": tot.view(np.uint64)}


def _miss_segments_tensors(pr, d_pose, d_w, nmac_h_ft, nmac_v_ft):
    """k_miss_segments on the pairing pr, as _miss_tensors: the device tensors (hmd, vmd, t_cpa_s, flags, totals [10]), launched on pr.stream
    and not waited for"""
    return _launch(pr, miss_segments_device, miss_params(*pr.sizes, nmac_h_ft, nmac_v_ft), (d_pose, d_w),
                   {"hmd": "float64", "vmd": "float64", "t_cpa_s": "float64", "flags": "uint8"}, 10)


def _miss_segments_dict(hmd, vmd, t_cpa_s, flags, totals):
    """miss_segments' dict from _miss_segments_tensors' device tensors"""
    hmd, vmd, t_cpa_s, fl, tot = _host(hmd, vmd, t_cpa_s, flags, totals)
    return {"hmd_ft": hmd, "vmd_ft": vmd, "t_cpa_s": t_cpa_s, "flags": fl, "nmac": (fl & L.MISS_NMAC_CPA) != 0,
            "nmac_any": (fl & L.MISS_NMAC_ANY) != 0, "between": (fl & L.MISS_NMAC_BETWEEN) != 0, "totals": tot.view(np.uint64)}


def _placement(want_weights, **between):
    """the outputs of a placement for _launch: pose and rate, what lies `between` them and the flags, and the weights where wanted"""
    return {"pose": ("float64", 5), "rate": "float64", **between, "flags": "uint8", "weights_out": "int32" if want_weights else None}


def _encounter_pose_tensors(pr, want_weights, radius_ft, half_height_ft, seed, rate_scale, first_index, max_attempts):
    """k_encounter_pose on the pairing pr: the device tensors (pose [5, n_pairs], rate, flags, weights or None), launched on pr.stream and
    not waited for"""
    p = encounter_params(*pr.sizes, radius_ft, half_height_ft, seed, first_index, max_attempts, 1.0 if rate_scale is None else rate_scale)
    return _launch(pr, encounter_pose_device, p, (pr.d_w,), _placement(want_weights))


def _encounter_dict(rate, flags, w_out, flags_key="flags"):
    """the rate, flags and weights of encounter_pose's dict from _encounter_pose_tensors' device tensors"""
    rate, fl, w = _host(rate, flags, w_out)
    return {"rate": rate, flags_key: fl, "weights": None if w is None else w.view(np.uint32)}


def _encounter_weights(weights, rate_scale, n_pairs):
    """(whether weights_out is wanted, weights_in as _weights_array or None) of encounter_pose's `weights`"""
    want = weights is not None and weights is not False
    if want and rate_scale is None:
        raise ValueError("weights need a rate_scale: the rate that leaves a weight as it is")
    return want, _weights_array(weights, n_pairs) if want and weights is not True else None


def _miss_inputs(xyz_a, xyz_b, idx_a, idx_b, pose_b, weights, layout):
    """(columns, w, pose_b) of miss_distance's arguments, checked before torch.cuda is touched"""
    import torch
    columns = _pair_columns(xyz_a, xyz_b, idx_a, idx_b, layout)
    w = None if weights is None else _weights_array(weights, columns[3])
    if pose_b is not None:
        pose_b = np.ascontiguousarray(pose_b, dtype=np.float64) if not isinstance(pose_b, torch.Tensor) else pose_b
        if tuple(pose_b.shape) != (5, columns[3]):
            raise ValueError("pose_b must be [5, n_pairs] (make_pose)")
    return columns, w, pose_b


def miss_distance(xyz_a, xyz_b, idx_a=None, idx_b=None, pose_b=None, weights=None, nmac_h_ft=500.0, nmac_v_ft=100.0, layout="rows", ctx=None,
                  stream=None):
    """Horizontal / vertical miss distance, time of closest approach and NMAC flags of paired 1 Hz tracks on the GPU
    (emgpu_miss_distance_device; the definition is in include/emgpu.h: CorTerminalModel.m:117-133, track.m:175).  xyz_a / xyz_b: numpy
    arrays [n, P, 3] in feet (layout "rows", what sample2track_host and a track file hold) or [P, 3, n] ("planar"), or torch tensors in
    that layout, on the device or not; both sets hold the same P points.  Torch does the plumbing: the upload, the transposition to
    PLANAR on the device, the outputs.  idx_a / idx_b: integer arrays, one column per pair; without idx_x pair i takes column i of set X,
    or column 0 of a set of one (one ownship against every intruder); the number of pairs is the longest of what is given.  pose_b:
    [5, n_pairs] float64 from make_pose.  weights: integers [n_pairs] in 0 .. 2**32 - 1 (quantize_weights), ValueError otherwise; they
    enter totals[5:8] only.
    Returns {"hmd_ft", "vmd_ft" float64, "t_cpa" int32, "flags" uint8 (L.MISS_*), "nmac" bool: NMAC at the CPA, "totals" uint64 [8]} as
    numpy arrays; totals[6] / totals[5] is the weighted NMAC rate.
    The kernel runs on `stream` (a raw hipStream_t) or, without one, on torch's current stream.  ctx: a Context whose earlier device
    calls produced the inputs -- its stream is used when it was given one (Context.stream), and when it runs on a stream of its own
    (Context.stream is None) ctx.sync() is called first, so that the inputs are complete."""
    columns, w, pose_b = _miss_inputs(xyz_a, xyz_b, idx_a, idx_b, pose_b, weights, layout)
    with _paired(xyz_a, xyz_b, columns, w, pose_b, layout, ctx, stream) as pr:
        out = _miss_tensors(pr, pr.d_pose, pr.d_w, nmac_h_ft, nmac_v_ft)
    return _miss_dict(*out)


def miss_segments(xyz_a, xyz_b, idx_a=None, idx_b=None, pose_b=None, weights=None, nmac_h_ft=500.0, nmac_v_ft=100.0, layout="rows", ctx=None,
                  stream=None):
    """miss_distance between the seconds (emgpu_miss_segments_device; the definition is in include/emgpu.h): both tracks are read as
    piecewise linear between their 1 Hz points, so the closest approach may lie inside a second and an NMAC that no sample sees is found.
    The arguments are miss_distance's.
    Returns {"hmd_ft", "vmd_ft", "t_cpa_s" float64 (seconds, real-valued), "flags" uint8 (L.MISS_*), "nmac" bool: NMAC at the CPA,
    "nmac_any" bool: NMAC at some point or inside some segment, "between" bool: an NMAC that no whole second shows
    (L.MISS_NMAC_BETWEEN), "totals" uint64 [10]: miss_distance's eight, the number of "between" pairs and the sum of their weights}."""
    columns, w, pose_b = _miss_inputs(xyz_a, xyz_b, idx_a, idx_b, pose_b, weights, layout)
    with _paired(xyz_a, xyz_b, columns, w, pose_b, layout, ctx, stream) as pr:
        out = _miss_segments_tensors(pr, pr.d_pose, pr.d_w, nmac_h_ft, nmac_v_ft)
    return _miss_segments_dict(*out)


def encounter_params(n_pairs, n_a, n_b, points, radius_ft, half_height_ft, seed, first_index=0, max_attempts=16, rate_scale=1.0, ld_a=0, ld_b=0):
    """emgpu_encounter_params: n_pairs pairs of a column of set A (the ownship; n_a columns, pitch ld_a, 0 = n_a) and a column of set B (the
    intruder), an encounter cylinder of radius_ft and half_height_ft around the ownship, the seed and the global index of pair 0;
    rate_scale divides the rate where it is folded into weights_out."""
    p = _pairing(L.EncounterParams(), n_pairs, n_a, n_b, points, ld_a, ld_b)
    p.max_attempts, p.seed, p.first_index = int(max_attempts), int(seed) & (2**64 - 1), int(first_index) & (2**64 - 1)
    p.radius_ft, p.half_height_ft, p.rate_scale = float(radius_ft), float(half_height_ft), float(rate_scale)
    return p


def encounter_pose_device(params, xyz_a, xyz_b, idx_a=0, idx_b=0, weights_in=0, pose=0, rate=0, flags=0, weights_out=0, stream=None):
    """emgpu_encounter_pose_device: asynchronous, raw device pointers (ints, 0 = none; params: encounter_params).  xyz_a / xyz_b f64 PLANAR
    [P, 3, ld] (points 0 and 1 are read), idx_a / idx_b int64 [n_pairs], weights_in uint32 [n_pairs]; pose f64 [5, n_pairs] (what
    miss_distance_device takes as pose_b), rate f64, flags uint8 (L.ENC_*), weights_out uint32 [n_pairs] each.  No context: the current
    device and `stream`, a raw hipStream_t (0: the HIP default stream; None: torch's current stream)."""
    _device_call("encounter_pose_device", (_stream_handle(stream),), params, xyz_a, xyz_b, idx_a, idx_b, weights_in, pose, rate, flags, weights_out)


def encounter_pose(xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a=None, idx_b=None, weights=None, rate_scale=None, first_index=0,
                   max_attempts=16, layout="rows", ctx=None, stream=None):
    """Places each intruder (set B) on the encounter cylinder of radius_ft and half_height_ft around its ownship (set A) on the GPU
    (emgpu_encounter_pose_device; the definition is in include/emgpu.h): a seeded random heading, an entry point where the intruder flies
    into the cylinder, drawn in proportion to the flux through the side and the ends, and the volume the cylinder sweeps per second
    relative to the intruder, in cubic feet per second.  xyz_a / xyz_b, idx_a / idx_b, layout, ctx and stream are miss_distance's; only the
    first two points of each track are read.  Pair i draws from the global index first_index + i, so a call on rows k .. of a set with
    first_index=k gives rows k .. of the call on the whole set.
    weights: integers [n_pairs] in 0 .. 2**32 - 1 (quantize_weights) to fold the rate into; True: fold it into weights of 1.  Either needs
    rate_scale (ValueError without): the weight is floor(w * rate / rate_scale + 0.5), clamped to 2**32 - 1 (L.ENC_SATURATED), so
    rate_scale is the rate that keeps a weight as it is -- ks times a bound on the relative speed is the caller's to give.
    Returns {"pose" float64 [5, n_pairs] (miss_distance's pose_b), "rate" float64, "flags" uint8 (L.ENC_*), "weights" uint32 or None}."""
    columns = _pair_columns(xyz_a, xyz_b, idx_a, idx_b, layout)
    want_weights, w = _encounter_weights(weights, rate_scale, columns[3])
    with _paired(xyz_a, xyz_b, columns, w, None, layout, ctx, stream) as pr:
        pose, *out = _encounter_pose_tensors(pr, want_weights, radius_ft, half_height_ft, seed, rate_scale, first_index, max_attempts)
    return {"pose": _host(pose)[0], **_encounter_dict(*out)}


def _placed_then(place, placed_dict, tensors, as_dict, xyz_a, xyz_b, idx_a, idx_b, weights, rate_scale, nmac_h_ft, nmac_v_ft, layout, ctx, stream):
    """A placement and then `tensors` (_miss_tensors or _miss_segments_tensors) on one stream, the pose and the weights staying on the
    device.  place(pr, want_weights): the device tensors of _encounter_pose_tensors or _cpa_pose_tensors, the pose first and the weights
    last; the dict of `as_dict` plus placed_dict of what the placement wrote beside the pose."""
    columns = _pair_columns(xyz_a, xyz_b, idx_a, idx_b, layout)
    want_weights, w = _encounter_weights(weights, rate_scale, columns[3])
    with _paired(xyz_a, xyz_b, columns, w, None, layout, ctx, stream) as pr:
        pose, *placed = place(pr, want_weights)
        out = tensors(pr, pose, placed[-1], nmac_h_ft, nmac_v_ft)
    return dict(as_dict(*out), **placed_dict(*placed))


def _encounter_then(tensors, as_dict, xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a, idx_b, weights, rate_scale, first_index,
                    max_attempts, nmac_h_ft, nmac_v_ft, layout, ctx, stream):
    """encounter_pose and then `tensors` (_miss_tensors or _miss_segments_tensors) on one stream; the dict of `as_dict` plus the encounter's"""
    return _placed_then(lambda pr, want: _encounter_pose_tensors(pr, want, radius_ft, half_height_ft, seed, rate_scale, first_index, max_attempts),
                        lambda *placed: _encounter_dict(*placed, "encounter_flags"), tensors, as_dict, xyz_a, xyz_b, idx_a, idx_b, weights,
                        rate_scale, nmac_h_ft, nmac_v_ft, layout, ctx, stream)


def encounter_miss(xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a=None, idx_b=None, weights=None, rate_scale=None, first_index=0,
                   max_attempts=16, nmac_h_ft=500.0, nmac_v_ft=100.0, layout="rows", ctx=None, stream=None):
    """encounter_pose and then miss_distance on one stream, the pose and the rate-folded weights never leaving the device: the intruders
    placed on the encounter cylinder, then HMD, VMD, CPA time and NMAC flags of the pairs.  The arguments are encounter_pose's and the
    NMAC thresholds.  With weights (and rate_scale) totals[5:8] are sums of w * rate / rate_scale, so totals[6] / totals[5] is
    P(NMAC | encounter); without, every pair counts 1 there.
    Returns miss_distance's dict plus "rate" float64, "encounter_flags" uint8 (L.ENC_*) and "weights" uint32 or None."""
    return _encounter_then(_miss_tensors, _miss_dict, xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a, idx_b, weights, rate_scale,
                           first_index, max_attempts, nmac_h_ft, nmac_v_ft, layout, ctx, stream)


def encounter_miss_segments(xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a=None, idx_b=None, weights=None, rate_scale=None, first_index=0,
                            max_attempts=16, nmac_h_ft=500.0, nmac_v_ft=100.0, layout="rows", ctx=None, stream=None):
    """encounter_miss with miss_segments in the place of miss_distance: the pose and the rate-folded weights stay on the device, and
    totals[6] / totals[5] is P(NMAC | encounter) with the closest approach found between the seconds.  The arguments are encounter_miss's.
    Returns miss_segments' dict plus "rate" float64, "encounter_flags" uint8 (L.ENC_*) and "weights" uint32 or None."""
    return _encounter_then(_miss_segments_tensors, _miss_segments_dict, xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a, idx_b, weights,
                           rate_scale, first_index, max_attempts, nmac_h_ft, nmac_v_ft, layout, ctx, stream)


def cpa_pose_params(n_pairs, n_a, n_b, points, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi=None, first_index=0, max_attempts=16, rate_scale=1.0,
                    ld_a=0, ld_b=0):
    """emgpu_cpa_pose_params: n_pairs pairs of a column of set A (the ownship; n_a columns, pitch ld_a, 0 = n_a) and a column of set B (the
    intruder), a miss plane of +-hmd_max_ft by +-vmd_max_ft, the seconds t_lo .. t_hi (None: t_lo alone) the pass is drawn from, the seed
    and the global index of pair 0; rate_scale divides the rate where it is folded into weights_out."""
    p = _pairing(L.CpaPoseParams(), n_pairs, n_a, n_b, points, ld_a, ld_b)
    p.max_attempts, p.seed, p.first_index = int(max_attempts), int(seed) & (2**64 - 1), int(first_index) & (2**64 - 1)
    p.t_lo, p.t_hi = int(t_lo), int(t_lo if t_hi is None else t_hi)
    p.hmd_max_ft, p.vmd_max_ft, p.rate_scale = float(hmd_max_ft), float(vmd_max_ft), float(rate_scale)
    return p


def cpa_pose_device(params, xyz_a, xyz_b, idx_a=0, idx_b=0, weights_in=0, pose=0, rate=0, t_cpa=0, flags=0, weights_out=0, stream=None):
    """emgpu_cpa_pose_device: asynchronous, raw device pointers (ints, 0 = none; params: cpa_pose_params).  xyz_a / xyz_b f64 PLANAR
    [P, 3, ld] (points tc and tc + 1 are read), idx_a / idx_b int64 [n_pairs], weights_in uint32 [n_pairs]; pose f64 [5, n_pairs] (what
    miss_distance_device takes as pose_b), rate f64, t_cpa int32 (the drawn second), flags uint8 (L.CPA_*), weights_out uint32 [n_pairs]
    each.  No context: the current device and `stream`, a raw hipStream_t (0: the HIP default stream; None: torch's current stream)."""
    _device_call("cpa_pose_device", (_stream_handle(stream),), params, xyz_a, xyz_b, idx_a, idx_b, weights_in, pose, rate, t_cpa, flags, weights_out)


def _cpa_pose_tensors(pr, want_weights, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi, rate_scale, first_index, max_attempts):
    """k_cpa_pose on the pairing pr: the device tensors (pose [5, n_pairs], rate, t_cpa, flags, weights or None), launched on pr.stream and
    not waited for"""
    p = cpa_pose_params(*pr.sizes, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi, first_index, max_attempts, 1.0 if rate_scale is None else rate_scale)
    return _launch(pr, cpa_pose_device, p, (pr.d_w,), _placement(want_weights, t_cpa="int32"))


def _cpa_dict(rate, t_cpa, flags, w_out, t_key="t_cpa", flags_key="flags"):
    """the rate, drawn second, flags and weights of cpa_pose's dict from _cpa_pose_tensors' device tensors"""
    return {t_key: _host(t_cpa)[0], **_encounter_dict(rate, flags, w_out, flags_key)}


def cpa_pose(xyz_a, xyz_b, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi=None, idx_a=None, idx_b=None, weights=None, rate_scale=None, first_index=0,
             max_attempts=16, layout="rows", ctx=None, stream=None):
    """Places each intruder (set B) by its closest approach to its ownship (set A) on the GPU (emgpu_cpa_pose_device; the definition is in
    include/emgpu.h): a seeded random heading, a second drawn from t_lo .. t_hi (t_hi=None: t_lo) at which the two pass, a lateral miss
    drawn uniformly within +-hmd_max_ft and a vertical offset within +-vmd_max_ft, and the pose with which, both flying on as they do in
    that second, the pass happens exactly so.  "rate" is the flux through that miss plane, (2 hmd_max_ft)(2 vmd_max_ft) times the relative
    horizontal speed, in cubic feet per second: it plays the part of encounter_pose's rate, and every placed pair passes close by, which is
    what a rare-event estimate wants.  xyz_a / xyz_b, idx_a / idx_b, layout, ctx and stream are miss_distance's; t_hi <= P - 2.  weights,
    rate_scale and first_index are encounter_pose's.
    Returns {"pose" float64 [5, n_pairs] (miss_distance's pose_b), "rate" float64, "t_cpa" int32 (the drawn second), "flags" uint8
    (L.CPA_*), "weights" uint32 or None}."""
    columns = _pair_columns(xyz_a, xyz_b, idx_a, idx_b, layout)
    want_weights, w = _encounter_weights(weights, rate_scale, columns[3])
    with _paired(xyz_a, xyz_b, columns, w, None, layout, ctx, stream) as pr:
        pose, *out = _cpa_pose_tensors(pr, want_weights, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi, rate_scale, first_index, max_attempts)
    return {"pose": _host(pose)[0], **_cpa_dict(*out)}


def _cpa_then(tensors, as_dict, xyz_a, xyz_b, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi, idx_a, idx_b, weights, rate_scale, first_index,
              max_attempts, nmac_h_ft, nmac_v_ft, layout, ctx, stream):
    """cpa_pose and then `tensors` on one stream; the dict of `as_dict` plus the placement's, the drawn second under "t_cpa_drawn" """
    return _placed_then(lambda pr, want: _cpa_pose_tensors(pr, want, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi, rate_scale, first_index, max_attempts),
                        lambda *placed: _cpa_dict(*placed, "t_cpa_drawn", "encounter_flags"), tensors, as_dict, xyz_a, xyz_b, idx_a, idx_b,
                        weights, rate_scale, nmac_h_ft, nmac_v_ft, layout, ctx, stream)


def cpa_miss(xyz_a, xyz_b, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi=None, idx_a=None, idx_b=None, weights=None, rate_scale=None, first_index=0,
             max_attempts=16, nmac_h_ft=500.0, nmac_v_ft=100.0, layout="rows", ctx=None, stream=None):
    """cpa_pose and then miss_distance on one stream, the pose and the rate-folded weights never leaving the device.  The arguments are
    cpa_pose's and the NMAC thresholds.  On straight tracks the miss distance found is the one drawn; on tracks that turn it is what the
    tracks make of that pass.  Returns miss_distance's dict plus "rate" float64, "t_cpa_drawn" int32, "encounter_flags" uint8 (L.CPA_*)
    and "weights" uint32 or None."""
    return _cpa_then(_miss_tensors, _miss_dict, xyz_a, xyz_b, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi, idx_a, idx_b, weights, rate_scale,
                     first_index, max_attempts, nmac_h_ft, nmac_v_ft, layout, ctx, stream)


def cpa_miss_segments(xyz_a, xyz_b, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi=None, idx_a=None, idx_b=None, weights=None, rate_scale=None,
                      first_index=0, max_attempts=16, nmac_h_ft=500.0, nmac_v_ft=100.0, layout="rows", ctx=None, stream=None):
    """cpa_miss with miss_segments in the place of miss_distance.  Returns miss_segments' dict plus "rate", "t_cpa_drawn",
    "encounter_flags" and "weights"."""
    return _cpa_then(_miss_segments_tensors, _miss_segments_dict, xyz_a, xyz_b, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi, idx_a, idx_b, weights,
                     rate_scale, first_index, max_attempts, nmac_h_ft, nmac_v_ft, layout, ctx, stream)


def well_clear_params(n_pairs, n_a, n_b, points, tau_s=35.0, dmod_ft=4000.0, hmd_ft=4000.0, h_ft=450.0, ld_a=0, ld_b=0):
    """emgpu_well_clear_params: miss_params' pairing and the four thresholds of DAA well clear: modified tau in seconds, DMOD, the predicted
    horizontal miss and the vertical separation in feet."""
    p = _pairing(L.WellClearParams(), n_pairs, n_a, n_b, points, ld_a, ld_b)
    p.tau_s, p.dmod_ft, p.hmd_ft, p.h_ft = float(tau_s), float(dmod_ft), float(hmd_ft), float(h_ft)
    return p


def well_clear_device(params, xyz_a, xyz_b, idx_a=0, idx_b=0, pose_b=0, weights=0, miss_flags=0, t_first=0, n_lost=0, tau_min=0, flags=0,
                      totals=0, stream=None):
    """emgpu_well_clear_device: asynchronous, raw device pointers (ints, 0 = none; params: well_clear_params).  The inputs are
    miss_distance_device's and miss_flags uint8 [n_pairs], the flags either miss kernel wrote for the same pairs (L.MISS_NMAC_ANY is
    read); t_first / n_lost int32, tau_min f64, flags uint8 (L.WC_*) [n_pairs] each, totals uint64 [10], ADDED to.  No context: the
    current device and `stream`, a raw hipStream_t (0: the HIP default stream; None: torch's current stream)."""
    _device_call("well_clear_device", (_stream_handle(stream),), params, xyz_a, xyz_b, idx_a, idx_b, pose_b, weights, miss_flags, t_first, n_lost,
                 tau_min, flags, totals)


def _well_clear_tensors(pr, d_pose, d_w, d_miss_flags, tau_s, dmod_ft, hmd_ft, h_ft):
    """k_well_clear on the pairing pr with the device tensors d_pose, d_w and d_miss_flags (or None): the device tensors (t_first, n_lost,
    tau_min, flags, totals [10]), launched on pr.stream and not waited for"""
    return _launch(pr, well_clear_device, well_clear_params(*pr.sizes, tau_s, dmod_ft, hmd_ft, h_ft), (d_pose, d_w, d_miss_flags),
                   {"t_first": "int32", "n_lost": "int32", "tau_min": "float64", "flags": "uint8"}, 10)


def _well_clear_dict(t_first, n_lost, tau_min, flags, totals, flags_key="flags", totals_key="totals"):
    """well_clear's dict from _well_clear_tensors' device tensors"""
    t_first, n_lost, tau_min, fl, tot = _host(t_first, n_lost, tau_min, flags, totals)
    return {"t_first": t_first, "n_lost": n_lost, "tau_min_s": tau_min, flags_key: fl, "lowc": (fl & L.WC_LOST) != 0,
            "at_start": (fl & L.WC_AT_START) != 0, totals_key: tot.view(np.uint64)}


def well_clear(xyz_a, xyz_b, idx_a=None, idx_b=None, pose_b=None, weights=None, miss_flags=None, tau_s=35.0, dmod_ft=4000.0, hmd_ft=4000.0,
               h_ft=450.0, layout="rows", ctx=None, stream=None):
    """Loss of DAA well clear of paired 1 Hz tracks on the GPU (emgpu_well_clear_device; the definition is in include/emgpu.h): at every
    whole second the pair has lost well clear when it is within h_ft vertically and horizontally either inside dmod_ft or closing with a
    modified tau of at most tau_s and a predicted horizontal miss of at most hmd_ft.  xyz_a / xyz_b, idx_a / idx_b, pose_b, weights,
    layout, ctx and stream are miss_distance's.  miss_flags: the "flags" of miss_distance or miss_segments for the same pairs (uint8
    [n_pairs], a numpy array or a torch tensor), which lets totals[8:10] count the NMACs among the losses.
    Returns {"t_first" int32: the first second of the loss, -1 without one, "n_lost" int32: the number of such seconds, "tau_min_s"
    float64: the smallest modified tau, "flags" uint8 (L.WC_*), "lowc" bool, "at_start" bool: lost at second 0, which a study has to
    exclude, "totals" uint64 [10]}; totals[6] / totals[5] is the weighted P(LoWC), (totals[6] - totals[7]) / (totals[5] - totals[7])
    the same over the pairs that did not start inside the volume, totals[9] / totals[6] P(NMAC | LoWC)."""
    import torch
    columns, w, pose_b = _miss_inputs(xyz_a, xyz_b, idx_a, idx_b, pose_b, weights, layout)
    if miss_flags is not None:
        if not isinstance(miss_flags, torch.Tensor):
            miss_flags = np.ascontiguousarray(miss_flags)
        if tuple(miss_flags.shape) != (columns[3],) or miss_flags.dtype != (torch.uint8 if isinstance(miss_flags, torch.Tensor) else np.uint8):
            raise ValueError("miss_flags must be uint8 [n_pairs]: the flags of miss_distance or miss_segments")
    with _paired(xyz_a, xyz_b, columns, w, pose_b, layout, ctx, stream) as pr:
        d_mf = None if miss_flags is None else (miss_flags if isinstance(miss_flags, torch.Tensor) else torch.from_numpy(miss_flags.copy()))
        d_mf = None if d_mf is None else d_mf.to(pr.dev).contiguous()
        out = _well_clear_tensors(pr, pr.d_pose, pr.d_w, d_mf, tau_s, dmod_ft, hmd_ft, h_ft)
    return _well_clear_dict(*out)


def _miss_then_well_clear(between, tau_s, dmod_ft, hmd_ft, h_ft):
    """(tensors, as_dict) for _placed_then: a miss kernel (k_miss_segments where `between`) and then k_well_clear on the same pose and
    weights, the miss kernel's flags handed over on the device; the miss dict plus well_clear's, its flags under "wc_flags" and its
    totals under "wc_totals" """
    miss_tensors, miss_dict = (_miss_segments_tensors, _miss_segments_dict) if between else (_miss_tensors, _miss_dict)

    def tensors(pr, d_pose, d_w, nmac_h_ft, nmac_v_ft):
        miss = miss_tensors(pr, d_pose, d_w, nmac_h_ft, nmac_v_ft)
        return tuple(miss) + tuple(_well_clear_tensors(pr, d_pose, d_w, miss[3], tau_s, dmod_ft, hmd_ft, h_ft))

    def as_dict(*out):
        return dict(miss_dict(*out[:5]), **_well_clear_dict(*out[5:], flags_key="wc_flags", totals_key="wc_totals"))
    return tensors, as_dict


def encounter_well_clear(xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a=None, idx_b=None, weights=None, rate_scale=None, first_index=0,
                         max_attempts=16, nmac_h_ft=500.0, nmac_v_ft=100.0, between=False, tau_s=35.0, dmod_ft=4000.0, hmd_ft=4000.0,
                         h_ft=450.0, layout="rows", ctx=None, stream=None):
    """encounter_miss (between=True: encounter_miss_segments) and then well_clear on one stream: the intruders placed on the encounter
    cylinder, the NMAC and the loss of well clear of the pairs, the pose, the rate-folded weights and the miss kernel's flags never
    leaving the device.  The arguments are encounter_miss's and well_clear's thresholds.  Returns encounter_miss's dict plus "t_first",
    "n_lost", "tau_min_s", "wc_flags" (L.WC_*), "lowc", "at_start" and "wc_totals" uint64 [10]: wc_totals[6] / wc_totals[5] is
    P(LoWC | encounter), wc_totals[9] / wc_totals[6] P(NMAC | LoWC).  A cylinder smaller than the well-clear volume places intruders
    inside it: "at_start" names them."""
    tensors, as_dict = _miss_then_well_clear(between, tau_s, dmod_ft, hmd_ft, h_ft)
    return _encounter_then(tensors, as_dict, xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a, idx_b, weights, rate_scale, first_index,
                           max_attempts, nmac_h_ft, nmac_v_ft, layout, ctx, stream)


def cpa_well_clear(xyz_a, xyz_b, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi=None, idx_a=None, idx_b=None, weights=None, rate_scale=None,
                   first_index=0, max_attempts=16, nmac_h_ft=500.0, nmac_v_ft=100.0, between=False, tau_s=35.0, dmod_ft=4000.0, hmd_ft=4000.0,
                   h_ft=450.0, layout="rows", ctx=None, stream=None):
    """cpa_miss (between=True: cpa_miss_segments) and then well_clear on one stream, as encounter_well_clear.  Returns cpa_miss's dict plus
    "t_first", "n_lost", "tau_min_s", "wc_flags", "lowc", "at_start" and "wc_totals"."""
    tensors, as_dict = _miss_then_well_clear(between, tau_s, dmod_ft, hmd_ft, h_ft)
    return _cpa_then(tensors, as_dict, xyz_a, xyz_b, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi, idx_a, idx_b, weights, rate_scale, first_index,
                     max_attempts, nmac_h_ft, nmac_v_ft, layout, ctx, stream)


def avoid_params(n_pairs, n_a, n_b, points, alert_tau_s=60.0, alert_dmod_ft=4000.0, alert_hmd_ft=4000.0, alert_h_ft=700.0, nmac_h_ft=500.0,
                 nmac_v_ft=100.0, delay_s=5, rate_fps=25.0, accel_fps2=8.0, dz_max_ft=float("inf"), ld_a=0, ld_b=0):
    """emgpu_avoid_params: miss_params' pairing; the alert volume (well_clear's four thresholds, with values of their own); the NMAC
    thresholds; the ownship's response: the whole seconds between the alert and the manoeuvre, the vertical rate it reaches in ft/s, the
    acceleration towards it in ft/s^2 (inf: at once) and the largest displacement in feet.  The defaults are an illustration (1500 ft/min
    after 5 s at about 0.25 g), not the alerting thresholds of any standard."""
    p = _pairing(L.AvoidParams(), n_pairs, n_a, n_b, points, ld_a, ld_b)
    p.delay_s = int(delay_s)
    p.alert_tau_s, p.alert_dmod_ft, p.alert_hmd_ft, p.alert_h_ft = float(alert_tau_s), float(alert_dmod_ft), float(alert_hmd_ft), float(alert_h_ft)
    p.nmac_h_ft, p.nmac_v_ft = float(nmac_h_ft), float(nmac_v_ft)
    p.rate_fps, p.accel_fps2, p.dz_max_ft = float(rate_fps), float(accel_fps2), float(dz_max_ft)
    return p


def avoid_device(params, xyz_a, xyz_b, idx_a=0, idx_b=0, pose_b=0, weights=0, hmd=0, vmd=0, vmd_mit=0, t_cpa=0, t_alert=0, flags=0, totals=0,
                 stream=None):
    """emgpu_avoid_device: asynchronous, raw device pointers (ints, 0 = none; params: avoid_params).  The inputs are
    miss_distance_device's; hmd / vmd / vmd_mit f64, t_cpa / t_alert int32, flags uint8 (L.AVOID_*) [n_pairs] each, totals uint64 [12],
    ADDED to.  No context: the current device and `stream`, a raw hipStream_t (0: the HIP default stream; None: torch's current stream)."""
    _device_call("avoid_device", (_stream_handle(stream),), params, xyz_a, xyz_b, idx_a, idx_b, pose_b, weights, hmd, vmd, vmd_mit, t_cpa, t_alert,
                 flags, totals)


def _avoid_tensors(pr, d_pose, d_w, **response):
    """k_avoid on the pairing pr with the device tensors d_pose and d_w (or None) and avoid_params' thresholds and response: the device
    tensors (hmd, vmd, vmd_mit, t_cpa, t_alert, flags, totals [12]), launched on pr.stream and not waited for"""
    return _launch(pr, avoid_device, avoid_params(*pr.sizes, **response), (d_pose, d_w),
                   {"hmd": "float64", "vmd": "float64", "vmd_mit": "float64", "t_cpa": "int32", "t_alert": "int32", "flags": "uint8"}, 12)


def _avoid_dict(hmd, vmd, vmd_mit, t_cpa, t_alert, flags, totals):
    """avoid's dict from _avoid_tensors' device tensors"""
    hmd, vmd, vmd_mit, t_cpa, t_alert, fl, tot = _host(hmd, vmd, vmd_mit, t_cpa, t_alert, flags, totals)
    tot, nmac, nmac_mit = tot.view(np.uint64), (fl & L.AVOID_NMAC_UNMIT) != 0, (fl & L.AVOID_NMAC_MIT) != 0
    return {"hmd_ft": hmd, "vmd_ft": vmd, "vmd_mit_ft": vmd_mit, "t_cpa": t_cpa, "t_alert": t_alert, "flags": fl,
            "alerted": (fl & L.AVOID_ALERTED) != 0, "climb": (fl & L.AVOID_CLIMB) != 0, "nmac": nmac, "nmac_mit": nmac_mit,
            "induced": nmac_mit & ~nmac, "totals": tot, "risk_ratio": float(tot[10]) / float(tot[9]) if tot[9] else float("nan")}


def avoid(xyz_a, xyz_b, idx_a=None, idx_b=None, pose_b=None, weights=None, alert_tau_s=60.0, alert_dmod_ft=4000.0, alert_hmd_ft=4000.0,
          alert_h_ft=700.0, nmac_h_ft=500.0, nmac_v_ft=100.0, delay_s=5, rate_fps=25.0, accel_fps2=8.0, dz_max_ft=float("inf"), layout="rows",
          ctx=None, stream=None):
    """The ownship's vertical avoidance manoeuvre on paired 1 Hz tracks on the GPU (emgpu_avoid_device; the definition is in
    include/emgpu.h): set A is the ownship, set B the intruder.  The first second at which the pair is inside the alert volume
    (well_clear's predicate with alert_tau_s, alert_dmod_ft, alert_hmd_ft, alert_h_ft) alerts the ownship; it picks the sense that moves it
    away from where the intruder will be at the horizontal closest approach, and delay_s seconds later accelerates with accel_fps2 (inf: at
    once) to the vertical rate rate_fps, up to dz_max_ft feet.  The intruder flies on as it did.  The defaults are an illustration, not
    the alerting thresholds of any standard.  xyz_a / xyz_b, idx_a / idx_b, pose_b, weights, layout, ctx and stream are miss_distance's.
    Returns {"hmd_ft", "vmd_ft" float64, "t_cpa" int32: miss_distance's, "vmd_mit_ft" float64: the vertical miss at that second with the
    manoeuvre, "t_alert" int32: the alert's second, -1 without one, "flags" uint8 (L.AVOID_*), "alerted", "climb", "nmac": an NMAC at some
    second without the manoeuvre, "nmac_mit": with it, "induced": with it only (bool each), "totals" uint64 [12], "risk_ratio":
    totals[10] / totals[9], the weighted P(NMAC with the manoeuvre) / P(NMAC without), NaN when totals[9] is 0}."""
    columns, w, pose_b = _miss_inputs(xyz_a, xyz_b, idx_a, idx_b, pose_b, weights, layout)
    with _paired(xyz_a, xyz_b, columns, w, pose_b, layout, ctx, stream) as pr:
        out = _avoid_tensors(pr, pr.d_pose, pr.d_w, alert_tau_s=alert_tau_s, alert_dmod_ft=alert_dmod_ft, alert_hmd_ft=alert_hmd_ft,
                             alert_h_ft=alert_h_ft, nmac_h_ft=nmac_h_ft, nmac_v_ft=nmac_v_ft, delay_s=delay_s, rate_fps=rate_fps,
                             accel_fps2=accel_fps2, dz_max_ft=dz_max_ft)
    return _avoid_dict(*out)


def _avoid_after(**response):
    """`tensors` for _placed_then: k_avoid on the placement's pose and weights, with the NMAC thresholds _placed_then hands over"""
    return lambda pr, d_pose, d_w, nmac_h_ft, nmac_v_ft: _avoid_tensors(pr, d_pose, d_w, nmac_h_ft=nmac_h_ft, nmac_v_ft=nmac_v_ft, **response)


def encounter_avoid(xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a=None, idx_b=None, weights=None, rate_scale=None, first_index=0,
                    max_attempts=16, alert_tau_s=60.0, alert_dmod_ft=4000.0, alert_hmd_ft=4000.0, alert_h_ft=700.0, nmac_h_ft=500.0,
                    nmac_v_ft=100.0, delay_s=5, rate_fps=25.0, accel_fps2=8.0, dz_max_ft=float("inf"), layout="rows", ctx=None, stream=None):
    """encounter_pose and then avoid on one stream, the pose and the rate-folded weights never leaving the device: the intruders placed on
    the encounter cylinder, then the ownship's alert and manoeuvre.  The arguments are encounter_pose's and avoid's thresholds and
    response.  With weights (and rate_scale) totals[7:12] are sums of w * rate / rate_scale, so "risk_ratio" is that of the encounters.
    Returns avoid's dict plus "rate" float64, "encounter_flags" uint8 (L.ENC_*) and "weights" uint32 or None."""
    tensors = _avoid_after(alert_tau_s=alert_tau_s, alert_dmod_ft=alert_dmod_ft, alert_hmd_ft=alert_hmd_ft, alert_h_ft=alert_h_ft,
                           delay_s=delay_s, rate_fps=rate_fps, accel_fps2=accel_fps2, dz_max_ft=dz_max_ft)
    return _encounter_then(tensors, _avoid_dict, xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a, idx_b, weights, rate_scale, first_index,
                           max_attempts, nmac_h_ft, nmac_v_ft, layout, ctx, stream)


def cpa_avoid(xyz_a, xyz_b, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi=None, idx_a=None, idx_b=None, weights=None, rate_scale=None, first_index=0,
              max_attempts=16, alert_tau_s=60.0, alert_dmod_ft=4000.0, alert_hmd_ft=4000.0, alert_h_ft=700.0, nmac_h_ft=500.0, nmac_v_ft=100.0,
              delay_s=5, rate_fps=25.0, accel_fps2=8.0, dz_max_ft=float("inf"), layout="rows", ctx=None, stream=None):
    """cpa_pose and then avoid on one stream, as encounter_avoid: every placed pair passes close by, which is what a risk ratio wants.  The
    arguments are cpa_pose's and avoid's thresholds and response.  Returns avoid's dict plus "rate" float64, "t_cpa_drawn" int32,
    "encounter_flags" uint8 (L.CPA_*) and "weights" uint32 or None."""
    tensors = _avoid_after(alert_tau_s=alert_tau_s, alert_dmod_ft=alert_dmod_ft, alert_hmd_ft=alert_hmd_ft, alert_h_ft=alert_h_ft,
                           delay_s=delay_s, rate_fps=rate_fps, accel_fps2=accel_fps2, dz_max_ft=dz_max_ft)
    return _cpa_then(tensors, _avoid_dict, xyz_a, xyz_b, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi, idx_a, idx_b, weights, rate_scale, first_index,
                     max_attempts, nmac_h_ft, nmac_v_ft, layout, ctx, stream)
