"""What is done to a trace: score it, count it (weighted or not), discretize its values, derive its values from tracks -- each from host
arrays or where it lies on the device -- and the pipelines that chain these steps in one device block."""
import contextlib
import ctypes as C
import types

import numpy as np

from .. import _lib as L
from .base import _device_arrays, _device_call, _p, _raise, _weights_array, device_download, device_upload, make_params
from .layout import TraceLayout, pack_dyn_bin, pack_dyn_val, unpack_dyn_bin, unpack_dyn_val
from .sampling import _same_shape, sample_dbn_device


def score_params(n, sample_time, transition_mode=L.TRANSITION_REFERENCE_AUTO, ld=0, col_offset=0):
    p = L.ScoreParams()
    p.n, p.sample_time, p.transition_mode, p.ld, p.col_offset = int(n), int(sample_time), int(transition_mode), int(ld), int(col_offset)
    return p


def score_dbn_device(ctx, model, params, init_bin, dyn_bin=0, log_lik=0, initial=0):
    """emgpu_score_dbn_device: asynchronous, raw device pointers (ints; dyn_bin 0 for sample_time 1 or a model without a transition network,
    initial 0 = not wanted).  log_lik / initial [n] f64 are not offset by col_offset.  A bin outside 1..r makes its trajectory NaN and the
    next ctx.sync() raise EmgpuError(ERR_ARG)."""
    _device_call("score_dbn_device", (ctx, model), params, init_bin, dyn_bin, log_lik, initial)


def _bin_arrays(model, init_bin, dyn_bin, T, raw, n, col_offset):
    """(init_bin [n_i, ld] u8, dyn_bin [G4, n_d, ld] u32 or None, ld, n) of a call's trace of bins, in the library layout (n: default
    ld - col_offset)"""
    if raw:
        ib = np.ascontiguousarray(init_bin, dtype=np.uint8)
        db = None if dyn_bin is None else np.ascontiguousarray(dyn_bin, dtype=np.uint32)
    else:
        ib = np.ascontiguousarray(np.asarray(init_bin, dtype=np.uint8).T)
        db = None if dyn_bin is None else pack_dyn_bin(dyn_bin)
    if ib.ndim != 2 or ib.shape[0] != model.n_initial:
        raise ValueError("init_bin must hold n_initial entries per trajectory")
    ld = ib.shape[1]
    n = ld - int(col_offset) if n is None else int(n)
    if db is not None and db.shape != TraceLayout(model.n_initial, model.n_dyn, ld, T).shape["dyn_bin"]:
        raise ValueError("dyn_bin must hold T columns of n_dyn variables for the trajectories of init_bin")
    return ib, db, ld, n


def score_dbn_host(ctx, model, init_bin, dyn_bin, T, transition_mode=L.TRANSITION_REFERENCE_AUTO, raw=False, n=None, col_offset=0):
    """log P(trajectory | model) of a host trace (emgpu_score_dbn_host; the definition is in include/emgpu.h).  raw=False: the user-facing
    shapes sample_dbn_host returns (init_bin [n, n_i] u8, dyn_bin [n, T, n_d] u8 or None); raw=True: the library layout (init_bin [n_i, ld]
    u8, dyn_bin [G4, n_d, ld] u32), of which columns col_offset .. col_offset + n are scored (n: default ld - col_offset).
    Returns {"log_lik" [n], "initial" [n], "kernel"}.  The rejection loop's normalisation (altitude / speed / layers) is not part of the
    number.  A bin outside 1..r raises EmgpuError(ERR_ARG) carrying .log_lik / .initial (NaN for exactly those trajectories)."""
    ib, db, ld, n = _bin_arrays(model, init_bin, dyn_bin, T, raw, n, col_offset)
    p = score_params(n, T, transition_mode, ld, col_offset)
    ll, ini = np.zeros(max(n, 0), dtype=np.float64), np.zeros(max(n, 0), dtype=np.float64)
    rc = L.lib().emgpu_score_dbn_host(ctx._h, model._h, C.byref(p), _p(ib), _p(db), _p(ll), _p(ini))
    if rc < 0:
        _raise(rc, log_lik=ll, initial=ini)
    return {"log_lik": ll, "initial": ini, "kernel": ctx.last_kernel()}


def count_dbn_device(ctx, model, params, init_bin, dyn_bin=0, counts_initial=0, counts_transition=0):
    """emgpu_count_dbn_device: asynchronous, raw device pointers (ints; params: score_params).  counts_initial / counts_transition are uint64
    arrays in the layout of model.count_layout(network), which the call ADDS to (the caller zeroes them); 0 = that network is not counted.
    An observation that reads a bin outside 1..r is skipped, and the next ctx.sync() raises EmgpuError(ERR_ARG)."""
    _device_call("count_dbn_device", (ctx, model), params, init_bin, dyn_bin, counts_initial, counts_transition)


def split_counts(model, raw):
    """(u64 initial array, u64 transition array) in the library's layout -> (N_initial, N_transition): one [r, q] float64 per variable, (0, 0)
    for a transition node without a table -- what NativeModel.from_arrays and EncounterModel.setParameters take.  Exact below 2**53."""
    out = []
    for network, a in enumerate(raw):
        off = model.count_layout(network).tolist()
        r = model.get_i32(L.F_R_TRANSITION if network else L.F_R_INITIAL)
        out.append([a[s:e].astype(np.float64).reshape(-1, int(r[v])).T.copy() if e > s else np.zeros((0, 0))
                    for v, (s, e) in enumerate(zip(off[:-1], off[1:]))])
    return out[0], out[1]


def _counts_arrays(model, counts):
    """the two u64 arrays of a call: fresh zeros, or a previous result's `raw` (accumulated into, in place)"""
    return _raw_pair(counts, [int(model.count_layout(network)[-1]) for network in (0, 1)],
                     "counts must be the `raw` pair of a count of this model: contiguous uint64 arrays of count_layout's lengths")


def _raw_pair(counts, sizes, complaint):
    """a previous result's `raw` pair (checked: two contiguous uint64 arrays of these sizes), or fresh zeros"""
    if counts is None:
        return [np.zeros(max(s, 1), dtype=np.uint64)[:s] for s in sizes]
    a, b = counts
    for x, s in ((a, sizes[0]), (b, sizes[1])):
        if not isinstance(x, np.ndarray) or x.dtype != np.uint64 or x.shape != (s,) or not x.flags["C_CONTIGUOUS"]:
            raise ValueError(complaint)
    return [a, b]


def _counts_result(model, ci, ct, pairs=None, **kernels):
    """the dict the counting calls return: the tables of the u64 arrays ci / ct, the two vectors of pairs = (u64 repeat, u64 change) where
    the call has them, and the kernels' names"""
    Ni, Nt = split_counts(model, (ci, ct))
    out = {"N_initial": Ni, "N_transition": Nt, "raw": (ci, ct)}
    if pairs is not None:
        out.update({"repeat": pairs[0].astype(np.float64), "change": pairs[1].astype(np.float64), "raw_pairs": pairs})
    out.update(kernels)
    return out


def count_dbn_host(ctx, model, init_bin, dyn_bin, T, transition_mode=L.TRANSITION_REFERENCE_AUTO, raw=False, n=None, col_offset=0, counts=None):
    """The sufficient statistics of a host trace (emgpu_count_dbn_host; the definition is in include/emgpu.h): how often every cell of the
    model's N_initial / N_transition was observed.  The trace is given as to score_dbn_host (raw=False: init_bin [n, n_i] u8, dyn_bin
    [n, T, n_d] u8 or None; raw=True: the library layout and its window n / col_offset).
    Returns {"N_initial": [r x q float64 per variable], "N_transition": [per node, (0, 0) where no table], "raw": (u64 initial, u64
    transition), "kernel"}.  counts=<a previous result's raw> accumulates into those arrays.  dyn_bin None counts the initial network alone.
    A bin outside 1..r skips the observations that read it and raises EmgpuError(ERR_ARG) carrying .counts (the same dict)."""
    return _count_host(ctx, model, init_bin, dyn_bin, T, None, transition_mode, raw, n, col_offset, counts)


def _count_host(ctx, model, init_bin, dyn_bin, T, weights, transition_mode, raw, n, col_offset, counts):
    """count_dbn_host (weights None) and count_dbn_weighted_host: the weights choose the entry point, which takes them before the counts"""
    ib, db, ld, n = _bin_arrays(model, init_bin, dyn_bin, T, raw, n, col_offset)
    w = None if weights is None else _weights_array(weights, n)
    ci, ct = _counts_arrays(model, counts)
    p = score_params(n, T, transition_mode, ld, col_offset)
    transitions = db is not None and int(T) > 1 and model.n_dyn > 0
    entry, w_arg = (L.lib().emgpu_count_dbn_host, ()) if w is None else (L.lib().emgpu_count_dbn_weighted_host, (_p(w),))
    rc = entry(ctx._h, model._h, C.byref(p), _p(ib), _p(db), *w_arg, _p(ci), _p(ct) if transitions else None)
    out = _counts_result(model, ci, ct, kernel=ctx.last_kernel())
    if rc < 0:
        _raise(rc, counts=out)
    return out


def _count_bytes(model, pairs=False):
    """the entries of a _device_arrays block that _count_scope counts into: the model's two tables and, with pairs, the two vectors"""
    return dict(ci=8 * int(model.count_layout(0)[-1]), ct=8 * int(model.count_layout(1)[-1]), rc=16 * model.n_initial if pairs else 0)


@contextlib.contextmanager
def _count_scope(ctx, model, at, counts=None, pairs=False):
    """The one on-device count, in a _device_arrays block `at` that has _count_bytes' entries: the tables at at["ci"] / at["ct"] (pairs: and
    the repeat / change vectors at at["rc"], 2 n_initial u64) are zeroed for the body's launches to add to.  The body puts the kernels'
    names into cs.kernels and clears cs.counted where it launched nothing into the tables.  Leaving it waits for the launches (ctx.sync():
    their deferred errors), downloads the tables, adds them into the caller's `raw` arrays (counts; default: fresh zeros) and leaves the
    counting calls' dict (_counts_result) in cs.result."""
    ci, ct = _counts_arrays(model, counts)
    rc = np.zeros(2 * model.n_initial if pairs else 0, dtype=np.uint64)
    tables = [(k, a) for k, a in (("ci", ci), ("ct", ct), ("rc", rc)) if a.size]
    for k, a in tables:
        device_upload(ctx, at[k], np.zeros_like(a))
    cs = types.SimpleNamespace(kernels={}, counted=True, result=None)
    yield cs
    if cs.counted:
        ctx.sync()                                  # the launches' deferred errors
        for k, a in tables:
            a += device_download(ctx, at[k], np.zeros_like(a))
    ni = model.n_initial
    cs.result = _counts_result(model, ci, ct, (rc[:ni].copy(), rc[ni:].copy()) if pairs else None, **cs.kernels)


def _sample_in_block(ctx, model, p, at, dense, log_weight=0):
    """sample_dbn_device into a _device_arrays block `at` that has TraceLayout's entries and `attempts` (dense: the dynamic half is wanted);
    returns the sampler's name"""
    sample_dbn_device(ctx, model, p, init_bin=at["init_bin"], init_val=at["init_val"], dyn_bin=at["dyn_bin"] if dense else 0,
                      dyn_val=at["dyn_val"] if dense else 0, attempts=at["attempts"], log_weight=log_weight)
    return ctx.last_kernel()


def sample_count_host(ctx, model, n, T, seed, transition_mode=L.TRANSITION_REFERENCE_AUTO, first_index=0, counts=None):
    """Sample n trajectories of T seconds into a device block (emgpu_sample_dbn_device), count them where they lie (emgpu_count_dbn_device)
    and bring back the tables alone: the trace never crosses PCIe.  The trace is the one sample_dbn_host(ctx, model, n, T, seed,
    transition_mode=..., first_index=...) returns, so the result equals count_dbn_host of that.  Returns count_dbn_host's dict, with
    `kernel` the sampler's and `count_kernel` the counting kernel's."""
    nd, T, n = model.n_dyn, int(T), int(n)
    with _device_arrays(ctx, **TraceLayout(model.n_initial, nd, n, T).nbytes, attempts=4 * n, **_count_bytes(model)) as at, \
            _count_scope(ctx, model, at, counts) as cs:
        p, keep = make_params(n, T, seed, first_index=first_index, transition_mode=transition_mode)
        kernel = _sample_in_block(ctx, model, p, at, nd > 0)
        transitions = nd > 0 and T > 1
        count_dbn_device(ctx, model, score_params(n, T, p.transition_mode), at["init_bin"], at["dyn_bin"] if transitions else 0,
                         at["ci"], at["ct"] if transitions else 0)
        cs.kernels.update(kernel=kernel, count_kernel=ctx.last_kernel())
    del keep
    return cs.result


def count_dbn_weighted_device(ctx, model, params, init_bin, dyn_bin, weights, counts_initial=0, counts_transition=0):
    """emgpu_count_dbn_weighted_device: count_dbn_device in which every observation of trajectory i adds weights[i] -- a device array of
    params.n uint32, not offset by col_offset -- instead of 1.  A trajectory of weight 0 adds nothing and reports nothing, whatever its bins
    hold.  One call takes n * max(1, sample_time - 1) <= 2**32."""
    _device_call("count_dbn_weighted_device", (ctx, model), params, init_bin, dyn_bin, weights, counts_initial, counts_transition)


def count_dbn_weighted_host(ctx, model, init_bin, dyn_bin, T, weights, transition_mode=L.TRANSITION_REFERENCE_AUTO, raw=False, n=None,
                            col_offset=0, counts=None):
    """count_dbn_host in which every observation of trajectory i adds weights[i] instead of 1 (emgpu_count_dbn_weighted_host; include/emgpu.h):
    the importance-weighted sufficient statistics of a trace, and, with weights in {0, 1}, the count of a subset.  weights: an integer array
    [n] with values in 0 .. 2**32 - 1, entry i for trajectory col_offset + i of a raw trace (ValueError otherwise, before the library is
    called).  A trajectory of weight 0 adds nothing and reports nothing, whatever its bins hold.  Returns count_dbn_host's dict; the tables are
    exact integers (float64 N_initial / N_transition: exact below 2**53, `raw` always)."""
    # np.asarray: never None, so a missing weights argument fails _weights_array's check like any other non-integer array
    return _count_host(ctx, model, init_bin, dyn_bin, T, np.asarray(weights), transition_mode, raw, n, col_offset, counts)


def quantize_weights(log_w, bits=24, keep=None):
    """Log-weights -> (w uint32 [n], log_scale): the integer weights count_dbn_weighted_* take, so that the real weight of trajectory i is
    w[i] * exp(log_scale).  The live entries are the finite log_w[i] (with keep[i] true where keep is given); m is their maximum,
    w = rint(exp(log_w - m) * (2**bits - 1)) for them (ties to even; the largest weight becomes 2**bits - 1) and 0 for every other entry:
    NaN (a trajectory whose scoring reported a bad bin), -inf, and entries not kept.  log_scale = m - log(2**bits - 1); with no live entry w
    is all zeros and log_scale is -inf.  +inf anywhere is a ValueError, and so is bits outside 1 .. 32.  Pure numpy."""
    bits = int(bits)
    if not 1 <= bits <= 32:
        raise ValueError("quantize_weights: bits must lie in 1 .. 32")
    lw = np.asarray(log_w, dtype=np.float64).reshape(-1)
    if np.isposinf(lw).any():
        raise ValueError("quantize_weights: a log-weight of +inf has no finite scale")
    live = np.isfinite(lw)
    if keep is not None:
        keep = np.asarray(keep, dtype=bool).reshape(-1)
        if keep.shape != lw.shape:
            raise ValueError("quantize_weights: keep must have one entry per log-weight")
        live &= keep
    w = np.zeros(lw.shape, dtype=np.uint32)
    if not live.any():
        return w, float("-inf")
    m = float(lw[live].max())
    top = float(2**bits - 1)
    w[live] = np.rint(np.exp(lw[live] - m) * top).astype(np.uint64).astype(np.uint32)
    return w, m - float(np.log(top))


def reweight_count_host(ctx, proposal, target, n, T, seed, bits=24, transition_mode=L.TRANSITION_REFERENCE_AUTO, first_index=0, counts=None):
    """The importance-weighted sufficient statistics of a sample without the trace crossing PCIe: draw n trajectories of T
    seconds under `proposal` into a device block, score the trace under both models where it lies, download the two log_lik arrays (16
    bytes per trajectory), quantize log_lik_target - log_lik_proposal on the host (quantize_weights, `bits`), upload the weights (4 bytes
    per trajectory), count the trace with them where it lies (emgpu_count_dbn_weighted_device, in `proposal`'s tables: both models have one
    shape) and download the tables.  Equals sample_weighted_host, quantize_weights and count_dbn_weighted_host in a row.
    Returns count_dbn_host's dict plus weights [n] uint32, log_scale (the real weight of trajectory i is weights[i] * exp(log_scale)),
    ess = (sum w)**2 / sum w**2 (0.0 when every weight is 0), log_lik_proposal, log_lik_target, kernel (the sampler's), score_kernel and
    count_kernel.  ValueError when the models differ in shape (sample_weighted_host's check)."""
    if not _same_shape(proposal, target):
        raise ValueError("reweight_count_host: proposal and target differ in n_initial, r_initial, the temporal map or the dynamic variables' r")
    nd, T, n = proposal.n_dyn, int(T), int(n)
    with _device_arrays(ctx, **TraceLayout(proposal.n_initial, nd, n, T).nbytes, attempts=4 * n, ll_p=8 * n, ll_t=8 * n, w=4 * n,
                        **_count_bytes(proposal)) as at, _count_scope(ctx, proposal, at, counts) as cs:
        p, keep = make_params(n, T, seed, first_index=first_index, transition_mode=transition_mode)
        dense = nd > 0
        kernel = _sample_in_block(ctx, proposal, p, at, dense)
        sp = score_params(n, T, p.transition_mode)
        score_dbn_device(ctx, proposal, sp, at["init_bin"], at["dyn_bin"] if dense else 0, at["ll_p"])
        score_dbn_device(ctx, target, sp, at["init_bin"], at["dyn_bin"] if dense else 0, at["ll_t"])
        score_kernel = ctx.last_kernel()
        ctx.sync()                                  # the three launches' deferred errors
        ll_p = device_download(ctx, at["ll_p"], np.zeros(n, np.float64))
        ll_t = device_download(ctx, at["ll_t"], np.zeros(n, np.float64))
        w, log_scale = quantize_weights(ll_t - ll_p, bits)
        transitions = dense and T > 1
        cs.counted, count_kernel = n > 0, ""
        if cs.counted:
            device_upload(ctx, at["w"], w)
            count_dbn_weighted_device(ctx, proposal, sp, at["init_bin"], at["dyn_bin"] if transitions else 0, at["w"],
                                      at["ci"], at["ct"] if transitions else 0)
            count_kernel = ctx.last_kernel()
        s1, s2 = float(w.astype(np.float64).sum()), float((w.astype(np.float64) ** 2).sum())
        cs.kernels.update(weights=w, log_scale=log_scale, ess=s1 * s1 / s2 if s2 > 0 else 0.0, log_lik_proposal=ll_p, log_lik_target=ll_t,
                          kernel=kernel, score_kernel=score_kernel, count_kernel=count_kernel)
    del keep
    return cs.result


def wrap_mask(wrap):
    """emgpu_discretize_params.wrap_mask of `wrap`: None, an int mask (bit v - 1 = variable v), or the 1-based ids of the variables that wrap"""
    if wrap is None:
        return 0
    if isinstance(wrap, (int, np.integer)):
        return int(wrap)
    mask = 0
    for v in wrap:
        if not 1 <= int(v) <= 32:
            raise ValueError("wrap holds 1-based variable ids")
        mask |= 1 << (int(v) - 1)
    return mask


def discretize_params(n, sample_time, n_fine=0, value_type=L.VALUE_F32, wrap=None, ld=0, col_offset=0):
    p = L.DiscretizeParams()
    p.n, p.sample_time, p.n_fine, p.ld, p.col_offset = int(n), int(sample_time), int(n_fine), int(ld), int(col_offset)
    p.value_type, p.wrap_mask = int(value_type), wrap_mask(wrap)
    return p


def discretize_dbn_device(ctx, model, params, init_val=0, dyn_val=0, init_bin=0, dyn_bin=0, repeat=0, change=0):
    """emgpu_discretize_dbn_device: asynchronous, raw device pointers (ints; params: discretize_params).  init_val / dyn_val in the sampler's
    layout (f32, or f64 under VALUE_F64) become init_bin u8 / dyn_bin u32 in the layout score_dbn_device and count_dbn_device read; either
    pair may be 0.  repeat / change are uint64 [n_initial] by variable id, which the call ADDS to (0 with n_fine 0).  A bad value (NaN, a
    categorical value that is no integer in 1..r) gets bin 0 and makes the next ctx.sync() raise EmgpuError(ERR_ARG)."""
    _device_call("discretize_dbn_device", (ctx, model), params, init_val, dyn_val, init_bin, dyn_bin, repeat, change)


def _value_arrays(model, init_val, dyn_val, T, raw):
    """(init_val [n_i, ld] or None, dyn_val [G4, n_d, ld, 4] or None, ld, value_type) of a call's values: one dtype, f32 or f64"""
    given = [np.asarray(a) for a in (init_val, dyn_val) if a is not None]
    if not given:
        raise ValueError("init_val and dyn_val are both None: nothing to discretize")
    dt = np.float64 if any(a.dtype == np.float64 for a in given) else np.float32
    iv = dv = None
    if init_val is not None:
        iv = np.ascontiguousarray(init_val, dtype=dt) if raw else np.ascontiguousarray(np.asarray(init_val, dtype=dt).T)
        if iv.ndim != 2 or iv.shape[0] != model.n_initial:
            raise ValueError("init_val must hold n_initial entries per trajectory")
    if dyn_val is not None:
        dv = np.ascontiguousarray(dyn_val, dtype=dt) if raw else pack_dyn_val(np.asarray(dyn_val, dtype=dt))
        ld = iv.shape[1] if iv is not None else dv.shape[2] if dv.ndim == 4 else 0
        if dv.shape != TraceLayout(model.n_initial, model.n_dyn, ld, T).shape["dyn_val"]:
            raise ValueError("dyn_val must hold T columns of n_dyn variables for the trajectories of init_val")
    ld = iv.shape[1] if iv is not None else dv.shape[2]
    return iv, dv, ld, (L.VALUE_F64 if dt == np.float64 else L.VALUE_F32)


def _pair_vectors(model, counts):
    """the repeat / change vectors of a call: fresh zeros, or a previous result's `raw` (accumulated into, in place)"""
    return _raw_pair(counts, [model.n_initial] * 2,
                     "counts must be the `raw` pair of a discretize of this model: contiguous uint64 arrays of n_initial entries")


def discretize_dbn_host(ctx, model, init_val, dyn_val, T, n_fine=0, wrap=None, raw=False, n=None, col_offset=0, counts=None):
    """Values to bins, and the repeat / change counts of their fine bins (emgpu_discretize_dbn_host; the definition is in include/emgpu.h).
    raw=False: the user-facing shapes sample_dbn_host returns (init_val [n, n_i], dyn_val [n, T, n_d]; either may be None); raw=True: the
    library layout (init_val [n_i, ld], dyn_val [G4, n_d, ld, 4]), of which columns col_offset .. col_offset + n are discretized (n:
    default ld - col_offset; the other columns of the outputs are 0).  float64 arrays are compared as doubles, anything else as float32.
    Returns {"init_bin", "dyn_bin"} in the same layout as the values (u8; raw dyn_bin: u32 [G4, n_d, ld]; None where the values were),
    "repeat" / "change" [n_initial] float64 by variable id, "raw": (u64 repeat, u64 change), "kernel".  counts=<a previous result's raw>
    accumulates.  A bad value gets bin 0 and raises EmgpuError(ERR_ARG) carrying .bins (the same dict)."""
    T = int(T)
    iv, dv, ld, vt = _value_arrays(model, init_val, dyn_val, T, raw)
    n = ld - int(col_offset) if n is None else int(n)
    rep, chg = _pair_vectors(model, counts)
    lay = TraceLayout(model.n_initial, model.n_dyn, ld, T)
    ib = None if iv is None else lay.make("init_bin")
    db = None if dv is None else lay.make("dyn_bin")
    p = discretize_params(n, T, n_fine, vt, wrap, ld, col_offset)
    rc = L.lib().emgpu_discretize_dbn_host(ctx._h if ctx is not None else None, model._h, C.byref(p), _p(iv), _p(dv), _p(ib), _p(db),
                                           _p(rep) if n_fine else None, _p(chg) if n_fine else None)
    out = {"init_bin": ib if raw or ib is None else ib.T.copy(), "dyn_bin": db if raw or db is None else unpack_dyn_bin(db, T),
           "repeat": rep.astype(np.float64), "change": chg.astype(np.float64), "raw": (rep, chg),
           "kernel": ctx.last_kernel() if ctx is not None else ""}
    if rc < 0:
        _raise(rc, bins=out)
    return out


def _discretize_count_in_block(ctx, model, at, n, T, n_fine, value_type, wrap, transition_mode, dense, **kernels):
    """The values that lie at at["init_val"] / at["dyn_val"] of a _device_arrays block (dense: it has the dynamic half) discretized into
    at["init_bin"] / at["dyn_bin"] and counted there, into fresh tables at at["ci"] / at["ct"] and vectors at at["rc"] (2 n_initial u64),
    which alone come back: discretize_count_host's dict."""
    with _count_scope(ctx, model, at, pairs=True) as cs:
        discretize_dbn_device(ctx, model, discretize_params(n, T, n_fine, value_type, wrap), at["init_val"], at["dyn_val"] if dense else 0,
                              at["init_bin"], at["dyn_bin"] if dense else 0, at["rc"] if n_fine else 0,
                              at["rc"] + 8 * model.n_initial if n_fine else 0)
        kernel = ctx.last_kernel()
        transitions = dense and T > 1
        count_dbn_device(ctx, model, score_params(n, T, transition_mode), at["init_bin"], at["dyn_bin"] if transitions else 0,
                         at["ci"], at["ct"] if transitions else 0)
        cs.kernels.update(kernel=kernel, count_kernel=ctx.last_kernel(), **kernels)
    return cs.result


def _discretize_count_bytes(model, n, T, dense):
    """the arrays of _discretize_count_in_block besides the values, for _device_arrays"""
    nb = TraceLayout(model.n_initial, model.n_dyn, n, T).nbytes
    return dict(init_bin=nb["init_bin"], dyn_bin=nb["dyn_bin"] if dense else 0, **_count_bytes(model, True))


def discretize_count_host(ctx, model, init_val, dyn_val, n_fine=0, wrap=None, transition_mode=L.TRANSITION_REFERENCE_AUTO):
    """Values in the user-facing shapes (init_val [n, n_i], dyn_val [n, T, n_d] or None; f32 or f64) to the model's count tables and the two
    vectors, all on the device: the values are uploaded, discretized (emgpu_discretize_dbn_device) and counted where the bins lie
    (emgpu_count_dbn_device), and only the tables and the vectors come back.  Equals discretize_dbn_host followed by count_dbn_host.
    Returns count_dbn_host's dict plus "repeat" / "change" [n_initial] float64 ("raw_pairs": the same as uint64), `kernel` the discretizer's,
    `count_kernel` the counter's.
    A bad value raises EmgpuError(ERR_ARG): its bin is 0, which counting skips."""
    if init_val is None:
        raise ValueError("counting needs init_val")
    T = 1 if dyn_val is None else int(np.asarray(dyn_val).shape[1])
    iv, dv, n, vt = _value_arrays(model, init_val, dyn_val, T, False)
    dense = dv is not None and model.n_dyn > 0
    with _device_arrays(ctx, init_val=iv.nbytes, dyn_val=dv.nbytes if dense else 0, **_discretize_count_bytes(model, n, T, dense)) as at:
        for name, a in (("init_val", iv), ("dyn_val", dv if dense else None)):
            if a is not None and a.size:
                device_upload(ctx, at[name], a)
        return _discretize_count_in_block(ctx, model, at, n, T, n_fine, vt, wrap, transition_mode, dense)


def track_values_params(n, points, ur_speed, ur_vertrate, ur_heading, n_initial=5, nd=3, rows=(0, 1, 2, 3, 4), slots=(0, 1, 2),
                        value_type=L.VALUE_F32, layout=L.TRACKS_ROWS, ld=0, col_offset=0):
    """emgpu_track_values_params.  rows: the 0-based rows of init_val that receive altitude, speed, vertical rate, acceleration and turn rate
    (-1: not written); slots: the 0-based rows of a dyn_val group that receive vertical rate, acceleration and turn rate."""
    p = L.TrackValuesParams()
    p.n, p.points, p.value_type, p.ld, p.col_offset = int(n), int(points), int(value_type), int(ld), int(col_offset)
    p.n_initial, p.nd, p.layout = int(n_initial), int(nd), int(layout)
    p.row_alt, p.row_speed, p.row_vertrate, p.row_acc, p.row_turnrate = (int(r) for r in rows)
    p.slot_vertrate, p.slot_acc, p.slot_turnrate = (int(s) for s in slots)
    p.ur_speed, p.ur_vertrate, p.ur_heading = float(ur_speed), float(ur_vertrate), float(ur_heading)
    return p


def track_values_device(ctx, params, xyz, init_val=0, dyn_val=0):
    """emgpu_track_values_device: asynchronous, raw device pointers (ints; params: track_values_params).  xyz f64 in params.layout
    (TRACKS_PLANAR [P, 3, n], what sample2track_device writes, or TRACKS_ROWS [n, P, 3]) becomes the named rows of init_val [n_initial, ld]
    and dyn_val [G4, nd, ld, 4] (f32, or f64 under VALUE_F64), the layout discretize_dbn_device reads; either may be 0.  Every other row is
    left as it is."""
    _device_call("track_values_device", (ctx,), params, xyz, init_val, dyn_val)


def _track_array(xyz):
    """(xyz [n, P, 3] as contiguous f64, n, P)"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    if xyz.ndim != 3 or xyz.shape[2] != 3:
        raise ValueError("xyz must be [n, points, 3]")
    n, P = int(xyz.shape[0]), int(xyz.shape[1])
    return xyz, n, P


def _fill_static(iv, static, written):
    """static = {1-based variable id: array [n] or scalar} into the rows of init_val [n_initial, n] the kernel leaves"""
    for v, a in (static or {}).items():
        v = int(v)
        if not 1 <= v <= iv.shape[0]:
            raise ValueError("static names variable %d of %d" % (v, iv.shape[0]))
        if v - 1 in written:
            raise ValueError("static names variable %d, which the tracks give" % v)
        iv[v - 1, :] = np.asarray(a, dtype=iv.dtype)


def track_values_host(ctx, xyz, ur_speed, ur_vertrate, ur_heading, n_initial=5, nd=3, rows=(0, 1, 2, 3, 4), slots=(0, 1, 2),
                      value_type=L.VALUE_F32, raw=False, static=None, want_init=True, want_dyn=True):
    """The values of a trace from 1 Hz tracks (emgpu_track_values_host; the definition is in include/emgpu.h).  xyz [n, P, 3] f64 in feet,
    P >= 3, gives T = P - 2 seconds.  rows / slots as in track_values_params.  Returns {"init_val", "dyn_val", "T", "kernel"}: init_val
    [n, n_initial] and dyn_val [n, T, nd] (raw=True: the library layout, [n_initial, n] and [G4, nd, n, 4]), float32 or float64 by
    value_type.  Rows the tracks do not give are 0, but for static = {1-based variable id: array [n] or scalar}, which fills rows of
    init_val (G, A, ... of a model).  want_init / want_dyn False: that half is None."""
    xyz, n, P = _track_array(xyz)
    T = P - 2
    lay = TraceLayout(n_initial, nd, n, T, 8 if value_type == L.VALUE_F64 else 4)
    iv = lay.make("init_val") if want_init else None
    dv = lay.make("dyn_val") if want_dyn else None
    if iv is not None:
        _fill_static(iv, static, [int(r) for r in rows if int(r) >= 0])
    p = track_values_params(n, P, ur_speed, ur_vertrate, ur_heading, n_initial, nd, rows, slots, value_type, L.TRACKS_ROWS)
    L.check(L.lib().emgpu_track_values_host(ctx._h if ctx is not None else None, C.byref(p), _p(xyz), _p(iv), _p(dv)))
    return {"init_val": iv if raw or iv is None else np.ascontiguousarray(iv.T),
            "dyn_val": dv if raw or dv is None else unpack_dyn_val(dv, T), "T": T, "kernel": ctx.last_kernel()}


def track_rows(model, variables):
    """(rows, slots) of track_values_params for a model: variables = the 1-based ids of L, v, \\dot h (vertical rate), \\dot v (acceleration),
    \\dot \\psi (turn rate), 0 = the model has none (L and v only); the slots are the rates' rows of the temporal map."""
    idL, idV, idDH, idDV, idDPsi = (int(v) for v in variables)
    tm = model.get_i32(L.F_TEMPORAL_MAP).reshape(-1, 2)[:, 0].tolist()
    if not all(v in tm for v in (idDH, idDV, idDPsi)):
        raise ValueError("the temporal map does not hold the three rates")
    return (idL - 1, idV - 1, idDH - 1, idDV - 1, idDPsi - 1), (tm.index(idDH), tm.index(idDV), tm.index(idDPsi))


def track_count_host(ctx, model, xyz, rows, static=None, n_fine=4, wrap=None, transition_mode=L.TRANSITION_REFERENCE_AUTO,
                     unit_ratios=((1852.0 / 0.3048) / 3600.0, 1.0 / 60.0, 1.0), value_type=L.VALUE_F64):
    """Tracks xyz [n, P, 3] f64 to the model's count tables and the repeat / change vectors, all on the device: the tracks are uploaded as
    they lie, turned into values (emgpu_track_values_device, ROWS), discretized (emgpu_discretize_dbn_device) and counted
    (emgpu_count_dbn_device) in one device block, and only the tables and the vectors come back.  rows: the 1-based variable ids of L, v,
    \\dot h, \\dot v, \\dot \\psi (track_rows); static = {1-based variable id: array [n] or scalar}: the values of the variables the tracks
    do not give (G, A), without which their bins are bad.  unit_ratios: (ur_speed, ur_vertrate, ur_heading) of sample2track.m:113-123.
    Equals track_values_host followed by discretize_count_host.  Returns discretize_count_host's dict, `values_kernel` the first kernel's."""
    xyz, n, P = _track_array(xyz)
    T, ni, nd = P - 2, model.n_initial, model.n_dyn
    r0, slots = track_rows(model, rows)
    lay = TraceLayout(ni, nd, n, T, 8 if value_type == L.VALUE_F64 else 4)
    iv = lay.make("init_val")
    _fill_static(iv, static, [r for r in r0 if r >= 0])
    p = track_values_params(n, P, *unit_ratios, n_initial=ni, nd=nd, rows=r0, slots=slots, value_type=value_type, layout=L.TRACKS_ROWS)
    with _device_arrays(ctx, xyz=xyz.nbytes, init_val=iv.nbytes, dyn_val=lay.nbytes["dyn_val"], **_discretize_count_bytes(model, n, T, True)) as at:
        for name, a in (("xyz", xyz), ("init_val", iv)):
            if a.size:
                device_upload(ctx, at[name], a)
        if nd > 3 and n:   # dynamic variables the tracks do not give: zeros, as track_values_host leaves them
            device_upload(ctx, at["dyn_val"], lay.make("dyn_val"))
        track_values_device(ctx, p, at["xyz"], at["init_val"], at["dyn_val"])
        return _discretize_count_in_block(ctx, model, at, n, T, n_fine, value_type, wrap, transition_mode, True, values_kernel=ctx.last_kernel())


def sample_weighted_host(ctx, proposal, target, n, T, seed, raw=False, want_log_weight=False, first_index=0,
                         transition_mode=L.TRANSITION_REFERENCE_AUTO, flags=0, max_attempts=1000, idx_L=0, idx_v=0, idx_dh=0, layers=None,
                         indices=None, start=None):
    """Importance sampling between two models of one shape: draw n trajectories of T seconds under `proposal` into a
    device-resident trace (emgpu_sample_dbn_device), score that trace under both models where it lies, and bring everything back.
    The keywords are make_params' sampling keywords, with sample_dbn_host's meaning; `indices` [n] uint64 and `start` [n, n_initial] (a
    start grid, 0 = unset) are numpy arrays, which this function copies to the device.  Returns a dict: init_bin, init_val, dyn_bin, dyn_val
    and attempts -- equal to what sample_dbn_host(ctx, proposal, n, T, seed, <the same keywords>) returns under these names (raw: in the
    library's layout) -- `kernel` (the sampler's) and `score_kernel`, log_weight (want_log_weight: the start grid's log-weights under the
    proposal, as sample_dbn_host's), log_lik_proposal, log_lik_target and log_weight_model = log_lik_target - log_lik_proposal, subtracted
    on the host.  No event lists and no host_stats: nothing goes through the chunked host path.
    The weights are those of the networks alone: a rejection loop (idx_L / idx_v / idx_dh, layers) renormalises both models differently,
    and that ratio is not part of them.  ValueError when the models differ in n_initial, r_initial, the temporal map or the dynamic
    variables' r, or when `start` / `indices` are not arrays of the shapes above."""
    if not _same_shape(proposal, target):
        raise ValueError("sample_weighted_host: proposal and target differ in n_initial, r_initial, the temporal map or the dynamic variables' r")
    ni, nd, T, n = proposal.n_initial, proposal.n_dyn, int(T), int(n)
    # a host address in params.start / .indices would be read by the kernel: both go to the device block first
    if start is not None:
        if isinstance(start, int):
            raise ValueError("sample_weighted_host: start is a numpy start grid [n, n_initial], not a device pointer")
        start = np.ascontiguousarray(start, dtype=np.int32)
        if start.shape != (n, ni):
            raise ValueError("sample_weighted_host: start must be [n, n_initial]")
    if indices is not None:
        if isinstance(indices, int):
            raise ValueError("sample_weighted_host: indices is a numpy array of n global indices, not a device pointer")
        indices = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        if indices.size != n:
            raise ValueError("sample_weighted_host: indices must hold n entries")
    lay = TraceLayout(ni, nd, n, T)
    with _device_arrays(ctx, **lay.nbytes, attempts=4 * n, ll_p=8 * n, ll_t=8 * n, lw=8 * n, start=4 * ni * n if start is not None else 0,
                        indices=8 * n if indices is not None else 0) as at:
        if start is not None:
            device_upload(ctx, at["start"], start)
        if indices is not None:
            device_upload(ctx, at["indices"], indices)
        p, keep = make_params(n, T, seed, first_index=first_index, transition_mode=transition_mode, flags=flags, max_attempts=max_attempts,
                              idx_L=idx_L, idx_v=idx_v, idx_dh=idx_dh, layers=layers, indices=at["indices"] if indices is not None else None,
                              start=at["start"] if start is not None else None)
        dense = nd > 0
        kernel = _sample_in_block(ctx, proposal, p, at, dense, log_weight=at["lw"] if want_log_weight else 0)
        sp = score_params(n, T, p.transition_mode)
        score_dbn_device(ctx, proposal, sp, at["init_bin"], at["dyn_bin"] if dense else 0, at["ll_p"])
        score_dbn_device(ctx, target, sp, at["init_bin"], at["dyn_bin"] if dense else 0, at["ll_t"])
        out = {"kernel": kernel, "score_kernel": ctx.last_kernel()}
        ctx.sync()                                  # the three launches' deferred errors
        ib, iv = (device_download(ctx, at[k], lay.make(k)) for k in ("init_bin", "init_val"))
        out["attempts"] = device_download(ctx, at["attempts"], np.zeros(n, np.int32))
        out["init_bin"], out["init_val"] = (ib, iv) if raw else (ib.T.copy(), iv.T.copy())
        if dense:
            db, dv = (device_download(ctx, at[k], lay.make(k)) for k in ("dyn_bin", "dyn_val"))
            out["dyn_bin"] = db if raw else unpack_dyn_bin(db, T)
            out["dyn_val"] = dv if raw else unpack_dyn_val(dv, T)
        if want_log_weight:
            out["log_weight"] = device_download(ctx, at["lw"], np.zeros(n, np.float64))
        out["log_lik_proposal"] = device_download(ctx, at["ll_p"], np.zeros(n, np.float64))
        out["log_lik_target"] = device_download(ctx, at["ll_t"], np.zeros(n, np.float64))
        out["log_weight_model"] = out["log_lik_target"] - out["log_lik_proposal"]
    del keep
    return out
