"""Text on the device: em_sample's rows formatted there, numeric tables parsed there, and the two number formatters on their own."""
import ctypes as C
import re

import numpy as np

from .. import _lib as L
from .base import _array_factory, _error, _event_cap_error, _last_message, _p, make_params
from .layout import TraceLayout, unpack_dyn_val


def text_bound(model, n, sample_time):
    """emgpu_text_bound: (bytes of the initial text, bytes of the transition text) that always hold sample_text_host's rows:
    n (21 + 13 n_initial) and n sample_time 13 (2 + n_dyn)."""
    b = np.zeros(2, dtype=np.int64)
    L.check(L.lib().emgpu_text_bound(model._h, int(n), int(sample_time), _p(b)))
    return int(b[0]), int(b[1])


def sample_text_host(ctx, model, n, sample_time, seed, id_first=1, want_arrays=True, pinned=True, initial_cap=None, transition_cap=None,
                     buffers=None, raw=False, **kw):
    """emgpu_sample_text_host: the rows of em_sample's initial and transition files (without their header lines), formatted on the device.
    Returns a dict: initial, transition (uint8 arrays: the bytes, views of the call's buffers), totals, init_val [n, n_i] f32 and
    dyn_val [n, T, n_d] f32 (the values the rows print; None unless want_arrays; raw: in the library's layout, as sample_dbn_host returns
    them), kernel, host_stats.  id_first: the id of trajectory 0.  pinned: the buffers come from the context's pinned pool, else pageable numpy
    arrays.  initial_cap / transition_cap: bytes of the buffers (default: text_bound); buffers: (initial, transition) uint8 arrays of a caller
    who makes several calls.  Text that outgrows a buffer raises EmgpuError(ERR_EVENT_CAP) with `.totals` (the bytes needed): a retry with
    that room gives the same bytes.  start= (make_params): a start grid [n, n_initial], trajectory i drawn under row i."""
    ni, nd, T, n = model.n_initial, model.n_dyn, int(sample_time), int(n)
    p, keep = make_params(n, T, seed, **kw)
    empty = _array_factory(ctx, pinned, np.empty)
    if buffers is not None:
        bi, bt = buffers
    else:
        b0, b1 = text_bound(model, n, T)
        bi = empty((max(int(b0 if initial_cap is None else initial_cap), 1),), np.uint8)
        bt = empty((max(int(b1 if transition_cap is None else transition_cap), 1),), np.uint8)
    o = L.TextOut()
    totals = np.zeros(2, dtype=np.int64)
    o.initial, o.transition, o.totals, o.id_first = _p(bi), _p(bt), _p(totals), int(id_first)
    o.initial_cap = bi.size if initial_cap is None else int(initial_cap)
    o.transition_cap = bt.size if transition_cap is None else int(transition_cap)
    iv = dv = None
    if want_arrays:
        lay = TraceLayout(ni, nd, n, T)
        iv = lay.make("init_val", empty)
        o.init_val = _p(iv)
        if nd > 0:
            dv = lay.make("dyn_val", empty)
            o.dyn_val = _p(dv)
    rc = L.lib().emgpu_sample_text_host(ctx._h, model._h, C.byref(p), C.byref(o))
    if rc == L.ERR_EVENT_CAP:
        raise _event_cap_error(rc, (int(totals[0]), int(totals[1])))
    L.check(rc)
    out = {"initial": bi[: int(totals[0])], "transition": bt[: int(totals[1])], "totals": (int(totals[0]), int(totals[1])),
           "init_val": None, "dyn_val": None, "kernel": ctx.last_kernel(), "host_stats": ctx.host_stats()}
    if want_arrays:
        out["init_val"] = iv if raw else iv.T.copy()
        if dv is not None:
            out["dyn_val"] = dv if raw else unpack_dyn_val(dv, T)
    return out


def format_g(ctx, x, cap=None, return_paths=False):
    """emgpu_format_g_host: "%g" of every f32 value of x by the device formatter of sample_text_host, non-finite values spelled NaN / Inf / -Inf.
    Returns the list of strings; return_paths: also (values formatted on the 64-bit path, on the multiword path) -- emgpu_debug_format_paths."""
    paths = np.zeros(2, dtype=np.uint64)
    if return_paths:
        L.check(L.lib().emgpu_debug_format_paths(ctx._h, _p(paths)))   # (reading clears)
    strings = _formatted(L.lib().emgpu_format_g_host, ctx, x, np.float32, 12, cap)
    if return_paths:
        L.check(L.lib().emgpu_debug_format_paths(ctx._h, _p(paths)))
        return strings, (int(paths[0]), int(paths[1]))
    return strings


def _formatted(entry, ctx, x, dtype, width, cap):
    """the strings a formatter entry point makes of the values of x: one text of at most cap bytes (default: width per value) and its offsets"""
    x = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
    n = x.size
    cap = width * n if cap is None else int(cap)
    buf = np.empty(max(cap, 1), dtype=np.uint8)
    offs = np.zeros(n + 1, dtype=np.uint64)
    L.check(entry(ctx._h, _p(x), n, _p(buf), cap, _p(offs)))
    text = buf[: int(offs[n])].tobytes().decode("ascii")
    o = offs.astype(np.int64).tolist()
    return [text[a:b] for a, b in zip(o[:-1], o[1:])]


def format_f0(ctx, x, cap=None):
    """emgpu_format_f0_host: "%0.0f" of every double of x by the device function the CSV rows use.  Returns the list of strings; a value the
    device does not format (not finite, or 2^63 and more in magnitude) gives None."""
    return [s or None for s in _formatted(L.lib().emgpu_format_f0_host, ctx, x, np.float64, 20, cap)]


def csv_bound(n, rows):
    """emgpu_csv_bound: bytes that always hold the CSV text of n tracks with `rows` position rows in all: 22 n + 74 rows."""
    return int(L.lib().emgpu_csv_bound(int(n), int(rows)))


def _buffer_address(data):
    """(address, bytes, keep-alive) of a bytes-like object or a uint8 array, without a copy."""
    if isinstance(data, np.ndarray):
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        return a.ctypes.data, a.size, a
    if isinstance(data, (bytes, bytearray, memoryview)):
        a = np.frombuffer(data, dtype=np.uint8)
        return (a.ctypes.data if a.size else 0), a.size, a
    raise TypeError("text: bytes, bytearray, memoryview or a uint8 array")


_LINE = re.compile(r"line (\d+)")


def _parse_error(rc, header_lines, what):
    """EMGPU_ERR_PARSE as the ValueError the host reader raises; the line is counted from the top of the file."""
    msg = _last_message()
    m = _LINE.search(msg)
    if m:
        msg = "%s: line %d is not a row of numbers with the expected columns (%s)" % (what, int(m.group(1)) + header_lines, msg)
    e = ValueError(msg)
    e.line = int(m.group(1)) + header_lines if m else None
    return e


def parse_table(ctx, data, ncol, return_stats=False, header_lines=0, rows_cap=None):
    """emgpu_parse_table_host: the numeric text table `data` (bytes-like, or a uint8 array -- a pinned one is read by the copy engine in
    place) parsed on the device -> f64 [rows, ncol], every value bit-equal to float(token).  Grammar: include/emgpu.h (narrower than
    numpy.loadtxt: no '#' comments).  A malformed line raises ValueError with `.line` (1-based, plus header_lines: the lines the caller cut off
    in front).  return_stats: also {"rows", "hard_tokens"} (hard tokens: those the device hands to the host's strtod).  rows_cap: rows of the
    output array (default: what the bytes can hold at most); too few raise EmgpuError(ERR_EVENT_CAP) with `.rows`."""
    addr, nbytes, keep = _buffer_address(data)
    ncol = int(ncol)
    cap = nbytes // (2 * ncol) + 1 if rows_cap is None else int(rows_cap)
    out = np.empty((max(cap, 1), ncol), dtype=np.float64)
    rows, hard = C.c_int64(0), C.c_uint64(0)
    rc = L.lib().emgpu_parse_table_host(ctx._h, C.c_void_p(addr), nbytes, ncol, _p(out), cap, C.byref(rows), C.byref(hard))
    del keep
    if rc == L.ERR_PARSE:
        raise _parse_error(rc, int(header_lines), "parse_table")
    if rc == L.ERR_EVENT_CAP:
        raise _error(rc, rows=int(rows.value))
    L.check(rc)
    table = out[: int(rows.value)]
    if rows_cap is None and table.shape[0] < out.shape[0] // 2:
        table = table.copy()
    return (table, {"rows": int(rows.value), "hard_tokens": int(hard.value)}) if return_stats else table
