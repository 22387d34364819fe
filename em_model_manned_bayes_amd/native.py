"""Thin object layer over the C ABI: NativeModel (emgpu_model*), Context (emgpu_ctx*) and the
sampling calls with numpy (host) or raw device pointers (torch tensors' data_ptr()).
"""
import contextlib
import ctypes as C
import re
import types

import numpy as np

from . import _lib as L

EVENT_DTYPE = np.dtype([("dt", "<u2"), ("var", "u1"), ("bin", "u1"), ("value", "<f4")])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class NativeModel:
    """Owns an emgpu_model handle (what em_read.m returns plus priors and start)."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)
        self._refresh()

    def _refresh(self):
        info = L.ModelInfo()
        L.check(L.lib().emgpu_model_info(self._h, C.byref(info)))
        self.info = info
        self.n_initial, self.n_transition, self.n_dyn = info.n_initial, info.n_transition, info.n_dyn
        self.is_dynvar_depend = bool(info.is_dynvar_depend)

    @classmethod
    def load_txt(cls, path, idx_zero_boundaries=(1, 2, 3), is_overwrite_zero_boundaries=False):
        idx = np.asarray(list(idx_zero_boundaries), dtype=np.int32)
        h = C.c_void_p()
        L.check(L.lib().emgpu_model_load_txt(str(path).encode(), _p(idx), len(idx), int(bool(is_overwrite_zero_boundaries)), C.byref(h)))
        return cls(h.value)

    def save_bin(self, path):
        """emgpu_model_save_bin: the parsed model + its compiled plan as one binary file."""
        L.check(L.lib().emgpu_model_save_bin(self._h, str(path).encode()))

    @classmethod
    def load_bin(cls, path):
        """emgpu_model_load_bin; raises EmgpuError(ERR_PARSE) for a file written by another build of the library."""
        h = C.c_void_p()
        L.check(L.lib().emgpu_model_load_bin(str(path).encode(), C.byref(h)))
        return cls(h.value)

    @classmethod
    def load_cached(cls, path, idx_zero_boundaries=(1, 2, 3), is_overwrite_zero_boundaries=False, cache_dir=None):
        """load_txt through the binary cache: `<name>.z<idx>.o<flag>.emgpubin` next to the .txt (or in cache_dir) is read when it is at
        least as new as the .txt and was written by this build of the library; otherwise the .txt is parsed and the cache (re)written."""
        import os
        tag = ".z%s.o%d.emgpubin" % ("".join(str(int(i)) for i in idx_zero_boundaries), int(bool(is_overwrite_zero_boundaries)))
        base = os.path.join(cache_dir, os.path.basename(str(path))) if cache_dir else str(path)
        binp = base + tag
        try:
            if os.path.getmtime(binp) >= os.path.getmtime(str(path)):
                return cls.load_bin(binp)
        except (OSError, L.EmgpuError):
            pass
        m = cls.load_txt(path, idx_zero_boundaries, is_overwrite_zero_boundaries)
        try:
            m.save_bin(binp)
        except L.EmgpuError:
            pass   # a read-only directory: the cache is an optimisation
        return m

    @classmethod
    def from_arrays(cls, G_initial, r_initial, N_initial, G_transition=None, r_transition=None, N_transition=None,
                    temporal_map=None, boundaries=None, zero_bins=None, resample_rates=None,
                    labels_initial=None, labels_transition=None):
        """N_initial: list of r_i x q_i arrays (all nodes); N_transition: list/dict for nodes n_i+1..n_t."""
        ni = len(r_initial)
        d = L.ModelDesc()
        keep = []

        def k(a, dt):
            a = np.ascontiguousarray(np.asarray(a, dtype=dt))
            keep.append(a)
            return a
        Gi = k(np.asarray(G_initial) != 0, np.uint8)
        ri = k(r_initial, np.int32)
        Ni = k(np.concatenate([np.asarray(N, dtype=np.float64).T.reshape(-1) for N in N_initial]), np.float64)
        d.n_initial = ni
        d.G_initial, d.r_initial, d.N_initial, d.n_N_initial = _p(Gi), _p(ri), _p(Ni), Ni.size
        if G_transition is not None and len(r_transition) > 0:
            nt = len(r_transition)
            Gt = k(np.asarray(G_transition) != 0, np.uint8)
            rt = k(r_transition, np.int32)
            if isinstance(N_transition, dict):
                seq = [N_transition[v] for v in range(ni, nt)]
            else:
                seq = list(N_transition)
                if len(seq) == nt:
                    seq = seq[ni:]
            Nt = k(np.concatenate([np.asarray(N, dtype=np.float64).T.reshape(-1) for N in seq]), np.float64)
            d.n_transition = nt
            d.G_transition, d.r_transition, d.N_transition, d.n_N_transition = _p(Gt), _p(rt), _p(Nt), Nt.size
            if temporal_map is not None:
                tm = k(np.asarray(temporal_map).reshape(-1, 2), np.int32)
                d.temporal_map, d.n_dyn = _p(tm), tm.shape[0]
        if boundaries is not None:
            bl = k([len(b) for b in boundaries], np.int32)
            bf = k(np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1) for b in boundaries] + [np.zeros(1)]), np.float64)
            d.boundaries, d.bnd_len = _p(bf), _p(bl)
        if zero_bins is not None:
            zb = k([0 if (z is None or (hasattr(z, "__len__") and len(z) == 0)) else int(np.asarray(z).reshape(-1)[0]) for z in zero_bins], np.int32)
            d.zero_bins = _p(zb)
        if resample_rates is not None:
            rr = k(resample_rates, np.float64)
            d.resample_rates = _p(rr)
        if labels_initial:
            d.labels_initial = "\n".join(labels_initial).encode()
        if labels_transition:
            d.labels_transition = "\n".join(labels_transition).encode()
        h = C.c_void_p()
        L.check(L.lib().emgpu_model_from_arrays(C.byref(d), C.byref(h)))
        return cls(h.value)

    def __del__(self):
        try:
            if self._h:
                L.lib().emgpu_model_free(self._h)
                self._h = None
        except Exception:
            pass

    # ---- field access
    def get_i32(self, field):
        n = L.check(L.lib().emgpu_model_get_i32(self._h, field, None, 0))
        out = np.zeros(n, dtype=np.int32)
        L.check(L.lib().emgpu_model_get_i32(self._h, field, _p(out), n))
        return out

    def get_f64(self, field, node=0):
        n = L.check(L.lib().emgpu_model_get_f64(self._h, field, node, None, 0))
        out = np.zeros(n, dtype=np.float64)
        L.check(L.lib().emgpu_model_get_f64(self._h, field, node, _p(out), n))
        return out

    def get_labels(self, field):
        n = L.check(L.lib().emgpu_model_get_text(self._h, field, None, 0))
        buf = C.create_string_buffer(n)
        L.check(L.lib().emgpu_model_get_text(self._h, field, buf, n))
        s = buf.value.decode()
        return s.split("\n") if s else []

    def set_f64(self, field, node, values):
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
        L.check(L.lib().emgpu_model_set_f64(self._h, field, node, _p(v), v.size))

    def set_prior(self, prior):
        """EncounterModel.prior semantics: number or 'dbe' (bn_dirichlet_prior.m:18-37)."""
        if isinstance(prior, str):
            if prior.lower() != "dbe":
                raise L.EmgpuError(L.ERR_PRIOR, "Unknown prior of %s, if char expecting prior = 'dbe'" % prior)
            L.check(L.lib().emgpu_model_set_prior(self._h, 1, 0.0))
        elif isinstance(prior, (int, float, np.floating, np.integer)):
            L.check(L.lib().emgpu_model_set_prior(self._h, 0, float(prior)))
        else:
            raise L.EmgpuError(L.ERR_PRIOR, "Second argument must be a char or double")

    def log_prob(self, network, node):
        """emgpu_model_log_prob: log P(bin | column) of one node (network 0 initial / 1 transition, node = 1-based variable id) as
        [r, q] -- the entries start_grid_log_weight and score_dbn_* add up.  [0, 0] for a transition node without a table."""
        n = L.check(L.lib().emgpu_model_log_prob(self._h, int(network), int(node), None, 0))
        out = np.zeros(n, dtype=np.float64)
        L.check(L.lib().emgpu_model_log_prob(self._h, int(network), int(node), _p(out), n))
        r = int(self.get_i32(L.F_R_TRANSITION if network else L.F_R_INITIAL)[node - 1]) if n else 0
        return out.reshape(-1, r).T if n else out.reshape(0, 0)

    def count_layout(self, network):
        """emgpu_count_layout: the element offsets of the nodes' tables in a counts array of count_dbn_* (network 0 initial / 1 transition):
        [n nodes + 1] int64, node v (1-based) at offsets[v - 1] : offsets[v], r x q column-major; the last entry is the array's length."""
        off = np.zeros((self.n_transition if network else self.n_initial) + 1, dtype=np.int64)
        L.check(L.lib().emgpu_count_layout(self._h, int(network), _p(off)))
        return off

    def set_transition_stay_prior(self, prior):
        L.check(L.lib().emgpu_model_set_transition_stay_prior(self._h, float(prior)))

    def start_log_weight(self):
        """log P(preset values of `start`) under the model: the importance weight of every sample drawn with it."""
        out = C.c_double(0.0)
        L.check(L.lib().emgpu_model_start_log_weight(self._h, C.byref(out)))
        return float(out.value)

    def set_zero_bins(self, zero_bins):
        zb = np.array([0 if (z is None or (hasattr(z, "__len__") and len(z) == 0)) else int(np.asarray(z).reshape(-1)[0]) for z in zero_bins],
                      dtype=np.int32)
        L.check(L.lib().emgpu_model_set_zero_bins(self._h, _p(zb), zb.size))

    def set_start(self, start):
        st = np.zeros(self.n_initial, dtype=np.int32)
        for i, s in enumerate(start):
            if s is None:
                continue
            a = np.asarray(s, dtype=np.float64).reshape(-1)
            if a.size == 0 or np.isnan(a[0]):
                continue
            st[i] = int(a[0])
        L.check(L.lib().emgpu_model_set_start(self._h, _p(st), st.size))


class Context:
    """One device + one stream (emgpu_ctx).  Raises EmgpuError(ERR_NO_DEVICE) without a GPU.  `stream` is the raw hipStream_t the context
    was last given (0: the HIP default stream), or None while it runs on the stream it created for itself: what a context-free call
    (miss_distance_device) takes to stay ordered behind this context's launches."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        L.check(L.lib().emgpu_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.stream = None
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream_ptr):
        L.check(L.lib().emgpu_ctx_set_stream(self._h, C.c_void_p(int(stream_ptr) if stream_ptr else 0)))
        self.stream = int(stream_ptr) if stream_ptr else 0

    def sync(self):
        L.check(L.lib().emgpu_ctx_sync(self._h))

    def trim(self):
        """emgpu_ctx_trim: release the device scratch the host-pointer / .track entry points keep between calls (the tables stay)."""
        L.check(L.lib().emgpu_ctx_trim(self._h))

    def last_kernel(self):
        return L.lib().emgpu_last_kernel_name(self._h).decode()

    def host_stats(self):
        """emgpu_host_stats: the phases of the last sample_dbn_host or sample_uncor_host call on this context, as a dict."""
        st = L.HostStats()
        L.check(L.lib().emgpu_host_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in L.HostStats._fields_}

    def device_alloc(self, nbytes):
        """emgpu_device_alloc: device memory from the allocator the traces come from; returns the address (free with device_free, or with the context)."""
        ptr = C.c_void_p()
        L.check(L.lib().emgpu_device_alloc(self._h, int(nbytes), C.byref(ptr)))
        return int(ptr.value)

    def device_free(self, addr):
        L.check(L.lib().emgpu_device_free(self._h, C.c_void_p(int(addr))))

    def pinned_empty(self, shape, dtype):
        """A numpy array over pinned host memory of this context's pool (emgpu_host_alloc): the copy engine writes the *_host entry
        points' outputs straight into it.  The block goes back to the pool when the array (and every view of it) is gone."""
        import weakref
        dt = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        ptr = C.c_void_p()
        L.check(L.lib().emgpu_host_alloc(self._h, max(nbytes, 1), C.byref(ptr)))
        buf = (C.c_char * max(nbytes, 1)).from_address(ptr.value)
        a = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)
        weakref.finalize(buf, _host_free, self, ptr.value)   # (numpy keeps `buf` alive as the base of every view; the finalizer keeps the context alive)
        return a

    def last_launches(self):
        """Kernel launches of the last sample_dbn_*_device call on this context."""
        return int(L.lib().emgpu_last_launch_count(self._h))

    def __del__(self):
        try:
            if self._h:
                L.lib().emgpu_ctx_free(self._h)
                self._h = None
        except Exception:
            pass


def _host_free(ctx, addr):
    try:
        if ctx._h:
            L.lib().emgpu_host_free(ctx._h, C.c_void_p(addr))
    except Exception:
        pass


class Trace:
    """emgpu_trace: device memory for the outputs of sample_dbn_device, allocated and PLACED by the library (emgpu_trace_alloc times the
    caller's own launch on a few candidate allocations and keeps the fastest: profiles/r05_placement_probe.txt).  `ptrs()` are the keyword
    arguments of sample_dbn_device / sample_dbn_blocks_device; `report` says what was measured."""

    def __init__(self, ctx, model, params, want=L.TRACE_INIT | L.TRACE_DENSE, candidates=0):
        self._ctx = ctx
        h = C.c_void_p()
        L.check(L.lib().emgpu_trace_alloc(ctx._h, model._h, C.byref(params), int(want), int(candidates), C.byref(h)))
        self._h = h
        o = L.SampleOut()
        L.check(L.lib().emgpu_trace_out(self._h, C.byref(o)))
        self.out = o
        r = L.TraceReport()
        L.check(L.lib().emgpu_trace_report(self._h, C.byref(r)))
        self.ld, self.bytes = int(r.ld), int(r.bytes)
        self.report = {"candidates": int(r.candidates), "kept": int(r.kept), "reused": int(r.reused),
                       "ms": [round(float(r.ms[i]), 3) for i in range(min(int(r.candidates), 8))] if r.candidates > 1 else [],
                       "first_allocation_ms": round(float(r.first_allocation_ms), 3), "kept_ms": round(float(r.kept_ms), 3)}

    def ptrs(self):
        o = self.out
        return dict(init_bin=o.init_bin or 0, init_val=o.init_val or 0, dyn_bin=o.dyn_bin or 0, dyn_val=o.dyn_val or 0,
                    ev_count=o.ev_count or 0, events=o.events or 0, attempts=o.attempts or 0, ld=int(o.ld))

    def free(self):
        """Back to the context's pool (the next Trace it fits takes it without a new probe)."""
        if self._h:
            L.check(L.lib().emgpu_trace_free(self._ctx._h, self._h))
            self._h = None

    def __del__(self):
        try:
            if self._h and self._ctx._h:
                L.lib().emgpu_trace_free(self._ctx._h, self._h)
                self._h = None
        except Exception:
            pass


_default_ctx = {}


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def all_device_contexts():
    """One default Context per visible device: pass the list as `ctx` to spread one call over every GPU."""
    return [default_context(d) for d in range(device_count())]


def make_params(n, sample_time, seed, first_index=0, transition_mode=L.TRANSITION_REFERENCE_AUTO, flags=0,
                max_attempts=1000, idx_L=0, idx_v=0, idx_dh=0, layers=None, event_cap=0, indices=None, start=None):
    """emgpu_sample_params.  indices: a numpy uint64 array (host calls) or a raw device pointer (device calls) of n
    global indices replacing first_index + i.  start: a start grid [n, n_initial] of preset bins (0 = unset), numpy (host calls) or a raw
    device pointer."""
    p = L.SampleParams()
    p.seed, p.first_index, p.n, p.sample_time = int(seed) & (2**64 - 1), int(first_index), int(n), int(sample_time)
    p.transition_mode, p.flags, p.max_attempts = int(transition_mode), int(flags), int(max_attempts)
    p.idx_L, p.idx_v, p.idx_dh = int(idx_L), int(idx_v), int(idx_dh)
    keep = None
    if layers is not None:
        keep = np.ascontiguousarray(np.asarray(layers, dtype=np.float64).reshape(-1, 2))
        p.layers, p.n_layers = _p(keep), keep.shape[0]
    p.event_cap = int(event_cap)
    if indices is not None:
        if isinstance(indices, int):
            p.indices = indices
        else:
            idx = np.ascontiguousarray(indices, dtype=np.uint64)
            assert idx.size == int(n)
            p.indices = idx.ctypes.data
            keep = (keep, idx)
    if start is not None:
        if isinstance(start, int):
            p.start = start
        else:
            st = np.ascontiguousarray(start, dtype=np.int32)
            assert st.ndim == 2 and st.shape[0] == int(n)
            p.start = st.ctypes.data
            keep = (keep, st)
    return p, keep


def device_count():
    c = C.c_int32(0)
    L.check(L.lib().emgpu_device_count(C.byref(c)))
    return int(c.value)


def shard_range(n_total, rank, world):
    """emgpu_shard_range: the split every sharded entry point uses (== sharding.shard_range)."""
    lo, hi = C.c_int64(0), C.c_int64(0)
    L.check(L.lib().emgpu_shard_range(int(n_total), int(rank), int(world), C.byref(lo), C.byref(hi)))
    return int(lo.value), int(hi.value)


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
    arr = (L.SampleOut * len(ctxs))()
    for d, kw in enumerate(outs):
        o = _sample_out(**kw)
        for f, _ in L.SampleOut._fields_:
            setattr(arr[d], f, getattr(o, f))
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
    G4 = (T + 3) // 4
    ctx0 = ctx[0] if isinstance(ctx, (list, tuple)) else ctx
    empty = ctx0.pinned_empty if pinned else (lambda shape, dt: np.zeros(shape, dtype=dt))
    o = L.SampleOut()
    ib = empty((ni, n), np.uint8)
    iv = empty((ni, n), np.float32)
    att = empty((n,), np.int32)
    o.init_bin, o.init_val, o.attempts = _p(ib), _p(iv), _p(att)
    if want_dense and nd > 0:
        db = empty((G4, nd, n), np.uint32)
        dv = empty((G4, nd, n, 4), np.float32)
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


def _event_cap_error(rc, totals, ev_count=None):
    """The EmgpuError of ERR_EVENT_CAP with the library's message, `.totals` (the room a retry needs) and `.ev_count` where there is one."""
    e = L.EmgpuError(rc, L.lib().emgpu_last_error().decode("utf-8", "replace"))
    e.totals = totals
    if ev_count is not None:
        e.ev_count = np.array(ev_count)
    return e


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
    empty = ctx.pinned_empty if pinned else (lambda shape, dt: np.empty(shape, dtype=dt))
    rows_empty = lambda cap_, shape, dt: (empty if cap_ is not None else (lambda sh, d: np.empty(sh, dtype=d)))(shape, dt)
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
    empty = ctx.pinned_empty if pinned else (lambda shape, dt: np.empty(shape, dtype=dt))
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
        iv = empty((ni, n), np.float32)
        o.init_val = _p(iv)
        if nd > 0:
            dv = empty(((T + 3) // 4, nd, n, 4), np.float32)
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
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    n = x.size
    cap = 12 * n if cap is None else int(cap)
    buf = np.empty(max(cap, 1), dtype=np.uint8)
    offs = np.zeros(n + 1, dtype=np.uint64)
    paths = np.zeros(2, dtype=np.uint64)
    if return_paths:
        L.check(L.lib().emgpu_debug_format_paths(ctx._h, _p(paths)))   # (reading clears)
    L.check(L.lib().emgpu_format_g_host(ctx._h, _p(x), n, _p(buf), cap, _p(offs)))
    text = buf[: int(offs[n])].tobytes().decode("ascii")
    o = offs.astype(np.int64).tolist()
    strings = [text[a:b] for a, b in zip(o[:-1], o[1:])]
    if return_paths:
        L.check(L.lib().emgpu_debug_format_paths(ctx._h, _p(paths)))
        return strings, (int(paths[0]), int(paths[1]))
    return strings


def split_rows(a, ends):
    """[a[0:ends[0]], a[ends[0]:ends[1]], ...] as views -- what np.split(a, ends[:-1]) returns, without its per-piece swapaxes round trip
    (a million pieces: 1 us each instead of 3)."""
    e = ends.tolist()
    return [a[s:t] for s, t in zip([0] + e[:-1], e)]


def unpack_dyn_bin(db, T):
    """[G4][nd][n] uint32 (4 seconds per word) -> [n, T, nd] uint8."""
    return unpack_dyn_val(db.view(np.uint8).reshape(db.shape + (4,)), T)     # little endian: byte w = column 4g+w


def unpack_dyn_val(dv, T):
    """[G4][nd][n][4] f32 -> [n, T, nd] f32."""
    G4, nd, n, _ = dv.shape
    return np.ascontiguousarray(dv.transpose(2, 0, 3, 1).reshape(n, G4 * 4, nd)[:, :T, :])


def pack_dyn_bin(db):
    """[n, T, nd] uint8 -> [G4][nd][n] uint32 (the inverse of unpack_dyn_bin; padding columns are 0)."""
    b = pack_dyn_val(np.asarray(db, dtype=np.uint8))
    return b.view(np.uint32).reshape(b.shape[:3])


def score_params(n, sample_time, transition_mode=L.TRANSITION_REFERENCE_AUTO, ld=0, col_offset=0):
    p = L.ScoreParams()
    p.n, p.sample_time, p.transition_mode, p.ld, p.col_offset = int(n), int(sample_time), int(transition_mode), int(ld), int(col_offset)
    return p


def score_dbn_device(ctx, model, params, init_bin, dyn_bin=0, log_lik=0, initial=0):
    """emgpu_score_dbn_device: asynchronous, raw device pointers (ints; dyn_bin 0 for sample_time 1 or a model without a transition network,
    initial 0 = not wanted).  log_lik / initial [n] f64 are not offset by col_offset.  A bin outside 1..r makes its trajectory NaN and the
    next ctx.sync() raise EmgpuError(ERR_ARG)."""
    L.check(L.lib().emgpu_score_dbn_device(ctx._h, model._h, C.byref(params), C.c_void_p(init_bin or None), C.c_void_p(dyn_bin or None),
                                           C.c_void_p(log_lik or None), C.c_void_p(initial or None)))


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
    if db is not None and (db.ndim != 3 or db.shape != ((int(T) + 3) // 4, model.n_dyn, ld)):
        raise ValueError("dyn_bin must hold T columns of n_dyn variables for the trajectories of init_bin")
    return ib, db, ld, n


def _raise(rc, **carried):
    """EmgpuError of a call's negative status and the library's message, carrying what the call has to show all the same"""
    e = L.EmgpuError(int(rc), L.lib().emgpu_last_error().decode("utf-8", "replace"))
    for k, v in carried.items():
        setattr(e, k, v)
    raise e


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
    L.check(L.lib().emgpu_count_dbn_device(ctx._h, model._h, C.byref(params), C.c_void_p(init_bin or None), C.c_void_p(dyn_bin or None),
                                           C.c_void_p(counts_initial or None), C.c_void_p(counts_transition or None)))


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
    sizes = [int(model.count_layout(network)[-1]) for network in (0, 1)]
    if counts is None:
        return [np.zeros(max(s, 1), dtype=np.uint64)[:s] for s in sizes]
    ci, ct = counts
    for a, s in ((ci, sizes[0]), (ct, sizes[1])):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint64 or a.shape != (s,) or not a.flags["C_CONTIGUOUS"]:
            raise ValueError("counts must be the `raw` pair of a count of this model: contiguous uint64 arrays of count_layout's lengths")
    return [ci, ct]


def _counts_result(model, ci, ct, pairs=None, **kernels):
    """the dict the counting calls return: the tables of the u64 arrays ci / ct, the two vectors of pairs = (u64 repeat, u64 change) where
    the call has them, and the kernels' names"""
    Ni, Nt = split_counts(model, (ci, ct))
    out = {"N_initial": Ni, "N_transition": Nt, "raw": (ci, ct)}
    if pairs is not None:
        out.update({"repeat": pairs[0].astype(np.float64), "change": pairs[1].astype(np.float64), "raw_pairs": pairs})
    out.update(kernels)
    return out


@contextlib.contextmanager
def _device_arrays(ctx, **nbytes):
    """One device block (emgpu_device_alloc) holding arrays of these sizes at 256-byte offsets, in the order given: {name: address}.  The
    block is freed when the scope ends, however it ends."""
    off, o = {}, 0
    for name, b in nbytes.items():
        off[name] = o
        o += (int(b) + 255) // 256 * 256
    base = ctx.device_alloc(max(o, 256))
    try:
        yield {k: base + v for k, v in off.items()}
    finally:
        ctx.device_free(base)


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


def sample_count_host(ctx, model, n, T, seed, transition_mode=L.TRANSITION_REFERENCE_AUTO, first_index=0, counts=None):
    """Sample n trajectories of T seconds into a device block (emgpu_sample_dbn_device), count them where they lie (emgpu_count_dbn_device)
    and bring back the tables alone: the trace never crosses PCIe.  The trace is the one sample_dbn_host(ctx, model, n, T, seed,
    transition_mode=..., first_index=...) returns, so the result equals count_dbn_host of that.  Returns count_dbn_host's dict, with
    `kernel` the sampler's and `count_kernel` the counting kernel's."""
    ni, nd, T, n = model.n_initial, model.n_dyn, int(T), int(n)
    G4 = (T + 3) // 4
    ci, ct = _counts_arrays(model, counts)
    with _device_arrays(ctx, init_bin=ni * n, init_val=4 * ni * n, dyn_bin=4 * G4 * nd * n, dyn_val=16 * G4 * nd * n, attempts=4 * n,
                        ci=8 * ci.size, ct=8 * ct.size) as at:
        for name, a in (("ci", ci), ("ct", ct)):
            if a.size:
                device_upload(ctx, at[name], np.zeros_like(a))
        p, keep = make_params(n, T, seed, first_index=first_index, transition_mode=transition_mode)
        dense = nd > 0
        sample_dbn_device(ctx, model, p, init_bin=at["init_bin"], init_val=at["init_val"], dyn_bin=at["dyn_bin"] if dense else 0,
                          dyn_val=at["dyn_val"] if dense else 0, attempts=at["attempts"])
        kernel = ctx.last_kernel()
        transitions = dense and T > 1
        count_dbn_device(ctx, model, score_params(n, T, p.transition_mode), at["init_bin"], at["dyn_bin"] if transitions else 0,
                         at["ci"], at["ct"] if transitions else 0)
        count_kernel = ctx.last_kernel()
        ctx.sync()                                  # both launches' deferred errors
        for name, a in (("ci", ci), ("ct", ct)):
            if a.size:
                a += device_download(ctx, at[name], np.zeros_like(a))
    del keep
    return _counts_result(model, ci, ct, kernel=kernel, count_kernel=count_kernel)


def count_dbn_weighted_device(ctx, model, params, init_bin, dyn_bin, weights, counts_initial=0, counts_transition=0):
    """emgpu_count_dbn_weighted_device: count_dbn_device in which every observation of trajectory i adds weights[i] -- a device array of
    params.n uint32, not offset by col_offset -- instead of 1.  A trajectory of weight 0 adds nothing and reports nothing, whatever its bins
    hold.  One call takes n * max(1, sample_time - 1) <= 2**32."""
    L.check(L.lib().emgpu_count_dbn_weighted_device(ctx._h, model._h, C.byref(params), C.c_void_p(init_bin or None), C.c_void_p(dyn_bin or None),
                                                    C.c_void_p(weights or None), C.c_void_p(counts_initial or None),
                                                    C.c_void_p(counts_transition or None)))


def _weights_array(weights, n):
    """a call's weights as contiguous uint32 [n]: an integer array of that shape with values in 0 .. 2**32 - 1, or ValueError"""
    w = np.asarray(weights)
    if w.dtype.kind not in "iu" or w.shape != (int(n),):
        raise ValueError("weights must be an integer array [n], one entry per trajectory (quantize_weights makes one from log-weights)")
    if w.size and (int(w.min()) < 0 or int(w.max()) > 2**32 - 1):
        raise ValueError("weights must lie in 0 .. 2**32 - 1")
    return np.ascontiguousarray(w, dtype=np.uint32)


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
    ni, nd, T, n = proposal.n_initial, proposal.n_dyn, int(T), int(n)
    G4 = (T + 3) // 4
    ci, ct = _counts_arrays(proposal, counts)
    with _device_arrays(ctx, init_bin=ni * n, init_val=4 * ni * n, dyn_bin=4 * G4 * nd * n, dyn_val=16 * G4 * nd * n, attempts=4 * n,
                        ll_p=8 * n, ll_t=8 * n, w=4 * n, ci=8 * ci.size, ct=8 * ct.size) as at:
        for name, a in (("ci", ci), ("ct", ct)):
            if a.size:
                device_upload(ctx, at[name], np.zeros_like(a))
        p, keep = make_params(n, T, seed, first_index=first_index, transition_mode=transition_mode)
        dense = nd > 0
        sample_dbn_device(ctx, proposal, p, init_bin=at["init_bin"], init_val=at["init_val"], dyn_bin=at["dyn_bin"] if dense else 0,
                          dyn_val=at["dyn_val"] if dense else 0, attempts=at["attempts"])
        kernel = ctx.last_kernel()
        sp = score_params(n, T, p.transition_mode)
        score_dbn_device(ctx, proposal, sp, at["init_bin"], at["dyn_bin"] if dense else 0, at["ll_p"])
        score_dbn_device(ctx, target, sp, at["init_bin"], at["dyn_bin"] if dense else 0, at["ll_t"])
        score_kernel = ctx.last_kernel()
        ctx.sync()                                  # the three launches' deferred errors
        ll_p = device_download(ctx, at["ll_p"], np.zeros(n, np.float64))
        ll_t = device_download(ctx, at["ll_t"], np.zeros(n, np.float64))
        w, log_scale = quantize_weights(ll_t - ll_p, bits)
        transitions = dense and T > 1
        count_kernel = ""
        if n > 0:
            device_upload(ctx, at["w"], w)
            count_dbn_weighted_device(ctx, proposal, sp, at["init_bin"], at["dyn_bin"] if transitions else 0, at["w"],
                                      at["ci"], at["ct"] if transitions else 0)
            count_kernel = ctx.last_kernel()
            ctx.sync()
            for name, a in (("ci", ci), ("ct", ct)):
                if a.size:
                    a += device_download(ctx, at[name], np.zeros_like(a))
    del keep
    s1, s2 = float(w.astype(np.float64).sum()), float((w.astype(np.float64) ** 2).sum())
    return _counts_result(proposal, ci, ct, weights=w, log_scale=log_scale, ess=s1 * s1 / s2 if s2 > 0 else 0.0, log_lik_proposal=ll_p,
                          log_lik_target=ll_t, kernel=kernel, score_kernel=score_kernel, count_kernel=count_kernel)


def pack_dyn_val(dv):
    """[n, T, nd] f32 or f64 -> [G4][nd][n][4] of the same dtype (the inverse of unpack_dyn_val; padding columns are 0)."""
    dv = np.asarray(dv)
    n, T, nd = dv.shape
    G4 = (T + 3) // 4
    b = np.zeros((n, G4 * 4, nd), dtype=dv.dtype)
    b[:, :T, :] = dv
    return np.ascontiguousarray(b.reshape(n, G4, 4, nd).transpose(1, 3, 0, 2))


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
    L.check(L.lib().emgpu_discretize_dbn_device(ctx._h, model._h, C.byref(params), C.c_void_p(init_val or None), C.c_void_p(dyn_val or None),
                                                C.c_void_p(init_bin or None), C.c_void_p(dyn_bin or None), C.c_void_p(repeat or None),
                                                C.c_void_p(change or None)))


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
        if dv.ndim != 4 or dv.shape[:2] != ((int(T) + 3) // 4, model.n_dyn) or dv.shape[3] != 4 or (iv is not None and dv.shape[2] != iv.shape[1]):
            raise ValueError("dyn_val must hold T columns of n_dyn variables for the trajectories of init_val")
    ld = iv.shape[1] if iv is not None else dv.shape[2]
    return iv, dv, ld, (L.VALUE_F64 if dt == np.float64 else L.VALUE_F32)


def _pair_vectors(model, counts):
    """the repeat / change vectors of a call: fresh zeros, or a previous result's `raw` (accumulated into, in place)"""
    if counts is None:
        return np.zeros(model.n_initial, dtype=np.uint64), np.zeros(model.n_initial, dtype=np.uint64)
    rep, chg = counts
    for a in (rep, chg):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint64 or a.shape != (model.n_initial,) or not a.flags["C_CONTIGUOUS"]:
            raise ValueError("counts must be the `raw` pair of a discretize of this model: contiguous uint64 arrays of n_initial entries")
    return rep, chg


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
    ib = None if iv is None else np.zeros(iv.shape, dtype=np.uint8)
    db = None if dv is None else np.zeros(dv.shape[:3], dtype=np.uint32)
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
    ni = model.n_initial
    ci, ct = _counts_arrays(model, None)
    rc = np.zeros(2 * ni, dtype=np.uint64)
    for name, a in (("ci", ci), ("ct", ct), ("rc", rc)):
        if a.size:
            device_upload(ctx, at[name], a)
    discretize_dbn_device(ctx, model, discretize_params(n, T, n_fine, value_type, wrap), at["init_val"], at["dyn_val"] if dense else 0,
                          at["init_bin"], at["dyn_bin"] if dense else 0, at["rc"] if n_fine else 0, at["rc"] + 8 * ni if n_fine else 0)
    kernel = ctx.last_kernel()
    transitions = dense and T > 1
    count_dbn_device(ctx, model, score_params(n, T, transition_mode), at["init_bin"], at["dyn_bin"] if transitions else 0,
                     at["ci"], at["ct"] if transitions else 0)
    count_kernel = ctx.last_kernel()
    ctx.sync()                                  # the launches' deferred errors
    for name, a in (("ci", ci), ("ct", ct), ("rc", rc)):
        if a.size:
            device_download(ctx, at[name], a)
    return _counts_result(model, ci, ct, (rc[:ni].copy(), rc[ni:].copy()), kernel=kernel, count_kernel=count_kernel, **kernels)


def _discretize_count_bytes(model, n, T, dense):
    """the arrays of _discretize_count_in_block besides the values, for _device_arrays"""
    return dict(init_bin=model.n_initial * n, dyn_bin=4 * ((T + 3) // 4) * model.n_dyn * n if dense else 0,
                ci=8 * int(model.count_layout(0)[-1]), ct=8 * int(model.count_layout(1)[-1]), rc=16 * model.n_initial)


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
    L.check(L.lib().emgpu_track_values_device(ctx._h if ctx is not None else None, C.byref(params), C.c_void_p(xyz or None),
                                              C.c_void_p(init_val or None), C.c_void_p(dyn_val or None)))


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
    T, dt = P - 2, (np.float64 if value_type == L.VALUE_F64 else np.float32)
    iv = np.zeros((int(n_initial), n), dtype=dt) if want_init else None
    dv = np.zeros(((max(T, 0) + 3) // 4, int(nd), n, 4), dtype=dt) if want_dyn else None
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
    G4 = (max(T, 0) + 3) // 4
    r0, slots = track_rows(model, rows)
    es, dt = (8, np.float64) if value_type == L.VALUE_F64 else (4, np.float32)
    iv = np.zeros((ni, n), dtype=dt)
    _fill_static(iv, static, [r for r in r0 if r >= 0])
    p = track_values_params(n, P, *unit_ratios, n_initial=ni, nd=nd, rows=r0, slots=slots, value_type=value_type, layout=L.TRACKS_ROWS)
    with _device_arrays(ctx, xyz=xyz.nbytes, init_val=iv.nbytes, dyn_val=4 * es * G4 * nd * n, **_discretize_count_bytes(model, n, T, True)) as at:
        for name, a in (("xyz", xyz), ("init_val", iv)):
            if a.size:
                device_upload(ctx, at[name], a)
        if nd > 3 and n:   # dynamic variables the tracks do not give: zeros, as track_values_host leaves them
            device_upload(ctx, at["dyn_val"], np.zeros(4 * G4 * nd * n, dtype=dt))
        track_values_device(ctx, p, at["xyz"], at["init_val"], at["dyn_val"])
        return _discretize_count_in_block(ctx, model, at, n, T, n_fine, value_type, wrap, transition_mode, True, values_kernel=ctx.last_kernel())


def miss_params(n_pairs, n_a, n_b, points, nmac_h_ft=500.0, nmac_v_ft=100.0, ld_a=0, ld_b=0):
    """emgpu_miss_params: n_pairs pairs of a column of set A (n_a columns, pitch ld_a, 0 = n_a) and a column of set B, `points` seconds each;
    the NMAC thresholds of track.m:175 in feet."""
    p = L.MissParams()
    p.n_pairs, p.n_a, p.n_b, p.ld_a, p.ld_b, p.points = int(n_pairs), int(n_a), int(n_b), int(ld_a), int(ld_b), int(points)
    p.nmac_h_ft, p.nmac_v_ft = float(nmac_h_ft), float(nmac_v_ft)
    return p


def miss_distance_device(params, xyz_a, xyz_b, idx_a=0, idx_b=0, pose_b=0, weights=0, hmd=0, vmd=0, t_cpa=0, flags=0, totals=0, stream=None):
    """emgpu_miss_distance_device: asynchronous, raw device pointers (ints, 0 = none; params: miss_params).  xyz_a / xyz_b f64 PLANAR
    [P, 3, ld], idx_a / idx_b int64 [n_pairs], pose_b f64 [5, n_pairs] (make_pose), weights uint32 [n_pairs]; hmd / vmd f64, t_cpa int32,
    flags uint8 [n_pairs] each, totals uint64 [8], ADDED to.  The call takes no context: it runs on the current device and on `stream`, a
    raw hipStream_t (0: the HIP default stream; None: torch's current stream).  To stay ordered behind a sampler, pass the stream its
    Context was given (Context.stream)."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    L.check(L.lib().emgpu_miss_distance_device(C.c_void_p(int(stream) or None), C.byref(params), *(C.c_void_p(int(a) or None) for a in (
        xyz_a, xyz_b, idx_a, idx_b, pose_b, weights, hmd, vmd, t_cpa, flags, totals))))


def make_pose(heading_deg, ox=0.0, oy=0.0, oz=0.0):
    """The pose_b of miss_distance: [5, n] float64 on the host, rows cos, sin of heading_deg (counter-clockwise, MATLAB's cosd / sind: the
    reduction in degrees of CorTerminalModel._sincosd, so that multiples of 90 give exact 0 and +-1), then the offsets ox, oy, oz in feet.
    Track B is turned about its own origin by the heading, then moved by the offset.  The arguments broadcast against each other."""
    from .encounter_model import CorTerminalModel
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
    dev, stream (resolved; None: torch's current stream), the PLANAR device tensors a / b, n_a, n_b, n_pairs, and d_ia, d_ib (int64), d_w
    (uint32 held as int32) and d_pose on the device or None.  columns = _pair_columns(...), w = _weights_array(...) or None: the caller has
    them before torch.cuda is touched.  The body runs on dev with the uploads complete for its stream; leaving it waits for that stream."""
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
        pr = types.SimpleNamespace(dev=dev, stream=stream, a=a, b=b, n_a=n_a, n_b=n_b, n_pairs=n_pairs, d_ia=up(idx[0], torch.int64),
                                   d_ib=up(idx[1], torch.int64), d_pose=up(pose_b, torch.float64),
                                   d_w=None if w is None else torch.from_numpy(w.view(np.int32)).to(dev))
        # torch.cuda.synchronize brackets the launches only when they do not run on torch's stream, where the uploads ran
        pr.guard = (lambda: None) if stream is None else (lambda: torch.cuda.synchronize(dev))
        pr.guard()
        yield pr
        pr.guard()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _miss_tensors(pr, d_pose, d_w, nmac_h_ft, nmac_v_ft):
    """k_miss_distance on the pairing pr with the device tensors d_pose and d_w (or None): the device tensors (hmd, vmd, t_cpa, flags,
    totals), launched on pr.stream and not waited for"""
    import torch
    n, dev = pr.n_pairs, pr.dev
    hmd, vmd = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    t_cpa, flags = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    totals = torch.zeros(8, dtype=torch.int64, device=dev)
    pr.guard()      # totals was zeroed on torch's stream
    miss_distance_device(miss_params(n, pr.n_a, pr.n_b, pr.a.shape[0], nmac_h_ft, nmac_v_ft), _ptr(pr.a), _ptr(pr.b), _ptr(pr.d_ia), _ptr(pr.d_ib),
                         _ptr(d_pose), _ptr(d_w), _ptr(hmd), _ptr(vmd), _ptr(t_cpa), _ptr(flags), _ptr(totals), stream=pr.stream)
    return hmd, vmd, t_cpa, flags, totals


def _miss_dict(hmd, vmd, t_cpa, flags, totals):
    """miss_distance's dict from _miss_tensors' device tensors"""
    fl = flags.cpu().numpy()
    return {"hmd_ft": hmd.cpu().numpy(), "vmd_ft": vmd.cpu().numpy(), "t_cpa": t_cpa.cpu().numpy(), "flags": fl,
            "nmac": (fl & L.MISS_NMAC_CPA) != 0, "totals": totals.cpu().numpy().view(np.uint64)}


def _encounter_pose_tensors(pr, want_weights, radius_ft, half_height_ft, seed, rate_scale, first_index, max_attempts):
    """k_encounter_pose on the pairing pr: the device tensors (pose [5, n_pairs], rate, flags, weights or None), launched on pr.stream and
    not waited for"""
    import torch
    n, dev = pr.n_pairs, pr.dev
    pose = torch.empty((5, n), dtype=torch.float64, device=dev)
    rate = torch.empty(n, dtype=torch.float64, device=dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    w_out = torch.empty(n, dtype=torch.int32, device=dev) if want_weights else None
    p = encounter_params(n, pr.n_a, pr.n_b, pr.a.shape[0], radius_ft, half_height_ft, seed, first_index, max_attempts,
                         1.0 if rate_scale is None else rate_scale)
    encounter_pose_device(p, _ptr(pr.a), _ptr(pr.b), _ptr(pr.d_ia), _ptr(pr.d_ib), _ptr(pr.d_w), _ptr(pose), _ptr(rate), _ptr(flags), _ptr(w_out),
                          stream=pr.stream)
    return pose, rate, flags, w_out


def _encounter_dict(rate, flags, w_out, flags_key="flags"):
    """the rate, flags and weights of encounter_pose's dict from _encounter_pose_tensors' device tensors"""
    return {"rate": rate.cpu().numpy(), flags_key: flags.cpu().numpy(), "weights": None if w_out is None else w_out.cpu().numpy().view(np.uint32)}


def _encounter_weights(weights, rate_scale, n_pairs):
    """(whether weights_out is wanted, weights_in as _weights_array or None) of encounter_pose's `weights`"""
    want = weights is not None and weights is not False
    if want and rate_scale is None:
        raise ValueError("weights need a rate_scale: the rate that leaves a weight as it is")
    return want, _weights_array(weights, n_pairs) if want and weights is not True else None


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
    import torch
    columns = _pair_columns(xyz_a, xyz_b, idx_a, idx_b, layout)
    w = None if weights is None else _weights_array(weights, columns[3])
    if pose_b is not None:
        pose_b = np.ascontiguousarray(pose_b, dtype=np.float64) if not isinstance(pose_b, torch.Tensor) else pose_b
        if tuple(pose_b.shape) != (5, columns[3]):
            raise ValueError("pose_b must be [5, n_pairs] (make_pose)")
    with _paired(xyz_a, xyz_b, columns, w, pose_b, layout, ctx, stream) as pr:
        out = _miss_tensors(pr, pr.d_pose, pr.d_w, nmac_h_ft, nmac_v_ft)
    return _miss_dict(*out)


def encounter_params(n_pairs, n_a, n_b, points, radius_ft, half_height_ft, seed, first_index=0, max_attempts=16, rate_scale=1.0, ld_a=0, ld_b=0):
    """emgpu_encounter_params: n_pairs pairs of a column of set A (the ownship; n_a columns, pitch ld_a, 0 = n_a) and a column of set B (the
    intruder), an encounter cylinder of radius_ft and half_height_ft around the ownship, the seed and the global index of pair 0;
    rate_scale divides the rate where it is folded into weights_out."""
    p = L.EncounterParams()
    p.n_pairs, p.n_a, p.n_b, p.ld_a, p.ld_b, p.points = int(n_pairs), int(n_a), int(n_b), int(ld_a), int(ld_b), int(points)
    p.max_attempts, p.seed, p.first_index = int(max_attempts), int(seed) & (2**64 - 1), int(first_index) & (2**64 - 1)
    p.radius_ft, p.half_height_ft, p.rate_scale = float(radius_ft), float(half_height_ft), float(rate_scale)
    return p


def encounter_pose_device(params, xyz_a, xyz_b, idx_a=0, idx_b=0, weights_in=0, pose=0, rate=0, flags=0, weights_out=0, stream=None):
    """emgpu_encounter_pose_device: asynchronous, raw device pointers (ints, 0 = none; params: encounter_params).  xyz_a / xyz_b f64 PLANAR
    [P, 3, ld] (points 0 and 1 are read), idx_a / idx_b int64 [n_pairs], weights_in uint32 [n_pairs]; pose f64 [5, n_pairs] (what
    miss_distance_device takes as pose_b), rate f64, flags uint8 (L.ENC_*), weights_out uint32 [n_pairs] each.  No context: the current
    device and `stream`, a raw hipStream_t (0: the HIP default stream; None: torch's current stream)."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    L.check(L.lib().emgpu_encounter_pose_device(C.c_void_p(int(stream) or None), C.byref(params), *(C.c_void_p(int(a) or None) for a in (
        xyz_a, xyz_b, idx_a, idx_b, weights_in, pose, rate, flags, weights_out))))


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
    return {"pose": pose.cpu().numpy(), **_encounter_dict(*out)}


def encounter_miss(xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a=None, idx_b=None, weights=None, rate_scale=None, first_index=0,
                   max_attempts=16, nmac_h_ft=500.0, nmac_v_ft=100.0, layout="rows", ctx=None, stream=None):
    """encounter_pose and then miss_distance on one stream, the pose and the rate-folded weights never leaving the device: the intruders
    placed on the encounter cylinder, then HMD, VMD, CPA time and NMAC flags of the pairs.  The arguments are encounter_pose's and the
    NMAC thresholds.  With weights (and rate_scale) totals[5:8] are sums of w * rate / rate_scale, so totals[6] / totals[5] is
    P(NMAC | encounter); without, every pair counts 1 there.
    Returns miss_distance's dict plus "rate" float64, "encounter_flags" uint8 (L.ENC_*) and "weights" uint32 or None."""
    columns = _pair_columns(xyz_a, xyz_b, idx_a, idx_b, layout)
    want_weights, w = _encounter_weights(weights, rate_scale, columns[3])
    with _paired(xyz_a, xyz_b, columns, w, None, layout, ctx, stream) as pr:
        pose, rate, eflags, w_out = _encounter_pose_tensors(pr, want_weights, radius_ft, half_height_ft, seed, rate_scale, first_index, max_attempts)
        out = _miss_tensors(pr, pose, w_out, nmac_h_ft, nmac_v_ft)
    return dict(_miss_dict(*out), **_encounter_dict(rate, eflags, w_out, "encounter_flags"))


def device_upload(ctx, addr, src):
    """emgpu_device_upload: the numpy array `src` into device memory at addr, on the context's stream; complete on return."""
    src = np.ascontiguousarray(src)
    L.check(L.lib().emgpu_device_upload(ctx._h, C.c_void_p(int(addr)), _p(src), src.nbytes))


def device_download(ctx, addr, out):
    """emgpu_device_download: out.nbytes bytes of device memory at addr (an emgpu_device_alloc block, a trace) into the contiguous numpy
    array `out`, behind the launches already issued on the context's stream; complete on return.  Returns out."""
    assert out.flags["C_CONTIGUOUS"]
    L.check(L.lib().emgpu_device_download(ctx._h, _p(out), C.c_void_p(int(addr)), out.nbytes))
    return out


def _same_shape(a, b):
    tm_a, tm_b = a.get_i32(L.F_TEMPORAL_MAP).reshape(-1, 2), b.get_i32(L.F_TEMPORAL_MAP).reshape(-1, 2)
    if a.n_initial != b.n_initial or not np.array_equal(a.get_i32(L.F_R_INITIAL), b.get_i32(L.F_R_INITIAL)):
        return False
    if not np.array_equal(tm_a, tm_b):
        return False
    return bool(np.array_equal(a.get_i32(L.F_R_TRANSITION)[tm_a[:, 1] - 1], b.get_i32(L.F_R_TRANSITION)[tm_b[:, 1] - 1])) if len(tm_a) else True


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
    G4 = (T + 3) // 4
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
    sizes = [("init_bin", ni * n), ("init_val", 4 * ni * n), ("dyn_bin", 4 * G4 * nd * n), ("dyn_val", 16 * G4 * nd * n), ("attempts", 4 * n),
             ("ll_p", 8 * n), ("ll_t", 8 * n), ("lw", 8 * n), ("start", 4 * ni * n if start is not None else 0),
             ("indices", 8 * n if indices is not None else 0)]
    off, o = {}, 0
    for name, b in sizes:
        off[name] = o
        o += (b + 255) // 256 * 256
    base = ctx.device_alloc(max(o, 256))
    try:
        at = {k: base + v for k, v in off.items()}
        if start is not None:
            device_upload(ctx, at["start"], start)
        if indices is not None:
            device_upload(ctx, at["indices"], indices)
        p, keep = make_params(n, T, seed, first_index=first_index, transition_mode=transition_mode, flags=flags, max_attempts=max_attempts,
                              idx_L=idx_L, idx_v=idx_v, idx_dh=idx_dh, layers=layers, indices=at["indices"] if indices is not None else None,
                              start=at["start"] if start is not None else None)
        dense = nd > 0
        sample_dbn_device(ctx, proposal, p, init_bin=at["init_bin"], init_val=at["init_val"], dyn_bin=at["dyn_bin"] if dense else 0,
                          dyn_val=at["dyn_val"] if dense else 0, attempts=at["attempts"], log_weight=at["lw"] if want_log_weight else 0)
        kernel = ctx.last_kernel()
        sp = score_params(n, T, p.transition_mode)
        score_dbn_device(ctx, proposal, sp, at["init_bin"], at["dyn_bin"] if dense else 0, at["ll_p"])
        score_dbn_device(ctx, target, sp, at["init_bin"], at["dyn_bin"] if dense else 0, at["ll_t"])
        out = {"kernel": kernel, "score_kernel": ctx.last_kernel()}
        ctx.sync()                                  # the three launches' deferred errors
        ib = device_download(ctx, at["init_bin"], np.zeros((ni, n), np.uint8))
        iv = device_download(ctx, at["init_val"], np.zeros((ni, n), np.float32))
        out["attempts"] = device_download(ctx, at["attempts"], np.zeros(n, np.int32))
        out["init_bin"], out["init_val"] = (ib, iv) if raw else (ib.T.copy(), iv.T.copy())
        if dense:
            db = device_download(ctx, at["dyn_bin"], np.zeros((G4, nd, n), np.uint32))
            dv = device_download(ctx, at["dyn_val"], np.zeros((G4, nd, n, 4), np.float32))
            out["dyn_bin"] = db if raw else unpack_dyn_bin(db, T)
            out["dyn_val"] = dv if raw else unpack_dyn_val(dv, T)
        if want_log_weight:
            out["log_weight"] = device_download(ctx, at["lw"], np.zeros(n, np.float64))
        out["log_lik_proposal"] = device_download(ctx, at["ll_p"], np.zeros(n, np.float64))
        out["log_lik_target"] = device_download(ctx, at["ll_t"], np.zeros(n, np.float64))
        out["log_weight_model"] = out["log_lik_target"] - out["log_lik_proposal"]
    finally:
        ctx.device_free(base)
    del keep
    return out


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
    dl = np.asarray(dyn_limits, dtype=np.float64).reshape(10)
    for i in range(10):
        p.dyn_limits[i] = float(dl[i])
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
    p = utrack_params(model, n, sample_time, seed, **kw)
    L.check(L.lib().emgpu_track_uncor_grid_device(ctx._h, model._h, C.byref(p), C.c_void_p(start or None), C.c_void_p(tracks or None),
                                                  C.c_void_p(limits or None), C.c_void_p(attempts or None)))
    return ctx.last_kernel()


def uncor_dynamic_limits(model, initial, up_min, up_max, speed_min, speed_max, is_rotorcraft=False):
    """emgpu_uncor_dynamic_limits: getDynamicLimits.m for one trajectory (host only, no GPU needed)."""
    p = utrack_params(model, 1, 1, 0, is_rotorcraft=is_rotorcraft)
    iv = np.ascontiguousarray(initial, dtype=np.float64)
    out = np.zeros(3)
    L.check(L.lib().emgpu_uncor_dynamic_limits(model._h, C.byref(p), _p(iv), float(up_min), float(up_max), float(speed_min), float(speed_max), _p(out)))
    return out


TERMINAL_GEO_FIELDS = ("distance", "bearing", "alt", "speed", "heading", "intent")


def _fill_terminal(p, geom_model, n, seed, first_index, tmax_s, dyn_limits, bounds_sample, max_attempts, max_resample, local_smooth):
    """The fields emgpu_tsample_params and emgpu_ttrack_params share, into either; returns the keep-alive of bounds_sample."""
    labels = [s.strip('"') for s in geom_model.get_labels(L.F_LABELS_INITIAL)]
    p.seed, p.first_index, p.n, p.tmax_s = int(seed) & (2**64 - 1), int(first_index), int(n), float(tmax_s)
    p.max_resample, p.max_attempts = int(max_resample), int(max_attempts)
    p.flags = L.FLAG_LOCAL_SMOOTH if local_smooth else 0
    for i, v in enumerate(np.asarray(dyn_limits, dtype=np.float64).reshape(10)):
        p.dyn_limits[i] = float(v)
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
    L.check(L.lib().emgpu_sample_terminal_device(ctx._h, geom_model._h, handles, 10, C.byref(p), C.c_void_p(geom_bin), C.c_void_p(geom_val),
                                                 C.c_void_p(geo), C.c_void_p(model_of), C.c_void_p(traj), C.c_void_p(rows), C.c_void_p(attempts)))


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
    msg = L.lib().emgpu_last_error().decode("utf-8", "replace")
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
        e = L.EmgpuError(rc, L.lib().emgpu_last_error().decode("utf-8", "replace"))
        e.rows = int(rows.value)
        raise e
    L.check(rc)
    table = out[: int(rows.value)]
    if rows_cap is None and table.shape[0] < out.shape[0] // 2:
        table = table.copy()
    return (table, {"rows": int(rows.value), "hard_tokens": int(hard.value)}) if return_stats else table


def format_f0(ctx, x, cap=None):
    """emgpu_format_f0_host: "%0.0f" of every double of x by the device function the CSV rows use.  Returns the list of strings; a value the
    device does not format (not finite, or 2^63 and more in magnitude) gives None."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    cap = 20 * n if cap is None else int(cap)
    buf = np.empty(max(cap, 1), dtype=np.uint8)
    offs = np.zeros(n + 1, dtype=np.uint64)
    L.check(L.lib().emgpu_format_f0_host(ctx._h, _p(x), n, _p(buf), cap, _p(offs)))
    text = buf[: int(offs[n])].tobytes().decode("ascii")
    o = offs.astype(np.int64).tolist()
    return [text[a:b] if b > a else None for a, b in zip(o[:-1], o[1:])]


def csv_bound(n, rows):
    """emgpu_csv_bound: bytes that always hold the CSV text of n tracks with `rows` position rows in all: 22 n + 74 rows."""
    return int(L.lib().emgpu_csv_bound(int(n), int(rows)))


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


def sample2track_device(ctx, params, alt0, speed0, dyn_val, xyz=0, flags=0, speed_minmax=0):
    """emgpu_sample2track_device with raw device pointers (ints, 0 = skip an output): consumes the sampler's
    device output in place (alt0 / speed0 = rows of init_val, dyn_val = the dense trace).  Asynchronous."""
    L.check(L.lib().emgpu_sample2track_device(ctx._h, C.byref(params), alt0, speed0, dyn_val, xyz or None, flags or None,
                                              speed_minmax or None))
