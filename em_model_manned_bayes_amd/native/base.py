"""The handles of the C ABI -- NativeModel (emgpu_model*), Context (emgpu_ctx*), Trace (emgpu_trace*) -- and what every other module of
the package calls the library with: the parameter block, the one error constructor, the one form of a device call, device memory.
"""
import contextlib
import ctypes as C

import numpy as np

from .. import _lib as L

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


def _last_message():
    return L.lib().emgpu_last_error().decode("utf-8", "replace")


def _error(rc, **carried):
    """The EmgpuError of a call's status and the library's message, carrying as attributes what the call has to show all the same"""
    e = L.EmgpuError(int(rc), _last_message())
    for k, v in carried.items():
        setattr(e, k, v)
    return e


def _raise(rc, **carried):
    """EmgpuError of a call's negative status and the library's message, carrying what the call has to show all the same"""
    raise _error(rc, **carried)


def _event_cap_error(rc, totals, ev_count=None):
    """The EmgpuError of ERR_EVENT_CAP with the library's message, `.totals` (the room a retry needs) and `.ev_count` where there is one."""
    return _error(rc, totals=totals, **({} if ev_count is None else {"ev_count": np.array(ev_count)}))


def _device_call(entry, handles, params, *ptrs):
    """emgpu_<entry>(handles..., &params, pointers...): the one form of the asynchronous device entry points.  handles: a Context or a
    NativeModel (None: NULL), anything else as it is (a raw hipStream_t, an array of handles and its length); pointers: raw device addresses
    as ints, 0 or None = NULL.  A negative status raises EmgpuError."""
    L.check(getattr(L.lib(), "emgpu_" + entry)(*(getattr(h, "_h", h) for h in handles), C.byref(params),
                                               *(C.c_void_p(int(a or 0) or None) for a in ptrs)))


def _stream_handle(stream):
    """a raw hipStream_t as a context-free device call takes it: None is torch's current stream, 0 the HIP default stream (NULL)"""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    return int(stream) or None


def _array_factory(ctx, pinned, pageable):
    """empty(shape, dtype) of a host-path call's output arrays: the context's pinned pool, or the pageable numpy constructor (np.zeros,
    np.empty) of the caller's choice"""
    return ctx.pinned_empty if pinned else (lambda shape, dt: pageable(shape, dtype=dt))


def _weights_array(weights, n):
    """a call's weights as contiguous uint32 [n]: an integer array of that shape with values in 0 .. 2**32 - 1, or ValueError"""
    w = np.asarray(weights)
    if w.dtype.kind not in "iu" or w.shape != (int(n),):
        raise ValueError("weights must be an integer array [n], one entry per trajectory (quantize_weights makes one from log-weights)")
    if w.size and (int(w.min()) < 0 or int(w.max()) > 2**32 - 1):
        raise ValueError("weights must lie in 0 .. 2**32 - 1")
    return np.ascontiguousarray(w, dtype=np.uint32)


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

