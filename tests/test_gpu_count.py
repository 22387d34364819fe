"""-m gpu: k_count_dbn against the numpy restatement of its definition (count_ref.count).  Counts are integers, so every comparison is exact
equality whatever the kernel's accumulation scheme does (run lengths per lane, LDS partials per workgroup, 64-bit global adds).  Traces come
from native.sample_dbn_host or are built by hand; each is counted by emgpu_count_dbn_host and by emgpu_count_dbn_device."""
import math

import numpy as np
import pytest

import count_ref as R
import score_ref as S
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native, synthetic
from em_model_manned_bayes_amd import encounter_model as E

pytestmark = pytest.mark.gpu

N, SEED = 777, 0xC0117
AUTO, PER_STEP = L.TRANSITION_REFERENCE_AUTO, L.TRANSITION_PER_STEP
GUARD = 0x5A5A5A5A5A5A5A5A
_paths, _traces, _refs = {}, {}, {}


def _model(name, model_dir):
    """(a fresh NativeModel, parms, graph) of the model's .txt: tests that change the model change their own copy"""
    if name not in _paths:
        if name == "synthetic_terminal":
            _paths[name] = model_dir + "/synthetic_terminal.txt"
            em_io.em_write(synthetic.terminal_trajectory_model(0x5EED), _paths[name])
        else:
            _paths[name] = em_io.materialize_model(name, model_dir)
    parms = em_io.em_read(_paths[name])
    return parms["native"], parms, R.graph(parms)


def _trace(ctx, name, model_dir, n, T, mode=AUTO):
    """a trace of the model drawn once and shared (raw layout, read-only), with the model it was drawn from"""
    key = (name, n, T, mode)
    if key not in _traces:
        nm, parms, g = _model(name, model_dir)
        got = native.sample_dbn_host(ctx, nm, n, T, SEED, raw=True, pinned=False, transition_mode=mode)
        _traces[key] = (nm, parms, g, got["init_bin"].copy(), got["dyn_bin"].copy())
        for a in _traces[key][3:]:
            a.setflags(write=False)
    return _traces[key]


def _ref(key, g, ib, db, T, mode, nt):
    """count_ref of a raw trace as the library's two flat arrays and the skipped observations; computed once per key and left unchanged"""
    if key is None or key not in _refs:
        Ni, Nt, skipped = R.count(g, ib.T, None if db is None else native.unpack_dyn_bin(db, T), mode, n_transition=nt)
        got = (R.flat(Ni), R.flat(Nt), skipped)
        for a in got[:2]:
            a.setflags(write=False)
        if key is None:
            return got
        _refs[key] = got
    return _refs[key]


def _name(g, mode):
    return "k_count_dbn[per-step]" if (mode == PER_STEP or g["depend"]) else "k_count_dbn[frozen]"


def _device(ctx, nm, ib, db, n, T, mode, ld=0, col=0, sync=True, start=None, want_t=True):
    """emgpu_count_dbn_device over device copies of the raw arrays, into buffers holding `start` (default zeros) with 4 guard words behind
    each, which must stay.  Returns (initial array, transition array, kernel, the error of ctx.sync() or None)."""
    import torch
    dev = torch.device("cuda", 0)
    d_ib = torch.from_numpy(np.array(ib, order="C")).to(dev)
    d_db = None if db is None else torch.from_numpy(np.array(db, order="C").view(np.int32)).to(dev)
    bufs = []
    for network in (0, 1):
        size = int(nm.count_layout(network)[-1])
        h = np.full(size + 4, GUARD, dtype=np.uint64)
        h[:size] = 0 if start is None else start[network]
        bufs.append((size, torch.from_numpy(h.view(np.int64)).to(dev)))
    torch.cuda.synchronize()
    native.count_dbn_device(ctx, nm, native.score_params(n, T, mode, ld, col), d_ib.data_ptr(), 0 if d_db is None else d_db.data_ptr(),
                            bufs[0][1].data_ptr(), bufs[1][1].data_ptr() if want_t else 0)
    kernel = ctx.last_kernel()
    err = None
    if sync:
        try:
            ctx.sync()
        except L.EmgpuError as e:
            err = e
    torch.cuda.synchronize()
    out = []
    for size, t in bufs:
        h = t.cpu().numpy().view(np.uint64)
        assert np.all(h[size:] == GUARD)
        out.append(h[:size].copy())
    return out[0], out[1], kernel, err


def _check(ctx, nm, g, ib, db, T, mode, key=None, expect_skips=False):
    """host and device counts of the raw trace (ib [ni, n], db [G4, nd, n] or None) equal the reference's"""
    n = ib.shape[1]
    want_i, want_t, skipped = _ref(key, g, ib, db, T, mode, nm.n_transition)
    assert (skipped > 0) == expect_skips
    try:
        host = native.count_dbn_host(ctx, nm, ib, db, T, mode, raw=True)
        assert not expect_skips
    except L.EmgpuError as e:
        assert expect_skips and e.code == L.ERR_ARG and "outside 1..r" in str(e)
        host = e.counts
    assert host["kernel"] == _name(g, mode), host["kernel"]
    assert np.array_equal(host["raw"][0], want_i) and np.array_equal(host["raw"][1], want_t)
    ci, ct, kernel, err = _device(ctx, nm, ib, db, n, T, mode)
    assert (err is not None) == expect_skips and kernel == _name(g, mode)
    assert np.array_equal(ci, want_i) and np.array_equal(ct, want_t)
    return want_i, want_t


# ---- 1. sampled traces
@pytest.mark.parametrize("name,mode", [("uncor_1200code_v2p1", AUTO), ("uncor_1200code_v2p1", PER_STEP), ("uncor_1200code_v1", AUTO),
                                       ("glider_v1", AUTO), ("cor_v1", AUTO)])
def test_counts_of_sampled_traces(gpu_ctx, model_dir, name, mode):
    T = 61
    nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, N, T, mode)
    assert g["depend"] == (name in ("uncor_1200code_v1", "glider_v1", "cor_v1"))
    if name == "cor_v1":
        assert nm.n_initial == 16
    want_i, want_t = _check(gpu_ctx, nm, g, ib, db, T, mode, key=(name, N, T, mode))
    assert int(want_i.sum()) == N * nm.n_initial and int(want_t.sum()) == N * (T - 1) * nm.n_dyn     # every observation, once
    # the user-facing shapes give the same tables, in the shapes of the model's own N
    user = native.count_dbn_host(gpu_ctx, nm, ib.T, native.unpack_dyn_bin(db, T), T, mode)
    assert np.array_equal(R.flat(user["N_initial"]), want_i) and np.array_equal(R.flat(user["N_transition"]), want_t)
    shp_i, shp_t = R.shapes(g)
    for v in range(nm.n_initial):
        Nv = user["N_initial"][v]
        assert Nv.shape == shp_i[v] and Nv.size == nm.get_f64(L.F_N_INITIAL, v + 1).size and Nv.dtype == np.float64
    for v in range(nm.n_transition):
        Nv = user["N_transition"][v]
        assert Nv.shape == shp_t.get(v, (0, 0)) and Nv.size == nm.get_f64(L.F_N_TRANSITION, v + 1).size
    if name == "glider_v1":            # the class layer, in the argument order of setParameters
        m = E.EncounterModel(_paths[name], idxZeroBoundaries=(1, 2, 3))
        Ni, Nt, rep, chg = m.count(ib.T, native.unpack_dyn_bin(db, T), ctx=gpu_ctx)
        assert rep is None and chg is None
        assert np.array_equal(R.flat(Ni), want_i) and np.array_equal(R.flat(Nt), want_t)
        Ni, Nt, _, _ = m.count(ib.T, ctx=gpu_ctx)
        assert np.array_equal(R.flat(Ni), want_i) and not R.flat(Nt).any()


def test_counts_of_the_terminal_geometry_model(gpu_ctx, model_dir):
    nm, parms, g = _model("terminal_v3_radar_encounter_model", model_dir)
    assert nm.n_transition == 0 and nm.n_dyn == 0
    bins, _, _ = native.sample_bn_host(gpu_ctx, nm, N, SEED)
    ib = np.ascontiguousarray(bins.T)
    want_i, want_t = _check(gpu_ctx, nm, g, ib, None, 1, AUTO)
    assert want_t.size == 0 and int(want_i.sum()) == N * nm.n_initial
    _check(gpu_ctx, nm, g, ib, None, 7, AUTO)            # no transition network: sample_time is of no consequence


# ---- 2. the packed-word edges
@pytest.mark.parametrize("T", [1, 2, 4, 5, 61])
@pytest.mark.parametrize("name", ["uncor_1200code_v2p1", "glider_v1"])
def test_sample_times_around_the_packed_word(gpu_ctx, model_dir, name, T):
    nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, N, T, AUTO)
    want_i, want_t = _check(gpu_ctx, nm, g, ib, db, T, AUTO, key=(name, N, T, AUTO))
    assert int(want_t.sum()) == N * (T - 1) * nm.n_dyn
    if T == 1:                                          # the transition array is left untouched, whatever it holds
        start = (np.zeros_like(want_i), np.full_like(want_t, 7))
        ci, ct, _, err = _device(gpu_ctx, nm, ib, db, N, 1, AUTO, start=start)
        assert err is None and np.array_equal(ci, want_i) and np.all(ct == 7)
        _check(gpu_ctx, nm, g, ib, None, 1, AUTO)      # dyn_bin may be absent
    else:                                               # the first T columns of a longer trace: padding bytes and later columns are not read
        _, _, _, ib2, db2 = _trace(gpu_ctx, name, model_dir, N, 61, AUTO)
        cut = np.ascontiguousarray(db2[:(T + 3) // 4])
        ref_i, ref_t, _ = _ref(None, g, ib2, np.ascontiguousarray(native.pack_dyn_bin(native.unpack_dyn_bin(db2, 61)[:, :T])), T, AUTO,
                               nm.n_transition)
        got = native.count_dbn_host(gpu_ctx, nm, ib2, cut, T, AUTO, raw=True)
        assert np.array_equal(got["raw"][0], ref_i) and np.array_equal(got["raw"][1], ref_t)


# ---- 3. the wave and workgroup edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 777])
def test_batch_sizes(gpu_ctx, model_dir, n):
    for name, mode in (("uncor_1200code_v2p1", PER_STEP), ("cor_v1", AUTO)):
        nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, n, 5, mode)
        _check(gpu_ctx, nm, g, ib, db, 5, mode, key=(name, n, 5, mode))


# ---- 4. everyone on the same cells: the smallest input at which a lost or doubled add of the LDS partials (a small table: every lane of
# every workgroup on one ds_add cell) or of the global adds (a large table: 4096 lanes on one address) shows
@pytest.mark.parametrize("mode", [AUTO, PER_STEP])
def test_everyone_on_the_same_cells(gpu_ctx, model_dir, mode):
    T, K = 61, 4096
    nm, parms, g, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T, mode)
    one_i, one_t, _ = _ref(None, g, ib[:, 5:6], db[:, :, 5:6], T, mode, nm.n_transition)
    rep_ib, rep_db = np.ascontiguousarray(np.repeat(ib[:, 5:6], K, axis=1)), np.ascontiguousarray(np.repeat(db[:, :, 5:6], K, axis=2))
    for got in (native.count_dbn_host(gpu_ctx, nm, rep_ib, rep_db, T, mode, raw=True)["raw"], _device(gpu_ctx, nm, rep_ib, rep_db, K, T, mode)[:2]):
        assert np.array_equal(got[0], one_i * np.uint64(K)) and np.array_equal(got[1], one_t * np.uint64(K))
    assert int(one_t.max()) > 1                                           # a run of the run-length form is in it
    # two rows only, alternating: every table's adds fall on at most two cells
    alt = np.arange(K) % 2
    two_ib, two_db = np.ascontiguousarray(ib[:, 5 + alt]), np.ascontiguousarray(db[:, :, 5 + alt])
    a_i, a_t, _ = _ref(None, g, ib[:, 5:7], db[:, :, 5:7], T, mode, nm.n_transition)
    for got in (native.count_dbn_host(gpu_ctx, nm, two_ib, two_db, T, mode, raw=True)["raw"], _device(gpu_ctx, nm, two_ib, two_db, K, T, mode)[:2]):
        assert np.array_equal(got[0], a_i * np.uint64(K // 2)) and np.array_equal(got[1], a_t * np.uint64(K // 2))


# ---- 5. run-length edges: hand-built dyn_bin for a small synthetic model (a lane's pending run is flushed when the cell changes and at its end)
@pytest.mark.parametrize("mode", [AUTO, PER_STEP])
@pytest.mark.parametrize("T", [6, 9])
def test_run_length_edges(gpu_ctx, model_dir, mode, T):
    nm, parms, g = _model("synthetic_terminal", model_dir)
    assert not g["depend"] and nm.n_dyn == 3
    r_i, r_d = g["r_i"], g["r_t"][g["tm"][:, 1]]
    rs = np.random.RandomState(T)
    n = 300
    ib = np.stack([rs.randint(1, int(r) + 1, size=n) for r in r_i], axis=1).astype(np.uint8)
    db = np.zeros((n, T, 3), dtype=np.uint8)
    t = np.arange(T)
    for i in range(n):
        kind = i % 5
        for k in range(3):
            r, b0 = int(r_d[k]), 1 + (i + k) % int(r_d[k])
            other = 1 + (b0 % r)
            if kind == 0:
                col = np.full(T, b0)                                      # never changes: one run of T-1
            elif kind == 1:
                col = np.where(t % 2 == 0, b0, other)                     # changes every second: runs of 1
            elif kind == 2:
                col = np.where(t == T - 1, other, b0)                     # changes only at t = T-1: the last run has one observation
            elif kind == 3:
                col = np.where(t >= 4, other, b0)                         # changes exactly at the word boundary 3 -> 4
            else:
                col = np.where(t == 4, other, b0)                         # ... and at 3 -> 4 and 4 -> 5
            db[i, :, k] = col
    raw_ib, raw_db = np.ascontiguousarray(ib.T), native.pack_dyn_bin(db)
    want_i, want_t = _check(gpu_ctx, nm, g, raw_ib, raw_db, T, mode)
    assert int(want_t.sum()) == n * (T - 1) * 3 and int(want_t.max()) >= T - 1


# ---- 6. accumulation
def test_calls_accumulate(gpu_ctx, model_dir):
    T, mode = 61, AUTO
    nm, parms, g, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T, mode)
    want_i, want_t, _ = _ref(("uncor_1200code_v2p1", N, T, mode), g, ib, db, T, mode, nm.n_transition)
    h = 400
    first = native.count_dbn_host(gpu_ctx, nm, ib, db, T, mode, raw=True, n=h, col_offset=0)
    assert not np.array_equal(first["raw"][1], want_t)
    both = native.count_dbn_host(gpu_ctx, nm, ib, db, T, mode, raw=True, n=N - h, col_offset=h, counts=first["raw"])
    assert both["raw"][0] is first["raw"][0]                              # accumulated in place
    assert np.array_equal(both["raw"][0], want_i) and np.array_equal(both["raw"][1], want_t)
    assert np.array_equal(R.flat(both["N_transition"]), want_t)
    # the same on the device: two calls into one buffer, which starts with one hot cell at 2^32 - 3
    hot_i, hot_t = int(np.argmax(want_i)), int(np.argmax(want_t))
    start = (np.zeros_like(want_i), np.zeros_like(want_t))
    start[0][hot_i] = start[1][hot_t] = 2 ** 32 - 3
    ci, ct, _, err = _device(gpu_ctx, nm, ib, db, N, T, mode, start=start)
    assert err is None and np.array_equal(ci, want_i + start[0]) and np.array_equal(ct, want_t + start[1])
    assert int(ci[hot_i]) == 2 ** 32 - 3 + int(want_i[hot_i]) > 2 ** 32 and int(ct[hot_t]) > 2 ** 32
    ci2, ct2, _, _ = _device(gpu_ctx, nm, ib, db, N, T, mode, start=(ci, ct))
    assert np.array_equal(ci2, 2 * want_i + start[0]) and np.array_equal(ct2, 2 * want_t + start[1])
    # counts_transition = NULL: nothing is written for that network
    ci, ct, kernel, err = _device(gpu_ctx, nm, ib, db, N, T, mode, start=(np.zeros_like(want_i), np.full_like(want_t, 9)), want_t=False)
    assert err is None and np.array_equal(ci, want_i) and np.all(ct == 9) and kernel == "k_count_dbn[frozen]"


# ---- 7. ld and col_offset
@pytest.mark.parametrize("name,mode", [("uncor_1200code_v2p1", AUTO), ("uncor_1200code_v1", AUTO)])
def test_ld_and_col_offset_with_poisoned_neighbours(gpu_ctx, model_dir, name, mode):
    T, LD, COL = 61, 1024, 100
    nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, N, T, mode)
    want_i, want_t, _ = _ref((name, N, T, mode), g, ib, db, T, mode, nm.n_transition)
    big_ib = np.zeros((ib.shape[0], LD), dtype=np.uint8)                          # bins no variable has: 0 on one side, 255 on the other
    big_db = np.zeros((db.shape[0], db.shape[1], LD), dtype=np.uint32)
    big_ib[:, COL + N:], big_db[:, :, COL + N:] = 255, 0xFFFFFFFF
    big_ib[:, COL: COL + N] = ib
    big_db[:, :, COL: COL + N] = db
    ci, ct, _, err = _device(gpu_ctx, nm, big_ib, big_db, N, T, mode, ld=LD, col=COL)
    assert err is None and np.array_equal(ci, want_i) and np.array_equal(ct, want_t)
    host = native.count_dbn_host(gpu_ctx, nm, big_ib, big_db, T, mode, raw=True, n=N, col_offset=COL)
    assert np.array_equal(host["raw"][0], want_i) and np.array_equal(host["raw"][1], want_t)
    with pytest.raises(L.EmgpuError) as ei:                                        # one column further reads a poisoned neighbour
        native.count_dbn_host(gpu_ctx, nm, big_ib, big_db, T, mode, raw=True, n=N, col_offset=COL + 1)
    assert ei.value.code == L.ERR_ARG
    assert int(ei.value.counts["raw"][0].sum()) == (N - 1) * nm.n_initial          # the poisoned trajectory's observations are skipped


# ---- 8. corrupt bins
@pytest.mark.parametrize("mode", [AUTO, PER_STEP])
def test_corrupt_bins_skip_their_observations_only(gpu_ctx, model_dir, mode):
    T = 61
    nm, parms, g, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T, mode)
    clean_i, clean_t, _ = _ref(("uncor_1200code_v2p1", N, T, mode), g, ib, db, T, mode, nm.n_transition)
    r_i, r_d = g["r_i"], g["r_t"][g["tm"][:, 1]]
    # plants that nothing reads: the padding bytes of the last word (columns 61 .. 63) -- neither a skip nor a report
    pad = native.unpack_dyn_bin(db, 64)
    assert pad.shape[1] == 64
    pad[:, T:, :] = 255
    pad[::2, T:, :] = 0
    _check(gpu_ctx, nm, g, ib, native.pack_dyn_bin(pad), T, mode, key=("uncor_1200code_v2p1", N, T, mode))
    # ... and the columns >= T of a larger trace: its first 30 columns count as the clean trace's do
    late = native.unpack_dyn_bin(db, T)
    late[:, 30:, :] = 255
    late[::2, 30:, :] = 0
    ref_i, ref_t, _ = _ref(None, g, ib, native.pack_dyn_bin(native.unpack_dyn_bin(db, T)[:, :30]), 30, mode, nm.n_transition)
    late = native.pack_dyn_bin(late)
    got = native.count_dbn_host(gpu_ctx, nm, ib, np.ascontiguousarray(late[:8]), 30, mode, raw=True)  # (no error; word 7 ends in two plants)
    assert np.array_equal(got["raw"][0], ref_i) and np.array_equal(got["raw"][1], ref_t)
    ci, ct, _, err = _device(gpu_ctx, nm, ib, late, N, 30, mode)                                       # the whole larger trace behind it
    assert err is None and np.array_equal(ci, ref_i) and np.array_equal(ct, ref_t)
    # plants that are read
    ib2, db2 = ib.copy(), native.unpack_dyn_bin(db, T)
    ib2[0, 5] = 0                       # a root of the initial network: bin 0 ...
    ib2[6, 70] = r_i[6] + 1             # ... and bin r + 1
    db2[200, 0, 0] = 0                  # column 0: a parent only
    db2[300, 0, 1] = r_d[1] + 1
    db2[400, 31, 1] = 0                 # a middle second
    db2[450, 32, 2] = r_d[2] + 1
    db2[500, T - 1, 2] = 0              # the last second, in the partly filled last word
    db2[640, T - 1, 0] = 255
    db2 = native.pack_dyn_bin(db2)
    want_i, want_t, skipped = _ref(None, g, ib2, db2, T, mode, nm.n_transition)
    assert skipped >= 8 and int(want_i.sum()) + int(want_t.sum()) + skipped == N * (nm.n_initial + (T - 1) * nm.n_dyn)
    assert int(want_i.sum()) < int(clean_i.sum()) and int(want_t.sum()) < int(clean_t.sum())
    with pytest.raises(L.EmgpuError) as ei:
        native.count_dbn_host(gpu_ctx, nm, ib2, db2, T, mode, raw=True)
    assert ei.value.code == L.ERR_ARG and "outside 1..r" in str(ei.value)
    assert np.array_equal(ei.value.counts["raw"][0], want_i) and np.array_equal(ei.value.counts["raw"][1], want_t)
    gpu_ctx.sync()                                   # the host call's report went with its return value
    ci, ct, _, _ = _device(gpu_ctx, nm, ib2, db2, N, T, mode, sync=False)
    assert np.array_equal(ci, want_i) and np.array_equal(ct, want_t)
    # the device call's report is pending: a host call on a valid trace is served without an error of its own and leaves it in place
    host = native.count_dbn_host(gpu_ctx, nm, ib, db, T, mode, raw=True)
    assert np.array_equal(host["raw"][0], clean_i) and np.array_equal(host["raw"][1], clean_t)
    with pytest.raises(L.EmgpuError) as ei:
        gpu_ctx.sync()
    assert ei.value.code == L.ERR_ARG and "outside 1..r" in str(ei.value)
    gpu_ctx.sync()                                   # reported once
    _check(gpu_ctx, nm, g, ib, db, T, mode, key=("uncor_1200code_v2p1", N, T, mode))   # and a valid call is served


# ---- 9. many host chunks equal one
def test_many_host_chunks_equal_one(gpu_ctx, model_dir, monkeypatch):
    n, T = 20011, 160
    nm, parms, g, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, n, T, AUTO)
    one = native.count_dbn_host(gpu_ctx, nm, ib, db, T, AUTO, raw=True)
    assert gpu_ctx.last_launches() == 1
    monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", "1")
    many = native.count_dbn_host(gpu_ctx, nm, ib, db, T, AUTO, raw=True)
    assert gpu_ctx.last_launches() >= 8
    assert np.array_equal(many["raw"][0], one["raw"][0]) and np.array_equal(many["raw"][1], one["raw"][1])
    want_i, want_t, _ = _ref(None, g, ib, db, T, AUTO, nm.n_transition)
    assert np.array_equal(one["raw"][0], want_i) and np.array_equal(one["raw"][1], want_t)


# ---- 10. the model follows
def test_counting_follows_the_model_on_the_same_context(gpu_ctx, model_dir):
    T = 61
    _, _, _, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T, AUTO)
    nm, parms, g = _model("uncor_1200code_v2p1", model_dir)     # a copy of its own: this test changes it
    want_i, want_t, _ = _ref(("uncor_1200code_v2p1", N, T, AUTO), g, ib, db, T, AUTO, nm.n_transition)

    def same():
        got = native.count_dbn_host(gpu_ctx, nm, ib, db, T, AUTO, raw=True)["raw"]
        return np.array_equal(got[0], want_i) and np.array_equal(got[1], want_t)
    assert same()
    nm.set_prior(1.0)                                           # counts depend on the graph only
    assert same()
    tv = int(g["tm"][1, 1])
    nm.set_f64(L.F_N_TRANSITION, tv + 1, nm.get_f64(L.F_N_TRANSITION, tv + 1)[::-1].copy())
    assert same()
    # another model, other r: the layout follows
    other, _, g2, ib2, db2 = _trace(gpu_ctx, "glider_v1", model_dir, N, T, AUTO)
    assert not np.array_equal(other.count_layout(1), nm.count_layout(1))
    _check(gpu_ctx, other, g2, ib2, db2, T, AUTO, key=("glider_v1", N, T, AUTO))
    assert same()


# ---- 11. ties to scoring
@pytest.mark.parametrize("mode", [AUTO, PER_STEP])
def test_counts_times_log_tables_is_the_traces_log_likelihood(gpu_ctx, model_dir, mode):
    """sum_i log_lik[i] = sum over cells of N[c] * logp[c].  Each log_lik carries at most ni + nd (T-1) = 187 roundings of about 1.1e-16
    relative to its partial sums (<= 2e-14 at T = 61); fsum adds none; 1e-9 is five orders of slack and still catches one miscounted cell
    at n = 777 (a single entry is >= 1e-6 of the total)."""
    T = 61
    _, _, _, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T, mode)
    nm, parms, g = _model("uncor_1200code_v2p1", model_dir)
    ll = native.score_dbn_host(gpu_ctx, nm, ib, db, T, mode, raw=True)["log_lik"]
    assert np.isfinite(ll).all()
    got = native.count_dbn_host(gpu_ctx, nm, ib, db, T, mode, raw=True)
    tabs = S.lib_tables(nm)
    terms = []
    for v, Nv in enumerate(got["N_initial"]):
        hit = Nv > 0
        terms += (Nv[hit] * tabs["initial"][v][hit]).tolist()
    for v, Nv in enumerate(got["N_transition"]):
        if Nv.size:
            hit = Nv > 0
            terms += (Nv[hit] * tabs["transition"][v][hit]).tolist()
    total, want = math.fsum(terms), math.fsum(ll.tolist())
    print("fsum(N * logp) = %.17g, fsum(log_lik) = %.17g, relative difference %.3g" % (total, want, abs(total - want) / abs(want)))
    assert abs(total - want) <= 1e-9 * abs(want)


def test_sample_count_host_equals_sample_then_count(gpu_ctx, model_dir):
    T = 61
    for name, mode in (("uncor_1200code_v2p1", AUTO), ("uncor_1200code_v2p1", PER_STEP), ("glider_v1", AUTO)):
        nm, parms, g = _model(name, model_dir)
        got = native.sample_count_host(gpu_ctx, nm, N, T, SEED + 1, transition_mode=mode)
        plain = native.sample_dbn_host(gpu_ctx, nm, N, T, SEED + 1, raw=True, pinned=False, transition_mode=mode)
        want = native.count_dbn_host(gpu_ctx, nm, plain["init_bin"], plain["dyn_bin"], T, mode, raw=True)
        assert got["kernel"].startswith("k_") and got["count_kernel"] == want["kernel"] == _name(g, mode)
        assert np.array_equal(got["raw"][0], want["raw"][0]) and np.array_equal(got["raw"][1], want["raw"][1])
        assert int(got["raw"][1].sum()) == N * (T - 1) * nm.n_dyn
        again = native.sample_count_host(gpu_ctx, nm, N, T, SEED + 1, transition_mode=mode, counts=got["raw"])      # accumulates
        assert np.array_equal(again["raw"][0], 2 * want["raw"][0]) and np.array_equal(again["raw"][1], 2 * want["raw"][1])


# ---- 12. round trip
def test_round_trip_of_the_root_nodes(gpu_ctx, model_dir):
    """sample -> count -> normalise gives back the model, for the initial network's root nodes (uncor_1200code_v2p1 has one, G: 4 cells): each
    normalised count lies within 5 standard errors, 5 sqrt(p (1 - p) / n), of the model's own probability.  The bound is derived, not
    measured: a cell misses it by chance about once in 1e6, and the CPU oracle's sample for this seed stays inside it (largest deviation:
    2.26 standard errors, checked on the oracle before the seed was committed)."""
    n, T, seed = 200000, 61, 0x2071D
    nm, parms, g = _model("uncor_1200code_v2p1", model_dir)
    got = native.sample_count_host(gpu_ctx, nm, n, T, seed)
    assert int(got["raw"][0].sum()) == n * nm.n_initial and int(got["raw"][1].sum()) == n * (T - 1) * nm.n_dyn
    plain = native.sample_dbn_host(gpu_ctx, nm, n, T, seed, raw=True, pinned=False)
    roots = [v for v in range(nm.n_initial) if not g["G_i"][:, v].any()]
    assert roots
    cells = 0
    for v in roots:
        r = int(g["r_i"][v])
        Nv = got["N_initial"][v]
        assert Nv.shape == (r, 1)
        assert np.array_equal(Nv[:, 0], np.bincount(plain["init_bin"][v], minlength=r + 1)[1:])       # exact
        model_N = nm.get_f64(L.F_N_INITIAL, v + 1).reshape(-1)
        p = model_N / model_N.sum()
        dev = np.abs(Nv[:, 0] / n - p)
        se = np.sqrt(p * (1 - p) / n)
        print("root %d: largest deviation %.3f standard errors" % (v, float(np.max(dev[se > 0] / se[se > 0]))))
        assert np.all(dev <= 5 * se)
        cells += r
    assert 2 <= cells <= 64
