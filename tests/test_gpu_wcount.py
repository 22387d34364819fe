"""-m gpu: the weighted k_count_dbn against the numpy restatement of its definition (count_ref.count(..., weights=w)).  Counts are integers,
so every comparison is exact equality whatever the kernel's accumulation scheme does (run lengths per lane, u64 LDS partials per workgroup,
64-bit global adds).  Traces come from native.sample_dbn_host or are built by hand; each is counted by emgpu_count_dbn_weighted_host and by
emgpu_count_dbn_weighted_device, the latter into buffers with guard words behind both tables."""
import numpy as np
import pytest

import count_ref as W
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native, synthetic
from em_model_manned_bayes_amd import encounter_model as E

pytestmark = pytest.mark.gpu

N, SEED = 777, 0xC0125
AUTO, PER_STEP = L.TRANSITION_REFERENCE_AUTO, L.TRANSITION_PER_STEP
GUARD = 0x5A5A5A5A5A5A5A5A
SPECIAL = np.array([0, 1, 2, 3, 2 ** 16, 2 ** 24 - 1, 2 ** 32 - 1], dtype=np.uint32)
_paths, _traces = {}, {}


def _model(name, model_dir):
    """(a fresh NativeModel, parms, graph) of the model's .txt: tests that change the model change their own copy"""
    if name not in _paths:
        if name == "synthetic_terminal":
            _paths[name] = model_dir + "/synthetic_terminal_w.txt"
            em_io.em_write(synthetic.terminal_trajectory_model(0x5EED), _paths[name])
        else:
            _paths[name] = em_io.materialize_model(name, model_dir)
    parms = em_io.em_read(_paths[name])
    return parms["native"], parms, W.graph(parms)


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


def _weights(kind, n, seed=1):
    rs = np.random.RandomState(seed)
    if kind == "special":
        return SPECIAL[rs.randint(0, len(SPECIAL), size=n)]
    if kind == "random24":
        return rs.randint(0, 2 ** 24, size=n).astype(np.uint32)
    return np.full(n, int(kind), dtype=np.uint32)


def _ref(g, ib, db, T, w, mode, nt):
    """count_ref with weights of a raw trace as the library's two flat arrays and the skipped observations"""
    Ni, Nt, skipped = W.count(g, ib.T, None if db is None else native.unpack_dyn_bin(db, T), mode, n_transition=nt, weights=w)
    return W.flat(Ni), W.flat(Nt), skipped


def _name(g, mode):
    return "k_count_dbn[per-step,weighted]" if (mode == PER_STEP or g["depend"]) else "k_count_dbn[frozen,weighted]"


def _device(ctx, nm, ib, db, w, n, T, mode, ld=0, col=0, sync=True, start=None, want_t=True):
    """emgpu_count_dbn_weighted_device over device copies of the raw arrays, into buffers holding `start` (default zeros) with 4 guard words
    behind each, which must stay.  Returns (initial array, transition array, kernel, the error of ctx.sync() or None)."""
    import torch
    dev = torch.device("cuda", 0)
    d_ib = torch.from_numpy(np.array(ib, order="C")).to(dev)
    d_db = None if db is None else torch.from_numpy(np.array(db, order="C").view(np.int32)).to(dev)
    d_w = torch.from_numpy(np.array(w, dtype=np.uint32, order="C").view(np.int32)).to(dev)
    bufs = []
    for network in (0, 1):
        size = int(nm.count_layout(network)[-1])
        h = np.full(size + 4, GUARD, dtype=np.uint64)
        h[:size] = 0 if start is None else start[network]
        bufs.append((size, torch.from_numpy(h.view(np.int64)).to(dev)))
    torch.cuda.synchronize()
    native.count_dbn_weighted_device(ctx, nm, native.score_params(n, T, mode, ld, col), d_ib.data_ptr(), 0 if d_db is None else d_db.data_ptr(),
                                     d_w.data_ptr(), bufs[0][1].data_ptr(), bufs[1][1].data_ptr() if want_t else 0)
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


def _check(ctx, nm, g, ib, db, T, mode, w, expect_skips=False):
    """host and device weighted counts of the raw trace (ib [ni, n], db [G4, nd, n] or None) equal the reference's"""
    n = ib.shape[1]
    want_i, want_t, skipped = _ref(g, ib, db, T, w, mode, nm.n_transition)
    assert (skipped > 0) == expect_skips
    try:
        host = native.count_dbn_weighted_host(ctx, nm, ib, db, T, w, mode, raw=True)
        assert not expect_skips
    except L.EmgpuError as e:
        assert expect_skips and e.code == L.ERR_ARG and "outside 1..r" in str(e)
        host = e.counts
    assert host["kernel"] == _name(g, mode), host["kernel"]
    assert np.array_equal(host["raw"][0], want_i) and np.array_equal(host["raw"][1], want_t)
    ci, ct, kernel, err = _device(ctx, nm, ib, db, w, n, T, mode)
    assert (err is not None) == expect_skips and kernel == _name(g, mode)
    assert np.array_equal(ci, want_i) and np.array_equal(ct, want_t)
    return want_i, want_t


# ---- 1. sampled traces: large tables (the global path), small tables (run-length flushes into the u64 partials), no transition network
@pytest.mark.parametrize("name,mode", [("uncor_1200code_v2p1", AUTO), ("uncor_1200code_v2p1", PER_STEP), ("glider_v1", AUTO), ("cor_v1", AUTO)])
def test_weighted_counts_of_sampled_traces(gpu_ctx, model_dir, name, mode):
    T = 61
    nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, N, T, mode)
    for kind in ("special", "random24"):
        w = _weights(kind, N)
        want_i, want_t = _check(gpu_ctx, nm, g, ib, db, T, mode, w)
        total = int(w.astype(np.uint64).sum())
        assert sum(int(x) for x in want_i) == total * nm.n_initial and sum(int(x) for x in want_t) == total * (T - 1) * nm.n_dyn
    # the user-facing shapes and the class layer give the same tables
    user = native.count_dbn_weighted_host(gpu_ctx, nm, ib.T, native.unpack_dyn_bin(db, T), T, w, mode)
    assert np.array_equal(W.flat(user["N_initial"]), want_i) and np.array_equal(W.flat(user["N_transition"]), want_t)
    if name == "glider_v1":
        m = E.EncounterModel(_paths[name], idxZeroBoundaries=(1, 2, 3))
        Ni, Nt, rep, chg = m.count(ib.T, native.unpack_dyn_bin(db, T), ctx=gpu_ctx, weights=w)
        assert rep is None and chg is None and np.array_equal(W.flat(Ni), want_i) and np.array_equal(W.flat(Nt), want_t)


def test_weighted_counts_of_the_terminal_geometry_model(gpu_ctx, model_dir):
    nm, parms, g = _model("terminal_v3_radar_encounter_model", model_dir)
    assert nm.n_transition == 0 and nm.n_dyn == 0
    bins, _, _ = native.sample_bn_host(gpu_ctx, nm, N, SEED)
    ib = np.ascontiguousarray(bins.T)
    want_i, want_t = _check(gpu_ctx, nm, g, ib, None, 1, AUTO, _weights("special", N))
    assert want_t.size == 0 and int(want_i.sum()) > 0
    _check(gpu_ctx, nm, g, ib, None, 7, AUTO, _weights("random24", N))      # no transition network: sample_time is of no consequence


# ---- 2. the packed-word edges and the wave and workgroup edges
@pytest.mark.parametrize("T", [1, 2, 4, 5, 61])
@pytest.mark.parametrize("name", ["uncor_1200code_v2p1", "glider_v1"])
def test_sample_times_around_the_packed_word(gpu_ctx, model_dir, name, T):
    nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, N, T, AUTO)
    w = _weights("special", N, seed=T)
    want_i, want_t = _check(gpu_ctx, nm, g, ib, db, T, AUTO, w)
    if T == 1:                                          # the transition array is left untouched, whatever it holds
        start = (np.zeros_like(want_i), np.full_like(want_t, 7))
        ci, ct, _, err = _device(gpu_ctx, nm, ib, db, w, N, 1, AUTO, start=start)
        assert err is None and np.array_equal(ci, want_i) and np.all(ct == 7)
        _check(gpu_ctx, nm, g, ib, None, 1, AUTO, w)   # dyn_bin may be absent


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 777])
def test_batch_sizes(gpu_ctx, model_dir, n):
    for name, mode in (("uncor_1200code_v2p1", PER_STEP), ("cor_v1", AUTO)):
        nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, n, 5, mode)
        w = _weights("special", n, seed=n)
        w[-1] = 2 ** 32 - 1                             # the last lane of the batch counts
        _check(gpu_ctx, nm, g, ib, db, 5, mode, w)


# ---- 3. all 1 and all 0
@pytest.mark.parametrize("name,mode", [("uncor_1200code_v2p1", AUTO), ("glider_v1", AUTO), ("uncor_1200code_v2p1", PER_STEP)])
def test_all_ones_is_the_unweighted_count_and_all_zeros_is_nothing(gpu_ctx, model_dir, name, mode):
    T = 61
    nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, N, T, mode)
    plain = native.count_dbn_host(gpu_ctx, nm, ib, db, T, mode, raw=True)
    ones = native.count_dbn_weighted_host(gpu_ctx, nm, ib, db, T, _weights(1, N), mode, raw=True)
    assert np.array_equal(ones["raw"][0], plain["raw"][0]) and np.array_equal(ones["raw"][1], plain["raw"][1])
    ci, ct, _, err = _device(gpu_ctx, nm, ib, db, _weights(1, N), N, T, mode)
    assert err is None and np.array_equal(ci, plain["raw"][0]) and np.array_equal(ct, plain["raw"][1])
    # all 0, over a trace full of bad bins: the tables keep what they held and nothing is reported, now or at the next sync
    ib2, db2 = ib.copy(), db.copy()
    ib2[:, ::3], db2[:, :, ::5] = 0, 0xFFFFFFFF
    ib2[0, 1], db2[0, 1, 2] = 255, 0
    start = (np.arange(plain["raw"][0].size, dtype=np.uint64) + 11, np.arange(plain["raw"][1].size, dtype=np.uint64) * 3 + 1)
    zeros = _weights(0, N)
    ci, ct, kernel, err = _device(gpu_ctx, nm, ib2, db2, zeros, N, T, mode, start=start)
    assert err is None and kernel == _name(g, mode) and np.array_equal(ci, start[0]) and np.array_equal(ct, start[1])
    host = native.count_dbn_weighted_host(gpu_ctx, nm, ib2, db2, T, zeros, mode, raw=True, counts=(start[0].copy(), start[1].copy()))
    assert np.array_equal(host["raw"][0], start[0]) and np.array_equal(host["raw"][1], start[1])
    gpu_ctx.sync()


# ---- 4. 64-bit carries: one trajectory 4096 times at weight 2^32 - 1.  A hot cell receives 4096 * 60 * (2^32 - 1), which carries past bit 32
# inside a partial (glider_v1: its tables are in LDS) and in the global add (uncor_1200code_v2p1: its transition tables are not)
@pytest.mark.parametrize("name,mode", [("uncor_1200code_v2p1", AUTO), ("uncor_1200code_v2p1", PER_STEP), ("glider_v1", AUTO)])
def test_sums_carry_past_32_bits(gpu_ctx, model_dir, name, mode):
    T, K, top = 61, 4096, 2 ** 32 - 1
    nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, N, T, mode)
    col = 5
    still = np.ascontiguousarray(np.broadcast_to((db[:1, :, col:col + 1] & 0xFF) * np.uint32(0x01010101), db[:, :, col:col + 1].shape))
    one_ib = ib[:, col:col + 1]                            # trajectory 5, holding its bins of second 0 for all T: one cell per table
    one_i, one_t, _ = _ref(g, one_ib, still, T, np.ones(1, np.uint32), mode, nm.n_transition)
    rep_ib, rep_db = np.ascontiguousarray(np.repeat(one_ib, K, axis=1)), np.ascontiguousarray(np.repeat(still, K, axis=2))
    w = _weights(top, K)
    want_i, want_t = one_i * np.uint64(K * top), one_t * np.uint64(K * top)
    assert int(one_t.max()) == T - 1 and int(want_t.max()) == 60 * K * top > 2 ** 49
    host = native.count_dbn_weighted_host(gpu_ctx, nm, rep_ib, rep_db, T, w, mode, raw=True)["raw"]
    assert np.array_equal(host[0], want_i) and np.array_equal(host[1], want_t)
    ci, ct, _, err = _device(gpu_ctx, nm, rep_ib, rep_db, w, K, T, mode)
    assert err is None and np.array_equal(ci, want_i) and np.array_equal(ct, want_t)
    # the hot cells preset to 2^63 - 5: the sum passes bit 63 and stays below 2^64
    hot_i, hot_t = int(np.argmax(want_i)), int(np.argmax(want_t))
    start = (np.zeros_like(want_i), np.zeros_like(want_t))
    start[0][hot_i] = start[1][hot_t] = 2 ** 63 - 5
    ci, ct, _, err = _device(gpu_ctx, nm, rep_ib, rep_db, w, K, T, mode, start=start)
    assert err is None and np.array_equal(ci, want_i + start[0]) and np.array_equal(ct, want_t + start[1])
    assert int(ct[hot_t]) == 2 ** 63 - 5 + int(want_t[hot_t]) > 2 ** 63
    # two halves added into one buffer
    h = K // 2
    first = native.count_dbn_weighted_host(gpu_ctx, nm, rep_ib, rep_db, T, w[:h], mode, raw=True, n=h, col_offset=0)
    both = native.count_dbn_weighted_host(gpu_ctx, nm, rep_ib, rep_db, T, w[h:], mode, raw=True, n=K - h, col_offset=h, counts=first["raw"])
    assert both["raw"][0] is first["raw"][0] and np.array_equal(both["raw"][0], want_i) and np.array_equal(both["raw"][1], want_t)
    ci1, ct1, _, _ = _device(gpu_ctx, nm, rep_ib[:, :h], rep_db[:, :, :h], w[:h], h, T, mode)
    ci2, ct2, _, _ = _device(gpu_ctx, nm, rep_ib[:, h:], rep_db[:, :, h:], w[h:], K - h, T, mode, start=(ci1, ct1))
    assert np.array_equal(ci2, want_i) and np.array_equal(ct2, want_t)


# ---- 5. run-length edges: §21's hand-built dyn_bin for a small synthetic model, under weights 1, 5 and 0
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
    for wt in (1, 5, 0):
        want_i, want_t = _check(gpu_ctx, nm, g, raw_ib, raw_db, T, mode, _weights(wt, n))
        assert int(want_t.sum()) == wt * n * (T - 1) * 3
    # the three weights side by side: every kind of run under every weight (15 = lcm(5 kinds, 3 weights))
    mixed = np.array([1, 5, 0], dtype=np.uint32)[np.arange(n) % 3]
    _check(gpu_ctx, nm, g, raw_ib, raw_db, T, mode, mixed)


# ---- 6. corrupt bins: reported for a weighted trajectory, of no consequence in one of weight 0
@pytest.mark.parametrize("mode", [AUTO, PER_STEP])
def test_corrupt_bins_count_only_where_the_weight_is_positive(gpu_ctx, model_dir, mode):
    T = 61
    nm, parms, g, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T, mode)
    r_i, r_d = g["r_i"], g["r_t"][g["tm"][:, 1]]
    planted = [5, 70, 200, 300, 400, 450, 500, 640]
    ib2, db2 = ib.copy(), native.unpack_dyn_bin(db, T)
    ib2[0, 5] = 0                       # a root of the initial network: bin 0 ...
    ib2[6, 70] = r_i[6] + 1             # ... and bin r + 1
    db2[200, 0, 0] = 0                  # column 0: a parent only
    db2[300, 0, 1] = r_d[1] + 1
    db2[400, 31, 1] = 0                 # a middle second, the last byte of a word
    db2[450, 32, 2] = r_d[2] + 1        # the first byte of the next
    db2[500, T - 1, 2] = 0              # the last second, in the partly filled last word
    db2[640, T - 1, 0] = 255
    db2 = native.pack_dyn_bin(db2)
    w = _weights("special", N, seed=6)
    w[w == 0] = 1
    # every planted trajectory has weight 0: the counts are those of the clean trace under the same weights, and nothing is reported
    w0 = w.copy()
    w0[planted] = 0
    clean_i, clean_t, skipped = _ref(g, ib, db, T, w0, mode, nm.n_transition)
    assert skipped == 0
    got_i, got_t = _check(gpu_ctx, nm, g, ib2, db2, T, mode, w0)
    assert np.array_equal(got_i, clean_i) and np.array_equal(got_t, clean_t)
    gpu_ctx.sync()
    # the planted trajectories weighted: _host reports now, with the reference's counts
    want_i, want_t, skipped = _ref(g, ib2, db2, T, w, mode, nm.n_transition)
    assert skipped >= 8
    with pytest.raises(L.EmgpuError) as ei:
        native.count_dbn_weighted_host(gpu_ctx, nm, ib2, db2, T, w, mode, raw=True)
    assert ei.value.code == L.ERR_ARG and "outside 1..r" in str(ei.value)
    assert np.array_equal(ei.value.counts["raw"][0], want_i) and np.array_equal(ei.value.counts["raw"][1], want_t)
    gpu_ctx.sync()                                   # the host call's report went with its return value
    # one weighted plant alone is enough
    w1 = w0.copy()
    w1[450] = 3
    _check(gpu_ctx, nm, g, ib2, db2, T, mode, w1, expect_skips=True)
    # _device reports at emgpu_ctx_sync, once; until then the report is pending, and a clean weighted _host call neither raises nor loses it
    ci, ct, _, _ = _device(gpu_ctx, nm, ib2, db2, w, N, T, mode, sync=False)
    assert np.array_equal(ci, want_i) and np.array_equal(ct, want_t)
    host = native.count_dbn_weighted_host(gpu_ctx, nm, ib2, db2, T, w0, mode, raw=True)
    assert np.array_equal(host["raw"][0], clean_i) and np.array_equal(host["raw"][1], clean_t)
    with pytest.raises(L.EmgpuError) as ei:
        gpu_ctx.sync()
    assert ei.value.code == L.ERR_ARG and "outside 1..r" in str(ei.value)
    gpu_ctx.sync()                                   # reported once


# ---- 7. ld and col_offset: the trace is a window between poisoned neighbours, the weights are read from index 0 of their own array
@pytest.mark.parametrize("name,mode", [("uncor_1200code_v2p1", AUTO), ("glider_v1", AUTO)])
def test_ld_and_col_offset_with_poisoned_neighbours(gpu_ctx, model_dir, name, mode):
    T, LD, COL = 61, 1024, 100
    nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, N, T, mode)
    w = _weights("special", N, seed=7)
    w[:3] = (2, 2 ** 32 - 1, 1)
    want_i, want_t, _ = _ref(g, ib, db, T, w, mode, nm.n_transition)
    big_ib = np.zeros((ib.shape[0], LD), dtype=np.uint8)                          # bins no variable has: 0 on one side, 255 on the other
    big_db = np.zeros((db.shape[0], db.shape[1], LD), dtype=np.uint32)
    big_ib[:, COL + N:], big_db[:, :, COL + N:] = 255, 0xFFFFFFFF
    big_ib[:, COL: COL + N] = ib
    big_db[:, :, COL: COL + N] = db
    big_w = np.concatenate([w, np.full(LD - N, 2 ** 32 - 1, np.uint32)])         # what a call that offset its weights would read
    ci, ct, _, err = _device(gpu_ctx, nm, big_ib, big_db, big_w, N, T, mode, ld=LD, col=COL)
    assert err is None and np.array_equal(ci, want_i) and np.array_equal(ct, want_t)
    host = native.count_dbn_weighted_host(gpu_ctx, nm, big_ib, big_db, T, w, mode, raw=True, n=N, col_offset=COL)
    assert np.array_equal(host["raw"][0], want_i) and np.array_equal(host["raw"][1], want_t)
    with pytest.raises(L.EmgpuError) as ei:                                        # one column further reads a poisoned neighbour ...
        native.count_dbn_weighted_host(gpu_ctx, nm, big_ib, big_db, T, w, mode, raw=True, n=N, col_offset=COL + 1)
    assert ei.value.code == L.ERR_ARG
    w[-1] = 0                                                                      # ... unless its weight is 0
    native.count_dbn_weighted_host(gpu_ctx, nm, big_ib, big_db, T, w, mode, raw=True, n=N, col_offset=COL + 1)


# ---- 8. the smallest n at which a workgroup walks a second tile (the grid is capped at 2048 workgroups of 256)
def test_a_second_tile(gpu_ctx, model_dir):
    n, T = 2048 * 256 + 257, 2
    for name in ("uncor_1200code_v2p1", "glider_v1"):
        nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, n, T, AUTO)
        w = _weights("special", n, seed=8)
        w[2048 * 256:] = np.arange(1, 258, dtype=np.uint32) * 65537               # the second tile's lanes, each with a weight of its own
        _check(gpu_ctx, nm, g, ib, db, T, AUTO, w)


# ---- 9. many host chunks equal one: the weights are one more array of 4 bytes per lane, chunk k uploads weights + c0
def test_many_host_chunks_equal_one(gpu_ctx, model_dir, monkeypatch):
    T = 61
    nm, parms, g = _model("uncor_1200code_v2p1", model_dir)
    per_lane = nm.n_initial + 4 * ((T + 3) // 4) * nm.n_dyn + 4
    c = (1 << 20) // per_lane // 256 * 256
    n = 2 * c + 89
    nm, parms, g, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, n, T, AUTO)
    w = _weights("random24", n, seed=9)
    w[[0, c - 1, c, 2 * c - 1, 2 * c, n - 1]] = (2 ** 32 - 1, 2 ** 32 - 2, 2 ** 32 - 3, 2 ** 32 - 4, 2 ** 32 - 5, 2 ** 32 - 6)   # the chunks' edges
    one = native.count_dbn_weighted_host(gpu_ctx, nm, ib, db, T, w, AUTO, raw=True)
    assert gpu_ctx.last_launches() == 1
    monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", "1")
    many = native.count_dbn_weighted_host(gpu_ctx, nm, ib, db, T, w, AUTO, raw=True)
    assert gpu_ctx.last_launches() == 3
    assert np.array_equal(many["raw"][0], one["raw"][0]) and np.array_equal(many["raw"][1], one["raw"][1])
    want_i, want_t, _ = _ref(g, ib, db, T, w, AUTO, nm.n_transition)
    assert np.array_equal(one["raw"][0], want_i) and np.array_equal(one["raw"][1], want_t)


# ---- 10. the pipeline
def _flat_proposal(model_dir):
    """(proposal, target, variable id of G, graph): uncor_1200code_v2p1 with N_initial{G} set to ones, and the shipped model"""
    target, parms, g = _model("uncor_1200code_v2p1", model_dir)
    proposal, _, _ = _model("uncor_1200code_v2p1", model_dir)
    v = next(v for v in range(target.n_initial) if not g["G_i"][:, v].any() and int(g["r_i"][v]) == 4)        # G: the root with 4 cells
    proposal.set_f64(L.F_N_INITIAL, v + 1, np.ones(4))
    return proposal, target, v, g


@pytest.mark.parametrize("mode", [AUTO, PER_STEP])
def test_reweight_count_host_equals_its_three_steps(gpu_ctx, model_dir, mode):
    T, seed = 61, SEED + 2
    proposal, target, v, g = _flat_proposal(model_dir)
    got = native.reweight_count_host(gpu_ctx, proposal, target, N, T, seed, transition_mode=mode)
    s = native.sample_weighted_host(gpu_ctx, proposal, target, N, T, seed, raw=True, transition_mode=mode)
    w, log_scale = native.quantize_weights(s["log_weight_model"])
    want = native.count_dbn_weighted_host(gpu_ctx, proposal, s["init_bin"], s["dyn_bin"], T, w, mode, raw=True)
    assert np.array_equal(got["weights"], w) and got["weights"].dtype == np.uint32 and got["log_scale"] == log_scale
    assert np.array_equal(got["log_lik_proposal"], s["log_lik_proposal"]) and np.array_equal(got["log_lik_target"], s["log_lik_target"])
    assert np.array_equal(got["raw"][0], want["raw"][0]) and np.array_equal(got["raw"][1], want["raw"][1])
    for a, b in zip(got["N_initial"] + got["N_transition"], want["N_initial"] + want["N_transition"]):
        assert np.array_equal(a, b)
    assert got["kernel"] == s["kernel"] and got["score_kernel"] == s["score_kernel"] and got["count_kernel"] == want["kernel"] == _name(g, mode)
    wf = w.astype(np.float64)
    assert got["ess"] == wf.sum() ** 2 / (wf ** 2).sum() and 1.0 < got["ess"] < N
    assert int(w.max()) == 2 ** 24 - 1 and len(np.unique(w)) >= 4                 # the weight is 4 P(G): a value per cell of G
    want_i, want_t, _ = _ref(g, s["init_bin"], s["dyn_bin"], T, w, mode, target.n_transition)
    assert np.array_equal(got["raw"][0], want_i) and np.array_equal(got["raw"][1], want_t)
    again = native.reweight_count_host(gpu_ctx, proposal, target, N, T, seed, transition_mode=mode, counts=got["raw"])      # accumulates
    assert np.array_equal(again["raw"][0], 2 * want_i) and np.array_equal(again["raw"][1], 2 * want_t)


# ---- 11. meaning
def test_the_reweighted_count_estimates_the_target(gpu_ctx, model_dir):
    """Sampled under a proposal whose P(G) is flat and reweighted to the shipped model, the self-normalised estimate of the four cells of P(G)
    from the weighted N_initial{G} lies within 5 delta-method standard errors, sqrt(sum w_i^2 (1[g_i = c] - p_c)^2) / sum w_i, of the
    target (0.9448, 0.0110, 0.0315, 0.0127; weights up to 85 : 1, ess about 0.28 n), and the unweighted count of the same trace does not.
    The bound is derived, not measured: over 200 seeds of a numpy simulation with the shipped table the worst deviation was 3.1 standard
    errors.  The weights are a function of g alone, so the estimate depends on the sample only through the four counts of g.  The CPU
    oracle's sample for this seed (dbn_sample, whose bins the GPU's equal) deviates by 0.58, 0.77, 1.01 and 1.08 standard errors, checked on
    the oracle before the seed was committed."""
    n, T, seed = 200000, 5, 0x2571D
    proposal, target, v, g = _flat_proposal(model_dir)
    got = native.reweight_count_host(gpu_ctx, proposal, target, n, T, seed)
    s = native.sample_weighted_host(gpu_ctx, proposal, target, n, T, seed, raw=True)
    gi = s["init_bin"][v].astype(np.int64) - 1
    w = got["weights"].astype(np.float64)
    p = np.exp(np.asarray(target.log_prob(0, v + 1), dtype=np.float64).reshape(-1))
    assert p.shape == (4,) and abs(p.sum() - 1) < 1e-12 and p.max() > 0.9
    Nw = got["N_initial"][v][:, 0]
    assert np.array_equal(Nw, np.bincount(gi, weights=w, minlength=4))            # exact: sums of integers below 2^53
    est = Nw / Nw.sum()
    se = np.array([np.sqrt((w ** 2 * ((gi == c) - est[c]) ** 2).sum()) for c in range(4)]) / w.sum()
    dev = np.abs(est - p) / se
    print("estimate %s, target %s, deviations %s standard errors, ess %.0f = %.3f n" % (est, p, dev, got["ess"], got["ess"] / n))
    assert np.all(dev <= 5)
    assert 0.2 * n < got["ess"] < 0.4 * n
    plain = np.bincount(gi, minlength=4) / n                                      # the unweighted count: the proposal's flat P(G)
    far = np.abs(plain - p) / np.sqrt(p * (1 - p) / n)
    assert far.max() > 5
