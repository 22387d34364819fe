"""-m gpu: k_score_dbn against the numpy restatement of its definition (score_ref.score) summing the library's OWN table entries
(emgpu_model_log_prob): the same IEEE additions in the same order, so every comparison is bitwise (NaN lanes by isnan).  Traces come from
native.sample_dbn_host; each is scored by emgpu_score_dbn_host and by emgpu_score_dbn_device."""
import numpy as np
import pytest

import score_ref as R
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native
from em_model_manned_bayes_amd import encounter_model as E

pytestmark = pytest.mark.gpu

N, SEED = 777, 0x5C02E
AUTO, PER_STEP = L.TRANSITION_REFERENCE_AUTO, L.TRANSITION_PER_STEP
_paths, _traces = {}, {}


def _model(name, model_dir):
    """(a fresh NativeModel, parms, graph) of the model's .txt: tests that change priors or counts change their own copy"""
    if name not in _paths:
        _paths[name] = em_io.materialize_model(name, model_dir)
    parms = em_io.em_read(_paths[name])
    return parms["native"], parms, R.graph(parms)


def _trace(ctx, name, model_dir, n, T, mode=AUTO):
    """a trace of the model drawn once and shared (raw layout), with the model it was drawn from"""
    key = (name, n, T, mode)
    if key not in _traces:
        nm, parms, g = _model(name, model_dir)
        got = native.sample_dbn_host(ctx, nm, n, T, SEED, raw=True, pinned=False, transition_mode=mode)
        _traces[key] = (nm, parms, g, got["init_bin"].copy(), got["dyn_bin"].copy())
        for a in _traces[key][3:]:
            a.setflags(write=False)
    return _traces[key]


def _name(g, mode):
    return "k_score_dbn[per-step]" if (mode == PER_STEP or g["depend"]) else "k_score_dbn[frozen]"


def _device(ctx, nm, ib, db, n, T, mode, ld=0, col=0, sync=True):
    """emgpu_score_dbn_device over device copies of the raw arrays; outputs preset to 123.0 (n + 5 entries: the tail must stay)"""
    import torch
    dev = torch.device("cuda", 0)
    d_ib = torch.from_numpy(np.array(ib, order="C")).to(dev)
    d_db = None if db is None else torch.from_numpy(np.array(db, order="C").view(np.int32)).to(dev)
    ll = torch.full((n + 5,), 123.0, dtype=torch.float64, device=dev)
    ini = torch.full((n + 5,), 123.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    native.score_dbn_device(ctx, nm, native.score_params(n, T, mode, ld, col), d_ib.data_ptr(), 0 if d_db is None else d_db.data_ptr(),
                            ll.data_ptr(), ini.data_ptr())
    kernel = ctx.last_kernel()
    err = None
    if sync:
        try:
            ctx.sync()
        except L.EmgpuError as e:
            err = e
    torch.cuda.synchronize()
    ll, ini = ll.cpu().numpy(), ini.cpu().numpy()
    assert np.all(ll[n:] == 123.0) and np.all(ini[n:] == 123.0)
    return ll[:n], ini[:n], kernel, err


def _check(ctx, nm, parms, g, ib, db, T, mode):
    """host and device scores of the raw trace (ib [ni, n], db [G4, nd, n] or None) equal the reference's, bit for bit"""
    n = ib.shape[1]
    user_db = None if db is None else native.unpack_dyn_bin(db, T)
    want, want_ini = R.score(R.lib_tables(nm), g, ib.T, user_db, mode)
    assert not np.isnan(want).any()
    host = native.score_dbn_host(ctx, nm, ib, db, T, mode, raw=True)
    assert host["kernel"] == _name(g, mode), host["kernel"]
    assert R.same_bits(host["log_lik"], want) and R.same_bits(host["initial"], want_ini)
    ll, ini, kernel, err = _device(ctx, nm, ib, db, n, T, mode)
    assert err is None and kernel == _name(g, mode)
    assert R.same_bits(ll, want) and R.same_bits(ini, want_ini)
    return want, want_ini


@pytest.mark.parametrize("name,mode", [("uncor_1200code_v2p1", AUTO), ("uncor_1200code_v2p1", PER_STEP), ("uncor_1200code_v1", AUTO),
                                       ("glider_v1", AUTO), ("cor_v1", AUTO), ("balloon_v1", AUTO), ("balloon_v1", PER_STEP)])
def test_score_of_sampled_traces(gpu_ctx, model_dir, name, mode):
    T = 61
    nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, N, T, mode)
    assert g["depend"] == (name in ("uncor_1200code_v1", "glider_v1", "cor_v1"))
    want, ini = _check(gpu_ctx, nm, parms, g, ib, db, T, mode)
    assert np.isfinite(want).all() and np.all(want <= ini)      # the model drew the trace: possible, and less likely than its first column
    # the user-facing shapes and the class layer give the same numbers
    user = native.score_dbn_host(gpu_ctx, nm, ib.T, native.unpack_dyn_bin(db, T), T, mode)
    assert R.same_bits(user["log_lik"], want)
    if name == "glider_v1":
        m = E.EncounterModel(_paths[name], idxZeroBoundaries=(1, 2, 3))
        assert R.same_bits(m.log_likelihood(ib.T, native.unpack_dyn_bin(db, T), ctx=gpu_ctx), want)
        assert R.same_bits(m.log_likelihood(ib.T, ctx=gpu_ctx), ini)


def test_score_of_the_terminal_geometry_model(gpu_ctx, model_dir):
    nm, parms, g = _model("terminal_v3_radar_encounter_model", model_dir)
    assert nm.n_transition == 0 and nm.n_dyn == 0
    bins, _, _ = native.sample_bn_host(gpu_ctx, nm, N, SEED)
    ib = np.ascontiguousarray(bins.T)
    want, ini = _check(gpu_ctx, nm, parms, g, ib, None, 1, AUTO)
    assert R.same_bits(want, ini) and np.isfinite(want).all()
    _check(gpu_ctx, nm, parms, g, ib, None, 7, AUTO)            # no transition network: sample_time is of no consequence


@pytest.mark.parametrize("T", [1, 2, 4, 5, 61])
@pytest.mark.parametrize("name,mode", [("uncor_1200code_v2p1", AUTO), ("glider_v1", AUTO)])
def test_sample_times_around_the_packed_word(gpu_ctx, model_dir, name, mode, T):
    nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, N, T, mode)
    want, ini = _check(gpu_ctx, nm, parms, g, ib, db, T, mode)
    if T == 1:
        assert R.same_bits(want, ini)
        _check(gpu_ctx, nm, parms, g, ib, None, 1, mode)       # dyn_bin may be absent
    # the first T columns of a longer trace score the same: padding bytes and later columns are not read
    nm2, _, _, ib2, db2 = _trace(gpu_ctx, name, model_dir, N, 61, mode)
    if T > 1:
        G4 = (T + 3) // 4
        cut = native.score_dbn_host(gpu_ctx, nm2, ib2, np.ascontiguousarray(db2[:G4]), T, mode, raw=True)
        ref = R.score(R.lib_tables(nm2), g, ib2.T, native.unpack_dyn_bin(db2, 61)[:, :T], mode)[0]
        assert R.same_bits(cut["log_lik"], ref)


@pytest.mark.parametrize("n", [1, 64, 777])
def test_batch_sizes(gpu_ctx, model_dir, n):
    for name, mode in (("uncor_1200code_v2p1", PER_STEP), ("cor_v1", AUTO)):
        nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, n, 5, mode)
        _check(gpu_ctx, nm, parms, g, ib, db, 5, mode)


@pytest.mark.parametrize("name,mode", [("uncor_1200code_v2p1", AUTO), ("uncor_1200code_v1", AUTO)])
def test_ld_and_col_offset_with_poisoned_neighbours(gpu_ctx, model_dir, name, mode):
    T, LD, COL = 61, 1024, 100
    nm, parms, g, ib, db = _trace(gpu_ctx, name, model_dir, N, T, mode)
    want, want_ini = R.score(R.lib_tables(nm), g, ib.T, native.unpack_dyn_bin(db, T), mode)
    big_ib = np.full((ib.shape[0], LD), 0xEE, dtype=np.uint8)                  # bins no variable has: reading one would turn a lane NaN
    big_db = np.full((db.shape[0], db.shape[1], LD), 0xEEEEEEEE, dtype=np.uint32)
    big_ib[:, COL: COL + N] = ib
    big_db[:, :, COL: COL + N] = db
    ll, ini, _, err = _device(gpu_ctx, nm, big_ib, big_db, N, T, mode, ld=LD, col=COL)
    assert err is None and R.same_bits(ll, want) and R.same_bits(ini, want_ini)    # (_device: outputs beyond n untouched)
    host = native.score_dbn_host(gpu_ctx, nm, big_ib, big_db, T, mode, raw=True, n=N, col_offset=COL)
    assert R.same_bits(host["log_lik"], want) and R.same_bits(host["initial"], want_ini)
    with pytest.raises(L.EmgpuError) as ei:                                        # one column further reads a poisoned neighbour
        native.score_dbn_host(gpu_ctx, nm, big_ib, big_db, T, mode, raw=True, n=N, col_offset=COL + 1)
    assert ei.value.code == L.ERR_ARG and np.flatnonzero(np.isnan(ei.value.log_lik)).tolist() == [N - 1]


def test_initial_of_a_fully_preset_start_grid_is_its_log_weight(gpu_ctx, model_dir):
    T = 5
    nm, parms, g, ib, _ = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T, AUTO)
    grid = np.ascontiguousarray(ib.T).astype(np.int32)                             # every initial node preset, to bins the model can draw
    got = native.sample_dbn_host(gpu_ctx, nm, N, T, SEED + 1, raw=True, pinned=False, want_log_weight=True, start=grid)
    assert np.array_equal(got["init_bin"], ib)
    s = native.score_dbn_host(gpu_ctx, nm, got["init_bin"], got["dyn_bin"], T, AUTO, raw=True)
    assert R.same_bits(s["initial"], got["log_weight"]) and np.isfinite(got["log_weight"]).all()


def test_proposal_and_target_and_sample_weighted_host(gpu_ctx, model_dir):
    T = 61
    prop, parms, g = _model("uncor_1200code_v2p1", model_dir)
    targ, _, _ = _model("uncor_1200code_v2p1", model_dir)
    prop.set_prior(1.0)
    got = native.sample_weighted_host(gpu_ctx, prop, targ, N, T, SEED)
    plain = native.sample_dbn_host(gpu_ctx, prop, N, T, SEED, pinned=False)
    for f in ("init_bin", "init_val", "dyn_bin", "dyn_val", "attempts"):
        assert got[f].dtype == plain[f].dtype and np.array_equal(got[f], plain[f]), f
    assert got["kernel"].startswith("k_") and got["score_kernel"] == "k_score_dbn[frozen]"
    want_p = R.score(R.lib_tables(prop), g, got["init_bin"], got["dyn_bin"], AUTO)[0]
    want_t = R.score(R.lib_tables(targ), g, got["init_bin"], got["dyn_bin"], AUTO)[0]
    assert R.same_bits(got["log_lik_proposal"], want_p) and R.same_bits(got["log_lik_target"], want_t)
    assert R.same_bits(got["log_weight_model"], want_t - want_p)
    assert np.isfinite(want_p).all()                                               # a constant prior makes everything possible ...
    assert np.isneginf(want_t).any() and np.isfinite(want_t).any()                 # ... the counts alone do not
    assert not np.isnan(got["log_weight_model"]).any()


def test_sample_weighted_host_with_a_start_grid_and_with_an_index_list(gpu_ctx, model_dir):
    """numpy `start` / `indices` reach the device kernel as device copies: the trace, the attempts and the grid's log-weights are those of
    sample_dbn_host for the same arguments, and the scores are the reference's"""
    T = 21
    prop, parms, g = _model("uncor_1200code_v2p1", model_dir)
    targ, _, _ = _model("uncor_1200code_v2p1", model_dir)
    prop.set_prior(1.0)
    grid = np.zeros((N, prop.n_initial), dtype=np.int32)
    grid[:, 0] = 1 + np.arange(N) % 4                       # G, a root: every row presets it, trajectory i to bin 1 + i % 4
    grid[::3, 1] = 2                                        # A (its only parent is G) in every third row
    rs = np.random.RandomState(11)
    idx = rs.randint(0, 2 ** 40, size=N).astype(np.uint64)
    for kw in (dict(start=grid), dict(indices=idx), dict(start=grid, first_index=5000)):
        lw = "start" in kw
        got = native.sample_weighted_host(gpu_ctx, prop, targ, N, T, SEED, want_log_weight=lw, **kw)
        plain = native.sample_dbn_host(gpu_ctx, prop, N, T, SEED, pinned=False, want_log_weight=lw, **kw)
        for f in ("init_bin", "init_val", "dyn_bin", "dyn_val", "attempts") + (("log_weight",) if lw else ()):
            assert got[f].dtype == plain[f].dtype and np.array_equal(got[f], plain[f]), (sorted(kw), f)
        if lw:
            assert np.array_equal(got["init_bin"][:, 0], grid[:, 0]) and np.all(got["init_bin"][::3, 1] == 2)
            assert R.same_bits(got["log_weight"], native.start_grid_log_weight(prop, grid))
        want_p = R.score(R.lib_tables(prop), g, got["init_bin"], got["dyn_bin"], AUTO)[0]
        want_t = R.score(R.lib_tables(targ), g, got["init_bin"], got["dyn_bin"], AUTO)[0]
        assert R.same_bits(got["log_lik_proposal"], want_p) and R.same_bits(got["log_lik_target"], want_t)
        assert R.same_bits(got["log_weight_model"], want_t - want_p) and np.isfinite(want_p).all()
    for bad in (dict(start=grid[:-1]), dict(start=12345), dict(indices=idx[:-1]), dict(indices=12345)):
        with pytest.raises(ValueError):
            native.sample_weighted_host(gpu_ctx, prop, targ, N, T, SEED, **bad)
    with pytest.raises(TypeError):
        native.sample_weighted_host(gpu_ctx, prop, targ, N, T, SEED, want_events=True)


def test_a_pending_device_report_is_not_a_host_calls(gpu_ctx, model_dir):
    """a _device call's bad-bin report stays pending through a _host call on a valid trace, which is served without an error of its own,
    and is returned by the next sync; a _host call on the corrupt trace reports its own and leaves nothing behind"""
    T = 5
    nm, parms, g, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T, AUTO)
    want = R.score(R.lib_tables(nm), g, ib.T, native.unpack_dyn_bin(db, T), AUTO)[0]
    bad_ib = ib.copy()
    bad_ib[0, 9] = 0
    ll = _device(gpu_ctx, nm, bad_ib, db, N, T, AUTO, sync=False)[0]
    assert np.flatnonzero(np.isnan(ll)).tolist() == [9]
    host = native.score_dbn_host(gpu_ctx, nm, ib, db, T, AUTO, raw=True)          # valid: no error, although one is pending
    assert R.same_bits(host["log_lik"], want)
    with pytest.raises(L.EmgpuError) as ei:
        gpu_ctx.sync()
    assert ei.value.code == L.ERR_ARG and "outside 1..r" in str(ei.value)
    gpu_ctx.sync()
    with pytest.raises(L.EmgpuError):
        native.score_dbn_host(gpu_ctx, nm, bad_ib, db, T, AUTO, raw=True)
    gpu_ctx.sync()                                                                # the host call's report went with its return value


def test_device_upload_and_download_round_trip(gpu_ctx):
    a = np.arange(100003, dtype=np.uint32)
    addr = gpu_ctx.device_alloc(a.nbytes)
    try:
        native.device_upload(gpu_ctx, addr, a)
        assert np.array_equal(native.device_download(gpu_ctx, addr, np.zeros_like(a)), a)
        assert np.array_equal(native.device_download(gpu_ctx, addr + 4 * 77, np.zeros(5, np.uint32)), a[77:82])
    finally:
        gpu_ctx.device_free(addr)


def test_a_corrupt_trace_gives_nan_for_its_trajectories_only(gpu_ctx, model_dir):
    T = 61
    nm, parms, g, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T, PER_STEP)
    want, want_ini = R.score(R.lib_tables(nm), g, ib.T, native.unpack_dyn_bin(db, T), PER_STEP)
    ib2, db2 = ib.copy(), native.unpack_dyn_bin(db, T)
    r_i, r_d = g["r_i"], g["r_t"][g["tm"][:, 1]]
    ib2[3, 5] = 0                       # an initial node: bin 0 ...
    ib2[6, 70] = r_i[6] + 1             # ... and bin r + 1
    db2[200, 7, 1] = 0                  # a transition byte: bin 0 ...
    db2[500, 60, 2] = r_d[2] + 1        # ... and bin r + 1, in the partly filled last word
    db2[640, 0, 0] = 255                # column 0 is read as a parent
    lanes, ini_lanes = [5, 70, 200, 500, 640], [5, 70]
    db2 = native.pack_dyn_bin(db2)
    ref, ref_ini = R.score(R.lib_tables(nm), g, ib2.T, native.unpack_dyn_bin(db2, T), PER_STEP)
    assert np.flatnonzero(np.isnan(ref)).tolist() == lanes and np.flatnonzero(np.isnan(ref_ini)).tolist() == ini_lanes
    keep = np.ones(N, dtype=bool)
    keep[lanes] = False
    with pytest.raises(L.EmgpuError) as ei:
        native.score_dbn_host(gpu_ctx, nm, ib2, db2, T, PER_STEP, raw=True)
    assert ei.value.code == L.ERR_ARG and "outside 1..r" in str(ei.value)
    for got, got_ini in ((ei.value.log_lik, ei.value.initial), _device(gpu_ctx, nm, ib2, db2, N, T, PER_STEP, sync=False)[:2]):
        assert np.flatnonzero(np.isnan(got)).tolist() == lanes and np.flatnonzero(np.isnan(got_ini)).tolist() == ini_lanes
        assert R.same_bits(got[keep], want[keep]) and R.same_bits(got_ini[keep], want_ini[keep])
    with pytest.raises(L.EmgpuError) as ei:          # the device call's error is a deferred one
        gpu_ctx.sync()
    assert ei.value.code == L.ERR_ARG and "outside 1..r" in str(ei.value)
    gpu_ctx.sync()                                   # reported once
    _check(gpu_ctx, nm, parms, g, ib, db, T, PER_STEP)   # and a valid call is served


def test_many_host_chunks_equal_one(gpu_ctx, model_dir, monkeypatch):
    n, T = 20011, 160
    nm, parms, g, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, n, T, AUTO)
    one = native.score_dbn_host(gpu_ctx, nm, ib, db, T, AUTO, raw=True)
    assert gpu_ctx.last_launches() == 1
    monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", "1")
    many = native.score_dbn_host(gpu_ctx, nm, ib, db, T, AUTO, raw=True)
    assert gpu_ctx.last_launches() >= 8
    assert R.same_bits(many["log_lik"], one["log_lik"]) and R.same_bits(many["initial"], one["initial"])
    want = R.score(R.lib_tables(nm), g, ib.T, native.unpack_dyn_bin(db, T), AUTO)[0]
    assert R.same_bits(one["log_lik"], want) and np.isfinite(want).all()


def test_the_score_follows_the_model_on_the_same_context(gpu_ctx, model_dir):
    T = 61
    _, _, _, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T, AUTO)
    nm, parms, g = _model("uncor_1200code_v2p1", model_dir)     # a copy of its own: this test changes it
    user_db = native.unpack_dyn_bin(db, T)

    def both():
        want = R.score(R.lib_tables(nm), g, ib.T, user_db, AUTO)[0]
        got = native.score_dbn_host(gpu_ctx, nm, ib, db, T, AUTO, raw=True)["log_lik"]
        assert R.same_bits(got, want)
        return got
    first = both()
    nm.set_prior(1.0)
    second = both()
    assert not np.array_equal(first, second)
    tv = int(g["tm"][1, 1])                                     # one (t+1) node: new counts
    Nt = nm.get_f64(L.F_N_TRANSITION, tv + 1)
    nm.set_f64(L.F_N_TRANSITION, tv + 1, Nt[::-1].copy())
    third = both()
    assert not np.array_equal(second, third)
    nm.set_transition_stay_prior(5.0)
    assert not np.array_equal(third, both())
