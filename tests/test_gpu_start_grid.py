"""-m gpu: start grids on the fast kernels -- the +start instances of k_uncor_fast_idx / k_uncor_fast_evu / _evu_long against the oracle, against
the library's own model-start path and against k_dbn_generic (which still serves the list and the dense trace together); the grid through the
index list, the chunked host paths, the class layer, em_sample and the track rounds.  Inputs and the oracle's answers: start_grid_cases.py.

Trajectory i gets rows[i % 6]: every wave holds all six rows.  Bins, attempts, counts and rows are compared bit for bit, f32 values with the
oracle's f64 rounded to f32 (util.assert_uncor_parity); log-weights with start_log_weight within 1e-12 and bit for bit with the host function."""
import ctypes as C
import filecmp

import numpy as np
import pytest

import oracle as O
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, legacy, native
from em_model_manned_bayes_amd import encounter_model as E
import start_grid_cases as S
from test_gpu_lazy_sample import assert_lazy_equals_eager
from util import assert_uncor_parity, load_pair, uncor_indices

pytestmark = pytest.mark.gpu

N, T, SEED, FIRST = S.N, S.T, S.SEED, S.FIRST
DENSE_FIELDS = ("init_bin", "init_val", "attempts", "dyn_bin", "dyn_val")
LIST_FIELDS = ("init_bin", "init_val", "attempts", "ev_count")
_both_cache = {}


def _call(ctx, nm, idx, form, n=N, log_weight=True, **kw):
    kw.setdefault("first_index", FIRST)
    return native.sample_dbn_host(ctx, nm, n, T, SEED, want_dense=form != "list", want_events=form != "dense", want_log_weight=log_weight,
                                  **dict(idx, **kw))


def _assert_same(a, b, form, rows=None, what=""):
    """every field of call a equals the rows `rows` (all of them: None) of call b"""
    pick = (lambda v: v) if rows is None else (lambda v: v[rows] if isinstance(v, np.ndarray) else [v[r] for r in rows])
    for f in (DENSE_FIELDS if form == "dense" else LIST_FIELDS):
        assert a[f].dtype == b[f].dtype and np.array_equal(a[f], pick(b[f])), (what, f)
    if form == "list":
        assert all(np.array_equal(x, y) for x, y in zip(a["events"], pick(b["events"]))), (what, "events")


def _name_ok(kernel, form):
    return kernel.endswith("+start") and kernel.startswith("k_uncor_fast_idx<" if form == "dense" else "k_uncor_fast_evu")


def _generic_both(ctx, nm, idx, name, grid):
    """the same grid through the list-plus-dense form, which stays on k_dbn_generic (one call per model, shared)"""
    if name not in _both_cache:
        _both_cache[name] = _call(ctx, nm, idx, "both", start=grid)
        assert _both_cache[name]["kernel"].startswith("k_dbn_generic"), _both_cache[name]["kernel"]
    return _both_cache[name]


def _device_call(ctx, nm, idx, form, grid):
    """emgpu_sample_dbn_device at column COL of arrays dimensioned LD: the leading COL & 255 lanes of workgroup 0 and the tail lanes have no
    trajectory and must read no row of the grid (which has exactly N rows) and write nothing."""
    import torch
    dev = torch.device("cuda", 0)
    ni, nd, G4, ld, col = nm.n_initial, nm.n_dyn, (T + 3) // 4, S.LD, S.COL
    cap = (ni + nd + 1) * T + 2
    buf = {"init_bin": torch.full((ni, ld), 0xEE, dtype=torch.uint8, device=dev), "init_val": torch.full((ni, ld), -77.0, dtype=torch.float32, device=dev),
           "attempts": torch.full((ld,), -7, dtype=torch.int32, device=dev)}
    if form == "dense":
        buf["dyn_bin"] = torch.full((G4, nd, ld), -0x5A5A5A5B, dtype=torch.int32, device=dev)
        buf["dyn_val"] = torch.full((G4, nd, ld, 4), -77.0, dtype=torch.float32, device=dev)
    else:
        buf["ev_count"] = torch.full((ld,), -7, dtype=torch.int32, device=dev)
        buf["events"] = torch.full((ld, cap, 2), -7, dtype=torch.int32, device=dev)
    lw = torch.full((N,), 123.0, dtype=torch.float64, device=dev)
    g = torch.from_numpy(grid).to(dev)
    assert g.dtype == torch.int32 and g.is_contiguous() and tuple(g.shape) == (N, ni)
    torch.cuda.synchronize()
    p, _keep = native.make_params(N, T, SEED, first_index=FIRST, event_cap=cap if form == "list" else 0, start=g.data_ptr(), **idx)
    native.sample_dbn_device(ctx, nm, p, ld=ld, col_offset=col, log_weight=lw.data_ptr(), **{k: v.data_ptr() for k, v in buf.items()})
    ctx.sync()
    kernel = ctx.last_kernel()
    h = {k: v.cpu().numpy() for k, v in buf.items()}
    out = np.ones(ld, dtype=bool)
    out[col: col + N] = False
    assert np.all(h["init_bin"][:, out] == 0xEE) and np.all(h["init_val"][:, out] == -77.0) and np.all(h["attempts"][out] == -7)
    got = {"kernel": kernel, "log_weight": lw.cpu().numpy(), "init_bin": h["init_bin"][:, col: col + N].T, "init_val": h["init_val"][:, col: col + N].T,
           "attempts": h["attempts"][col: col + N]}
    if form == "dense":
        assert np.all(h["dyn_bin"][:, :, out] == -0x5A5A5A5B) and np.all(h["dyn_val"][:, :, out] == -77.0)
        got["dyn_bin"] = native.unpack_dyn_bin(np.ascontiguousarray(h["dyn_bin"].view(np.uint32)[:, :, col: col + N]), T)
        got["dyn_val"] = native.unpack_dyn_val(np.ascontiguousarray(h["dyn_val"][:, :, col: col + N]), T)
    else:
        assert np.all(h["ev_count"][out] == -7) and np.all(h["events"][out] == -7)
        cnt = h["ev_count"][col: col + N].astype(np.uint32)
        evh = h["events"].reshape(ld, cap * 2).view(native.EVENT_DTYPE)
        got["ev_count"], got["events"] = cnt, [evh[col + i, : cnt[i]] for i in range(N)]
    return got


@pytest.mark.parametrize("form", ["dense", "list"])
@pytest.mark.parametrize("name", S.MODELS)
def test_start_grid_on_the_fast_kernels(name, form, gpu_ctx, model_dir):
    nm, pp, _ = load_pair(name, model_dir)
    idx = uncor_indices(pp)
    rows, grid, ref = S.rows_of(name, model_dir), S.grid_of(name, model_dir), S.oracle_of(name, model_dir)
    got = _call(gpu_ctx, nm, idx, form, start=grid)
    assert _name_ok(got["kernel"], form), got["kernel"]
    if name == "haa_v1" and form == "list":
        assert got["kernel"] == "k_uncor_fast_evu_long<9,6,6,6>+start"
    assert_uncor_parity(got, ref, T)
    # the device-pointer call at a column offset: the same numbers, nothing outside its columns
    dev = _device_call(gpu_ctx, nm, idx, form, grid)
    assert dev["kernel"] == got["kernel"]
    _assert_same(dev, got, form, what="device call")
    assert np.array_equal(dev["log_weight"], got["log_weight"])
    # the library's own model-start path: the model's start set to the row, the row's trajectories through an index list
    try:
        for k, row in enumerate(rows):
            nm.set_start([int(v) or None for v in row])
            own = _call(gpu_ctx, nm, idx, form, n=len(range(k, N, 6)), log_weight=False, first_index=0,
                        indices=(FIRST + np.arange(k, N, 6)).astype(np.uint64))
            assert not own["kernel"].endswith("+start") and own["kernel"].startswith("k_uncor_fast"), own["kernel"]
            _assert_same(own, got, form, rows=np.arange(k, N, 6), what="row %d" % k)
            # log-weights: the row's start_log_weight (the tolerance of test_host.py::test_start_log_weight)
            assert np.all(got["log_weight"][k::6] == got["log_weight"][k]) and abs(got["log_weight"][k] - nm.start_log_weight()) < 1e-12, k
    finally:
        nm.set_start([None] * nm.n_initial)
    assert got["log_weight"][1] == 0.0 and np.all(got["log_weight"][np.arange(N) % 6 != 1] < 0)
    assert np.array_equal(got["log_weight"], native.start_grid_log_weight(nm, grid))        # bit for bit
    # the list-plus-dense form of the same grid runs on k_dbn_generic: its arrays and lists equal the new form's
    both = _generic_both(gpu_ctx, nm, idx, name, grid)
    _assert_same(got, both, form, what="k_dbn_generic")
    assert np.array_equal(got["log_weight"], both["log_weight"])


@pytest.mark.parametrize("form", ["dense", "list"])
@pytest.mark.parametrize("name", S.MODELS)
def test_an_index_list_with_its_rows_of_the_grid(name, form, gpu_ctx, model_dir):
    """A permuted subset of 300 of the 700 with the gathered grid rows: those rows of the full call (the lane's row is the lane's, whatever
    its global index)."""
    nm, pp, _ = load_pair(name, model_dir)
    idx = uncor_indices(pp)
    grid = S.grid_of(name, model_dir)
    full = _call(gpu_ctx, nm, idx, form, start=grid)
    pick = np.random.RandomState(11).permutation(N)[:300]
    assert np.any(np.diff(pick) < 0) and len(set((pick % 6).tolist())) == 6
    sub = _call(gpu_ctx, nm, idx, form, n=300, first_index=0, indices=(FIRST + pick).astype(np.uint64), start=np.ascontiguousarray(grid[pick]))
    assert sub["kernel"] == full["kernel"] and _name_ok(sub["kernel"], form)
    _assert_same(sub, full, form, rows=pick)
    assert np.array_equal(sub["log_weight"], full["log_weight"][pick])


def _ctrl(pp):
    labs = pp["labels_initial"]
    return tuple(labs.index('"%s"' % s) + 1 for s in ("\\dot h", "\\dot \\psi", "\\dot v"))


def test_the_chunked_host_paths_read_their_own_rows(gpu_ctx, model_dir, tmp_path, monkeypatch):
    """2 500 trajectories in three chunks of 1 024 (1 024 is no multiple of 6: chunk k reads the grid from row 1 024 k on) against one chunk,
    through the three host-pointer entry points; the text bytes are em_sample(text="host", start_grid=...)'s."""
    name, n = "uncor_1200code_v2p1", 2500
    nm, pp, path = load_pair(name, model_dir)
    idx, grid = uncor_indices(pp), S.grid_of(name, model_dir, n)
    calls = {
        "dbn": lambda: native.sample_dbn_host(gpu_ctx, nm, n, T, SEED, first_index=FIRST, want_dense=True, want_log_weight=True, start=grid, **idx),
        "uncor": lambda: native.sample_uncor_host(gpu_ctx, nm, n, T, SEED, _ctrl(pp), first_index=FIRST, start=grid, **idx),
        "text": lambda: native.sample_text_host(gpu_ctx, nm, n, T, SEED, max_attempts=1, start=grid),   # em_sample's own call
    }
    fields = {"dbn": DENSE_FIELDS + ("log_weight",), "uncor": ("inits", "ev_count", "events", "ctrl_count", "controls", "samples", "attempts"),
              "text": ("initial", "transition", "init_val", "dyn_val")}
    want_kernel = {"dbn": "k_uncor_fast_idx<7,2,4,2>+start", "uncor": "k_uncor_fast_evu<7,2,4,2>+start", "text": "k_uncor_fast_idx<7,2,4,2>+start"}
    res = {}
    for mb, chunks in (("8192", 1), ("1", 3)):
        monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", mb)
        for what, fn in calls.items():
            r = fn()
            assert r["host_stats"]["chunks"] == chunks and r["kernel"] == want_kernel[what], (what, r["host_stats"], r["kernel"])
            res[what, chunks] = {f: np.array(r[f]) for f in fields[what]}
    for what in calls:
        for f in fields[what]:
            a, b = res[what, 3][f], res[what, 1][f]
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (what, f)
    # one chunk is right: the oracle on the first 700 (the same interleaving), and the lazy outputs' inits are the dense call's
    sub = {f: res["dbn", 1][f][:N] for f in DENSE_FIELDS}
    assert_uncor_parity(sub, S.oracle_of(name, model_dir), T)
    assert np.array_equal(res["uncor", 1]["inits"].astype(np.float32), res["dbn", 1]["init_val"])
    fi, ft = str(tmp_path / "i.txt"), str(tmp_path / "t.txt")
    legacy.em_sample(path, fi, ft, num_initial_samples=n, num_transition_samples=T, rng_seed=SEED, ctx=gpu_ctx, start_grid=grid)
    body = lambda f: open(f, "rb").read().split(b"\n", 1)[1]
    assert res["text", 3]["initial"].tobytes() == body(fi) and res["text", 3]["transition"].tobytes() == body(ft)


def test_the_class_layer_eager_lazy_and_per_row(gpu_ctx, model_dir):
    name = "uncor_1200code_v2p1"
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model(name, model_dir))
    rows, grid = S.rows_of(name, model_dir), S.grid_of(name, model_dir)
    eager = mdl.sample(N, T, seed=SEED, first_index=FIRST, ctx=gpu_ctx, start_grid=grid, return_log_weight=True)
    assert gpu_ctx.last_kernel() == "k_uncor_fast_evu<7,2,4,2>+start"
    lazy = mdl.sample(N, T, seed=SEED, first_index=FIRST, ctx=gpu_ctx, start_grid=grid, return_log_weight=True, lazy=True)
    assert gpu_ctx.last_kernel() == "k_uncor_fast_evu<7,2,4,2>+start"
    assert len(eager) == 5 and len(lazy) == 5
    assert_lazy_equals_eager(lazy[:4], eager[:4])
    assert np.array_equal(eager[4], lazy[4]) and np.array_equal(eager[4], native.start_grid_log_weight(mdl.native, grid))
    ref = S.oracle_of(name, model_dir)
    assert np.array_equal(eager[0].astype(np.float32), ref["init_val"].astype(np.float32))
    assert all(np.array_equal(e[:, :2], r[:, :2]) for e, r in zip(eager[1], ref["events"]))
    assert len(mdl.sample(N, T, seed=SEED, first_index=FIRST, ctx=gpu_ctx, start_grid=grid)) == 4       # the four outputs without the switch
    try:
        for k, row in enumerate(rows):                                     # rows i = k mod 6 are the model-level start's
            mdl.start = [int(v) or None for v in row]
            one = mdl.sample(N, T, seed=SEED, first_index=FIRST, ctx=gpu_ctx)
            assert not gpu_ctx.last_kernel().endswith("+start")
            assert abs(mdl.start_log_weight - eager[4][k]) < 1e-12
            assert np.array_equal(one[0][k::6], eager[0][k::6]), k
            for i in range(k, N, 6):
                assert np.array_equal(one[1][i], eager[1][i]) and np.array_equal(one[2][i], eager[2][i]) and np.array_equal(one[3][i].event, eager[3][i].event), i
    finally:
        mdl.preallocStart()
    # list-like grids with None for "unset", as CorTerminalModel.sample takes them
    as_list = [[int(v) or None for v in r] for r in grid[:50]]
    again = mdl.sample(50, T, seed=SEED, first_index=FIRST, ctx=gpu_ctx, start_grid=as_list)
    assert np.array_equal(again[0], eager[0][:50])
    with pytest.raises(ValueError):
        mdl.sample(49, T, seed=SEED, ctx=gpu_ctx, start_grid=as_list)


def test_em_sample_with_a_grid_writes_the_same_files_under_both_writers(gpu_ctx, model_dir, tmp_path):
    name = "uncor_1200only_fwse_v1p2"
    path = em_io.materialize_model(name, model_dir)
    grid = S.grid_of(name, model_dir)
    names = [str(tmp_path / ("%s_%s.txt" % (w, f))) for w in ("host", "device") for f in ("initial", "transition")]
    host = legacy.em_sample(path, names[0], names[1], num_initial_samples=N, num_transition_samples=T, rng_seed=SEED, ctx=gpu_ctx, start_grid=grid)
    k_host = gpu_ctx.last_kernel()
    dev = legacy.em_sample(path, names[2], names[3], num_initial_samples=N, num_transition_samples=T, rng_seed=SEED, ctx=gpu_ctx, start_grid=grid,
                           text="device", text_batch=256)                # three batches: batch b reads the grid from row 256 b on
    assert k_host == gpu_ctx.last_kernel() == "k_uncor_fast_idx<7,4,6,6>+start"
    assert filecmp.cmp(names[0], names[2], shallow=False) and filecmp.cmp(names[1], names[3], shallow=False)
    assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1])
    rows = S.rows_of(name, model_dir)
    for k in (0, 2, 3, 4, 5):                                              # the preset root variable (a categorical one: its value is its bin)
        assert np.all(host[0][k::6, 0] == rows[k][0]), k
    # the model-level `start` stays, and a row's own entry wins over it
    st = [2] + [None] * 6
    both = legacy.em_sample(path, names[0], names[1], num_initial_samples=60, num_transition_samples=8, rng_seed=SEED, ctx=gpu_ctx, start=st, start_grid=grid[:60])
    assert np.all(both[0][1::6, 0] == 2) and np.all(both[0][2::6, 0] == 3)


# ------------------------------------------------------------------------------------------------ track
TN, TT, TSEED = 300, 30, 5


def _track_call(ctx, nm, grid, max_track_attempts):
    """emgpu_track_uncor_grid_host through ctypes (grid None: NULL, i.e. emgpu_track_uncor_host): the status and the arrays, also when the
    round cap is hit (native.track_uncor_host raises then)."""
    p = native.utrack_params(nm, TN, TT, TSEED, max_track_attempts=max_track_attempts)
    tracks, limits, attempts = np.zeros((TN, 10 * TT + 1, 8)), np.zeros((TN, 3)), np.zeros(TN, dtype=np.int32)
    g = None if grid is None else np.ascontiguousarray(grid, dtype=np.int32)
    rc = L.lib().emgpu_track_uncor_grid_host(ctx._h, nm._h, C.byref(p), None if g is None else g.ctypes.data, tracks.ctypes.data, limits.ctypes.data,
                                             attempts.ctypes.data)
    return rc, tracks, limits, attempts, ctx.last_kernel(), L.lib().emgpu_last_error().decode()


def test_track_rounds_read_the_rows_of_the_trajectories_they_redraw(gpu_ctx, model_dir):
    """All six rows, eight rounds.  Row R4 (the lowest speed bin) cannot fly: the oracle rejects its 50 trajectories in every round, so they
    stay in the slot list to the last round, next to the trajectories of the other rows that need two or three rounds -- attempts (the -1 of
    the 50 included) against the oracle per row, tracks and limits against the library's own per-row calls."""
    name = "uncor_1200code_v2p1"
    nm, pp, _ = load_pair(name, model_dir)
    rows, grid = S.rows_of(name, model_dir), S.grid_of(name, model_dir, TN)
    want, per_row = np.zeros(TN, dtype=np.int32), []
    for k, row in enumerate(rows):
        per_row.append(O.uncor_track(O.OracleModel(pp, start=[int(v) for v in row]), TN, TT, TSEED, max_track_attempts=8, want_tracks=False)["attempts"])
        want[k::6] = per_row[k][k::6]
    later = (want > 1) & (np.arange(TN) % 6 != 4)
    assert later.sum() >= 4 and want.max() >= 3 and np.all(want[4::6] == -1) and np.all(want[np.arange(TN) % 6 != 4] > 0)   # (checked before the seed was fixed)
    rc, tracks, limits, attempts, kernel, msg = _track_call(gpu_ctx, nm, grid, 8)
    assert rc == L.ERR_REJECT_CAP and "50 trajectories" in msg, (rc, msg)
    assert np.array_equal(attempts, want)
    sampler, tracker = kernel.split(" + ")
    assert sampler == "k_uncor_fast_idx<7,2,4,2>+start" and tracker.startswith("k_uncor_track"), kernel     # round 7: R4's lanes through the slot list
    rc1, _, _, att1, kernel1, _ = _track_call(gpu_ctx, nm, grid, 1)
    assert rc1 == L.ERR_REJECT_CAP and kernel1.split(" + ")[0] == sampler                                  # round 0
    assert np.array_equal(att1 == 1, want == 1)
    try:
        for k, row in enumerate(rows):
            nm.set_start([int(v) or None for v in row])
            rck, tk, lk, ak, kk, _ = _track_call(gpu_ctx, nm, None, 8)
            assert rck == (L.ERR_REJECT_CAP if np.any(per_row[k] < 0) else L.OK) and not kk.split(" + ")[0].endswith("+start"), (k, rck, kk)
            assert np.array_equal(ak, per_row[k]), k
            ok = np.flatnonzero((np.arange(TN) % 6 == k) & (want > 0))
            assert np.array_equal(ak[k::6], attempts[k::6]) and np.array_equal(tk[ok], tracks[ok]) and np.array_equal(lk[ok], limits[ok]), k
    finally:
        nm.set_start([None] * nm.n_initial)


def test_the_class_track_with_a_grid(gpu_ctx, model_dir):
    """UncorEncounterModel.track(start_grid=...).  With all six rows the call ends as the oracle says it must: R4's 50 trajectories are still
    rejected after max_track_attempts rounds.  The five rows that can fly, interleaved the same way: attempts against the oracle per row, the
    tracks against the per-row class calls bit for bit, the weights as the last output."""
    name = "uncor_1200code_v2p1"
    nm, pp, path = load_pair(name, model_dir)
    mdl = E.UncorEncounterModel(parameters_filename=path)
    rows = S.rows_of(name, model_dir)
    r4 = O.uncor_track(O.OracleModel(pp, start=[int(v) for v in rows[4]]), TN, TT, TSEED, want_tracks=False)["attempts"][4::6]
    assert np.all(r4 == -1) and r4.size == 50
    with pytest.raises(L.EmgpuError) as ei:
        mdl.track(TN, TT, initialSeed=TSEED, ctx=gpu_ctx, start_grid=S.grid_of(name, model_dir, TN), return_info=True)
    assert ei.value.code == L.ERR_REJECT_CAP and "50 trajectories" in str(ei.value)
    assert gpu_ctx.last_kernel().split(" + ")[0] == "k_uncor_fast_idx<7,2,4,2>+start"
    fly = rows[[0, 1, 2, 3, 5]]
    grid = np.ascontiguousarray(fly[np.arange(TN) % 5])
    res, info, lw = mdl.track(TN, TT, initialSeed=TSEED, ctx=gpu_ctx, start_grid=grid, return_info=True, return_log_weight=True)
    assert info["kernel"].split(" + ")[0] == "k_uncor_fast_idx<7,2,4,2>+start"
    assert len(res) == TN and set(res[0]) == set(E.UncorEncounterModel.TRACK_FIELDS) and res[0]["time_s"].shape == (10 * TT + 1,)
    assert np.array_equal(lw, native.start_grid_log_weight(nm, grid))
    only = mdl.track(TN, TT, initialSeed=TSEED, ctx=gpu_ctx, start_grid=grid)
    assert isinstance(only, list) and len(only) == TN and np.array_equal(only[7]["up_ft"], res[7]["up_ft"])
    try:
        for k, row in enumerate(fly):
            ref = O.uncor_track(O.OracleModel(pp, start=[int(v) for v in row]), TN, TT, TSEED, want_tracks=False)
            assert np.array_equal(info["attempts"][k::5], ref["attempts"][k::5]), k
            mdl.start = [int(v) or None for v in row]
            one, info1 = mdl.track(TN, TT, initialSeed=TSEED, ctx=gpu_ctx, return_info=True)
            assert np.array_equal(info1["tracks"][k::5], info["tracks"][k::5]) and np.array_equal(info1["limits"][k::5], info["limits"][k::5]), k
            assert all(np.array_equal(one[i][f], res[i][f]) for i in range(k, TN, 5) for f in E.UncorEncounterModel.TRACK_FIELDS)
    finally:
        mdl.preallocStart()
    assert info["attempts"].max() > 1                                      # some trajectory went through a later round's slot list


# ------------------------------------------------------------------------------------------------ errors
def test_bad_rows_are_refused_and_the_context_serves_the_next_call(gpu_ctx, model_dir, tmp_path):
    name = "uncor_1200code_v2p1"
    nm, pp, path = load_pair(name, model_dir)
    mdl = E.UncorEncounterModel(parameters_filename=path)
    idx, good = uncor_indices(pp), S.grid_of(name, model_dir)
    for bad_row in ([0, 0, 2, 0, 0, 0, 0], [9, 0, 0, 0, 0, 0, 0]):       # L without its parents; bin 9 of G
        grid = good.copy()
        grid[397] = bad_row
        sampling_calls = [
            lambda: _call(gpu_ctx, nm, idx, "dense", start=grid),
            lambda: _call(gpu_ctx, nm, idx, "list", start=grid),
            lambda: native.sample_uncor_host(gpu_ctx, nm, N, T, SEED, _ctrl(pp), first_index=FIRST, start=grid, **idx),
            lambda: native.sample_text_host(gpu_ctx, nm, N, T, SEED, start=grid),
            lambda: native.track_uncor_host(gpu_ctx, nm, N, TT, TSEED, start=np.where((np.arange(N) % 6 == 4)[:, None], good[0], grid)),
        ]
        for q, fn in enumerate(sampling_calls):
            with pytest.raises(L.EmgpuError) as ei:
                fn()
            assert ei.value.code == L.ERR_PRESET, (q, str(ei.value))
            ok = _call(gpu_ctx, nm, idx, "dense", start=good)             # a valid call on the same ctx afterwards
            assert _name_ok(ok["kernel"], "dense") and ok["attempts"].min() >= 1
        named = [
            lambda: native.start_grid_log_weight(nm, grid),
            lambda: mdl.sample(N, T, seed=SEED, ctx=gpu_ctx, start_grid=grid),
            lambda: mdl.sample(N, T, seed=SEED, ctx=gpu_ctx, start_grid=grid, lazy=True),
            lambda: mdl.track(N, TT, initialSeed=TSEED, ctx=gpu_ctx, start_grid=grid),
            lambda: legacy.em_sample(path, str(tmp_path / "i.txt"), str(tmp_path / "t.txt"), num_initial_samples=N, num_transition_samples=T, ctx=gpu_ctx,
                                     start_grid=grid),
        ]
        for q, fn in enumerate(named):
            with pytest.raises(L.EmgpuError) as ei:
                fn()
            assert ei.value.code == L.ERR_PRESET and "row 397 " in str(ei.value), (q, str(ei.value))
    assert len(mdl.sample(N, T, seed=SEED, ctx=gpu_ctx, start_grid=good, lazy=True)) == 4
    # an index list stays refused by the device-formatted entry points, with or without a grid
    for fn in (lambda **kw: native.sample_uncor_host(gpu_ctx, nm, 4, T, SEED, _ctrl(pp), **kw), lambda **kw: native.sample_text_host(gpu_ctx, nm, 4, T, SEED, **kw)):
        with pytest.raises(L.EmgpuError) as ei:
            fn(indices=np.arange(4, dtype=np.uint64), start=good[:4])
        assert ei.value.code == L.ERR_ARG
