"""-m gpu: start grids on k_dbn_step2 -- the +start twins of the general instance of each shape (<7,3>, <9,3>, <16,4>, <16,4>[frozen]; dense and
list alone) against the oracle, against the library's own model-start path on the family instance and against k_dbn_generic (which still serves
the list and the dense trace together, and an index list); the chunked host paths, the class layer, em_sample and the track rounds.  Inputs and
the oracle's answers: step2_start_cases.py.

Trajectory i gets rows[i % 6]: every wave holds all six rows.  Bins, attempts, counts and rows are compared bit for bit, f32 values with the
oracle's f64 rounded to f32 (util.assert_uncor_parity); log-weights with start_log_weight within 1e-12 and bit for bit with the host function.
On a library without the twins every one of these grid calls reports k_dbn_generic<...>: the kernel-name assertions fail there."""
import filecmp

import numpy as np
import pytest

from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import legacy, native
from em_model_manned_bayes_amd import encounter_model as E
import step2_start_cases as S
from test_gpu_lazy_sample import assert_lazy_equals_eager
from test_gpu_start_grid import DENSE_FIELDS, _assert_same, _ctrl
from util import assert_uncor_parity, uncor_indices

pytestmark = pytest.mark.gpu

N, T, SEED, FIRST = S.N, S.T, S.SEED, S.FIRST
_both_cache = {}


def _mode(case):
    return L.TRANSITION_PER_STEP if S.per_step(case) else L.TRANSITION_REFERENCE_AUTO


def _call(ctx, nm, idx, case, form, n=N, log_weight=True, **kw):
    kw.setdefault("first_index", FIRST)
    return native.sample_dbn_host(ctx, nm, n, T, SEED, want_dense=form != "list", want_events=form != "dense", want_log_weight=log_weight,
                                  transition_mode=_mode(case), **dict(idx, **kw))


def _generic_both(ctx, nm, idx, case, grid):
    """the same grid through the list-plus-dense form, which stays on k_dbn_generic (one call per case, shared)"""
    if case not in _both_cache:
        _both_cache[case] = _call(ctx, nm, idx, case, "both", start=grid)
        assert _both_cache[case]["kernel"].startswith("k_dbn_generic"), _both_cache[case]["kernel"]
    return _both_cache[case]


def _device_call(ctx, nm, idx, case, form, grid):
    """emgpu_sample_dbn_device at column COL of arrays dimensioned LD: the tail lanes of the last workgroup have no trajectory and must read no
    row of the grid (which has exactly N rows) and write nothing."""
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
    p, _keep = native.make_params(N, T, SEED, first_index=FIRST, transition_mode=_mode(case), event_cap=cap if form == "list" else 0, start=g.data_ptr(), **idx)
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
@pytest.mark.parametrize("case", S.NAMES)
def test_start_grid_on_the_per_timestep_kernel(case, form, gpu_ctx, model_dir):
    nm, pp, _ = S.load(case, model_dir)
    idx = uncor_indices(pp)
    rows, grid, ref = S.rows_of(case, model_dir), S.grid_of(case, model_dir), S.oracle_of(case, model_dir)
    got = _call(gpu_ctx, nm, idx, case, form, start=grid)
    assert got["kernel"] == S.kernel_name(case, form), got["kernel"]
    assert_uncor_parity(got, ref, T)
    if form == "list":
        assert np.array_equal(got["ev_count"], [len(e) for e in ref["events"]])
    # the device-pointer call at a column offset: the same numbers, nothing outside its columns
    dev = _device_call(gpu_ctx, nm, idx, case, form, grid)
    assert dev["kernel"] == got["kernel"]
    _assert_same(dev, got, form, what="device call")
    assert np.array_equal(dev["log_weight"], got["log_weight"])
    # the library's own model-start path on the family instance: the model's start set to the row, all N trajectories from the same first
    # index (an index list would leave k_dbn_step2), rows k::6 compared
    try:
        for k, row in enumerate(rows):
            nm.set_start([int(v) or None for v in row])
            own = _call(gpu_ctx, nm, idx, case, form, log_weight=False)
            assert not own["kernel"].endswith("+start") and own["kernel"].startswith("k_dbn_step2<"), own["kernel"]
            sub = {f: (v[k::6] if isinstance(v, (np.ndarray, list)) else v) for f, v in own.items()}
            _assert_same(sub, got, form, rows=np.arange(k, N, 6), what="row %d" % k)
            # log-weights: the row's start_log_weight (the tolerance of test_host.py::test_start_log_weight)
            # (cor_v1's R4 has probability 0 under the model's counts: both are -inf, which no difference is taken of)
            lw, slw = got["log_weight"][k], nm.start_log_weight()
            assert np.all(got["log_weight"][k::6] == lw) and (lw == slw or abs(lw - slw) < 1e-12), (k, lw, slw)
    finally:
        nm.set_start([None] * nm.n_initial)
    assert np.all(got["log_weight"][1::6] == 0.0)                                           # the empty row
    assert np.array_equal(got["log_weight"], native.start_grid_log_weight(nm, grid))        # bit for bit
    # the list-plus-dense form of the same grid runs on k_dbn_generic: its arrays and lists equal the new form's
    both = _generic_both(gpu_ctx, nm, idx, case, grid)
    _assert_same(got, both, form, what="k_dbn_generic")
    assert np.array_equal(got["log_weight"], both["log_weight"])


def test_the_chunked_host_paths_read_their_own_rows(gpu_ctx, model_dir, tmp_path, monkeypatch):
    """2 500 trajectories in three chunks of 1 024 (1 024 is no multiple of 6: chunk k reads the grid from row 1 024 k on) against one chunk:
    sample_dbn_host and sample_text_host on cor_v1, sample_uncor_host on glider_v1; the text bytes are em_sample(text="host", start_grid=...)'s."""
    n = 2500
    cor, _, cor_path = S.load("cor_v1", model_dir)
    gl, gl_pp, _ = S.load("glider_v1", model_dir)
    cor_grid, gl_grid = S.grid_of("cor_v1", model_dir, n), S.grid_of("glider_v1", model_dir, n)
    calls = {
        "dbn": lambda: native.sample_dbn_host(gpu_ctx, cor, n, T, SEED, first_index=FIRST, want_dense=True, want_log_weight=True, start=cor_grid),
        "uncor": lambda: native.sample_uncor_host(gpu_ctx, gl, n, T, SEED, _ctrl(gl_pp), first_index=FIRST, start=gl_grid, **uncor_indices(gl_pp)),
        "text": lambda: native.sample_text_host(gpu_ctx, cor, n, T, SEED, max_attempts=1, start=cor_grid),   # em_sample's own call
    }
    fields = {"dbn": DENSE_FIELDS + ("log_weight",), "uncor": ("inits", "ev_count", "events", "ctrl_count", "controls", "samples", "attempts"),
              "text": ("initial", "transition", "init_val", "dyn_val")}
    want_kernel = {"dbn": S.kernel_name("cor_v1", "dense"), "uncor": S.kernel_name("glider_v1", "list"), "text": S.kernel_name("cor_v1", "dense")}
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
    # one chunk is right: the oracle on the first 700 (the same interleaving)
    sub = {f: res["dbn", 1][f][:N] for f in DENSE_FIELDS}
    assert_uncor_parity(sub, S.oracle_of("cor_v1", model_dir), T)
    assert np.array_equal(res["uncor", 1]["inits"][:N].astype(np.float32), S.oracle_of("glider_v1", model_dir)["init_val"].astype(np.float32))
    fi, ft = str(tmp_path / "i.txt"), str(tmp_path / "t.txt")
    legacy.em_sample(cor_path, fi, ft, num_initial_samples=n, num_transition_samples=T, rng_seed=SEED, ctx=gpu_ctx, start_grid=cor_grid)
    body = lambda f: open(f, "rb").read().split(b"\n", 1)[1]
    assert res["text", 3]["initial"].tobytes() == body(fi) and res["text", 3]["transition"].tobytes() == body(ft)


def test_the_class_layer_eager_lazy_and_per_row(gpu_ctx, model_dir):
    case = "glider_v1"
    _, _, path = S.load(case, model_dir)
    mdl = E.UncorEncounterModel(parameters_filename=path)
    rows, grid = S.rows_of(case, model_dir), S.grid_of(case, model_dir)
    eager = mdl.sample(N, T, seed=SEED, first_index=FIRST, ctx=gpu_ctx, start_grid=grid, return_log_weight=True)
    assert gpu_ctx.last_kernel() == S.kernel_name(case, "list")
    lazy = mdl.sample(N, T, seed=SEED, first_index=FIRST, ctx=gpu_ctx, start_grid=grid, return_log_weight=True, lazy=True)
    assert gpu_ctx.last_kernel() == S.kernel_name(case, "list")
    assert len(eager) == 5 and len(lazy) == 5
    assert_lazy_equals_eager(lazy[:4], eager[:4])
    assert np.array_equal(eager[4], lazy[4]) and np.array_equal(eager[4], native.start_grid_log_weight(mdl.native, grid))
    ref = S.oracle_of(case, model_dir)
    assert np.array_equal(eager[0].astype(np.float32), ref["init_val"].astype(np.float32))
    assert all(np.array_equal(e[:, :2], r[:, :2]) for e, r in zip(eager[1], ref["events"]))
    try:
        for k, row in enumerate(rows):                                     # rows i = k mod 6 are the model-level start's
            mdl.start = [int(v) or None for v in row]
            one = mdl.sample(N, T, seed=SEED, first_index=FIRST, ctx=gpu_ctx)
            assert gpu_ctx.last_kernel().startswith("k_dbn_step2<") and not gpu_ctx.last_kernel().endswith("+start")
            assert mdl.start_log_weight == eager[4][k] or abs(mdl.start_log_weight - eager[4][k]) < 1e-12
            assert np.array_equal(one[0][k::6], eager[0][k::6]), k
            for i in range(k, N, 6):
                assert np.array_equal(one[1][i], eager[1][i]) and np.array_equal(one[2][i], eager[2][i]) and np.array_equal(one[3][i].event, eager[3][i].event), i
    finally:
        mdl.preallocStart()


def test_em_sample_with_a_grid_writes_the_same_files_under_both_writers(gpu_ctx, model_dir, tmp_path):
    case = "cor_v1"
    _, _, path = S.load(case, model_dir)
    grid = S.grid_of(case, model_dir)
    names = [str(tmp_path / ("%s_%s.txt" % (w, f))) for w in ("host", "device") for f in ("initial", "transition")]
    host = legacy.em_sample(path, names[0], names[1], num_initial_samples=N, num_transition_samples=T, rng_seed=SEED, ctx=gpu_ctx, start_grid=grid)
    k_host = gpu_ctx.last_kernel()
    dev = legacy.em_sample(path, names[2], names[3], num_initial_samples=N, num_transition_samples=T, rng_seed=SEED, ctx=gpu_ctx, start_grid=grid,
                           text="device", text_batch=256)                # three batches: batch b reads the grid from row 256 b on
    assert k_host == gpu_ctx.last_kernel() and k_host.startswith("k_dbn_step2") and k_host.endswith("+start"), (k_host, gpu_ctx.last_kernel())
    assert k_host == S.kernel_name(case, "dense")
    assert filecmp.cmp(names[0], names[2], shallow=False) and filecmp.cmp(names[1], names[3], shallow=False)
    assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1])
    rows = S.rows_of(case, model_dir)
    for k in (0, 2, 3, 4, 5):                                              # the preset layer (a categorical variable: its value is its bin)
        assert np.all(host[0][k::6, 1] == rows[k][1]), k


# ------------------------------------------------------------------------------------------------ track
def test_track_round_0_runs_on_the_new_kernel(gpu_ctx, model_dir):
    """native.track_uncor_host(start=...) on uncor_1200code_v1, the four rows that can fly interleaved: attempts against the oracle's per row
    (every trajectory accepted within 8 rounds, TRACK_LATER of them in a later round, whose index lists run on k_dbn_generic), tracks and
    limits against the library's own per-row calls; a call cut after round 0 reports the new kernel."""
    nm, pp, _ = S.load(S.TRACK_CASE, model_dir)
    rows = S.track_rows(model_dir)
    nr = len(rows)
    grid = np.ascontiguousarray(rows[np.arange(S.TN) % nr])
    want, per_row = S.track_oracle(model_dir)
    got = native.track_uncor_host(gpu_ctx, nm, S.TN, S.TT, S.TSEED, start=grid, max_track_attempts=S.TRACK_ROUNDS)
    assert np.array_equal(got["attempts"], want)
    assert got["kernel"].split(" + ")[0].startswith("k_dbn_generic"), got["kernel"]                         # the last round: an index list
    with pytest.raises(L.EmgpuError) as ei:                                                                # round 0 alone
        native.track_uncor_host(gpu_ctx, nm, S.TN, S.TT, S.TSEED, start=grid, max_track_attempts=1)
    assert ei.value.code == L.ERR_REJECT_CAP and "%d trajectories" % S.TRACK_LATER in str(ei.value), str(ei.value)
    assert gpu_ctx.last_kernel().split(" + ")[0] == S.kernel_name(S.TRACK_CASE, "dense"), gpu_ctx.last_kernel()
    try:
        for k, row in enumerate(rows):
            nm.set_start([int(v) or None for v in row])
            one = native.track_uncor_host(gpu_ctx, nm, S.TN, S.TT, S.TSEED, max_track_attempts=S.TRACK_ROUNDS)
            assert not one["kernel"].split(" + ")[0].endswith("+start"), one["kernel"]
            assert np.array_equal(one["attempts"], per_row[k]), k
            assert np.array_equal(one["tracks"][k::nr], got["tracks"][k::nr]) and np.array_equal(one["limits"][k::nr], got["limits"][k::nr]), k
    finally:
        nm.set_start([None] * nm.n_initial)


# ------------------------------------------------------------------------------------------------ errors
def test_bad_rows_are_refused_by_the_new_kernel_and_an_index_list_stays_generic(gpu_ctx, model_dir):
    case = "cor_v1"
    nm, pp, _ = S.load(case, model_dir)
    idx, good = uncor_indices(pp), S.grid_of(case, model_dir)
    hmd_alone = [0] * 16
    hmd_alone[14] = 2                                                     # hmd (variable 15) without v_1, v_2 and vmd
    layer_6 = [0] * 16
    layer_6[1] = int(np.asarray(pp["r_initial"]).ravel()[1]) + 1         # bin r + 1 of L
    for bad_row in (hmd_alone, layer_6):
        grid = good.copy()
        grid[397] = bad_row
        for form in ("dense", "list"):
            with pytest.raises(L.EmgpuError) as ei:
                _call(gpu_ctx, nm, idx, case, form, start=grid)
            assert ei.value.code == L.ERR_PRESET, (form, str(ei.value))
            assert gpu_ctx.last_kernel() == S.kernel_name(case, form)     # raised at the sync behind the new kernel
            ok = _call(gpu_ctx, nm, idx, case, "dense", start=good)       # a valid call on the same ctx afterwards
            assert ok["kernel"] == S.kernel_name(case, "dense") and ok["attempts"].min() >= 1
    # an index list with a grid: not step2_eligible, k_dbn_generic as before, those rows of the full call
    full = _call(gpu_ctx, nm, idx, case, "dense", start=good)
    pick = np.random.RandomState(11).permutation(N)[:300]
    sub = _call(gpu_ctx, nm, idx, case, "dense", n=300, first_index=0, indices=(FIRST + pick).astype(np.uint64), start=np.ascontiguousarray(good[pick]))
    assert sub["kernel"].startswith("k_dbn_generic"), sub["kernel"]
    _assert_same(sub, full, "dense", rows=pick)
    assert np.array_equal(sub["log_weight"], full["log_weight"][pick])
