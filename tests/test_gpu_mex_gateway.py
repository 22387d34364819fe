"""-m gpu: every sampling command of the MATLAB gateway (em_model_manned_bayes_amd/matlab/emgpu_mex.c), run through the working mex
runtime (tests/mexrt.py) and checked twice: bit-equal to native.py's wrapper of the same entry point with the same arguments (the
gateway widens f32 to f64, which is exact), and against the CPU oracle by the rule the parity test of that entry point uses
(tests/test_gpu_parity.py) -- gateway and native.py share the library, so only the oracle sees a misconception both repeat.
Outputs are indexed as the .m files index them: initial(i, :), E(1:cnt(i), :, i), out(lane, second, field), tracks(:, :, i).
Inputs are chosen so that a transposed or mis-strided read cannot pass by symmetry (asymmetric bounds, different limits for the two
aircraft, n off every block size, first indices above 2^32)."""
import os
import time

import numpy as np
import pytest

import em_model_manned_bayes_amd as E
import mexrt
import oracle as O
import util
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native
from util import assert_f32_of_f64, assert_parting_only_on_a_threshold, assert_uncor_parity, label_index, uncor_indices

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIRST = 2**35 + 7
T0 = time.perf_counter()


@pytest.fixture(scope="module")
def gw(tmp_path_factory):
    g = mexrt.build(tmp_path_factory.mktemp("mex"))
    yield g
    assert g.run_at_exit()                 # the gateway registered its shutdown with mexAtExit; this frees its contexts
    g.check("module teardown")
    print("\ngateway module: %.1f s" % (time.perf_counter() - T0))


@pytest.fixture(scope="module")
def terminal_dir(tmp_path_factory):
    from em_model_manned_bayes_amd import synthetic
    return synthetic.write_terminal_directory(str(tmp_path_factory.mktemp("terminal")))


class Loaded:
    """A model on all three sides: gateway handle, native model, oracle parms, from the same .txt file."""

    def __init__(self, gw, path, **read_kw):
        self.gw, self.path = gw, path
        idx, over = read_kw.get("idx", (1, 2, 3)), read_kw.get("overwrite", False)
        self.h = gw.call("load_txt", path, np.array(idx, dtype=np.float64), bool(over))
        self.nm = native.NativeModel.load_txt(path, idx, over)
        self.pp = O.parse_model_txt(path, idx, over)
        self.ni = self.pp["n_initial"]

    def free(self):
        self.gw.call("free", self.h, nlhs=0)


@pytest.fixture
def loaded(gw, model_dir):
    made = []

    def make(name, **kw):
        path = name if os.path.sep in name else em_io.materialize_model(name, model_dir)
        made.append(Loaded(gw, path, **kw))
        return made[-1]
    yield make
    for m in made:
        m.free()


def event_rows(E_, cnt, i):
    """E(1:ev_count(i), :, i): rows [dt var value], as UncorEncounterModelGPU.m reads them."""
    return E_[: int(cnt[i, 0]), :, i]


def check_uncor_outputs(init, cnt, E_, got, ref, n, ni, cap, value_col=2):
    """Gateway outputs against native.sample_dbn_host's dict (bit-equal) and the oracle's dict (assert_uncor_parity's rule on the
    fields the gateway returns: counts, dt and var exact, values equal to the oracle's f64 rounded to f32).
    value_col: column of the oracle's event rows that holds the value (2; the bin, 3, for a call without dediscretize)."""
    assert init.shape == (n, ni) and init.dtype == np.float64 and cnt.shape == (n, 1) and E_.shape == (cap, 3, n)
    assert np.array_equal(init, got["init_val"].astype(np.float64))
    assert np.array_equal(init.astype(np.float32), ref["init_val"].astype(np.float32)), "initial values differ from the oracle's"
    assert np.array_equal(cnt[:, 0], got["ev_count"])
    for i in range(n):
        rows, g, r = event_rows(E_, cnt, i), got["events"][i], ref["events"][i]
        assert rows.shape[0] == len(g) == r.shape[0], "trajectory %d: %d / %d / %d event rows" % (i, rows.shape[0], len(g), r.shape[0])
        assert np.array_equal(rows[:, 0], g["dt"]) and np.array_equal(rows[:, 1], g["var"]) and np.array_equal(rows[:, 2], g["value"].astype(np.float64)), i
        assert np.array_equal(rows[:, 0], r[:, 0]) and np.array_equal(rows[:, 1], r[:, 1]), "trajectory %d: dt / var differ from the oracle's" % i
        assert np.array_equal(rows[:, 2].astype(np.float32), r[:, value_col].astype(np.float32)), "trajectory %d: values differ from the oracle's" % i
        assert not E_[rows.shape[0]:, :, i].any()                      # rows beyond ev_count stay zero


# ---------------------------------------------------------------------------------------------------------------------------------

def test_device_count(gw):
    import torch
    c = gw.call("device_count")
    assert c.shape == (1, 1) and c[0, 0] == torch.cuda.device_count() >= 1


@pytest.mark.parametrize("name", ["uncor_1200code_v2p1", "terminal_v3_radar_encounter_model"])
def test_bn_sample(gw, loaded, gpu_ctx, name):
    m = loaded(name)
    om = O.OracleModel(m.pp)
    for n, seed, first in ((1, 2024, FIRST), (255, 2024, FIRST), (257, 2024, FIRST), (5, 2**53 - 1, 2**53 - 6)):   # the largest exact doubles
        S = gw.call("bn_sample", m.h, float(n), float(seed), float(first))
        assert S.shape == (n, m.ni) and S.dtype == np.float64                                # num_samples x n bins (bn_sample.m:39)
        ob, _, _ = native.sample_bn_host(gpu_ctx, m.nm, n, seed, first_index=first, dediscretize=False, max_attempts=1)
        rb, _, _ = O.geom_sample(om, n, seed, first_index=first, max_attempts=1)
        assert np.array_equal(S, ob) and np.array_equal(S, rb), (name, n)
        assert S.min() >= 1 and np.all(S.max(axis=0) <= m.pp["r_initial"])


@pytest.mark.parametrize("name", ["uncor_1200code_v2p1", "uncor_1200only_fwse_v1p2", "cor_v1"])
def test_sample_uncor_hierarchical_with_the_minimum_of_arguments(gw, loaded, gpu_ctx, name):
    """idxL / idxV / idxDH from the labels as UncorEncounterModelGPU.m finds them; no layers, no event_cap: the defaults (512 rows, 1000
    attempts of the rejection test) are then in force."""
    m = loaded(name)
    n, T, seed = 300, 61, 0x5EED0002
    idx = uncor_indices(m.pp)
    init, cnt, E_ = gw.call("sample_uncor", m.h, float(n), float(T), float(seed), float(FIRST), 0.0,
                            float(idx["idx_L"]), float(idx["idx_v"]), float(idx["idx_dh"]), nlhs=3)
    got = native.sample_dbn_host(gpu_ctx, m.nm, n, T, seed, first_index=FIRST, want_dense=False, want_events=True, event_cap=512, pinned=False, **idx)
    ref = O.uncor_sample(O.OracleModel(m.pp), n, T, seed, first_index=FIRST, want_dense=False, max_attempts=1000)
    assert_uncor_parity(got, ref, T)
    check_uncor_outputs(init, cnt, E_, got, ref, n, m.ni, 512)
    assert cnt.max() > 5
    # fewer outputs: only what was asked for is written (the runtime reports a slot written beyond nlhs)
    only = gw.call("sample_uncor", m.h, float(n), float(T), float(seed), float(FIRST), 0.0, float(idx["idx_L"]), float(idx["idx_v"]), float(idx["idx_dh"]))
    assert np.array_equal(only, init)
    two = gw.call("sample_uncor", m.h, float(n), float(T), float(seed), float(FIRST), 0.0, float(idx["idx_L"]), float(idx["idx_v"]), float(idx["idx_dh"]), nlhs=2)
    assert np.array_equal(two[0], init) and np.array_equal(two[1], cnt)


def test_sample_uncor_quantize_plain_dbn_and_layers(gw, loaded, gpu_ctx, tmp_path):
    n, T, seed = 257, 40, 77
    # isQuantize500
    m = loaded("uncor_1200code_v2p1")
    idx = uncor_indices(m.pp)
    args = [float(idx["idx_L"]), float(idx["idx_v"]), float(idx["idx_dh"])]
    init, cnt, E_ = gw.call("sample_uncor", m.h, float(n), float(T), float(seed), float(FIRST), float(L.FLAG_QUANTIZE500), *args, np.zeros((0, 0)), 300.0, nlhs=3)
    got = native.sample_dbn_host(gpu_ctx, m.nm, n, T, seed, first_index=FIRST, want_dense=False, want_events=True, event_cap=300, flags=L.FLAG_QUANTIZE500, pinned=False, **idx)
    ref = O.uncor_sample(O.OracleModel(m.pp), n, T, seed, first_index=FIRST, want_dense=False, is_quantize500=True)
    assert_uncor_parity(got, ref, T)
    check_uncor_outputs(init, cnt, E_, got, ref, n, m.ni, 300)
    level = init[:, idx["idx_dh"] - 1] == 0
    assert level.any() and np.all(init[level, idx["idx_L"] - 1] % 500 == 0)
    # dbn_sample.m itself, as shadow/emgpu_dbn_call.m asks for it: no resampling, no dediscretize, no terminator row, indices 0
    flags = L.FLAG_NO_RESAMPLE | L.FLAG_NO_DEDISC | L.FLAG_NO_TERMINATOR
    init, cnt, E_ = gw.call("sample_uncor", m.h, float(n), float(T), float(seed), float(FIRST), float(flags), 0.0, 0.0, 0.0, np.zeros((0, 0)), 256.0, nlhs=3)
    got = native.sample_dbn_host(gpu_ctx, m.nm, n, T, seed, first_index=FIRST, want_dense=False, want_events=True, event_cap=256, flags=flags, pinned=False)
    rb, rev = O.dbn_sample(O.OracleModel(m.pp), n, T, seed, first_index=FIRST)
    assert np.array_equal(got["init_bin"], rb)
    ref = {"init_val": rb.astype(np.float64), "events": [np.column_stack([e, e[:, 2]]) if len(e) else np.zeros((0, 4)) for e in rev]}
    check_uncor_outputs(init, cnt, E_, got, ref, n, m.ni, 256, value_col=3)          # rows (dt, variable, new bin): dbn_sample.m:84-91
    assert np.array_equal(init, rb) and cnt.max() > 2
    # layers of THREE rows with unequal bounds: L is a three-bin variable that stays a bin index (a prescribed small model)
    spec = None
    for s in range(40):
        cand = util.shaped_model(np.random.RandomState(s), 5, meff=(2, 2), r=[3, 4, 3, 3, 3])
        free = [v for v in range(2, 5) if len(cand["boundaries"][v]) == 0]
        if free:
            spec, idx_L = cand, free[0] + 1
            break
    assert spec is not None
    spec["N_initial"][idx_L - 1] = np.tile([[300.0], [500.0], [700.0]], (1, spec["N_initial"][idx_L - 1].shape[1]))   # every layer is drawn
    path = str(tmp_path / "three_layers.txt")
    em_io.em_write(spec, path)
    m3 = loaded(path, idx=(idx_L,), overwrite=False)
    layers = np.array([[50.0, 500.0], [500.0, 1200.0], [1200.0, 5000.0]])
    init, cnt, E_ = gw.call("sample_uncor", m3.h, float(n), float(T), float(seed), float(FIRST), 0.0, float(idx_L), 0.0, 0.0, layers, 256.0, nlhs=3)
    got = native.sample_dbn_host(gpu_ctx, m3.nm, n, T, seed, first_index=FIRST, want_dense=False, want_events=True, event_cap=256, layers=layers, idx_L=idx_L, pinned=False)
    om = O.OracleModel(m3.pp)
    om.label_index = lambda name: idx_L if name == "L" else 0
    ref = O.uncor_sample(om, n, T, seed, first_index=FIRST, want_dense=False, layers=layers)
    assert_uncor_parity(got, ref, T)
    check_uncor_outputs(init, cnt, E_, got, ref, n, m3.ni, 256)
    alt = init[:, idx_L - 1]
    assert alt.min() >= 50 and alt.max() <= 5000 and (alt > 1200).any() and ((alt > 500) & (alt < 1200)).any() and (alt < 500).any()
    with pytest.raises(mexrt.MexError) as ei:                                            # two rows for three bins: the library's check
        gw.call("sample_uncor", m3.h, float(n), float(T), float(seed), float(FIRST), 0.0, float(idx_L), 0.0, 0.0, layers[:2], 256.0, nlhs=3)
    assert ei.value.identifier == "emgpu:arg"


def test_event_cap_identifier_and_the_doubling_loop_of_the_m_classes(gw, loaded, gpu_ctx):
    m = loaded("uncor_1200code_v2p1")
    n, T, seed = 130, 120, 5
    idx = uncor_indices(m.pp)
    args = [m.h, float(n), float(T), float(seed), float(FIRST), 0.0, float(idx["idx_L"]), float(idx["idx_v"]), float(idx["idx_dh"]), np.zeros((0, 0))]
    ref = O.uncor_sample(O.OracleModel(m.pp), n, T, seed, first_index=FIRST, want_dense=False)
    longest = max(len(e) for e in ref["events"])
    assert longest > 16
    with pytest.raises(mexrt.MexError) as ei:
        gw.call("sample_uncor", *args, 8.0, nlhs=3)
    assert ei.value.identifier == "emgpu:eventcap"
    cap, tries = 8, 0                                       # UncorEncounterModelGPU.m:38-46: catch emgpu:eventcap, double, retry
    while True:
        try:
            init, cnt, E_ = gw.call("sample_uncor", *args, float(cap), nlhs=3)
            break
        except mexrt.MexError as e:
            assert e.identifier == "emgpu:eventcap" and cap < longest
            cap, tries = 2 * cap, tries + 1
    assert tries >= 2 and cap >= longest > cap // 2
    big = gw.call("sample_uncor", *args, 4096.0, nlhs=3)
    assert np.array_equal(init, big[0]) and np.array_equal(cnt, big[1]) and np.array_equal(E_, big[2][:cap])
    got = native.sample_dbn_host(gpu_ctx, m.nm, n, T, seed, first_index=FIRST, want_dense=False, want_events=True, event_cap=cap, pinned=False, **idx)
    check_uncor_outputs(init, cnt, E_, got, ref, n, m.ni, cap)


def test_use_devices_with_two_entries_equals_one_context(gw, loaded):
    if gw.call("device_count")[0, 0] < 2:
        pytest.skip("one device visible: emgpu_sample_dbn_multi_host over two devices needs device_count >= 2")
    m = loaded("uncor_1200code_v2p1")
    idx = uncor_indices(m.pp)
    args = [m.h, 700.0, 61.0, 9.0, float(FIRST), 0.0, float(idx["idx_L"]), float(idx["idx_v"]), float(idx["idx_dh"])]
    one = gw.call("sample_uncor", *args, nlhs=3)
    gw.call("use_devices", np.array([0.0, 1.0]), nlhs=0)
    try:
        two = gw.call("sample_uncor", *args, nlhs=3)
    finally:
        gw.call("use_devices", np.array([0.0]), nlhs=0)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)


def test_use_devices_with_one_entry_and_shutdown_recreate_the_context(gw, loaded):
    m = loaded("terminal_v3_radar_encounter_model")
    want = gw.call("bn_sample", m.h, 257.0, 3.0, float(FIRST))
    gw.call("use_devices", np.array([0.0]), nlhs=0)
    assert np.array_equal(gw.call("bn_sample", m.h, 257.0, 3.0, float(FIRST)), want)
    assert gw.call("shutdown", nlhs=0) is None
    assert np.array_equal(gw.call("bn_sample", m.h, 257.0, 3.0, float(FIRST)), want)      # a new context, the same answer
    gw.call("shutdown", nlhs=0)
    gw.call("shutdown", nlhs=0)                                                            # twice is harmless
    with pytest.raises(mexrt.MexError) as ei:
        gw.call("use_devices", np.array([99.0]), nlhs=0)
    assert ei.value.identifier in ("emgpu:nodevice", "emgpu:arg")
    assert np.array_equal(gw.call("bn_sample", m.h, 257.0, 3.0, float(FIRST)), want)      # and after the failed use_devices


def start_log_weight(pp, row):
    """log P(preset values) from the counts (bn_sample.m:44-50 presets, select_random's N / sum(N)): sum over the preset variables of
    log(N(bin, column of the parents' bins) / sum(N(:, column))), asub2ind's first parent fastest."""
    G, r = np.asarray(pp["G_initial"]), np.asarray(pp["r_initial"])
    lw = 0.0
    for v, b in enumerate(row):
        if not b:
            continue
        col, stride = 0, 1
        for p in np.flatnonzero(G[:, v]):
            col += (row[p] - 1) * stride
            stride *= int(r[p])
        N = pp["N_initial"][v]
        lw += np.log(N[b - 1, col] / N[:, col].sum())
    return lw


@pytest.mark.parametrize("name", ["terminal_v3_radar_encounter_model", "terminal_v3_opensky_encounter_model"])
def test_geom_sample(gw, loaded, gpu_ctx, name):
    m = loaded(name)
    om = O.OracleModel(m.pp)
    labs, ni = m.pp["labels_initial"], m.ni
    io, ii = label_index(labs, "own_speed"), label_index(labs, "int_speed")
    assert io and ii and io != ii
    n, seed = 257, 2024
    bs = np.column_stack([-np.inf * np.ones(ni), np.inf * np.ones(ni)])
    bs[label_index(labs, "own_distance") - 1] = [0.5, 3.0]                 # an asymmetric box: a transposed read puts -inf where 3.0 belongs
    bs[label_index(labs, "int_distance") - 1] = [-np.inf, 4.0]
    lim1, lim2 = (169.0, 491.0), (68.0, 186.0)                             # RTCA228_A1 / RTCA228_A3: the two aircraft differ
    full = [m.h, float(n), float(seed), float(FIRST), bs, float(io), float(ii), np.array(lim1), np.array(lim2)]
    out, att = gw.call("geom_sample", *full, nlhs=2)
    nb, nv, na = native.sample_bn_host(gpu_ctx, m.nm, n, seed, first_index=FIRST, dediscretize=True, bounds_sample=bs, idx_own_speed=io, idx_int_speed=ii, lim1=lim1, lim2=lim2)
    rb, rv, ra = O.geom_sample(om, n, seed, first_index=FIRST, bounds_sample=bs, idx_own_speed=io, idx_int_speed=ii, lim1=lim1, lim2=lim2)
    assert out.shape == (n, ni) and att.shape == (n, 1)
    assert np.array_equal(out, nv.astype(np.float64)) and np.array_equal(att[:, 0], na)
    assert np.array_equal(out.astype(np.float32), rv.astype(np.float32)) and np.array_equal(att[:, 0], ra)
    assert ra.max() > 1                                                     # the rejection loop ran
    assert out[:, io - 1].min() >= 169 and out[:, io - 1].max() > 186 and out[:, ii - 1].max() <= 186
    d = out[:, label_index(labs, "own_distance") - 1]
    assert d.min() >= 0.5 and d.max() <= 3.0 and out[:, label_index(labs, "int_distance") - 1].max() <= 4.0
    assert np.array_equal(gw.call("geom_sample", *full), out)              # nlhs = 1
    # the minimum of arguments: no box, no speed test (limits 0 .. inf), 100000 attempts
    out0, att0 = gw.call("geom_sample", m.h, float(n), float(seed), float(FIRST), nlhs=2)
    _, rv0, ra0 = O.geom_sample(om, n, seed, first_index=FIRST)
    assert np.array_equal(out0.astype(np.float32), rv0.astype(np.float32)) and np.array_equal(att0[:, 0], ra0) and ra0.max() == 1
    # a start grid: the 18 InitStartTerminal rows tiled to n, unset cells as NaN and as 0; log-weights with nlhs = 3
    rows = E.CorTerminalModel(srcData="opensky" if "opensky" in name else "terminalradar").InitStartTerminal(nSamples=18)
    assert len(rows) == 18 and len({tuple(r_[:3]) for r_ in rows}) == 18
    per = 10
    n = 18 * per
    grid_rows = [rows[i // per] for i in range(n)]
    grid = np.array([[float(v) if v else (np.nan if (i + j) % 2 else 0.0) for j, v in enumerate(r_)] for i, r_ in enumerate(grid_rows)])
    assert np.isnan(grid).any() and (grid == 0).any() and grid.shape == (n, ni)
    lim = (50.0, 506.0)
    out, att, lw = gw.call("geom_sample", m.h, float(n), float(seed), float(FIRST), np.zeros((0, 0)), float(io), float(ii), np.array(lim), np.array(lim), grid, nlhs=3)
    st = np.array([[int(v or 0) for v in r_] for r_ in grid_rows], dtype=np.int32)
    _, nv, na, nlw = native.sample_bn_host(gpu_ctx, m.nm, n, seed, first_index=FIRST, dediscretize=True, idx_own_speed=io, idx_int_speed=ii, lim1=lim, lim2=lim,
                                           start=st, want_log_weight=True)
    assert out.shape == (n, ni) and att.shape == (n, 1) and lw.shape == (n, 1)
    assert np.array_equal(out, nv.astype(np.float64)) and np.array_equal(att[:, 0], na) and np.array_equal(lw[:, 0], nlw)
    for k in range(18):
        sl = slice(k * per, (k + 1) * per)
        row = [int(v or 0) for v in rows[k]]
        assert np.all(out[sl, :3] == np.array(row[:3], dtype=float))
        _, ov, oa = O.geom_sample(O.OracleModel(m.pp, start=row), per, seed, first_index=FIRST + k * per, idx_own_speed=io, idx_int_speed=ii, lim1=lim, lim2=lim)
        assert np.array_equal(out[sl].astype(np.float32), ov.astype(np.float32)) and np.array_equal(att[sl, 0], oa), "row %d of the grid" % k
        want = start_log_weight(m.pp, row)
        assert np.all(np.abs(lw[sl, 0] - want) < 1e-12) and np.isfinite(want) and want < 0, k        # the tolerance of tests/test_host.py::test_start_log_weight
    assert len(set(np.round(lw[:, 0], 9))) > 6                                 # the rows weigh differently: a mis-strided grid cannot pass


def gateway_trajectory_models(gw, t):
    """The 10 trajectory models as CorTerminalModelGPU.nativeModels makes them: loaded, then the stay prior of
    setTransitionPriors(..., 1) (createEncounter.m:128-129) passed through set_alpha.  Returns (1 x 10 uint64, oracle models)."""
    hs, oms = [], []
    for k, mdl in enumerate(t._traj):
        pp = O.parse_model_txt(mdl.parameters_filename)
        alpha = O.stay_prior_alpha(pp, 1.0)
        oms.append(O.OracleModel(pp, alpha_transition=alpha))
        h = gw.call("load_txt", mdl.parameters_filename)
        gw.call("set_alpha", h, [], [np.asfortranarray(alpha[v]) if v in alpha else None for v in range(pp["n_transition"])], nlhs=0)
        for v in alpha:
            assert np.array_equal(native.NativeModel.get_f64(_Borrowed(mexrt.handle(h)), L.F_ALPHA_TRANSITION, v + 1), mdl.native.get_f64(L.F_ALPHA_TRANSITION, v + 1))
        hs.append(mexrt.handle(h))
    return np.array([hs], dtype=np.uint64), oms


class _Borrowed(native.NativeModel):
    def __del__(self):
        pass


def free_all(gw, handles):
    for h in handles.reshape(-1):
        gw.call("free", np.array([[h]], dtype=np.uint64), nlhs=0)


def test_propagate_terminal(gw, terminal_dir, gpu_ctx):
    t = E.CorTerminalModel(srcData="terminalradar", parameters_directory=terminal_dir)
    t.acType1, t.acType2 = "RTCA228_A1", "RTCA228_A2"
    dl = t._dyn_rows()
    assert not np.array_equal(dl[0], dl[1])                                # the two columns of dyn_limits differ
    handles, oms = gateway_trajectory_models(gw, t)
    seed, cap = 0x5EED0005, 123
    try:
        for n in (1, 150):
            _, samples = t.sample(n, seed=seed, ctx=gpu_ctx)
            geo, mo = t._geo_rows(samples)
            out, rows = gw.call("propagate_terminal", handles, np.asfortranarray(geo.T), mo.T.astype(np.float64), float(seed), float(FIRST), 120.0, dl.T.copy(), nlhs=2)
            assert out.shape == (4 * n, cap, 6) and rows.shape == (4 * n, 1) and out.dtype == np.float64
            nat, nrows = native.propagate_terminal_host(gpu_ctx, [m.native for m in t._traj], geo, mo, seed, first_index=FIRST, tmax_s=120.0, dyn_limits=dl)
            assert np.array_equal(rows[:, 0], nrows) and np.array_equal(out, nat.astype(np.float64))
            ref, ref_rows = O.propagate(oms, mo, geo, seed, dl, first_index=FIRST, tmax_s=120.0)
            assert np.array_equal(rows[:, 0], ref_rows)                    # exact
            assert rows.min() >= 1 and rows.max() <= 122
            for lane in range(4 * n):
                r = int(rows[lane, 0])
                assert_f32_of_f64(out[lane, :r], ref[lane, :r], "lane %d" % lane)   # the rule of test_terminal_propagation_matches_oracle
                sign = -1.0 if lane & 1 else 1.0                            # lane 4e + 2a + backward: t_s = 0, +-1, +-2 ...
                assert np.array_equal(out[lane, :r, 0], sign * np.arange(r)) and np.array_equal(out[lane, :r, 0], ref[lane, :r, 0])
                assert not out[lane, r:].any()                              # zeros beyond rows
            if n > 1:
                assert (rows[1::2, 0] > 2).any() and (rows[0::2, 0] > 2).any()
                back, fwd = out[1::2, 1, 1:3], out[0::2, 1, 1:3]          # second 1 backward and forward are different places
                assert not np.array_equal(back, fwd)
            assert np.array_equal(gw.call("propagate_terminal", handles, np.asfortranarray(geo.T), mo.T.astype(np.float64), float(seed), float(FIRST), 120.0, dl.T.copy()), out)
    finally:
        free_all(gw, handles)


@pytest.mark.parametrize("name,rot", [("uncor_1200code_v2p1", False), ("uncor_1200only_rotorcraft_v1p2", True)])
def test_track_uncor(gw, loaded, gpu_ctx, name, rot):
    m = loaded(name)
    labs = m.pp["labels_initial"]
    idx7 = np.array([label_index(labs, s) for s in ("G", "A", "L", "v", "\\dot v", "\\dot h", "\\dot \\psi")], dtype=np.float64)
    assert (idx7 > 0).all() and len(set(idx7)) == 7
    n, T, seed, first = 300, 45, 0xF1, 77
    ref = O.uncor_track(O.OracleModel(m.pp), n, T, seed, first_index=first, is_rotorcraft=rot)
    assert (ref["attempts"] > 1).sum() > 3, "the case must exercise the retry rounds"
    for stride in (1, 10):
        extra = [] if stride == 1 else [float(stride), 200.0]               # stride 1: the minimum of arguments (stride 1, 200 attempts)
        tracks, limits, att = gw.call("track_uncor", m.h, float(n), float(T), float(seed), float(first), 0.0, float(rot), idx7, *extra, nlhs=3)
        S = 10 * T // stride + 1
        assert tracks.shape == (8, S, n) and limits.shape == (3, n) and att.shape == (n, 1)
        got = native.track_uncor_host(gpu_ctx, m.nm, n, T, seed, first_index=first, is_rotorcraft=rot, record_stride=stride)
        assert np.array_equal(tracks, got["tracks"].transpose(2, 1, 0)) and np.array_equal(limits, got["limits"].T) and np.array_equal(att[:, 0], got["attempts"])
        # the rule of test_uncor_track_matches_oracle
        same = assert_parting_only_on_a_threshold(att[:, 0], ref["attempts"], ref["margins"], 1e-9, "trajectory")
        assert same.sum() >= n - 3
        assert np.array_equal(limits[:, same].T, ref["limits"][same])
        for i in np.flatnonzero(same):
            np.testing.assert_allclose(tracks[:, :, i].T, ref["tracks"][i, ::stride], rtol=1e-9, atol=1e-6)
            assert np.array_equal(tracks[:5, 0, i], ref["tracks"][i, 0, :5])          # time 0 = the sampled initial state, bit-exact
        assert np.array_equal(tracks[0, :, 0], np.arange(S) * 0.1 * stride) or np.allclose(tracks[0, :, 0], np.arange(S) * 0.1 * stride, rtol=0, atol=1e-9)
    one = gw.call("track_uncor", m.h, float(n), float(T), float(seed), float(first), 0.0, float(rot), idx7)        # nlhs = 1
    assert one.shape == (8, 10 * T + 1, n)
    with pytest.raises(mexrt.MexError) as ei:
        gw.call("track_uncor", m.h, float(n), float(T), float(seed), float(first), 0.0, float(rot), idx7, 1.0, 1.0, nlhs=3)
    assert ei.value.identifier == "emgpu:rejectcap"


def test_track_terminal(gw, loaded, terminal_dir, gpu_ctx):
    """GENERIC / GENERIC at the n and cap of test_terminal_track_matches_oracle, by its rule.  The gateway passes no
    EMGPU_FLAG_LOCAL_SMOOTH, so both references run without the smoothing stand-in."""
    t = E.CorTerminalModel(srcData="terminalradar", parameters_directory=terminal_dir)
    t.acType1 = t.acType2 = "GENERIC"
    g = loaded(t.parameters_filename)
    gom = O.OracleModel(g.pp)
    handles, oms = gateway_trajectory_models(gw, t)
    labels = [s.strip('"') for s in g.pp["labels_initial"]]
    idx12 = np.array([labels.index(pre + "_" + f) + 1 for pre in ("own", "int") for f in native.TERMINAL_GEO_FIELDS], dtype=np.float64)
    d = (t.dynLimits1, t.dynLimits2)
    cum, pitch = [x["maxCumTurn_deg"] for x in d], [x["pitch_deg"] for x in d]
    dl = t._dyn_rows()
    thresholds = np.array([30.0, 2.5 * 6076, 750.0, 300.0 / 60.0])
    seed, first, ni, cap2 = 0xF2, 5, g.ni, 2 * 123
    try:
        for n, cap in ((300, 30), (2000, 150)):                          # the small cap first: it also ends soonest when the limits are wrong
            ref = O.terminal_track(gom, oms, n, seed, dl, cum, pitch, first_index=first, max_track_attempts=cap, local_smooth=False)
            sample, traj, ln, meta, att = gw.call("track_terminal", g.h, handles, float(n), float(seed), float(first), dl.T.copy(), np.array(cum + pitch, dtype=np.float64),
                                                  thresholds, idx12, np.zeros((0, 0)), float(cap), nlhs=5)      # returns at the cap: no error
            assert sample.shape == (ni, n) and traj.shape == (6, cap2, 2, n) and ln.shape == (2, n) and meta.shape == (4, n) and att.shape == (n, 1)
            got = native.track_terminal_host(gpu_ctx, t.native, [m.native for m in t._traj], n, seed, dl, cum, pitch, first_index=first, max_track_attempts=cap,
                                             allow_cap=True, local_smooth=False)
            # bit-equal for every accepted encounter; for a rejected one the library copies back whatever its device buffers held before
            # the call (native.py hands that out as it is), and the gateway returns zeros
            acc = got["attempts"] > 0
            assert np.array_equal(att[:, 0], got["attempts"]) and acc.sum() > 20 and (~acc).sum() > 20
            assert np.array_equal(sample[:, acc], got["sample"][acc].T) and np.array_equal(traj[:, :, :, acc], got["traj"][acc].transpose(3, 2, 1, 0))
            assert np.array_equal(ln[:, acc], got["len"][acc].T) and np.array_equal(meta[:, acc], got["meta"][acc].T)
            assert not sample[:, ~acc].any() and not traj[:, :, :, ~acc].any() and not ln[:, ~acc].any() and not meta[:, ~acc].any()
            same = assert_parting_only_on_a_threshold(att[:, 0], ref["attempts"], ref["margins"], 2.0 ** -22, "encounter")
            assert same.sum() >= n - max(2, n // 500)
            assert (ref["attempts"] < 0).sum() > 20 and (ref["attempts"] > 0).sum() > 20
            if cap == 30:                                                    # a cap too small for most encounters
                assert np.array_equal(att[:, 0] == -1, ref["attempts"] < 0)   # exactly the encounters the oracle leaves rejected
            ok = same & (ref["attempts"] > 0)
            assert ok.sum() >= (n // 5 if cap == 150 else 20)
            assert np.array_equal(sample[:, ok].T, ref["sample"][ok]) and np.array_equal(ln[:, ok].T, ref["len"][ok])
            np.testing.assert_allclose(meta[:, ok].T, ref["meta"][ok], rtol=1e-5, atol=1e-3)
            for i in np.flatnonzero(ok)[:400]:
                for a in range(2):
                    k = ref["len"][i, a]
                    assert_f32_of_f64(traj[1:, :k, a, i].T, ref["traj"][i, a, :k, 1:], "encounter %d aircraft %d" % (i, a))
                    assert np.array_equal(traj[0, :k, a, i], ref["traj"][i, a, :k, 0]) and np.all(np.diff(traj[0, :k, a, i]) == 1)
        # the minimum of arguments: no box, 2000 attempts (and tmax_s = 120: cap2 = 246 rows)
        n = 40
        sample, traj, ln, meta, att = gw.call("track_terminal", g.h, handles, float(n), float(seed), float(first), dl.T.copy(), np.array(cum + pitch, dtype=np.float64),
                                              thresholds, idx12, nlhs=5)
        ref = O.terminal_track(gom, oms, n, seed, dl, cum, pitch, first_index=first, max_track_attempts=2000, local_smooth=False)
        same = assert_parting_only_on_a_threshold(att[:, 0], ref["attempts"], ref["margins"], 2.0 ** -22, "encounter")
        assert same.sum() >= n - 2 and traj.shape == (6, cap2, 2, n)
        assert np.array_equal(sample[:, same].T, ref["sample"][same]) and np.array_equal(ln[:, same].T, ref["len"][same])
        assert np.array_equal(gw.call("track_terminal", g.h, handles, float(n), float(seed), float(first), dl.T.copy(), np.array(cum + pitch, dtype=np.float64),
                                      thresholds, idx12), sample)            # nlhs = 1
    finally:
        free_all(gw, handles)


def test_sample2track(gw, gpu_ctx):
    g = np.load(os.path.join(GOLD, "sample2track_48x40.npz"))
    n, T = g["updates"].shape[:2]
    assert (n, T) == (48, 40)
    ur, lo, hi = g["ur"].astype(np.float64), float(g["min_speed"][0]), float(g["max_speed"][0])
    upd = np.asfortranarray(g["updates"].transpose(2, 1, 0))               # 3 x T x n
    xyz, flags, vmm = gw.call("sample2track", g["alt0"].astype(np.float64), g["speed0"].astype(np.float64), upd, ur, lo, hi, nlhs=3)
    assert xyz.shape == (3, T + 1, n) and flags.shape == (n, 1) and flags.dtype == np.uint8 and vmm.shape == (2, n)
    nx, nf, nv = native.sample2track_host(gpu_ctx, g["alt0"], g["speed0"], g["updates"], *ur, lo, hi)
    assert np.array_equal(xyz, nx.transpose(2, 1, 0)) and np.array_equal(flags[:, 0], nf) and np.array_equal(vmm, nv.T)
    rx, rf, rv = O.sample2track(g["alt0"], g["speed0"], g["updates"], *ur, lo, hi)
    for want_xyz, want_f, want_v in ((g["xyz"], g["flags"], g["speed_minmax"]), (rx, rf, rv)):      # the golden file and the oracle, by the existing tests' rule
        assert np.array_equal(flags[:, 0], want_f)
        np.testing.assert_allclose(xyz.transpose(2, 1, 0), want_xyz, rtol=1e-12, atol=1e-7)
        np.testing.assert_allclose(vmm.T, want_v, rtol=1e-14)
    assert 0 < (flags == 0).sum() < n
    assert np.array_equal(gw.call("sample2track", g["alt0"].astype(np.float64), g["speed0"].astype(np.float64), upd, ur, lo, hi), xyz)      # nlhs = 1: no other slot
    two = gw.call("sample2track", g["alt0"].astype(np.float64), g["speed0"].astype(np.float64), upd, ur, lo, hi, nlhs=2)
    assert np.array_equal(two[1], flags)


def test_no_samples_give_empty_arrays_of_the_right_dims(gw, loaded):
    m = loaded("uncor_1200code_v2p1")
    S = gw.call("bn_sample", m.h, 0.0, 1.0, 0.0)
    assert S.shape == (0, m.ni)
    init, cnt, E_ = gw.call("sample_uncor", m.h, 0.0, 10.0, 1.0, 0.0, 0.0, 3.0, 4.0, 6.0, np.zeros((0, 0)), 16.0, nlhs=3)
    assert init.shape == (0, m.ni) and cnt.shape == (0, 1) and E_.shape == (16, 3, 0)
    g = loaded("terminal_v3_radar_encounter_model")
    out, att, lw = gw.call("geom_sample", g.h, 0.0, 1.0, 0.0, nlhs=3)
    assert out.shape == (0, g.ni) and att.shape == (0, 1) and lw.shape == (0, 1)


def test_a_from_struct_model_with_an_edited_table_samples_what_the_oracle_samples(gw, model_dir, gpu_ctx):
    path = em_io.materialize_model("uncor_1200code_v2p1", model_dir)
    s = gw.call("em_read", path)
    pp = O.parse_model_txt(path)
    v = 3                                                                    # the speed variable: every column redrawn
    rs = np.random.RandomState(11)
    new = np.asfortranarray(rs.randint(0, 50, s["N_initial"][v, 0].shape).astype(np.float64) + np.eye(*s["N_initial"][v, 0].shape)[:, :1])
    N = s["N_initial"].copy()
    N[v, 0] = new
    d = dict(s)
    d["N_initial"] = N
    h = gw.call("from_struct", d)
    try:
        n, T, seed = 257, 30, 21
        idx = uncor_indices(pp)
        init, cnt, E_ = gw.call("sample_uncor", h, float(n), float(T), float(seed), float(FIRST), 0.0, float(idx["idx_L"]), float(idx["idx_v"]), float(idx["idx_dh"]), nlhs=3)
        before = O.uncor_sample(O.OracleModel(pp), n, T, seed, first_index=FIRST, want_dense=False)
        pp["N_initial"][v] = np.array(new)
        ref = O.uncor_sample(O.OracleModel(pp), n, T, seed, first_index=FIRST, want_dense=False)
        assert not np.array_equal(before["init_val"], ref["init_val"])      # the edit matters
        got = native.sample_dbn_host(gpu_ctx, _Borrowed(mexrt.handle(h)), n, T, seed, first_index=FIRST, want_dense=False, want_events=True, event_cap=512, pinned=False, **idx)
        assert_uncor_parity(got, ref, T)
        check_uncor_outputs(init, cnt, E_, got, ref, n, 7, 512)
    finally:
        gw.call("free", h, nlhs=0)
