"""UncorEncounterModel.sample(..., lazy=True) on the GPU: the four outputs against the eager call bit for bit (dtype, shape and every element),
and against the oracle's events2samples / events2controls."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native
from em_model_manned_bayes_amd import encounter_model as E

pytestmark = pytest.mark.gpu

MODELS = ["uncor_1200code_v2p1", "uncor_1200only_fwse_v1p2", "uncor_1200exclude_rotorcraft_v1p2", "uncor_allcode_fwsingle_v1"]


def _same(a, b):
    return isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def assert_lazy_equals_eager(lazy, eager):
    li, le, ls, lE = lazy
    ei, ee, es, eE = eager
    assert _same(li, ei)
    assert isinstance(le, E.LazyEvents) and isinstance(ls, E.LazySamples) and isinstance(lE, E.LazyControls)
    n = len(ee)
    assert len(le) == len(ls) == len(lE) == len(es) == len(eE) == n
    for i in range(n):
        assert _same(le[i], ee[i]), i
        assert _same(ls[i], es[i]), i
        g, r = lE[i], eE[i]
        assert isinstance(g, E.EncounterModelEvents) and _same(g.event, r.event), i
        for f in ("time_s", "verticalRate_fps", "turnRate_radps", "longitudeAccel_ftpss"):
            assert _same(getattr(g, f), getattr(r, f)), (i, f)
    if n:   # negative indices, slices and iteration reach the same items
        assert _same(le[-1], ee[-1]) and _same(ls[-n], es[0]) and _same(lE[-1].event, eE[-1].event)
        assert all(_same(a, b) for a, b in zip(ls[n // 2:], es[n // 2:]))
        assert all(_same(a.event, b.event) for a, b in zip(lE, eE))


def _both(mdl, ctx, *args, **kw):
    eager = mdl.sample(*args, ctx=ctx, **kw)
    k_eager = ctx.last_kernel()
    lazy = mdl.sample(*args, ctx=ctx, lazy=True, **kw)
    assert ctx.last_kernel() == k_eager, (ctx.last_kernel(), k_eager)   # the sampler instance, not a formatting kernel
    return lazy, eager


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("n", [1, 255, 257])
def test_lazy_sample_equals_eager(name, n, gpu_ctx, model_dir):
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model(name, model_dir))
    lazy, eager = _both(mdl, gpu_ctx, n, 240, seed=7, first_index=2 ** 35 + 13)
    assert_lazy_equals_eager(lazy, eager)
    tm = mdl.last_sample_timing
    assert {"native_s", "format_s", "kernel_ms", "d2h_ms", "bytes_d2h", "calls", "total_s"} <= set(tm)


def test_lazy_sample_across_several_chunks_equals_eager(gpu_ctx, model_dir, monkeypatch):
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", "64")
    lazy, eager = _both(mdl, gpu_ctx, 20011, 240, seed=11, first_index=123457)
    assert gpu_ctx.host_stats()["chunks"] >= 4
    assert_lazy_equals_eager(lazy, eager)
    # the flat arrays behind the sequences are the eager lists laid end to end
    le, lE = lazy[1], lazy[3]
    assert np.array_equal(le.offsets[1:], np.cumsum([len(x) for x in eager[1]]))
    assert np.array_equal(lE.flat, np.concatenate([x.event for x in eager[3] if len(x.time_s)]))


@pytest.mark.parametrize("name", ["uncor_1200only_fwse_v1p2", "uncor_1200exclude_rotorcraft_v1p2"])
def test_lazy_sample_with_quantize_and_layers_equals_eager(name, gpu_ctx, model_dir):
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model(name, model_dir), isOverwriteZeroBoundaries=True)
    layers = np.array([[50, 500], [500, 1200], [1200, 3000], [3000, 5000]], dtype=np.float64)
    for kw in (dict(isQuantize500=True), dict(layers=layers), dict(layers=layers, isQuantize500=True)):
        lazy, eager = _both(mdl, gpu_ctx, 777, 120, seed=3, first_index=99, **kw)
        assert_lazy_equals_eager(lazy, eager)


def test_lazy_sample_per_step_equals_eager(gpu_ctx, model_dir):
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    lazy, eager = _both(mdl, gpu_ctx, 513, 200, seed=5, first_index=2 ** 33, transition_mode=L.TRANSITION_PER_STEP)
    assert_lazy_equals_eager(lazy, eager)


def test_lazy_sample_retries_a_list_that_outgrows_the_first_capacity(gpu_ctx, model_dir):
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    lazy, eager = _both(mdl, gpu_ctx, 300, 2400, seed=9)
    tm = mdl.last_sample_timing
    assert tm["retries"] >= 1 and tm["event_cap"] > 256 and max(len(x) for x in eager[1]) > 256
    assert_lazy_equals_eager(lazy, eager)


@pytest.mark.parametrize("pinned", [True, False])
def test_uncor_host_outputs_pinned_and_pageable_and_capacity_errors(pinned, gpu_ctx, model_dir):
    name = "uncor_1200code_v2p1"
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model(name, model_dir))
    nm, n, T, seed = mdl.native, 3001, 240, 21
    labs = mdl.labels_initial
    var = lambda s: labs.index('"%s"' % s) + 1
    ids = dict(idx_L=var("L"), idx_v=var("v"), idx_dh=var("\\dot h"))
    ctrl = (var("\\dot h"), var("\\dot \\psi"), var("\\dot v"))
    eager = mdl.sample(n, T, seed=seed, first_index=5, ctx=gpu_ctx)
    ref = native.sample_uncor_host(gpu_ctx, nm, n, T, seed, ctrl, first_index=5, pinned=pinned, **ids)
    rows_ev, rows_ct = ref["events"].shape[0], ref["controls"].shape[0]
    assert _same(ref["inits"], eager[0]) and np.array_equal(ref["samples"], np.stack(eager[2]))
    assert ref["attempts"].min() >= 1 and ref["host_stats"]["direct"] == 0   # the packed rows went through staging
    # rows into arrays of exactly the room they need (pinned when `pinned`), and into arrays one row short: the totals come back
    exact = native.sample_uncor_host(gpu_ctx, nm, n, T, seed, ctrl, first_index=5, pinned=pinned, events_cap=rows_ev, controls_cap=rows_ct, **ids)
    assert exact["host_stats"]["direct"] == (1 if pinned else 0)
    for k in ("inits", "ev_count", "events", "ctrl_count", "controls", "samples", "attempts"):
        assert _same(exact[k], ref[k]), k
    for short in (dict(events_cap=rows_ev - 1, controls_cap=rows_ct), dict(events_cap=rows_ev, controls_cap=rows_ct - 1)):
        with pytest.raises(L.EmgpuError) as ei:
            native.sample_uncor_host(gpu_ctx, nm, n, T, seed, ctrl, first_index=5, pinned=pinned, **short, **ids)
        assert ei.value.code == L.ERR_EVENT_CAP and ei.value.totals == (rows_ev, rows_ct)
    # a list longer than event_cap: the rows the lists need in full
    with pytest.raises(L.EmgpuError) as ei:
        native.sample_uncor_host(gpu_ctx, nm, n, T, seed, ctrl, event_cap=8, first_index=5, pinned=pinned, **ids)
    assert ei.value.code == L.ERR_EVENT_CAP and ei.value.totals[0] == rows_ev and np.array_equal(ei.value.ev_count, ref["ev_count"])
    # without samples: the rest unchanged
    nos = native.sample_uncor_host(gpu_ctx, nm, n, T, seed, ctrl, first_index=5, pinned=pinned, want_samples=False, **ids)
    assert nos["samples"] is None and _same(nos["controls"], ref["controls"]) and _same(nos["events"], ref["events"])


def test_lazy_sample_matches_reference_outputs(gpu_ctx, model_dir):
    """As test_uncor_class_sample_matches_reference_outputs, through the lazy outputs: the oracle's events2samples / events2controls."""
    for name in ("uncor_1200code_v2p1", "uncor_1200only_fwse_v1p2"):
        path = em_io.materialize_model(name, model_dir)
        mdl = E.UncorEncounterModel(parameters_filename=path)
        om = O.OracleModel(O.parse_model_txt(path))
        n, T, seed = 300, 120, 1
        out_inits, out_events, out_samples, out_EME = mdl.sample(n, T, seed=seed, ctx=gpu_ctx, lazy=True)
        ref = O.uncor_sample(om, n, T, seed)
        for i in range(n):
            r32 = ref["events"][i].copy()
            assert np.array_equal(out_events[i][:, :2], r32[:, :2])
            assert np.array_equal(out_inits[i].astype(np.float32), ref["init_val"][i].astype(np.float32))
            s = O.events2samples(ref["init_val"][i], r32[:, :3])
            assert out_samples[i].shape == (mdl.n_initial, T)
            assert np.array_equal(out_samples[i].astype(np.float32), s.astype(np.float32))
            ctl = O.events2controls(om, ref["init_val"][i], r32[:, :3])[:, [0, 2, 3, 1]]
            ctl[:, 1] /= 60.0; ctl[:, 2] = np.deg2rad(ctl[:, 2]); ctl[:, 3] *= 1.68780972222222
            np.testing.assert_allclose(out_EME[i].event, ctl, rtol=1.2e-7, atol=0)
            assert out_EME[i].event[0, 0] == 0


def _uncor_host_call(ctx, nm, n, T, seed, ctrl, ids, traj_pinned, rows_pinned, events_cap, controls_cap):
    """emgpu_sample_uncor_host through ctypes, the per-trajectory arrays and the row arrays each pinned (the context's pool) or pageable.
    Returns (rc, totals, arrays trimmed to the totals, host_stats)."""
    ni = nm.n_initial
    tr = ctx.pinned_empty if traj_pinned else (lambda shape, dt: np.full(shape, 0xAB, dtype=dt) if np.dtype(dt).kind in "ui" else np.full(shape, np.nan, dt))
    ro = ctx.pinned_empty if rows_pinned else (lambda shape, dt: np.zeros(shape, dtype=dt))
    p, keep = native.make_params(n, T, seed, event_cap=256, first_index=77, **ids)
    a = dict(inits=tr((n, ni), np.float64), ev_count=tr((n,), np.uint32), ctrl_count=tr((n,), np.uint32), attempts=tr((n,), np.int32),
             samples=tr((n, ni, T), np.float64), events=ro((max(events_cap, 1),), native.EVENT_DTYPE), controls=ro((max(controls_cap, 1), 4), np.float64))
    totals = np.zeros(2, dtype=np.int64)
    o = L.UncorOut()
    for k, v in a.items():
        setattr(o, k, v.ctypes.data)
    o.events_cap, o.controls_cap, o.totals = events_cap, controls_cap, totals.ctypes.data
    o.ctrl_var[:] = list(ctrl)
    rc = L.lib().emgpu_sample_uncor_host(ctx._h, nm._h, C.byref(p), C.byref(o))
    a["events"], a["controls"] = a["events"][: int(totals[0])], a["controls"][: int(totals[1])]
    return rc, (int(totals[0]), int(totals[1])), {k: np.array(v) for k, v in a.items()}, ctx.host_stats()


@pytest.mark.parametrize("traj_pinned,rows_pinned", [(True, True), (False, False), (True, False), (False, True)])
def test_uncor_host_across_several_chunks_equals_one_chunk(traj_pinned, rows_pinned, gpu_ctx, model_dir, monkeypatch):
    """emgpu_sample_uncor_host in chunks of 1 024 trajectories (five chunks) against one chunk, bit for bit, with the per-trajectory arrays
    and the row arrays pinned or pageable in every combination; then capacities that run out in a later chunk (events in the second,
    controls in the third): ERR_EVENT_CAP with the one-chunk call's totals."""
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    nm, labs = mdl.native, mdl.labels_initial
    var = lambda s: labs.index('"%s"' % s) + 1
    ids = dict(idx_L=var("L"), idx_v=var("v"), idx_dh=var("\\dot h"))
    ctrl = (var("\\dot h"), var("\\dot \\psi"), var("\\dot v"))
    n, T, seed = 5000, 240, 31
    call = lambda ev_cap, ct_cap: _uncor_host_call(gpu_ctx, nm, n, T, seed, ctrl, ids, traj_pinned, rows_pinned, ev_cap, ct_cap)
    monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", "8192")
    rc, totals, one, st = call(n * 256, n * 256)
    assert rc == L.OK and st["chunks"] == 1 and totals == (len(one["events"]), len(one["controls"]))
    assert one["attempts"].min() >= 1 and totals[0] > 0 and totals[1] > 0
    rc, t_exact, one_exact, _ = call(*totals)
    assert rc == L.OK and t_exact == totals
    monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", "1")
    rc, t_many, many, st = call(*totals)
    assert rc == L.OK and t_many == totals
    assert st["chunks"] == 5 and st["chunk_n"] == 1024 and st["direct"] == int(traj_pinned and rows_pinned), st
    assert st["event_rows"] == totals[0]
    for k in one:
        assert _same(many[k], one[k]), k
        assert _same(one_exact[k], one[k]), k
    # capacities that run out after the first chunk: the rows the call needs, as from one chunk
    ev_cap = int(one["ev_count"][:2048].sum()) - 1
    ct_cap = int(one["ctrl_count"][:3072].sum()) - 1
    assert ev_cap >= int(one["ev_count"][:1024].sum()) and ct_cap >= int(one["ctrl_count"][:2048].sum())
    for caps in ((ev_cap, totals[1]), (totals[0], ct_cap), (ev_cap, ct_cap)):
        rc, t_short, _, st = call(*caps)
        assert rc == L.ERR_EVENT_CAP and t_short == totals and st["chunks"] == 5, (caps, t_short)
        monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", "8192")
        rc, t_short1, _, st = call(*caps)
        assert rc == L.ERR_EVENT_CAP and t_short1 == totals and st["chunks"] == 1, (caps, t_short1)
        monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", "1")
