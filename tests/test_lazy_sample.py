"""UncorEncounterModel.sample(..., lazy=True) without a GPU: the lazy per-sample sequences on hand-made flat arrays, and the C entry point
emgpu_sample_uncor_host's argument checks and binding."""
import ctypes as C
import inspect

import numpy as np
import pytest

from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import encounter_model as E
from em_model_manned_bayes_amd import native


def _flat_events(counts, seed=0):
    rng = np.random.default_rng(seed)
    rows = int(np.sum(counts))
    ev = np.zeros(rows, dtype=native.EVENT_DTYPE)
    ev["dt"] = rng.integers(0, 30, rows)
    ev["var"] = rng.integers(0, 8, rows)
    ev["bin"] = rng.integers(1, 5, rows)
    ev["value"] = rng.standard_normal(rows).astype(np.float32)
    return ev


def test_lazy_events_index_slice_iterate_like_the_eager_list():
    counts = np.array([3, 0, 5, 1, 2], dtype=np.uint32)
    flat = _flat_events(counts)
    seq = E.LazyEvents(flat, counts)
    # the eager call's list: [dt, var, value] as float64, split by the counts (encounter_model.py, UncorEncounterModel.sample)
    ev_all = np.stack([flat["dt"].astype(np.float64), flat["var"].astype(np.float64), flat["value"].astype(np.float64)], axis=1)
    eager = native.split_rows(ev_all, np.cumsum(counts.astype(np.int64)))
    assert len(seq) == 5 and list(seq.offsets) == [0, 3, 3, 8, 9, 11] and seq.flat is flat
    for i in range(-5, 5):
        g = seq[i]
        assert g.dtype == np.float64 and g.shape == eager[i].shape and np.array_equal(g, eager[i])
    assert seq[1].shape == (0, 3)
    for a, b in zip(seq, eager):
        assert np.array_equal(a, b)
    assert isinstance(seq[1:4], list) and len(seq[1:4]) == 3 and np.array_equal(seq[::-2][0], eager[4])
    assert seq[np.int64(2)].shape == (5, 3)
    for bad in (5, -6, 100):
        with pytest.raises(IndexError):
            seq[bad]
    with pytest.raises(TypeError):
        seq[1.0]
    with pytest.raises(TypeError):
        seq[0] = None


def test_lazy_samples_are_views_of_the_flat_block():
    block = np.arange(4 * 3 * 7, dtype=np.float64).reshape(4, 3, 7)
    seq = E.LazySamples(block)
    assert len(seq) == 4 and seq.flat is block
    for i in range(-4, 4):
        assert seq[i].base is block or seq[i].base is block.base
        assert np.array_equal(seq[i], block[i]) and seq[i].shape == (3, 7) and seq[i].dtype == np.float64
    assert [s.shape for s in seq] == [(3, 7)] * 4 and len(seq[:]) == 4 and seq[5:] == []
    with pytest.raises(IndexError):
        seq[4]


def test_lazy_controls_build_encounter_model_events_only_on_access(monkeypatch):
    counts = np.array([2, 0, 3], dtype=np.uint32)
    flat = np.arange(5 * 4, dtype=np.float64).reshape(5, 4)
    built = []
    orig = E.EncounterModelEvents._of_rows.__func__

    def counting(cls, m):
        built.append(m.shape)
        return orig(cls, m)
    monkeypatch.setattr(E.EncounterModelEvents, "_of_rows", classmethod(counting))
    seq = E.LazyControls(flat, counts)
    assert len(seq) == 3 and built == []          # nothing is created per sample before it is accessed
    e = seq[-1]
    assert built == [(3, 4)] and isinstance(e, E.EncounterModelEvents)
    assert np.array_equal(e.event, flat[2:5]) and np.array_equal(e.time_s, flat[2:5, 0])
    assert np.array_equal(seq[1].event, np.zeros((1, 4)))   # an empty list reads as one zero row (EncounterModelEvents.m:41-47)
    assert len(built) == 2
    assert [x.event.shape[0] for x in seq] == [2, 1, 3] and len(built) == 5
    with pytest.raises(IndexError):
        seq[-4]


def test_sample_has_the_lazy_switch_and_the_binding_declares_the_entry_point():
    sig = inspect.signature(E.UncorEncounterModel.sample)
    assert sig.parameters["lazy"].default is False
    assert "emgpu_sample_uncor_host" in L.SYMBOLS
    assert C.sizeof(L.UncorOut) == 10 * 8 + 4 * 4


def test_uncor_host_entry_point_rejects_missing_handles_without_a_device():
    lib = L.lib()
    p, _ = native.make_params(10, 10, 1, event_cap=16)
    o = L.UncorOut()
    assert lib.emgpu_sample_uncor_host(None, None, C.byref(p), C.byref(o)) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
    assert lib.emgpu_sample_uncor_host(None, None, None, None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
