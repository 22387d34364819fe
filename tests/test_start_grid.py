"""CPU: the host side of start grids on the fast kernels -- emgpu_start_grid_log_weight against start_log_weight, its errors, makeStartGrid,
the binding's symbol list and the structs whose sizes other tests pin.  The GPU side: test_gpu_start_grid.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, legacy, native
from em_model_manned_bayes_amd import encounter_model as E
import start_grid_cases as S
from util import load_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", S.MODELS)
def test_grid_log_weight_is_start_log_weight_row_by_row(name, model_dir):
    nm, _, _ = load_pair(name, model_dir)
    rows = S.rows_of(name, model_dir)
    grid = S.grid_of(name, model_dir, 25)
    lw = native.start_grid_log_weight(nm, grid)
    assert lw.dtype == np.float64 and lw.shape == (25,)
    try:
        for k, row in enumerate(rows):
            nm.set_start([int(v) or None for v in row])
            want = nm.start_log_weight()
            assert np.all(lw[k::6] == lw[k]) and abs(lw[k] - want) < 1e-12, (k, lw[k], want)   # the tolerance of test_host.py::test_start_log_weight
        assert lw[1] == 0.0 and np.all(lw[[0, 2, 3, 4, 5]] < 0) and np.all(np.isfinite(lw))
        # a 0 entry means the model's own start: an all-zero grid under start = R0 weighs like R0, and a row's own entry wins over it
        nm.set_start([int(v) or None for v in rows[0]])
        assert np.all(native.start_grid_log_weight(nm, np.zeros((3, nm.n_initial), dtype=np.int32)) == lw[0])
        assert native.start_grid_log_weight(nm, rows[3:4])[0] != lw[0]
    finally:
        nm.set_start([None] * nm.n_initial)


@pytest.mark.parametrize("name", S.MODELS)
def test_grid_log_weight_refuses_what_the_sampler_refuses(name, model_dir):
    nm, _, _ = load_pair(name, model_dir)
    ni = nm.n_initial
    good = S.grid_of(name, model_dir, 12)
    orphan = np.zeros(ni, dtype=np.int32); orphan[2] = 2          # the third variable without its parents
    too_big = np.zeros(ni, dtype=np.int32); too_big[0] = 9        # the root has 4 or 5 bins
    negative = np.zeros(ni, dtype=np.int32); negative[0] = -1
    for bad, at in ((orphan, 7), (too_big, 0), (negative, 11)):
        g = good.copy()
        g[at] = bad
        if at < 11:
            g[11] = bad                                               # a later bad row does not change which one is named
        with pytest.raises(L.EmgpuError) as ei:
            native.start_grid_log_weight(nm, g)
        assert ei.value.code == L.ERR_PRESET and ("row %d " % at) in str(ei.value), str(ei.value)
        assert ei.value.identifier == "Attempt to preset a dependent variable"
    assert np.all(np.isfinite(native.start_grid_log_weight(nm, good)))   # and a valid call afterwards is served


def test_grid_log_weight_of_nothing_and_null_arguments(model_dir):
    nm, _, _ = load_pair("uncor_1200code_v2p1", model_dir)
    assert native.start_grid_log_weight(nm, np.zeros((0, 7), dtype=np.int32)).shape == (0,)
    lib = L.lib()
    grid = np.zeros((2, 7), dtype=np.int32)
    out = np.zeros(2)
    assert lib.emgpu_start_grid_log_weight(nm._h, None, 0, None) == L.OK
    assert lib.emgpu_start_grid_log_weight(None, grid.ctypes.data, 2, out.ctypes.data) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
    assert lib.emgpu_start_grid_log_weight(nm._h, None, 2, out.ctypes.data) == L.ERR_ARG
    assert lib.emgpu_start_grid_log_weight(nm._h, grid.ctypes.data, 2, None) == L.ERR_ARG
    assert lib.emgpu_start_grid_log_weight(nm._h, grid.ctypes.data, -1, out.ctypes.data) == L.ERR_ARG
    with pytest.raises(ValueError):
        native.start_grid_log_weight(nm, np.zeros((2, 6), dtype=np.int32))
    # the track entry points with a grid: null handles are an argument error, no device is touched
    p = native.utrack_params(nm, 4, 10, 1)
    for f in (lib.emgpu_track_uncor_grid_host, lib.emgpu_track_uncor_grid_device):
        assert f(None, nm._h, C.byref(p), None, None, None, None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()


def test_make_start_grid_order_and_counts(model_dir):
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    grid, comb = mdl.makeStartGrid({"G": [1], "A": [1, 2, 3, 4], "L": [1, 2, 3, 4]}, 5)       # RUN_uncor.m:35-47
    assert grid.dtype == np.int32 and grid.shape == (80, 7) and comb.shape == (80,)
    assert np.array_equal(comb, np.repeat(np.arange(16), 5))
    # InitStartTerminal.m:57-90: the first label is the outermost loop, the last the innermost, each combination nSamples times in a row
    want = [[1, a, l, 0, 0, 0, 0] for a in (1, 2, 3, 4) for l in (1, 2, 3, 4) for _ in range(5)]
    assert np.array_equal(grid, np.array(want, dtype=np.int32))
    g2, c2 = mdl.makeStartGrid({'"A"': [4, 2], "G": [3, 1, 2]})                               # the dict's order, not the variables'
    assert np.array_equal(g2[:, :2], [[3, 4], [1, 4], [2, 4], [3, 2], [1, 2], [2, 2]]) and np.all(g2[:, 2:] == 0)
    assert np.array_equal(c2, np.arange(6))
    for bad in ({"nope": [1]}, {"G": [5]}, {"G": [0]}, {"G": []}, {"G": [1], '"G"': [2]}):
        with pytest.raises(ValueError):
            mdl.makeStartGrid(bad)
    with pytest.raises(ValueError):
        mdl.makeStartGrid({"G": [1]}, 0)
    # the grid is what the log-weight function and the class methods take
    lw = native.start_grid_log_weight(mdl.native, grid)
    assert lw.shape == (80,) and np.all(lw < 0) and np.all(lw.reshape(16, 5) == lw.reshape(16, 5)[:, :1])
    with pytest.raises(ValueError):
        mdl._start_grid(grid, 79)


def test_the_class_layer_has_the_keywords_and_the_binding_the_entry_points():
    for f in (E.UncorEncounterModel.sample, E.UncorEncounterModel.track):
        sig = inspect.signature(f)
        assert sig.parameters["start_grid"].default is None and sig.parameters["return_log_weight"].default is False
    assert inspect.signature(legacy.em_sample).parameters["start_grid"].default is None
    assert inspect.signature(native.track_uncor_host).parameters["start"].default is None
    hdr = open(os.path.join(ROOT, "include", "emgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(emgpu_[a-z0-9_]+)\s*\(", hdr)) == set(L.SYMBOLS)
    for s in ("emgpu_start_grid_log_weight", "emgpu_track_uncor_grid_host", "emgpu_track_uncor_grid_device"):
        assert s in L.SYMBOLS and hasattr(L.lib(), s)
    # new data travels in new functions: the structs keep the sizes that test_lazy_sample.py and test_text_format.py pin
    assert C.sizeof(L.UncorOut) == 10 * 8 + 4 * 4 and C.sizeof(L.TextOut) == 8 * 8
    assert C.sizeof(L.SampleParams) == 3 * 8 + 8 * 4 + 8 + 2 * 4 + 2 * 8 and C.sizeof(L.SampleOut) == 10 * 8 and C.sizeof(L.UTrackParams) == 3 * 8 + 14 * 4
