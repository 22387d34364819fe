"""Without a GPU: the argument checks, bounds and bindings of sample2track's device text path (emgpu_parse_table_host, emgpu_format_f0_host,
emgpu_csv_bound, emgpu_tracks_text_host, legacy.sample2track(text=...)).  What they compute is checked on the GPU: tests/test_gpu_track_text.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from em_model_manned_bayes_amd import _lib as L, legacy, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("emgpu_parse_table_host", "emgpu_format_f0_host", "emgpu_csv_bound", "emgpu_tracks_text_host")


def test_null_handles_are_argument_errors_without_a_device():
    lib = L.lib()
    p = native.track_params(1, 1, 1.0, 1.0, 1.0, 0.0, 1.0)
    rows = C.c_int64(7)
    assert lib.emgpu_parse_table_host(None, None, 0, 3, None, 0, C.byref(rows), None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
    assert lib.emgpu_format_f0_host(None, None, 0, None, 0, None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
    assert lib.emgpu_tracks_text_host(None, C.byref(p), C.byref(L.TracksTextIn()), C.byref(L.TracksTextOut())) == L.ERR_ARG
    assert b"null" in lib.emgpu_last_error()
    assert lib.emgpu_tracks_text_host(None, None, None, None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
    assert lib.emgpu_csv_bound(-1, 0) == -1 and lib.emgpu_csv_bound(0, -1) == -1      # (no handle to be null: negative counts are the bad argument)


def test_csv_bound_is_its_closed_form():
    """22 bytes of header per file and 74 per row: "%i" of a second at most 10 characters, three times a sign and 19 digits, three commas, the
    newline."""
    assert len("time_s,x_ft,y_ft,z_ft\n") == 22 and len("%i,%0.0f,%0.0f,%0.0f\n" % (2 ** 31 - 1, -(2.0 ** 63 - 1024), -(2.0 ** 63 - 1024), -(2.0 ** 63 - 1024))) == 74
    for n, rows in ((0, 0), (1, 1), (25000, 25000 * 161), (10 ** 6, 241 * 10 ** 6), (2 ** 31, 2 ** 40)):
        assert native.csv_bound(n, rows) == 22 * n + 74 * rows


def struct_fields(name):
    """the field names of a typedef struct of include/emgpu.h, in order"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "emgpu.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [re.sub(r"[\s*]", "", part).split("[")[0] for part in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    return out


def test_struct_mirrors_have_the_headers_sizes_and_field_order():
    # emgpu_tracks_text_in: char*, i64, 4 x i32, 3 x double*        emgpu_tracks_text_out: 4 pointers, i64, 3 pointers, i64, pointer
    assert C.sizeof(L.TracksTextIn) == 8 + 8 + 4 * 4 + 3 * 8 and C.sizeof(L.TracksTextOut) == 10 * 8
    assert [f for f, _ in L.TracksTextIn._fields_] == struct_fields("emgpu_tracks_text_in")
    assert [f for f, _ in L.TracksTextOut._fields_] == struct_fields("emgpu_tracks_text_out")
    assert [f for f, _ in L.TracksTextOut._fields_] == ["flags", "speed_minmax", "lengths", "csv", "csv_cap", "offsets", "totals", "xyz", "xyz_cap", "phase_ms"]
    for s in NEW:
        assert s in L.SYMBOLS and hasattr(L.lib(), s)


def boom(*a, **k):
    raise AssertionError("called")


def test_sample2track_refuses_an_unknown_reader_before_a_file_is_opened(monkeypatch):
    monkeypatch.setattr(legacy, "em_read", boom)
    monkeypatch.setattr(legacy, "_read_table", boom)
    monkeypatch.setattr(legacy, "_read_rows", boom)
    monkeypatch.setattr(native, "default_context", boom)
    with pytest.raises(ValueError, match="text"):
        legacy.sample2track("no_such_model.txt", "no_initial.txt", "no_transition.txt", text="bogus")
    assert inspect.signature(legacy.sample2track).parameters["text"].default == "host"


def test_the_host_reader_never_calls_the_new_bindings(monkeypatch, tmp_path, model_dir):
    """text="host" (the default) goes the parent's way: with the new bindings replaced by functions that raise, it gets as far as the parent
    did -- to the track kernel's context (no device here, or a device and then a complete run)."""
    from em_model_manned_bayes_amd import em_io
    for f in ("parse_table", "tracks_text_host", "format_f0"):
        monkeypatch.setattr(native, f, boom)
    monkeypatch.setattr(legacy, "_sample2track_device_text", boom)
    monkeypatch.setattr(legacy, "_read_rows", boom)
    path = em_io.materialize_model("uncor_1200code_v2p1", model_dir)
    fi, ft = tmp_path / "initial.txt", tmp_path / "transition.txt"
    fi.write_text("id G A L v dotV dotH dotPsi \n1 1 2 1500 100 0 0 0\n")
    ft.write_text("initial_id t dotV dotH dotPsi \n1 0 0 0 0\n1 1 0.5 100 1\n")
    seen = []
    real = native.sample2track_host
    monkeypatch.setattr(native, "default_context", lambda *a: seen.append("ctx") or (_ for _ in ()).throw(L.EmgpuError(L.ERR_NO_DEVICE, "no device in this test")))
    monkeypatch.setattr(native, "sample2track_host", lambda *a, **k: seen.append("kernel") or real(*a, **k))
    with pytest.raises(L.EmgpuError):
        legacy.sample2track(path, str(fi), str(ft), out_dir_parent=str(tmp_path / "out"), verbose=False)
    assert seen == ["ctx"]                     # both files were read and grouped by the host code; nothing new was touched
    with pytest.raises(AssertionError, match="called"):
        legacy.sample2track(path, str(fi), str(ft), out_dir_parent=str(tmp_path / "out"), verbose=False, text="device", ctx=object())


def test_the_epilogue_helpers_give_sample2track_ms_directories_and_names():
    """The pieces both readers share, against answers worked out by hand from sample2track.m.
    :150-158: the model's altitude limits 50 and 5000 ft are no multiples of 100, so the edges are floor(50 - 50) : 100 : 5000 + 200, i.e.
    0, 100, ..., 5200; a first edge below zero becomes 0 (limits 20 .. 1000: -30, 70, 170, ... -> 0, 70, 170, ...).
    :263: discretize(z0, L) puts z0 into [L(k), L(k + 1)) and the last edge into the last bin; outside the edges it gives NaN, an error here.
    :249: sprintf('%i', round(x)) with MATLAB's round, half away from zero: 2500.5 -> 2501, 202.5 -> 203 (numpy and Python give 202)."""
    g = legacy._altitude_grid(50.0, 5000.0)
    assert g[0] == 0 and g[-1] == 5200 and len(g) == 53 and np.all(np.diff(g) == 100)
    assert legacy._altitude_grid(0.0, 5000.0).tolist() == list(range(0, 5201, 100))       # limits on the grid: min : 100 : max + 200
    low = legacy._altitude_grid(20.0, 1000.0)
    assert low[0] == 0 and low[1] == 70 and low[2] == 170
    assert legacy._altitude_directory(g, 1500.0) == "1500ft" and legacy._altitude_directory(g, 1499.9) == "1400ft"
    assert legacy._altitude_directory(g, 5200.0) == "5100ft"
    with pytest.raises(ValueError, match="outside the altitude directories"):
        legacy._altitude_directory(g, 5201.0)
    with pytest.raises(ValueError, match="outside the altitude directories"):
        legacy._altitude_directory(g, -1.0)
    assert legacy._track_file_name(12, 2, 2500.5, 202.5) == "BAYES_t12_id2_alt2501_speed203.csv"
    assert legacy._track_file_name(0, 1, 1499.4, 99.5) == "BAYES_t0_id1_alt1499_speed100.csv"
    assert legacy._host_csv(np.array([[0.0, 0.0, 1500.0], [168.8, -0.4, 1501.5]])) == b"time_s,x_ft,y_ft,z_ft\n0,0,0,1500\n1,169,-0,1502\n"
