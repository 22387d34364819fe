"""Without a GPU: the argument checks, bounds and bindings of the device text writer (emgpu_sample_text_host, emgpu_text_bound,
emgpu_format_g_host).  What the writer writes is checked on the GPU: tests/test_gpu_text_format.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from em_model_manned_bayes_amd import _lib as L, em_io, legacy, native

ALL_MODELS = sorted(f[:-4] for f in os.listdir(em_io.MODELS_DIR) if f.endswith(".npz"))


def test_null_handles_are_argument_errors_without_a_device():
    lib = L.lib()
    p, _ = native.make_params(10, 10, 1)
    o = L.TextOut()
    two = (C.c_int64 * 2)()
    assert lib.emgpu_sample_text_host(None, None, C.byref(p), C.byref(o)) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
    assert lib.emgpu_text_bound(None, 10, 10, two) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
    assert lib.emgpu_format_g_host(None, None, 0, None, 0, None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
    assert lib.emgpu_debug_format_paths(None, None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()


def test_struct_mirror_has_the_headers_size():
    # emgpu_text_out: char*, i64, char*, i64, i64*, i64, float*, float*
    assert C.sizeof(L.TextOut) == 8 * 8
    assert [f for f, _ in L.TextOut._fields_] == ["initial", "initial_cap", "transition", "transition_cap", "totals", "id_first", "init_val", "dyn_val"]
    for s in ("emgpu_sample_text_host", "emgpu_text_bound", "emgpu_format_g_host", "emgpu_debug_format_paths"):
        assert s in L.SYMBOLS and hasattr(L.lib(), s)


@pytest.mark.parametrize("name", ALL_MODELS)
def test_text_bound_is_its_closed_form(name, model_dir):
    """bytes[0] = n (21 + 13 n_initial), bytes[1] = n T 13 (2 + n_dyn): a "%g" of an f32 or of an id is at most 12 characters ("-1.17549e-38"),
    an id through "%d" at most 20, and one character (a space or the newline) follows each."""
    nm = native.NativeModel.load_txt(em_io.materialize_model(name, model_dir))
    assert len(ALL_MODELS) == 27
    for n, T in ((0, 1), (1, 1), (25000, 160), (10 ** 6, 240), (2 ** 40, 65535)):
        assert native.text_bound(nm, n, T) == (n * (21 + 13 * nm.n_initial), n * T * 13 * (2 + nm.n_dyn))
    two = (C.c_int64 * 2)()
    assert L.lib().emgpu_text_bound(nm._h, -1, 1, two) == L.ERR_ARG and L.lib().emgpu_text_bound(nm._h, 1, 0, two) == L.ERR_ARG


def test_no_value_is_longer_than_the_bound_assumes():
    """12 characters per "%g": the longest spellings of an f32 and of an id below 2^53, as the host writer spells them"""
    rs = np.random.RandomState(1)
    x = rs.randint(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    with np.errstate(invalid="ignore"):      # (signalling NaNs among the patterns)
        wide = x.astype(np.float64).tolist()
    assert max(len(legacy._g(v)) for v in wide) == 12
    assert max(len(legacy._g(v)) for v in (2 ** 53, 2 ** 31 - 1, 999999, 123456789)) <= 12 and len("%d" % (2 ** 63 - 1)) + 1 <= 21


def test_em_sample_refuses_an_unknown_writer_before_sampling(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("sampled")
    monkeypatch.setattr(native, "sample_dbn_host", boom)
    monkeypatch.setattr(native, "sample_text_host", boom)
    monkeypatch.setattr(native, "default_context", boom)
    with pytest.raises(ValueError, match="text"):
        legacy.em_sample("no_such_model.txt", text="bogus")
    for kw in (dict(return_arrays=False), dict(id_first=5), dict(text_batch=100)):
        with pytest.raises(ValueError, match="device"):
            legacy.em_sample("no_such_model.txt", **kw)                 # the host writer has none of these
    sig = inspect.signature(legacy.em_sample)
    assert sig.parameters["text"].default == "host" and sig.parameters["return_arrays"].default is True
