"""Scoring a trace, the parts that need no GPU: the log tables emgpu_model_log_prob hands out against score_ref.tables, their identity with
what emgpu_start_grid_log_weight sums, the getter's conventions, and the argument checks of emgpu_score_dbn_* (made before any device work:
there is no context on this box to do any)."""
import ctypes as C

import numpy as np
import pytest

import score_ref as R
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native

MODELS = ("uncor_1200code_v2p1", "cor_v1", "glider_v1", "balloon_v1")
_cache = {}


def _model(name, model_dir):
    """(a fresh NativeModel, the parms of em_read) of the model's .txt"""
    if name not in _cache:
        _cache[name] = em_io.materialize_model(name, model_dir)
    parms = em_io.em_read(_cache[name])
    return parms["native"], parms


def _assert_tables(nm, want):
    checked = 0
    for network, nodes in ((0, range(nm.n_initial)), (1, sorted(want["transition"]))):
        for v in nodes:
            got, ref = nm.log_prob(network, v + 1), (want["initial"][v] if network == 0 else want["transition"][v])
            assert got.shape == ref.shape, (network, v)
            special = np.isinf(ref) | (ref == 0.0)
            assert np.array_equal(got[special], ref[special]), (network, v)          # -inf and 0.0: exactly
            assert np.all(np.abs(got[~special] - ref[~special]) <= 1e-12), (network, v)
            assert not np.isnan(got).any()
            checked += got.size
    return checked


@pytest.mark.parametrize("name", MODELS)
def test_log_prob_tables_against_the_numpy_restatement(name, model_dir):
    nm, parms = _model(name, model_dir)
    assert _assert_tables(nm, R.tables(parms, 0.0)) > 0
    if name != "balloon_v1":
        assert any(np.isinf(t).any() for t in R.tables(parms, 0.0)["initial"] + list(R.tables(parms, 0.0)["transition"].values()))
    nm.set_prior(1.0)
    want = R.tables(parms, 1.0)
    _assert_tables(nm, want)
    assert all(np.isfinite(t).all() for t in want["initial"])       # a constant prior leaves no empty column and no impossible bin
    for v in range(nm.n_initial):                                    # first-slice nodes of the transition network have no table
        assert nm.log_prob(1, v + 1).size == 0


@pytest.mark.parametrize("name", ("uncor_1200code_v2p1", "cor_v1"))
def test_initial_entries_are_what_start_grid_log_weight_sums(name, model_dir):
    nm, parms = _model(name, model_dir)
    g = R.graph(parms)
    rs = np.random.RandomState(5)
    grid = np.stack([rs.randint(1, int(r) + 1, size=200) for r in g["r_i"]], axis=1).astype(np.int32)     # every node preset
    got = native.start_grid_log_weight(nm, grid)
    want, initial = R.score(R.lib_tables(nm), g, grid)
    assert R.same_bits(got, want) and R.same_bits(got, initial)
    assert np.isfinite(got).any()


def test_log_prob_getter_conventions(model_dir):
    nm, parms = _model("uncor_1200code_v2p1", model_dir)
    lib = L.lib()
    r, q = parms["N_transition"][8].shape
    assert lib.emgpu_model_log_prob(nm._h, 1, 9, None, 0) == r * q                       # the count alone
    buf = np.zeros(r * q)
    assert lib.emgpu_model_log_prob(nm._h, 1, 9, buf.ctypes.data_as(C.c_void_p), r * q - 1) == L.ERR_ARG and b"too small" in lib.emgpu_last_error()
    assert lib.emgpu_model_log_prob(nm._h, 1, 9, buf.ctypes.data_as(C.c_void_p), r * q) == r * q
    assert np.array_equal(buf.reshape(q, r).T, nm.log_prob(1, 9))                        # column-major
    assert lib.emgpu_model_log_prob(None, 0, 1, None, 0) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
    for network in (-1, 2):
        assert lib.emgpu_model_log_prob(nm._h, network, 1, None, 0) == L.ERR_ARG and b"network" in lib.emgpu_last_error()
    for network, node in ((0, 0), (0, nm.n_initial + 1), (1, 0), (1, nm.n_transition + 1)):
        assert lib.emgpu_model_log_prob(nm._h, network, node, None, 0) == L.ERR_ARG and b"node" in lib.emgpu_last_error()
    assert lib.emgpu_model_log_prob(nm._h, 1, 1, None, 0) == 0


def test_score_entry_points_check_their_arguments_before_any_device_work(model_dir):
    nm, _ = _model("uncor_1200code_v2p1", model_dir)
    lib = L.lib()
    ib, db, ll = np.ones((7, 64), np.uint8), np.ones((2, 3, 64), np.uint32), np.zeros(64)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for f in (lib.emgpu_score_dbn_device, lib.emgpu_score_dbn_host):
        def call(p, model=nm, init=ib, dyn=db, out=ll, ctx=None):
            return f(ctx, None if model is None else model._h, None if p is None else C.byref(p), None if init is None else P(init),
                     None if dyn is None else P(dyn), None if out is None else P(out), None)
        ok = native.score_params(64, 5)
        assert call(None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
        assert call(ok, model=None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
        assert call(ok, init=None) == L.ERR_ARG and b"null init_bin" in lib.emgpu_last_error()
        assert call(ok, out=None) == L.ERR_ARG and b"null init_bin or log_lik" in lib.emgpu_last_error()
        assert call(ok, dyn=None) == L.ERR_ARG and b"null dyn_bin" in lib.emgpu_last_error()
        assert call(native.score_params(-1, 5)) == L.ERR_ARG and b"n < 0" in lib.emgpu_last_error()
        assert call(native.score_params(64, 0)) == L.ERR_ARG and b"sample_time" in lib.emgpu_last_error()
        assert call(native.score_params(64, 5, transition_mode=2)) == L.ERR_ARG and b"transition_mode" in lib.emgpu_last_error()
        assert call(native.score_params(64, 5, ld=100, col_offset=37)) == L.ERR_ARG and b"col_offset + n exceeds ld" in lib.emgpu_last_error()
        assert call(native.score_params(64, 5, ld=100, col_offset=-1)) == L.ERR_ARG and b"col_offset" in lib.emgpu_last_error()
        # nothing left to object to but the missing context (sample_time 1 needs no dyn_bin)
        assert call(ok) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(native.score_params(64, 1), dyn=None) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(native.score_params(64, 5, ld=100, col_offset=36)) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
    assert C.sizeof(L.ScoreParams) == 8 + 4 + 4 + 8 + 8


def test_the_new_symbols_are_bound():
    for s in ("emgpu_model_log_prob", "emgpu_score_dbn_device", "emgpu_score_dbn_host", "emgpu_device_upload", "emgpu_device_download"):
        assert s in L.SYMBOLS and hasattr(L.lib(), s)
    lib, buf = L.lib(), np.zeros(4)
    for f in (lib.emgpu_device_upload, lib.emgpu_device_download):      # no context: an argument error, whatever else is passed
        assert f(None, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), 32) == L.ERR_ARG and b"null ctx" in lib.emgpu_last_error()


def test_pack_dyn_bin_inverts_unpack():
    rs = np.random.RandomState(3)
    for n, T, nd in ((1, 1, 1), (5, 4, 3), (7, 5, 2), (3, 61, 4)):
        db = rs.randint(1, 9, size=(n, T, nd)).astype(np.uint8)
        packed = native.pack_dyn_bin(db)
        assert packed.shape == ((T + 3) // 4, nd, n) and packed.dtype == np.uint32
        assert np.array_equal(native.unpack_dyn_bin(packed, T), db)
        if T % 4:
            assert not (packed[-1] >> (8 * (T % 4))).any()           # padding columns are 0


def test_sample_weighted_refuses_models_of_different_shapes(model_dir):
    a, _ = _model("uncor_1200code_v2p1", model_dir)
    b, _ = _model("uncor_1200code_v1", model_dir)
    with pytest.raises(ValueError):
        native.sample_weighted_host(None, a, b, 10, 5, 1)
    # a start grid or an index list must be an array of the call's shape: a host address never reaches the device call
    for bad in (dict(start=np.zeros((9, 7), np.int32)), dict(start=4096), dict(indices=np.zeros(9, np.uint64)), dict(indices=4096)):
        with pytest.raises(ValueError):
            native.sample_weighted_host(None, a, a, 10, 5, 1, **bad)
