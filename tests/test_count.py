"""Counting a trace, the parts that need no GPU: the numpy restatement count_ref.count against a triple Python loop written out here, the
layout emgpu_count_layout hands out against the shapes of the model's own N tables for every shipped model, and the argument checks of
emgpu_count_dbn_* (made before any device work: there is no context on this box to do any)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import count_ref as R
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native
from em_model_manned_bayes_amd import encounter_model as E

SHIPPED = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(em_io.MODELS_DIR, "*.npz")))


def _hand_model(depend):
    """A (r 2) -> B (r 3) -> C (r 2, parents A and B); B and C are dynamic: B' <- A, B; C' <- B, C (and B' when depend)"""
    G_i = np.zeros((3, 3), dtype=bool)
    G_i[0, 1] = G_i[0, 2] = G_i[1, 2] = True
    G_t = np.zeros((5, 5), dtype=bool)
    G_t[[0, 1], 3] = True
    G_t[[1, 2], 4] = True
    G_t[3, 4] = depend
    return {"n_initial": 3, "G_initial": G_i, "r_initial": np.array([2, 3, 2]), "order_initial": np.array([1, 2, 3]), "n_transition": 5,
            "G_transition": G_t, "r_transition": np.array([2, 3, 2, 3, 2]), "temporal_map": np.array([[2, 4], [3, 5]])}


@pytest.mark.parametrize("depend,mode", [(False, R.AUTO), (False, R.PER_STEP), (True, R.AUTO)])
def test_count_ref_equals_a_triple_loop_on_a_hand_written_model(depend, mode):
    g = R.graph(_hand_model(depend))
    assert g["depend"] == depend
    per_step = depend or mode == R.PER_STEP
    ib = np.array([[1, 1, 1], [2, 3, 2], [1, 2, 2], [2, 2, 1], [0, 1, 2]])          # trajectory 4: A has bin 0
    T = 6
    db = np.zeros((5, T, 2), dtype=np.int64)
    db[0] = [[1, 1]] * T                                                           # never changes
    db[1] = [[1 + t % 3, 1 + t % 2] for t in range(T)]                             # changes every second
    db[2] = [[2, 2]] * (T - 1) + [[3, 1]]                                          # changes at T-1 only
    db[3] = [[1, 1], [1, 2], [4, 2], [2, 2], [2, 1], [2, 1]]                       # B has bin r + 1 at t = 2
    db[4] = [[1, 2]] * T
    # the definition, one observation at a time
    Ni = [np.zeros((2, 1), int), np.zeros((3, 2), int), np.zeros((2, 6), int)]
    Nt = [np.zeros((0, 0), int)] * 3 + [np.zeros((3, 6), int), np.zeros((2, 18 if depend else 6), int)]
    r = [2, 3, 2]
    good = lambda b, rr: 1 <= b <= rr   # noqa: E731
    skipped = 0
    for i in range(5):
        a, b, c = ib[i]
        for v, (own, parents) in enumerate(((a, []), (b, [(a, 2)]), (c, [(a, 2), (b, 3)]))):
            if not good(own, r[v]) or not all(good(x, rr) for x, rr in parents):
                skipped += 1
                continue
            col, stride = 0, 1
            for x, rr in parents:
                col += stride * (x - 1)
                stride *= rr
            Ni[v][own - 1, col] += 1
        for t in range(1, T):
            for k in range(2):
                own = db[i, t, k]
                tp = t - 1 if per_step else 0
                if k == 0:
                    parents = [(a, 2), (db[i, tp, 0], 3)]
                else:
                    parents = [(db[i, tp, 0], 3), (db[i, tp, 1], 2)] + ([(db[i, t if per_step else 0, 0], 3)] if depend else [])
                if not good(own, (3, 2)[k]) or not all(good(x, rr) for x, rr in parents):
                    skipped += 1
                    continue
                col, stride = 0, 1
                for x, rr in parents:
                    col += stride * (x - 1)
                    stride *= rr
                Nt[3 + k][own - 1, col] += 1
    got_i, got_t, got_skipped = R.count(g, ib, db, mode)
    assert got_skipped == skipped and skipped > 3
    for a, b in zip(got_i + got_t, Ni + Nt):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert sum(int(x.sum()) for x in got_i + got_t) == 5 * 3 + 5 * (T - 1) * 2 - skipped
    # the initial network alone, and T = 1: no transition is counted
    for d in (None, db[:, :1]):
        only_i, only_t, _ = R.count(g, ib, d, mode)
        assert all(np.array_equal(a, b) for a, b in zip(only_i, Ni)) and not any(x.any() for x in only_t)
    assert R.flat(Ni).tolist() == [int(x) for N in Ni for x in N.T.reshape(-1)] and R.flat(Ni).dtype == np.uint64


def test_count_ref_with_unit_weights_is_the_unweighted_count():
    """the one restatement's two forms agree where they must: weights of 1 change no table and no skip, corrupt bins included"""
    ib = np.array([[1, 1, 1], [2, 3, 2], [1, 2, 2], [2, 2, 1], [0, 1, 2]])          # trajectory 4: A has bin 0
    T = 6
    db = np.array([[[1 + (i + t) % 3, 1 + (i * t) % 2] for t in range(T)] for i in range(5)])
    db[3, 2, 0] = 4                                                                # B has bin r + 1 at t = 2
    for depend, mode in ((False, R.AUTO), (False, R.PER_STEP), (True, R.AUTO)):
        g = R.graph(_hand_model(depend))
        want_i, want_t, want_skipped = R.count(g, ib, db, mode)
        got_i, got_t, got_skipped = R.count(g, ib, db, mode, weights=np.ones(5, dtype=np.uint32))
        assert got_skipped == want_skipped and want_skipped > 3
        assert all(a.dtype == np.int64 for a in want_i + want_t) and all(a.dtype == np.uint64 for a in got_i + got_t)
        assert len(got_i) == len(want_i) == 3 and len(got_t) == len(want_t) == 5
        for a, b in zip(got_i + got_t, want_i + want_t):
            assert a.shape == b.shape and np.array_equal(a, b)
        assert sum(int(x.sum()) for x in got_i + got_t) == 5 * 3 + 5 * (T - 1) * 2 - want_skipped


@pytest.mark.parametrize("name", SHIPPED)
def test_count_layout_matches_the_models_own_tables(name, model_dir):
    assert len(SHIPPED) >= 20
    nm = native.NativeModel.load_txt(em_io.materialize_model(name, model_dir))
    for network, field, nodes in ((0, L.F_N_INITIAL, nm.n_initial), (1, L.F_N_TRANSITION, nm.n_transition)):
        off = nm.count_layout(network)
        assert off.dtype == np.int64 and off.shape == (nodes + 1,) and off[0] == 0
        sizes = [nm.get_f64(field, v + 1).size for v in range(nodes)]
        assert np.array_equal(np.diff(off), sizes)
        if network == 1 and nodes:
            assert sizes[0] == 0 and max(sizes) > 0            # first-slice nodes have no table and take no room
    # split_counts hands the arrays back in the shapes the model's setters take
    raw = [np.arange(int(nm.count_layout(k)[-1]), dtype=np.uint64) for k in (0, 1)]
    Ni, Nt = native.split_counts(nm, raw)
    g = R.graph(em_io.em_read(em_io.materialize_model(name, model_dir)))
    shp_i, shp_t = R.shapes(g)
    assert [a.shape for a in Ni] == shp_i
    assert [a.shape for a in Nt] == [shp_t.get(v, (0, 0)) for v in range(nm.n_transition)]
    assert np.array_equal(R.flat(Ni), raw[0]) and np.array_equal(R.flat(Nt), raw[1])


def test_count_layout_checks_its_arguments(model_dir):
    nm = native.NativeModel.load_txt(em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    lib, off = L.lib(), np.zeros(64, dtype=np.int64)
    P = off.ctypes.data_as(C.c_void_p)
    assert lib.emgpu_count_layout(None, 0, P) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
    assert lib.emgpu_count_layout(nm._h, 0, None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
    for network in (-1, 2):
        assert lib.emgpu_count_layout(nm._h, network, P) == L.ERR_ARG and b"network" in lib.emgpu_last_error()
    assert lib.emgpu_count_layout(nm._h, 1, P) == L.OK and off[nm.n_transition] == 74480    # the headline model's transition cells


def test_count_entry_points_check_their_arguments_before_any_device_work(model_dir):
    nm = native.NativeModel.load_txt(em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    lib = L.lib()
    ib, db = np.ones((7, 64), np.uint8), np.ones((2, 3, 64), np.uint32)
    ci, ct = (np.zeros(int(nm.count_layout(k)[-1]), np.uint64) for k in (0, 1))
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for f in (lib.emgpu_count_dbn_device, lib.emgpu_count_dbn_host):
        def call(p, model=nm, init=ib, dyn=db, out_i=ci, out_t=ct, ctx=None):
            return f(ctx, None if model is None else model._h, None if p is None else C.byref(p), None if init is None else P(init),
                     None if dyn is None else P(dyn), None if out_i is None else P(out_i), None if out_t is None else P(out_t))
        ok = native.score_params(64, 5)
        assert call(None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
        assert call(ok, model=None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
        assert call(ok, init=None) == L.ERR_ARG and b"null init_bin" in lib.emgpu_last_error()
        assert call(ok, out_i=None, out_t=None) == L.ERR_ARG and b"both counts arrays" in lib.emgpu_last_error()
        assert call(ok, dyn=None) == L.ERR_ARG and b"null dyn_bin" in lib.emgpu_last_error()
        assert call(native.score_params(-1, 5)) == L.ERR_ARG and b"n < 0" in lib.emgpu_last_error()
        assert call(native.score_params(64, 0)) == L.ERR_ARG and b"sample_time" in lib.emgpu_last_error()
        assert call(native.score_params(64, 65536)) == L.ERR_ARG and b"sample_time" in lib.emgpu_last_error()
        assert call(native.score_params(64, 5, transition_mode=2)) == L.ERR_ARG and b"transition_mode" in lib.emgpu_last_error()
        assert call(native.score_params(64, 5, ld=100, col_offset=37)) == L.ERR_ARG and b"col_offset + n exceeds ld" in lib.emgpu_last_error()
        assert call(native.score_params(64, 5, ld=100, col_offset=-1)) == L.ERR_ARG and b"col_offset" in lib.emgpu_last_error()
        # nothing left to object to but the missing context: one network alone, no dyn_bin where no transition is counted
        assert call(ok) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(ok, out_t=None) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(ok, out_i=None) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(ok, dyn=None, out_t=None) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(native.score_params(64, 1), dyn=None) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
    assert not ci.any() and not ct.any()


def test_the_counting_surface_exists(model_dir):
    for s in ("emgpu_count_layout", "emgpu_count_dbn_device", "emgpu_count_dbn_host"):
        assert s in L.SYMBOLS and hasattr(L.lib(), s)
    for f in ("count_dbn_device", "count_dbn_host", "sample_count_host", "split_counts"):
        assert callable(getattr(native, f))
    assert callable(E.EncounterModel.count) and callable(native.NativeModel.count_layout)
    nm = native.NativeModel.load_txt(em_io.materialize_model("glider_v1", model_dir))
    with pytest.raises(ValueError):            # a trace of another model's shape never reaches the library
        native.count_dbn_host(None, nm, np.ones((5, nm.n_initial + 1), np.uint8), None, 1)
    with pytest.raises(ValueError):            # nor does a counts= pair of another model's layout
        native.count_dbn_host(None, nm, np.ones((5, nm.n_initial), np.uint8), None, 1, counts=(np.zeros(3, np.uint64), np.zeros(3, np.uint64)))
