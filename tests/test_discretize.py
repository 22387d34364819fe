"""Discretizing a trace of values, the parts that need no GPU: the numpy restatement discretize_ref against functions.discretize_bayes /
hierarchical_cutpoints / hierarchical_discretize (the line-by-line mirror of the reference's three functions), the argument checks of
emgpu_discretize_dbn_* (made before any device work: there is no context on this box to do any), and the Python surface."""
import ctypes as C

import numpy as np
import pytest

import discretize_ref as R
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, functions, native
from em_model_manned_bayes_amd import encounter_model as E


def _one(b, zero=0):
    """the definition's view of a single dynamic variable with boundaries b"""
    b = np.asarray(b, dtype=np.float64)
    return {"ni": 1, "r": [b.size - 1], "bnd": [b], "zero": [zero], "dvar": [0]}


def _mirror(x, b, n_fine, zero=0, wrap=0):
    b = np.asarray(b, dtype=np.float64)
    fine = functions.hierarchical_cutpoints(b[1:-1], [b[0], b[-1]], n_fine)
    d, rep, chg = functions.hierarchical_discretize(x, b[1:-1], fine, [zero] if zero else None, wrap)
    return np.asarray(d).astype(np.uint8), int(rep), int(chg)


def _ref(x, b, n_fine, zero=0, wrap=0):
    _, d, rep, chg, bad = R.discretize(_one(b, zero), None, np.asarray(x)[None, :, None], n_fine, 1 if wrap else 0)
    assert bad == 0
    return d[0, :, 0], int(rep[0]), int(chg[0])


def test_the_references_own_example():
    """hierarchical_discretize.m:5-8"""
    b = np.concatenate([[60.0], np.arange(80.0, 161.0, 20.0), [180.0]])
    x = np.array([65, 100, 100, 100, 100, 72, 71, 78], dtype=np.float64)
    d, rep, chg = _ref(x, b, 4)
    assert d.tolist() == [1, 3, 3, 3, 3, 1, 1, 1] and (rep, chg) == (4, 1)
    md, mrep, mchg = _mirror(x, b, 4)
    assert md.tolist() == d.tolist() and (mrep, mchg) == (rep, chg)
    assert np.array_equal(R.coarse(x, b, 6)[0], np.asarray(functions.discretize_bayes(x, b[1:-1])).astype(np.uint8))


def _series(b, rs, n=48):
    """a short series that visits every kind of value: inside the bins (with repeats), on the cut points, on fine cuts, outside both ends"""
    lo, hi = b[0], b[-1]
    x = rs.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), size=n)
    x[1::4] = x[0::4][: x[1::4].size] + 1e-3 * (hi - lo) * rs.standard_normal(x[1::4].size)      # near its predecessor: pairs in one bin
    cuts = np.concatenate([b, b[:-1] + (b[1:] - b[:-1]) / 4 * 2])
    x[2::8] = rs.choice(cuts, size=x[2::8].size)
    return x


@pytest.mark.parametrize("name", ["uncor_1200code_v2p1", "glider_v1", "cor_v1"])
def test_ref_equals_the_mirror_on_every_variable(name, model_dir):
    parms = em_io.em_read(em_io.materialize_model(name, model_dir))
    g = R.info(parms)
    rs = np.random.RandomState(len(name))
    seen = 0
    for v in range(g["ni"]):
        b = g["bnd"][v]
        if b.size == 0:
            continue
        assert b.size == g["r"][v] + 1
        for n_fine, as32 in ((2, False), (4, True), (7, False)):
            x = _series(b, rs)
            if as32:
                x = x.astype(np.float32)
            got, want = _ref(x, b, n_fine, g["zero"][v]), _mirror(x, b, n_fine, g["zero"][v])
            assert got[0].tolist() == want[0].tolist() and got[1:] == want[1:], (name, v, n_fine)
            assert got[1] + got[2] > 0
            seen += 1
    assert seen >= 3 * 5
    if name == "glider_v1":                  # boundaries that are no f32 values: a compare in f32 would differ from the f64 one
        assert any((b != b.astype(np.float32)).any() for b in g["bnd"] if b.size)


def test_wrap_and_zero_bin():
    b = np.array([0.0, 90.0, 180.0, 270.0, 360.0, 450.0])        # r = 5: bin 5 is bin 1 again under wrap
    x = np.array([10.0, 370.0, 380.0, 440.0, 100.0, 110.0, 460.0, -5.0])
    plain, wrapped = _ref(x, b, 4), _ref(x, b, 4, wrap=1)
    assert plain[0].tolist() == [1, 5, 5, 5, 2, 2, 5, 1] and wrapped[0].tolist() == [1, 1, 1, 1, 2, 2, 1, 1]
    assert plain[1:] == _mirror(x, b, 4)[1:]
    mw = _mirror(x, b, 4, wrap=1)
    assert wrapped[0].tolist() == mw[0].tolist() and wrapped[1:] == mw[1:]
    assert wrapped[1] + wrapped[2] > plain[1] + plain[2]
    # a run inside the zero bin counts nothing
    z = np.array([100.0, 101.0, 150.0, 200.0, 201.0])
    assert _ref(z, b, 4)[1:] == (2, 1) and _ref(z, b, 4, zero=2)[1:] == (1, 0)
    assert _ref(z, b, 4, zero=2)[1:] == _mirror(z, b, 4, zero=2)[1:]


def test_bad_values_in_the_restatement():
    g = {"ni": 2, "r": [3, 2], "bnd": [np.zeros(0), np.array([0.0, 1.0, 2.0])], "zero": [0, 0], "dvar": [1]}
    iv = np.array([[1.0, 0.5], [0.0, np.nan], [4.0, 1.0], [2.5, np.inf], [3.0, -np.inf]])
    dv = np.array([[[0.5], [np.nan], [0.5], [0.5]]])
    ib, db, rep, chg, bad = R.discretize(g, iv, dv, 2)
    assert ib.tolist() == [[1, 1], [0, 0], [0, 2], [0, 2], [3, 1]] and db[0, :, 0].tolist() == [1, 0, 1, 1]
    assert bad == 5 and int(rep[1]) == 1 and int(chg[1]) == 0 and int(rep[0]) == 0       # only the pair (2, 3); both pairs with the NaN are out


def test_discretize_entry_points_check_their_arguments_before_any_device_work(model_dir):
    nm = native.NativeModel.load_txt(em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    lib = L.lib()
    iv, dv = np.ones((7, 64), np.float32), np.ones((2, 3, 64, 4), np.float32)
    ib, db = np.full((7, 64), 9, np.uint8), np.full((2, 3, 64), 9, np.uint32)
    rep, chg = np.zeros(7, np.uint64), np.zeros(7, np.uint64)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for f in (lib.emgpu_discretize_dbn_device, lib.emgpu_discretize_dbn_host):
        def call(p, model=nm, a=iv, b=dv, c=ib, d=db, e=rep, g=chg):
            return f(None, None if model is None else model._h, None if p is None else C.byref(p), P(a), P(b), P(c), P(d), P(e), P(g))
        ok = native.discretize_params(64, 5, 4)
        assert call(None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
        assert call(ok, model=None) == L.ERR_ARG and b"null" in lib.emgpu_last_error()
        for bad_fine in (1, 256, -1):
            assert call(native.discretize_params(64, 5, bad_fine)) == L.ERR_ARG and b"n_fine" in lib.emgpu_last_error()
        assert call(native.discretize_params(64, 5, 4, value_type=2)) == L.ERR_ARG and b"value_type" in lib.emgpu_last_error()
        assert call(native.discretize_params(64, 5, 4, wrap=[8])) == L.ERR_ARG and b"wrap_mask" in lib.emgpu_last_error()
        for half in ({"a": None}, {"c": None}, {"b": None}, {"d": None}):
            assert call(ok, **half) == L.ERR_ARG and b"pair" in lib.emgpu_last_error()
        assert call(ok, a=None, b=None, c=None, d=None) == L.ERR_ARG and b"nothing to discretize" in lib.emgpu_last_error()
        assert call(ok, e=None) == L.ERR_ARG and b"repeat" in lib.emgpu_last_error()
        assert call(ok, g=None) == L.ERR_ARG and b"repeat" in lib.emgpu_last_error()
        assert call(native.discretize_params(-1, 5)) == L.ERR_ARG and b"n < 0" in lib.emgpu_last_error()
        assert call(native.discretize_params(64, 0)) == L.ERR_ARG and b"sample_time" in lib.emgpu_last_error()
        assert call(native.discretize_params(64, 65536)) == L.ERR_ARG and b"sample_time" in lib.emgpu_last_error()
        assert call(native.discretize_params(64, 5, ld=100, col_offset=37)) == L.ERR_ARG and b"col_offset + n exceeds ld" in lib.emgpu_last_error()
        # nothing left to object to but the missing context
        assert call(ok) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(native.discretize_params(64, 5, 255, value_type=L.VALUE_F64, wrap=[7])) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(native.discretize_params(64, 5, 0), e=None, g=None) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(ok, a=None, c=None) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(ok, b=None, d=None) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
    assert np.all(ib == 9) and np.all(db == 9) and not rep.any() and not chg.any()


def test_the_discretizing_surface(model_dir):
    for s in ("emgpu_discretize_dbn_device", "emgpu_discretize_dbn_host"):
        assert s in L.SYMBOLS and hasattr(L.lib(), s)
    for f in ("discretize_params", "discretize_dbn_device", "discretize_dbn_host", "discretize_count_host", "pack_dyn_val"):
        assert callable(getattr(native, f))
    assert callable(E.EncounterModel.count_values)
    p = native.discretize_params(10, 7, 4, L.VALUE_F64, wrap=[3, 7], ld=16, col_offset=2)
    assert (p.n, p.sample_time, p.n_fine, p.ld, p.col_offset, p.value_type, p.wrap_mask) == (10, 7, 4, 16, 2, 1, 0b1000100)
    assert C.sizeof(L.DiscretizeParams) == 40 and native.wrap_mask(None) == 0 and native.wrap_mask(5) == 5
    # pack_dyn_val is the inverse of unpack_dyn_val, in both dtypes, and keeps the dtype
    for dt in (np.float32, np.float64):
        dv = np.random.RandomState(1).standard_normal((5, 6, 3)).astype(dt)
        raw = native.pack_dyn_val(dv)
        assert raw.shape == (2, 3, 5, 4) and raw.dtype == dt and raw.flags["C_CONTIGUOUS"]
        assert np.array_equal(native.unpack_dyn_val(raw, 6), dv) and not raw[1, :, :, 2:].any()
    nm = native.NativeModel.load_txt(em_io.materialize_model("glider_v1", model_dir))
    with pytest.raises(ValueError):            # values of another model's shape never reach the library
        native.discretize_dbn_host(None, nm, np.ones((5, nm.n_initial + 1), np.float32), None, 1)
    with pytest.raises(ValueError):
        native.discretize_dbn_host(None, nm, np.ones((5, nm.n_initial), np.float32), np.ones((4, 3, nm.n_dyn)), 3)
    with pytest.raises(ValueError):
        native.discretize_dbn_host(None, nm, None, None, 1)
    with pytest.raises(ValueError):            # nor does a counts= pair of another length
        native.discretize_dbn_host(None, nm, np.ones((5, nm.n_initial), np.float32), None, 1, counts=(np.zeros(3, np.uint64), np.zeros(3, np.uint64)))
    # without a context the call itself is refused by the library, after the Python layer has shaped its arrays: f64 in, u8 out
    with pytest.raises(L.EmgpuError) as ei:
        native.discretize_dbn_host(None, nm, np.ones((5, nm.n_initial)), np.ones((5, 3, nm.n_dyn)), 3, n_fine=4)
    assert ei.value.code == L.ERR_ARG and "null ctx" in str(ei.value)
    bins = ei.value.bins
    assert bins["init_bin"].shape == (5, nm.n_initial) and bins["init_bin"].dtype == np.uint8
    assert bins["dyn_bin"].shape == (5, 3, nm.n_dyn) and bins["dyn_bin"].dtype == np.uint8
    assert bins["repeat"].shape == (nm.n_initial,) and bins["repeat"].dtype == np.float64 and bins["raw"][0].dtype == np.uint64
