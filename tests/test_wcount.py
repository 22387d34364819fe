"""Counting a trace with integer weights, the parts that need no GPU: native.quantize_weights against hand-computed answers,
the numpy restatement count_ref.count(..., weights=w) against a triple Python loop and against count_ref through three identities, the argument checks of
emgpu_count_dbn_weighted_* (made before any device work: there is no context on this box to do any), and the Python surface."""
import ctypes as C
import math

import numpy as np
import pytest

import count_ref as R
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native
from em_model_manned_bayes_amd import encounter_model as E

AUTO, PER_STEP = R.AUTO, R.PER_STEP


# ---- 1. quantize_weights
def test_quantize_weights_against_hand_computed_answers():
    half = math.log(0.5)
    assert math.exp(half) == 0.5                                     # the ties below are exact ties
    # top = 3: 1 -> 3, 1/2 -> 1.5 -> 2; -inf and NaN are dead
    w, s = native.quantize_weights([0.0, half, -np.inf, np.nan], bits=2)
    assert w.dtype == np.uint32 and w.tolist() == [3, 2, 0, 0] and s == 0.0 - math.log(3.0)
    # top = 1: 1/2 -> 0.5, a tie that goes to the even neighbour 0 (rounding half up would give 1)
    w, s = native.quantize_weights([0.0, half], bits=1)
    assert w.tolist() == [1, 0] and s == 0.0
    # top = 7: 1/2 -> 3.5 -> 4 (even), 1/4 -> 1.75 -> 2, 1/8 -> 0.875 -> 1, 1/16 -> 0.4375 -> 0
    w, s = native.quantize_weights([0.0, half, 2 * half, 3 * half, 4 * half], bits=3)
    assert w.tolist() == [7, 4, 2, 1, 0] and s == -math.log(7.0)
    # the scale follows the maximum, not the magnitudes: exp(800) alone would overflow, exp(-800) underflow
    w, s = native.quantize_weights([800.0, 799.0, -800.0], bits=24)
    assert w.tolist() == [2 ** 24 - 1, 6171992, 0] and s == 800.0 - math.log(2 ** 24 - 1)      # rint(16777215 / e) = 6171992
    w, s = native.quantize_weights([-801.0, -800.0])
    assert w.tolist() == [6171992, 2 ** 24 - 1] and s == -800.0 - math.log(2 ** 24 - 1)       # bits defaults to 24
    # bits = 32 fills the u32 range exactly
    w, s = native.quantize_weights([0.0, 0.0, half], bits=32)
    assert w.tolist() == [2 ** 32 - 1, 2 ** 32 - 1, 2 ** 31] and s == -math.log(2 ** 32 - 1)      # 2147483647.5 -> 2147483648 (even)
    # keep: the maximum is taken over the kept entries alone
    w, s = native.quantize_weights([10.0, 0.0, half, np.nan], bits=2, keep=[False, True, True, True])
    assert w.tolist() == [0, 3, 2, 0] and s == -math.log(3.0)
    # nothing alive
    for lw, keep in (([-np.inf, np.nan], None), ([1.0, 2.0], [False, False]), ([], None)):
        w, s = native.quantize_weights(lw, keep=keep)
        assert w.dtype == np.uint32 and w.shape == (len(lw),) and not w.any() and s == -np.inf
    for bad in (0, 33, -1):
        with pytest.raises(ValueError):
            native.quantize_weights([0.0], bits=bad)
    with pytest.raises(ValueError):
        native.quantize_weights([0.0, np.inf])
    with pytest.raises(ValueError):
        native.quantize_weights([0.0, np.inf], keep=[True, False])     # +inf is refused wherever it stands
    with pytest.raises(ValueError):
        native.quantize_weights([0.0, 1.0], keep=[True])


# ---- 2. the reference against the definition, one observation at a time
def _hand_model(depend):
    """§21's hand-written model: A (r 2) -> B (r 3) -> C (r 2, parents A and B); B and C are dynamic: B' <- A, B; C' <- B, C (and B' when
    depend)"""
    G_i = np.zeros((3, 3), dtype=bool)
    G_i[0, 1] = G_i[0, 2] = G_i[1, 2] = True
    G_t = np.zeros((5, 5), dtype=bool)
    G_t[[0, 1], 3] = True
    G_t[[1, 2], 4] = True
    G_t[3, 4] = depend
    return {"n_initial": 3, "G_initial": G_i, "r_initial": np.array([2, 3, 2]), "order_initial": np.array([1, 2, 3]), "n_transition": 5,
            "G_transition": G_t, "r_transition": np.array([2, 3, 2, 3, 2]), "temporal_map": np.array([[2, 4], [3, 5]])}


T_HAND = 6


def _hand_trace():
    T = T_HAND
    ib = np.array([[1, 1, 1], [2, 3, 2], [1, 2, 2], [2, 2, 0], [0, 1, 3], [2, 1, 1]])   # 3: C has bin 0; 4: A has bin 0, C bin r + 1
    db = np.zeros((6, T, 2), dtype=np.int64)
    db[0] = [[1, 1]] * T                                                           # never changes
    db[1] = [[1 + t % 3, 1 + t % 2] for t in range(T)]                             # changes every second
    db[2] = [[2, 2]] * (T - 1) + [[3, 1]]                                          # changes at T-1 only
    db[3] = [[1, 1], [1, 2], [4, 2], [2, 2], [2, 1], [2, 1]]                       # B has bin r + 1 at t = 2
    db[4] = [[1, 2], [0, 2], [1, 255], [4, 3], [1, 2], [1, 2]]                     # bins 0, r + 1 and 255
    db[5] = [[3, 2]] * T
    weights = np.array([1, 5, 2 ** 32 - 1, 3, 0, 0], dtype=np.uint32)              # 3: planted and weighted; 4: planted and left out
    return ib, db, weights


@pytest.mark.parametrize("depend,mode", [(False, AUTO), (False, PER_STEP), (True, AUTO)])
def test_wcount_ref_equals_a_triple_loop_on_a_hand_written_model(depend, mode):
    g = R.graph(_hand_model(depend))
    assert g["depend"] == depend
    per_step = depend or mode == PER_STEP
    ib, db, weights = _hand_trace()
    T = T_HAND
    Ni = [np.zeros((2, 1), object), np.zeros((3, 2), object), np.zeros((2, 6), object)]      # Python integers
    Nt = [np.zeros((0, 0), object)] * 3 + [np.zeros((3, 6), object), np.zeros((2, 18 if depend else 6), object)]
    r = [2, 3, 2]
    good = lambda b, rr: 1 <= b <= rr   # noqa: E731
    skipped = 0
    for i in range(len(ib)):
        wt = int(weights[i])
        if wt == 0:
            continue
        a, b, c = (int(x) for x in ib[i])
        for v, (own, parents) in enumerate(((a, []), (b, [(a, 2)]), (c, [(a, 2), (b, 3)]))):
            if not good(own, r[v]) or not all(good(x, rr) for x, rr in parents):
                skipped += 1
                continue
            col, stride = 0, 1
            for x, rr in parents:
                col += stride * (x - 1)
                stride *= rr
            Ni[v][own - 1, col] += wt
        for t in range(1, T):
            for k in range(2):
                own = int(db[i, t, k])
                tp = t - 1 if per_step else 0
                if k == 0:
                    parents = [(a, 2), (int(db[i, tp, 0]), 3)]
                else:
                    parents = [(int(db[i, tp, 0]), 3), (int(db[i, tp, 1]), 2)] + ([(int(db[i, t if per_step else 0, 0]), 3)] if depend else [])
                if not good(own, (3, 2)[k]) or not all(good(x, rr) for x, rr in parents):
                    skipped += 1
                    continue
                col, stride = 0, 1
                for x, rr in parents:
                    col += stride * (x - 1)
                    stride *= rr
                Nt[3 + k][own - 1, col] += wt
    got_i, got_t, got_skipped = R.count(g, ib, db, mode, weights=weights)
    assert got_skipped == skipped and 2 <= skipped <= 6      # trajectory 3's plants only: trajectory 4's are not looked at
    for x, y in zip(got_i + got_t, Ni + Nt):
        assert x.dtype == np.uint64 and x.shape == y.shape and [int(v) for v in x.reshape(-1)] == [int(v) for v in y.reshape(-1)]
    total = sum(int(v) for N in got_i + got_t for v in N.reshape(-1))
    assert total > 2 ** 32 and total < sum(int(x) for x in weights) * (3 + (T - 1) * 2)
    # without trajectory 3 nothing is skipped, although trajectory 4 is full of bad bins
    w2 = weights.copy()
    w2[3] = 0
    assert R.count(g, ib, db, mode, weights=w2)[2] == 0
    # the initial network alone, and T = 1
    for d in (None, db[:, :1]):
        only_i, only_t, _ = R.count(g, ib, d, mode, weights=weights)
        assert all(np.array_equal(x, y) for x, y in zip(only_i, got_i)) and not any(x.any() for x in only_t)


# ---- 3. three identities on the reference alone
@pytest.mark.parametrize("depend,mode", [(False, AUTO), (False, PER_STEP), (True, AUTO)])
def test_wcount_ref_identities(depend, mode):
    g = R.graph(_hand_model(depend))
    rs = np.random.RandomState(25)
    n, T = 40, 7
    ib = np.stack([rs.randint(1, r + 1, size=n) for r in (2, 3, 2)], axis=1)
    db = np.stack([rs.randint(1, r + 1, size=(n, T)) for r in (3, 2)], axis=2)
    ib[3, 1], db[7, 2, 0], db[9, T - 1, 1] = 0, 4, 0              # bad bins take part in all three
    same = lambda x, y: all(np.array_equal(a.astype(np.int64), b) for a, b in zip(x[0] + x[1], y[0] + y[1])) and x[2] == y[2]   # noqa: E731
    # all weights 1: count_ref
    assert same(R.count(g, ib, db, mode, weights=np.ones(n, np.uint32)), R.count(g, ib, db, mode))
    # weights in {0, 1}: count_ref of the subset
    m = rs.randint(0, 2, size=n).astype(np.uint32)
    m[[3, 7]] = (0, 1)
    assert same(R.count(g, ib, db, mode, weights=m), R.count(g, ib[m > 0], db[m > 0], mode))
    # weight k: the trajectory repeated k times
    k = rs.randint(0, 5, size=n).astype(np.uint32)
    k[[3, 7, 9]] = (2, 0, 4)
    rep = np.repeat(np.arange(n), k)
    got, want = R.count(g, ib, db, mode, weights=k), R.count(g, ib[rep], db[rep], mode)
    assert same(got[:2] + (0,), want[:2] + (0,))                  # (a skipped observation is one, whatever its trajectory's weight:
    assert 0 < got[2] < want[2]                                   # the repeated trace skips it k times)


# ---- 4. the entry points' argument checks
def test_weighted_entry_points_check_their_arguments_before_any_device_work(model_dir):
    nm = native.NativeModel.load_txt(em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    lib = L.lib()
    ib, db, wt = np.ones((7, 64), np.uint8), np.ones((2, 3, 64), np.uint32), np.full(64, 3, np.uint32)
    ci, ct = (np.full(int(nm.count_layout(k)[-1]), 0xA5, np.uint64) for k in (0, 1))
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for f in (lib.emgpu_count_dbn_weighted_device, lib.emgpu_count_dbn_weighted_host):
        def call(p, model=nm, init=ib, dyn=db, weights=wt, out_i=ci, out_t=ct, ctx=None):
            return f(ctx, None if model is None else model._h, None if p is None else C.byref(p), None if init is None else P(init),
                     None if dyn is None else P(dyn), None if weights is None else P(weights), None if out_i is None else P(out_i),
                     None if out_t is None else P(out_t))
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
        # the weights: there must be some, even for n = 0
        assert call(ok, weights=None) == L.ERR_ARG and b"null weights" in lib.emgpu_last_error()
        assert call(native.score_params(0, 5), weights=None) == L.ERR_ARG and b"null weights" in lib.emgpu_last_error()
        # one call's bound n * max(1, sample_time - 1) <= 2^32, with stand-in pointers: nothing is read before the check
        over = 2 ** 32 // 4 + 1
        assert call(native.score_params(over, 5)) == L.ERR_ARG and b"2^32" in lib.emgpu_last_error() and b"split the call" in lib.emgpu_last_error()
        assert call(native.score_params(2 ** 32 + 1, 1), dyn=None) == L.ERR_ARG and b"split the call" in lib.emgpu_last_error()
        assert call(native.score_params(2 ** 32 + 1, 2)) == L.ERR_ARG and b"split the call" in lib.emgpu_last_error()
        # nothing left to object to but the missing context: at the bound itself, one network alone, no dyn_bin where nothing transitions
        assert call(native.score_params(over - 1, 5)) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(native.score_params(2 ** 32, 1), dyn=None) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(ok) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(ok, out_t=None) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(ok, out_i=None) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
        assert call(ok, dyn=None, out_t=None) == L.ERR_ARG and lib.emgpu_last_error() == b"null ctx"
    assert np.all(ci == 0xA5) and np.all(ct == 0xA5) and np.all(wt == 3) and np.all(ib == 1) and np.all(db == 1)


# ---- 5. the Python surface
def test_the_weighted_counting_surface(model_dir, monkeypatch):
    for s in ("emgpu_count_dbn_weighted_device", "emgpu_count_dbn_weighted_host"):
        assert s in L.SYMBOLS and hasattr(L.lib(), s)
    for f in ("count_dbn_weighted_device", "count_dbn_weighted_host", "quantize_weights", "reweight_count_host"):
        assert callable(getattr(native, f))
    path = em_io.materialize_model("glider_v1", model_dir)
    nm = native.NativeModel.load_txt(path)
    ib = np.ones((5, nm.n_initial), np.uint8)
    # weights that are no integer array [n] in 0 .. 2^32 - 1 never reach the library (there is no context here to reach it with)
    for bad in (np.ones(5), np.ones(4, np.uint32), np.ones((5, 1), np.uint32), np.array([1, 2, 3, 4, -1]), np.array([1, 2, 3, 4, 2 ** 32]),
                [0.5] * 5, np.ones(5, bool)):
        with pytest.raises(ValueError, match="weights"):
            native.count_dbn_weighted_host(None, nm, ib, None, 1, bad)
    with pytest.raises(ValueError):            # a trace of another model's shape
        native.count_dbn_weighted_host(None, nm, np.ones((5, nm.n_initial + 1), np.uint8), None, 1, np.ones(5, np.uint32))
    with pytest.raises(ValueError):            # a counts= pair of another model's layout
        native.count_dbn_weighted_host(None, nm, ib, None, 1, np.ones(5, np.uint32), counts=(np.zeros(3, np.uint64), np.zeros(3, np.uint64)))
    other = native.NativeModel.load_txt(em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    with pytest.raises(ValueError, match="proposal and target differ"):
        native.reweight_count_host(None, nm, other, 10, 5, 1)
    # EncounterModel.count: weights=None takes the unweighted path with the arguments it always had; weights go to the weighted call
    calls = []
    fake = {"N_initial": "Ni", "N_transition": "Nt"}
    monkeypatch.setattr(native, "count_dbn_host", lambda *a, **k: calls.append(("plain", a, k)) or fake)
    monkeypatch.setattr(native, "count_dbn_weighted_host", lambda *a, **k: calls.append(("weighted", a, k)) or fake)
    m = E.EncounterModel(path, idxZeroBoundaries=(1, 2, 3))
    ctx, db = object(), np.ones((5, 9, nm.n_dyn), np.uint8)
    assert m.count(ib, db, ctx=ctx) == ("Ni", "Nt", None, None)
    assert m.count(ib, db, ctx=ctx, weights=None) == ("Ni", "Nt", None, None)
    assert m.count(ib, ctx=ctx) == ("Ni", "Nt", None, None)
    w = np.arange(5, dtype=np.uint32)
    assert m.count(ib, db, L.TRANSITION_PER_STEP, ctx=ctx, weights=w) == ("Ni", "Nt", None, None)
    assert [c[0] for c in calls] == ["plain", "plain", "plain", "weighted"]
    for kind, a, k in calls[:2]:
        assert a == (ctx, m.native, ib, db, 9, L.TRANSITION_REFERENCE_AUTO) and not k
    assert calls[2][1] == (ctx, m.native, ib, None, 1, L.TRANSITION_REFERENCE_AUTO)
    assert calls[3][1] == (ctx, m.native, ib, db, 9, w, L.TRANSITION_PER_STEP)
