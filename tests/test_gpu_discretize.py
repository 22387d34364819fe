"""-m gpu: k_discretize_dbn against the numpy restatement of its definition (discretize_ref.discretize) on the very same arrays.  Bins and
counts are integers and every compare is an IEEE compare of doubles, so every comparison is exact equality.  Values come from
native.sample_dbn_host or are built by hand; each is discretized by emgpu_discretize_dbn_host and by emgpu_discretize_dbn_device, as f32 and
as f64, the device outputs pre-filled with a pattern and followed by guard words that must stay."""
import os
import sys

import numpy as np
import pytest

import count_ref as CR
import discretize_ref as R
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native
from em_model_manned_bayes_amd import encounter_model as E

pytestmark = pytest.mark.gpu

N, SEED = 777, 0xD15C
GUARD, FILL8, FILL32 = 0x5A5A5A5A5A5A5A5A, 0xEE, 0xEEEEEEEE
_paths, _traces = {}, {}


def _model(name, model_dir):
    if name not in _paths:
        _paths[name] = em_io.materialize_model(name, model_dir)
    parms = em_io.em_read(_paths[name])
    return parms["native"], parms, R.info(parms)


def _trace(ctx, name, model_dir, n, T):
    """a sampled trace drawn once and shared (raw layout, read-only): (nm, g, init_val, dyn_val, init_bin, dyn_bin)"""
    key = (name, n, T)
    if key not in _traces:
        nm, parms, g = _model(name, model_dir)
        if nm.n_dyn:
            got = native.sample_dbn_host(ctx, nm, n, T, SEED, raw=True, pinned=False)
            arrs = [got["init_val"].copy(), got["dyn_val"].copy(), got["init_bin"].copy(), got["dyn_bin"].copy()]
        else:
            bins, vals, _ = native.sample_bn_host(ctx, nm, n, SEED, dediscretize=True)
            arrs = [np.ascontiguousarray(vals.T), None, np.ascontiguousarray(bins.T), None]
        for a in arrs:
            if a is not None:
                a.setflags(write=False)
        _traces[key] = (nm, g, *arrs)
    return _traces[key]


def _want(g, iv, dv, n, T, n_fine, wrap=0, col=0):
    """discretize_ref of the window of raw arrays, in the raw layout: (init_bin [ni, n], dyn_bin [G4, nd, n] u32, repeat, change, bad)"""
    G4 = (T + 3) // 4
    uiv = None if iv is None else iv[:, col:col + n].T
    udv = None if dv is None else native.unpack_dyn_val(np.ascontiguousarray(dv[:G4, :, col:col + n]), T)
    ib, db, rep, chg, bad = R.discretize(g, uiv, udv, n_fine, wrap)
    return (None if ib is None else np.ascontiguousarray(ib.T)), (None if db is None else native.pack_dyn_bin(db)), rep, chg, bad


def _device(ctx, nm, iv, dv, n, T, n_fine, wrap=0, ld=0, col=0, sync=True, start=None):
    """emgpu_discretize_dbn_device over device copies of the raw arrays.  The bins go into buffers of the inputs' extent filled with 0xEE, the
    vectors into buffers holding `start` (default zeros); 64 guard bytes / 4 guard words behind each must stay.  Returns (init_bin [ni, ld],
    dyn_bin [G4 of dv, nd, ld], repeat, change, kernel, the error of ctx.sync() or None)."""
    import torch
    dev = torch.device("cuda", 0)
    ni = nm.n_initial
    bufs, ptr = {}, {}
    for name, a in (("iv", iv), ("dv", dv)):
        if a is not None:
            bufs[name] = torch.from_numpy(np.array(a, order="C")).to(dev)
            ptr[name] = bufs[name].data_ptr()
    if iv is not None:
        bufs["ib"] = torch.from_numpy(np.full(iv.size + 64, FILL8, dtype=np.uint8)).to(dev)
    if dv is not None:
        h = np.full(dv[..., 0].size + 16, FILL32, dtype=np.uint32)
        bufs["db"] = torch.from_numpy(h.view(np.int32)).to(dev)
    for k, name in enumerate(("rep", "chg")):
        h = np.full(ni + 4, GUARD, dtype=np.uint64)
        h[:ni] = 0 if start is None else start[k]
        bufs[name] = torch.from_numpy(h.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    vt = L.VALUE_F64 if (iv if iv is not None else dv).dtype == np.float64 else L.VALUE_F32
    p = native.discretize_params(n, T, n_fine, vt, wrap, ld, col)
    native.discretize_dbn_device(ctx, nm, p, ptr.get("iv", 0), ptr.get("dv", 0), bufs["ib"].data_ptr() if iv is not None else 0,
                                 bufs["db"].data_ptr() if dv is not None else 0, bufs["rep"].data_ptr() if n_fine else 0,
                                 bufs["chg"].data_ptr() if n_fine else 0)
    kernel = ctx.last_kernel()
    err = None
    if sync:
        try:
            ctx.sync()
        except L.EmgpuError as e:
            err = e
    torch.cuda.synchronize()
    ib = db = None
    if iv is not None:
        h = bufs["ib"].cpu().numpy()
        assert np.all(h[iv.size:] == FILL8)
        ib = h[:iv.size].reshape(iv.shape).copy()
    if dv is not None:
        h = bufs["db"].cpu().numpy().view(np.uint32)
        assert np.all(h[dv[..., 0].size:] == FILL32)
        db = h[:dv[..., 0].size].reshape(dv.shape[:3]).copy()
    vec = []
    for name in ("rep", "chg"):
        h = bufs[name].cpu().numpy().view(np.uint64)
        assert np.all(h[ni:] == GUARD)
        vec.append(h[:ni].copy())
    return ib, db, vec[0], vec[1], kernel, err


def _check_one(ctx, nm, g, iv, dv, T, n_fine, wrap=0, expect_bad=False, n=None, ld=0, col=0):
    """host and device results of the raw values (one dtype) equal the reference's; the device buffers are untouched outside the window"""
    width = (iv if iv is not None else dv[..., 0]).shape[-1]
    n = width - col if n is None else n
    G4 = (T + 3) // 4
    want_ib, want_db, rep, chg, bad = _want(g, iv, dv, n, T, n_fine, wrap, col)
    assert (bad > 0) == expect_bad
    f64 = (iv if iv is not None else dv).dtype == np.float64
    name = "k_discretize_dbn[f64]" if f64 else "k_discretize_dbn[f32]"
    try:
        host = native.discretize_dbn_host(ctx, nm, iv, None if dv is None else np.ascontiguousarray(dv[:G4]), T, n_fine, wrap, raw=True, n=n,
                                          col_offset=col)
        assert not expect_bad
    except L.EmgpuError as e:
        assert expect_bad and e.code == L.ERR_ARG and "discretize" in str(e)
        host = e.bins
    assert host["kernel"] == name
    if iv is not None:
        full = np.zeros(iv.shape, np.uint8)
        full[:, col:col + n] = want_ib
        assert np.array_equal(host["init_bin"], full)
    if dv is not None:
        full = np.zeros((G4,) + dv.shape[1:3], np.uint32)
        full[:, :, col:col + n] = want_db
        assert np.array_equal(host["dyn_bin"], full)
    assert np.array_equal(host["raw"][0], rep) and np.array_equal(host["raw"][1], chg)
    ib, db, drep, dchg, kernel, err = _device(ctx, nm, iv, dv, n, T, n_fine, wrap, ld, col)
    assert (err is not None) == expect_bad and kernel == name
    if iv is not None:
        full = np.full(iv.shape, FILL8, np.uint8)
        full[:, col:col + n] = want_ib
        assert np.array_equal(ib, full)
    if dv is not None:
        full = np.full(dv.shape[:3], FILL32, np.uint32)
        full[:G4, :, col:col + n] = want_db
        assert np.array_equal(db, full)
    assert np.array_equal(drep, rep) and np.array_equal(dchg, chg)
    return want_ib, want_db, rep, chg


def _check(ctx, nm, g, iv, dv, T, n_fine, **kw):
    """... as f32 and as f64 (an f32 array promoted: the same values, the other kernel instance)"""
    out = None
    for dt in (np.float32, np.float64):
        a = None if iv is None else np.ascontiguousarray(iv, dtype=dt)
        b = None if dv is None else np.ascontiguousarray(dv, dtype=dt)
        if (a is not None and not np.array_equal(a, iv, equal_nan=True)) or (b is not None and not np.array_equal(b, dv, equal_nan=True)):
            assert dt == np.float32              # doubles that are no floats: the f32 run sees the rounded values, and so does its reference
        out = _check_one(ctx, nm, g, a, b, T, n_fine, **kw)
    return out


# ---- 1. sampled traces
@pytest.mark.parametrize("n_fine", [0, 2, 4, 255])
@pytest.mark.parametrize("name", ["uncor_1200code_v2p1", "glider_v1", "cor_v1", "terminal_v3_radar_encounter_model"])
def test_sampled_traces(gpu_ctx, model_dir, name, n_fine):
    T = 61 if name != "terminal_v3_radar_encounter_model" else 1
    nm, g, iv, dv, ib, db = _trace(gpu_ctx, name, model_dir, N, T)
    if dv is None:
        assert nm.n_dyn == 0 and max(g["r"]) == 36
    _, _, rep, chg = _check(gpu_ctx, nm, g, iv, dv, T, n_fine)
    if dv is not None and n_fine:
        for v in g["dvar"]:
            assert int(rep[v]) > 0 and int(chg[v]) > 0
        assert int(rep.sum() + chg.sum()) <= N * (T - 1) * nm.n_dyn
        static = [v for v in range(nm.n_initial) if v not in g["dvar"]]
        assert not rep[static].any() and not chg[static].any()
    else:
        assert not rep.any() and not chg.any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 777])
def test_batch_sizes(gpu_ctx, model_dir, n):
    for name in ("uncor_1200code_v2p1", "cor_v1"):
        nm, g, iv, dv, _, _ = _trace(gpu_ctx, name, model_dir, n, 5)
        _check(gpu_ctx, nm, g, iv, dv, 5, 4)


@pytest.mark.parametrize("T", [1, 2, 4, 5, 61])
@pytest.mark.parametrize("name", ["uncor_1200code_v2p1", "glider_v1"])
def test_sample_times_around_the_packed_word(gpu_ctx, model_dir, name, T):
    nm, g, iv, dv, _, _ = _trace(gpu_ctx, name, model_dir, N, T)
    _check(gpu_ctx, nm, g, iv, dv, T, 2)
    _check(gpu_ctx, nm, g, None, dv, T, 2)                    # either half alone
    _check(gpu_ctx, nm, g, iv, None, T, 0)
    if T < 61:                                                # the first T columns of a longer trace: the later groups are neither read nor written
        _, _, iv2, dv2, _, _ = _trace(gpu_ctx, name, model_dir, N, 61)
        _check_one(gpu_ctx, nm, g, iv2, dv2, T, 4)


# ---- 2. hand-built values
def _special(b, n_fine):
    """every cut point and fine cut of a variable with its f64 neighbours, both ends, infinities, zeros, a denormal"""
    out = [b[0] - 1.0, b[-1], np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324]
    for q in range(b.size):
        out += [np.nextafter(b[q], -np.inf), b[q], np.nextafter(b[q], np.inf)]
    for d in range(1, b.size):
        a, h = b[d - 1], (b[d] - b[d - 1]) / n_fine
        for k in range(1, n_fine):
            c = a + k * h
            out += [np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)]
    return np.array(out, dtype=np.float64)


@pytest.mark.parametrize("name,n_fine", [("glider_v1", 4), ("glider_v1", 7), ("uncor_1200code_v2p1", 4), ("cor_v1", 3)])
def test_hand_built_values(gpu_ctx, model_dir, name, n_fine):
    nm, parms, g = _model(name, model_dir)
    T = 8
    rows = [_special(g["bnd"][v], n_fine) for v in g["dvar"]]
    n = max((r.size + T - 1) // T for r in rows) * 2
    dyn = np.zeros((n, T, nm.n_dyn))
    for k, r in enumerate(rows):
        flat = np.resize(r, n * T)                            # the list, then again: every value also meets every neighbour of the list
        flat[n * T // 2:] = np.resize(r[::-1], n * T - n * T // 2)
        dyn[:, :, k] = flat.reshape(n, T)
    ini = np.zeros((n, nm.n_initial))
    for v in range(nm.n_initial):
        b = g["bnd"][v]
        ini[:, v] = np.resize(_special(b, n_fine), n) if b.size else 1 + np.arange(n) % g["r"][v]
    iv, dv = np.ascontiguousarray(ini.T), native.pack_dyn_val(dyn)
    zb = [g["zero"][v] for v in g["dvar"]]
    assert any(zb)
    for wrap in (0, sum(1 << v for v in g["dvar"])):
        want_ib, want_db, rep, chg = _check(gpu_ctx, nm, g, iv, dv, T, n_fine, wrap=wrap)
        for k, v in enumerate(g["dvar"]):
            seen = np.unique(native.unpack_dyn_bin(want_db, T)[:, :, k])
            assert seen.tolist() == list(range(1, g["r"][v] + (0 if wrap else 1)))       # every bin, no bin 0; the last one only unwrapped
    if name == "glider_v1":                                   # doubles that a float cannot hold decide differently as floats
        a32, _, _, _, _ = _want(g, iv.astype(np.float32), None, n, 1, 0)
        a64, _, _, _, _ = _want(g, iv, None, n, 1, 0)
        assert not np.array_equal(a32, a64)


# ---- 3. bad values and where they lie
def _clean(gpu_ctx, model_dir, n=130, T=6, T_big=12):
    """uncor_1200code_v2p1 (variables 1 and 2 are categorical): a sampled trace of T_big columns, of which T are discretized"""
    nm, g, iv, dv, _, _ = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, n, T_big)
    assert not g["bnd"][0].size and not g["bnd"][1].size and g["bnd"][3].size
    return nm, g, iv.copy(), dv.copy()


PLANTS = {
    "init NaN": ("iv", (3, 7), np.nan, True), "init categorical 0": ("iv", (0, 8), 0.0, True),
    "init categorical r + 1": ("iv", (1, 9), 5.0, True), "init categorical 2.5": ("iv", (0, 129), 2.5, True),
    "column 0": ("dv", (0, 0, 64, 0), np.nan, True), "column 3": ("dv", (0, 1, 65, 3), np.nan, True),
    "column 4": ("dv", (1, 2, 0, 0), np.nan, True), "column T-1": ("dv", (1, 0, 128, 1), np.nan, True),
    "the last word's padding": ("dv", (1, 1, 5, 2), np.nan, False), "behind T of a larger trace": ("dv", (2, 1, 5, 0), np.nan, False),
}


@pytest.mark.parametrize("where", list(PLANTS))
def test_bad_values_and_their_placement(gpu_ctx, model_dir, where):
    T = 6
    nm, g, iv, dv = _clean(gpu_ctx, model_dir)
    clean = _want(g, iv, dv, iv.shape[1], T, 4)
    arr, at, value, reported = PLANTS[where]
    (iv if arr == "iv" else dv)[at] = value
    for a, b in ((iv, dv), (iv.astype(np.float64), dv.astype(np.float64))):
        want = _want(g, a, b, a.shape[1], T, 4)
        assert (want[4] == 1) == reported
        if reported:                          # bin 0 there, and nowhere else; at most two pairs are gone
            assert int((want[0] == 0).sum()) + int((native.unpack_dyn_bin(want[1], T) == 0).sum()) == 1
            lost = int(clean[2].sum() + clean[3].sum()) - int(want[2].sum() + want[3].sum())
            assert 0 <= lost <= 2
        else:
            assert all(np.array_equal(x, y) for x, y in zip(want[:4], clean[:4]))
        gpu_ctx.sync()
        _check_one(gpu_ctx, nm, g, a, b, T, 4, expect_bad=reported)          # _host: now; _device: at its own sync
        gpu_ctx.sync()                                                        # nothing is left of either
        if not reported:
            continue
        ib, db, rep, chg, _, _ = _device(gpu_ctx, nm, a, b, a.shape[1], T, 4, sync=False)
        assert np.array_equal(ib, want[0]) and np.array_equal(db[:2], want[1]) and np.array_equal(rep, want[2]) and np.array_equal(chg, want[3])
        # the device call's report is pending: a host call on clean values is served without an error of its own and leaves it in place
        _, _, iv0, dv0, _, _ = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, 130, 12)
        host = native.discretize_dbn_host(gpu_ctx, nm, iv0, np.ascontiguousarray(dv0[:2]), T, 4, raw=True)
        assert np.array_equal(host["init_bin"], clean[0]) and np.array_equal(host["raw"][1], clean[3])
        with pytest.raises(L.EmgpuError) as ei:
            gpu_ctx.sync()
        assert ei.value.code == L.ERR_ARG and "discretize" in str(ei.value)
        gpu_ctx.sync()                                                        # reported once


# ---- 4. pair edges
def test_pair_edges(gpu_ctx, model_dir):
    nm, parms, g = _model("glider_v1", model_dir)
    T, n_fine = 9, 4
    t = np.arange(T)
    kinds = 6
    n = 5 * kinds
    dyn = np.zeros((n, T, nm.n_dyn))
    expect = np.zeros((nm.n_initial, 2), dtype=np.int64)
    for k, v in enumerate(g["dvar"]):
        b, z = g["bnd"][v], g["zero"][v]
        assert z and g["r"][v] >= 3
        d = 1 if z != 1 else 2                                 # a bin that is not the zero bin
        lo, w = b[d - 1], (b[d] - b[d - 1]) / n_fine
        x0, x1 = lo + 0.5 * w, lo + 2.5 * w                    # fine bins 1 and 3 of bin d
        zlo, zw = b[z - 1], (b[z] - b[z - 1]) / n_fine
        for i in range(n):
            kind = i % kinds
            if kind == 0:
                col = np.full(T, x0); expect[v] += (T - 1, 0)                                  # never changes
            elif kind == 1:
                col = np.where(t % 2 == 0, x0, x1); expect[v] += (0, T - 1)                    # changes every second
            elif kind == 2:
                col = np.where(t >= 4, x1, x0); expect[v] += (T - 2, 1)                        # only across the word boundary 3 -> 4
            elif kind == 3:
                col = np.where(t == T - 1, x1, x0); expect[v] += (T - 2, 1)                    # only at T-1
            elif kind == 4:
                col = np.where(t % 2 == 0, zlo + 0.5 * zw, zlo + 2.5 * zw)                     # a run in the zero bin: nothing
            else:
                col = np.where(t < 5, x0, b[d] + 0.5 * (b[d + 1] - b[d]) / n_fine); expect[v] += (T - 2, 0)   # the coarse bin changes: no pair
            dyn[i, :, k] = col
    iv = np.ascontiguousarray(np.stack([np.full(n, 0.5 * (g["bnd"][v][0] + g["bnd"][v][1])) for v in range(nm.n_initial)]))
    _, _, rep, chg = _check(gpu_ctx, nm, g, iv, native.pack_dyn_val(dyn), T, n_fine)
    assert np.array_equal(rep.astype(np.int64), expect[:, 0]) and np.array_equal(chg.astype(np.int64), expect[:, 1]) and expect[g["dvar"], 1].min() > 0
    # a pair whose first member is bad, and one whose second is: both are out, the pairs around them stay
    dyn[0, 2, 0] = np.nan
    _, want_db, rep2, chg2 = _check(gpu_ctx, nm, g, iv, native.pack_dyn_val(dyn), T, n_fine, expect_bad=True)
    v0 = g["dvar"][0]
    assert int(rep2[v0]) == int(rep[v0]) - 2 and np.array_equal(chg2, chg) and native.unpack_dyn_bin(want_db, T)[0, 2, 0] == 0


# ---- 5. windows and accumulation
def test_ld_and_col_offset_between_poisoned_neighbours(gpu_ctx, model_dir):
    T, LD, COL = 61, 1024, 100
    nm, g, iv, dv, _, _ = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T)
    big_iv = np.full((iv.shape[0], LD), np.nan, dtype=np.float32)                 # NaN neighbours: reading one would be reported
    big_dv = np.full(dv.shape[:2] + (LD, 4), np.nan, dtype=np.float32)
    big_iv[:, COL:COL + N], big_dv[:, :, COL:COL + N] = iv, dv
    got = _check(gpu_ctx, nm, g, big_iv, big_dv, T, 4, n=N, ld=LD, col=COL)       # (untouched outside the window: _check_one)
    want = _want(g, iv, dv, N, T, 4)
    assert all(np.array_equal(a, b) for a, b in zip(got, want[:4]))
    with pytest.raises(L.EmgpuError):                                             # one column further reads a neighbour
        native.discretize_dbn_host(gpu_ctx, nm, big_iv, big_dv, T, 4, raw=True, n=N, col_offset=COL + 1)


def test_calls_accumulate(gpu_ctx, model_dir):
    T = 61
    nm, g, iv, dv, _, _ = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T)
    _, _, rep, chg, _ = _want(g, iv, dv, N, T, 4)
    h = 400
    first = native.discretize_dbn_host(gpu_ctx, nm, iv, dv, T, 4, raw=True, n=h, col_offset=0)
    assert not np.array_equal(first["raw"][0], rep)
    both = native.discretize_dbn_host(gpu_ctx, nm, iv, dv, T, 4, raw=True, n=N - h, col_offset=h, counts=first["raw"])
    assert both["raw"][0] is first["raw"][0]
    assert np.array_equal(both["raw"][0], rep) and np.array_equal(both["raw"][1], chg) and np.array_equal(both["repeat"], rep.astype(np.float64))
    # on the device: into vectors that start with an entry at 2^32 - 3, then once more into the result
    v = g["dvar"][0]
    start = (np.zeros_like(rep), np.zeros_like(chg))
    start[0][v] = start[1][v] = 2 ** 32 - 3
    _, _, r1, c1, _, err = _device(gpu_ctx, nm, iv, dv, N, T, 4, start=start)
    assert err is None and np.array_equal(r1, rep + start[0]) and np.array_equal(c1, chg + start[1])
    assert int(r1[v]) > 2 ** 32 and int(c1[v]) > 2 ** 32
    _, _, r2, c2, _, _ = _device(gpu_ctx, nm, iv, dv, N, T, 4, start=(r1, c1))
    assert np.array_equal(r2, 2 * rep + start[0]) and np.array_equal(c2, 2 * chg + start[1])
    # n_fine = 0: the vectors may be absent and are not touched
    _, _, r3, c3, _, _ = _device(gpu_ctx, nm, iv, dv, N, T, 0, start=(np.full_like(rep, 9), np.full_like(chg, 9)))
    assert np.all(r3 == 9) and np.all(c3 == 9)


def test_many_host_chunks_equal_one(gpu_ctx, model_dir, monkeypatch):
    n, T = 20011, 61
    nm, g, iv, dv, _, _ = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, n, T)
    one = native.discretize_dbn_host(gpu_ctx, nm, iv, dv, T, 4, raw=True)
    assert gpu_ctx.last_launches() == 1
    monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", "1")
    many = native.discretize_dbn_host(gpu_ctx, nm, iv, dv, T, 4, raw=True)
    assert gpu_ctx.last_launches() >= 8
    for k in ("init_bin", "dyn_bin", "repeat", "change"):
        assert np.array_equal(many[k], one[k])
    want = _want(g, iv, dv, n, T, 4)
    assert np.array_equal(one["init_bin"], want[0]) and np.array_equal(one["dyn_bin"], want[1])
    assert np.array_equal(one["raw"][0], want[2]) and np.array_equal(one["raw"][1], want[3])


# ---- 6. composition
@pytest.mark.parametrize("name", ["uncor_1200code_v2p1", "glider_v1"])
def test_discretize_count_host_equals_discretize_then_count(gpu_ctx, model_dir, name):
    T = 61
    nm, g, iv, dv, _, _ = _trace(gpu_ctx, name, model_dir, N, T)
    uiv, udv = iv.T.copy(), native.unpack_dyn_val(dv, T)
    for dt in (np.float32, np.float64):
        got = native.discretize_count_host(gpu_ctx, nm, uiv.astype(dt), udv.astype(dt), n_fine=4)
        bins = native.discretize_dbn_host(gpu_ctx, nm, uiv.astype(dt), udv.astype(dt), T, n_fine=4)
        assert bins["init_bin"].shape == (N, nm.n_initial) and bins["dyn_bin"].shape == (N, T, nm.n_dyn) and bins["dyn_bin"].dtype == np.uint8
        want = native.count_dbn_host(gpu_ctx, nm, bins["init_bin"], bins["dyn_bin"], T)
        assert got["kernel"] == bins["kernel"] and got["count_kernel"] == want["kernel"]
        assert np.array_equal(got["raw"][0], want["raw"][0]) and np.array_equal(got["raw"][1], want["raw"][1])
        assert np.array_equal(got["repeat"], bins["repeat"]) and np.array_equal(got["change"], bins["change"])
        assert int(got["raw"][1].sum()) == N * (T - 1) * nm.n_dyn
    # the class layer: count_values equals count on the discretized bins, and its result sets the tables and the resample rates
    m = E.EncounterModel(_paths[name], idxZeroBoundaries=(1, 2, 3))
    Ni, Nt, rep, chg = m.count_values(uiv, udv, n_fine=4, ctx=gpu_ctx)
    Ni2, Nt2, _, _ = m.count(bins["init_bin"], bins["dyn_bin"], ctx=gpu_ctx)
    assert np.array_equal(CR.flat(Ni), CR.flat(Ni2)) and np.array_equal(CR.flat(Nt), CR.flat(Nt2))
    assert rep.shape == chg.shape == (nm.n_initial, 1) and rep.dtype == chg.dtype == np.float64
    assert np.array_equal(rep[:, 0], bins["repeat"]) and np.array_equal(chg[:, 0], bins["change"])
    with np.errstate(invalid="ignore"):
        m.setParameters(Ni, Nt, rep, chg)
    rates = np.asarray(m.resample_rates).reshape(-1)
    for v in g["dvar"]:
        if v >= 2:
            assert rates[v] == chg[v, 0] / (rep[v, 0] + chg[v, 0]) > 0


# ---- 7. round trip
def test_round_trip_of_the_sampled_bins(gpu_ctx, model_dir):
    """Discretizing the sampled values gives back the sampled bins, but for a cell whose f32 value equals the upper boundary of its sampled
    bin (the one way rounding a + (b - a) u to f32 leaves [a, b) when b is a float: all 36 boundaries of this model are).  At most 1e-4 of the
    cells may be such: a condition, not a measurement.  The CPU oracle's f64 values for this shape and seed, cast to f32 and put through
    discretize_ref, give 0 such cells of 147 630."""
    T = 61
    nm, g, iv, dv, ib, db = _trace(gpu_ctx, "uncor_1200code_v2p1", model_dir, N, T)
    assert all(np.array_equal(b, b.astype(np.float32)) for b in g["bnd"])
    got = native.discretize_dbn_host(gpu_ctx, nm, iv, dv, T, 0, raw=True)
    off_i, off_d = got["init_bin"] != ib, native.unpack_dyn_bin(got["dyn_bin"], T) != native.unpack_dyn_bin(db, T)
    cells = ib.size + N * T * nm.n_dyn
    print("cells off: %d initial, %d dynamic of %d" % (off_i.sum(), off_d.sum(), cells))
    for v in range(nm.n_initial):
        m = off_i[v]
        assert not m.any() or np.array_equal(iv[v][m].astype(np.float64), g["bnd"][v][ib[v][m]])
    vals, sampled = native.unpack_dyn_val(dv, T), native.unpack_dyn_bin(db, T)
    for k, v in enumerate(g["dvar"]):
        m = off_d[:, :, k]
        assert not m.any() or np.array_equal(vals[:, :, k][m].astype(np.float64), g["bnd"][v][sampled[:, :, k][m]])
    assert int(off_i.sum() + off_d.sum()) <= 1e-4 * cells


# ---- 8. rates
def test_rates_agree_with_the_cpu_oracles_sample(gpu_ctx, model_dir):
    """change / (repeat + change) of a dynamic variable estimates rate * (1 - 1 / n_fine): a resampled value is uniform in its bin.  The GPU
    sample's estimate and the estimate from the CPU oracle's own sample (another seed: an independent draw) through discretize_ref differ by
    at most 5 standard errors of the difference of two binomial proportions, sqrt(p1 (1 - p1) / m1 + p2 (1 - p2) / m2), computed here from the
    counts."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import oracle as O
    n, T, n_fine = 20000, 61, 4
    nm, parms, g = _model("uncor_1200code_v2p1", model_dir)
    s = native.sample_dbn_host(gpu_ctx, nm, n, T, 0x2A7E5, raw=True, pinned=False)
    got = native.discretize_dbn_host(gpu_ctx, nm, s["init_val"], s["dyn_val"], T, n_fine, raw=True)
    om = O.OracleModel(O.parse_model_txt(_paths["uncor_1200code_v2p1"]))
    ref = O.uncor_sample(om, n, T, 0x0DDBA11, want_events=False, reject=False)
    _, _, rep, chg, bad = R.discretize(g, ref["init_val"], ref["dense_val"], n_fine)
    assert bad == 0
    rates = np.asarray(parms["resample_rates"]).reshape(-1)
    for v in g["dvar"]:
        m1, m2 = got["repeat"][v] + got["change"][v], float(rep[v] + chg[v])
        p1, p2 = got["change"][v] / m1, float(chg[v]) / m2
        se = np.sqrt(p1 * (1 - p1) / m1 + p2 * (1 - p2) / m2)
        print("variable %d: GPU %.6f of %d pairs, oracle %.6f of %d pairs, rate * 3/4 = %.6f, deviation %.2f standard errors"
              % (v + 1, p1, m1, p2, m2, rates[v] * (1 - 1 / n_fine), abs(p1 - p2) / se))
        assert m1 > 1e5 and m2 > 1e5 and abs(p1 - p2) <= 5 * se
