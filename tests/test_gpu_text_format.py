"""-m gpu: em_sample's text files from rows formatted on the device (emgpu_sample_text_host, emgpu_format_g_host).

The yardstick for every byte is the host code: Python's "%g" % float(np.float32(x)) through legacy._g for single values, the files
em_sample(text="host") writes for whole runs.  No tolerance: the bytes are equal or the test fails."""
import filecmp

import numpy as np
import pytest

from em_model_manned_bayes_amd import _lib as L, em_io, legacy, native
from em_model_manned_bayes_amd.legacy import _g

pytestmark = pytest.mark.gpu


def f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def bits_of(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def assert_formats_like_g(ctx, x, what):
    """format_g(x) == [_g(v) for v in x], string by string; returns (fast, slow): the values that took each path of the formatter."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    got, paths = native.format_g(ctx, x, return_paths=True)
    with np.errstate(invalid="ignore"):      # (signalling NaNs among random patterns)
        want = [_g(v) for v in x.astype(np.float64).tolist()]
    assert len(got) == len(want)
    if got != want:
        bad = [(i, float(x[i]).hex(), got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
        raise AssertionError("%s: %d of %d values differ, the first: %r" % (what, len(bad), len(want), bad[:10]))
    return paths


def neighbours(centres, k=3):
    """the f32 nearest every centre and the k f32 values on either side of it, both signs"""
    b = bits_of(np.asarray(centres, dtype=np.float64).astype(np.float32)).astype(np.int64)
    b = (b[:, None] + np.arange(-k, k + 1)[None, :]).reshape(-1)
    b = b[(b >= 0) & (b < 0x7F800000)]
    return f32(np.concatenate([b, b | 0x80000000]).astype(np.uint32))


def test_specials(gpu_ctx):
    b = [0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000]
    x = f32(b + [v | 0x80000000 for v in b] + [0x7FC00000, 0xFFC00000, 0x7F800001])
    got = native.format_g(gpu_ctx, x)
    with np.errstate(invalid="ignore"):      # (the signalling NaN)
        assert got == [_g(v) for v in x.astype(np.float64).tolist()]
    assert got[:6] == ["0", "1.4013e-45", "1.17549e-38", "1.17549e-38", "3.40282e+38", "Inf"]
    assert got[6:12] == ["-0", "-1.4013e-45", "-1.17549e-38", "-1.17549e-38", "-3.40282e+38", "-Inf"] and got[12:] == ["NaN"] * 3


def test_decade_boundaries_and_notation_switches(gpu_ctx):
    ks = np.arange(-45, 39)
    centres = np.concatenate([10.0 ** ks, 9.999995 * 10.0 ** ks[ks < 38]])
    fast, slow = assert_formats_like_g(gpu_ctx, neighbours(centres), "decade boundaries")
    assert fast > 0 and slow > 0, (fast, slow)
    # where the notation switches: below 1e-4 and from 1e+6 on (six digits that round up into 1e+06 included)
    ks = np.arange(-5, 7)
    centres = np.concatenate([10.0 ** ks, 9.999995 * 10.0 ** ks, 9.99999 * 10.0 ** ks, 1.000001 * 10.0 ** ks])
    x = neighbours(centres, 8)
    assert_formats_like_g(gpu_ctx, x, "notation switches")
    got = native.format_g(gpu_ctx, np.float32([0.0001, 0.00009999999, 0.00009999, 999999.0, 999999.5, 1000000.0, 100000.0, 123456.0, 0.5, 1234567.0]))
    assert got == ["0.0001", "0.0001", "9.999e-05", "999999", "1e+06", "1e+06", "100000", "123456", "0.5", "1.23457e+06"]


TIE_COUNTS = {-10: 1, -9: 3, -8: 12, -7: 58, -6: 288, -5: 1440, -4: 7200, -3: 36000, -2: 180000, -1: 900000, 0: 900000, 1: 235544}


def exact_ties():
    """Every f32 whose exact decimal expansion has seven significant digits ending in 5: N * 10^p, N = 1000005, 1000015 .. 9999995, that 24 bits
    hold.  p < 0: 5^-p must divide N (N / 5^-p / 2^-p is then exact: N < 2^24); p >= 0: N 5^p (odd) must be below 2^24."""
    N = np.arange(1000005, 10000000, 10, dtype=np.int64)
    out = {}
    for p in range(-12, 4):
        if p < 0:
            keep = N[N % 5 ** -p == 0]
            v = (keep // 5 ** -p).astype(np.float64) / 2.0 ** -p
        else:
            keep = N[N * 5 ** p < 2 ** 24]
            v = (keep * 5 ** p).astype(np.float64) * 2.0 ** p
        if keep.size:
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
            out[p] = v.astype(np.float32)
    return out


def test_every_exact_tie_rounds_half_to_even(gpu_ctx):
    ties = exact_ties()
    assert {p: v.size for p, v in ties.items()} == TIE_COUNTS and sum(v.size for v in ties.values()) == 2260546
    fast = slow = 0
    for p, v in sorted(ties.items()):
        f, s = assert_formats_like_g(gpu_ctx, np.concatenate([v, -v]), "ties with p = %d" % p)
        fast, slow = fast + f, slow + s
    # what half to even means here: 1000005 -> 1e+06 (down to the even 100000), 1000015 -> 1.00002e+06 (up to the even 100002)
    assert native.format_g(gpu_ctx, np.float32([1000005.0, 1000015.0, 1000025.0, 100000.5, 100001.5])) == \
        ["1e+06", "1.00002e+06", "1.00002e+06", "100000", "100002"]
    assert fast > 0 and slow == 0, (fast, slow)   # (a tie has at most 24 + 23 bits: none is beyond the 64-bit path)


def test_random_patterns_and_model_ranges(gpu_ctx, model_dir):
    rs = np.random.RandomState(20261016)
    x = f32(rs.randint(0, 2 ** 32, size=2 ** 22, dtype=np.uint64).astype(np.uint32))
    fast, slow = assert_formats_like_g(gpu_ctx, x, "random bit patterns")
    assert fast > 0 and slow > 0, (fast, slow)       # (most exponents of a random pattern are outside 1e-6 .. 2^64)
    # values from the shipped models' boundary ranges: uniform inside every bin of every variable of three models
    edges = []
    for name in ("uncor_1200code_v2p1", "cor_v1", "glider_v1"):
        parms = em_io.em_read(em_io.materialize_model(name, model_dir))
        for b in parms["boundaries"]:
            b = np.asarray(b, dtype=np.float64).reshape(-1)
            if b.size >= 2:
                edges.append(np.stack([b[:-1], b[1:]], axis=1))
    edges = np.concatenate(edges)
    pick = edges[rs.randint(0, edges.shape[0], size=2 ** 20)]
    v = (pick[:, 0] + (pick[:, 1] - pick[:, 0]) * rs.random_sample(2 ** 20)).astype(np.float32)
    assert_formats_like_g(gpu_ctx, v, "values inside the models' bins")


def test_integers_as_ids_and_seconds_print(gpu_ctx):
    x = np.concatenate([np.arange(0, 2001), np.arange(999990, 1000011)]).astype(np.float32)
    assert_formats_like_g(gpu_ctx, x, "integers")
    assert native.format_g(gpu_ctx, np.float32([0, 7, 240, 999999, 1000000, 1000010])) == ["0", "7", "240", "999999", "1e+06", "1.00001e+06"]


def test_format_g_capacity_protocol(gpu_ctx):
    x = np.float32([1.5, -2.25, 1e-30, 3e30])
    want = "".join(_g(v) for v in x.astype(np.float64).tolist())
    with pytest.raises(L.EmgpuError) as ei:
        native.format_g(gpu_ctx, x, cap=len(want) - 1)
    assert ei.value.code == L.ERR_EVENT_CAP and str(len(want)) in str(ei.value)
    assert "".join(native.format_g(gpu_ctx, x, cap=len(want))) == want
    assert native.format_g(gpu_ctx, np.zeros(0, dtype=np.float32)) == []


def test_a_second_pass_continues_the_first(gpu_ctx):
    """emgpu_format_g_host and emgpu_format_f0_host format 2^22 values per pass.  n = 2^22 + 5 is the smallest call with a second pass, which
    starts at a total that is not zero and writes offsets from k0 = 2^22 on: text and offsets are those of two calls, on the first 2^22 values
    and on the last 5, put together.  With a cap that holds the first pass only (exactly, or all but the last byte of the call) the status is
    EMGPU_ERR_EVENT_CAP, the message and offsets[n] name the full total, the first pass's text has arrived and nothing was written behind it.
    Through ctypes: no list of four million strings is built."""
    n1 = 2 ** 22
    n = n1 + 5
    rs = np.random.RandomState(20261018)
    cases = [("emgpu_format_g_host", f32(rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)), 12),
             ("emgpu_format_f0_host", rs.uniform(-1e6, 1e6, n), 20)]     # (inside +-2^63: every value is formatted on the device)
    for name, x, per in cases:
        fn = getattr(L.lib(), name)

        def call(v, cap):
            v = np.ascontiguousarray(v)
            out = np.full(cap + 64, 0xA5, dtype=np.uint8)                # (0xA5: no byte of a number's text)
            offs = np.zeros(v.size + 1, dtype=np.uint64)
            return fn(gpu_ctx._h, native._p(v), v.size, native._p(out), cap, native._p(offs)), out, offs

        rc1, out1, o1 = call(x[:n1], per * n1)
        rc2, out2, o2 = call(x[n1:], per * 5)
        t1, t2 = int(o1[n1]), int(o2[5])
        assert rc1 == 0 and rc2 == 0 and np.all(np.diff(o1.astype(np.int64)) > 0) and np.all(np.diff(o2.astype(np.int64)) > 0), name
        want = np.concatenate([out1[:t1], out2[:t2]])
        want_offs = np.concatenate([o1, o2[1:] + np.uint64(t1)])
        rc, out, o = call(x, per * n)
        assert rc == 0 and int(o[n]) == t1 + t2, (name, rc, int(o[n]), t1, t2)
        assert np.array_equal(o[:n1 + 1], o1) and np.array_equal(o[n1:], o2 + np.uint64(t1)), name
        assert np.array_equal(out[:t1 + t2], want) and np.all(out[t1 + t2:] == 0xA5), name
        for cap in (t1, t1 + t2 - 1):
            rc, out, o = call(x, cap)
            msg = L.lib().emgpu_last_error().decode()
            assert rc == L.ERR_EVENT_CAP and name in msg and str(t1 + t2) in msg, (name, cap, rc, msg)
            assert int(o[n]) == t1 + t2 and np.array_equal(o, want_offs), (name, cap)
            assert np.array_equal(out[:t1], out1[:t1]) and np.all(out[t1:] == 0xA5), (name, cap)


# ------------------------------------------------------------------------------------------------ whole files
def run_both(path, tmp_path, n, T, ctx, tag="", device_kw=None, **kw):
    """em_sample with the host writer and with the device writer: the four file names and the two results"""
    names = [str(tmp_path / ("%s%s_%s.txt" % (tag, w, f))) for w in ("host", "device") for f in ("initial", "transition")]
    host = legacy.em_sample(path, names[0], names[1], num_initial_samples=n, num_transition_samples=T, ctx=ctx, **kw)
    dev = legacy.em_sample(path, names[2], names[3], num_initial_samples=n, num_transition_samples=T, ctx=ctx, text="device", **dict(kw, **(device_kw or {})))
    return names, host, dev


def assert_same_files(names, host, dev):
    assert filecmp.cmp(names[0], names[2], shallow=False), "initial files differ"
    assert filecmp.cmp(names[1], names[3], shallow=False), "transition files differ"
    assert dev[0].dtype == np.float64 and dev[1].dtype == np.float64
    assert np.array_equal(host[0], dev[0], equal_nan=True) and np.array_equal(host[1], dev[1], equal_nan=True)


SHAPES = [(1, 1), (255, 7), (257, 60), (1, 160), (255, 240), (257, 160)]   # every n and every T at least once per model


@pytest.mark.parametrize("n,T", SHAPES)
@pytest.mark.parametrize("name", ["uncor_1200code_v2p1", "uncor_1200only_fwse_v1p2", "cor_v1", "glider_v1"])
def test_device_writer_writes_the_host_writers_files(name, n, T, gpu_ctx, model_dir, tmp_path):
    path = em_io.materialize_model(name, model_dir)
    names, host, dev = run_both(path, tmp_path, n, T, gpu_ctx, rng_seed=1234 + n)
    assert_same_files(names, host, dev)
    nm = native.NativeModel.load_txt(path)
    b = native.text_bound(nm, n, T)
    assert b == (n * (21 + 13 * nm.n_initial), n * T * 13 * (2 + nm.n_dyn))
    hi, ht = open(names[2], "rb").read(), open(names[3], "rb").read()
    assert len(hi) - hi.index(b"\n") - 1 <= b[0] and len(ht) - ht.index(b"\n") - 1 <= b[1]


def body(filename):
    data = open(filename, "rb").read()
    return data[data.index(b"\n") + 1:]


def test_chunks_and_batches(gpu_ctx, model_dir, tmp_path, monkeypatch):
    """n = 20 011, T = 160: a library call in 20 chunks (EMGPU_HOST_CHUNK_MB=1: chunks of 1 024 trajectories), em_sample in three library calls
    (text_batch = 7 000), pinned and pageable buffers -- the same bytes as the host writer's every time."""
    n, T, seed = 20011, 160, 77
    path = em_io.materialize_model("uncor_1200code_v2p1", model_dir)
    monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", "1")
    calls = []
    real = native.sample_text_host
    monkeypatch.setattr(native, "sample_text_host", lambda *a, **k: (calls.append(a[2]), real(*a, **k))[1])
    names, host, dev = run_both(path, tmp_path, n, T, gpu_ctx, rng_seed=seed, device_kw={"text_batch": 7000})
    assert calls == [7000, 7000, 6011]
    assert gpu_ctx.host_stats()["chunks"] == 6 and gpu_ctx.host_stats()["chunk_n"] == 1024        # the last call: 6 011 trajectories
    assert_same_files(names, host, dev)
    nm = native.NativeModel.load_txt(path)
    want_i, want_t = body(names[0]), body(names[1])
    for pinned in (True, False):
        res = real(gpu_ctx, nm, n, T, seed, pinned=pinned, max_attempts=1)
        st = res["host_stats"]
        assert st["chunks"] == 20 and st["chunk_n"] == 1024 and st["direct"] == (1 if pinned else 0), st
        assert st["kernel_ms"] > 0 and st["d2h_ms"] > 0 and st["bytes_d2h"] >= len(want_i) + len(want_t)
        assert res["totals"] == (len(want_i), len(want_t))
        assert res["initial"].tobytes() == want_i, "initial text, pinned=%s" % pinned
        assert res["transition"].tobytes() == want_t, "transition text, pinned=%s" % pinned
        assert np.array_equal(res["init_val"].astype(np.float64), host[0]) and np.array_equal(res["dyn_val"].astype(np.float64), host[1])
        assert native.text_bound(nm, n, T)[0] >= len(want_i) and native.text_bound(nm, n, T)[1] >= len(want_t)


def expected_rows(initial, trace, id_first):
    """the rows of both files as the host writer builds them (legacy.em_sample), for ids from id_first on"""
    n, T = trace.shape[0], trace.shape[1]
    ri = "".join("%d " % (id_first + i) + " ".join(_g(v) for v in initial[i]) + "\n" for i in range(n))
    rt = "".join("%s %s " % (_g(id_first + i), _g(j)) + " ".join(_g(v) for v in trace[i, j]) + "\n" for i in range(n) for j in range(T))
    return ri.encode(), rt.encode()


@pytest.mark.parametrize("id_first", [999990, 2 ** 31 - 40])
def test_ids_beyond_six_digits(id_first, gpu_ctx, model_dir, tmp_path):
    """the transition file prints its ids through %g (exponent notation from id 1 000 000 on, 2.14748e+09 near 2^31), the initial file through %d"""
    n, T = 30, 7
    path = em_io.materialize_model("uncor_1200code_v2p1", model_dir)
    fi, ft = str(tmp_path / "i.txt"), str(tmp_path / "t.txt")
    initial, trace = legacy.em_sample(path, fi, ft, num_initial_samples=n, num_transition_samples=T, ctx=gpu_ctx, rng_seed=5, text="device", id_first=id_first)
    want_i, want_t = expected_rows(initial, trace, id_first)
    assert body(fi) == want_i and body(ft) == want_t
    ids_t = [r.split(b" ")[0] for r in body(ft).split(b"\n")[:-1]][::T]
    ids_i = [r.split(b" ")[0] for r in body(fi).split(b"\n")[:-1]]
    assert ids_i == [b"%d" % (id_first + i) for i in range(n)]
    if id_first == 999990:
        # six digits: 1 000 000 .. 1 000 005 print 1e+06 (1 000 005 is a tie: down to the even digit), 1 000 006 .. 1 000 014 print
        # 1.00001e+06 and 1 000 015 (a tie: up) .. 1 000 019 print 1.00002e+06 -- what "%g" % 1000006.0 gives on the host as well
        assert ids_t[:10] == [b"%d" % (999990 + i) for i in range(10)]
        assert ids_t[10:] == [b"1e+06"] * 6 + [b"1.00001e+06"] * 9 + [b"1.00002e+06"] * 5
        assert ids_t == [_g(id_first + i).encode() for i in range(n)]
    else:
        assert set(ids_t) == {b"2.14748e+09"}
    # the same draws as the run that counts from 1
    again = legacy.em_sample(path, fi, ft, num_initial_samples=n, num_transition_samples=T, ctx=gpu_ctx, rng_seed=5, text="device")
    assert np.array_equal(again[0], initial) and np.array_equal(again[1], trace)


def test_em_samples_other_arguments(gpu_ctx, model_dir, tmp_path):
    path = em_io.materialize_model("uncor_1200code_v2p1", model_dir)
    ni = em_io.em_read(path)["n_initial"]
    variants = [dict(isOverwriteZeroBoundaries=True), dict(start=[2] + [None] * (ni - 1)), dict(prior=1.5), dict(rng_seed=2 ** 32 + 12345)]
    seen = []
    for k, kw in enumerate(variants):
        names, host, dev = run_both(path, tmp_path, 300, 30, gpu_ctx, tag="v%d_" % k, **dict(dict(rng_seed=9), **kw))
        assert_same_files(names, host, dev)
        seen.append(body(names[3]))
        if "start" in kw:
            assert np.all(dev[0][:, 0] == 2)                            # the preset root variable (a categorical one: its value is its bin)
    assert len(set(seen)) == len(seen)                                  # every argument changed what was written


def test_capacity_protocol(gpu_ctx, model_dir):
    path = em_io.materialize_model("cor_v1", model_dir)
    nm = native.NativeModel.load_txt(path)
    n, T, seed = 700, 33, 4242
    one = native.sample_text_host(gpu_ctx, nm, n, T, seed, max_attempts=1)
    ti, tt = one["totals"]
    want_i, want_t = one["initial"].tobytes(), one["transition"].tobytes()
    assert ti == len(want_i) and tt == len(want_t) and want_t.count(b"\n") == n * T and want_i.count(b"\n") == n
    with pytest.raises(L.EmgpuError) as ei:
        native.sample_text_host(gpu_ctx, nm, n, T, seed, max_attempts=1, transition_cap=tt - 1)
    assert ei.value.code == L.ERR_EVENT_CAP and ei.value.totals == (ti, tt)
    with pytest.raises(L.EmgpuError) as ei:
        native.sample_text_host(gpu_ctx, nm, n, T, seed, max_attempts=1, initial_cap=ti - 1, pinned=False)
    assert ei.value.code == L.ERR_EVENT_CAP and ei.value.totals == (ti, tt)
    again = native.sample_text_host(gpu_ctx, nm, n, T, seed, max_attempts=1, initial_cap=ti, transition_cap=tt, want_arrays=False)
    assert again["initial"].tobytes() == want_i and again["transition"].tobytes() == want_t and again["init_val"] is None
    # start grids and index lists are refused, like emgpu_sample_uncor_host refuses them
    with pytest.raises(L.EmgpuError) as ei:
        native.sample_text_host(gpu_ctx, nm, 4, T, seed, indices=np.arange(4, dtype=np.uint64))
    assert ei.value.code == L.ERR_ARG
    with pytest.raises(L.EmgpuError) as ei:
        native.sample_text_host(gpu_ctx, nm, 4, T, seed, id_first=-1)
    assert ei.value.code == L.ERR_ARG
    empty = native.sample_text_host(gpu_ctx, nm, 0, T, seed)
    assert empty["totals"] == (0, 0)


def test_last_kernel_is_the_samplers(gpu_ctx, model_dir, tmp_path):
    for name in ("uncor_1200code_v2p1", "cor_v1"):
        path = em_io.materialize_model(name, model_dir)
        a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
        legacy.em_sample(path, a, b, num_initial_samples=500, num_transition_samples=40, ctx=gpu_ctx)
        host_kernel = gpu_ctx.last_kernel()
        legacy.em_sample(path, a, b, num_initial_samples=500, num_transition_samples=40, ctx=gpu_ctx, text="device")
        assert gpu_ctx.last_kernel() == host_kernel and host_kernel.startswith("k_")


def test_return_arrays_false(gpu_ctx, model_dir, tmp_path):
    path = em_io.materialize_model("glider_v1", model_dir)
    names, host, dev = run_both(path, tmp_path, 1000, 20, gpu_ctx, rng_seed=3, device_kw={"return_arrays": False, "text_batch": 256})
    assert dev == (None, None)
    assert filecmp.cmp(names[0], names[2], shallow=False) and filecmp.cmp(names[1], names[3], shallow=False)
