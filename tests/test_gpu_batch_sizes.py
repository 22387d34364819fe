"""-m gpu: the support kernels that run after the sampler, at the batch sizes where their scans take the multi-block path.

k_pack_scan (the host path's event packing) and k_scan_rejected (the compaction of the .track rounds) scan per-workgroup counts with
ONE workgroup of 1 024 threads, thread t owning workgroups [t * per, t * per + per) with per = ceil(nb / 1024), nb = ceil(n / 256).
Up to n = 262 144 every thread owns one workgroup; above it the loops run more than once and the last threads' ranges are ragged or
empty.  Every test here asserts, from host_stats() or from its own arithmetic, that it reached the case it names.
References, strongest first: the CPU oracle on windows where the arithmetic changes; the same sampler without the support kernel
(emgpu_sample_dbn_device's event lists are the sampler's own, before any packing); the same call at a size below the threshold
(results depend only on the global index)."""
import ctypes as C
import gc

import numpy as np
import pytest

import oracle as O
import em_model_manned_bayes_amd as E
from em_model_manned_bayes_amd import native, _lib as L
from util import load_pair, uncor_indices, assert_uncor_parity, assert_parting_only_on_a_threshold

pytestmark = pytest.mark.gpu

ONE_PASS = 262_144                           # the largest n whose scan gives every thread one workgroup


def scan_shape(n):
    """(nb, per, last): workgroups of 256, workgroups per scan thread, the last scan thread that owns any."""
    nb = -(-n // 256)
    per = -(-nb // 1024)
    return nb, per, (nb - 1) // per


def scan_windows(n, m):
    """Starts of m-list windows where the scan's arithmetic changes: the first list of scan threads 1, 2, the middle one, the last two
    (the last one's range is ragged when per does not divide nb), around 262 144, and the end of the batch."""
    nb, per, last = scan_shape(n)
    starts = [256 * per * t for t in sorted({1, 2, last // 2, last - 1, last})] + [ONE_PASS - m // 2, n - m]
    return sorted({min(max(s, 0), n - m) for s in starts})


@pytest.fixture(scope="module")
def ctx():
    """A context on torch's stream of cuda:0: the device-resident calls write into torch buffers in stream order."""
    import torch
    c = native.Context(0, stream=torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
    yield c
    c.trim()


@pytest.fixture(scope="module")
def terminal_dir(tmp_path_factory):
    from em_model_manned_bayes_amd import synthetic
    return synthetic.write_terminal_directory(str(tmp_path_factory.mktemp("terminal")))


@pytest.fixture(autouse=True)
def _release(ctx):
    """The large buffers of one test are gone before the next: the host arrays, torch's cached blocks and the library's scratch."""
    yield
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    ctx.trim()


def host_call(ctx, nm, n, T, seed, first, idx, cap=0, dense=False, pinned=False):
    """emgpu_sample_dbn_host into arrays of the library's layout (init_* [n_i, n], dyn_bin [G4, n_d, n], dyn_val [G4, n_d, n, 4],
    events [n, cap] as u64 rows); pageable arrays are zeroed, pinned ones come from the pool as they are."""
    ni, nd, G4 = nm.n_initial, nm.n_dyn, (T + 3) // 4
    empty = ctx.pinned_empty if pinned else (lambda shape, dt: np.zeros(shape, dt))
    r = {"init_bin": empty((ni, n), np.uint8), "init_val": empty((ni, n), np.float32), "attempts": empty((n,), np.int32)}
    if dense:
        r["dyn_bin"], r["dyn_val"] = empty((G4, nd, n), np.uint32), empty((G4, nd, n, 4), np.float32)
    if cap:
        r["ev_count"], r["events"] = empty((n,), np.uint32), empty((n, cap), np.uint64)
    p, _keep = native.make_params(n, T, seed, first_index=first, event_cap=cap, **idx)
    o = L.SampleOut()
    for k, a in r.items():
        setattr(o, k, a.ctypes.data)
    L.check(L.lib().emgpu_sample_dbn_host(ctx._h, nm._h, C.byref(p), C.byref(o)))
    r["host_stats"] = ctx.host_stats()
    return r


def device_call(ctx, nm, n, T, seed, first, idx, cap=0, dense=False):
    """The same outputs from emgpu_sample_dbn_device into torch buffers (ld = n), copied back: the sampler's own event lists, unpacked."""
    import torch
    dev = torch.device("cuda", 0)
    ni, nd, G4 = nm.n_initial, nm.n_dyn, (T + 3) // 4
    t = {"init_bin": torch.empty((ni, n), dtype=torch.uint8, device=dev), "init_val": torch.empty((ni, n), dtype=torch.float32, device=dev),
         "attempts": torch.empty((n,), dtype=torch.int32, device=dev)}
    if dense:
        t["dyn_bin"] = torch.empty((G4, nd, n), dtype=torch.int32, device=dev)
        t["dyn_val"] = torch.empty((G4, nd, n, 4), dtype=torch.float32, device=dev)
    if cap:
        t["ev_count"] = torch.empty((n,), dtype=torch.int32, device=dev)
        t["events"] = torch.empty((n, cap), dtype=torch.int64, device=dev)
    p, _keep = native.make_params(n, T, seed, first_index=first, event_cap=cap, **idx)
    native.sample_dbn_device(ctx, nm, p, ld=n, **{k: v.data_ptr() for k, v in t.items()})
    ctx.sync()
    out = {}
    for k in list(t):
        out[k] = t.pop(k).cpu().numpy()
    for k, dt in (("dyn_bin", np.uint32), ("ev_count", np.uint32), ("events", np.uint64)):
        if k in out:
            out[k] = out[k].view(dt)
    return out


def assert_equal_to_device(got, ref, pageable):
    """Every output of the host path equals the device-resident call's; event lists compared as u64 rows under col < ev_count."""
    for k in ("init_bin", "init_val", "attempts", "dyn_bin", "dyn_val", "ev_count"):
        if k in ref:
            assert np.array_equal(got[k], ref[k]), k
    if "events" in ref:
        ec = ref["ev_count"]
        mask = np.arange(ref["events"].shape[1], dtype=np.uint32)[None, :] < ec[:, None]
        bad = np.flatnonzero((got["events"] != ref["events"]).any(axis=1, where=mask))
        assert bad.size == 0, "%d lists differ from the sampler's own, the first at list %d" % (bad.size, bad[0])
        if pageable:   # the host writes a list's first ev_count rows and nothing else
            assert not got["events"][~mask].any()
        del mask


def window(r, lo, m, T):
    """Lists [lo, lo + m) of a host_call / device_call result, in the shapes assert_uncor_parity reads."""
    sl = slice(lo, lo + m)
    g = {"init_bin": r["init_bin"][:, sl].T, "init_val": r["init_val"][:, sl].T, "attempts": r["attempts"][sl]}
    if "dyn_bin" in r:
        g["dyn_bin"], g["dyn_val"] = native.unpack_dyn_bin(r["dyn_bin"][:, :, sl], T), native.unpack_dyn_val(r["dyn_val"][:, :, sl], T)
    if "events" in r:
        g["events"] = [r["events"][lo + i, : r["ev_count"][lo + i]].view(native.EVENT_DTYPE) for i in range(m)]
    return g


def assert_windows_match_oracle(r, om, T, seed, first, windows, dense, events=True):
    for lo, m in windows:
        ref = O.uncor_sample(om, m, T, seed, mode=O.RNG_PHILOX, first_index=first + lo, want_dense=dense, want_events=events)
        assert_uncor_parity(window(r, lo, m, T), ref, T, check_events=events)


# ---------------------------------------------------------------------------------------------------------------------------------
# A. k_pack_count / k_pack_scan / k_pack_rows on single chunks across the threshold

@pytest.mark.parametrize("name,n,dense,pinned", [
    ("uncor_1200code_v2p1", 262_144, True, True),       # per = 1; the one chunk with ld == c == Cp: one linear copy per dense array
    ("uncor_1200code_v2p1", 262_145, False, False),     # per = 2, nb = 1 025: 511 scan threads idle
    ("uncor_1200code_v2p1", 1_048_577, False, True),    # per = 5, nb = 4 097: thread 819 owns two workgroups, 820.. none
    ("uncor_1200code_v2p1", 1_048_577, True, False),
    ("cor_v1", 262_145, True, True),                    # k_dbn_step2 + events: 44 rows per list on average
])
def test_packed_event_lists_of_one_chunk_across_the_scan_threshold(name, n, dense, pinned, ctx, model_dir, monkeypatch):
    """emgpu_sample_dbn_host as ONE chunk (EMGPU_HOST_CHUNK_MB = 8 GiB) of n lists, T = 120, event_cap = 128 (the longest list of these
    ranges has 113 rows): the packed lists, unpacked by the host, equal the sampler's own lists (emgpu_sample_dbn_device) row for row,
    and the oracle on windows at the scan threads' first lists, around 262 144 and at the end.  Sizes at n = 1 048 577 with dense
    output: host 6.5 GB, device 5 GB."""
    monkeypatch.setenv("EMGPU_HOST_CHUNK_MB", "8192")
    nm, pp, _ = load_pair(name, model_dir)
    idx = uncor_indices(pp)
    T, cap, seed, first = 120, 128, 0xB175, 2**33 + 17
    _, per, last = scan_shape(n)
    assert (per == 1) == (n <= ONE_PASS)
    got = host_call(ctx, nm, n, T, seed, first, idx, cap=cap, dense=dense, pinned=pinned)
    st = got["host_stats"]
    assert st["chunks"] == 1 and st["chunk_n"] == n and st["direct"] == int(pinned), st
    if pinned and dense and n == ONE_PASS:
        assert n % 256 == 0          # ld == c and Cp == round_up(c, 256) == c: the contiguous copy of emgpu_sample_dbn_host
    ref = device_call(ctx, nm, n, T, seed, first, idx, cap=cap, dense=dense)
    assert int(ref["ev_count"].max()) <= cap
    assert st["event_rows"] == int(ref["ev_count"].sum(dtype=np.int64))
    assert_equal_to_device(got, ref, pageable=not pinned)
    del ref
    om = O.OracleModel(pp)
    wins = [(lo, 64) for lo in scan_windows(n, 64)] + [(n - 200, 200)]
    assert any(lo <= 256 * per * last < lo + m for lo, m in wins)      # the last scan thread's first list
    assert_windows_match_oracle(got, om, T, seed, first, wins, dense)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. the host path at its default chunk sizes (no EMGPU_HOST_CHUNK_MB)

def test_events_only_pageable_at_the_default_chunk_size(ctx, model_dir, monkeypatch):
    """n = 2 500 000 lists, T = 6, event_cap = 16 (the longest list of this range has 11 rows), pageable: the 256 MiB target gives three
    equal chunks of about 833 000 lists (per = 4 in every chunk's scan).  The whole range equals the device-resident call; the oracle on the
    chunk boundaries and on the first chunk's scan windows.  Sizes: host 1 GB, device 1 GB."""
    monkeypatch.delenv("EMGPU_HOST_CHUNK_MB", raising=False)
    nm, pp, _ = load_pair("uncor_1200code_v2p1", model_dir)
    idx = uncor_indices(pp)
    n, T, cap, seed, first = 2_500_000, 6, 16, 0xB176, 10**11
    got = host_call(ctx, nm, n, T, seed, first, idx, cap=cap)
    st = got["host_stats"]
    C_ = st["chunk_n"]
    assert st["direct"] == 0 and st["chunks"] >= 3 and C_ > ONE_PASS and st["chunks"] == -(-n // C_), st
    assert scan_shape(C_)[1] > 1
    ref = device_call(ctx, nm, n, T, seed, first, idx, cap=cap)
    assert st["event_rows"] == int(ref["ev_count"].sum(dtype=np.int64))
    assert_equal_to_device(got, ref, pageable=True)
    del ref
    wins = [(0, 64), (n - 64, 64)] + [(k * C_ - 32, 64) for k in range(1, st["chunks"])] + [(lo, 64) for lo in scan_windows(C_, 64)]
    assert_windows_match_oracle(got, O.OracleModel(pp), T, seed, first, wins, dense=False)


def test_dense_pinned_at_the_default_chunk_size(ctx, model_dir, monkeypatch):
    """n = 1 300 000 trajectories, T = 120, dense output into pinned arrays: the 1 GiB target gives three chunks, the last one short
    (pitched copies into the caller's arrays).  The whole range equals the device-resident call; the oracle on the chunk boundaries.
    Sizes: host 5 GB (2.4 GB pinned), device 3.5 GB."""
    monkeypatch.delenv("EMGPU_HOST_CHUNK_MB", raising=False)
    nm, pp, _ = load_pair("uncor_1200code_v2p1", model_dir)
    idx = uncor_indices(pp)
    n, T, seed, first = 1_300_000, 120, 0xB177, 7 * 10**9
    got = host_call(ctx, nm, n, T, seed, first, idx, dense=True, pinned=True)
    st = got["host_stats"]
    C_, k = st["chunk_n"], st["chunks"]
    assert st["direct"] == 1 and k >= 2 and C_ > ONE_PASS and k == -(-n // C_), st
    assert n - (k - 1) * C_ < C_, "the last chunk must be short"
    ref = device_call(ctx, nm, n, T, seed, first, idx, dense=True)
    assert_equal_to_device(got, ref, pageable=False)
    del ref
    wins = [(0, 64), (n - 64, 64)] + [(j * C_ - 32, 64) for j in range(1, k)]
    assert_windows_match_oracle(got, O.OracleModel(pp), T, seed, first, wins, dense=True, events=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. UncorEncounterModel.track rounds past the threshold, through both entry points

@pytest.mark.parametrize("name,rot,n", [("uncor_1200code_v2p1", False, 262_145), ("uncor_1200code_v2p1", False, 1_000_003),
                                        ("uncor_1200only_rotorcraft_v1p2", True, 262_145)])
def test_uncor_track_rounds_past_the_scan_threshold(name, rot, n, ctx, model_dir):
    """emgpu_track_uncor_device into torch buffers prefilled with sentinels (NaN tracks and limits, attempts -7), n lanes, T = 30,
    record_stride = 10: round 1's compaction scans nb = ceil(n / 256) workgroups with per > 1.  No sentinel survives, every lane accepts an
    attempt in [1, max_track_attempts], the host entry point gives the same bits, 1 024-lane windows at scan-thread boundaries equal small
    batches (per = 1) bit for bit, and 1 800 lanes of those windows agree with the oracle (UncorEncounterModel.m:419-471, the rules of
    test_uncor_track_matches_oracle).  Sizes at n = 1 000 003: tracks 2 GB, host 4.5 GB, device 3 GB."""
    import torch
    nm, pp, _ = load_pair(name, model_dir)
    T, stride, seed, first, cap = 30, 10, 0xC0DE, 3 * 10**9 + 11, 200
    S = 10 * T // stride + 1
    assert scan_shape(n)[1] > 1
    kw = dict(first_index=first, is_rotorcraft=rot, record_stride=stride, max_track_attempts=cap)
    dev = torch.device("cuda", 0)
    tracks = torch.full((n, S, 8), float("nan"), dtype=torch.float64, device=dev)
    limits = torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev)
    att = torch.full((n,), -7, dtype=torch.int32, device=dev)
    kern = native.track_uncor_device(ctx, nm, n, T, seed, tracks=tracks.data_ptr(), limits=limits.data_ptr(), attempts=att.data_ptr(), **kw)
    ctx.sync()
    assert "k_uncor_track" in kern
    assert not bool(torch.isnan(tracks).any()) and not bool(torch.isnan(limits).any()), "lanes the rounds never wrote"
    a = att.cpu().numpy()
    assert a.min() >= 1 and a.max() <= cap, "attempts outside [1, %d]: %s" % (cap, np.unique(a[(a < 1) | (a > cap)])[:10])
    assert (a >= 2).sum() > n // 50, "round 1 must reject a good part of the lanes"
    lim = limits.cpu().numpy()
    del limits
    host = native.track_uncor_host(ctx, nm, n, T, seed, **kw)
    assert np.array_equal(host["attempts"], a) and np.array_equal(host["limits"], lim)
    tr = tracks.cpu().numpy()
    del tracks
    assert np.array_equal(host["tracks"], tr)
    del host
    # batch-cut invariance at the scan threads' boundaries of round 1 (lanes [256 per t, 256 per (t + 1)) are thread t's)
    m = 1024
    wins = scan_windows(n, m)
    for lo in wins:
        part = native.track_uncor_host(ctx, nm, m, T, seed, **dict(kw, first_index=first + lo))
        sl = slice(lo, lo + m)
        assert (a[sl] >= 2).any(), "window %d holds no lane rejected in round 1" % lo
        assert np.array_equal(part["attempts"], a[sl]) and np.array_equal(part["limits"], lim[sl]) and np.array_equal(part["tracks"], tr[sl]), lo
    # the oracle: 1 800 lanes, the first ones of each of those windows
    om = O.OracleModel(pp)
    q, retried = 1800 // len(wins), 0
    for lo in wins:
        ref = O.uncor_track(om, q, T, seed, first_index=first + lo, is_rotorcraft=rot, max_track_attempts=cap)
        sl = slice(lo, lo + q)
        same = assert_parting_only_on_a_threshold(a[sl], ref["attempts"], ref["margins"], 1e-9, "trajectory")
        assert same.sum() >= q - 3, "window %d: more threshold coincidences than %d lanes can explain: %d" % (lo, q, (~same).sum())
        assert np.array_equal(lim[sl][same], ref["limits"][same])
        rt = ref["tracks"][:, ::stride]
        np.testing.assert_allclose(tr[sl][same], rt[same], rtol=1e-9, atol=1e-6)
        assert np.array_equal(tr[sl][same][:, 0, :5], rt[same][:, 0, :5])
        retried += int((ref["attempts"] >= 2).sum())
    assert retried >= 100, retried


# ---------------------------------------------------------------------------------------------------------------------------------
# D. CorTerminalModel.track rounds past the threshold

def test_terminal_track_rounds_past_the_scan_threshold(terminal_dir, ctx):
    """emgpu_track_terminal_host on n = 262 145 encounters (GENERIC / GENERIC on the synthetic tables, 150 attempts, no track buffer):
    round 1's compaction scans 1 025 workgroups (per = 2).  Attempts are in [1, 150] or -1, windows at the scan threads' boundaries equal
    small batches bit for bit (sample, len and meta where an attempt was accepted), and 300 encounters agree with the oracle (the rules
    of test_terminal_track_matches_oracle).  Sizes: host 0.1 GB, device 3 GB."""
    t = E.CorTerminalModel(srcData="terminalradar", parameters_directory=terminal_dir)
    t.acType1, t.acType2 = "GENERIC", "GENERIC"
    n, seed, first, cap = 262_145, 0xF3, 2**36 + 3, 150
    per = scan_shape(n)[1]
    assert per == 2
    d = (t.dynLimits1, t.dynLimits2)
    cum, pitch = [x["maxCumTurn_deg"] for x in d], [x["pitch_deg"] for x in d]
    trajs = [m.native for m in t._traj]

    def run(count, lo):
        return native.track_terminal_host(ctx, t.native, trajs, count, seed, t._dyn_rows(), cum, pitch, first_index=first + lo, max_track_attempts=cap,
                                          allow_cap=True, local_smooth=False, want_traj=False)
    big = run(n, 0)
    assert big["traj"] is None and "k_terminal_filter" in big["kernel"]
    a = big["attempts"]
    assert (((a >= 1) & (a <= cap)) | (a == -1)).all(), np.unique(a[((a < 1) | (a > cap)) & (a != -1)])[:10]
    assert (a >= 2).sum() > n // 10 and (a == -1).any()
    m = 512
    for lo in scan_windows(n, m):
        part = run(m, lo)
        sl = slice(lo, lo + m)
        assert (a[sl] >= 2).any(), "window %d holds no encounter rejected in round 1" % lo
        assert np.array_equal(part["attempts"], a[sl]), lo
        ok = part["attempts"] > 0
        for k in ("sample", "len", "meta"):
            assert np.array_equal(part[k][ok], big[k][sl][ok]), (lo, k)
    gom = O.OracleModel(O.parse_model_txt(t.parameters_filename))
    oms = []
    for x in t._traj:
        pp = O.parse_model_txt(x.parameters_filename)
        oms.append(O.OracleModel(pp, alpha_transition=O.stay_prior_alpha(pp, 1.0)))
    for lo in (256 * per * 1, ONE_PASS // 2, n - 100):          # (the last window holds the last scan thread's list 262 144)
        q = 100
        ref = O.terminal_track(gom, oms, q, seed, t._dyn_rows(), cum, pitch, first_index=first + lo, max_track_attempts=cap, local_smooth=False)
        sl = slice(lo, lo + q)
        same = assert_parting_only_on_a_threshold(a[sl], ref["attempts"], ref["margins"], 2.0 ** -22, "encounter")
        assert same.sum() >= q - 2, "window %d: %d encounters parted" % (lo, (~same).sum())
        ok = same & (ref["attempts"] > 0)
        assert ok.sum() >= q // 5 and (ref["attempts"][ok] > 1).any()
        assert np.array_equal(big["sample"][sl][ok], ref["sample"][ok]) and np.array_equal(big["len"][sl][ok], ref["len"][ok])
        np.testing.assert_allclose(big["meta"][sl][ok], ref["meta"][ok], rtol=1e-5, atol=1e-3)
