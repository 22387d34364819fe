"""-m gpu: k_encounter_pose against the numpy restatement of its definition (encounter_ref.encounter) on the very same tracks.

The comparison rule.  Every number is a sum, a product, a quotient or a square root of doubles, the same IEEE operations on both sides (the
device's f64 multiply, add, divide and square root are correctly rounded; nothing is contracted), and the draws are the same Philox words,
so pose and rate are compared BIT FOR BIT (a NaN against a NaN), and flags and weights are integers.  Every call writes into device buffers
pre-filled with a pattern, with guard bytes before and behind each output that must stay."""
import numpy as np
import pytest

import encounter_ref as R
import miss_ref
import pair_cases as PC
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native
from em_model_manned_bayes_amd import encounter_model as E

pytestmark = pytest.mark.gpu

OUTS = (("pose", np.float64, 5), ("rate", np.float64, 1), ("flags", np.uint8, 1), ("weights", np.uint32, 1))
RADIUS, HALF_HEIGHT, SCALE = 6000.0, 800.0, 1.0e9


def _run(a, b, n_a, n_b, n_pairs, seed=7, idx_a=None, idx_b=None, weights_in=None, want=("pose", "rate", "flags", "weights"), first_index=0,
         max_attempts=16, rate_scale=SCALE, stream=None):
    """One call on PLANAR host arrays a [P, 3, ld_a], b [P, 3, ld_b]: the wanted outputs as numpy arrays (the others are passed as NULL)"""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)          # noqa: E731
    d_a, d_b = up(a, np.float64), up(b, np.float64)
    d_ia, d_ib = up(idx_a, np.int64), up(idx_b, np.int64)
    d_w = None if weights_in is None else torch.from_numpy(np.asarray(weights_in, dtype=np.uint32).view(np.int32).copy()).to(dev)
    size = {name: k * n_pairs * np.dtype(dt).itemsize for name, dt, k in OUTS if name in want}
    bufs = PC.guarded(size, dev)
    ptr = lambda t: 0 if t is None else t.data_ptr()          # noqa: E731
    at = lambda name: bufs[name].data_ptr() + PC.GUARD if name in want else 0          # noqa: E731
    p = native.encounter_params(n_pairs, n_a, n_b, a.shape[0], RADIUS, HALF_HEIGHT, seed, first_index, max_attempts, rate_scale,
                                ld_a=a.shape[2], ld_b=b.shape[2])
    torch.cuda.synchronize()
    native.encounter_pose_device(p, ptr(d_a), ptr(d_b), ptr(d_ia), ptr(d_ib), ptr(d_w), at("pose"), at("rate"), at("flags"), at("weights"),
                                 stream=stream)
    torch.cuda.synchronize()
    dts = {name: dt for name, dt, _k in OUTS}
    return {name: raw.view(dts[name]).reshape((5, n_pairs) if name == "pose" else (n_pairs,)) for name, raw in PC.payloads(bufs, size).items()}


_same = lambda got, want, names=("pose", "rate", "flags", "weights"): PC.same(got, want, names)          # noqa: E731


def _check(a, b, n_a, n_b, n_pairs, **kw):
    got = _run(a, b, n_a, n_b, n_pairs, **kw)
    want = R.encounter(a, b, n_a, n_b, n_pairs, RADIUS, HALF_HEIGHT, kw.get("seed", 7), idx_a=kw.get("idx_a"), idx_b=kw.get("idx_b"),
                       weights_in=kw.get("weights_in"), rate_scale=kw.get("rate_scale", SCALE), first_index=kw.get("first_index", 0),
                       max_attempts=kw.get("max_attempts", 16), with_weights="weights" in got)
    _same(got, want, [k for k in got])
    return got, want


# ---- 1. tiles and tails
@pytest.mark.parametrize("P", [2, 3, 9])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 600])
def test_tiles_and_tails(n, P):
    a, b = miss_ref.planar(PC.tracks(n, P, 1), n + 3), miss_ref.planar(PC.tracks(n, P, 2), n + 9)       # ld > n
    got, _ = _check(a, b, n, n, n, seed=n * 16 + P)                                                  # identity
    assert not (got["flags"] & (L.ENC_BAD_INDEX | L.ENC_NO_ENTRY | L.ENC_FALLBACK)).any() and (got["rate"] > 0.0).all()
    own = miss_ref.planar(PC.tracks(1, P, 3), 5)
    _check(own, b, 1, n, n)                                                                          # one ownship
    _check(a, own, n, 1, n)
    rs = np.random.RandomState(n * 64 + P)
    m = n + 17
    _check(a, b, n, n, m, idx_a=rs.randint(0, n, m), idx_b=rs.randint(0, n, m), weights_in=rs.randint(0, 1000, m))   # indices with repeats


def test_a_workgroup_walks_a_second_tile():
    n = 2048 * 256 + 300
    a, b = miss_ref.planar(PC.tracks(n, 2, 4)), miss_ref.planar(PC.tracks(n, 2, 5))
    got, _ = _check(a, b, n, n, n, max_attempts=3)
    end = (got["flags"] & L.ENC_END) != 0
    assert 0.05 < end.mean() < 0.95 and 0 < ((got["flags"] & L.ENC_FALLBACK) != 0).sum() < 0.03 * n      # 0.215^3 = 0.0099, ends once more


# ---- 2. indices
def test_a_bad_index_loads_nothing_and_leaves_its_neighbours_alone():
    n, P = 70, 5
    a, b = miss_ref.planar(PC.tracks(n, P, 6), n + 2), miss_ref.planar(PC.tracks(n, P, 7), n)
    ia, ib = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)[::-1].copy()
    good, _ = _check(a, b, n, n, n, idx_a=ia, idx_b=ib, weights_in=np.full(n, 3))
    ia[[0, 64]], ia[33], ib[5], ib[69] = -1, n, 2**62, -2**63
    bad = np.zeros(n, dtype=bool)
    bad[[0, 64, 33, 5, 69]] = True
    got, _ = _check(a, b, n, n, n, idx_a=ia, idx_b=ib, weights_in=np.full(n, 3))
    assert (got["flags"][bad] == L.ENC_BAD_INDEX).all() and not (got["flags"][~bad] & L.ENC_BAD_INDEX).any()
    assert np.isnan(got["pose"][:, bad]).all() and (got["rate"][bad] == 0.0).all() and (got["weights"][bad] == 0).all()
    for name in ("pose", "rate", "flags", "weights"):
        assert np.array_equal(got[name][..., ~bad], good[name][..., ~bad])


# ---- 3. the rejection loop
def test_one_attempt_and_sixteen():
    n, P = 1000, 2
    a, b = miss_ref.planar(PC.tracks(n, P, 8)), miss_ref.planar(PC.tracks(n, P, 9))
    one, want = _check(a, b, n, n, n, max_attempts=1)
    fell = (one["flags"] & L.ENC_FALLBACK) != 0
    assert fell.any() and np.array_equal(fell, (want["flags"] & R.FALLBACK) != 0)
    heading = fell & ((one["flags"] & L.ENC_END) == 0)                       # a side entry's fallback is the heading's
    assert heading.any() and (one["pose"][0, heading] == 1.0).all() and (one["pose"][1, heading] == 0.0).all()
    full, _ = _check(a, b, n, n, n, max_attempts=16)
    assert not (full["flags"] & L.ENC_FALLBACK).any()
    assert np.array_equal(full["pose"][:, ~fell & ((one["flags"] & L.ENC_END) == 0)], one["pose"][:, ~fell & ((one["flags"] & L.ENC_END) == 0)])
    for k in (2, 3, 15):
        _check(a, b, n, n, n, max_attempts=k)


def test_first_index_names_the_rows_of_a_longer_call():
    n, P, k = 600, 3, 277
    a, b = PC.tracks(n, P, 10), PC.tracks(n, P, 11)
    whole, _ = _check(miss_ref.planar(a), miss_ref.planar(b), n, n, n)
    part, _ = _check(miss_ref.planar(a[k:]), miss_ref.planar(b[k:]), n - k, n - k, n - k, first_index=k)
    for name in ("pose", "rate", "flags", "weights"):
        assert np.array_equal(whole[name][..., k:], part[name], equal_nan=whole[name].dtype == np.float64)
    big = 2**32 - 100                                                        # the index crosses into the counter's second word
    _check(miss_ref.planar(a), miss_ref.planar(b), n, n, n, first_index=big, seed=2**63 + 12345)


# ---- 4. no entry, ends only, NaN
def test_two_aircraft_standing_still_have_no_entry():
    n, P = 130, 2
    a, b = PC.tracks(n, P, 12).copy(), PC.tracks(n, P, 13).copy()
    still = np.zeros(n, dtype=bool)
    still[[0, 63, 64, 129]] = True
    a[still, 1], b[still, 1] = a[still, 0], b[still, 0]
    got, _ = _check(miss_ref.planar(a), miss_ref.planar(b), n, n, n, weights_in=np.full(n, 5))
    assert ((got["flags"] & ~np.uint8(L.ENC_FALLBACK))[still] == L.ENC_NO_ENTRY).all() and not (got["flags"][~still] & L.ENC_NO_ENTRY).any()
    assert np.isnan(got["pose"][2:, still]).all() and np.isfinite(got["pose"][:2, still]).all()
    assert (got["rate"][still] == 0.0).all() and (got["weights"][still] == 0).all()


def test_purely_vertical_relative_motion_enters_through_an_end():
    n, P = 300, 2
    a, b = PC.tracks(n, P, 14).copy(), PC.tracks(n, P, 15).copy()
    a[:, 1, :2], b[:, 1, :2] = a[:, 0, :2], b[:, 0, :2]                      # no horizontal motion at all: g = 0 whatever the heading
    got, _ = _check(miss_ref.planar(a), miss_ref.planar(b), n, n, n)
    wr = (b[:, 1, 2] - b[:, 0, 2]) - (a[:, 1, 2] - a[:, 0, 2])
    assert (wr != 0.0).all() and ((got["flags"] & L.ENC_END) != 0).all() and not (got["flags"] & L.ENC_NO_ENTRY).any()
    dz = (got["pose"][4] + b[:, 0, 2]) - a[:, 0, 2]
    assert np.allclose(np.abs(dz), HALF_HEIGHT, rtol=0, atol=1e-9) and ((dz > 0) == (wr < 0)).all()
    assert np.array_equal(got["rate"], (np.pi * RADIUS) * RADIUS * np.abs(wr))


def test_a_nan_coordinate_in_either_point_is_no_entry():
    n, P = 66, 3
    a, b = PC.tracks(n, P, 16).copy(), PC.tracks(n, P, 17).copy()
    a[1, 0, 0], a[2, 1, 1], b[3, 0, 2], b[65, 1, 0], a[64, 1, 2], b[5, 0, 1] = (np.nan,) * 6
    b[6, 1, 0], a[7, 2, 0] = np.inf, np.nan                                  # an infinite speed; a NaN in point 2, which is not read
    got, _ = _check(miss_ref.planar(a), miss_ref.planar(b), n, n, n)
    hit = np.zeros(n, dtype=bool)
    hit[[1, 2, 3, 65, 64, 5, 6]] = True
    assert ((got["flags"] & L.ENC_NO_ENTRY) != 0).tolist() == hit.tolist()
    assert (got["rate"][hit] == 0.0).all() and np.isnan(got["pose"][2:, hit]).all() and np.isfinite(got["pose"][:, ~hit]).all()


# ---- 5. weights
def test_weights_that_saturate_and_weights_out_alone():
    n, P = 257, 2
    a, b = miss_ref.planar(PC.tracks(n, P, 18)), miss_ref.planar(PC.tracks(n, P, 19))
    plain, want = _check(a, b, n, n, n)                                      # weights_out without weights_in: w = 1
    live = want["rate"] > 0.0
    assert np.array_equal(plain["weights"][live], np.floor(want["rate"][live] / SCALE + 0.5).astype(np.uint32)) and plain["weights"].max() > 1
    w = np.array([0, 1, 2**24 - 1, 2**32 - 1], dtype=np.uint64)[np.random.RandomState(3).randint(0, 4, n)]
    got, _ = _check(a, b, n, n, n, weights_in=w)
    sat = (got["flags"] & L.ENC_SATURATED) != 0
    assert sat.any() and (got["weights"][sat] == 2**32 - 1).all() and (got["weights"][w == 0] == 0).all() and not sat[w <= 1].any()
    _same(got, plain, ("pose", "rate"))
    tiny, _ = _check(a, b, n, n, n, rate_scale=1e-300)                        # every quotient is huge: all clamp
    assert ((tiny["flags"] & L.ENC_SATURATED) != 0).all() and (tiny["weights"] == 2**32 - 1).all()
    none, _ = _check(a, b, n, n, n, rate_scale=1e-300, want=("pose", "rate", "flags"))
    assert not (none["flags"] & L.ENC_SATURATED).any()                       # no weight is formed, so none saturates


# ---- 6. NULL outputs, streams
def test_each_output_alone_and_each_output_left_out():
    n, P = 257, 3
    a, b = miss_ref.planar(PC.tracks(n, P, 20)), miss_ref.planar(PC.tracks(n, P, 21))
    w = np.random.RandomState(4).randint(0, 1000, n)
    full, _ = _check(a, b, n, n, n, weights_in=w)
    assert not (full["flags"] & L.ENC_SATURATED).any()
    names = [name for name, _dt, _k in OUTS]
    for name in names:
        rest = tuple(x for x in names if x != name)
        _same(_run(a, b, n, n, n, weights_in=w if "weights" in rest else None, want=rest), full, rest)
        _same(_run(a, b, n, n, n, weights_in=w if name == "weights" else None, want=(name,)), full, (name,))


def test_a_stream_of_its_own_and_the_helpers():
    import torch
    n, P = 300, 6
    rows_a, rows_b = PC.tracks(n, P, 22), PC.tracks(n, P, 23)
    a, b = miss_ref.planar(rows_a), miss_ref.planar(rows_b)
    want = R.encounter(a, b, n, n, n, RADIUS, HALF_HEIGHT, 7, rate_scale=SCALE)
    side = torch.cuda.Stream()
    _same(_run(a, b, n, n, n, stream=side.cuda_stream), want)
    _same(_run(a, b, n, n, n, stream=0), want)                               # the HIP default stream
    ctx = native.Context(0, stream=side.cuda_stream)
    for kw in ({}, {"ctx": ctx}, {"stream": 0}):
        res = native.encounter_pose(rows_a, rows_b, RADIUS, HALF_HEIGHT, 7, weights=True, rate_scale=SCALE, **kw)
        _same(res, want)
    res = native.encounter_pose(torch.from_numpy(a).cuda(), b, RADIUS, HALF_HEIGHT, 7, layout="planar")
    assert res["weights"] is None
    _same(res, want, ("pose", "rate", "flags"))
    perm = np.random.RandomState(5).permutation(n)
    w = np.random.RandomState(6).randint(0, 2**16, n)
    res = native.encounter_pose(rows_a[:1], rows_b, RADIUS, HALF_HEIGHT, 9, idx_b=perm, weights=w, rate_scale=SCALE, first_index=40, max_attempts=2)
    _same(res, R.encounter(a[:, :, :1], b, 1, n, n, RADIUS, HALF_HEIGHT, 9, idx_b=perm, weights_in=w, rate_scale=SCALE, first_index=40, max_attempts=2))


# ---- 7. the chain: pose -> miss distance, nothing of the pair on the host in between
def test_the_pose_feeds_the_miss_distance_kernel(model_dir):
    import torch
    n, P = 600, 9
    rs = np.random.RandomState(24)

    def straight(seed):
        rs = np.random.RandomState(seed)
        start = np.concatenate([rs.uniform(-2500.0, 2500.0, (n, 1, 2)), rs.uniform(1000.0, 1600.0, (n, 1, 1))], axis=2)
        vel = np.concatenate([rs.uniform(-250.0, 250.0, (n, 1, 2)), rs.uniform(-30.0, 30.0, (n, 1, 1))], axis=2)
        return np.ascontiguousarray(start + vel * np.arange(P)[None, :, None])
    rows_a, rows_b = straight(25), straight(26)
    a, b = miss_ref.planar(rows_a), miss_ref.planar(rows_b)
    w = rs.randint(0, 2**12, n)
    # a cylinder of NMAC size, so that a good part of the entries are NMACs at some second
    radius, half = 500.0, 100.0
    scale = 4.0 * radius * half * 600.0
    enc = R.encounter(a, b, n, n, n, radius, half, 31, weights_in=w, rate_scale=scale)
    want = miss_ref.miss(a, b, n, n, n, pose_b=enc["pose"], weights=enc["weights"])
    assert 0 < want["totals"][1] <= want["totals"][2] and want["totals"][0] == n
    dev = torch.device("cuda", 0)
    d_a, d_b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    d_w = torch.from_numpy(w.astype(np.uint32).view(np.int32)).to(dev)
    pose, w_out = torch.empty((5, n), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    outs = {"hmd": torch.zeros(n, dtype=torch.float64, device=dev), "vmd": torch.zeros(n, dtype=torch.float64, device=dev),
            "t_cpa": torch.zeros(n, dtype=torch.int32, device=dev), "flags": torch.zeros(n, dtype=torch.uint8, device=dev),
            "totals": torch.zeros(8, dtype=torch.int64, device=dev)}
    native.encounter_pose_device(native.encounter_params(n, n, n, P, radius, half, 31, rate_scale=scale), d_a.data_ptr(), d_b.data_ptr(),
                                 weights_in=d_w.data_ptr(), pose=pose.data_ptr(), weights_out=w_out.data_ptr())
    native.miss_distance_device(native.miss_params(n, n, n, P), d_a.data_ptr(), d_b.data_ptr(), 0, 0, pose.data_ptr(), w_out.data_ptr(),
                                **{k: v.data_ptr() for k, v in outs.items()})
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    got["totals"] = got["totals"].view(np.uint64)
    for name in ("hmd", "vmd", "t_cpa", "flags", "totals"):
        g, x = got[name], want[name]
        assert np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g, x.view(np.int64) if x.dtype == np.float64 else x), name
    # the same through the model's method
    path = em_io.materialize_model("uncor_1200code_v2p1", model_dir)
    res = E.UncorEncounterModel(parameters_filename=path).encounter(rows_a, rows_b, radius, half, 31, weights=w, rate_scale=scale)
    names = {"hmd_ft": "hmd", "vmd_ft": "vmd", "t_cpa": "t_cpa", "flags": "flags", "totals": "totals"}
    for k, name in names.items():
        assert np.array_equal(res[k], want[name], equal_nan=res[k].dtype == np.float64), k
    assert np.array_equal(res["rate"], enc["rate"]) and np.array_equal(res["encounter_flags"], enc["flags"]) and np.array_equal(res["weights"], enc["weights"])
