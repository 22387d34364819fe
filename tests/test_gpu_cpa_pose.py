"""-m gpu: k_cpa_pose against the numpy restatement of its definition (cpa_pose_ref.cpa_pose) on the very same tracks.

The comparison rule is test_gpu_encounter's.  Every number is a sum, a product, a quotient or a square root of doubles, the same IEEE
operations on both sides (nothing is contracted), the drawn second is integer arithmetic on the same Philox word, so pose and rate are
compared BIT FOR BIT (a NaN against a NaN), and t_cpa, flags and weights are integers.  Every call writes into device buffers pre-filled
with a pattern, with guard bytes before and behind each output that must stay."""
import numpy as np
import pytest

import cpa_pose_ref as R
import miss_ref
import miss_seg_ref
import pair_cases as PC
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native
from em_model_manned_bayes_amd import encounter_model as E

pytestmark = pytest.mark.gpu

OUTS = (("pose", np.float64, 5), ("rate", np.float64, 1), ("t_cpa", np.int32, 1), ("flags", np.uint8, 1), ("weights", np.uint32, 1))
NAMES = tuple(name for name, _dt, _k in OUTS)
HM, VM, SCALE = 1000.0, 200.0, 1.0e7


def _run(a, b, n_a, n_b, n_pairs, t_lo, t_hi=None, seed=7, idx_a=None, idx_b=None, weights_in=None, want=NAMES, first_index=0, max_attempts=16,
         rate_scale=SCALE, stream=None):
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
    p = native.cpa_pose_params(n_pairs, n_a, n_b, a.shape[0], HM, VM, seed, t_lo, t_hi, first_index, max_attempts, rate_scale,
                               ld_a=a.shape[2], ld_b=b.shape[2])
    torch.cuda.synchronize()
    native.cpa_pose_device(p, ptr(d_a), ptr(d_b), ptr(d_ia), ptr(d_ib), ptr(d_w), at("pose"), at("rate"), at("t_cpa"), at("flags"), at("weights"),
                           stream=stream)
    torch.cuda.synchronize()
    dts = {name: dt for name, dt, _k in OUTS}
    return {name: raw.view(dts[name]).reshape((5, n_pairs) if name == "pose" else (n_pairs,)) for name, raw in PC.payloads(bufs, size).items()}


_same = lambda got, want, names=NAMES: PC.same(got, want, names)          # noqa: E731


def _check(a, b, n_a, n_b, n_pairs, t_lo, t_hi=None, **kw):
    got = _run(a, b, n_a, n_b, n_pairs, t_lo, t_hi, **kw)
    want = R.cpa_pose(a, b, n_a, n_b, n_pairs, HM, VM, kw.get("seed", 7), t_lo, t_hi, idx_a=kw.get("idx_a"), idx_b=kw.get("idx_b"),
                      weights_in=kw.get("weights_in"), rate_scale=kw.get("rate_scale", SCALE), first_index=kw.get("first_index", 0),
                      max_attempts=kw.get("max_attempts", 16), with_weights="weights" in got)
    _same(got, want, [k for k in got])
    return got, want


# ---- 1. tiles and tails, a fixed second and a drawn one
@pytest.mark.parametrize("P", [2, 3, 9])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 600])
def test_tiles_and_tails(n, P):
    a, b = PC.planar(PC.tracks(n, P, 1), n + 3), PC.planar(PC.tracks(n, P, 2), n + 9)                 # ld > n
    fixed, drawn = (P - 2, None), (0, P - 2)
    for t_lo, t_hi in (fixed, drawn):
        got, _ = _check(a, b, n, n, n, t_lo, t_hi, seed=n * 16 + P)                                  # identity
        assert not got["flags"].any() and (got["rate"] > 0.0).all() and (got["t_cpa"] >= t_lo).all() and (got["t_cpa"] <= P - 2).all()
    assert (got["weights"] == np.floor(got["rate"] / SCALE + 0.5)).all()
    own = PC.planar(PC.tracks(1, P, 3), 5)
    _check(own, b, 1, n, n, *drawn)                                                                  # one ownship
    _check(a, own, n, 1, n, *fixed)
    rs = np.random.RandomState(n * 64 + P)
    m = n + 17
    _check(a, b, n, n, m, *drawn, idx_a=rs.randint(0, n, m), idx_b=rs.randint(0, n, m), weights_in=rs.randint(0, 1000, m))   # repeats


def test_a_workgroup_walks_a_second_tile():
    n = 2048 * 256 + 300
    own, b = PC.planar(PC.tracks(1, 2, 3)), PC.planar(PC.tracks(n, 2, 5))
    got, _ = _check(own, b, 1, n, n, 0, max_attempts=3)
    assert 0 < ((got["flags"] & L.CPA_FALLBACK) != 0).sum() < 0.02 * n                                 # 0.215^3 = 0.0099
    assert ((got["flags"] & ~np.uint8(L.CPA_FALLBACK)) == 0).all()


# ---- 2. the second
def test_a_span_of_one_at_the_last_legal_second_a_span_of_two_and_the_widest_span():
    n, P = 300, 7
    a, b = PC.planar(PC.tracks(n, P, 6), n + 1), PC.planar(PC.tracks(n, P, 7))
    got, _ = _check(a, b, n, n, n, P - 2, P - 2)
    assert (got["t_cpa"] == P - 2).all()
    got, _ = _check(a, b, n, n, n, 3, 4)
    assert sorted(set(got["t_cpa"].tolist())) == [3, 4]
    # 65537 points, t_hi = 65535, two columns: the widest span and the largest row offset
    P, m = 65537, 600
    a, b = PC.planar(PC.tracks(2, P, 8), 3), PC.planar(PC.tracks(2, P, 9))
    rs = np.random.RandomState(10)
    got, _ = _check(a, b, 2, 2, m, 0, P - 2, idx_a=rs.randint(0, 2, m), idx_b=rs.randint(0, 2, m))
    assert got["t_cpa"].min() < 1000 and got["t_cpa"].max() > P - 1000 and len(set(got["t_cpa"].tolist())) > 0.9 * m
    got, _ = _check(a, b, 2, 2, m, P - 2, idx_a=rs.randint(0, 2, m), idx_b=rs.randint(0, 2, m))        # the last row pair of the buffer
    assert (got["t_cpa"] == P - 2).all() and not got["flags"].any()


# ---- 3. indices
def test_a_bad_index_loads_nothing_and_leaves_its_neighbours_alone():
    n, P = 70, 5
    a, b = PC.planar(PC.tracks(n, P, 6), n + 2), PC.planar(PC.tracks(n, P, 7), n)
    ia, ib = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)[::-1].copy()
    good, _ = _check(a, b, n, n, n, 0, 3, idx_a=ia, idx_b=ib, weights_in=np.full(n, 3))
    ia[[0, 64]], ia[33], ib[5], ib[69] = -1, n, 2**62, -2**63
    bad = np.zeros(n, dtype=bool)
    bad[[0, 64, 33, 5, 69]] = True
    got, _ = _check(a, b, n, n, n, 0, 3, idx_a=ia, idx_b=ib, weights_in=np.full(n, 3))
    assert (got["flags"][bad] == L.CPA_BAD_INDEX).all() and not (got["flags"][~bad] & L.CPA_BAD_INDEX).any()
    assert np.isnan(got["pose"][:, bad]).all() and (got["rate"][bad] == 0.0).all() and (got["weights"][bad] == 0).all()
    assert (got["t_cpa"][bad] == -1).all() and (got["t_cpa"][~bad] >= 0).all()
    for name in NAMES:
        assert np.array_equal(got[name][..., ~bad], good[name][..., ~bad])


# ---- 4. the rejection loop, the global index
def test_one_attempt_and_sixteen():
    n, P = 1000, 4
    a, b = PC.planar(PC.tracks(n, P, 8)), PC.planar(PC.tracks(n, P, 9))
    one, want = _check(a, b, n, n, n, 0, 2, max_attempts=1)
    fell = (one["flags"] & L.CPA_FALLBACK) != 0
    assert fell.any() and (one["pose"][0, fell] == 1.0).all() and (one["pose"][1, fell] == 0.0).all()
    full, _ = _check(a, b, n, n, n, 0, 2, max_attempts=16)
    assert not (full["flags"] & L.CPA_FALLBACK).any()
    assert np.array_equal(full["pose"][:, ~fell], one["pose"][:, ~fell]) and np.array_equal(full["t_cpa"], one["t_cpa"])
    for k in (2, 3, 15):
        _check(a, b, n, n, n, 0, 2, max_attempts=k)


def test_first_index_names_the_rows_of_a_longer_call():
    n, P, k = 600, 5, 277
    a, b = PC.tracks(n, P, 10), PC.tracks(n, P, 11)
    whole, _ = _check(PC.planar(a), PC.planar(b), n, n, n, 1, 3)
    part, _ = _check(PC.planar(a[k:]), PC.planar(b[k:]), n - k, n - k, n - k, 1, 3, first_index=k)
    for name in NAMES:
        assert np.array_equal(whole[name][..., k:], part[name], equal_nan=whole[name].dtype == np.float64)
    big = 2**32 - 100                                                        # the index crosses into the counter's second word
    _check(PC.planar(a), PC.planar(b), n, n, n, 1, 3, first_index=big, seed=2**63 + 12345)
    _check(PC.planar(a), PC.planar(b), n, n, n, 1, 3, first_index=2**40 + 5)


# ---- 5. no pass, NaN
def test_two_aircraft_standing_still_do_not_pass():
    n, P = 130, 4
    a, b = PC.tracks(n, P, 12).copy(), PC.tracks(n, P, 13).copy()
    still = np.zeros(n, dtype=bool)
    still[[0, 63, 64, 129]] = True
    a[still, 1:], b[still, 1:] = a[still, :1], b[still, :1]
    got, want = _check(PC.planar(a), PC.planar(b), n, n, n, 0, 2, weights_in=np.full(n, 5))
    assert (got["flags"][still] == L.CPA_NO_PASS).all() and not (got["flags"][~still] & L.CPA_NO_PASS).any()
    assert np.isnan(got["pose"][2:, still]).all() and np.isfinite(got["pose"][:2, still]).all() and (got["t_cpa"][still] >= 0).all()
    assert (got["rate"][still] == 0.0).all() and (got["weights"][still] == 0).all()


def test_a_nan_in_a_point_that_is_read_is_no_pass_and_elsewhere_changes_nothing():
    """The second is fixed at 2, so points 2 and 3 are read.  The rate is formed from the horizontal coordinates alone: a NaN in x or y of
    any of the four points read gives NO_PASS; a NaN in z of point tc gives a NaN oz and no flag, as the definition says."""
    n, P, t = 66, 6, 2
    a, b = PC.tracks(n, P, 16).copy(), PC.tracks(n, P, 17).copy()
    clean, _ = _check(PC.planar(a), PC.planar(b), n, n, n, t)
    a[1, 2, 0], a[2, 3, 1], b[3, 2, 1], b[65, 3, 0], a[64, 3, 0], b[5, 2, 0] = (np.nan,) * 6
    b[6, 3, 0] = np.inf                                                      # an infinite speed
    a[7, 0, 0], a[8, 1, 1], b[9, 4, 0], b[10, 5, 2], a[11, 4, 1] = (np.nan,) * 5                       # points that are not read
    a[12, 2, 2] = np.nan                                                     # z of point tc
    got, _ = _check(PC.planar(a), PC.planar(b), n, n, n, t)
    hit = np.zeros(n, dtype=bool)
    hit[[1, 2, 3, 65, 64, 5, 6]] = True
    assert ((got["flags"] & L.CPA_NO_PASS) != 0).tolist() == hit.tolist()
    assert (got["rate"][hit] == 0.0).all() and np.isnan(got["pose"][2:, hit]).all() and np.isfinite(got["pose"][:2]).all()
    assert np.isnan(got["pose"][4, 12]) and np.isfinite(got["pose"][:4, 12]).all() and got["flags"][12] == 0
    rest = ~hit
    rest[12] = False
    for name in NAMES:
        assert np.array_equal(got[name][..., rest], clean[name][..., rest]), name


# ---- 6. weights
def test_weights_that_saturate_and_weights_out_alone():
    n, P = 257, 3
    a, b = PC.planar(PC.tracks(n, P, 18)), PC.planar(PC.tracks(n, P, 19))
    plain, want = _check(a, b, n, n, n, 0, 1)                                # weights_out without weights_in: w = 1
    assert np.array_equal(plain["weights"], np.floor(want["rate"] / SCALE + 0.5).astype(np.uint32)) and plain["weights"].max() > 1
    w = np.array([0, 1, 2**24 - 1, 2**32 - 1], dtype=np.uint64)[np.random.RandomState(3).randint(0, 4, n)]
    got, _ = _check(a, b, n, n, n, 0, 1, weights_in=w)
    sat = (got["flags"] & L.CPA_SATURATED) != 0
    assert sat.any() and (got["weights"][sat] == 2**32 - 1).all() and (got["weights"][w == 0] == 0).all() and not sat[w <= 1].any()
    _same(got, plain, ("pose", "rate", "t_cpa"))
    tiny, _ = _check(a, b, n, n, n, 0, 1, rate_scale=1e-300)                  # every quotient is huge: all clamp
    assert ((tiny["flags"] & L.CPA_SATURATED) != 0).all() and (tiny["weights"] == 2**32 - 1).all()
    none, _ = _check(a, b, n, n, n, 0, 1, rate_scale=1e-300, want=("pose", "rate", "t_cpa", "flags"))
    assert not (none["flags"] & L.CPA_SATURATED).any()                       # no weight is formed, so none saturates


# ---- 7. NULL outputs, streams
def test_each_output_alone_and_each_output_left_out():
    n, P = 257, 4
    a, b = PC.planar(PC.tracks(n, P, 20)), PC.planar(PC.tracks(n, P, 21))
    w = np.random.RandomState(4).randint(0, 1000, n)
    full, _ = _check(a, b, n, n, n, 0, 2, weights_in=w)
    assert not (full["flags"] & L.CPA_SATURATED).any()
    for name in NAMES:
        rest = tuple(x for x in NAMES if x != name)
        _same(_run(a, b, n, n, n, 0, 2, weights_in=w if "weights" in rest else None, want=rest), full, rest)
        _same(_run(a, b, n, n, n, 0, 2, weights_in=w if name == "weights" else None, want=(name,)), full, (name,))


def test_a_stream_of_its_own_and_the_helpers():
    import torch
    n, P = 300, 6
    rows_a, rows_b = PC.tracks(n, P, 22), PC.tracks(n, P, 23)
    a, b = PC.planar(rows_a), PC.planar(rows_b)
    want = R.cpa_pose(a, b, n, n, n, HM, VM, 7, 1, 4, rate_scale=SCALE)
    side = torch.cuda.Stream()
    _same(_run(a, b, n, n, n, 1, 4, stream=side.cuda_stream), want)
    _same(_run(a, b, n, n, n, 1, 4, stream=0), want)                         # the HIP default stream
    ctx = native.Context(0, stream=side.cuda_stream)
    for kw in ({}, {"ctx": ctx}, {"stream": 0}):
        res = native.cpa_pose(rows_a, rows_b, HM, VM, 7, 1, 4, weights=True, rate_scale=SCALE, **kw)
        assert res["t_cpa"].dtype == np.int32 and res["flags"].dtype == np.uint8 and res["weights"].dtype == np.uint32
        _same(res, want)
    res = native.cpa_pose(torch.from_numpy(a).cuda(), b, HM, VM, 7, 1, 4, layout="planar")
    assert res["weights"] is None
    _same(res, want, ("pose", "rate", "t_cpa", "flags"))
    perm = np.random.RandomState(5).permutation(n)
    w = np.random.RandomState(6).randint(0, 2**16, n)
    res = native.cpa_pose(rows_a[:1], rows_b, HM, VM, 9, 3, idx_b=perm, weights=w, rate_scale=SCALE, first_index=40, max_attempts=2)
    _same(res, R.cpa_pose(a[:, :, :1], b, 1, n, n, HM, VM, 9, 3, idx_b=perm, weights_in=w, rate_scale=SCALE, first_index=40, max_attempts=2))


# ---- 8. the chain: pose -> miss distance, nothing of the pair on the host in between
def test_cpa_miss_and_cpa_miss_segments_and_the_models_method(model_dir, gpu_ctx):
    n, P = 400, 12
    rows_a, rows_b = miss_seg_ref.crossing(n, P, 37)
    a, b = PC.planar(rows_a), PC.planar(rows_b)
    w = np.random.RandomState(37).randint(1, 2**12, n)
    kw = dict(hmd_max_ft=HM, vmd_max_ft=VM, seed=0x37, t_lo=2, t_hi=9)
    placed = R.cpa_pose(a, b, n, n, n, HM, VM, 0x37, 2, 9, weights_in=w, rate_scale=SCALE)
    assert not placed["flags"].any()
    beside = {"rate": placed["rate"], "t_cpa_drawn": placed["t_cpa"], "encounter_flags": placed["flags"], "weights": placed["weights"]}
    want = miss_ref.miss(a, b, n, n, n, pose_b=placed["pose"], weights=placed["weights"])
    assert 0 < want["totals"][1] <= want["totals"][2] and want["totals"][0] == n
    one = native.cpa_miss(rows_a, rows_b, weights=w, rate_scale=SCALE, **kw)
    PC.same({"hmd": one["hmd_ft"], "vmd": one["vmd_ft"], "t_cpa": one["t_cpa"], "flags": one["flags"], "totals": one["totals"]}, want,
            ("hmd", "vmd", "t_cpa", "flags", "totals"))
    PC.same(one, beside, list(beside))
    assert one["totals"][5] == placed["weights"].sum(dtype=np.uint64)
    want_seg = miss_seg_ref.miss_segments(a, b, n, n, n, pose_b=placed["pose"], weights=placed["weights"])
    seg = native.cpa_miss_segments(rows_a, rows_b, weights=w, rate_scale=SCALE, **kw)
    PC.same({"hmd": seg["hmd_ft"], "vmd": seg["vmd_ft"], "t_cpa_s": seg["t_cpa_s"], "flags": seg["flags"], "totals": seg["totals"]}, want_seg,
            ("hmd", "vmd", "t_cpa_s", "flags", "totals"))
    PC.same(seg, beside, list(beside))
    # without weights every pair counts 1 and no weight comes back
    bare = native.cpa_miss(rows_a, rows_b, **kw)
    assert bare["weights"] is None and bare["totals"][5] == n and np.array_equal(bare["hmd_ft"], one["hmd_ft"])
    # the model's method, on the parent's wrappers and on a small .track result
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    PC.same(mdl.encounter_cpa(rows_a, rows_b, HM, VM, 0x37, 2, 9, weights=w, rate_scale=SCALE), one, list(one))
    PC.same(mdl.encounter_cpa(rows_a, rows_b, HM, VM, 0x37, 2, 9, weights=w, rate_scale=SCALE, between=True), seg, list(seg))
    xyz = E.UncorEncounterModel.track_xyz(mdl.track(40, 30, initialSeed=5, ctx=gpu_ctx))
    own, intruders = xyz[:1], xyz[1:]
    assert xyz.shape == (40, 31, 3)
    res = mdl.encounter_cpa(own, intruders, HM, VM, 11, 5, 25, weights=True, rate_scale=SCALE)
    pa, pb = PC.planar(own), PC.planar(intruders)
    placed = R.cpa_pose(pa, pb, 1, 39, 39, HM, VM, 11, 5, 25, rate_scale=SCALE)
    want = miss_ref.miss(pa, pb, 1, 39, 39, pose_b=placed["pose"], weights=placed["weights"])
    PC.same({"hmd": res["hmd_ft"], "vmd": res["vmd_ft"], "t_cpa": res["t_cpa"], "flags": res["flags"], "totals": res["totals"]}, want,
            ("hmd", "vmd", "t_cpa", "flags", "totals"))
    PC.same(res, {"rate": placed["rate"], "t_cpa_drawn": placed["t_cpa"], "encounter_flags": placed["flags"], "weights": placed["weights"]},
            ("rate", "t_cpa_drawn", "encounter_flags", "weights"))
    assert (res["hmd_ft"] <= HM + 1e-6).all()                                # at the drawn second the pair is |l| apart, wherever the tracks turn
