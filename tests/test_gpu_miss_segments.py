"""-m gpu: k_miss_segments against the numpy restatement of its definition (miss_seg_ref.miss_segments) on the very same tracks, and against
k_miss_distance where the two definitions say the same.

The comparison rule is test_gpu_miss's.  Every number is a sum, a product, a quotient or a square root of doubles, the same IEEE operations
on both sides, so hmd, vmd and t_cpa_s are compared BIT FOR BIT (a NaN against a NaN), and flags and totals are integers.  Every call
writes into device buffers pre-filled with a pattern, with guard bytes before and behind each output that must stay."""
import numpy as np
import pytest

import miss_ref
import miss_seg_ref as R
import pair_cases as PC
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import native
from em_model_manned_bayes_amd import encounter_model as E

pytestmark = pytest.mark.gpu

OUTS = (("hmd", np.float64), ("vmd", np.float64), ("t_cpa_s", np.float64), ("flags", np.uint8), ("totals", np.uint64))
ALL = tuple(name for name, _ in OUTS)
NAMES = {"hmd_ft": "hmd", "vmd_ft": "vmd", "t_cpa_s": "t_cpa_s", "flags": "flags", "totals": "totals"}


def _run(a, b, n_a, n_b, n_pairs, idx_a=None, idx_b=None, pose=None, weights=None, want=ALL, totals=None, nmac=(500.0, 100.0), per_second=False):
    """One call on PLANAR host arrays a [P, 3, ld_a], b [P, 3, ld_b]: the wanted outputs as numpy arrays (the others are passed as NULL).
    per_second: k_miss_distance on the same device inputs, its five outputs."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)          # noqa: E731
    d_a, d_b = up(a, np.float64), up(b, np.float64)
    d_ia, d_ib, d_pose = up(idx_a, np.int64), up(idx_b, np.int64), up(pose, np.float64)
    d_w = None if weights is None else torch.from_numpy(np.asarray(weights, dtype=np.uint32).view(np.int32).copy()).to(dev)
    outs = dict(OUTS) if not per_second else {"hmd": np.float64, "vmd": np.float64, "t_cpa": np.int32, "flags": np.uint8, "totals": np.uint64}
    n_tot = 8 if per_second else 10
    want = tuple(outs) if per_second else want
    size = {name: (n_tot if name == "totals" else n_pairs) * np.dtype(outs[name]).itemsize for name in want}
    zero = np.asarray(np.zeros(n_tot) if totals is None else totals, dtype=np.uint64).view(np.uint8)
    bufs = PC.guarded(size, dev, {"totals": zero})
    ptr = lambda t: 0 if t is None else t.data_ptr()          # noqa: E731
    p = native.miss_params(n_pairs, n_a, n_b, a.shape[0], nmac[0], nmac[1], ld_a=a.shape[2], ld_b=b.shape[2])
    call = native.miss_distance_device if per_second else native.miss_segments_device
    call(p, ptr(d_a), ptr(d_b), ptr(d_ia), ptr(d_ib), ptr(d_pose), ptr(d_w), **{name: bufs[name].data_ptr() + PC.GUARD for name in want})
    torch.cuda.synchronize()
    return {name: raw.view(outs[name]) for name, raw in PC.payloads(bufs, size).items()}


def _check(a, b, n_a, n_b, n_pairs, **kw):
    got = _run(a, b, n_a, n_b, n_pairs, **kw)
    nmac = kw.get("nmac", (500.0, 100.0))
    want = R.miss_segments(a, b, n_a, n_b, n_pairs, idx_a=kw.get("idx_a"), idx_b=kw.get("idx_b"), pose_b=kw.get("pose"), weights=kw.get("weights"),
                           nmac_h_ft=nmac[0], nmac_v_ft=nmac[1], totals=kw.get("totals"))
    PC.same(got, want, list(got))
    return got, want


def _against_the_per_second_kernel(seg, a, b, n_a, n_b, n_pairs, **kw):
    """the exact statements that tie k_miss_segments to k_miss_distance on the same inputs"""
    sec = _run(a, b, n_a, n_b, n_pairs, per_second=True, **kw)
    fl, fs = seg["flags"], sec["flags"]
    num = ~np.isnan(sec["hmd"])
    assert (seg["hmd"][num] <= sec["hmd"][num]).all() and np.array_equal(np.isnan(seg["hmd"]), ~num)
    at_point = (fl & L.MISS_CPA_BETWEEN) == 0
    PC.same({k: seg[k][at_point] for k in ("hmd", "vmd")}, {k: sec[k][at_point] for k in ("hmd", "vmd")}, ("hmd", "vmd"))
    assert np.array_equal(seg["t_cpa_s"][at_point], sec["t_cpa"][at_point].astype(np.float64))
    assert np.array_equal(((fl & L.MISS_NMAC_ANY) != 0) & ((fl & L.MISS_NMAC_BETWEEN) == 0), (fs & L.MISS_NMAC_ANY) != 0)
    for bit in (L.MISS_NO_CPA, L.MISS_BAD_INDEX):
        assert np.array_equal(fl & bit, fs & bit)
    assert np.array_equal(seg["totals"][[0, 3, 4, 5]], sec["totals"][[0, 3, 4, 5]])
    if a.shape[0] == 1:
        PC.same(seg, sec, ("hmd", "vmd", "flags"))
        assert np.array_equal(seg["totals"][:8], sec["totals"]) and not seg["totals"][8:].any()


# ---- 1. tiles and tails
@pytest.mark.parametrize("P", [1, 2, 3, 5, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_tiles_and_tails(n, P):
    rows_a, rows_b, pose = R.posed_crossing(n, P, 1)
    a, b = R.planar(rows_a, n + 3), R.planar(rows_b, n + 9)
    got, _ = _check(a, b, n, n, n, pose=pose)                                          # crossing tracks through a random pose
    assert got["totals"][0] == n
    _against_the_per_second_kernel(got, a, b, n, n, n, pose=pose)
    plain_a, plain_b = R.crossing(n, P, 1)
    got, _ = _check(R.planar(plain_a, n + 3), R.planar(plain_b, n), n, n, n)           # without a pose
    _against_the_per_second_kernel(got, R.planar(plain_a, n + 3), R.planar(plain_b, n), n, n, n)
    own = R.planar(rows_a[:1], 5)
    _check(own, b, 1, n, n, pose=pose)                                                 # one ownship
    rs = np.random.RandomState(n * 64 + P)
    m = n + 17
    _check(a, b, n, n, m, idx_a=rs.randint(0, n, m), idx_b=rs.randint(0, n, m), pose=np.ascontiguousarray(pose[:, rs.randint(0, n, m)]))


# ---- 2. a workgroup that walks two tiles
def test_grid_walk():
    n, P = 2048 * 256 + 300, 3
    rows_a, rows_b = R.crossing(1000, P, 1)
    a, b = R.planar(rows_a), R.planar(rows_b)
    rs = np.random.RandomState(2)
    ia, ib = rs.randint(0, 1000, n), np.arange(n, dtype=np.int64) % 1000
    w = rs.randint(0, 2**32, n, dtype=np.uint64)
    got, want = _check(a, b, 1000, 1000, n, idx_a=ia, idx_b=ib, weights=w)
    assert got["totals"][0] == n and got["totals"][8] > 0 and got["totals"][9] > 2**32


# ---- 3. the hand-computed cases
@pytest.mark.parametrize("case", R.HAND, ids=[c[0] for c in R.HAND])
def test_hand_computed(case):
    _, (a, b), nmac, hmd, vmd, t, flags = case
    got, _ = _check(R.planar(a, 3), R.planar(b, 2), 1, 1, 1, nmac=nmac)
    want = {"hmd": np.array([hmd]), "vmd": np.array([vmd]), "t_cpa_s": np.array([t]), "flags": np.array([flags], dtype=np.uint8)}
    PC.same(got, want, ("hmd", "vmd", "t_cpa_s", "flags"))
    # the same case in lane 70 of 130, between crossing pairs
    rows_a, rows_b = (x.copy() for x in R.crossing(130, a.shape[1], 3))
    rows_a[70], rows_b[70] = a[0], b[0]
    got, _ = _check(R.planar(rows_a), R.planar(rows_b), 130, 130, 130, nmac=nmac)
    PC.same({k: v[70:71] for k, v in got.items() if k != "totals"}, want, ("hmd", "vmd", "t_cpa_s", "flags"))


# ---- 4. NaN and inf
def test_nan_and_inf():
    n, P = 300, 9
    rows_a, rows_b, pose = R.posed_crossing(n, P, 4)
    clean_a, clean_b = rows_a, rows_b
    rows_a, rows_b = rows_a.copy(), rows_b.copy()
    rs = np.random.RandomState(4)
    for bad in (np.nan, np.inf, -np.inf):
        for rows in (rows_a, rows_b):
            rows[rs.randint(0, n, 40), rs.randint(0, P, 40), rs.randint(0, 3, 40)] = bad
    rows_a[8], rows_b[8] = clean_a[8], clean_b[8]
    rows_a[7] = np.nan                                   # a pair with no number at all
    rows_b[8, :, 0] = np.inf                             # inf at every second: d = inf is a number, every segment is invalid
    a, b = R.planar(rows_a), R.planar(rows_b)
    got, _ = _check(a, b, n, n, n, pose=pose)
    assert got["flags"][7] == L.MISS_NO_CPA and got["t_cpa_s"][7] == -1.0
    assert got["hmd"][8] == np.inf and got["t_cpa_s"][8] == 0.0 and got["flags"][8] == 0
    _against_the_per_second_kernel(got, a, b, n, n, n, pose=pose)
    _check(a, b, n, n, n)


# ---- 5. bad indices
def test_bad_indices_load_nothing_and_leave_their_neighbours_alone():
    n, P = 70, 5
    rows_a, rows_b, pose = R.posed_crossing(n, P, 5)
    a, b = R.planar(rows_a, n + 2), R.planar(rows_b, n)
    ia, ib = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)
    good, _ = _check(a, b, n, n, n, idx_a=ia, idx_b=ib, pose=pose)
    ia[[0, 64]], ia[33], ib[5], ib[69] = -1, n, 2**62, -2**63
    bad = np.zeros(n, dtype=bool)
    bad[[0, 64, 33, 5, 69]] = True
    got, _ = _check(a, b, n, n, n, idx_a=ia, idx_b=ib, pose=pose, weights=np.full(n, 3))
    assert (got["flags"][bad] == L.MISS_BAD_INDEX).all() and not (got["flags"][~bad] & L.MISS_BAD_INDEX).any()
    assert np.isnan(got["hmd"][bad]).all() and np.isnan(got["vmd"][bad]).all() and (got["t_cpa_s"][bad] == -1.0).all()
    assert got["totals"][4] == 5 and got["totals"][0] == n - 5 and got["totals"][5] == 3 * (n - 5)
    for name in ("hmd", "vmd", "t_cpa_s", "flags"):
        assert np.array_equal(got[name][~bad], good[name][~bad])
    _against_the_per_second_kernel(got, a, b, n, n, n, idx_a=ia, idx_b=ib, pose=pose, weights=np.full(n, 3))


# ---- 6. pose and pairing
def test_a_null_pose_equals_the_identity_pose():
    n, P = 300, 7
    rows_a, rows_b = R.crossing(n, P, 6)
    a, b = R.planar(rows_a), R.planar(rows_b)
    none, _ = _check(a, b, n, n, n)
    ident, _ = _check(a, b, n, n, n, pose=native.make_pose(np.zeros(n)))
    PC.same(ident, none, ALL)


def test_one_ownship_and_a_permutation():
    n, P = 321, 6
    rows_a, rows_b = R.crossing(n, P, 7)
    a, b = R.planar(rows_a), R.planar(rows_b)
    perm = np.random.RandomState(7).permutation(n).astype(np.int64)
    got, _ = _check(a, b, n, n, n, idx_b=perm)
    moved, _ = _check(a, np.ascontiguousarray(b[:, :, perm]), n, n, n)                 # the permutation done on the host
    PC.same(got, moved, ALL)
    straight, _ = _check(a, b, n, n, n)
    # n_a = 1: the one ownship is pair 5's, so pair 5 is what it was
    one, _ = _check(R.planar(rows_a[5:6]), b, 1, n, n)
    PC.same({k: v[5:6] for k, v in one.items() if k != "totals"}, {k: v[5:6] for k, v in straight.items()}, ("hmd", "vmd", "t_cpa_s", "flags"))


# ---- 7. weights and accumulation
def test_weights_enter_the_totals_only_and_a_second_call_accumulates():
    n, P = 513, 4
    rows_a, rows_b, pose = R.posed_crossing(n, P, 8)
    a, b = R.planar(rows_a), R.planar(rows_b)
    w = np.array([0, 1, 2**24 - 1, 2**32 - 1], dtype=np.uint64)[np.random.RandomState(3).randint(0, 4, n)]
    plain, _ = _check(a, b, n, n, n, pose=pose)
    t = plain["totals"]
    assert t[5] == t[0] == n and t[6] == t[1] and t[7] == t[2] and t[9] == t[8] and t[2] >= t[8] > 0 and t[1] > 0
    got, _ = _check(a, b, n, n, n, pose=pose, weights=w)
    PC.same(got, plain, ("hmd", "vmd", "t_cpa_s", "flags"))            # a weight-0 pair is evaluated like any other
    assert np.array_equal(got["totals"][[0, 1, 2, 3, 4, 8]], t[[0, 1, 2, 3, 4, 8]])
    fl = plain["flags"]
    for k, bit in ((6, L.MISS_NMAC_CPA), (7, L.MISS_NMAC_ANY), (9, L.MISS_NMAC_BETWEEN)):
        assert got["totals"][k] == w[(fl & bit) != 0].sum(dtype=np.uint64) > 0
    assert got["totals"][5] == w.sum(dtype=np.uint64)
    again, _ = _check(a, b, n, n, n, pose=pose, weights=w, totals=got["totals"])
    assert (again["totals"] == 2 * got["totals"]).all()


# ---- 8. NULL outputs
def test_each_output_alone_gives_what_all_together_give():
    n, P = 257, 3
    rows_a, rows_b = R.crossing(n, P, 9)
    a, b = R.planar(rows_a), R.planar(rows_b)
    w = np.random.RandomState(4).randint(0, 1000, n)
    full, _ = _check(a, b, n, n, n, weights=w)
    for name in ALL:
        one = _run(a, b, n, n, n, weights=w, want=(name,))
        PC.same(one, full, (name,))


# ---- 9. the Python surface
def _as_ref(res):
    return {NAMES[k]: v for k, v in res.items() if k in NAMES}


def test_miss_segments_on_numpy_and_torch_inputs_and_a_contexts_stream(gpu_ctx):
    import torch
    n, P = 300, 6
    rows_a, rows_b, pose = R.posed_crossing(n, P, 10)
    want = R.miss_segments(R.planar(rows_a), R.planar(rows_b), n, n, n, pose_b=pose)
    pl_a, pl_b = R.planar(rows_a), R.planar(rows_b)
    side = torch.cuda.Stream()
    ctx = native.Context(0, stream=side.cuda_stream)
    assert gpu_ctx.stream is None and ctx.stream == side.cuda_stream
    for res in (native.miss_segments(rows_a, rows_b, pose_b=pose),                                               # numpy rows
                native.miss_segments(pl_a, pl_b, pose_b=pose, layout="planar"),                                  # numpy planar
                native.miss_segments(torch.from_numpy(rows_a.copy()), torch.from_numpy(rows_b.copy()), pose_b=pose),   # a torch CPU tensor
                native.miss_segments(torch.from_numpy(pl_a).cuda(), torch.from_numpy(pl_b).cuda(), pose_b=torch.from_numpy(pose).cuda(),
                                     layout="planar"),                                                           # a torch device tensor
                native.miss_segments(rows_a, rows_b, pose_b=pose, ctx=gpu_ctx),                                  # a context on its own stream
                native.miss_segments(rows_a, rows_b, pose_b=pose, ctx=ctx),                                      # a context that was given one
                native.miss_segments(rows_a, rows_b, pose_b=pose, stream=0)):                                    # the HIP default stream
        PC.same(_as_ref(res), want, ALL)
        fl = want["flags"]
        assert res["t_cpa_s"].dtype == np.float64 and res["flags"].dtype == np.uint8 and res["totals"].shape == (10,)
        assert np.array_equal(res["nmac"], (fl & 1) != 0) and np.array_equal(res["nmac_any"], (fl & 2) != 0)
        assert np.array_equal(res["between"], (fl & 32) != 0) and res["between"].any()


def test_encounter_miss_segments_and_the_models_between(model_dir):
    from em_model_manned_bayes_amd import em_io
    n, P = 400, 8
    rows_a, rows_b = R.crossing(n, P, 11)
    w = np.random.RandomState(11).randint(1, 2**16, n)
    kw = dict(radius_ft=3000.0, half_height_ft=500.0, seed=0x36)
    enc = native.encounter_pose(rows_a, rows_b, weights=w, rate_scale=4.0e9, **kw)
    two = native.miss_segments(rows_a, rows_b, pose_b=enc["pose"], weights=enc["weights"])
    one = native.encounter_miss_segments(rows_a, rows_b, weights=w, rate_scale=4.0e9, **kw)
    PC.same(one, two, ("hmd_ft", "vmd_ft", "t_cpa_s", "flags", "totals", "nmac", "nmac_any", "between"))
    PC.same(one, {"rate": enc["rate"], "encounter_flags": enc["flags"], "weights": enc["weights"]}, ("rate", "encounter_flags", "weights"))
    assert one["totals"][5] == enc["weights"].sum(dtype=np.uint64)
    PC.same(_as_ref(one), R.miss_segments(R.planar(rows_a), R.planar(rows_b), n, n, n, pose_b=enc["pose"], weights=enc["weights"]), ALL)
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    PC.same(mdl.encounter(rows_a, rows_b, weights=w, rate_scale=4.0e9, between=True, **kw), one, list(one))
    plain = mdl.encounter(rows_a, rows_b, weights=w, rate_scale=4.0e9, **kw)
    PC.same(plain, native.encounter_miss(rows_a, rows_b, weights=w, rate_scale=4.0e9, **kw), list(plain))
    assert "t_cpa" in plain and "t_cpa_s" not in plain and plain["totals"].shape == (8,)
    # .pair
    rows_a, rows_b, pose = R.posed_crossing(n, P, 12)
    want = R.miss_segments(R.planar(rows_a), R.planar(rows_b), n, n, n, pose_b=pose, weights=w)
    got = mdl.pair(rows_a, rows_b, pose=pose, weights=w, between=True)
    PC.same(_as_ref(got), want, ALL)
    assert got["between"].any()
    plain = mdl.pair(rows_a, rows_b, pose=pose, weights=w)
    PC.same({"hmd": plain["hmd_ft"], "t_cpa": plain["t_cpa"], "totals": plain["totals"]},
            miss_ref.miss(R.planar(rows_a), R.planar(rows_b), n, n, n, pose_b=pose, weights=w), ("hmd", "t_cpa", "totals"))
