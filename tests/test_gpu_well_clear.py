"""-m gpu: k_well_clear against the numpy restatement of its definition (well_clear_ref.well_clear) on the very same tracks, and against
k_miss_distance where the two events are tied.

The comparison rule is test_gpu_miss_segments': every number is a sum, a product or a quotient of doubles, the same IEEE operations on
both sides, so tau_min is compared BIT FOR BIT (a NaN against a NaN), and t_first, n_lost, flags and totals are integers.  Every call
writes into device buffers pre-filled with a pattern, with guard bytes before and behind each output that must stay."""
import numpy as np
import pytest

import pair_cases as PC
import well_clear_ref as R
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import native
from em_model_manned_bayes_amd import encounter_model as E

pytestmark = pytest.mark.gpu

OUTS = (("t_first", np.int32), ("n_lost", np.int32), ("tau_min", np.float64), ("flags", np.uint8), ("totals", np.uint64))
ALL = tuple(name for name, _ in OUTS)
MISS_OUTS = (("hmd", np.float64), ("vmd", np.float64), ("t_cpa", np.int32), ("flags", np.uint8), ("totals", np.uint64))
NAMES = {"t_first": "t_first", "n_lost": "n_lost", "tau_min_s": "tau_min", "flags": "flags", "totals": "totals"}
PLACED = {"t_first": "t_first", "n_lost": "n_lost", "tau_min_s": "tau_min", "wc_flags": "flags", "wc_totals": "totals"}


def _run(a, b, n_a, n_b, n_pairs, idx_a=None, idx_b=None, pose=None, weights=None, miss_flags=None, want=ALL, totals=None, thr=R.DEFAULTS,
         miss=None):
    """One call on PLANAR host arrays a [P, 3, ld_a], b [P, 3, ld_b]: the wanted outputs as numpy arrays (the others are passed as NULL).
    miss=(nmac_h, nmac_v): k_miss_distance first, on the same device inputs, its flags handed over on the device as miss_flags; returns
    (the well-clear outputs, the miss kernel's five)."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)          # noqa: E731
    d_a, d_b = up(a, np.float64), up(b, np.float64)
    d_ia, d_ib, d_pose, d_mf = up(idx_a, np.int64), up(idx_b, np.int64), up(pose, np.float64), up(miss_flags, np.uint8)
    d_w = None if weights is None else torch.from_numpy(np.asarray(weights, dtype=np.uint32).view(np.int32).copy()).to(dev)
    ptr = lambda t: 0 if t is None else t.data_ptr()          # noqa: E731
    inputs = (ptr(d_a), ptr(d_b), ptr(d_ia), ptr(d_ib), ptr(d_pose), ptr(d_w))
    sec = None
    if miss is not None:
        m_types = dict(MISS_OUTS)
        m_size = {name: (8 if name == "totals" else n_pairs) * np.dtype(m_types[name]).itemsize for name in m_types}
        m_bufs = PC.guarded(m_size, dev, {"totals": np.zeros(64, dtype=np.uint8)})
        native.miss_distance_device(native.miss_params(n_pairs, n_a, n_b, a.shape[0], miss[0], miss[1], ld_a=a.shape[2], ld_b=b.shape[2]), *inputs,
                                    **{name: m_bufs[name].data_ptr() + PC.GUARD for name in m_types})
        mf_ptr = m_bufs["flags"].data_ptr() + PC.GUARD
    else:
        mf_ptr = ptr(d_mf)
    types = dict(OUTS)
    size = {name: (10 if name == "totals" else n_pairs) * np.dtype(types[name]).itemsize for name in want}
    zero = np.asarray(np.zeros(10) if totals is None else totals, dtype=np.uint64).view(np.uint8)
    bufs = PC.guarded(size, dev, {"totals": zero})
    p = native.well_clear_params(n_pairs, n_a, n_b, a.shape[0], ld_a=a.shape[2], ld_b=b.shape[2], **thr)
    native.well_clear_device(p, *inputs, miss_flags=mf_ptr, **{name: bufs[name].data_ptr() + PC.GUARD for name in want})
    torch.cuda.synchronize()
    got = {name: raw.view(types[name]) for name, raw in PC.payloads(bufs, size).items()}
    if miss is not None:
        sec = {name: raw.view(m_types[name]) for name, raw in PC.payloads(m_bufs, m_size).items()}
        return got, sec
    return got


def _check(a, b, n_a, n_b, n_pairs, **kw):
    got = _run(a, b, n_a, n_b, n_pairs, **kw)
    want = R.well_clear(a, b, n_a, n_b, n_pairs, idx_a=kw.get("idx_a"), idx_b=kw.get("idx_b"), pose_b=kw.get("pose"), weights=kw.get("weights"),
                        miss_flags=kw.get("miss_flags"), totals=kw.get("totals"), **kw.get("thr", R.DEFAULTS))
    PC.same(got, want, list(got))
    return got, want


def _floors(want, n, P):
    """the conditions on the inputs (test_well_clear.py), where the case is large enough to carry them"""
    if n >= 257 and P >= 2:
        share = R.shares(want, n)
        for name, floor in R.FLOORS.items():
            assert share[name] >= floor, (name, share[name])
        if P == 64:
            assert share["later"] >= 0.05


# ---- 1. tiles and tails
@pytest.mark.parametrize("P", [1, 2, 3, 5, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_tiles_and_tails(n, P):
    plain_a, plain_b = R.approaching(n, P, 1)
    got, want = _check(R.planar(plain_a, n + 3), R.planar(plain_b, n), n, n, n)        # without a pose
    assert got["totals"][0] == n
    _floors(want, n, P)
    rows_a, rows_b, pose = R.posed_approaching(n, P, 1)
    a, b = R.planar(rows_a, n + 3), R.planar(rows_b, n + 9)
    got, _ = _check(a, b, n, n, n, pose=pose)                                          # through a random pose
    assert got["totals"][0] == n
    own = R.planar(rows_a[:1], 5)
    _check(own, b, 1, n, n, pose=pose)                                                 # one ownship
    rs = np.random.RandomState(n * 64 + P)
    m = n + 17
    _check(a, b, n, n, m, idx_a=rs.randint(0, n, m), idx_b=rs.randint(0, n, m), pose=np.ascontiguousarray(pose[:, rs.randint(0, n, m)]))


# ---- 2. a workgroup that walks two tiles
def test_grid_walk():
    n, P = 2048 * 256 + 300, 3
    rows_a, rows_b = R.approaching(1000, P, 1)
    a, b = R.planar(rows_a), R.planar(rows_b)
    rs = np.random.RandomState(2)
    ia, ib = np.arange(n, dtype=np.int64) % 1000, np.arange(n, dtype=np.int64) % 1000
    w = rs.randint(0, 2**32, n, dtype=np.uint64)
    mf = rs.randint(0, 64, n).astype(np.uint8)
    got, want = _check(a, b, 1000, 1000, n, idx_a=ia, idx_b=ib, weights=w, miss_flags=mf)
    assert got["totals"][0] == n and got["totals"][8] > 0 and got["totals"][9] > 2**32


# ---- 3. the hand-computed cases
@pytest.mark.parametrize("case", R.HAND, ids=[c[0] for c in R.HAND])
def test_hand_computed(case):
    _, (a, b), thr, t_first, n_lost, tau_min, flags, _ = case
    got, _ = _check(R.planar(a, 3), R.planar(b, 2), 1, 1, 1, thr=thr)
    want = {"t_first": np.array([t_first], dtype=np.int32), "n_lost": np.array([n_lost], dtype=np.int32), "tau_min": np.array([tau_min]),
            "flags": np.array([flags], dtype=np.uint8)}
    PC.same(got, want, ("t_first", "n_lost", "tau_min", "flags"))
    # the same case in lane 70 of 130, between approaching pairs
    rows_a, rows_b = (x.copy() for x in R.approaching(130, a.shape[1], 3))
    rows_a[70], rows_b[70] = a[0], b[0]
    got, _ = _check(R.planar(rows_a), R.planar(rows_b), 130, 130, 130, thr=thr)
    PC.same({k: v[70:71] for k, v in got.items() if k != "totals"}, want, ("t_first", "n_lost", "tau_min", "flags"))


# ---- 4. NaN and inf
def test_nan_and_inf():
    n, P = 300, 9
    rows_a, rows_b, pose = R.posed_approaching(n, P, 4)
    rows_a, rows_b, pose = rows_a.copy(), rows_b.copy(), pose.copy()
    rs = np.random.RandomState(4)
    for bad in (np.nan, np.inf, -np.inf):
        for rows in (rows_a, rows_b):
            rows[rs.randint(0, n, 40), rs.randint(0, P, 40), rs.randint(0, 3, 40)] = bad
    rows_a[7] = np.nan                                   # a pair with no number at all
    rows_b[8, :, 0] = np.inf                             # inf at every second: rr is inf, no point is valid
    a, b = R.planar(rows_a), R.planar(rows_b)
    got, _ = _check(a, b, n, n, n)
    for i in (7, 8):
        assert got["flags"][i] == L.WC_NO_DATA and got["t_first"][i] == -1 and got["n_lost"][i] == 0 and np.isnan(got["tau_min"][i])
    pose[rs.randint(0, 5, 30), rs.randint(9, n, 30)] = np.array([np.nan, np.inf, -np.inf])[rs.randint(0, 3, 30)]          # and in a pose
    got, _ = _check(a, b, n, n, n, pose=pose)
    assert (got["flags"] == L.WC_NO_DATA).sum() > 2 and ((got["flags"] & L.WC_LOST) != 0).any()


# ---- 5. bad indices
def test_bad_indices_load_nothing_and_leave_their_neighbours_alone():
    n, P = 70, 5
    rows_a, rows_b, pose = R.posed_approaching(n, P, 5)
    a, b = R.planar(rows_a, n + 2), R.planar(rows_b, n)
    ia, ib = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)
    mf = np.full(n, L.MISS_NMAC_ANY, dtype=np.uint8)
    good, _ = _check(a, b, n, n, n, idx_a=ia, idx_b=ib, pose=pose)
    ia[[0, 64]], ia[33], ib[5], ib[69] = -1, n, 2**62, -2**63
    bad = np.zeros(n, dtype=bool)
    bad[[0, 64, 33, 5, 69]] = True
    got, _ = _check(a, b, n, n, n, idx_a=ia, idx_b=ib, pose=pose, weights=np.full(n, 3), miss_flags=mf)
    assert (got["flags"][bad] == L.WC_BAD_INDEX).all() and not (got["flags"][~bad] & L.WC_BAD_INDEX).any()
    assert np.isnan(got["tau_min"][bad]).all() and (got["t_first"][bad] == -1).all() and (got["n_lost"][bad] == 0).all()
    assert got["totals"][4] == 5 and got["totals"][0] == n - 5 and got["totals"][5] == 3 * (n - 5)
    assert got["totals"][8] == got["totals"][1] and got["totals"][9] == got["totals"][6]          # a bad pair is no NMAC among the losses
    for name in ("t_first", "n_lost", "tau_min", "flags"):
        assert np.array_equal(got[name][~bad], good[name][~bad], equal_nan=name == "tau_min")


# ---- 6. NULL outputs
def test_each_output_alone_and_every_output_but_one():
    n, P = 257, 3
    rows_a, rows_b = R.approaching(n, P, 9)
    a, b = R.planar(rows_a), R.planar(rows_b)
    w = np.random.RandomState(4).randint(0, 1000, n)
    mf = np.random.RandomState(5).randint(0, 4, n).astype(np.uint8)
    full, _ = _check(a, b, n, n, n, weights=w, miss_flags=mf)
    for name in ALL:
        one = _run(a, b, n, n, n, weights=w, miss_flags=mf, want=(name,))
        PC.same(one, full, (name,))
        rest = tuple(k for k in ALL if k != name)
        PC.same(_run(a, b, n, n, n, weights=w, miss_flags=mf, want=rest), full, rest)


# ---- 7. weights and accumulation
def test_totals_are_added_to_and_without_miss_flags_the_last_two_stay():
    n, P = 513, 4
    rows_a, rows_b, pose = R.posed_approaching(n, P, 8)
    a, b = R.planar(rows_a), R.planar(rows_b)
    w = np.array([0, 1, 2**24 - 1, 2**32 - 1], dtype=np.uint64)[np.random.RandomState(3).randint(0, 4, n)]
    start = np.arange(10, dtype=np.uint64) * 1000 + 7
    plain, _ = _check(a, b, n, n, n, pose=pose)
    t = plain["totals"]
    assert t[5] == t[0] == n and t[6] == t[1] > 0 and t[7] == t[2] > 0 and t[8] == t[9] == 0
    got, _ = _check(a, b, n, n, n, pose=pose, weights=w, totals=start)
    PC.same(got, plain, ("t_first", "n_lost", "tau_min", "flags"))            # a weight-0 pair is evaluated like any other
    fl = plain["flags"]
    assert np.array_equal(got["totals"][:5], t[:5] + start[:5]) and np.array_equal(got["totals"][8:], start[8:])
    for k, bit in ((6, L.WC_LOST), (7, L.WC_AT_START)):
        assert got["totals"][k] - start[k] == w[(fl & bit) != 0].sum(dtype=np.uint64) > 0
    assert got["totals"][5] - start[5] == w.sum(dtype=np.uint64)
    mf = np.random.RandomState(6).randint(0, 64, n).astype(np.uint8)
    again, _ = _check(a, b, n, n, n, pose=pose, weights=w, miss_flags=mf, totals=got["totals"])
    hit = ((fl & L.WC_LOST) != 0) & ((mf & L.MISS_NMAC_ANY) != 0)
    assert again["totals"][8] - start[8] == hit.sum() > 0 and again["totals"][9] - start[9] == w[hit].sum(dtype=np.uint64)


# ---- 8. against k_miss_distance on the same device inputs
@pytest.mark.parametrize("thr", [dict(tau_s=35.0, dmod_ft=4000.0, hmd_ft=4000.0, h_ft=450.0), dict(tau_s=0.0, dmod_ft=500.0, hmd_ft=0.0, h_ft=100.0)],
                         ids=["the defaults", "the NMAC cylinder itself"])
def test_every_nmac_is_a_loss_of_well_clear(thr):
    """d < 500 && |dz| < 100 at some second implies rr <= dmod^2 && |z| <= h there when dmod >= 500 and h >= 100: the IEEE root is
    monotone, so rr > 250000 would give d >= sqrt(250000) = 500.  With k_miss_distance's flags as miss_flags, totals[8] is its totals[2]."""
    n, P = 1000, 12
    rows_a, rows_b = R.approaching(n, P, 13, dmod=600.0, h=120.0)                     # close starts: NMACs at some second
    a, b = R.planar(rows_a), R.planar(rows_b)
    w = np.random.RandomState(13).randint(1, 2**20, n)
    (got, sec) = _run(a, b, n, n, n, weights=w, miss=(500.0, 100.0), thr=thr)
    nmac = (sec["flags"] & L.MISS_NMAC_ANY) != 0
    assert nmac.sum() >= n // 20 and not nmac.all()
    assert ((got["flags"][nmac] & L.WC_LOST) != 0).all()
    assert got["totals"][8] == sec["totals"][2] == nmac.sum() and got["totals"][9] == sec["totals"][7]
    want = R.well_clear(a, b, n, n, n, weights=w, miss_flags=sec["flags"], **thr)
    PC.same(got, want, ALL)


# ---- 9. the Python surface
def _as_ref(res, names=NAMES):
    return {names[k]: v for k, v in res.items() if k in names}


def test_well_clear_on_numpy_and_torch_inputs_and_a_contexts_stream(gpu_ctx):
    import torch
    n, P = 300, 12
    rows_a, rows_b, pose = R.posed_approaching(n, P, 10)
    mf = np.random.RandomState(10).randint(0, 64, n).astype(np.uint8)
    want = R.well_clear(R.planar(rows_a), R.planar(rows_b), n, n, n, pose_b=pose, miss_flags=mf)
    pl_a, pl_b = R.planar(rows_a), R.planar(rows_b)
    side = torch.cuda.Stream()
    ctx = native.Context(0, stream=side.cuda_stream)
    for res in (native.well_clear(rows_a, rows_b, pose_b=pose, miss_flags=mf),                                       # numpy rows
                native.well_clear(pl_a, pl_b, pose_b=pose, miss_flags=mf, layout="planar"),                          # numpy planar
                native.well_clear(torch.from_numpy(pl_a).cuda(), torch.from_numpy(pl_b).cuda(), pose_b=torch.from_numpy(pose).cuda(),
                                  miss_flags=torch.from_numpy(mf).cuda(), layout="planar"),                          # torch device tensors
                native.well_clear(rows_a, rows_b, pose_b=pose, miss_flags=mf, ctx=gpu_ctx),                          # a context on its own stream
                native.well_clear(rows_a, rows_b, pose_b=pose, miss_flags=mf, ctx=ctx),                              # a context that was given one
                native.well_clear(rows_a, rows_b, pose_b=pose, miss_flags=mf, stream=0)):                            # the HIP default stream
        PC.same(_as_ref(res), want, ALL)
        fl = want["flags"]
        assert res["t_first"].dtype == res["n_lost"].dtype == np.int32 and res["flags"].dtype == np.uint8 and res["totals"].shape == (10,)
        assert np.array_equal(res["lowc"], (fl & 1) != 0) and np.array_equal(res["at_start"], (fl & 2) != 0) and res["lowc"].any()
    other = dict(tau_s=20.0, dmod_ft=2500.0, hmd_ft=1500.0, h_ft=300.0)
    PC.same(_as_ref(native.well_clear(rows_a, rows_b, pose_b=pose, **other)), R.well_clear(pl_a, pl_b, n, n, n, pose_b=pose, **other), ALL)


@pytest.mark.parametrize("between", [False, True])
def test_the_placed_forms_and_the_models_method(between, model_dir):
    from em_model_manned_bayes_amd import em_io
    n, P = 300, 12
    rows_a, rows_b = R.approaching(n, P, 11)
    pl_a, pl_b = R.planar(rows_a), R.planar(rows_b)
    w = np.random.RandomState(11).randint(1, 2**16, n)
    miss_keys = ("hmd_ft", "vmd_ft", "t_cpa_s" if between else "t_cpa", "flags", "nmac", "totals", "rate", "encounter_flags", "weights")
    for placed, miss, pose_of, kw in (
            (native.encounter_well_clear, native.encounter_miss_segments if between else native.encounter_miss, native.encounter_pose,
             dict(radius_ft=12000.0, half_height_ft=800.0, seed=0x38)),
            (native.cpa_well_clear, native.cpa_miss_segments if between else native.cpa_miss, native.cpa_pose,
             dict(hmd_max_ft=3000.0, vmd_max_ft=900.0, seed=0x38, t_lo=2, t_hi=9))):          # (half of the passes are above h_ft)
        one = placed(rows_a, rows_b, weights=w, rate_scale=4.0e9, between=between, **kw)
        two = miss(rows_a, rows_b, weights=w, rate_scale=4.0e9, **kw)
        PC.same(one, two, list(two))                                                     # the miss part is what the miss form returns
        assert set(miss_keys) <= set(two) and set(one) == set(two) | set(PLACED) | {"lowc", "at_start"}
        pose = pose_of(rows_a, rows_b, weights=w, rate_scale=4.0e9, **kw)
        want = R.well_clear(pl_a, pl_b, n, n, n, pose_b=pose["pose"], weights=pose["weights"], miss_flags=two["flags"])
        PC.same(_as_ref(one, PLACED), want, ALL)
        assert one["lowc"].any() and not one["lowc"].all() and one["wc_totals"][5] == pose["weights"].sum(dtype=np.uint64)
        assert np.array_equal(one["lowc"], (want["flags"] & 1) != 0) and np.array_equal(one["at_start"], (want["flags"] & 2) != 0)
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    rows_a, rows_b, pose = R.posed_approaching(n, P, 12)
    mf = mdl.pair(rows_a, rows_b, pose=pose, weights=w, between=between)["flags"]
    got = mdl.well_clear(rows_a, rows_b, pose=pose, weights=w, miss_flags=mf)
    PC.same(_as_ref(got), R.well_clear(R.planar(rows_a), R.planar(rows_b), n, n, n, pose_b=pose, weights=w, miss_flags=mf), ALL)
