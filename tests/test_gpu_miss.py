"""-m gpu: k_miss_distance against the numpy restatement of its definition (miss_ref.miss) on the very same tracks.

The comparison rule.  Every number is a sum, a product or a square root of doubles, the same IEEE operations on both sides (the device's
f64 multiply, add and square root are the ones k_track_values' tests rely on), so hmd and vmd are compared BIT FOR BIT (a NaN against a
NaN), and t_cpa, flags and totals are integers.  Every call writes into device buffers pre-filled with a pattern, with guard bytes before
and behind each output that must stay."""
import numpy as np
import pytest

import miss_ref as R
import pair_cases as PC
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native
from em_model_manned_bayes_amd import encounter_model as E
from em_model_manned_bayes_amd import functions as F

pytestmark = pytest.mark.gpu

OUTS = (("hmd", np.float64), ("vmd", np.float64), ("t_cpa", np.int32), ("flags", np.uint8), ("totals", np.uint64))
UR = ((1852.0 / 0.3048) / 3600.0, 1.0 / 60.0, 1.0)
_cache = {}


def _run(a, b, n_a, n_b, n_pairs, idx_a=None, idx_b=None, pose=None, weights=None, want=("hmd", "vmd", "t_cpa", "flags", "totals"),
         totals=None, nmac=(500.0, 100.0)):
    """One call on PLANAR host arrays a [P, 3, ld_a], b [P, 3, ld_b]: the wanted outputs as numpy arrays (the others are passed as NULL)"""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)          # noqa: E731
    d_a, d_b = up(a, np.float64), up(b, np.float64)
    d_ia, d_ib, d_pose = up(idx_a, np.int64), up(idx_b, np.int64), up(pose, np.float64)
    d_w = None if weights is None else torch.from_numpy(np.asarray(weights, dtype=np.uint32).view(np.int32).copy()).to(dev)
    size = {name: (8 if name == "totals" else n_pairs) * np.dtype(dt).itemsize for name, dt in OUTS if name in want}
    zero = np.asarray(np.zeros(8) if totals is None else totals, dtype=np.uint64).view(np.uint8)
    bufs = PC.guarded(size, dev, {"totals": zero})
    ptr = lambda t: 0 if t is None else t.data_ptr()          # noqa: E731
    p = native.miss_params(n_pairs, n_a, n_b, a.shape[0], nmac[0], nmac[1], ld_a=a.shape[2], ld_b=b.shape[2])
    native.miss_distance_device(p, ptr(d_a), ptr(d_b), ptr(d_ia), ptr(d_ib), ptr(d_pose), ptr(d_w),
                                **{name: bufs[name].data_ptr() + PC.GUARD for name in want})
    torch.cuda.synchronize()
    return {name: raw.view(dict(OUTS)[name]) for name, raw in PC.payloads(bufs, size).items()}


_same = lambda got, want, names=("hmd", "vmd", "t_cpa", "flags", "totals"): PC.same(got, want, names)          # noqa: E731


def _check(a, b, n_a, n_b, n_pairs, **kw):
    got = _run(a, b, n_a, n_b, n_pairs, **kw)
    nmac = kw.pop("nmac", (500.0, 100.0))
    kw.pop("want", None)
    want = R.miss(a, b, n_a, n_b, n_pairs, idx_a=kw.get("idx_a"), idx_b=kw.get("idx_b"), pose_b=kw.get("pose"), weights=kw.get("weights"),
                  nmac_h_ft=nmac[0], nmac_v_ft=nmac[1], totals=kw.get("totals"))
    _same(got, want, [k for k in got])
    return got, want


def _pose(n, seed):
    rs = np.random.RandomState(seed)
    return native.make_pose(rs.uniform(-180.0, 180.0, n), rs.uniform(-2000.0, 2000.0, n), rs.uniform(-2000.0, 2000.0, n), rs.uniform(-300.0, 300.0, n))


# ---- 1. tiles and tails
@pytest.mark.parametrize("P", [1, 2, 5, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_tiles_and_tails(n, P):
    a, b = R.planar(PC.tracks(n, P, 1), n + 3), R.planar(PC.tracks(n, P, 2), n + 9)
    got, _ = _check(a, b, n, n, n)                                                     # identity
    assert got["totals"][0] == n
    _check(a, b, n, n, n, pose=_pose(n, n + P))
    own = R.planar(PC.tracks(1, P, 3), 5)
    _check(own, b, 1, n, n, pose=_pose(n, 5))                                          # one ownship
    _check(a, own, n, 1, n)
    rs = np.random.RandomState(n * 64 + P)
    m = n + 17
    _check(a, b, n, n, m, idx_a=rs.randint(0, n, m), idx_b=rs.randint(0, n, m), pose=_pose(m, 9))     # arbitrary indices, with repeats
    _check(a, b, n, n, m, idx_b=rs.randint(0, n, m), idx_a=np.zeros(m, dtype=np.int64))


# ---- 2. two squares that round to one root
def test_the_minimum_is_over_the_roots_not_the_squares():
    dx, dy = 2607.925961031258, 4757.272111997083
    a, b = PC.tracks(256, 2, 4).copy(), PC.tracks(256, 2, 5).copy()
    for lane in (0, 200):
        b[lane] = 0.0
        a[lane, :, 0], a[lane, :, 1], a[lane, :, 2] = [dx, np.nextafter(dx, 0.0)], dy, 0.0
    got, want = _check(R.planar(a), R.planar(b), 256, 256, 256)
    assert got["t_cpa"][0] == 0 and got["t_cpa"][200] == 0 and want["t_cpa"][0] == 0
    assert float(got["hmd"][0]).hex() == "0x1.531360c60e4d8p+12" == float(got["hmd"][200]).hex()


# ---- 3. where the minimum lies
def test_equal_minima_the_last_second_and_a_single_point():
    a = np.zeros((3, 9, 3))
    b = np.zeros((3, 9, 3))
    b[0, :, 0] = [9.0, 8.0, 7.0, 2.0, 5.0, 6.0, 4.0, 2.0, 3.0]                         # equal minima at seconds 3 and 7
    b[1, :, 1] = [9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0]                         # the minimum at the last second
    b[2, :, 0] = 1.0                                                                   # every second equal
    b[:, :, 2] = np.arange(9.0)[None, :] * 10.0
    got, _ = _check(R.planar(a), R.planar(b), 3, 3, 3)
    assert got["t_cpa"].tolist() == [3, 8, 0] and got["vmd"].tolist() == [30.0, 80.0, 0.0] and got["hmd"].tolist() == [2.0, 1.0, 1.0]
    got, _ = _check(R.planar(a[:, :1]), R.planar(b[:, :1]), 3, 3, 3)                   # P = 1
    assert got["t_cpa"].tolist() == [0, 0, 0] and got["hmd"].tolist() == [9.0, 9.0, 1.0]


# ---- 4. NaN and inf
def test_nan_and_inf():
    a = np.zeros((4, 6, 3))
    b = np.zeros((4, 6, 3))
    b[:, :, 0] = [7.0, 5.0, 1.0, 3.0, 2.0, 6.0]
    b[:, :, 2] = np.arange(6.0) * 10.0
    b[0, 2, 0] = np.nan                      # a NaN x at the second that would be the CPA: skipped, the next best (second 4) wins
    b[1, 2, 2] = np.nan                      # a NaN z at the CPA: vmd NaN, bit 0 clear (nmac_h is 1.5: no other second is inside)
    b[2, :, 0] = np.nan                      # all-NaN x
    b[3, :, 0] = np.inf                      # an infinite x at every second
    got, _ = _check(R.planar(a), R.planar(b), 4, 4, 4, nmac=(1.5, 100.0))
    assert got["t_cpa"].tolist() == [4, 2, -1, 0]
    assert got["hmd"][0] == 2.0 and got["vmd"][0] == 40.0 and got["flags"][0] == 0
    assert got["hmd"][1] == 1.0 and np.isnan(got["vmd"][1]) and got["flags"][1] == 0
    assert np.isnan(got["hmd"][2]) and np.isnan(got["vmd"][2]) and got["flags"][2] == L.MISS_NO_CPA
    assert got["hmd"][3] == np.inf and got["vmd"][3] == 0.0 and got["flags"][3] == 0
    assert got["totals"].tolist() == [4, 0, 0, 1, 0, 4, 0, 0]
    # NaN in A, in y, and a NaN before any number: the same rules
    a[0, 0, 1] = np.nan
    a[3, :, 0] = np.inf                      # inf - inf: NaN at every second
    got, _ = _check(R.planar(a), R.planar(b), 4, 4, 4)
    assert got["t_cpa"].tolist() == [4, 2, -1, -1]


# ---- 5. thresholds
def test_thresholds_are_strict():
    a = np.zeros((3, 2, 3))
    b = np.zeros((3, 2, 3))
    b[0, :, 0], b[0, :, 2] = 500.0, 10.0                     # hmd exactly nmac_h
    b[1, :, 0], b[1, :, 2] = 10.0, -100.0                    # |vmd| exactly nmac_v
    b[2, :, 0], b[2, :, 2] = [400.0, 100.0], [50.0, 150.0]   # inside both at second 0, outside the vertical one at the CPA (second 1)
    got, _ = _check(R.planar(a), R.planar(b), 3, 3, 3)
    assert got["hmd"].tolist() == [500.0, 10.0, 100.0] and got["vmd"].tolist() == [10.0, -100.0, 150.0]
    assert got["flags"].tolist() == [0, 0, L.MISS_NMAC_ANY] and got["totals"].tolist() == [3, 0, 1, 0, 0, 3, 0, 1]
    # the same distances one ulp below the thresholds
    got, _ = _check(R.planar(a), R.planar(b), 3, 3, 3, nmac=(float(np.nextafter(500.0, np.inf)), float(np.nextafter(100.0, np.inf))))
    assert got["flags"].tolist() == [3, 3, L.MISS_NMAC_ANY]
    got, _ = _check(R.planar(a), R.planar(b), 3, 3, 3, nmac=(0.0, 0.0))
    assert got["flags"].tolist() == [0, 0, 0]


# ---- 6. bad indices
def test_bad_indices_load_nothing_and_leave_their_neighbours_alone():
    n, P = 70, 5
    a, b = R.planar(PC.tracks(n, P, 6), n + 2), R.planar(PC.tracks(n, P, 7), n)
    ia, ib = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)[::-1].copy()
    good, _ = _check(a, b, n, n, n, idx_a=ia, idx_b=ib, pose=_pose(n, 1))
    ia[[0, 64]], ia[33], ib[5], ib[69] = -1, n, 2**62, -2**63
    bad = np.zeros(n, dtype=bool)
    bad[[0, 64, 33, 5, 69]] = True
    got, _ = _check(a, b, n, n, n, idx_a=ia, idx_b=ib, pose=_pose(n, 1), weights=np.full(n, 3))
    assert (got["flags"][bad] == L.MISS_BAD_INDEX).all() and not (got["flags"][~bad] & L.MISS_BAD_INDEX).any()
    assert np.isnan(got["hmd"][bad]).all() and np.isnan(got["vmd"][bad]).all() and (got["t_cpa"][bad] == -1).all()
    assert got["totals"][4] == 5 and got["totals"][0] == n - 5 and got["totals"][5] == 3 * (n - 5)
    for name in ("hmd", "vmd", "t_cpa", "flags"):
        assert np.array_equal(got[name][~bad], good[name][~bad])


# ---- 7. pose
def test_a_null_pose_equals_the_identity_pose():
    n, P = 300, 7
    a, b = R.planar(PC.tracks(n, P, 8)), R.planar(PC.tracks(n, P, 9))
    none, _ = _check(a, b, n, n, n)
    ident, _ = _check(a, b, n, n, n, pose=native.make_pose(np.zeros(n)))
    _same(ident, none)


# ---- 8. weights and accumulation
def test_weights_enter_the_totals_only_and_a_second_call_accumulates():
    n, P = 513, 4
    a, b = R.planar(PC.tracks(n, P, 10)), R.planar(PC.tracks(n, P, 11))
    pose = native.make_pose(0.0, np.zeros(n), 0.0, 0.0)
    w = np.array([0, 1, 2**24 - 1, 2**32 - 1], dtype=np.uint64)[np.random.RandomState(3).randint(0, 4, n)]
    plain, _ = _check(a, b, n, n, n, pose=pose)
    assert plain["totals"][5] == plain["totals"][0] == n and plain["totals"][6] == plain["totals"][1] and plain["totals"][7] == plain["totals"][2]
    assert plain["totals"][2] >= plain["totals"][1] > 0                 # (the case holds NMACs: the weighted sums below are not all zero)
    got, _ = _check(a, b, n, n, n, pose=pose, weights=w)
    _same(got, plain, ("hmd", "vmd", "t_cpa", "flags"))                 # a weight-0 pair is evaluated like any other
    assert got["totals"][5] == w.sum(dtype=np.uint64) and got["totals"][6] == w[(plain["flags"] & 1) != 0].sum(dtype=np.uint64) > 0
    again, _ = _check(a, b, n, n, n, pose=pose, weights=w, totals=got["totals"])
    assert (again["totals"] == 2 * got["totals"]).all()
    # the largest weight on every pair: the sum passes 2^32 and stays exact
    top, _ = _check(a, b, n, n, n, pose=pose, weights=np.full(n, 2**32 - 1, dtype=np.uint64))
    assert int(top["totals"][5]) == n * (2**32 - 1)


# ---- 9. NULL outputs
def test_each_output_alone_gives_what_all_together_give():
    n, P = 257, 3
    a, b = R.planar(PC.tracks(n, P, 12)), R.planar(PC.tracks(n, P, 13))
    w = np.random.RandomState(4).randint(0, 1000, n)
    full, _ = _check(a, b, n, n, n, weights=w)
    for name, _dt in OUTS:
        one = _run(a, b, n, n, n, weights=w, want=(name,))
        _same(one, full, (name,))


def test_a_context_hands_its_stream_to_the_context_free_call(gpu_ctx):
    """Context.stream: None for a context on its own stream (the helper then syncs it), the raw stream for one that was given one (the
    helper then launches on it); either way the answers are the restatement's."""
    import torch
    n, P = 300, 6
    rows_a, rows_b, pose = PC.tracks(n, P, 14), PC.tracks(n, P, 15), _pose(n, 16)
    want = R.miss(R.planar(rows_a), R.planar(rows_b), n, n, n, pose_b=pose)
    names = {"hmd_ft": "hmd", "vmd_ft": "vmd", "t_cpa": "t_cpa", "flags": "flags", "totals": "totals"}
    side = torch.cuda.Stream()
    ctx = native.Context(0, stream=side.cuda_stream)
    assert gpu_ctx.stream is None and ctx.stream == side.cuda_stream
    for c in (gpu_ctx, ctx):
        res = native.miss_distance(rows_a, rows_b, pose_b=pose, ctx=c)
        _same({names[k]: v for k, v in res.items() if k in names}, want)
    res = native.miss_distance(rows_a, rows_b, pose_b=pose, stream=0)             # the HIP default stream
    _same({names[k]: v for k, v in res.items() if k in names}, want)


# ---- 10. the library's own tracks
def _sampled(gpu_ctx, model_dir):
    """(device tensor xyz [T + 1, 3, n] of emgpu_sample2track_device, the same on the host, the model's path): 512 trajectories x 32 s"""
    if "sampled" not in _cache:
        import torch
        dev = torch.device("cuda", 0)
        n, T = 512, 32
        path = em_io.materialize_model("uncor_1200code_v2p1", model_dir)
        parms = em_io.em_read(path)
        nm, labs = parms["native"], parms["labels_initial"]
        ids = [labs.index('"%s"' % s) for s in ("L", "v", "\\dot h", "\\dot v", "\\dot \\psi")]
        tm = [int(r[0]) - 1 for r in np.asarray(parms["temporal_map"]).reshape(-1, 2)]
        slots = [tm.index(v) for v in ids[2:]]
        s = native.sample_dbn_host(gpu_ctx, nm, n, T, 0x3155, raw=True, pinned=False)
        d_iv, d_dv = torch.from_numpy(s["init_val"].copy()).to(dev), torch.from_numpy(s["dyn_val"].copy()).to(dev)
        d_xyz = torch.zeros((T + 1, 3, n), dtype=torch.float64, device=dev)
        b_v = np.asarray(parms["boundaries"][ids[1]], dtype=np.float64)
        torch.cuda.synchronize()
        tp = native.track_params(n, T, *UR, float(b_v[0]), float(b_v[-1]), nd=nm.n_dyn, slot_vertrate=slots[0], slot_acc=slots[1], slot_turnrate=slots[2])
        native.sample2track_device(gpu_ctx, tp, d_iv[ids[0]].data_ptr(), d_iv[ids[1]].data_ptr(), d_dv.data_ptr(), d_xyz.data_ptr())
        gpu_ctx.sync()
        _cache["sampled"] = (d_xyz, d_xyz.cpu().numpy(), path)
    return _cache["sampled"]


def test_round_trip_with_the_librarys_own_tracks(gpu_ctx, model_dir):
    import torch
    d_xyz, xyz, path = _sampled(gpu_ctx, model_dir)
    P, _, n = xyz.shape
    assert np.isfinite(xyz).all() and np.abs(xyz[-1, :2]).max() > 100.0            # tracks that moved
    perm = np.random.RandomState(5).permutation(n).astype(np.int64)
    # every intruder turned at random and placed within 600 ft and 150 ft of its ownship's start, so that a good part are NMACs
    rs = np.random.RandomState(6)
    pose = native.make_pose(rs.uniform(-180.0, 180.0, n), rs.uniform(-600.0, 600.0, n), rs.uniform(-600.0, 600.0, n),
                            xyz[0, 2, :] - xyz[0, 2, perm] + rs.uniform(-150.0, 150.0, n))
    want = R.miss(xyz, xyz, n, n, n, idx_b=perm, pose_b=pose)
    assert 0 < want["totals"][1] <= want["totals"][2] < n
    # the device tensor as it lies
    d_perm, d_pose = torch.from_numpy(perm).cuda(), torch.from_numpy(pose).cuda()
    outs = {"hmd": torch.zeros(n, dtype=torch.float64, device="cuda"), "vmd": torch.zeros(n, dtype=torch.float64, device="cuda"),
            "t_cpa": torch.zeros(n, dtype=torch.int32, device="cuda"), "flags": torch.zeros(n, dtype=torch.uint8, device="cuda"),
            "totals": torch.zeros(8, dtype=torch.int64, device="cuda")}
    native.miss_distance_device(native.miss_params(n, n, n, P), d_xyz.data_ptr(), d_xyz.data_ptr(), 0, d_perm.data_ptr(), d_pose.data_ptr(), 0,
                                **{k: v.data_ptr() for k, v in outs.items()})
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    got["totals"] = got["totals"].view(np.uint64)
    _same(got, want)
    # numpy ROWS input through the helper, and the torch tensor through the PLANAR layout
    rows = np.ascontiguousarray(np.transpose(xyz, (2, 0, 1)))
    names = {"hmd_ft": "hmd", "vmd_ft": "vmd", "t_cpa": "t_cpa", "flags": "flags", "totals": "totals"}
    mdl = E.UncorEncounterModel(parameters_filename=path)
    for res in (native.miss_distance(rows, rows, idx_b=perm, pose_b=pose),
                native.miss_distance(d_xyz, d_xyz, idx_b=perm, pose_b=pose, layout="planar", ctx=gpu_ctx),
                mdl.pair(rows, rows, pose=pose, idx_intruder=perm, ctx=gpu_ctx)):
        _same({names[k]: v for k, v in res.items() if k in names}, want)
        assert np.array_equal(res["nmac"], (want["flags"] & 1) != 0)
    # one ownship against every intruder, weighted
    w = np.random.RandomState(7).randint(0, 2**24, n)
    res = mdl.pair(rows[:1], rows, pose=pose, weights=w)
    _same({names[k]: v for k, v in res.items() if k in names}, R.miss(xyz[:, :, :1], xyz, 1, n, n, pose_b=pose, weights=w))


def test_get_generated_miss_distance_on_times_that_partly_overlap(gpu_ctx, model_dir):
    _, xyz, _ = _sampled(gpu_ctx, model_dir)
    P = xyz.shape[0]
    own = {"t_s": np.arange(P, dtype=np.float64), "x_nm": xyz[:, 0, 3] / F.NM_TO_FT, "y_nm": xyz[:, 1, 3] / F.NM_TO_FT, "z_ft": xyz[:, 2, 3]}
    t_int = np.arange(10, 10 + P, dtype=np.float64)                                  # the intruder starts ten seconds later
    intr = {"t_s": t_int, "x_nm": (xyz[:, 0, 4] + 900.0) / F.NM_TO_FT, "y_nm": xyz[:, 1, 4] / F.NM_TO_FT, "z_ft": xyz[:, 2, 4] + 40.0}
    hmd, vmd, tcpa, i_own, i_int = F.getGeneratedMissDistance([own, intr])
    # the definition on the overlap: own seconds 10 .. P-1 against the intruder's 0 .. P-11, in feet as the function converts them
    k = P - 10
    a = np.stack([own["x_nm"][10:] * F.NM_TO_FT, own["y_nm"][10:] * F.NM_TO_FT, own["z_ft"][10:]], axis=1)[:, :, None]
    b = np.stack([intr["x_nm"][:k] * F.NM_TO_FT, intr["y_nm"][:k] * F.NM_TO_FT, intr["z_ft"][:k]], axis=1)[:, :, None]
    want = R.miss(a, b, 1, 1, 1)
    t = int(want["t_cpa"][0])
    assert (hmd, vmd) == (want["hmd"][0], want["vmd"][0]) and (tcpa, i_own, i_int) == (10.0 + t, 10 + t, t)
    # the reference's own order of operations (the root in nautical miles, then the factor) agrees to rounding
    d_nm = np.sqrt((own["x_nm"][10:] - intr["x_nm"][:k]) ** 2 + (own["y_nm"][10:] - intr["y_nm"][:k]) ** 2) * F.NM_TO_FT
    assert abs(d_nm.min() - hmd) <= 1e-9 * max(hmd, 1.0)
    assert np.isnan(F.getGeneratedMissDistance([own, dict(intr, t_s=t_int + 1000.0)])[0])
