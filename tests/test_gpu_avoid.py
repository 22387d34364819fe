"""-m gpu: k_avoid against the numpy restatement of its definition (avoid_ref.avoid) on the very same tracks, and against k_miss_distance
and k_well_clear where their events are tied to its own.

The comparison rule is test_gpu_well_clear's: every number is a sum, a product, a quotient or a root of doubles, the same IEEE operations
on both sides, so hmd, vmd and vmd_mit are compared BIT FOR BIT (a NaN against a NaN), and t_cpa, t_alert, flags and totals are integers.
Every call writes into device buffers pre-filled with a pattern, with guard bytes before and behind each output that must stay."""
import numpy as np
import pytest

import avoid_ref as R
import pair_cases as PC
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import native
from em_model_manned_bayes_amd import encounter_model as E

pytestmark = pytest.mark.gpu

OUTS = (("hmd", np.float64), ("vmd", np.float64), ("vmd_mit", np.float64), ("t_cpa", np.int32), ("t_alert", np.int32), ("flags", np.uint8),
        ("totals", np.uint64))
ALL = tuple(name for name, _ in OUTS)
PER_PAIR = ALL[:-1]
MISS_OUTS = (("hmd", np.float64), ("vmd", np.float64), ("t_cpa", np.int32), ("flags", np.uint8), ("totals", np.uint64))
WC_OUTS = (("t_first", np.int32), ("flags", np.uint8))
NAMES = {"hmd_ft": "hmd", "vmd_ft": "vmd", "vmd_mit_ft": "vmd_mit", "t_cpa": "t_cpa", "t_alert": "t_alert", "flags": "flags", "totals": "totals"}
RESPONSES = [R.DEFAULTS, R.PROMPT]
RESPONSE_IDS = ["the defaults", "at once"]


def _guarded_call(call, outs, n_pairs, n_totals, dev, totals=None):
    """call(**pointers) with every output of `outs` between guard bytes: {name: the output as a numpy array}"""
    import torch
    types = dict(outs)
    size = {name: (n_totals if name == "totals" else n_pairs) * np.dtype(types[name]).itemsize for name in types}
    zero = np.asarray(np.zeros(n_totals) if totals is None else totals, dtype=np.uint64).view(np.uint8)
    bufs = PC.guarded(size, dev, {"totals": zero})
    call(**{name: bufs[name].data_ptr() + PC.GUARD for name in types})
    torch.cuda.synchronize()
    return {name: raw.view(types[name]) for name, raw in PC.payloads(bufs, size).items()}


def _run(a, b, n_a, n_b, n_pairs, idx_a=None, idx_b=None, pose=None, weights=None, want=ALL, totals=None, par=R.DEFAULTS, miss=False,
         well_clear=False):
    """One call on PLANAR host arrays a [P, 3, ld_a], b [P, 3, ld_b]: the wanted outputs as numpy arrays (the others are passed as NULL).
    miss / well_clear: k_miss_distance / k_well_clear too, on the same device inputs and with the same thresholds; returns (k_avoid's
    outputs, theirs ...)."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)          # noqa: E731
    d_a, d_b = up(a, np.float64), up(b, np.float64)
    d_ia, d_ib, d_pose = up(idx_a, np.int64), up(idx_b, np.int64), up(pose, np.float64)
    d_w = None if weights is None else torch.from_numpy(np.asarray(weights, dtype=np.uint32).view(np.int32).copy()).to(dev)
    ptr = lambda t: 0 if t is None else t.data_ptr()          # noqa: E731
    inputs = (ptr(d_a), ptr(d_b), ptr(d_ia), ptr(d_ib), ptr(d_pose), ptr(d_w))
    dims = dict(ld_a=a.shape[2], ld_b=b.shape[2])
    p = native.avoid_params(n_pairs, n_a, n_b, a.shape[0], **dims, **par)
    out = [_guarded_call(lambda **o: native.avoid_device(p, *inputs, **o), [o for o in OUTS if o[0] in want], n_pairs, 12, dev, totals)]
    if miss:
        mp = native.miss_params(n_pairs, n_a, n_b, a.shape[0], par["nmac_h_ft"], par["nmac_v_ft"], **dims)
        out.append(_guarded_call(lambda **o: native.miss_distance_device(mp, *inputs, **o), MISS_OUTS, n_pairs, 8, dev))
    if well_clear:
        wp = native.well_clear_params(n_pairs, n_a, n_b, a.shape[0], par["alert_tau_s"], par["alert_dmod_ft"], par["alert_hmd_ft"],
                                      par["alert_h_ft"], **dims)
        out.append(_guarded_call(lambda **o: native.well_clear_device(wp, *inputs, **o), WC_OUTS, n_pairs, 10, dev))
    return out[0] if len(out) == 1 else tuple(out)


def _check(a, b, n_a, n_b, n_pairs, **kw):
    got = _run(a, b, n_a, n_b, n_pairs, **kw)
    want = R.avoid(a, b, n_a, n_b, n_pairs, idx_a=kw.get("idx_a"), idx_b=kw.get("idx_b"), pose_b=kw.get("pose"), weights=kw.get("weights"),
                   totals=kw.get("totals"), **kw.get("par", R.DEFAULTS))
    PC.same(got, want, list(got))
    return got, want


# ---- 1. tiles and tails
@pytest.mark.parametrize("par", RESPONSES, ids=RESPONSE_IDS)
@pytest.mark.parametrize("P", [1, 2, 3, 5, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_tiles_and_tails(n, P, par):
    plain_a, plain_b = R.encounters(n, P, 1)
    got, want = _check(R.planar(plain_a, n + 3), R.planar(plain_b, n), n, n, n, par=par)        # without a pose
    assert got["totals"][0] == n
    R.check_floors(want, n, P, par)
    rows_a, rows_b, pose = R.posed_encounters(n, P, 1)
    a, b = R.planar(rows_a, n + 3), R.planar(rows_b, n + 9)
    got, want = _check(a, b, n, n, n, pose=pose, par=par)                                       # through a random pose
    assert got["totals"][0] == n
    R.check_floors(want, n, P, par)
    own = R.planar(rows_a[:1], 5)
    _check(own, b, 1, n, n, pose=pose, par=par)                                                 # one ownship
    rs = np.random.RandomState(n * 64 + P)
    m = n + 17
    _check(a, b, n, n, m, idx_a=rs.randint(0, n, m), idx_b=rs.randint(0, n, m), pose=np.ascontiguousarray(pose[:, rs.randint(0, n, m)]), par=par)


# ---- 2. a workgroup that walks two tiles
def test_grid_walk():
    n, P = 2048 * 256 + 300, 3
    rows_a, rows_b = R.encounters(1000, P, 1)
    a, b = R.planar(rows_a), R.planar(rows_b)
    rs = np.random.RandomState(2)
    ia, ib = np.arange(n, dtype=np.int64) % 1000, np.arange(n, dtype=np.int64) % 1000
    w = rs.randint(0, 2**32, n, dtype=np.uint64)
    got, want = _check(a, b, 1000, 1000, n, idx_a=ia, idx_b=ib, weights=w, par=R.PROMPT)
    assert w.max() > 2**32 - 2**20 and got["totals"][0] == n and got["totals"][7] > 2**32
    assert got["totals"][3] > 0 and got["totals"][10] > 2**32 and got["totals"][9] > got["totals"][10]          # some resolved, most not


# ---- 3. the hand-computed cases
@pytest.mark.parametrize("case", R.HAND, ids=[c[0] for c in R.HAND])
def test_hand_computed(case):
    _, (a, b), par = case[:3]
    want = R.hand_want(case)
    got, _ = _check(R.planar(a, 3), R.planar(b, 2), 1, 1, 1, par=par)
    PC.same(got, want, ALL)
    # the same case in lane 70 of 130, between generated pairs
    rows_a, rows_b = (x.copy() for x in R.encounters(130, a.shape[1], 3))
    rows_a[70], rows_b[70] = a[0], b[0]
    got, _ = _check(R.planar(rows_a), R.planar(rows_b), 130, 130, 130, par=par)
    PC.same({k: v[70:71] for k, v in got.items() if k != "totals"}, want, PER_PAIR)


# ---- 4. NaN and inf
def test_nan_and_inf():
    n, P = 300, 24
    rows_a, rows_b, pose = R.posed_encounters(n, P, 4)
    rows_a, rows_b, pose = rows_a.copy(), rows_b.copy(), pose.copy()
    rs = np.random.RandomState(4)
    for bad in (np.nan, np.inf, -np.inf):
        for rows in (rows_a, rows_b):
            rows[rs.randint(0, n, 40), rs.randint(0, P, 40), rs.randint(0, 3, 40)] = bad
    rows_a[7] = np.nan                                   # a pair with no number at all
    rows_a[8], rows_b[8] = R.posed_encounters(n, P, 4)[0][8], R.posed_encounters(n, P, 4)[1][8]
    rows_b[8, :, 0] = np.inf                             # inf at every second and nothing else: every root is inf, a number
    a, b = R.planar(rows_a), R.planar(rows_b)
    for par in RESPONSES:
        got, _ = _check(a, b, n, n, n, par=par)
        assert got["flags"][7] == L.AVOID_NO_CPA and got["t_cpa"][7] == got["t_alert"][7] == -1
        assert np.isnan([got["hmd"][7], got["vmd"][7], got["vmd_mit"][7]]).all()
        assert got["hmd"][8] == np.inf and got["t_cpa"][8] == 0 and got["flags"][8] == 0
    pose[rs.randint(0, 5, 30), rs.randint(9, n, 30)] = np.array([np.nan, np.inf, -np.inf])[rs.randint(0, 3, 30)]          # and in a pose
    got, _ = _check(a, b, n, n, n, pose=pose, par=R.PROMPT)
    assert (got["flags"] == L.AVOID_NO_CPA).sum() > 2 and ((got["flags"] & L.AVOID_ALERTED) != 0).any()


# ---- 5. bad indices
def test_bad_indices_load_nothing_and_leave_their_neighbours_alone():
    n, P = 70, 32
    rows_a, rows_b, pose = R.posed_encounters(n, P, 5)
    a, b = R.planar(rows_a, n + 2), R.planar(rows_b, n)
    ia, ib = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)
    good, _ = _check(a, b, n, n, n, idx_a=ia, idx_b=ib, pose=pose)
    ia[[0, 64]], ia[33], ib[5], ib[69] = -1, n, 2**62, -2**63
    bad = np.zeros(n, dtype=bool)
    bad[[0, 64, 33, 5, 69]] = True
    got, _ = _check(a, b, n, n, n, idx_a=ia, idx_b=ib, pose=pose, weights=np.full(n, 3))
    assert (got["flags"][bad] == L.AVOID_BAD_INDEX).all() and not (got["flags"][~bad] & L.AVOID_BAD_INDEX).any()
    assert np.isnan(got["hmd"][bad]).all() and np.isnan(got["vmd"][bad]).all() and np.isnan(got["vmd_mit"][bad]).all()
    assert (got["t_cpa"][bad] == -1).all() and (got["t_alert"][bad] == -1).all()
    assert got["totals"][6] == 5 and got["totals"][0] == n - 5 and got["totals"][7] == 3 * (n - 5)
    for name in PER_PAIR:
        assert np.array_equal(got[name][~bad], good[name][~bad], equal_nan=True)


# ---- 6. NULL outputs
def test_each_output_alone_and_every_output_but_one():
    n, P = 257, 32
    rows_a, rows_b = R.encounters(n, P, 9)
    a, b = R.planar(rows_a), R.planar(rows_b)
    w = np.random.RandomState(4).randint(0, 1000, n)
    full, _ = _check(a, b, n, n, n, weights=w)
    for name in ALL:
        one = _run(a, b, n, n, n, weights=w, want=(name,))
        PC.same(one, full, (name,))
        rest = tuple(k for k in ALL if k != name)
        PC.same(_run(a, b, n, n, n, weights=w, want=rest), full, rest)


# ---- 7. weights and accumulation
def test_totals_are_added_to():
    n, P = 513, 32
    rows_a, rows_b, pose = R.posed_encounters(n, P, 8)
    a, b = R.planar(rows_a), R.planar(rows_b)
    w = np.array([0, 1, 2**24 - 1, 2**32 - 1], dtype=np.uint64)[np.random.RandomState(3).randint(0, 4, n)]
    start = np.arange(12, dtype=np.uint64) * 1000 + 7
    plain, _ = _check(a, b, n, n, n, pose=pose)
    t = plain["totals"]
    assert t[7] == t[0] == n and t[8] == t[1] > 0 and t[9] == t[2] > 0 and t[10] == t[3] > 0 and t[11] == t[4] and t[5] == t[6] == 0
    got, _ = _check(a, b, n, n, n, pose=pose, weights=w, totals=start)
    PC.same(got, plain, PER_PAIR)                                              # a weight-0 pair is evaluated like any other
    fl = plain["flags"]
    assert np.array_equal(got["totals"][:7], t[:7] + start[:7])
    for k, bit in ((8, L.AVOID_ALERTED), (9, L.AVOID_NMAC_UNMIT), (10, L.AVOID_NMAC_MIT)):
        assert got["totals"][k] - start[k] == w[(fl & bit) != 0].sum(dtype=np.uint64) > 0
    assert got["totals"][7] - start[7] == w.sum(dtype=np.uint64)
    again, _ = _check(a, b, n, n, n, pose=pose, weights=w, totals=got["totals"])
    assert np.array_equal(again["totals"] - got["totals"], got["totals"] - start)


# ---- 8. against k_miss_distance on the same device inputs
@pytest.mark.parametrize("par", RESPONSES, ids=RESPONSE_IDS)
def test_the_unmitigated_part_is_the_miss_kernels(par):
    n, P = 1000, 32
    rows_a, rows_b, pose = R.posed_encounters(n, P, 13)
    a, b = R.planar(rows_a), R.planar(rows_b)
    w = np.random.RandomState(13).randint(1, 2**20, n)
    got, sec = _run(a, b, n, n, n, pose=pose, weights=w, par=par, miss=True)
    PC.same(got, sec, ("hmd", "vmd", "t_cpa"))
    unmit, any_ = (got["flags"] & L.AVOID_NMAC_UNMIT) != 0, (sec["flags"] & L.MISS_NMAC_ANY) != 0
    assert np.array_equal(unmit, any_) and unmit.sum() >= n // 20 and not unmit.all()
    assert got["totals"][2] == sec["totals"][2] == unmit.sum() and got["totals"][9] == sec["totals"][7]
    assert got["totals"][0] == sec["totals"][0] and got["totals"][7] == sec["totals"][5] and got["totals"][5] == sec["totals"][3]


# ---- 9. against k_well_clear with the alert thresholds
@pytest.mark.parametrize("par", [R.DEFAULTS, dict(R.PROMPT, alert_tau_s=35.0, alert_dmod_ft=2500.0, alert_hmd_ft=1500.0, alert_h_ft=450.0)],
                         ids=["the defaults", "a smaller volume"])
def test_the_alert_is_the_loss_of_well_clear_with_the_alert_thresholds(par):
    n, P = 1000, 64
    rows_a, rows_b, pose = R.posed_encounters(n, P, 14)
    a, b = R.planar(rows_a), R.planar(rows_b)
    got, wc = _run(a, b, n, n, n, pose=pose, par=par, well_clear=True)
    alerted = (got["flags"] & L.AVOID_ALERTED) != 0
    assert np.array_equal(got["t_alert"], wc["t_first"]) and np.array_equal(alerted, (wc["flags"] & L.WC_LOST) != 0)
    assert alerted.sum() >= n // 20 and not alerted.all() and (got["t_alert"] > 0).sum() >= n // 20


# ---- 10. a manoeuvre that goes nowhere
@pytest.mark.parametrize("par", [dict(R.DEFAULTS, rate_fps=0.0), dict(R.PROMPT, rate_fps=0.0), dict(R.PROMPT, dz_max_ft=0.0)],
                         ids=["rate 0", "rate 0 at once", "dz_max 0"])
def test_a_zero_rate_changes_nothing(par):
    n, P = 1000, 32
    rows_a, rows_b = R.encounters(n, P, 15)
    got, _ = _check(R.planar(rows_a), R.planar(rows_b), n, n, n, par=par)
    PC.same({"vmd_mit": got["vmd_mit"]}, {"vmd_mit": got["vmd"]}, ("vmd_mit",))
    fl = got["flags"]
    assert np.array_equal((fl & L.AVOID_NMAC_MIT) != 0, (fl & L.AVOID_NMAC_UNMIT) != 0)
    assert got["totals"][4] == got["totals"][11] == 0 and got["totals"][3] == got["totals"][2] > 0 and got["totals"][1] > 0


# ---- 11. the Python surface
def _as_ref(res):
    return {NAMES[k]: v for k, v in res.items() if k in NAMES}


def _derived(res, want):
    fl, tot = want["flags"], want["totals"]
    assert res["hmd_ft"].dtype == res["vmd_mit_ft"].dtype == np.float64 and res["t_cpa"].dtype == res["t_alert"].dtype == np.int32
    assert res["flags"].dtype == np.uint8 and res["totals"].shape == (12,) and res["totals"].dtype == np.uint64
    for key, bit in (("alerted", R.ALERTED), ("climb", R.CLIMB), ("nmac", R.NMAC_UNMIT), ("nmac_mit", R.NMAC_MIT)):
        assert res[key].dtype == bool and np.array_equal(res[key], (fl & bit) != 0)
    assert np.array_equal(res["induced"], ((fl & R.NMAC_MIT) != 0) & ((fl & R.NMAC_UNMIT) == 0))
    assert res["risk_ratio"] == float(tot[10]) / float(tot[9]) and 0.0 < res["risk_ratio"] < 1.0


def test_avoid_on_numpy_and_torch_inputs_and_a_contexts_stream(gpu_ctx):
    import torch
    n, P = 300, 32
    rows_a, rows_b, pose = R.posed_encounters(n, P, 10)
    w = np.random.RandomState(10).randint(1, 2**16, n)
    pl_a, pl_b = R.planar(rows_a), R.planar(rows_b)
    want = R.avoid(pl_a, pl_b, n, n, n, pose_b=pose, weights=w)
    side = torch.cuda.Stream()
    ctx = native.Context(0, stream=side.cuda_stream)
    for res in (native.avoid(rows_a, rows_b, pose_b=pose, weights=w),                                            # numpy rows
                native.avoid(pl_a, pl_b, pose_b=pose, weights=w, layout="planar"),                               # numpy planar
                native.avoid(torch.from_numpy(pl_a).cuda(), torch.from_numpy(pl_b).cuda(), pose_b=torch.from_numpy(pose).cuda(), weights=w,
                             layout="planar"),                                                                   # torch device tensors
                native.avoid(rows_a, rows_b, pose_b=pose, weights=w, ctx=gpu_ctx),                               # a context on its own stream
                native.avoid(rows_a, rows_b, pose_b=pose, weights=w, ctx=ctx),                                   # a context that was given one
                native.avoid(rows_a, rows_b, pose_b=pose, weights=w, stream=0)):                                 # the HIP default stream
        PC.same(_as_ref(res), want, ALL)
        _derived(res, want)
    other = dict(alert_tau_s=40.0, alert_dmod_ft=2500.0, alert_hmd_ft=1500.0, alert_h_ft=450.0, nmac_h_ft=600.0, nmac_v_ft=150.0, delay_s=2,
                 rate_fps=40.0, accel_fps2=16.0, dz_max_ft=300.0)
    PC.same(_as_ref(native.avoid(rows_a, rows_b, pose_b=pose, **other)), R.avoid(pl_a, pl_b, n, n, n, pose_b=pose, **other), ALL)
    none = native.avoid(rows_a[:4], rows_b[:4] + 1.0e6)                              # nothing near: no NMAC, no ratio
    assert none["totals"][9] == 0 and np.isnan(none["risk_ratio"])


def test_the_placed_forms_and_the_models_method(model_dir):
    from em_model_manned_bayes_amd import em_io
    n, P = 600, 32
    rows_a, rows_b = R.encounters(n, P, 11)
    pl_a, pl_b = R.planar(rows_a), R.planar(rows_b)
    w = np.random.RandomState(11).randint(1, 2**16, n)
    resp = dict(R.DEFAULTS, delay_s=2)
    for placed, pose_of, extra, kw in (
            (native.encounter_avoid, native.encounter_pose, {"rate", "encounter_flags", "weights"},
             dict(radius_ft=12000.0, half_height_ft=800.0, seed=0x41)),
            (native.cpa_avoid, native.cpa_pose, {"rate", "t_cpa_drawn", "encounter_flags", "weights"},
             dict(hmd_max_ft=800.0, vmd_max_ft=200.0, seed=0x41, t_lo=3, t_hi=28))):
        one = placed(rows_a, rows_b, weights=w, rate_scale=4.0e9, **kw, **resp)
        pose = pose_of(rows_a, rows_b, weights=w, rate_scale=4.0e9, **kw)
        want = R.avoid(pl_a, pl_b, n, n, n, pose_b=pose["pose"], weights=pose["weights"], **resp)
        PC.same(_as_ref(one), want, ALL)
        assert set(one) == set(NAMES) | {"alerted", "climb", "nmac", "nmac_mit", "induced", "risk_ratio"} | extra
        assert np.array_equal(one["rate"], pose["rate"]) and np.array_equal(one["weights"], pose["weights"])
        assert one["totals"][7] == pose["weights"].sum(dtype=np.uint64) and one["alerted"].any()
        if placed is native.cpa_avoid:
            assert np.array_equal(one["t_cpa_drawn"], pose["t_cpa"])
            _derived(one, want)                                                      # every pair passes close by: some NMACs, some resolved
    mdl = E.UncorEncounterModel(parameters_filename=em_io.materialize_model("uncor_1200code_v2p1", model_dir))
    rows_a, rows_b, pose = R.posed_encounters(n, P, 12)
    got = mdl.avoid(rows_a, rows_b, pose=pose, weights=w, delay_s=3)
    want = R.avoid(R.planar(rows_a), R.planar(rows_b), n, n, n, pose_b=pose, weights=w, **dict(R.DEFAULTS, delay_s=3))
    PC.same(_as_ref(got), want, ALL)
    _derived(got, want)
