"""-m gpu: the host code around the track kernels -- the rejection-round loop both .track drivers iterate over (RejectionRounds in
emgpu_rounds.hpp), the copy-back that keeps the rounds' message, and the terminal encounter chain's kernel names and smoothing-cap refusal.

The uncor case is small enough for the CPU oracle to name every lane: n = 257, T = 30, record_stride = 10, seed 0xC0DE, first_index 0 on
uncor_1200code_v2p1.  O.uncor_track accepts 243 lanes at attempt 1, 12 at attempt 2 and 2 (lanes 126 and 154) at attempt 3, so rounds 0, 1
and 2 run and both halves of the (index, slot) ping-pong are written and read; its smallest decision margin is 1.3e-5, four orders above
the 1e-9 of assert_parting_only_on_a_threshold, so no lane may part and attempts are compared with array_equal."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import em_model_manned_bayes_amd as E
from em_model_manned_bayes_amd import native, _lib as L
from util import load_pair

pytestmark = pytest.mark.gpu

NAME, N, T, STRIDE, SEED = "uncor_1200code_v2p1", 257, 30, 10, 0xC0DE
S = 10 * T // STRIDE + 1
ROUND0_REJECTS = [5, 18, 25, 42, 45, 73, 126, 154, 192, 208, 212, 228, 232, 233]
ROUND1_REJECTS = [126, 154]
CAPS = (1, 2, 3, 200)
LEFT = {1: 14, 2: 2, 3: 0, 200: 0}           # lanes the oracle leaves at -1 under each cap

# emgpu_last_kernel_name as the parent of the refactor (b976646) reported it, recorded in the same GPU job as the first run of this file
UNCOR_KERNELS = "k_uncor_fast_idx<7,2,4,2> + k_uncor_track<fastbank>"
TERMINAL_KERNELS = {
    ("sample", False): "k_bn<16> + k_terminal_geo + k_terminal_propagate<35,6,4>",
    ("sample", True): "k_bn<16> + k_terminal_geo + k_terminal_smooth + k_terminal_propagate<35,6,4>",
    ("propagate", False): "k_terminal_propagate<35,6,4>",
    ("propagate", True): "k_terminal_propagate<35,6,4> + k_terminal_smooth",
    ("track", False): "k_bn<16> + k_terminal_propagate<35,6,4> + k_terminal_filter",
    ("track", True): "k_bn<16> + k_terminal_propagate<35,6,4> + k_terminal_smooth + k_terminal_filter",
}


def _params(nm, n, first, cap):
    return native.utrack_params(nm, n, T, SEED, first_index=first, is_rotorcraft=False, max_track_attempts=cap, record_stride=STRIDE)


def uncor_host(ctx, nm, n, first, cap):
    """emgpu_track_uncor_host through the library itself: the arrays survive the status."""
    p = _params(nm, n, first, cap)
    tracks, limits, att = np.full((n, S, 8), np.nan), np.full((n, 3), np.nan), np.full(n, -7, dtype=np.int32)
    rc = L.lib().emgpu_track_uncor_host(ctx._h, nm._h, C.byref(p), tracks.ctypes.data, limits.ctypes.data, att.ctypes.data)
    return rc, L.lib().emgpu_last_error().decode(), tracks, limits, att, ctx.last_kernel()


def uncor_device(ctx, nm, n, first, cap):
    """emgpu_track_uncor_device into torch buffers prefilled with NaN / -7."""
    import torch
    dev = torch.device("cuda", 0)
    tracks = torch.full((n, S, 8), float("nan"), dtype=torch.float64, device=dev)
    limits = torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev)
    att = torch.full((n,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    p = _params(nm, n, first, cap)
    rc = L.lib().emgpu_track_uncor_device(ctx._h, nm._h, C.byref(p), C.c_void_p(tracks.data_ptr()), C.c_void_p(limits.data_ptr()), C.c_void_p(att.data_ptr()))
    msg = L.lib().emgpu_last_error().decode()
    ctx.sync()
    return rc, msg, tracks.cpu().numpy(), limits.cpu().numpy(), att.cpu().numpy(), ctx.last_kernel()


@pytest.fixture(scope="module")
def uncor(gpu_ctx, model_dir):
    """The model, the oracle's attempts per cap and both entry points' results per cap: computed once, read by every test."""
    nm, pp, _ = load_pair(NAME, model_dir)
    om = O.OracleModel(pp)
    ref = {k: O.uncor_track(om, N, T, SEED, first_index=0, is_rotorcraft=False, max_track_attempts=k, want_tracks=False) for k in CAPS}
    return {"nm": nm, "ref": ref, "host": {k: uncor_host(gpu_ctx, nm, N, 0, k) for k in CAPS},
            "device": {k: uncor_device(gpu_ctx, nm, N, 0, k) for k in CAPS}}


def test_the_oracle_runs_three_rounds_on_these_lanes(uncor):
    """What the cases below rest on, from the oracle alone: which lanes each round rejects, and the margin that lets attempts be compared
    lane for lane."""
    a = uncor["ref"][200]["attempts"]
    assert [(a == j).sum() for j in (1, 2, 3)] == [243, 12, 2] and a.max() == 3
    assert np.flatnonzero(a > 1).tolist() == ROUND0_REJECTS and np.flatnonzero(a > 2).tolist() == ROUND1_REJECTS
    for k in CAPS:
        assert (uncor["ref"][k]["attempts"] == -1).sum() == LEFT[k]
    m = uncor["ref"][200]["margins"]
    assert np.nanmin(m) > 1e-5, np.nanmin(m)


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("k", CAPS)
def test_uncor_rounds_at_the_caps(uncor, entry, k):
    """max_track_attempts = k through emgpu_track_uncor_device / _host: the status, the message after the host's copy-back, the oracle's
    attempts at the same cap (-1 for the lanes left rejected), and accepted lanes bit-equal to the k = 200 run."""
    rc, msg, tracks, limits, att, _ = uncor[entry][k]
    want = uncor["ref"][k]["attempts"]
    print(entry, k, "rc", rc, "msg", repr(msg), "left", int((att == -1).sum()))
    assert rc == (L.ERR_REJECT_CAP if LEFT[k] else L.OK), (rc, msg)
    if LEFT[k]:
        assert msg == "track: %d trajectories were still rejected after max_track_attempts" % LEFT[k], msg
    assert np.array_equal(att, want), np.flatnonzero(att != want)
    rejected = np.flatnonzero(want == -1)
    assert rejected.tolist() == {1: ROUND0_REJECTS, 2: ROUND1_REJECTS}.get(k, []) and np.all(att[rejected] == -1)
    ok = want > 0
    _, _, tracks200, limits200, att200, _ = uncor[entry][200]
    assert np.array_equal(att[ok], att200[ok])
    assert not np.isnan(tracks[ok]).any() and not np.isnan(limits[ok]).any()
    assert np.array_equal(tracks[ok], tracks200[ok]) and np.array_equal(limits[ok], limits200[ok])


def test_uncor_entry_points_agree_and_name_their_kernels(uncor):
    _, _, th, lh, ah, kh = uncor["host"][200]
    _, _, td, ld, ad, kd = uncor["device"][200]
    assert np.array_equal(th, td) and np.array_equal(lh, ld) and np.array_equal(ah, ad)
    print("kernel", repr(kh), repr(kd))
    assert kh == UNCOR_KERNELS and kd == UNCOR_KERNELS


@pytest.mark.parametrize("lo,n", [(0, 63), (126, 1)])
def test_uncor_rounds_do_not_depend_on_the_batch_cut(uncor, gpu_ctx, lo, n):
    """Lanes [0, 63) (five of them redrawn in round 1) and lane 126 alone (three rounds of one lane) as calls of their own: the big call's rows."""
    _, _, tracks, limits, att, _ = uncor["host"][200]
    rc, msg, tp, lp, ap, _ = uncor_host(gpu_ctx, uncor["nm"], n, lo, 200)
    assert rc == L.OK, msg
    sl = slice(lo, lo + n)
    assert (att[sl] > 1).any()
    assert np.array_equal(ap, att[sl]) and np.array_equal(tp, tracks[sl]) and np.array_equal(lp, limits[sl])


# ------------------------------------------------------------------------------------------------ the terminal chain
TN, TSEED = 120, 0xF3


@pytest.fixture(scope="module")
def terminal(tmp_path_factory):
    from em_model_manned_bayes_amd import synthetic
    t = E.CorTerminalModel(srcData="terminalradar", parameters_directory=synthetic.write_terminal_directory(str(tmp_path_factory.mktemp("terminal"))))
    t.acType1, t.acType2 = "GENERIC", "GENERIC"
    return t


class _Buffers:
    """The device buffers of a terminal call of TN encounters with `cap` rows per direction, prefilled with sentinels."""

    def __init__(self, t, cap):
        import torch
        dev, ni, c0 = torch.device("cuda", 0), t.native.n_initial, native.terminal_t0_row(cap)
        self.gval = torch.full((ni, TN), float("nan"), dtype=torch.float32, device=dev)
        self.geo = torch.full((TN, 12), float("nan"), dtype=torch.float64, device=dev)
        self.mof = torch.full((4 * TN,), -7, dtype=torch.int32, device=dev)
        self.traj = torch.full((2 * TN, 2 * c0, 5), float("nan"), dtype=torch.float32, device=dev)
        self.rows = torch.full((4 * TN,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

    def untouched(self):
        import torch
        return (bool(torch.isnan(self.gval).all()) and bool(torch.isnan(self.geo).all()) and bool(torch.isnan(self.traj).all())
                and bool((self.mof == -7).all()) and bool((self.rows == -7).all()))


def _sample(ctx, t, b, cap, smooth):
    """emgpu_sample_terminal_device: the status (the context synchronized)."""
    p, keep = native.terminal_sample_params(t.native, TN, TSEED, t._dyn_rows(), cap=cap, local_smooth=smooth)
    handles = (C.c_void_p * 10)(*[m.native._h for m in t._traj])
    rc = L.lib().emgpu_sample_terminal_device(ctx._h, t.native._h, handles, 10, C.byref(p), None, C.c_void_p(b.gval.data_ptr()), C.c_void_p(b.geo.data_ptr()),
                                              C.c_void_p(b.mof.data_ptr()), C.c_void_p(b.traj.data_ptr()), C.c_void_p(b.rows.data_ptr()), None)
    msg = L.lib().emgpu_last_error().decode()
    ctx.sync()
    return rc, msg


def _propagate(ctx, t, geo, mof, b, cap, smooth):
    """emgpu_propagate_terminal_device on the geometry of an earlier call."""
    p = L.TermParams()
    p.seed, p.first_index, p.n, p.tmax_s, p.max_resample, p.cap = TSEED, 0, TN, 120.0, 100000, cap
    p.flags = L.FLAG_LOCAL_SMOOTH if smooth else 0
    for i, v in enumerate(np.asarray(t._dyn_rows(), dtype=np.float64).reshape(-1)):
        p.dyn_limits[i] = float(v)
    handles = (C.c_void_p * 10)(*[m.native._h for m in t._traj])
    rc = L.lib().emgpu_propagate_terminal_device(ctx._h, handles, 10, C.byref(p), C.c_void_p(geo.data_ptr()), C.c_void_p(mof.data_ptr()),
                                                 C.c_void_p(b.traj.data_ptr()), C.c_void_p(b.rows.data_ptr()))
    msg = L.lib().emgpu_last_error().decode()
    ctx.sync()
    return rc, msg


def terminal_kernel_names(ctx, t):
    """{(entry point, local_smooth): emgpu_last_kernel_name} of the three terminal entry points, and the sampler's launch counts."""
    names, launches = {}, {}
    d = (t.dynLimits1, t.dynLimits2)
    for smooth in (False, True):
        b = _Buffers(t, 123)
        rc, msg = _sample(ctx, t, b, 123, smooth)
        assert rc == L.OK, msg
        names["sample", smooth], launches[smooth] = ctx.last_kernel(), ctx.last_launches()
        again = _Buffers(t, 123)
        rc, msg = _propagate(ctx, t, b.geo, b.mof, again, 123, smooth)
        assert rc == L.OK, msg
        names["propagate", smooth] = ctx.last_kernel()
        got = native.track_terminal_host(ctx, t.native, [m.native for m in t._traj], TN, TSEED, t._dyn_rows(), [x["maxCumTurn_deg"] for x in d],
                                         [x["pitch_deg"] for x in d], max_track_attempts=150, allow_cap=True, local_smooth=smooth, want_traj=False)
        names["track", smooth] = got["kernel"]
    return names, launches


def test_terminal_entry_points_name_their_kernels(gpu_ctx, terminal):
    names, launches = terminal_kernel_names(gpu_ctx, terminal)
    print(names, launches)
    assert names == TERMINAL_KERNELS
    assert launches == {False: 3, True: 4}


def test_smoothing_above_its_cap_is_refused_before_anything_is_launched(gpu_ctx, terminal):
    """EMGPU_FLAG_LOCAL_SMOOTH with cap = 129 (EMGPU_TERMINAL_BLOCK_ROWS = 272 > 256): the fused sampler and the propagation both return
    EMGPU_ERR_UNSUPPORTED and write nothing."""
    good = _Buffers(terminal, 123)
    rc, msg = _sample(gpu_ctx, terminal, good, 123, False)
    assert rc == L.OK, msg
    b = _Buffers(terminal, 129)
    rc, msg = _sample(gpu_ctx, terminal, b, 129, True)
    assert rc == L.ERR_UNSUPPORTED and msg == "EMGPU_FLAG_LOCAL_SMOOTH: cap above 128", (rc, msg)
    assert b.untouched()
    rc, msg = _propagate(gpu_ctx, terminal, good.geo, good.mof, b, 129, True)
    assert rc == L.ERR_UNSUPPORTED and msg == "EMGPU_FLAG_LOCAL_SMOOTH: cap above 128", (rc, msg)
    assert b.untouched()
