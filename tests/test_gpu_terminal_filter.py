"""-m gpu: k_terminal_filter and k_terminal_smooth on hand-made tracks, through emgpu_filter_terminal_device and
emgpu_smooth_terminal_device.

The encounters are terminal_filter_cases.py's: pairs around one accepted base encounter that differ in one quantity and are decided by one
named filter, most of them with that quantity ON its threshold on one side and one f32 step off on the other (test_terminal_filter.py shows
on the CPU that they are what they claim).  The reference is the C oracle's O.terminal_filters on the very same rows, never the kernel.

The comparison rule: the inputs are exact in f32 and so the same numbers on both sides; both sides round every f64 operation once, with
contraction off, and the f64 square root is correctly rounded on both, so for an accepted encounter meta (tcpa, hmd, vmd, enc_time), len and
traj are compared BIT FOR BIT; hypot and asin, which are not pinned, only feed compares that the cases keep away from their thresholds.  A
rejected encounter's outputs must keep the bytes they held.  Every output lies between guard bytes that must stay, and every row of a
block outside a track's span holds NaN, which poisons whatever reads it."""
import numpy as np
import pytest

import pair_cases as PC
import terminal_filter_cases as K
import terminal_filter_ref as R
from em_model_manned_bayes_amd import native

pytestmark = pytest.mark.gpu

OUTS = ("meta", "len", "traj")
DTYPES = {"accepted": np.uint8, "meta": np.float64, "len": np.int32, "traj": np.float64, "tracks": np.float32}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _filter(sides, opts, cap2=None, want=OUTS, fill=np.nan, blocks=None):
    """one launch of k_terminal_filter on the sides (all of the launch options `opts`): {accepted, and the wanted outputs}, reshaped.
    blocks: (tracks, rows) to read instead of the packed sides' (the chain test's smoothed blocks)"""
    import torch
    n, cap = len(sides), opts["cap"]
    cap2 = 2 * cap if cap2 is None else cap2
    geo, tracks, rows = K.pack(sides, cap, fill=fill)
    if blocks is not None:
        tracks, rows = blocks
    d_geo, d_tracks, d_rows = (torch.from_numpy(a).to(_dev()) for a in (geo, tracks, rows))
    sizes = {"accepted": n, "meta": n * 32, "len": n * 8, "traj": n * 2 * cap2 * 48}
    sizes = {k: v for k, v in sizes.items() if k == "accepted" or k in want}
    bufs = PC.guarded(sizes, _dev())
    p = native.terminal_filter_params(n, cap, opts["dl"], opts["cum"], opts["pitch"], cap2=cap2, min_enc_time_s=opts["min_enc"], thres_dist_ft=opts["dist"],
                                      thres_alt_low_ft=opts["alt_low"], thres_vertrate_ft_s=opts["vrate"])
    native.filter_terminal_device(p, d_geo.data_ptr(), d_tracks.data_ptr(), d_rows.data_ptr(), **{k: bufs[k].data_ptr() + PC.GUARD for k in sizes})
    torch.cuda.synchronize()
    shapes = {"accepted": (n,), "meta": (n, 4), "len": (n, 2), "traj": (n, 2, cap2, 6)}
    return {k: raw.view(DTYPES[k]).reshape(shapes[k]) for k, raw in PC.payloads(bufs, sizes).items()}


def _same_bits(got, want, names, what):
    for k in names:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k)
        bits = {1: np.uint8, 4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
        diff = np.argwhere(g.view(bits) != w.view(bits))
        if len(diff):
            at = tuple(diff[0])
            raise AssertionError("%s: %s differs in %d places, first at %s: got %r, want %r (%d apart in bits)"
                                 % (what, k, len(diff), at, g[at], w[at], abs(int(g.view(bits)[at]) - int(w.view(bits)[at]))))


def _check(sides, opts, what, **kw):
    got = _filter(sides, opts, **kw)
    cap2 = kw.get("cap2")
    want = R.expected(sides, 2 * opts["cap"] if cap2 is None else cap2)
    wrong = np.flatnonzero(got["accepted"] != want["accepted"])
    assert wrong.size == 0, "%s: sides %s decided differently from the oracle (device %s)" % (what, wrong.tolist(), got["accepted"][wrong].tolist())
    _same_bits(got, want, [k for k in got if k != "accepted"], what)
    return got


@pytest.mark.parametrize("family", K.FAMILIES)
def test_decisions_and_outputs_of_a_family(family):
    """every side of the family's cases, one launch per set of launch options: the oracle's decision, and the oracle's outputs to the bit"""
    for opts, group in K.batches(K.sides_of(family)):
        _check(group, opts, family)
    for c in K.CASES:                                       # what _check compared with, said per case
        if c["family"] == family:
            assert [R.oracle(s)[0] for s in c["sides"]] == [True, False], c["name"]


def _default_batch():
    opts, sides = K.batches(K.sides_of())[0]
    assert opts == K.DEFAULT and len(sides) >= 60
    return opts, sides


def _tiled(n):
    opts, sides = _default_batch()
    return opts, [sides[i % len(sides)] for i in range(n)]


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, 1025))
def test_lanes_and_blocks(n):
    opts, sides = _tiled(n)
    got = _check(sides, opts, "n = %d" % n)
    if n == 257:      # what lies outside the spans changes nothing: zeros and a large number instead of the NaN poison
        for fill in (0.0, 3.0e38):
            other = _filter(sides, opts, fill=fill)
            _same_bits(other, got, list(got), "fill %r" % fill)
        assert 0 < got["accepted"].sum() < n


def test_cap2_smaller_than_a_track_writes_cap2_rows_and_the_full_length():
    opts, sides = _tiled(70)
    for cap2 in (1, 10, 40):
        got = _check(sides, opts, "cap2 = %d" % cap2, cap2=cap2)
        acc = got["accepted"] == 1
        assert acc.any() and (got["len"][acc] > cap2).any()


def test_each_output_may_be_null_alone():
    opts, sides = _tiled(70)
    for missing in OUTS:
        want = tuple(k for k in OUTS if k != missing)
        got = _check(sides, opts, "without " + missing, want=want)
        assert set(got) == set(want) | {"accepted"}
    _check(sides, opts, "accepted alone", want=())


# ---- k_terminal_smooth
def _smooth(tracks, rows, cap):
    import torch
    size = {"tracks": tracks.nbytes}
    bufs = PC.guarded(size, _dev(), {"tracks": tracks.view(np.uint8).reshape(-1)})
    d_rows = torch.from_numpy(rows).to(_dev())
    native.smooth_terminal_device(tracks.shape[0], cap, bufs["tracks"].data_ptr() + PC.GUARD, d_rows.data_ptr())
    torch.cuda.synchronize()
    return PC.payloads(bufs, size)["tracks"].view(np.float32).reshape(tracks.shape)


def _check_smooth(shapes, cap, seed):
    tracks, rows = K.smooth_block(shapes, cap, seed)
    got, want = _smooth(tracks, rows, cap), R.smoothed(tracks, rows, cap)
    # speed and altitude: f32 of the oracle's f64 window means; x, y, heading, the rows outside the spans (NaN) and void tracks: as they were
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), "cap %d: first difference at (track, row, field) %s, shape %s" % (cap, tuple(np.argwhere(~same)[0]), shapes[np.argwhere(~same)[0][0]])
    keep = np.ones(tracks.shape, dtype=bool)
    keep[:, :, [2, 4]] = False
    assert np.array_equal(got.view(np.uint32)[keep], tracks.view(np.uint32)[keep])
    return tracks, got


SMOOTH_CAP_LIST = sorted(set(K.SMOOTH_CAPS) | {max(rf, rb, 2) for rf, rb in K.SMOOTH_SHAPES})


@pytest.mark.parametrize("cap", SMOOTH_CAP_LIST)
def test_smooth_shapes_and_caps(cap):
    """every (rf, rb) of the list that fits the cap, a void track beside live ones in the first workgroup (four tracks each)"""
    fit = [s for s in K.SMOOTH_SHAPES if max(s) <= cap]
    shapes = fit[:1] + [(-1, min(cap, 5))] + fit[1:] + [(min(cap, 3), 0)]
    tracks, got = _check_smooth(shapes, cap, cap)
    for a in (1, len(shapes) - 1):
        assert np.array_equal(got[a].view(np.uint32), tracks[a].view(np.uint32))          # the void tracks' blocks, values all over, stayed
    if cap >= 3:
        assert not np.array_equal(got.view(np.uint32), tracks.view(np.uint32))            # (a track of three rows has a window of three)


def test_smooth_covers_the_issue_s_lists():
    assert set(K.SMOOTH_SHAPES) == {(1, 1), (2, 1), (1, 2), (3, 1), (3, 3), (8, 8), (15, 1), (16, 16), (64, 1), (33, 33), (128, 128), (125, 125), (1, 128)}
    assert set(K.SMOOTH_CAPS) == {2, 8, 123, 125} <= set(SMOOTH_CAP_LIST) and max(SMOOTH_CAP_LIST) == 128


@pytest.mark.parametrize("n2", (1, 2, 3, 4, 5, 1023))
def test_smooth_track_counts(n2):
    fit = [s for s in K.SMOOTH_SHAPES if max(s) <= 16]
    shapes = [(0, 4) if i % 7 == 2 else fit[i % len(fit)] for i in range(n2)]
    _check_smooth(shapes, 16, 100 + n2)


# ---- the chain: smooth, then filter, the order CorTerminalModel.track runs them in
def test_smooth_then_filter_is_the_oracle_s_chain():
    by_name = {c["name"]: c for c in K.CASES}
    sides = [K.BASE, by_name["descent_exactly_5_fraction_8_7"]["sides"][0], by_name["own_floor_750_next"]["sides"][1]]
    assert all(s["opts"] == K.DEFAULT for s in sides)
    cap = K.DEFAULT["cap"]
    geo, tracks, rows = K.pack(sides, cap)
    rows2 = rows.reshape(-1, 2).reshape(-1)                 # [4n] is [2n][2]: forward, backward per aircraft
    on_device = _smooth(tracks, rows2, cap)
    want_blocks = R.smoothed(tracks, rows2, cap)
    assert np.array_equal(on_device.view(np.uint32), want_blocks.view(np.uint32))
    smoothed_sides = [dict(s, own=o, intr=i) for s, (o, i) in zip(sides, K.unpack(want_blocks, rows, cap))]
    got = _filter(sides, K.DEFAULT, blocks=(on_device, rows))
    want = R.expected(smoothed_sides, 2 * cap)
    assert np.array_equal(got["accepted"], want["accepted"]) and 0 < want["accepted"].sum() < len(sides), (got["accepted"], want["accepted"])
    _same_bits(got, want, OUTS, "chain")
    assert not np.array_equal(want_blocks.view(np.uint32), tracks.view(np.uint32))
