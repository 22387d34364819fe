"""Hand-made encounters for k_terminal_filter and k_terminal_smooth, shared by test_terminal_filter.py (CPU) and
test_gpu_terminal_filter.py: the tracks, the packer into k_terminal_propagate's block layout and the list of cases.  It never imports the
library.

A track is rows [t_s x_nm y_nm z_ft heading_deg v_ft_s] at consecutive integer seconds through t = 0, every value exactly representable in
f32 (track() asserts it), so the f32 blocks the device reads and the f64 rows the references read hold the same numbers.  A SIDE is one
encounter: two tracks, two intents and the launch options.  A CASE is a pair of sides around the accepted base encounter that differ in one
quantity; it names the one filter (FILTERS) that is meant to decide between them and is accepted on exactly one side.

What the layout cannot express: two tracks without a common second.  A block holds second t in row C + t and a live track has at least one
row in each direction, so every live track holds t = 0 and nc >= 1; the kernel's `nc <= 0` branch is as unreachable as its `m > 248` one
(test_terminal_filter.py holds the two references against each other there, NO_COMMON)."""
import numpy as np

F32 = np.float32
INF = float("inf")
FILTERS = ("void", "cpa", "enc_time", "prox_own", "prox_int", "vert_own", "vert_int", "heading", "limits_own", "limits_int", "cum_own", "cum_int")

# launch options: the block's rows per direction, per aircraft minVel maxVel maxTurnRate maxAltitude maxVertRate, then track.m:14-17
DEFAULT = dict(cap=48, dl=((100.0, 300.0, 12.0, 5000.0, 50.0), (50.0, 250.0, 12.0, 5000.0, 12.0)), cum=(180.0, 180.0), pitch=(10.0, 10.0),
               min_enc=30.0, dist=2.5 * 6076, alt_low=750.0, vrate=5.0)


def up(x):
    """the next f32 above x, as a float"""
    return float(np.nextafter(F32(x), F32(np.inf)))


def down(x):
    return float(np.nextafter(F32(x), F32(-np.inf)))


def t0_row(cap):
    return (int(cap) + 7) & ~7                       # EMGPU_TERMINAL_T0_ROW


def track(t0, t1, x, y, z, h, v):
    """rows [t1 - t0 + 1, 6] f64 for t = t0..t1; a column is a number, an array or a function of the times"""
    assert t0 <= 0 <= t1
    t = np.arange(t0, t1 + 1, dtype=np.float64)
    cols = [t] + [np.broadcast_to(np.asarray(c(t) if callable(c) else c, dtype=np.float64), t.shape) for c in (x, y, z, h, v)]
    rows = np.ascontiguousarray(np.stack(cols, axis=1))
    assert np.array_equal(rows, rows.astype(F32).astype(np.float64)), "a value is not exact in f32"
    rows.setflags(write=False)
    return rows


def own(t0=-20, t1=20, z=None, h=90.0, v=190.0, y=0.0):
    """the base ownship: landing, heading 90, 190 ft/s along x (1/32 nm per second), 900 ft at t = 0 descending 8 ft/s"""
    return track(t0, t1, lambda t: t / 32.0, y, (lambda t: 900.0 - 8.0 * t) if z is None else z, h, v)


def intr(t0=-15, t1=25, tc=0, z=2500.0, h=200.0, v=95.0, y0=0.0):
    """the base intruder: in transit, level at 2500 ft, beside the ownship: 0.375 nm ahead and 1 + |t - tc| / 64 nm abeam, so that the
    horizontal distance has its minimum at second tc (several tc: equal minima at each) and an inexact square root at every second"""
    tcs = np.atleast_1d(np.asarray(tc, dtype=np.float64))
    return track(t0, t1, lambda t: t / 32.0 + 0.375, lambda t: y0 + 1.0 + np.abs(t[:, None] - tcs[None, :]).min(axis=1) / 64.0, z, h, v)


def steps(first, d):
    """a column from its first value and its differences"""
    return np.concatenate([[first], first + np.cumsum(np.asarray(d, dtype=np.float64))])


def side(own_rows=None, intr_rows=None, intents=(1, 3), void=None, **opts):
    """one encounter.  void: (k, value) puts `value` into entry k of its four row counts (own fwd, own bck, int fwd, int bck)"""
    assert set(opts) <= set(DEFAULT)
    o = dict(DEFAULT, **opts)
    s = dict(own=own() if own_rows is None else own_rows, intr=intr() if intr_rows is None else intr_rows, intents=tuple(intents), void=void, opts=o,
             key=tuple(sorted(o.items())))
    for rows in (s["own"], s["intr"]):
        assert -rows[0, 0] + 1 <= o["cap"] and rows[-1, 0] + 1 <= o["cap"]
    return s


BASE = side()
CASES = []


def case(family, name, filt, a, b):
    assert filt in FILTERS and name not in {c["name"] for c in CASES}
    CASES.append(dict(family=family, name=name, filter=filt, sides=(a, b)))


def _cpa():
    case("cpa", "tcpa_10_11", "cpa", side(intr_rows=intr(tc=10)), side(intr_rows=intr(tc=11)))
    case("cpa", "tcpa_m10_m11", "cpa", side(intr_rows=intr(tc=-10)), side(intr_rows=intr(tc=-11)))
    # two equal minima, the first wins: (3, 12) is decided at 3 and accepted, (-12, 3) at -12 and rejected
    case("cpa", "equal_minima_first_wins", "cpa", side(intr_rows=intr(tc=(3, 12))), side(intr_rows=intr(tc=(-12, 3))))
    case("cpa", "equal_minima_both_inside", "cpa", side(intr_rows=intr(tc=(-9, 3))), side(intr_rows=intr(tc=(-12, -11))))
    # the spans overlap in second 0 only; the closest approach of the longer overlap lies at -11
    short = lambda t: 740.0 - 8.0 * t          # noqa: E731  (the ownship ends at t = 0, and low)
    case("cpa", "one_common_second", "cpa", side(own(-20, 0, z=short), intr(0, 40, tc=-11), min_enc=1.0),
         side(own(-20, 0, z=short), intr(-15, 40, tc=-11), min_enc=1.0))
    case("enc_time", "nc_30_29", "enc_time", side(intr_rows=intr(-15, 14)), side(intr_rows=intr(-15, 13)))
    case("enc_time", "nc_1_min_1_2", "enc_time", side(own(-20, 0, z=short), intr(0, 40), min_enc=1.0), side(own(-20, 0, z=short), intr(0, 40), min_enc=2.0))


def _proximity():
    floor = lambda last: np.concatenate([910.0 - 8.0 * np.arange(-20, 20), [last]])          # noqa: E731  (the 41 altitudes, the last one given)
    case("proximity", "own_floor_740_752", "prox_own", side(own(z=lambda t: 900.0 - 8.0 * t)), side(own(z=lambda t: 912.0 - 8.0 * t)))
    case("proximity", "own_floor_750_next", "prox_own", side(own(z=floor(750.0))), side(own(z=floor(up(750.0)))))
    case("proximity", "transit_level_2500_700", "prox_int", side(intr_rows=intr(z=2500.0)), side(intr_rows=intr(z=700.0)))
    case("proximity", "transit_level_next_750", "prox_int", side(intr_rows=intr(z=up(750.0))), side(intr_rows=intr(z=750.0)))
    # the same two descending intruders under both intents: the rule inverts for a transit intruder
    low, high = intr(z=lambda t: 900.0 - 8.0 * t), intr(z=lambda t: 1000.0 - 8.0 * t)          # floors 700 and 800
    case("proximity", "descending_transit", "prox_int", side(intr_rows=high, intents=(1, 3)), side(intr_rows=low, intents=(1, 3)))
    case("proximity", "descending_landing", "prox_int", side(intr_rows=low, intents=(1, 1)), side(intr_rows=high, intents=(1, 1)))
    # thres_dist_ft = 0.5: an ownship through the origin is close for |t| <= 9 (0.475 ft against 0.527 at |t| = 10), one 2 nm abeam never
    # is and need not be low; the intruder, 1 nm from either, never is
    case("proximity", "never_close", "prox_own", side(own(z=lambda t: 912.0 - 8.0 * t, y=2.0), intr(y0=2.0), dist=0.5),
         side(own(z=lambda t: 912.0 - 8.0 * t), dist=0.5))
    # low from t = 10 on (748 ft), close for |t| <= 9 under 0.5 and for |t| <= 11 under 0.6 (0.580 ft against 0.633 at |t| = 12)
    case("proximity", "close_only_while_high", "prox_own", side(own(z=lambda t: 828.0 - 8.0 * t), dist=0.6), side(own(z=lambda t: 828.0 - 8.0 * t), dist=0.5))


def _vertical():
    def z40(first, d):           # 40 altitudes from 39 differences
        assert len(d) == 39
        return steps(first, d)
    e = 2.0 ** -14               # one f32 step between 512 and 1024
    # 8 of the 40 rates at exactly -5 (the repeated last one among them): 8 / 40 = 0.2 = pth; one of them a step inside: 7 of 40
    at, inside = [-1.0] * 32 + [-5.0] * 7, [-1.0] * 32 + [-5.0 + e] + [-5.0] * 6
    case("vertical", "descent_exactly_5_fraction_8_7", "vert_own", side(own(-20, 19, z=z40(800.0, at))), side(own(-20, 19, z=z40(800.0, inside))))
    case("vertical", "fraction_8_7_of_40", "vert_own", side(own(-20, 19, z=z40(800.0, [-1.0] * 32 + [-6.0] * 7))),
         side(own(-20, 19, z=z40(800.0, [-1.0] * 33 + [-6.0] * 6))))
    case("vertical", "fraction_counts_the_repeated_last", "vert_own", side(own(-20, 19, z=z40(800.0, [-6.0] * 6 + [-1.0] * 32 + [-6.0]))),
         side(own(-20, 19, z=z40(800.0, [-6.0] * 6 + [-1.0] * 33))))
    # own climb: intent 2, band 240..300, +5 exactly against a step inside
    cl_at, cl_in = [1.0] * 32 + [5.0] * 7, [1.0] * 32 + [5.0 - e] + [5.0] * 6
    case("vertical", "own_climb_exactly_5", "vert_own", side(own(-20, 19, z=z40(700.0, cl_at), h=270.0), intents=(2, 3)),
         side(own(-20, 19, z=z40(700.0, cl_in), h=270.0), intents=(2, 3)))
    case("vertical", "own_climb_needs_climb", "vert_own", side(own(z=lambda t: 900.0 + 8.0 * t, h=270.0), intents=(2, 3)), side(own(h=270.0), intents=(2, 3)))
    # a level track: zmax == zmin, pth = 0, and 0 / n >= 0 passes; one altitude a step off: pth > 0 and nothing descends
    one_off = np.full(41, 700.0)
    one_off[17] = up(700.0)
    case("vertical", "level_landing_intruder", "vert_int", side(intr_rows=intr(z=700.0), intents=(1, 1)), side(intr_rows=intr(z=one_off), intents=(1, 1)))
    down8, up8 = intr(z=lambda t: 900.0 - 8.0 * t), intr(z=lambda t: 900.0 + 8.0 * t)          # 1020 -> 700 and 780 <- 700 ... 1100
    case("vertical", "intruder_intent_1", "vert_int", side(intr_rows=down8, intents=(1, 1)), side(intr_rows=intr(z=lambda t: 740.0 + 8.0 * t), intents=(1, 1)))
    case("vertical", "intruder_intent_2", "vert_int", side(intr_rows=intr(z=lambda t: 740.0 + 8.0 * t), intents=(1, 2)), side(intr_rows=down8, intents=(1, 2)))
    case("vertical", "intruder_intent_3_or_1", "vert_int", side(intr_rows=up8, intents=(1, 3)), side(intr_rows=intr(z=lambda t: 740.0 + 8.0 * t), intents=(1, 1)))


def _heading():
    def h40(deciding):           # 37 rows at 90, two out of the band, and the deciding row
        h = np.full(40, 90.0)
        h[5], h[6], h[30] = 130.0, 130.0, deciding
        return h
    case("heading", "exactly_60", "heading", side(own(-20, 19, h=h40(60.0))), side(own(-20, 19, h=h40(down(60.0)))))
    case("heading", "exactly_120", "heading", side(own(-20, 19, h=h40(120.0))), side(own(-20, 19, h=h40(up(120.0)))))
    case("heading", "fraction_38_37_of_40", "heading", side(own(-20, 19, h=h40(90.0))), side(own(-20, 19, h=h40(130.0))))
    hc = h40(270.0) + 180.0
    hc[30] = 240.0
    ho = hc.copy()
    ho[30] = down(240.0)
    climb = lambda t: 860.0 + 8.0 * t          # noqa: E731
    case("heading", "climb_band_exactly_240", "heading", side(own(-20, 19, z=climb, h=hc), intents=(2, 3)), side(own(-20, 19, z=climb, h=ho), intents=(2, 3)))


def _limits():
    def one(n, k, base, value):
        a = np.full(n, base)
        a[k] = value
        return a
    case("limits", "z_max_altitude", "limits_int", side(intr_rows=intr(z=5000.0)), side(intr_rows=intr(z=one(41, 12, 5000.0, up(5000.0)))))
    case("limits", "z_zero", "limits_own", side(own(z=np.concatenate([8.0 * np.arange(40, 0, -1), [0.5]]))), side(own(z=lambda t: 8.0 * (20.0 - t))))
    case("limits", "own_min_vel", "limits_own", side(own(v=one(41, 9, 190.0, 100.0))), side(own(v=one(41, 9, 190.0, down(100.0)))))
    case("limits", "own_max_vel", "limits_own", side(own(v=one(41, 33, 190.0, 300.0))), side(own(v=one(41, 33, 190.0, up(300.0)))))
    case("limits", "intruder_min_vel_first_row", "limits_int", side(intr_rows=intr(v=one(41, 0, 95.0, 50.0))), side(intr_rows=intr(v=one(41, 0, 95.0, down(50.0)))))
    case("limits", "intruder_max_vel_last_row", "limits_int", side(intr_rows=intr(v=one(41, 40, 95.0, 250.0))), side(intr_rows=intr(v=one(41, 40, 95.0, up(250.0)))))
    # |dh| == maxVertRate (12 for the intruder) and one step out, in the middle and as the last difference, which the last row repeats
    e = 2.0 ** -11               # one f32 step between 2048 and 4096
    for name, k in (("middle", 20), ("last", 39)):
        for sign in (1.0, -1.0):
            d_at, d_out = np.zeros(40), np.zeros(40)
            d_at[k], d_out[k] = sign * 12.0, sign * (12.0 + e)
            case("limits", "vert_rate_%s_%s" % (name, "up" if sign > 0 else "down"), "limits_int", side(intr_rows=intr(z=steps(2500.0, d_at))),
                 side(intr_rows=intr(z=steps(2500.0, d_out))))
    # the turn-rate test compares rad/s with its limit: 0.05 lets 2 deg/s (0.0349) through and stops 3 deg/s (0.0524)
    slow = ((100.0, 300.0, 12.0, 5000.0, 50.0), (50.0, 250.0, 0.05, 5000.0, 12.0))
    turn = lambda r, k: steps(200.0, [0.0] * k + [r] * 3 + [0.0] * (37 - k))          # noqa: E731
    case("limits", "turn_rate_2_3_deg_s", "limits_int", side(intr_rows=intr(h=turn(2.0, 10)), dl=slow), side(intr_rows=intr(h=turn(3.0, 10)), dl=slow))
    case("limits", "turn_rate_last_difference", "limits_int", side(intr_rows=intr(h=turn(-2.0, 37)), dl=slow), side(intr_rows=intr(h=turn(-3.0, 37)), dl=slow))
    case("limits", "turn_rate_across_360", "limits_int", side(intr_rows=intr(h=steps(357.0, [0.0] * 10 + [2.0] * 3 + [0.0] * 27) % 360.0), dl=slow),
         side(intr_rows=intr(h=steps(357.0, [0.0] * 10 + [3.0] * 3 + [0.0] * 27) % 360.0), dl=slow))
    # pitch: asin(8 / 190) is 2.4132 degrees
    case("limits", "pitch_2p5_2p4", "limits_own", side(pitch=(2.5, 10.0)), side(pitch=(2.4, 10.0)))
    # |dz| / v > 1: MATLAB's asind turns complex, its magnitude above 90: only an infinite limit lets it through
    steep = ((100.0, 300.0, 12.0, 5000.0, 50.0), (50.0, 250.0, 12.0, 5000.0, 200.0))
    jump = np.zeros(40)
    jump[18] = 96.0
    case("limits", "ratio_above_1_infinite_pitch", "limits_int", side(intr_rows=intr(z=steps(2500.0, jump)), dl=steep, pitch=(10.0, INF)),
         side(intr_rows=intr(z=steps(2500.0, jump)), dl=steep, pitch=(10.0, 89.0)))
    jump1 = np.zeros(40)
    jump1[18] = 95.0
    case("limits", "ratio_exactly_1_is_90_degrees", "limits_int", side(intr_rows=intr(z=steps(2500.0, jump1)), dl=steep, pitch=(10.0, 91.0)),
         side(intr_rows=intr(z=steps(2500.0, jump)), dl=steep, pitch=(10.0, 91.0)))
    # a track of one row (rf = rb = 1) has no rates: rejected; two rows pass
    short = lambda t: 740.0 - 8.0 * t          # noqa: E731
    case("limits", "one_row_intruder", "limits_int", side(intr_rows=intr(0, 1), min_enc=1.0), side(intr_rows=intr(0, 0), min_enc=1.0))
    case("limits", "one_row_ownship", "limits_own", side(own(-1, 0, z=short), min_enc=1.0), side(own(0, 0, z=740.0), min_enc=1.0))


def _cum_turn():
    def hd(d, first=200.0, t0=None):
        """an intruder whose headings start at `first` and differ by d"""
        n = len(d) + 1
        t0 = -(n // 2) if t0 is None else t0
        return intr(t0, t0 + n - 1, h=steps(first, d) % 360.0)
    lim = lambda x: dict(cum=(180.0, float(x)), min_enc=1.0)          # noqa: E731
    # CheckCumTurn's known answers: a steady 3 deg/s turn through 210 deg is rejected at 180, the same amount split into a left and a
    # right turn is not, and no sum exceeds an infinite limit
    case("cum_turn", "steady_zigzag", "cum_int", side(intr_rows=intr(-40, 41, h=ZIGZAG)), side(intr_rows=intr(-40, 40, h=STEADY)))
    case("cum_turn", "steady_limit_inf_180", "cum_int", side(intr_rows=intr(-40, 40, h=STEADY), **lim(INF)), side(intr_rows=intr(-40, 40, h=STEADY), **lim(180.0)))
    t35 = [0.0] * 5 + [2.5] * 14 + [0.0] * 5
    case("cum_turn", "sum_equals_limit_35", "cum_int", side(intr_rows=hd(t35), **lim(35.0)), side(intr_rows=hd([0.0] * 5 + [2.5] * 13 + [2.625] + [0.0] * 5), **lim(35.0)))
    case("cum_turn", "sum_35p5_limit_36_35", "cum_int", side(intr_rows=hd([0.0] * 5 + [2.5] * 13 + [3.0] + [0.0] * 5), **lim(36.0)),
         side(intr_rows=hd([0.0] * 5 + [2.5] * 13 + [3.0] + [0.0] * 5), **lim(35.0)))
    case("cum_turn", "sign_change_resets", "cum_int", side(intr_rows=hd([0.0] * 4 + [30.0, -10.0, 30.0] + [0.0] * 4), **lim(45.0)),
         side(intr_rows=hd([0.0] * 4 + [30.0, 10.0, 30.0] + [0.0] * 4), **lim(45.0)))
    # a track that begins mid-turn: the first turn end (2) lies before the first turn start (5); the reference pairs them, an empty range,
    # and never sums either turn.  The same turns behind a still first second are found.
    case("cum_turn", "begins_mid_turn", "cum_int", side(intr_rows=hd([50.0, 50.0, 0.0, 0.0, 50.0, 50.0, 0.0, 0.0]), **lim(45.0)),
         side(intr_rows=hd([0.0, 50.0, 50.0, 0.0, 0.0, 50.0, 50.0, 0.0]), **lim(45.0)))
    case("cum_turn", "ends_mid_turn_end_appended", "cum_int", side(intr_rows=hd([0.0, 30.0, 0.0, 0.0, 20.0, 20.0]), **lim(45.0)),
         side(intr_rows=hd([0.0, 30.0, 0.0, 0.0, 30.0, 30.0]), **lim(45.0)))
    case("cum_turn", "ends_mid_turn_only_turn", "cum_int", side(intr_rows=hd([0.0, 0.0, 0.0, 20.0, 20.0]), **lim(45.0)),
         side(intr_rows=hd([0.0, 0.0, 0.0, 30.0, 30.0]), **lim(45.0)))
    case("cum_turn", "no_turn_limit_0", "cum_int", side(**lim(0.0)), side(intr_rows=hd([0.0] * 20 + [0.25] + [0.0] * 19), **lim(0.0)))
    case("cum_turn", "all_turn", "cum_int", side(intr_rows=hd([1.0] * 40), **lim(40.0)), side(intr_rows=hd([1.0] * 40), **lim(39.5)))
    # 0.25 rounds half away to 0.3 (ten of them pass 2.5), 0.03125 rounds to 0: no turn at all
    case("cum_turn", "quarter_degree_rounds_half_away", "cum_int", side(intr_rows=hd([0.0] * 3 + [0.25] * 10 + [0.0] * 3), **lim(3.5)),
         side(intr_rows=hd([0.0] * 3 + [0.25] * 10 + [0.0] * 3), **lim(2.5)))
    case("cum_turn", "minus_quarter_degree_rounds_half_away", "cum_int", side(intr_rows=hd([0.0] * 3 + [-0.25] * 10 + [0.0] * 3), **lim(3.5)),
         side(intr_rows=hd([0.0] * 3 + [-0.25] * 10 + [0.0] * 3), **lim(2.5)))
    case("cum_turn", "thirty_second_degree_is_no_turn", "cum_int", side(intr_rows=hd([0.03125] * 40), **lim(0.5)), side(intr_rows=hd([0.0625] * 40), **lim(0.5)))
    case("cum_turn", "across_180", "cum_int", side(intr_rows=hd([0.0] + [5.0] * 8 + [0.0], first=160.0), **lim(40.0)),
         side(intr_rows=hd([0.0] + [5.0] * 8 + [0.0], first=160.0), **lim(39.0)))
    case("cum_turn", "across_360_downwards", "cum_int", side(intr_rows=hd([0.0] + [-5.0] * 8 + [0.0], first=20.0), **lim(40.0)),
         side(intr_rows=hd([0.0] + [-5.0] * 8 + [0.0], first=20.0), **lim(39.0)))
    at360 = steps(340.0, [0.0] + [10.0] * 4 + [0.0])
    assert at360[3] == 360.0     # (360 itself, not 0)
    case("cum_turn", "through_360_itself", "cum_int", side(intr_rows=intr(-3, 3, h=at360), **lim(40.0)),
         side(intr_rows=intr(-3, 3, h=at360), **lim(39.0)))
    case("cum_turn", "own_turn_inside_the_band", "cum_own", side(own(h=steps(70.0, [0.0] * 5 + [1.0] * 30 + [0.0] * 5)), cum=(30.0, 180.0)),
         side(own(h=steps(70.0, [0.0] * 5 + [1.0] * 30 + [0.0] * 5)), cum=(29.0, 180.0)))
    # the longest track the entry accepts: cap = 125, rf = rb = 125, 248 differences, still and turning seconds in turn (124 turns of one
    # second, the last one closed by the appended end), and only the last turn exceeds the limit
    d = np.zeros(248)
    d[1::4], d[3::4] = 2.0, -2.0
    big = d.copy()
    big[247] = -4.0
    case("cum_turn", "longest_track_last_turn", "cum_int", side(intr_rows=hd(d, t0=-124), cap=125, **lim(3.0)), side(intr_rows=hd(big, t0=-124), cap=125, **lim(3.0)))


STEADY = np.concatenate([np.zeros(5), np.arange(0, 211, 3.0), np.full(5, 210.0)])
ZIGZAG = np.concatenate([np.zeros(5), np.arange(0, 106, 3.0), np.arange(105, -1, -3.0), np.zeros(5)])


def _void():
    for k, who in enumerate(("own_fwd", "own_bck", "int_fwd", "int_bck")):
        case("void", "void_" + who, "void", BASE, side(void=(k, 0 if k % 2 else -7)))


for _family in (_cpa, _proximity, _vertical, _heading, _limits, _cum_turn, _void):
    _family()
FAMILIES = tuple(dict.fromkeys(c["family"] for c in CASES))

# two tracks without a common second, as rows (the block layout cannot hold them): both references reject them
NO_COMMON = (own(-20, 0)[:-5], intr(0, 40))


def sides_of(family=None):
    """every side of the family's cases (all cases: None), each once, in order"""
    out, seen = [], set()
    for c in CASES:
        if family in (None, c["family"]):
            for s in c["sides"]:
                if id(s) not in seen:
                    seen.add(id(s))
                    out.append(s)
    return out


def batches(sides):
    """the sides grouped by their launch options, in order of first appearance: [(opts, [side, ...])]"""
    groups = {}
    for s in sides:
        groups.setdefault(s["key"], (s["opts"], []))[1].append(s)
    return list(groups.values())


def row_counts(s):
    """rows [4] of a side: own fwd, own bck, int fwd, int bck"""
    r = []
    for rows in (s["own"], s["intr"]):
        r += [int(rows[-1, 0]) + 1, int(-rows[0, 0]) + 1]
    if s["void"]:
        r[s["void"][0]] = s["void"][1]
    return r


def pack(sides, cap, fill=np.nan):
    """the sides in k_terminal_propagate's layout: geo [n, 12] f64 (only the intents set, the rest NaN), tracks [2n, 2 C, 5] f32 with second
    t of a track in row C + t and `fill` in every row outside its span, rows [4n] i32"""
    n, C = len(sides), t0_row(cap)
    geo = np.full((n, 12), np.nan)
    tracks = np.full((2 * n, 2 * C, 5), fill, dtype=F32)
    rows = np.zeros(4 * n, dtype=np.int32)
    for e, s in enumerate(sides):
        geo[e, 5], geo[e, 11] = s["intents"]
        for a, tr in enumerate((s["own"], s["intr"])):
            lo = C + int(tr[0, 0])
            assert lo >= 1 and lo + tr.shape[0] <= 2 * C
            tracks[2 * e + a, lo: lo + tr.shape[0]] = tr[:, 1:]
        rows[4 * e: 4 * e + 4] = row_counts(s)
    return geo, tracks, rows


def unpack(tracks, rows, cap):
    """what pack() packed, read back as the kernel reads it: [(own rows, intruder rows)] f64, None for a void track"""
    C, out = t0_row(cap), []
    for e in range(rows.size // 4):
        pair = []
        for a in range(2):
            rf, rb = int(rows[4 * e + 2 * a]), int(rows[4 * e + 2 * a + 1])
            if rf < 1 or rb < 1:
                pair.append(None)
                continue
            lo = C - (rb - 1)
            t = np.arange(lo, lo + rf + rb - 1, dtype=np.float64) - C
            pair.append(np.concatenate([t[:, None], tracks[2 * e + a, lo: lo + rf + rb - 1].astype(np.float64)], axis=1))
        out.append(tuple(pair))
    return out


# ---- k_terminal_smooth
SMOOTH_SHAPES = ((1, 1), (2, 1), (1, 2), (3, 1), (3, 3), (8, 8), (15, 1), (16, 16), (64, 1), (33, 33), (128, 128), (125, 125), (1, 128))
SMOOTH_CAPS = (2, 8, 123, 125)


def smooth_block(shapes, cap, seed, fill=np.nan):
    """tracks [len(shapes), 2 C, 5] f32 and rows [2 len(shapes)] for k_terminal_smooth: shapes (rf, rb), a non-positive entry for a void
    track.  The values are not symmetric and not small integers (a drifting random walk in thousandths), so that the window sums are
    inexact in f32; a void track's whole block holds values, which must stay."""
    C = t0_row(cap)
    rs = np.random.RandomState(seed)
    tracks = np.full((len(shapes), 2 * C, 5), fill, dtype=F32)
    rows = np.zeros(2 * len(shapes), dtype=np.int32)
    for a, (rf, rb) in enumerate(shapes):
        rows[2 * a: 2 * a + 2] = rf, rb
        live = rf >= 1 and rb >= 1
        assert rf <= cap and rb <= cap
        lo, n = (C - (rb - 1), rf + rb - 1) if live else (0, 2 * C)
        base = np.array([1.0, -2.0, 1500.0, 90.0, 150.0])
        walk = base + np.cumsum(rs.uniform(-1.0, 1.5, (n, 5)) * np.array([0.01, 0.01, 9.0, 2.0, 3.0]), axis=0) + np.arange(n)[:, None] * 0.001
        tracks[a, lo: lo + n] = walk.astype(F32)
    return tracks, rows
