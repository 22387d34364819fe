"""The definition of emgpu_avoid_device (include/emgpu.h) restated in numpy, statement by statement: f64, the same operations in the same
order, vectorised over the pairs and looping over the seconds, integer totals in uint64.  It never imports the library.  Also
`encounters`: four interleaved groups of pairs, so that every outcome of the alert and of the manoeuvre is taken by some of them, and
`HAND`: answers worked out by hand.

xyz_a / xyz_b are PLANAR [P, 3, ld] as the library takes them; only columns 0 .. n_x-1 are looked at."""
import numpy as np

import pair_cases
from pair_cases import planar  # noqa: F401
from well_clear_ref import _rel, relative

ALERTED, CLIMB, NMAC_UNMIT, NMAC_MIT, LATE, NO_CPA, BAD_INDEX = 1, 2, 4, 8, 16, 32, 64
DEFAULTS = dict(alert_tau_s=60.0, alert_dmod_ft=4000.0, alert_hmd_ft=4000.0, alert_h_ft=700.0, nmac_h_ft=500.0, nmac_v_ft=100.0, delay_s=5,
                rate_fps=25.0, accel_fps2=8.0, dz_max_ft=np.inf)
PROMPT = dict(DEFAULTS, delay_s=0, accel_fps2=np.inf)          # the other response of the tests: at once, at the full rate
_cache = {}


def avoid(xyz_a, xyz_b, n_a, n_b, n_pairs, idx_a=None, idx_b=None, pose_b=None, weights=None, totals=None, alert_tau_s=60.0,
          alert_dmod_ft=4000.0, alert_hmd_ft=4000.0, alert_h_ft=700.0, nmac_h_ft=500.0, nmac_v_ft=100.0, delay_s=5, rate_fps=25.0, accel_fps2=8.0,
          dz_max_ft=np.inf):
    """{"hmd", "vmd", "vmd_mit" f64 [n_pairs], "t_cpa", "t_alert" int32, "flags" uint8, "totals" uint64 [12]: `totals` (or zeros) plus this
    call's}"""
    bad, dx, dy, dz = relative(xyz_a, xyz_b, n_a, n_b, n_pairs, idx_a, idx_b, pose_b)
    P = dx.shape[0]
    tau_s, h, Hn, Vn = np.float64(alert_tau_s), np.float64(alert_h_ft), np.float64(nmac_h_ft), np.float64(nmac_v_ft)
    D2, H2 = np.float64(alert_dmod_ft) * np.float64(alert_dmod_ft), np.float64(alert_hmd_ft) * np.float64(alert_hmd_ft)
    rate, accel, dz_max = np.float64(rate_fps), np.float64(accel_fps2), np.float64(dz_max_ft)
    tr = rate / accel
    half_tr, half_a = np.float64(0.5) * tr, np.float64(0.5) * accel
    zeros = np.zeros(n_pairs)
    with np.errstate(all="ignore"):
        # the alert second and the sense: the first p with alert[p]
        t_alert, climb = np.full(n_pairs, -1, dtype=np.int32), np.zeros(n_pairs, dtype=bool)
        for p in range(P):
            q = min(p, P - 2)
            ux, uy, wz = (dx[q + 1] - dx[q], dy[q + 1] - dy[q], dz[q + 1] - dz[q]) if P > 1 else (zeros, zeros, zeros)
            x, y, z = dx[p], dy[p], dz[p]
            rr, rv, vv = x * x + y * y, x * ux + y * uy, ux * ux + uy * uy
            valid = np.isfinite(rr) & np.isfinite(rv) & np.isfinite(vv) & np.isfinite(z)
            inside, closing = rr <= D2, rv < 0.0
            tau = np.where(inside, 0.0, np.where(closing, (D2 - rr) / rv, np.inf))
            tc = np.where(vv > 0.0, (-rv) / vv, 0.0)
            tc = np.where(tc > 0.0, tc, 0.0)
            px, py = x + tc * ux, y + tc * uy
            hp2 = px * px + py * py
            by_tau = ~inside & closing & (tau <= tau_s) & (hp2 <= H2)
            alert = valid & (np.abs(z) <= h) & (inside | by_tau)
            zp = z + tc * wz
            descend = (zp > 0.0) | (~(zp < 0.0) & (z > 0.0))
            first = alert & (t_alert < 0)
            t_alert = np.where(first, np.int32(p), t_alert).astype(np.int32)
            climb = np.where(first, ~descend, climb)
        # the manoeuvre, the two NMAC tests and the CPA
        alerted = t_alert >= 0
        t0 = t_alert.astype(np.int64) + int(delay_s)
        best, vmd, vmd_mit = (np.full(n_pairs, np.nan) for _ in range(3))
        t_cpa = np.full(n_pairs, -1, dtype=np.int32)
        unmit, mit = np.zeros(n_pairs, dtype=bool), np.zeros(n_pairs, dtype=bool)
        for p in range(P):
            k = p - t0
            kd = k.astype(np.float64)
            g = np.where(kd < tr, half_a * (kd * kd), rate * (kd - half_tr))
            g = np.where(g < dz_max, g, dz_max)
            zm = np.where(alerted & (k >= 1), np.where(climb, dz[p] - g, dz[p] + g), dz[p])
            d = np.sqrt(dx[p] * dx[p] + dy[p] * dy[p])
            take = (d == d) & ((t_cpa < 0) | (d < best))
            best, vmd, vmd_mit = np.where(take, d, best), np.where(take, dz[p], vmd), np.where(take, zm, vmd_mit)
            t_cpa = np.where(take, np.int32(p), t_cpa).astype(np.int32)
            unmit |= (d < Hn) & (np.abs(dz[p]) < Vn)
            mit |= (d < Hn) & (np.abs(zm) < Vn)
    ok = ~bad
    alerted, climb, unmit, mit = alerted & ok, climb & ok, unmit & ok, mit & ok
    late, none, induced = alerted & (t0 >= P - 1), (t_cpa < 0) & ok, mit & ~unmit
    best, vmd, vmd_mit = (np.where(bad, np.nan, v) for v in (best, vmd, vmd_mit))
    t_cpa, t_alert = (np.where(bad, np.int32(-1), v).astype(np.int32) for v in (t_cpa, t_alert))
    flags = (np.where(alerted, ALERTED, 0) | np.where(climb, CLIMB, 0) | np.where(unmit, NMAC_UNMIT, 0) | np.where(mit, NMAC_MIT, 0) |
             np.where(late, LATE, 0) | np.where(none, NO_CPA, 0) | np.where(bad, BAD_INDEX, 0)).astype(np.uint8)
    w = np.ones(n_pairs, dtype=np.uint64) if weights is None else np.asarray(weights).astype(np.uint64)
    tot = np.zeros(12, dtype=np.uint64) if totals is None else np.array(totals, dtype=np.uint64)
    add = [ok.sum(), alerted.sum(), unmit.sum(), mit.sum(), induced.sum(), none.sum(), bad.sum()] + \
          [w[m].sum(dtype=np.uint64) for m in (ok, alerted, unmit, mit, induced)]
    tot += np.array([int(v) for v in add], dtype=np.uint64)
    return {"hmd": best, "vmd": vmd, "vmd_mit": vmd_mit, "t_cpa": t_cpa, "t_alert": t_alert, "flags": flags, "totals": tot}


def encounters(n, P, seed):
    """(a, b): two sets of n tracks [n, P, 3], four interleaved groups by i % 4.  A flies start + v p + cumsum(U(-3, 3)) with v = U(-250, 250)
    ft/s per horizontal axis, and so does B, placed so that at a drawn second tc it is off A by a drawn miss, perpendicular to the relative
    horizontal velocity of the straight parts:
      0  a close pass: the miss within 800 ft, 200 ft vertically, tc in [0.25 P, 1.1 P]: most are alerted at second 0 and resolved
      1  the same at tc in [2, min(14, P - 1)]: short notice, the manoeuvre comes late or not at all
      2  a wide pass, the miss up to 9000 ft and 1500 ft: many are never alerted
      3  a close pass with vertical rates up to +-60 ft/s (the others: +-5): many are above or below the alert volume at first
    Drawn once per shape and shared (read-only)."""
    key = (n, P, seed)
    if key not in _cache:
        rs = np.random.RandomState(seed * 104729 + n * 193 + P)
        group = np.arange(n) % 4
        t = np.arange(P)[None, :, None]
        start = np.concatenate([rs.uniform(-2500.0, 2500.0, (n, 1, 2)), rs.uniform(3000.0, 3600.0, (n, 1, 1))], axis=2)
        vz_max = np.where(group == 3, 60.0, 5.0)[:, None, None]
        va, vb = (np.concatenate([rs.uniform(-250.0, 250.0, (n, 1, 2)), rs.uniform(-1.0, 1.0, (n, 1, 1)) * vz_max], axis=2) for _ in range(2))
        wa, wb = (np.cumsum(rs.uniform(-3.0, 3.0, (n, P, 3)), axis=1) for _ in range(2))
        tc = np.where(group == 1, rs.randint(2, max(min(14, P - 1), 2) + 1, n), np.floor(rs.uniform(0.25 * P, 1.1 * P, n))).astype(np.int64)
        wide = group == 2
        m = rs.uniform(-1.0, 1.0, n) * np.where(wide, 9000.0, 800.0)
        mz = rs.uniform(-1.0, 1.0, n) * np.where(wide, 1500.0, 200.0)
        rel = (vb - va)[:, 0, :2]
        speed = np.maximum(np.hypot(rel[:, 0], rel[:, 1]), 1.0e-9)
        off = np.stack([-m * rel[:, 1] / speed, m * rel[:, 0] / speed, mz], axis=1)[:, None, :]
        a = start + va * t + wa
        at_tc = start[:, 0, :] + va[:, 0, :] * tc[:, None]                     # A's straight part at second tc
        b = (at_tc[:, None, :] + off) + vb * (t - tc[:, None, None]) + wb
        out = []
        for xyz in (a, b):
            xyz = np.ascontiguousarray(xyz)
            xyz.setflags(write=False)
            out.append(xyz)
        _cache[key] = tuple(out)
    return _cache[key]


def posed_encounters(n, P, seed):
    """(a, b, pose): `encounters` seen through a random pose: pose_b [5, n] turns and moves B, and b is B turned and moved back, so that the
    pair still flies as `encounters` made it, to rounding"""
    a, b = encounters(n, P, seed)
    rs = np.random.RandomState(seed * 41 + n + P)
    th, o = rs.uniform(-np.pi, np.pi, n), np.stack([rs.uniform(-2000.0, 2000.0, n), rs.uniform(-2000.0, 2000.0, n), rs.uniform(-300.0, 300.0, n)])
    c, s = np.cos(th), np.sin(th)
    x, y, z = b[:, :, 0] - o[0][:, None], b[:, :, 1] - o[1][:, None], b[:, :, 2] - o[2][:, None]
    back = np.stack([c[:, None] * x + s[:, None] * y, c[:, None] * y - s[:, None] * x, z], axis=2)
    return a, np.ascontiguousarray(back), np.ascontiguousarray(np.stack([c, s, o[0], o[1], o[2]]))


def shares(res, n):
    """the shares of the pairs that the floors of the tests are about, from avoid's result"""
    fl = res["flags"]
    has = lambda bit: (fl & bit) != 0          # noqa: E731
    return {"never": (~has(ALERTED)).sum() / n, "climb": has(CLIMB).sum() / n, "descend": (has(ALERTED) & ~has(CLIMB)).sum() / n,
            "later": (res["t_alert"] > 0).sum() / n, "unresolved": (has(NMAC_UNMIT) & has(NMAC_MIT)).sum() / n,
            "resolved": (has(NMAC_UNMIT) & ~has(NMAC_MIT)).sum() / n, "late": has(LATE).sum() / n}


FLOOR = 0.05                                                                # at n >= 257, P in (32, 64), the default parameters
FLOORS = ("never", "climb", "descend", "later", "unresolved", "resolved")
LATE_FLOOR = 0.5                                                            # at P in (3, 5), the default parameters


def check_floors(res, n, P, params):
    """the conditions on the inputs, where the case carries them (asserted on the restatement's result)"""
    share = shares(res, n)
    if n >= 257 and P in (32, 64) and params == DEFAULTS:
        for name in FLOORS:
            assert share[name] >= FLOOR, (name, share[name])
    if n >= 257 and P in (3, 5):
        if params == DEFAULTS:
            assert share["late"] >= LATE_FLOOR, share["late"]
        if params == PROMPT:
            assert share["resolved"] > 0.0
    return share


def _par(**kw):
    return dict(PROMPT, **kw)


_N, _INF = np.nan, np.inf
_CLOSING = 10000.0 - 400.0 * np.arange(27)          # head-on at 400 ft/s: x = 400, 0, -400 at seconds 24, 25, 26
_HEAD_ON = [10000.0, 9600.0, 9600.0]                # closing during the first second only
_below_500 = np.nextafter(500.0, 0.0)
# (name, (a, b), parameters, hmd, vmd, vmd_mit, t_cpa, t_alert, flags): answers worked out by hand.  accel = inf unless stated: g = 25 k.
# Second 0 of _CLOSING: rr = 1e8, rv = 10000 * -400 = -4e6, tau = (1.6e7 - 1e8) / -4e6 = 21 <= 60; vv = 1.6e5, tc = 25, px = 0: the alert.
HAND = [
    # z = 0, wz = 0: zp = 0, so the sign of z decides, and z = 0 climbs.  t0 = 5, g = 25 (p - 5): 475 at second 24, 500 at the CPA
    ("level head-on, resolved by a climb", _rel(_CLOSING, 0.0, 0.0), _par(delay_s=5), 0.0, 0.0, -500.0, 25, 0, ALERTED | CLIMB | NMAC_UNMIT),
    ("the intruder 50 ft above: descend", _rel(_CLOSING, 0.0, 50.0), _par(delay_s=5), 0.0, 50.0, 550.0, 25, 0, ALERTED | NMAC_UNMIT),
    # x = 1600 .. -800: inside DMOD at second 0, t0 = 5, only second 6 is moved; the NMAC seconds 3, 4, 5 are not
    ("short notice, unresolved", _rel(1600.0 - 400.0 * np.arange(7), 0.0, 0.0), _par(delay_s=5), 0.0, 0.0, 0.0, 4, 0,
     ALERTED | CLIMB | NMAC_UNMIT | NMAC_MIT),
    # 300 ft above and level at the alert (zp = 300: descend), then the intruder descends 32 ft/s: dz = -436, -468, -500 at seconds
    # 24 .. 26, no NMAC; the ownship has descended 475, 500, 525 ft by then: dz' = 39, 32, 25
    ("induced: the intruder descends into the escape", _rel(_CLOSING, 0.0, 300.0 - 32.0 * np.maximum(np.arange(27) - 1, 0)), _par(delay_s=5),
     0.0, -468.0, 32.0, 25, 0, ALERTED | NMAC_MIT),
    ("late: t0 = 5 >= P - 1 = 3", _rel(_CLOSING[:4], 0.0, 0.0), _par(delay_s=5), 8800.0, 0.0, 0.0, 3, 0, ALERTED | CLIMB | LATE),
    # second 1 (15400, u = -400): tau = (1.6e7 - 2.3716e8) / -6.16e6 = 35.9 > 35; second 2 takes the same velocity at 15000: tau = 34.83
    ("late: the alert at the last point", _rel([15400.0, 15400.0, 15000.0], 0.0, 0.0), _par(alert_tau_s=35.0), 15000.0, 0.0, 0.0, 2, 2,
     ALERTED | CLIMB | LATE),
    ("no alert: no relative motion outside DMOD", _rel([10000.0] * 3, 0.0, 0.0), _par(), 10000.0, 0.0, 0.0, 0, -1, 0),
    ("one point, inside, the intruder above", _rel([3000.0], 0.0, 100.0), _par(), 3000.0, 100.0, 100.0, 0, 0, ALERTED | LATE),
    ("one point, outside", _rel([10000.0], 0.0, 0.0), _par(), 10000.0, 0.0, 0.0, 0, -1, 0),
    # D2 = 9e6, rr = 2.5e7, rv = 5000 * -100 = -5e5, tau = (9e6 - 2.5e7) / -5e5 = 32; the CPA is second 1, the first of two at 4900 ft
    ("tau == alert_tau_s", _rel([5000.0, 4900.0, 4900.0], 0.0, 0.0), _par(alert_dmod_ft=3000.0, alert_tau_s=32.0), 4900.0, 0.0, -25.0, 1, 0,
     ALERTED | CLIMB),
    ("tau just above alert_tau_s", _rel([5000.0, 4900.0, 4900.0], 0.0, 0.0), _par(alert_dmod_ft=3000.0, alert_tau_s=np.nextafter(32.0, 0.0)),
     4900.0, 0.0, 0.0, 1, -1, 0),
    ("|z| == alert_h_ft, below: climb", _rel(_HEAD_ON, 0.0, -700.0), _par(), 9600.0, -700.0, -725.0, 1, 0, ALERTED | CLIMB),
    ("|z| just above alert_h_ft", _rel(_HEAD_ON, 0.0, np.nextafter(700.0, _INF)), _par(), 9600.0, np.nextafter(700.0, _INF),
     np.nextafter(700.0, _INF), 1, -1, 0),
    # the root of a square is the number itself
    ("d just below nmac_h_ft", _rel([_below_500] * 2, 0.0, 0.0), _par(), _below_500, 0.0, 0.0, 0, 0, ALERTED | CLIMB | NMAC_UNMIT | NMAC_MIT),
    ("d == nmac_h_ft", _rel([500.0] * 2, 0.0, 0.0), _par(), 500.0, 0.0, 0.0, 0, 0, ALERTED | CLIMB),
    # a NaN x spoils its own second and the velocity of the one before: the alert is second 2, only second 3 is moved
    ("a NaN x at one second", _rel([1000.0, _N, 1000.0, 1000.0], 0.0, 0.0), _par(), 1000.0, 0.0, 0.0, 0, 2, ALERTED | CLIMB),
    # wz is NaN at second 0, tc = 0: zp = 0 + 0 * NaN is NaN, the sign of z = 0 decides: climb.  dz' = 0, NaN, -50, -75
    ("a NaN z at one second", _rel(400.0, 0.0, [0.0, _N, 0.0, 0.0]), _par(), 400.0, 0.0, 0.0, 0, 0, ALERTED | CLIMB | NMAC_UNMIT | NMAC_MIT),
    ("every second NaN", _rel([_N, _N, _N], 0.0, 0.0), _par(), _N, _N, _N, -1, -1, NO_CPA),
]
# accel = 8, rate = 25: tr = 3.125, half_tr = 1.5625, half_a = 4: g(1 .. 4) = 4, 16, 36, 25 (4 - 1.5625) = 60.9375; the track ends at its
# CPA, second k, and the response starts at second 0
for _k, _g in ((1, 4.0), (2, 16.0), (3, 36.0), (4, 60.9375)):
    HAND.append(("accel 8, rate 25: g(%d) = %s" % (_k, _g), _rel(_CLOSING[:_k + 1], 0.0, 0.0), _par(accel_fps2=8.0), float(_CLOSING[_k]), 0.0, -_g,
                 _k, 0, ALERTED | CLIMB))
HAND.append(("accel 8, rate 25, dz_max_ft 50: g(3) = 36", _rel(_CLOSING[:4], 0.0, 0.0), _par(accel_fps2=8.0, dz_max_ft=50.0), 8800.0, 0.0, -36.0, 3,
             0, ALERTED | CLIMB))
HAND.append(("accel 8, rate 25, dz_max_ft 50: g(4) = 50", _rel(_CLOSING[:5], 0.0, 0.0), _par(accel_fps2=8.0, dz_max_ft=50.0), 8400.0, 0.0, -50.0, 4,
             0, ALERTED | CLIMB))


def hand_want(case):
    """the expected outputs of a HAND case as avoid's arrays of one pair, and its totals"""
    _, _, _, hmd, vmd, vmd_mit, t_cpa, t_alert, flags = case
    bit = lambda b: int((flags & b) != 0)          # noqa: E731
    ind = int(bit(NMAC_MIT) and not bit(NMAC_UNMIT))
    counts = [1, bit(ALERTED), bit(NMAC_UNMIT), bit(NMAC_MIT), ind, bit(NO_CPA), 0]
    return {"hmd": np.array([hmd]), "vmd": np.array([vmd]), "vmd_mit": np.array([vmd_mit]), "t_cpa": np.array([t_cpa], dtype=np.int32),
            "t_alert": np.array([t_alert], dtype=np.int32), "flags": np.array([flags], dtype=np.uint8),
            "totals": np.array(counts + [counts[0]] + counts[1:5], dtype=np.uint64)}
