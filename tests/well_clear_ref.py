"""The definition of emgpu_well_clear_device (include/emgpu.h) restated in numpy, statement by statement: f64, the same operations in the
same order, vectorised over the pairs and looping over the seconds, integer totals in uint64.  It never imports the library.  Also
`approaching`: pairs that start up to three DMOD apart and fly anywhere, so that every branch of the predicate is taken by some of them,
and `HAND`: answers worked out by hand.

xyz_a / xyz_b are PLANAR [P, 3, ld] as the library takes them; only columns 0 .. n_x-1 are looked at."""
import numpy as np

import pair_cases
from pair_cases import pairing, planar  # noqa: F401

LOST, AT_START, NO_DATA, BAD_INDEX, INSIDE_DMOD, BY_TAU = 1, 2, 4, 8, 16, 32
MISS_NMAC_ANY = 2
DEFAULTS = dict(tau_s=35.0, dmod_ft=4000.0, hmd_ft=4000.0, h_ft=450.0)
_cache = {}


def relative(xyz_a, xyz_b, n_a, n_b, n_pairs, idx_a=None, idx_b=None, pose_b=None):
    """(bad, dx, dy, dz), the last three [P, n_pairs]: the relative state of the miss-distance definition, without its root"""
    xyz_a, xyz_b = np.asarray(xyz_a, dtype=np.float64), np.asarray(xyz_b, dtype=np.float64)
    P = xyz_a.shape[0]
    assert xyz_b.shape[0] == P and P >= 1 and xyz_a.shape[1] == xyz_b.shape[1] == 3
    bad, ja, jb = pairing(idx_a, idx_b, n_a, n_b, n_pairs)
    xa, ya, za = (xyz_a[:, c, :][:, ja] for c in range(3))           # [P, n_pairs]
    xb, yb, zb = (xyz_b[:, c, :][:, jb] for c in range(3))
    with np.errstate(all="ignore"):
        if pose_b is not None:
            c, s, ox, oy, oz = (np.asarray(pose_b, dtype=np.float64)[k][None, :] for k in range(5))
            xb, yb, zb = (c * xb - s * yb) + ox, (s * xb + c * yb) + oy, zb + oz
        return bad, xa - xb, ya - yb, zb - za


def well_clear(xyz_a, xyz_b, n_a, n_b, n_pairs, idx_a=None, idx_b=None, pose_b=None, weights=None, miss_flags=None, tau_s=35.0, dmod_ft=4000.0,
               hmd_ft=4000.0, h_ft=450.0, totals=None):
    """{"t_first", "n_lost" int32 [n_pairs], "tau_min" f64, "flags" uint8, "totals" uint64 [10]: `totals` (or zeros) plus this call's, and
    the diagnostic "wide" bool [n_pairs]: some valid point had !inside && closing && tau <= tau_s && !(hp2 <= H2), "tau met, predicted
    miss too wide"}"""
    bad, dx, dy, dz = relative(xyz_a, xyz_b, n_a, n_b, n_pairs, idx_a, idx_b, pose_b)
    P = dx.shape[0]
    tau_s, h = np.float64(tau_s), np.float64(h_ft)
    D2, H2 = np.float64(dmod_ft) * np.float64(dmod_ft), np.float64(hmd_ft) * np.float64(hmd_ft)
    t_first, n_lost = np.full(n_pairs, -1, dtype=np.int32), np.zeros(n_pairs, dtype=np.int32)
    tau_min = np.full(n_pairs, np.nan)
    have, some_inside, some_tau, wide = (np.zeros(n_pairs, dtype=bool) for _ in range(4))
    with np.errstate(all="ignore"):
        for p in range(P):
            q = min(p, P - 2)
            ux, uy = (dx[q + 1] - dx[q], dy[q + 1] - dy[q]) if P > 1 else (np.zeros(n_pairs), np.zeros(n_pairs))
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
            lost = valid & (np.abs(z) <= h) & (inside | by_tau)
            take = valid & (~have | (tau < tau_min))
            tau_min = np.where(take, tau, tau_min)
            have |= valid
            t_first = np.where(lost & (t_first < 0), np.int32(p), t_first).astype(np.int32)
            n_lost = n_lost + lost.astype(np.int32)
            some_inside |= lost & inside
            some_tau |= lost & by_tau
            wide |= valid & ~inside & closing & (tau <= tau_s) & ~(hp2 <= H2)
    ok = ~bad
    is_lost, start, none = (n_lost > 0) & ok, (t_first == 0) & ok, ~have & ok
    t_first, n_lost = np.where(bad, np.int32(-1), t_first).astype(np.int32), np.where(bad, np.int32(0), n_lost).astype(np.int32)
    tau_min = np.where(bad, np.nan, tau_min)
    flags = (np.where(is_lost, LOST, 0) | np.where(start, AT_START, 0) | np.where(none, NO_DATA, 0) | np.where(bad, BAD_INDEX, 0) |
             np.where(some_inside & ok, INSIDE_DMOD, 0) | np.where(some_tau & ok, BY_TAU, 0)).astype(np.uint8)
    w = np.ones(n_pairs, dtype=np.uint64) if weights is None else np.asarray(weights).astype(np.uint64)
    nmac = np.zeros(n_pairs, dtype=bool) if miss_flags is None else is_lost & ((np.asarray(miss_flags, dtype=np.uint8)[:n_pairs] & MISS_NMAC_ANY) != 0)
    tot = np.zeros(10, dtype=np.uint64) if totals is None else np.array(totals, dtype=np.uint64)
    add = [ok.sum(), is_lost.sum(), start.sum(), none.sum(), bad.sum(), w[ok].sum(dtype=np.uint64), w[is_lost].sum(dtype=np.uint64),
           w[start].sum(dtype=np.uint64), nmac.sum(), w[nmac].sum(dtype=np.uint64)]
    tot += np.array([int(v) for v in add], dtype=np.uint64)
    return {"t_first": t_first, "n_lost": n_lost, "tau_min": tau_min, "flags": flags, "totals": tot, "wide": wide & ok}


def approaching(n, P, seed, dmod=4000.0, h=450.0):
    """(a, b): two sets of n tracks [n, P, 3].  B starts r0 ~ U(0, 3 dmod) from A in a direction theta ~ U(0, 2 pi) and U(-2 h, 2 h) above
    it; both fly start + v p + cumsum(U(-5, 5)) with v up to 400 ft/s horizontally and 50 ft/s vertically, in any direction: some pairs
    start inside DMOD, some close fast enough for tau, some of those aim wide, most never come near.  Drawn once per shape and shared
    (read-only)."""
    key = (n, P, seed, dmod, h)
    if key not in _cache:
        rs = np.random.RandomState(seed * 15485863 + n * 211 + P)
        r0, theta = rs.uniform(0.0, 3.0 * dmod, (n, 1)), rs.uniform(0.0, 2.0 * np.pi, (n, 1))
        start = np.concatenate([rs.uniform(-2500.0, 2500.0, (n, 1, 2)), rs.uniform(3000.0, 3600.0, (n, 1, 1))], axis=2)
        m = np.stack([r0 * np.cos(theta), r0 * np.sin(theta), rs.uniform(-2.0 * h, 2.0 * h, (n, 1))], axis=2)
        out = []
        for off in (0.0, m):
            v = np.concatenate([rs.uniform(-400.0, 400.0, (n, 1, 2)), rs.uniform(-50.0, 50.0, (n, 1, 1))], axis=2)
            wob = np.cumsum(rs.uniform(-5.0, 5.0, (n, P, 3)), axis=1)
            xyz = np.ascontiguousarray((start + off) + v * np.arange(P)[None, :, None] + wob)
            xyz.setflags(write=False)
            out.append(xyz)
        _cache[key] = tuple(out)
    return _cache[key]


def posed_approaching(n, P, seed):
    """(a, b, pose): `approaching` seen through a random pose: pose_b [5, n] turns and moves B, and b is B turned and moved back, so that
    the pair still flies as `approaching` made it, to rounding"""
    a, b = approaching(n, P, seed)
    rs = np.random.RandomState(seed * 37 + n + P)
    th, o = rs.uniform(-np.pi, np.pi, n), np.stack([rs.uniform(-2000.0, 2000.0, n), rs.uniform(-2000.0, 2000.0, n), rs.uniform(-300.0, 300.0, n)])
    c, s = np.cos(th), np.sin(th)
    x, y, z = b[:, :, 0] - o[0][:, None], b[:, :, 1] - o[1][:, None], b[:, :, 2] - o[2][:, None]
    back = np.stack([c[:, None] * x + s[:, None] * y, c[:, None] * y - s[:, None] * x, z], axis=2)
    return a, np.ascontiguousarray(back), np.ascontiguousarray(np.stack([c, s, o[0], o[1], o[2]]))


def shares(res, n):
    """the shares of the pairs that the floors of the tests are about, from well_clear's result"""
    fl = res["flags"]
    return {"lost": ((fl & LOST) != 0).sum() / n, "inside": ((fl & INSIDE_DMOD) != 0).sum() / n, "by_tau": ((fl & BY_TAU) != 0).sum() / n,
            "wide": res["wide"].sum() / n, "never": ((fl & LOST) == 0).sum() / n, "later": (res["t_first"] > 0).sum() / n}


FLOORS = {"lost": 0.15, "inside": 0.12, "by_tau": 0.03, "wide": 0.05, "never": 0.50}     # and "later" >= 0.05 at P = 64


def _rel(x, y, z):
    """(a, b) [1, P, 3] with dx = x, dy = y, dz = z exactly: A carries x and y, B carries z"""
    x, y, z = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(z, dtype=np.float64))
    zero = np.zeros(z.shape)          # (not 0.0 * z: a NaN in one coordinate stays in that coordinate)
    return np.stack([x, y, zero], axis=1)[None], np.stack([zero, zero, z], axis=1)[None]


def _thr(**kw):
    return dict(DEFAULTS, **kw)


_N, _INF = np.nan, np.inf
_HEAD_ON = [10000.0, 9600.0, 9600.0]     # closing 400 ft/s during the first second, then no relative motion: tau is inf at points 1 and 2
# (name, (a, b), thresholds, t_first, n_lost, tau_min, flags, wide): answers worked out by hand.  D2 = 1.6e7 with the defaults.
HAND = [
    # point 0: rr = 1e8, rv = 10000 * -400 = -4e6, tau = (1.6e7 - 1e8) / -4e6 = 21; vv = 1.6e5, tc = 25, px = 10000 - 25 * 400 = 0, hp2 = 0
    ("level head-on, tau = 21", _rel(_HEAD_ON, 0.0, 0.0), _thr(), 0, 1, 21.0, LOST | AT_START | BY_TAU, False),
    ("the same 600 ft apart vertically", _rel(_HEAD_ON, 0.0, 600.0), _thr(), -1, 0, 21.0, 0, False),
    # rr = 1.25e8, rv = -4e6, tau = (1.6e7 - 1.25e8) / -4e6 = 27.25; tc = 25, px = 0, py = 5000, hp2 = 2.5e7 > 1.6e7
    ("the same 5000 ft to the side: tau met, miss too wide", _rel(_HEAD_ON, 5000.0, 0.0), _thr(), -1, 0, 27.25, 0, True),
    ("diverging inside DMOD", _rel([1000.0, 1400.0, 1800.0], 0.0, 0.0), _thr(), 0, 3, 0.0, LOST | AT_START | INSIDE_DMOD, False),
    # D2 = 9e6, rr = 2.5e7, rv = 5000 * -100 = -5e5, tau = (9e6 - 2.5e7) / -5e5 = 32; tc = 5e5 / 1e4 = 50, px = 0
    ("tau == tau_s", _rel([5000.0, 4900.0, 4900.0], 0.0, 0.0), _thr(dmod_ft=3000.0, tau_s=32.0), 0, 1, 32.0, LOST | AT_START | BY_TAU, False),
    ("tau just above tau_s", _rel([5000.0, 4900.0, 4900.0], 0.0, 0.0), _thr(dmod_ft=3000.0, tau_s=np.nextafter(32.0, 0.0)), -1, 0, 32.0, 0, False),
    ("|z| == h_ft", _rel(_HEAD_ON, 0.0, -450.0), _thr(), 0, 1, 21.0, LOST | AT_START | BY_TAU, False),
    ("|z| just above h_ft", _rel(_HEAD_ON, 0.0, np.nextafter(450.0, _INF)), _thr(), -1, 0, 21.0, 0, False),
    ("rr == D2", _rel([4000.0, 4000.0], 0.0, 0.0), _thr(), 0, 2, 0.0, LOST | AT_START | INSIDE_DMOD, False),
    ("rr just above D2, no relative motion", _rel([np.nextafter(4000.0, _INF)] * 2, 0.0, 0.0), _thr(), -1, 0, _INF, 0, False),
    ("one point, inside", _rel([3000.0], 0.0, 100.0), _thr(), 0, 1, 0.0, LOST | AT_START | INSIDE_DMOD, False),
    ("one point, outside", _rel([10000.0], 0.0, 0.0), _thr(), -1, 0, _INF, 0, False),
    # point 1 (15400, u = -400): tau = (1.6e7 - 2.3716e8) / -6.16e6 = 35.9 > 35; point 2 takes the same velocity at 15000:
    # tau = (1.6e7 - 2.25e8) / -6e6 = 34.83, tc = 6e6 / 1.6e5 = 37.5, px = 0
    ("lost at the last point only", _rel([15400.0, 15400.0, 15000.0], 0.0, 0.0), _thr(), 2, 1, -2.09e8 / -6.0e6, LOST | BY_TAU, False),
    ("a NaN altitude at one second", _rel(1000.0, 0.0, [0.0, _N, 0.0, 0.0]), _thr(), 0, 3, 0.0, LOST | AT_START | INSIDE_DMOD, False),
    # a NaN x spoils its own second and the velocity of the one before
    ("a NaN x at one second", _rel([1000.0, _N, 1000.0, 1000.0], 0.0, 0.0), _thr(), 2, 2, 0.0, LOST | INSIDE_DMOD, False),
    ("every second NaN", _rel([_N, _N, _N], 0.0, 0.0), _thr(), -1, 0, _N, NO_DATA, False),
]
