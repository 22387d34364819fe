"""The definition of emgpu_miss_segments_device (include/emgpu.h) restated in numpy: f64, the same operations in the same order, vectorised
over the pairs and looping over the seconds as the kernel does, np.sqrt for the roots, integer totals in uint64.  It never imports the
library.  Also `crossing`: pairs of tracks that pass near a common point at a time that is no whole second, and `brute`: dense sampling
of the piecewise-linear tracks.

xyz_a / xyz_b are PLANAR [P, 3, ld] as the library takes them; only columns 0 .. n_x-1 are looked at."""
import numpy as np

import pair_cases
from pair_cases import pairing, planar  # noqa: F401

NMAC_CPA, NMAC_ANY, NO_CPA, BAD_INDEX, CPA_BETWEEN, NMAC_BETWEEN = 1, 2, 4, 8, 16, 32
_cache = {}


def relative(xyz_a, xyz_b, n_a, n_b, n_pairs, idx_a=None, idx_b=None, pose_b=None):
    """(bad, dx, dy, dz, d), the last four [P, n_pairs]: the per-point part of the definition"""
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
        dx, dy = xa - xb, ya - yb
        return bad, dx, dy, zb - za, np.sqrt(dx * dx + dy * dy)


def miss_segments(xyz_a, xyz_b, n_a, n_b, n_pairs, idx_a=None, idx_b=None, pose_b=None, weights=None, nmac_h_ft=500.0, nmac_v_ft=100.0,
                  totals=None):
    """{"hmd", "vmd", "t_cpa_s" f64 [n_pairs], "flags" uint8, "totals" uint64 [10]: `totals` (or zeros) plus this call's}"""
    bad, dx, dy, dz, d = relative(xyz_a, xyz_b, n_a, n_b, n_pairs, idx_a, idx_b, pose_b)
    P, H, V = dx.shape[0], np.float64(nmac_h_ft), np.float64(nmac_v_ft)
    best, vmd, t = np.full(n_pairs, np.nan), np.full(n_pairs, np.nan), np.full(n_pairs, -1.0)
    inside, at_point, on_segment = (np.zeros(n_pairs, dtype=bool) for _ in range(3))
    with np.errstate(all="ignore"):
        for p in range(P):
            if p > 0:
                x0, y0, z0, z1 = dx[p - 1], dy[p - 1], dz[p - 1], dz[p]
                ex, ey, ez = dx[p] - x0, dy[p] - y0, z1 - z0
                ee, re = ex * ex + ey * ey, x0 * ex + y0 * ey
                valid = np.isfinite(ee) & np.isfinite(re) & np.isfinite(z0) & np.isfinite(ez)
                ts = np.where(ee > 0.0, (-re) / ee, 0.0)
                px, py = x0 + ts * ex, y0 + ts * ey
                ds, zs = np.sqrt(px * px + py * py), z0 + ts * ez
                take = valid & (ts > 0.0) & (ts < 1.0) & (ds == ds) & ((t < 0.0) | (ds < best))
                best, vmd, t = np.where(take, ds, best), np.where(take, zs, vmd), np.where(take, np.float64(p - 1) + ts, t)
                inside = np.where(take, True, inside)
                near = (np.where(z0 < z1, z0, z1) < V) & (np.where(z0 < z1, z1, z0) > -V)
                t0, t1 = (-V - z0) / ez, (V - z0) / ez
                mn, mx = np.where(t0 < t1, t0, t1), np.where(t0 < t1, t1, t0)
                lo = np.where(ez != 0.0, np.where(mn > 0.0, mn, 0.0), 0.0)
                hi = np.where(ez != 0.0, np.where(mx < 1.0, mx, 1.0), 1.0)
                tc = np.where(ts > lo, ts, lo)
                tc = np.where(tc < hi, tc, hi)
                qx, qy = x0 + tc * ex, y0 + tc * ey
                dc = np.sqrt(qx * qx + qy * qy)
                on_segment |= valid & near & (lo < hi) & (dc < H)
            take = (d[p] == d[p]) & ((t < 0.0) | (d[p] < best))
            best, vmd, t = np.where(take, d[p], best), np.where(take, dz[p], vmd), np.where(take, np.float64(p), t)
            inside = np.where(take, False, inside)
            at_point |= (d[p] < H) & (np.abs(dz[p]) < V)
        cpa = (best < H) & (np.abs(vmd) < V)
    ok = ~bad
    none = (t < 0.0) & ok
    cpa, any_, btw, inside = cpa & ok, (at_point | on_segment) & ok, on_segment & ~at_point & ok, inside & ok
    hmd, vmd, t = np.where(bad, np.nan, best), np.where(bad, np.nan, vmd), np.where(bad, -1.0, t)
    flags = (np.where(cpa, NMAC_CPA, 0) | np.where(any_, NMAC_ANY, 0) | np.where(none, NO_CPA, 0) | np.where(bad, BAD_INDEX, 0) |
             np.where(inside, CPA_BETWEEN, 0) | np.where(btw, NMAC_BETWEEN, 0)).astype(np.uint8)
    w = np.ones(n_pairs, dtype=np.uint64) if weights is None else np.asarray(weights).astype(np.uint64)
    tot = np.zeros(10, dtype=np.uint64) if totals is None else np.array(totals, dtype=np.uint64)
    add = [ok.sum(), cpa.sum(), any_.sum(), none.sum(), bad.sum(), w[ok].sum(dtype=np.uint64), w[cpa].sum(dtype=np.uint64),
           w[any_].sum(dtype=np.uint64), btw.sum(), w[btw].sum(dtype=np.uint64)]
    tot += np.array([int(x) for x in add], dtype=np.uint64)
    return {"hmd": hmd, "vmd": vmd, "t_cpa_s": t, "flags": flags, "totals": tot}


def crossing(n, P, seed):
    """(a, b): two sets of n tracks [n, P, 3] whose pair i passes near a common point at a real-valued time tc ~ U(0, P-1): both are
    c (+ m for B) + v (p - tc) + cumsum(U(-5, 5)), v up to 400 ft/s horizontally and 50 ft/s vertically, the offset m in
    U(-600, 600)^2 x U(-150, 150).  Drawn once per shape and shared (read-only).  P = 1: pair_cases.tracks."""
    if P == 1:
        return pair_cases.tracks(n, 1, seed), pair_cases.tracks(n, 1, seed + 1000)
    key = (n, P, seed)
    if key not in _cache:
        rs = np.random.RandomState(seed * 104729 + n * 193 + P)
        tc = rs.uniform(0.0, P - 1.0, (n, 1, 1))
        c = np.concatenate([rs.uniform(-2500.0, 2500.0, (n, 1, 2)), rs.uniform(1000.0, 1600.0, (n, 1, 1))], axis=2)
        m = np.concatenate([rs.uniform(-600.0, 600.0, (n, 1, 2)), rs.uniform(-150.0, 150.0, (n, 1, 1))], axis=2)
        out = []
        for off in (0.0, m):
            v = np.concatenate([rs.uniform(-400.0, 400.0, (n, 1, 2)), rs.uniform(-50.0, 50.0, (n, 1, 1))], axis=2)
            xyz = np.ascontiguousarray((c + off) + v * (np.arange(P)[None, :, None] - tc) + np.cumsum(rs.uniform(-5.0, 5.0, (n, P, 3)), axis=1))
            xyz.setflags(write=False)
            out.append(xyz)
        _cache[key] = tuple(out)
    return _cache[key]


def brute(a_rows, b_rows, K, nmac_h_ft=500.0, nmac_v_ft=100.0, block=250):
    """Dense sampling of the piecewise-linear tracks [n, P, 3], K sub-steps per second, the points included: (hmd [n], nmac_any bool [n],
    the largest |e| = length of a segment of the relative horizontal track).  `block` pairs at a time, to bound the memory."""
    r_all = np.asarray(a_rows, dtype=np.float64) - np.asarray(b_rows, dtype=np.float64)      # [n, P, 3]; dz's sign does not matter here
    n, P, _ = r_all.shape
    f = (np.arange(1, K) / float(K))[None, :, None]
    hmd_all, hit_all, e_max = np.empty(n), np.empty(n, dtype=bool), 0.0
    for lo in range(0, n, block):
        r = r_all[lo:lo + block]
        dp = np.sqrt(r[:, :, 0] ** 2 + r[:, :, 1] ** 2)
        hmd, hit = dp.min(axis=1), ((dp < nmac_h_ft) & (np.abs(r[:, :, 2]) < nmac_v_ft)).any(axis=1)
        for p in range(1, P):
            e = (r[:, p] - r[:, p - 1])[:, None, :]
            q = r[:, p - 1, None, :] + f * e                                                # [block, K-1, 3]
            dq = np.sqrt(q[:, :, 0] ** 2 + q[:, :, 1] ** 2)
            hmd = np.minimum(hmd, dq.min(axis=1))
            hit |= ((dq < nmac_h_ft) & (np.abs(q[:, :, 2]) < nmac_v_ft)).any(axis=1)
            e_max = max(e_max, float(np.sqrt(e[:, 0, 0] ** 2 + e[:, 0, 1] ** 2).max()))
        hmd_all[lo:lo + block], hit_all[lo:lo + block] = hmd, hit
    return hmd_all, hit_all, e_max


def posed_crossing(n, P, seed):
    """(a, b, pose): `crossing` seen through a random pose: pose_b [5, n] turns and moves B, and b is B turned and moved back, so that the
    pair still passes as `crossing` made it, to rounding"""
    a, b = crossing(n, P, seed)
    rs = np.random.RandomState(seed * 31 + n + P)
    th, o = rs.uniform(-np.pi, np.pi, n), np.stack([rs.uniform(-2000.0, 2000.0, n), rs.uniform(-2000.0, 2000.0, n), rs.uniform(-300.0, 300.0, n)])
    c, s = np.cos(th), np.sin(th)
    x, y, z = b[:, :, 0] - o[0][:, None], b[:, :, 1] - o[1][:, None], b[:, :, 2] - o[2][:, None]
    back = np.stack([c[:, None] * x + s[:, None] * y, c[:, None] * y - s[:, None] * x, z], axis=2)
    return a, np.ascontiguousarray(back), np.ascontiguousarray(np.stack([c, s, o[0], o[1], o[2]]))


def _rel(x, y, z):
    """(a, b) [1, P, 3] with dx = x, dy = y, dz = z exactly: A carries x and y, B carries z"""
    x, y, z = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(z, dtype=np.float64))
    return np.stack([x, y, 0.0 * z], axis=1)[None], np.stack([0.0 * z, 0.0 * z, z], axis=1)[None]


_N = np.nan
# (name, (a, b), (nmac_h, nmac_v), hmd, vmd, t_cpa_s, flags): answers worked out by hand
HAND = [
    # 2400 -> 800 -> -800 -> -2400 at y = 100: segment 2 has re = -1280000, ee = 2560000, ts = 0.5, the foot at (0, 100); the points are 806 ft away
    ("head-on, ts = 0.5, ez = 0", _rel([2400.0, 800.0, -800.0, -2400.0], 100.0, 30.0), (500.0, 100.0), 100.0, 30.0, 1.5, 1 | 2 | 16 | 32),
    # segment 2 from 600 to -1800: re = -1440000, ee = 5760000, ts = 0.25; zs = 20 + 0.25 * 10
    ("head-on, ts = 0.25", _rel([3000.0, 600.0, -1800.0], 100.0, [10.0, 20.0, 30.0]), (500.0, 100.0), 100.0, 22.5, 1.25, 1 | 2 | 16 | 32),
    # the interior of segment 1 is 400 ft away at t = 0.5; point 2 is 400 ft away too and comes later; segments 2 and 3 have ts = 1 and ts = 0
    ("an interior equals a later point", _rel([300.0, -300.0, 0.0, 300.0], 400.0, 150.0), (500.0, 100.0), 400.0, 150.0, 0.5, 16),
    # segment 1 ends at its foot (ts = 1), segment 2 starts at it (ts = 0): the point is the candidate, no interior
    ("a segment's end against the next one's start", _rel([500.0, 0.0, 500.0], 300.0, 0.0), (500.0, 100.0), 300.0, 0.0, 1.0, 1 | 2),
    # the same, the band touched from outside at that point alone: |dz| = V there and beyond it elsewhere
    ("the band touched at a point", _rel([500.0, 0.0, 500.0], 300.0, [300.0, 100.0, 300.0]), (500.0, 100.0), 300.0, 100.0, 1.0, 0),
    # point 2 is NaN: segments 2 and 3 are gone, points 1 and 3 are sqrt(500000) away and the first stays
    ("a NaN point", _rel([900.0, 700.0, _N, -700.0, -900.0], 100.0, 0.0), (500.0, 100.0), np.sqrt(500000.0), 0.0, 1.0, 0),
    # ... and its two segments only: segment 5 from -900 to 900 has ts = 0.5
    ("a NaN point and a later pass", _rel([900.0, 700.0, _N, -700.0, -900.0, 900.0], 100.0, 0.0), (500.0, 100.0), 100.0, 0.0, 4.5, 1 | 2 | 16 | 32),
    ("every point NaN", _rel([_N, _N, _N], 0.0, 0.0), (500.0, 100.0), _N, _N, -1.0, 4),
    # no relative motion: ts = 0, no interior; the points see the NMAC themselves
    ("ee == 0", _rel([300.0, 300.0, 300.0], 0.0, 0.0), (500.0, 100.0), 300.0, 0.0, 0.0, 1 | 2),
    # V = 0: segment 2 crosses dz = 0 at t0 = t1 = 0.5, lo == hi: the band is empty; vmd = 10 + 0.5 * (-20) = 0 is not < 0
    ("V == 0", _rel([2400.0, 800.0, -800.0, -2400.0], 100.0, [30.0, 10.0, -10.0, -30.0]), (500.0, 0.0), 100.0, 0.0, 1.5, 16),
    ("dc == H", _rel([2400.0, 800.0, -800.0, -2400.0], 500.0, 30.0), (500.0, 100.0), 500.0, 30.0, 1.5, 16),
]
