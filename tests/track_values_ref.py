"""A numpy restatement of the values of a trace derived from 1 Hz tracks (DESIGN.md "Values from tracks"; include/emgpu.h), the inverse of
sample2track.m:183-237, independent of the library's code.  Everything is float64; numpy contracts nothing, np.sqrt is the IEEE square root and
np.arctan2 the host library's atan2.  It never calls the library.

values() takes xyz [n, P, 3] (feet, one second apart, P >= 3) and returns (init [n, 5], dyn [n, T, 3]) with T = P - 2:
init columns: altitude, speed, vertical rate, acceleration, turn rate; dyn columns: vertical rate, acceleration, turn rate."""
import numpy as np

DEG_PER_RAD = 57.29577951308232
ALT, SPEED, VERTRATE, ACC, TURNRATE = range(5)


def headings(dx, dy, s):
    """h[t] = atan2(dy, dx) in degrees; where s[t] == 0 the previous heading is kept, and the one before the first is 0"""
    h = np.arctan2(dy, dx) * DEG_PER_RAD
    prev = np.zeros(h.shape[0])
    for t in range(h.shape[1]):
        h[:, t] = np.where(s[:, t] == 0.0, prev, h[:, t])
        prev = h[:, t]
    return h


def values(xyz, ur_speed, ur_vertrate, ur_heading):
    xyz = np.asarray(xyz, dtype=np.float64)
    n, P, _ = xyz.shape
    T = P - 2
    assert T >= 1
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (xyz[:, 1:, c] - xyz[:, :-1, c] for c in range(3))        # displacement t = 0 .. P-2
        s = np.sqrt(dx * dx + dy * dy)
        h = headings(dx, dy, s)
        vr = dz[:, :T] / np.float64(ur_vertrate)
        acc = (s[:, 1:] - s[:, :-1]) / np.float64(ur_speed)
        d = h[:, 1:] - h[:, :-1]
        w = d - 360.0 * np.floor((d + 180.0) / 360.0)
        tr = w / np.float64(ur_heading)
        dyn = np.stack([vr, acc, tr], axis=2)
        init = np.stack([xyz[:, 0, 2], s[:, 0] / np.float64(ur_speed), vr[:, 0], acc[:, 0], tr[:, 0]], axis=1)
    return init, dyn


def touched(P, k, coord):
    """What a single bad coordinate (0 x, 1 y, 2 z) at point k may change, on a track that never stands: (the init columns, a bool
    [T, 3] of the dyn cells)."""
    T = P - 2
    dyn = np.zeros((T, 3), dtype=bool)
    init = set()
    if coord == 2:
        secs, cols = [k - 1, k], [0]
        if k == 0:
            init.add(ALT)
    else:
        secs, cols = [k - 2, k - 1, k], [1, 2]
        if k <= 1:
            init.add(SPEED)
    for t in secs:
        if 0 <= t < T:
            dyn[t, cols] = True
            if t == 0:
                init.update(VERTRATE + c for c in cols)
    return sorted(init), dyn


def _polyline(headings_deg, speeds, z=None):
    """a track that leaves the origin and flies the given heading and speed in every second"""
    hd, sp = np.radians(np.asarray(headings_deg, dtype=np.float64)), np.asarray(speeds, dtype=np.float64)
    x = np.concatenate([[0.0], np.cumsum(sp * np.cos(hd))])
    y = np.concatenate([[0.0], np.cumsum(sp * np.sin(hd))])
    z = np.zeros(x.size) if z is None else np.asarray(z, dtype=np.float64)
    return np.stack([x, y, z], axis=1)


def hand_tracks():
    """The hand-written cases, {name: xyz [P, 3]} with P 3 or 6, and what they are about"""
    t = {}
    t["right angle"] = np.array([[0, 0, 0], [1, 0, 10], [1, 1, 30]], dtype=np.float64)                   # heading 0 -> 90
    t["across 180"] = _polyline([179, -179, 179, -179, 179], [100] * 5, [0, 5, 10, 15, 20, 25])          # 179 -> -179 is +2, back is -2
    t["more than a circle"] = _polyline([0, 100, 200, 300, 400], [50] * 5)                               # +100 four times: 400 in total
    t["reversal"] = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0]], dtype=np.float64)                        # 0 -> 180: exactly -180
    t["stands in the middle"] = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [1, 1, 0], [1, 2, 0], [1, 2, 0]], dtype=np.float64)
    t["stands first"] = np.array([[0, 0, 7], [0, 0, 7], [0, 1, 7]], dtype=np.float64)                    # h[0] = h[-1] = 0, then 90
    t["never moves"] = np.array([[3, 4, 100 - 10 * k] for k in range(6)], dtype=np.float64)
    t["dx -0.0 climbing north"] = np.array([[0.0, 0, 0], [-0.0, 1, 0], [-0.0, 2, 0]], dtype=np.float64)  # atan2(1, -0.0) = 90
    t["dx -0.0 standing"] = np.array([[0.0, 0, 0], [-0.0, 0, 0], [1.0, 0, 0]], dtype=np.float64)         # s == 0: held at 0, not atan2(0, -0.0) = 180
    return t
