"""The definition of emgpu_encounter_pose_device (include/emgpu.h) restated in numpy, statement by statement: f64,
the same operations in the same order, np.sqrt for the roots, Philox from the oracle's independent restatement at the oracle's number of
rounds.  It never imports the library.

xyz_a / xyz_b are PLANAR [P, 3, ld] as the library takes them; only columns 0 .. n_x-1 and points 0 and 1 are looked at."""
import numpy as np

import oracle as O
from pair_cases import pairing

END, FALLBACK, NO_ENTRY, SATURATED, BAD_INDEX = 1, 2, 4, 8, 16
SECTION = 13


def uniform32(x):
    """u = (min(x, 2^32 - 2) + 0.5) * 2^-32"""
    return (np.minimum(np.asarray(x, dtype=np.uint64), np.uint64(0xFFFFFFFE)).astype(np.float64) + 0.5) * (1.0 / 4294967296.0)


def _block(gidx, seed, a, block):
    """the four words of block `block` of stream a, per global index: counter {g_lo, g_hi, 0, 13 << 28 | a << 20 | block}, key = seed"""
    g = np.asarray(gidx, dtype=np.uint64)
    return O.philox4x32_np((g & np.uint64(0xFFFFFFFF)).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32), np.uint32(0),
                           np.uint32((SECTION << 28) | (a << 20) | block), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF,
                           O.philox_rounds())


def disc_point(gidx, seed, a, max_attempts):
    """(p, q, fallback) of the unit-disc point of stream a: attempt j takes words 2 (j & 1) and 2 (j & 1) + 1 of block j >> 1"""
    n = len(gidx)
    p, q, got = np.ones(n), np.zeros(n), np.zeros(n, dtype=bool)
    for j in range(max_attempts):
        if got.all():
            break              # (a later attempt is looked at by no pair)
        if j & 1 == 0:
            words = _block(gidx, seed, a, j >> 1)
        pj = 2.0 * uniform32(words[2 * (j & 1)]) - 1.0
        qj = 2.0 * uniform32(words[2 * (j & 1) + 1]) - 1.0
        d = pj * pj + qj * qj
        take = ~got & (d > 0.0) & (d <= 1.0)
        p, q, got = np.where(take, pj, p), np.where(take, qj, q), got | take
    return p, q, ~got


def encounter(xyz_a, xyz_b, n_a, n_b, n_pairs, radius_ft, half_height_ft, seed, idx_a=None, idx_b=None, weights_in=None, rate_scale=1.0,
              first_index=0, max_attempts=16, with_weights=True):
    """{"pose" f64 [5, n_pairs], "rate" f64, "flags" uint8, "weights" uint32 (what weights_out receives; with_weights=False: no weights_out
    is given, zeros are returned and SATURATED is never set), and the intermediate values "rel" [3, n_pairs], "rxy" [2, n_pairs], "Qs", "m"
    for the tests of the geometry}"""
    xyz_a, xyz_b = np.asarray(xyz_a, dtype=np.float64), np.asarray(xyz_b, dtype=np.float64)
    assert xyz_a.shape[0] >= 2 and xyz_b.shape[0] >= 2 and xyz_a.shape[1] == xyz_b.shape[1] == 3
    R, H = float(radius_ft), float(half_height_ft)
    ks, ke = (4.0 * R) * H, (np.pi * R) * R

    bad, ja, jb = pairing(idx_a, idx_b, n_a, n_b, n_pairs)
    A0, A1, B0, B1 = xyz_a[0][:, ja], xyz_a[1][:, ja], xyz_b[0][:, jb], xyz_b[1][:, jb]           # [3, n_pairs] each
    gidx = (np.uint64(int(first_index) & (2**64 - 1)) + np.arange(n_pairs, dtype=np.uint64))
    with np.errstate(all="ignore"):
        # 1. the displacements of the first second
        ax, ay, az = A1 - A0
        bx, by, bz = B1 - B0
        # 2. the heading
        p, q, fb0 = disc_point(gidx, seed, 0, max_attempts)
        r = np.sqrt(p * p + q * q)
        c, s = p / r, q / r
        vx, vy = c * bx - s * by, s * bx + c * by
        # 3. the relative velocity
        rx, ry, wr = vx - ax, vy - ay, bz - az
        g = np.sqrt(rx * rx + ry * ry)
        # 4. the swept volume per second
        Qs, Qe = ks * g, ke * np.abs(wr)
        Q = Qs + Qe
        entry = (Q > 0.0) & np.isfinite(Q)
        # 5. the entry point
        w2 = _block(gidx, seed, 2, 0)
        u1, u2, u3 = uniform32(w2[0]), uniform32(w2[1]), uniform32(w2[2])
        side = entry & (u1 * Q < Qs)
        end = entry & ~side
        ex, ey = rx / g, ry / g
        m = 2.0 * u2 - 1.0
        l, h = R * m, R * np.sqrt(1.0 - m * m)
        pe, qe, fb1 = disc_point(gidx, seed, 1, max_attempts)
        relx = np.where(side, (-h) * ex - l * ey, R * pe)
        rely = np.where(side, l * ex - h * ey, R * qe)
        dz = np.where(side, H * (2.0 * u3 - 1.0), np.where(wr < 0.0, H, -H))
        # 6. the pose
        ox = (A0[0] + relx) - (c * B0[0] - s * B0[1])
        oy = (A0[1] + rely) - (s * B0[0] + c * B0[1])
        oz = (A0[2] + dz) - B0[2]
        # 8. the weight
        w = np.ones(n_pairs) if weights_in is None else np.asarray(weights_in).astype(np.uint64).astype(np.float64)
        f = np.floor(w * (Q / float(rate_scale)) + 0.5)
        fits = f <= 4294967295.0
        wout = np.where(fits, f, 4294967295.0)
    nan = np.nan
    live = entry & ~bad
    pose = np.stack([np.where(bad, nan, c), np.where(bad, nan, s), np.where(live, ox, nan), np.where(live, oy, nan), np.where(live, oz, nan)])
    rate = np.where(live, Q, 0.0)
    sat = live & ~fits & bool(with_weights)
    flags = (np.where(end & ~bad, END, 0) | np.where(~bad & (fb0 | (end & fb1)), FALLBACK, 0) | np.where(~entry & ~bad, NO_ENTRY, 0)
             | np.where(sat, SATURATED, 0) | np.where(bad, BAD_INDEX, 0)).astype(np.uint8)
    weights = np.where(live & bool(with_weights), wout, 0.0).astype(np.uint64).astype(np.uint32)
    return {"pose": pose, "rate": rate, "flags": flags, "weights": weights, "rel": np.stack([relx, rely, dz]), "rxy": np.stack([rx, ry]),
            "Qs": Qs, "m": m}
