"""The definition of emgpu_cpa_pose_device (include/emgpu.h) restated in numpy, statement by statement: f64, the
same operations in the same order, np.sqrt for the roots, the draws of encounter_ref (Philox from the oracle's independent restatement).
It never imports the library.

xyz_a / xyz_b are PLANAR [P, 3, ld] as the library takes them; only columns 0 .. n_x-1 and points tc and tc + 1 are looked at."""
import numpy as np

from encounter_ref import _block, disc_point, uniform32
from pair_cases import pairing

FALLBACK, NO_PASS, SATURATED, BAD_INDEX = 2, 4, 8, 16


def cpa_pose(xyz_a, xyz_b, n_a, n_b, n_pairs, hmd_max_ft, vmd_max_ft, seed, t_lo, t_hi=None, idx_a=None, idx_b=None, weights_in=None,
             rate_scale=1.0, first_index=0, max_attempts=16, with_weights=True):
    """{"pose" f64 [5, n_pairs], "rate" f64, "t_cpa" int32, "flags" uint8, "weights" uint32 (what weights_out receives; with_weights=False:
    no weights_out is given, zeros are returned and SATURATED is never set), and the intermediate values "rel" [3, n_pairs] (relx, rely,
    dz), "e" [2, n_pairs] (ex, ey), "l", "g" and "tc" (the drawn second of every pair, a bad one's too) for the tests of the geometry}"""
    xyz_a, xyz_b = np.asarray(xyz_a, dtype=np.float64), np.asarray(xyz_b, dtype=np.float64)
    P = xyz_a.shape[0]
    t_hi = t_lo if t_hi is None else t_hi
    assert P >= 2 and xyz_b.shape[0] == P and xyz_a.shape[1] == xyz_b.shape[1] == 3 and 0 <= t_lo <= t_hi <= P - 2
    Hm, Vm = float(hmd_max_ft), float(vmd_max_ft)
    kc = (4.0 * Hm) * Vm

    bad, ja, jb = pairing(idx_a, idx_b, n_a, n_b, n_pairs)
    gidx = (np.uint64(int(first_index) & (2**64 - 1)) + np.arange(n_pairs, dtype=np.uint64))
    # the draws of stream 4
    w4 = _block(gidx, seed, 4, 0)
    u1, u2, x = uniform32(w4[0]), uniform32(w4[1]), np.asarray(w4[2], dtype=np.uint64)
    # 0. the second
    span = np.uint64(t_hi - t_lo + 1)
    tc = (t_lo + ((x * span) >> np.uint64(32)).astype(np.int64)).astype(np.int64)
    At, At1, Bt, Bt1 = xyz_a[tc, :, ja].T, xyz_a[tc + 1, :, ja].T, xyz_b[tc, :, jb].T, xyz_b[tc + 1, :, jb].T     # [3, n_pairs] each
    with np.errstate(all="ignore"):
        # 1. the displacements of second tc
        ax, ay, _az = At1 - At
        bx, by, _bz = Bt1 - Bt
        # 2. the heading
        p, q, fb = disc_point(gidx, seed, 3, max_attempts)
        r = np.sqrt(p * p + q * q)
        c, s = p / r, q / r
        vx, vy = c * bx - s * by, s * bx + c * by
        # 3. the relative horizontal velocity
        rx, ry = vx - ax, vy - ay
        g = np.sqrt(rx * rx + ry * ry)
        # 4. the rate
        Q = kc * g
        passes = (Q > 0.0) & np.isfinite(Q)
        # 5. the offsets
        ex, ey = rx / g, ry / g
        l = Hm * (2.0 * u1 - 1.0)
        relx, rely = (-l) * ey, l * ex
        dz = Vm * (2.0 * u2 - 1.0)
        # 6. the pose
        ox = (At[0] + relx) - (c * Bt[0] - s * Bt[1])
        oy = (At[1] + rely) - (s * Bt[0] + c * Bt[1])
        oz = (At[2] + dz) - Bt[2]
        # 8. the weight
        w = np.ones(n_pairs) if weights_in is None else np.asarray(weights_in).astype(np.uint64).astype(np.float64)
        f = np.floor(w * (Q / float(rate_scale)) + 0.5)
        fits = f <= 4294967295.0
        wout = np.where(fits, f, 4294967295.0)
    nan = np.nan
    live = passes & ~bad
    pose = np.stack([np.where(bad, nan, c), np.where(bad, nan, s), np.where(live, ox, nan), np.where(live, oy, nan), np.where(live, oz, nan)])
    rate = np.where(live, Q, 0.0)
    sat = live & ~fits & bool(with_weights)
    flags = (np.where(~bad & fb, FALLBACK, 0) | np.where(~passes & ~bad, NO_PASS, 0) | np.where(sat, SATURATED, 0)
             | np.where(bad, BAD_INDEX, 0)).astype(np.uint8)
    weights = np.where(live & bool(with_weights), wout, 0.0).astype(np.uint64).astype(np.uint32)
    return {"pose": pose, "rate": rate, "t_cpa": np.where(bad, -1, tc).astype(np.int32), "flags": flags, "weights": weights,
            "rel": np.stack([relx, rely, dz]), "e": np.stack([ex, ey]), "l": l, "g": g, "tc": tc}
