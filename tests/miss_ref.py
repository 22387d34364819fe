"""The definition of emgpu_miss_distance_device (include/emgpu.h) restated in numpy: f64, the same operations in the same order, np.sqrt
for the root, the minimum over the ROOTS with NaNs masked, integer totals in uint64.  It never imports the library.

xyz_a / xyz_b are PLANAR [P, 3, ld] as the library takes them; only columns 0 .. n_x-1 are looked at."""
import numpy as np

from pair_cases import pairing, planar  # noqa: F401  (planar: the tests of other layers take it from here)

NMAC_CPA, NMAC_ANY, NO_CPA, BAD_INDEX = 1, 2, 4, 8


def miss(xyz_a, xyz_b, n_a, n_b, n_pairs, idx_a=None, idx_b=None, pose_b=None, weights=None, nmac_h_ft=500.0, nmac_v_ft=100.0, totals=None):
    """{"hmd", "vmd" f64 [n_pairs], "t_cpa" int32, "flags" uint8, "totals" uint64 [8]: `totals` (or zeros) plus this call's}"""
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
        d = np.sqrt(dx * dx + dy * dy)
        dz = zb - za
        live = ~np.isnan(d)
        none = ~live.any(axis=0)
        t = np.argmin(np.where(live, d, np.inf), axis=0)             # the first of equal minima; an all-inf column gives 0
        t = np.where(live[t, np.arange(n_pairs)], t, np.argmax(live, axis=0))   # (+inf everywhere it is a number, NaN elsewhere: the first number)
        col = np.arange(n_pairs)
        hmd, vmd = d[t, col], dz[t, col]
        cpa = (hmd < nmac_h_ft) & (np.abs(vmd) < nmac_v_ft)
        any_ = ((d < nmac_h_ft) & (np.abs(dz) < nmac_v_ft)).any(axis=0)
    hmd = np.where(none | bad, np.nan, hmd)
    vmd = np.where(none | bad, np.nan, vmd)
    t = np.where(none | bad, -1, t).astype(np.int32)
    cpa, any_ = cpa & ~none & ~bad, any_ & ~bad
    flags = (np.where(cpa, NMAC_CPA, 0) | np.where(any_, NMAC_ANY, 0) | np.where(none & ~bad, NO_CPA, 0) | np.where(bad, BAD_INDEX, 0)).astype(np.uint8)
    w = np.ones(n_pairs, dtype=np.uint64) if weights is None else np.asarray(weights).astype(np.uint64)
    ok = ~bad
    tot = np.zeros(8, dtype=np.uint64) if totals is None else np.array(totals, dtype=np.uint64)
    add = [ok.sum(), cpa.sum(), any_.sum(), (none & ok).sum(), bad.sum(), w[ok].sum(dtype=np.uint64), w[cpa].sum(dtype=np.uint64),
           w[any_].sum(dtype=np.uint64)]
    tot += np.array([int(x) for x in add], dtype=np.uint64)
    return {"hmd": hmd, "vmd": vmd, "t_cpa": t, "flags": flags, "totals": tot}
