"""A numpy restatement of discretizing a trace of values (DESIGN.md "Discretizing a trace"), independent of the library's code: written from
the definition in include/emgpu.h, discretize_bayes.m:14-22 (coarse bin), hierarchical_discretize.m:29 (wrap), hierarchical_cutpoints.m:14
(fine cuts a + k * h, one f64 multiply and one f64 add each: numpy contracts nothing) and hierarchical_discretize.m:37-49 (fine bin, pairs),
over the model's own arrays as em_io.em_read returns them.  It never calls the library.

discretize() takes the user-facing shapes (init_val [n, ni], dyn_val [n, T, nd], either None) and returns (init_bin, dyn_bin, repeat,
change, bad): uint8 bins in the same shapes (0 for a bad value), uint64 [ni] vectors by variable id, and the number of bad values."""
import numpy as np


def info(parms):
    """what the definition reads of a model: r, boundaries (f64; empty = categorical) and zero bin (0 = none) by variable id, and the variable
    id of every temporal-map row"""
    ni = int(parms["n_initial"])
    bnd = [np.asarray(b, dtype=np.float64).reshape(-1) for b in parms["boundaries"]]
    zero = [int(np.atleast_1d(z)[0]) if np.size(z) else 0 for z in parms["zero_bins"]]
    tm = np.asarray(parms["temporal_map"]).reshape(-1, 2) if "temporal_map" in parms and np.size(parms["temporal_map"]) else np.zeros((0, 2), int)
    return {"ni": ni, "r": [int(r) for r in np.asarray(parms["r_initial"]).reshape(-1)[:ni]], "bnd": bnd, "zero": zero,
            "dvar": [int(v) - 1 for v in tm[:, 0]]}


def coarse(x, b, r, wrap=False):
    """x (any shape) -> (d uint8 with 0 for a bad value, good)"""
    x = np.asarray(x).astype(np.float64)                 # exact for f32
    if b.size == 0:                                      # categorical: the value is the bin
        good = (x >= 1) & (x <= r) & (x == np.floor(x))
        return np.where(good, x, 0).astype(np.uint8), good
    d = np.ones(x.shape, dtype=np.int64)
    for q in range(1, r):
        d += x >= b[q]
    if wrap and r > 1:
        d = 1 + np.mod(d - 1, r - 1)
    good = ~np.isnan(x)
    return np.where(good, d, 0).astype(np.uint8), good


def fine(x, d, b, n_fine):
    """the fine bin of x inside its coarse bin d (1-based; entries with d == 0 give 0)"""
    x = np.asarray(x).astype(np.float64)
    dd = np.maximum(d.astype(np.int64), 1)
    a = b[dd - 1]
    with np.errstate(invalid="ignore"):
        h = (b[dd] - a) / np.float64(n_fine)
        f = np.ones(x.shape, dtype=np.int64)
        for k in range(1, n_fine):
            f += x >= a + np.float64(k) * h
    return np.where(d > 0, f, 0)


def discretize(g, init_val=None, dyn_val=None, n_fine=0, wrap_mask=0):
    ni = g["ni"]
    repeat, change = np.zeros(ni, dtype=np.uint64), np.zeros(ni, dtype=np.uint64)
    bad = 0
    init_bin = dyn_bin = None
    if init_val is not None:
        iv = np.asarray(init_val)
        init_bin = np.zeros(iv.shape, dtype=np.uint8)
        for v in range(ni):
            init_bin[:, v], good = coarse(iv[:, v], g["bnd"][v], g["r"][v], bool((wrap_mask >> v) & 1))
            bad += int((~good).sum())
    if dyn_val is not None:
        dv = np.asarray(dyn_val)
        dyn_bin = np.zeros(dv.shape, dtype=np.uint8)
        for k, v in enumerate(g["dvar"]):
            b, r = g["bnd"][v], g["r"][v]
            d, good = coarse(dv[:, :, k], b, r, bool((wrap_mask >> v) & 1))
            dyn_bin[:, :, k] = d
            bad += int((~good).sum())
            if n_fine and b.size and dv.shape[1] > 1:
                f = fine(dv[:, :, k], d, b, n_fine)
                pair = (d[:, 1:] != 0) & (d[:, :-1] != 0) & (d[:, 1:] == d[:, :-1]) & (d[:, 1:] != g["zero"][v])
                same = f[:, 1:] == f[:, :-1]
                repeat[v] += np.uint64((pair & same).sum())
                change[v] += np.uint64((pair & ~same).sum())
    return init_bin, dyn_bin, repeat, change, bad
