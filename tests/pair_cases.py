"""What the tests of the paired-tracks layer and their references share: the random tracks, the PLANAR layout, the pairing restated in
numpy, output buffers between guard bytes and the bit-for-bit comparison.  It never imports the library."""
import numpy as np

GUARD, FILL = 64, 0xA5
_cache = {}


def tracks(n, P, seed):
    """n random tracks [n, P, 3] of a few thousand feet extent, drawn once per shape and shared (read-only)"""
    key = (n, P, seed)
    if key not in _cache:
        rs = np.random.RandomState(seed * 7919 + n * 131 + P)
        start = np.concatenate([rs.uniform(-2500.0, 2500.0, (n, 1, 2)), rs.uniform(1000.0, 1600.0, (n, 1, 1))], axis=2)
        vel = np.concatenate([rs.uniform(-250.0, 250.0, (n, 1, 2)), rs.uniform(-30.0, 30.0, (n, 1, 1))], axis=2)
        wob = np.cumsum(rs.uniform(-20.0, 20.0, (n, P, 3)), axis=1)
        xyz = np.ascontiguousarray(start + vel * np.arange(P)[None, :, None] + wob)
        xyz.setflags(write=False)
        _cache[key] = xyz
    return _cache[key]


def planar(xyz_rows, ld=None):
    """tracks [n, P, 3] as PLANAR [P, 3, ld] (ld >= n; the columns behind n hold a pattern no result may depend on)"""
    xyz_rows = np.asarray(xyz_rows, dtype=np.float64)
    n, P, _ = xyz_rows.shape
    out = np.full((P, 3, n if ld is None else ld), 7.0e9)
    out[:, :, :n] = np.transpose(xyz_rows, (1, 2, 0))
    return out


def pairing(idx_a, idx_b, n_a, n_b, n_pairs):
    """(bad, ja, jb): whether pair i names a column outside its set, and its columns of set A and B (0 for a bad pair, which the caller
    masks).  Pair i takes idx_x[i]; without idx_x, i of a set of several and 0 of a set of one."""
    def columns(idx, n):
        if idx is not None:
            return np.asarray(idx, dtype=np.int64).reshape(-1)[:n_pairs]
        return np.arange(n_pairs, dtype=np.int64) if n > 1 else np.zeros(n_pairs, dtype=np.int64)
    ia, ib = columns(idx_a, n_a), columns(idx_b, n_b)
    bad = (ia < 0) | (ia >= n_a) | (ib < 0) | (ib >= n_b)
    return bad, np.where(bad, 0, ia), np.where(bad, 0, ib)


def guarded(sizes, dev, init=None):
    """{name: device byte buffer of sizes[name] bytes between GUARD bytes before and behind}, every byte FILL but the payloads init names"""
    import torch
    bufs = {}
    for name, size in sizes.items():
        host = np.full(size + 2 * GUARD, FILL, dtype=np.uint8)
        host[GUARD:GUARD + size] = (init or {}).get(name, FILL)
        bufs[name] = torch.from_numpy(host).to(dev)
    return bufs


def payloads(bufs, sizes):
    """{name: the sizes[name] bytes between the guards}, once the guard bytes are seen to have stayed"""
    out = {}
    for name, buf in bufs.items():
        raw = buf.cpu().numpy()
        assert (raw[:GUARD] == FILL).all() and (raw[GUARD + sizes[name]:] == FILL).all(), "guard bytes of " + name
        out[name] = raw[GUARD:GUARD + sizes[name]].copy()
    return out


def same(got, want, names):
    """got[name] equals want[name] BIT FOR BIT for every name: doubles by their bits, a NaN against a NaN; integers as they are"""
    for name in names:
        g, w = got[name], want[name]
        if g.dtype == np.float64:
            nan = np.isnan(w)
            ulps = np.abs(g.view(np.int64)[~nan] - w.view(np.int64)[~nan])
            assert np.array_equal(np.isnan(g), nan) and not ulps.any(), "%s: largest difference %d ulps" % (name, ulps.max(initial=0))
        else:
            assert np.array_equal(g, w), (name, g, w)
