"""The library's layout of a trace -- the one description of it -- and the conversions between it and the user-facing shapes."""
import numpy as np


class TraceLayout:
    """A trace of n trajectories (columns; ld where a call addresses a window of them) of T seconds, n_i initial and n_d dynamic variables:
    init_bin [n_i, n] u8, init_val [n_i, n], dyn_bin [G4, n_d, n] u32 (4 seconds per word), dyn_val [G4, n_d, n, 4], G4 = ceil(T / 4); the
    values are f32, or f64 with value_bytes=8.  `shape`, `dtype` and `nbytes` are dicts by these four names, in this order."""

    def __init__(self, n_i, n_d, n, T, value_bytes=4):
        n_i, n_d, n, val = int(n_i), int(n_d), int(n), np.dtype(np.float64 if value_bytes == 8 else np.float32)
        self.G4 = G4 = (max(int(T), 0) + 3) // 4
        self.shape = {"init_bin": (n_i, n), "init_val": (n_i, n), "dyn_bin": (G4, n_d, n), "dyn_val": (G4, n_d, n, 4)}
        self.dtype = {"init_bin": np.dtype(np.uint8), "init_val": val, "dyn_bin": np.dtype(np.uint32), "dyn_val": val}
        self.nbytes = {k: int(np.prod(s, dtype=np.int64)) * self.dtype[k].itemsize for k, s in self.shape.items()}

    def make(self, name, factory=np.zeros):
        return factory(self.shape[name], self.dtype[name])


def split_rows(a, ends):
    """[a[0:ends[0]], a[ends[0]:ends[1]], ...] as views -- what np.split(a, ends[:-1]) returns, without its per-piece swapaxes round trip
    (a million pieces: 1 us each instead of 3)."""
    e = ends.tolist()
    return [a[s:t] for s, t in zip([0] + e[:-1], e)]


def unpack_dyn_bin(db, T):
    """[G4][nd][n] uint32 (4 seconds per word) -> [n, T, nd] uint8."""
    return unpack_dyn_val(db.view(np.uint8).reshape(db.shape + (4,)), T)     # little endian: byte w = column 4g+w


def unpack_dyn_val(dv, T):
    """[G4][nd][n][4] f32 -> [n, T, nd] f32."""
    G4, nd, n, _ = dv.shape
    return np.ascontiguousarray(dv.transpose(2, 0, 3, 1).reshape(n, G4 * 4, nd)[:, :T, :])


def pack_dyn_bin(db):
    """[n, T, nd] uint8 -> [G4][nd][n] uint32 (the inverse of unpack_dyn_bin; padding columns are 0)."""
    b = pack_dyn_val(np.asarray(db, dtype=np.uint8))
    return b.view(np.uint32).reshape(b.shape[:3])


def pack_dyn_val(dv):
    """[n, T, nd] f32 or f64 -> [G4][nd][n][4] of the same dtype (the inverse of unpack_dyn_val; padding columns are 0)."""
    dv = np.asarray(dv)
    n, T, nd = dv.shape
    G4 = TraceLayout(0, nd, n, T).G4
    b = np.zeros((n, G4 * 4, nd), dtype=dv.dtype)
    b[:, :T, :] = dv
    return np.ascontiguousarray(b.reshape(n, G4, 4, nd).transpose(1, 3, 0, 2))
