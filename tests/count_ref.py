"""A numpy restatement of the sufficient statistics of a trace (DESIGN.md "Counting a trace"), independent of the library's code: written
from the definition in include/emgpu.h, asub2ind.m:13-14 (column of the parents' bins, parents in ascending index), dbn_sample.m:65-93 (per
step) and :97-135 (frozen), over the graph score_ref.graph() reads from the model's own arrays.  It never calls the library.

count() takes the user-facing shapes and returns the two lists of [r, q] integer tables plus the number of skipped observations: an
observation whose own bin, or any parent bin it reads, is outside 1..r adds nothing; every other observation adds 1 (np.add.at).

With weights (include/emgpu.h "Counting a trace with integer weights") the observations, their cells and the parent bins are
the same; what changes is the weighting:
  - a trajectory of weight 0 is REMOVED first: it adds nothing and is not part of the bad-bin accounting, whatever its bins hold;
  - every observation of a remaining trajectory i adds weights[i] to its cell (np.add.at in uint64: exact, order-free);
  - an observation of a remaining trajectory whose own bin, or any parent bin it reads, is outside 1..r adds nothing and is counted in `skipped`."""
import numpy as np

from score_ref import AUTO, PER_STEP, graph  # noqa: F401  (re-exported for the tests)


def shapes(g):
    """([(r, q) per initial variable], {0-based transition node id: (r, q)}) from the graph alone"""
    ini = []
    for v in range(g["ni"]):
        q = 1
        for u in np.flatnonzero(g["G_i"][:, v]):
            q *= int(g["r_i"][u])
        ini.append((int(g["r_i"][v]), q))
    tr = {}
    for tv in g["tm"][:, 1]:
        q = 1
        for u in np.flatnonzero(g["G_t"][:, tv]):
            q *= int(g["r_t"][u])
        tr[int(tv)] = (int(g["r_t"][tv]), q)
    return ini, tr


def count(g, init_bin, dyn_bin=None, mode=AUTO, n_transition=None, weights=None):
    """init_bin [n, ni], dyn_bin [n, T, nd] or None (1-based bins), weights None or [n] integers in 0 .. 2**32 - 1 -> (N_initial: list of
    [r, q] tables by variable id (int64; uint64 with weights), N_transition: list by transition node id, (0, 0) where the node has no table,
    skipped observations)"""
    ib = np.asarray(init_bin).astype(np.int64)
    w, dtype = (lambda ok: 1), np.int64                          # what the observations `ok` add, and the tables' type
    if weights is not None:
        wt = np.asarray(weights)
        assert wt.ndim == 1 and wt.dtype.kind in "iu" and (wt.size == 0 or (int(wt.min()) >= 0 and int(wt.max()) <= 2**32 - 1))
        assert len(wt) == ib.shape[0]
        live = wt > 0                                            # weight 0: removed before anything is looked at
        wt, ib = wt[live].astype(np.uint64), ib[live]
        dyn_bin = None if dyn_bin is None else np.asarray(dyn_bin)[live]
        w, dtype = (lambda ok: wt[ok]), np.uint64
    n, ni = ib.shape
    shp_i, shp_t = shapes(g)
    ok_i = (ib >= 1) & (ib <= g["r_i"][None, :])
    ibc = np.clip(ib, 1, g["r_i"][None, :])
    skipped = 0
    N_i = []
    for v in range(ni):
        col, stride, ok = np.zeros(n, dtype=np.int64), 1, ok_i[:, v].copy()
        for u in np.flatnonzero(g["G_i"][:, v]):
            col += stride * (ibc[:, u] - 1)
            stride *= int(g["r_i"][u])
            ok &= ok_i[:, u]
        N = np.zeros(shp_i[v], dtype=dtype)
        np.add.at(N, (ibc[ok, v] - 1, col[ok]), w(ok))
        skipped += int((~ok).sum())
        N_i.append(N)
    tm = g["tm"]
    nt = (len(g["r_t"]) if "r_t" in g else 0) if n_transition is None else int(n_transition)
    N_t = [np.zeros(shp_t.get(v, (0, 0)), dtype=dtype) for v in range(nt)]
    if dyn_bin is not None and len(tm) and np.asarray(dyn_bin).shape[1] > 1:
        db = np.asarray(dyn_bin).astype(np.int64)
        T = db.shape[1]
        r_d = g["r_t"][tm[:, 1]]
        ok_d = (db >= 1) & (db <= r_d[None, None, :])
        dbc = np.clip(db, 1, r_d[None, None, :])
        per_step = mode == PER_STEP or g["depend"]
        old, new = list(tm[:, 0]), list(tm[:, 1])
        for t in range(1, T):
            for k in range(len(tm)):
                tv = new[k]
                col, stride, ok = np.zeros(n, dtype=np.int64), 1, ok_d[:, t, k].copy()
                for u in np.flatnonzero(g["G_t"][:, tv]):
                    if u >= ni:
                        c, j = (t if per_step else 0), new.index(u)            # a (t+1) node: column t
                        b, o = dbc[:, c, j], ok_d[:, c, j]
                    elif u in old:
                        c, j = (t - 1 if per_step else 0), old.index(u)        # the time-t node of a dynamic variable: column t-1
                        b, o = dbc[:, c, j], ok_d[:, c, j]
                    else:
                        b, o = ibc[:, u], ok_i[:, u]                           # a static parent
                    col += stride * (b - 1)
                    stride *= int(g["r_t"][u])
                    ok &= o
                np.add.at(N_t[tv], (dbc[ok, t, k] - 1, col[ok]), w(ok))
                skipped += int((~ok).sum())
    return N_i, N_t, skipped


def flat(tables):
    """the library's array of one network: the tables column-major, node after node (uint64)"""
    parts = [np.asarray(N, dtype=np.uint64).T.reshape(-1) for N in tables]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
