"""A numpy restatement of the weighted sufficient statistics of a trace (include/emgpu.h "Counting a trace with integer
weights"), independent of the library's code and never calling it.  The observations, their cells and the parent bins per transition mode are
count_ref's (whose graph() / shapes() it imports); what is restated here is the weighting:
  - a trajectory of weight 0 is REMOVED first: it adds nothing and is not part of the bad-bin accounting, whatever its bins hold;
  - every observation of a remaining trajectory i adds weights[i] to its cell (np.add.at in uint64: exact, order-free);
  - an observation of a remaining trajectory whose own bin, or any parent bin it reads, is outside 1..r adds nothing and is counted in `skipped`.

wcount() takes the user-facing shapes and returns the two lists of [r, q] uint64 tables plus the number of skipped observations."""
import numpy as np

from count_ref import AUTO, PER_STEP, graph, shapes  # noqa: F401  (re-exported for the tests)


def wcount(g, init_bin, dyn_bin, weights, mode=AUTO, n_transition=None):
    """init_bin [n, ni], dyn_bin [n, T, nd] or None (1-based bins), weights [n] integers in 0 .. 2**32 - 1 -> (N_initial: list of [r, q]
    uint64 by variable id, N_transition: list by transition node id, (0, 0) where the node has no table, skipped observations)"""
    w = np.asarray(weights)
    assert w.ndim == 1 and w.dtype.kind in "iu" and (w.size == 0 or (int(w.min()) >= 0 and int(w.max()) <= 2**32 - 1))
    live = w > 0                                             # weight 0: removed before anything is looked at
    w = w[live].astype(np.uint64)
    ib = np.asarray(init_bin).astype(np.int64)[live]
    assert len(live) == np.asarray(init_bin).shape[0]
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
        N = np.zeros(shp_i[v], dtype=np.uint64)
        np.add.at(N, (ibc[ok, v] - 1, col[ok]), w[ok])
        skipped += int((~ok).sum())
        N_i.append(N)
    tm = g["tm"]
    nt = (len(g["r_t"]) if "r_t" in g else 0) if n_transition is None else int(n_transition)
    N_t = [np.zeros(shp_t.get(v, (0, 0)), dtype=np.uint64) for v in range(nt)]
    if dyn_bin is not None and len(tm) and np.asarray(dyn_bin).shape[1] > 1:
        db = np.asarray(dyn_bin).astype(np.int64)[live]
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
                np.add.at(N_t[tv], (dbc[ok, t, k] - 1, col[ok]), w[ok])
                skipped += int((~ok).sum())
    return N_i, N_t, skipped


def flat(tables):
    """the library's array of one network: the tables column-major, node after node (uint64)"""
    parts = [np.asarray(N, dtype=np.uint64).T.reshape(-1) for N in tables]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
