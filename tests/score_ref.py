"""A numpy restatement of the trace log-likelihood (DESIGN.md "Scoring a trace"), independent of the library's code: written from
dbn_sample.m:65-93 (per step), :97-135 (frozen), asub2ind.m:13-14 (column of the parents' bins, parents in ascending index) and
select_random.m:17-20 (an all-zero column is bin 1 with certainty), over the model's own arrays as em_io.em_read returns them.

tables(parms, alpha) builds the log tables; lib_tables(native model) reads the library's own (emgpu_model_log_prob), which is what the GPU
tests sum so that no libm difference enters their bitwise comparison.  score() does acc = acc + term, vectorised over trajectories and
sequential over the nodes and then over (t, k): the same IEEE additions in the same order as the definition."""
import numpy as np

AUTO, PER_STEP = 0, 1


def _log_table(N, alpha):
    """[r, q] counts -> [r, q] log(w / tot), tot added in ascending bin order; all-zero column: 0.0 for bin 1, -inf for the others"""
    P = np.asarray(N, dtype=np.float64) + alpha
    r, q = P.shape
    tot = np.zeros(q)
    for b in range(r):
        tot = tot + P[b]
    out = np.full((r, q), -np.inf)
    pos = tot > 0
    with np.errstate(divide="ignore"):
        out[:, pos] = np.log(P[:, pos] / tot[pos])
    out[0, ~pos] = 0.0
    return out


def tables(parms, alpha=0.0):
    """{"initial": [r x q per variable], "transition": {0-based node id: r x q}} from the counts of parms and a constant prior alpha"""
    t = {"initial": [_log_table(N, alpha) for N in parms["N_initial"]], "transition": {}}
    if int(parms.get("n_transition", 0)) > 0:
        for v, N in enumerate(parms["N_transition"]):
            if np.asarray(N).size:
                t["transition"][v] = _log_table(N, alpha)
    return t


def lib_tables(nm):
    """the same structure from the library's getter"""
    t = {"initial": [nm.log_prob(0, v + 1) for v in range(nm.n_initial)], "transition": {}}
    for v in range(nm.n_initial, nm.n_transition):
        t["transition"][v] = nm.log_prob(1, v + 1)
    return t


def graph(parms):
    g = {"ni": int(parms["n_initial"]), "G_i": np.asarray(parms["G_initial"]).astype(bool), "r_i": np.asarray(parms["r_initial"]).astype(np.int64),
         "order_i": np.asarray(parms["order_initial"]).astype(np.int64) - 1, "tm": np.zeros((0, 2), dtype=np.int64), "depend": False}
    if int(parms.get("n_transition", 0)) > 0:
        g["G_t"] = np.asarray(parms["G_transition"]).astype(bool)
        g["r_t"] = np.asarray(parms["r_transition"]).astype(np.int64)
        g["tm"] = np.asarray(parms["temporal_map"]).astype(np.int64).reshape(-1, 2) - 1
        new = g["tm"][:, 1]
        g["depend"] = bool(g["G_t"][np.ix_(new, new)].any())          # dbn_sample.m:55
    return g


def score(tabs, g, init_bin, dyn_bin=None, mode=AUTO):
    """init_bin [n, ni], dyn_bin [n, T, nd] or None (1-based bins) -> (log_lik [n], initial [n]).  A bin outside 1..r among init_bin and,
    for T > 1, columns 0 .. T-1 of dyn_bin makes that trajectory's log_lik NaN (initial: a bin of init_bin)."""
    ib = np.asarray(init_bin).astype(np.int64)
    n, ni = ib.shape
    bad = ((ib < 1) | (ib > g["r_i"][None, :])).any(axis=1)
    ib = np.clip(ib, 1, g["r_i"][None, :])
    acc = np.zeros(n)
    for v in g["order_i"]:
        col, stride = np.zeros(n, dtype=np.int64), 1
        for u in np.flatnonzero(g["G_i"][:, v]):
            col += stride * (ib[:, u] - 1)
            stride *= int(g["r_i"][u])
        acc = acc + tabs["initial"][v][ib[:, v] - 1, col]
    initial = np.where(bad, np.nan, acc)
    tm = g["tm"]
    if dyn_bin is not None and len(tm) and np.asarray(dyn_bin).shape[1] > 1:
        db = np.asarray(dyn_bin).astype(np.int64)
        T = db.shape[1]
        r_d = g["r_t"][tm[:, 1]]
        bad = bad | ((db < 1) | (db > r_d[None, None, :])).any(axis=(1, 2))
        db = np.clip(db, 1, r_d[None, None, :])
        per_step = mode == PER_STEP or g["depend"]
        old, new = list(tm[:, 0]), list(tm[:, 1])
        for t in range(1, T):
            for k in range(len(tm)):
                tv = new[k]
                col, stride = np.zeros(n, dtype=np.int64), 1
                for u in np.flatnonzero(g["G_t"][:, tv]):
                    if u >= ni:
                        b = db[:, t if per_step else 0, new.index(u)]       # a (t+1) node: column t
                    elif u in old:
                        b = db[:, t - 1 if per_step else 0, old.index(u)]   # the time-t node of a dynamic variable: column t-1
                    else:
                        b = ib[:, u]                                        # a static parent
                    col += stride * (b - 1)
                    stride *= int(g["r_t"][u])
                acc = acc + tabs["transition"][tv][db[:, t, k] - 1, col]
    return np.where(bad, np.nan, acc), initial


def same_bits(a, b):
    """bitwise equality of two f64 arrays, NaN lanes compared by isnan"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))
