"""Shared helpers for the parity tests: run the HIP path and the oracle on the same inputs."""
import numpy as np

import oracle as O
from em_model_manned_bayes_amd import em_io, native, _lib as L

_cache = {}


def load_pair(name, model_dir, **read_kw):
    """(native model, oracle parms dict) for a packed model, both parsed from the SAME .txt file:
    the native one by the C++ loader, the oracle one by oracle.parse_model_txt."""
    key = (name, tuple(sorted(read_kw.items())))
    if key not in _cache:
        if name == "cor_v2p1_like":           # the generator-made stand-in for the absent cor_v2p1.txt
            from em_model_manned_bayes_amd import synthetic
            path = synthetic.write_correlated_v2p1_like(model_dir)
        else:
            path = em_io.materialize_model(name, model_dir)
        nm = native.NativeModel.load_txt(path, read_kw.get("idx_zero_boundaries", (1, 2, 3)), read_kw.get("is_overwrite_zero_boundaries", False))
        pp = O.parse_model_txt(path, read_kw.get("idx_zero_boundaries", (1, 2, 3)), read_kw.get("is_overwrite_zero_boundaries", False))
        _cache[key] = (nm, pp, path)
    return _cache[key]


def label_index(labels, name):
    q = '"%s"' % name
    return labels.index(q) + 1 if q in labels else 0


def uncor_indices(pp):
    labs = pp["labels_initial"]
    return dict(idx_L=label_index(labs, "L"), idx_v=label_index(labs, "v"), idx_dh=label_index(labs, "\\dot h"))


def assert_uncor_parity(got, ref, T, check_events=True, tol_rel=1e-6):
    """got: native.sample_dbn_host dict; ref: oracle.uncor_sample dict.
    Discrete state/event sequence bit-exact; dediscretised floats within tol_rel relative
    (north_star: 1e-6) -- and, because both sides round the same f64 expression to f32, we also
    require exact equality of the f32 values."""
    assert np.array_equal(got["init_bin"].astype(np.int32), ref["init_bin"]), "initial bins differ"
    assert np.array_equal(got["attempts"], ref["attempts"]), "rejection attempts differ"
    rv = ref["init_val"].astype(np.float32)
    np.testing.assert_allclose(got["init_val"], ref["init_val"], rtol=tol_rel, atol=0)
    assert np.array_equal(got["init_val"], rv), "initial values not bit-equal after f32 rounding"
    if "dyn_bin" in got:
        assert np.array_equal(got["dyn_bin"], ref["dense_bin"]), "dense bins differ"
        np.testing.assert_allclose(got["dyn_val"], ref["dense_val"], rtol=tol_rel, atol=0)
        assert np.array_equal(got["dyn_val"], ref["dense_val"].astype(np.float32)), "dense values not bit-equal"
    if check_events and "events" in got:
        for i, (e, r) in enumerate(zip(got["events"], ref["events"])):
            assert len(e) == r.shape[0], "trajectory %d: %d vs %d event rows" % (i, len(e), r.shape[0])
            assert np.array_equal(e["dt"].astype(np.float64), r[:, 0]), "trajectory %d: dt differs" % i
            assert np.array_equal(e["var"].astype(np.float64), r[:, 1]), "trajectory %d: var differs" % i
            assert np.array_equal(e["bin"].astype(np.float64), r[:, 3]), "trajectory %d: bin differs" % i
            np.testing.assert_allclose(e["value"], r[:, 2], rtol=tol_rel, atol=0)
            assert np.array_equal(e["value"], r[:, 2].astype(np.float32)), "trajectory %d: values not bit-equal" % i


def random_model(rs, dependent=None, nd=None, ni=None):
    """A random small model in the em_read dict layout (for em_io.em_write): random DAGs, sparse count tables
    (zero entries, all-zero columns), categorical and continuous variables, zero-crossing boundaries,
    zero and non-zero resample rates.  rs: numpy RandomState."""
    ni = int(ni or rs.randint(3, 8))
    r = rs.randint(2, 9, ni)
    if rs.rand() < 0.3:
        r[rs.randint(ni)] = rs.randint(9, 13)
    nd = int(nd or rs.randint(1, min(ni, 4) + 1))
    dyn = sorted(rs.choice(ni, nd, replace=False).tolist())
    Gi = np.zeros((ni, ni), dtype=np.uint8)
    for v in range(1, ni):
        cand = list(range(v))
        rs.shuffle(cand)
        q = 1
        for p in cand[: rs.randint(0, 4)]:
            if q * r[p] <= 400:
                Gi[p, v] = 1
                q *= r[p]
    nt = ni + nd
    rt = np.concatenate([r, r[dyn]])
    Gt = np.zeros((nt, nt), dtype=np.uint8)
    dependent = (rs.rand() < 0.5) if dependent is None else dependent
    for k, d in enumerate(dyn):
        v = ni + k
        Gt[d, v] = 1
        q = r[d]
        cand = [p for p in range(ni) if p != d]
        rs.shuffle(cand)
        for p in cand[: rs.randint(0, 3)]:
            if q * r[p] <= 600:
                Gt[p, v] = 1
                q *= r[p]
        if dependent and k > 0:
            for kk in range(k):
                if rs.rand() < 0.6 and q * rt[ni + kk] <= 900:
                    Gt[ni + kk, v] = 1
                    q *= rt[ni + kk]

    def counts(rv, parents_r):
        q = int(np.prod(parents_r)) if len(parents_r) else 1
        N = rs.randint(1, 2000, (rv, q)).astype(np.float64)
        N *= rs.rand(rv, q) < rs.choice([0.35, 0.6, 0.9])
        N[:, rs.rand(q) < 0.05] = 0                      # all-zero columns: select_random gives bin 1
        if rs.rand() < 0.3:
            N[:, rs.randint(q)] = 0
            N[rs.randint(rv), rs.randint(q)] = 1.56e9    # one huge count (dueregard-size)
        return N

    N_initial = [counts(r[v], r[Gi[:, v] > 0]) for v in range(ni)]
    N_transition = [np.zeros((0, 0))] * ni + [counts(rt[v], rt[Gt[:, v] > 0]) for v in range(ni, nt)]
    boundaries = []
    for v in range(ni):
        if v not in dyn and rs.rand() < 0.35:
            boundaries.append(np.zeros(0))               # categorical
            continue
        if rs.rand() < 0.6:                              # a bin that straddles 0 => zero bin (em_read.m:143-156)
            lo, hi = -rs.uniform(1, 50), rs.uniform(1, 50)
        else:
            lo = rs.uniform(0, 100); hi = lo + rs.uniform(1, 500)
        e = np.sort(np.round(rs.uniform(lo, hi, r[v] - 1), 3))
        boundaries.append(np.unique(np.concatenate([[np.round(lo, 3)], e, [np.round(hi, 3)]])) if len(np.unique(e)) == r[v] - 1 else np.round(np.linspace(lo, hi, r[v] + 1), 3))
    rates = np.where(rs.rand(ni) < 0.4, 0.0, np.round(rs.uniform(0.001, 0.25, ni), 6))
    labels_initial = ['"v%d"' % (v + 1) for v in range(ni)]
    labels_transition = ['"v%d(t)"' % (v + 1) if v in dyn else '"v%d"' % (v + 1) for v in range(ni)] + ['"v%d(t+1)"' % (d + 1) for d in dyn]
    return {"n_initial": ni, "n_transition": nt, "labels_initial": labels_initial, "labels_transition": labels_transition,
            "G_initial": Gi, "G_transition": Gt, "r_initial": r, "r_transition": rt, "N_initial": N_initial,
            "N_transition": N_transition, "boundaries": boundaries, "resample_rates": rates}


def assert_parting_only_on_a_threshold(got_attempts, ref_attempts, margins, tol, what):
    """.track parity, exact about every disagreement: GPU and oracle must accept the SAME attempt of every unit, except where the
    oracle's own decision margin of the attempt at which the two part (one side accepted it, the other rejected it) is below `tol`
    -- some value of that attempt sat on a threshold to within the last bits in which device and host arithmetic differ.
    margins[i, j]: smallest |value - threshold| / scale over every discrete decision of attempt j + 1 of unit i (oracle em_note).
    Returns the boolean mask of units that agree."""
    got_attempts, ref_attempts = np.asarray(got_attempts), np.asarray(ref_attempts)
    same = got_attempts == ref_attempts
    for i in np.flatnonzero(~same):
        g, r = int(got_attempts[i]), int(ref_attempts[i])
        j = min(x for x in (g, r) if x > 0)   # the earlier acceptance: the other side rejected this attempt (or never accepted)
        assert j - 1 < margins.shape[1], "%s %d: parted at attempt %d, beyond the recorded margins" % (what, i, j)
        m = margins[i, j - 1]
        assert m < tol, ("%s %d: GPU accepted attempt %d, oracle attempt %d, but no decision of attempt %d was closer than %.3g "
                         "to its threshold (tolerance %.3g): a real accept/reject difference" % (what, i, g, r, j, m, tol))
    return same


def f32_ulp_distance(a, b):
    """|a - b| counted in f32 representation steps (a, b: f32 arrays of one shape; +0 and -0 are 0 apart)."""
    ia = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def assert_f32_of_f64(got, ref, what="", abs_floor=1e-9):
    """`got` (f32, what the device stored) against `ref` (the oracle's f64): equal after rounding the oracle's value to f32, or ONE f32 step
    apart -- the device's and the host's f64 transcendental functions differ in their last bits (1e-15 relative), which moves a value
    across an f32 rounding boundary now and then but never further.  abs_floor: a value that is a difference of larger quantities (x_nm
    near the runway, a heading just past 0) carries their absolute error; below abs_floor the absolute difference is compared instead.
    Replaces rtol = atol = 1e-6 on the terminal tracks (the soak's worst observation was 6e-8 relative = half an f32 step)."""
    got = np.asarray(got, dtype=np.float32)
    ref = np.asarray(ref, dtype=np.float64)
    d = f32_ulp_distance(got, ref.astype(np.float32))
    bad = (d > 1) & (np.abs(got.astype(np.float64) - ref) > abs_floor)
    if bad.any():
        k = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d values more than one f32 step from the oracle, first at %s: %r vs %r"
                             % (what, int(bad.sum()), bad.size, tuple(k), got[tuple(k)], ref[tuple(k)]))
    return int(d.max()) if d.size else 0


def shaped_model(rs, ni, meff=(2, 2, 2), dependent=False, parents=None, rates=None, r=None):
    """A model in the em_read dict layout whose compiled plan is prescribed (the dispatch tests reach each kernel instance with one).
    meff: distinct real thresholds of every transition column of each dynamic variable (its length is the number of dynamic
    variables, initial variables 0 .. nd - 1): every column has exactly meff[k] + 1 nonzero bins, so EmgpuPlan::d_meff[k] = meff[k]
    and d_pw[k] = 4 (meff <= 3), 8 (<= 6) or 0 (7).
    parents: (cur, new) parent masks as emgpu_debug_parent_masks reports them, bit 4 k + q = dynamic variable k has the current
    (cur) / new (new) value of dynamic variable q as a transition parent (new parents must come earlier: q < k).  Default: each
    variable its own current value, plus the chain k <- k - 1 of new values when dependent.
    rates: resample rate per initial variable (default: 0.02 - 0.15 on the dynamic variables, 0 elsewhere).
    r: bins per initial variable (default: meff[k] + 1 .. meff[k] + 3 for the dynamic ones, at most 9; 2 .. 5 for the others).
    Dynamic variables are continuous (boundaries r + 1); the transition table of dynamic variable k also has static variable
    nd + k mod min(ni - nd, 4) as a parent.
    Every table, boundary set and default draws from a stream of its own (one seed taken from rs, then the part and the variable):
    two calls that differ in one argument differ only in what that argument reaches -- one more variable, one variable's bins or
    meff, the rates -- which is what an eligibility-edge pair needs."""
    meff = tuple(int(m) for m in meff)
    nd = len(meff)
    assert 1 <= nd <= 4 and nd <= ni
    base = int(rs.randint(2**31))

    def stream(part, v):
        return np.random.RandomState([base, part, v])

    if parents is None:
        cur = sum(1 << (5 * k) for k in range(nd))
        new = sum(1 << (4 * k + k - 1) for k in range(1, nd)) if dependent else 0
    else:
        cur, new = parents
    if r is None:
        r = [min(meff[v] + 1 + stream(1, v).randint(0, 3), 9) if v < nd else stream(1, v).randint(2, 6) for v in range(ni)]
    r = np.array(r, dtype=np.int64)
    for k in range(nd):
        assert meff[k] + 1 <= r[k]
    nt = ni + nd
    rt = np.concatenate([r, r[:nd]])
    Gi = np.zeros((ni, ni), dtype=np.uint8)
    for v in range(1, ni):
        p = stream(2, v).randint(v)
        if r[p] * r[v] <= 200:
            Gi[p, v] = 1
    Gt = np.zeros((nt, nt), dtype=np.uint8)
    for k in range(nd):
        for q in range(nd):
            if cur >> (4 * k + q) & 1:
                Gt[q, ni + k] = 1
            if new >> (4 * k + q) & 1:
                assert q < k, "a new-value parent must be an earlier dynamic variable"
                Gt[ni + q, ni + k] = 1
        if ni > nd:
            Gt[nd + k % min(ni - nd, 4), ni + k] = 1

    def counts(s, rv, q, m=None):
        N = s.randint(1, 2000, (rv, q)).astype(np.float64)
        if m is None:
            N *= s.rand(rv, q) < 0.7
            return N
        for j in range(q):             # exactly m + 1 nonzero bins: m distinct thresholds strictly between "always" and "never"
            keep = np.zeros(rv, dtype=bool)
            keep[s.choice(rv, m + 1, replace=False)] = True
            N[~keep, j] = 0
        return N

    N_initial = [counts(stream(3, v), r[v], int(np.prod(r[Gi[:, v] > 0]))) for v in range(ni)]
    N_transition = [np.zeros((0, 0))] * ni + [counts(stream(4, k), rt[ni + k], int(np.prod(rt[Gt[:, ni + k] > 0])), meff[k]) for k in range(nd)]
    boundaries = []
    for v in range(ni):
        s = stream(5, v)
        if v >= nd and s.rand() < 0.4:
            boundaries.append(np.zeros(0))
            continue
        lo = -s.uniform(1, 50) if s.rand() < 0.5 else s.uniform(0, 100)
        boundaries.append(np.round(np.linspace(lo, lo + s.uniform(5, 400), r[v] + 1), 3))
    if rates is None:
        rates = [np.round(stream(6, v).uniform(0.02, 0.15), 6) if v < nd else 0.0 for v in range(ni)]
    rates = np.asarray(rates, dtype=np.float64)
    assert rates.shape == (ni,)
    return {"n_initial": ni, "n_transition": nt, "labels_initial": ['"v%d"' % (v + 1) for v in range(ni)],
            "labels_transition": ['"v%d(t)"' % (v + 1) if v < nd else '"v%d"' % (v + 1) for v in range(ni)] + ['"v%d(t+1)"' % (k + 1) for k in range(nd)],
            "G_initial": Gi, "G_transition": Gt, "r_initial": r, "r_transition": rt, "N_initial": N_initial,
            "N_transition": N_transition, "boundaries": boundaries, "resample_rates": rates}


def plan_facts(nm, every=1):
    """What the plan compiler made of a native model, over EVERY transition column (the host-only debug hooks; every `every`-th column of
    a large table): per dynamic variable the distinct real thresholds of each column (min and max over the columns), d_meff, the padded
    width; the parent masks."""
    import ctypes as C
    lib = L.lib()
    cm, nw = C.c_uint32(), C.c_uint32()
    L.check(lib.emgpu_debug_parent_masks(nm._h, C.byref(cm), C.byref(nw)))
    out = {"cur": cm.value, "new": nw.value, "meff": [], "col_meff": [], "width": [], "r": []}
    for k in range(nm.n_dyn):
        tvar, r, q, meff, mp = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_uint32()
        thr = np.zeros(64, dtype=np.uint32)
        full = np.zeros(64, dtype=np.uint32)         # a whole row: EMGPU_MAX_R - 1 thresholds at most
        cthr = np.zeros(7, dtype=np.uint32)
        width, pw = C.c_int32(), np.zeros(8, dtype=np.uint32)
        lo, hi = 99, -1
        col, ncol = 0, 1
        weights = None
        while col < ncol:
            L.check(lib.emgpu_debug_dynamic_column(nm._h, k, col, C.byref(tvar), C.byref(r), C.byref(q), thr.ctypes.data, C.byref(meff),
                                                   cthr.ctypes.data, C.byref(mp)))
            L.check(lib.emgpu_debug_padded_column(nm._h, k, col, C.byref(width), pw.ctypes.data))
            row = thr[: r.value - 1]
            if r.value - 1 > 15:
                # the hook hands out a row's first 15 thresholds; a longer row is counted in full on the thresholds the same compiler
                # makes of the column's weights (counts + prior), which must begin with the 15 the plan holds
                if weights is None:
                    weights = (nm.get_f64(L.F_N_TRANSITION, tvar.value) + nm.get_f64(L.F_ALPHA_TRANSITION, tvar.value)).reshape(q.value, r.value)
                w = np.ascontiguousarray(weights[col])
                L.check(lib.emgpu_debug_column_thresholds(w.ctypes.data, r.value, full.ctypes.data))
                row = full[: r.value - 1]
                assert np.array_equal(row[:15], thr[:15]), (k, col)
            d = len(set(int(x) for x in row if 0 < x < 0xFFFFFFFF))
            lo, hi = min(lo, d), max(hi, d)
            ncol = q.value
            col += every
        out["meff"].append(meff.value)
        out["col_meff"].append((lo, hi))
        out["width"].append(width.value)
        out["r"].append(r.value)
    return out


def load_row_model(spec, model_dir):
    """(native model, oracle parms dict, path) of an instances.py model: a shipped model's name, or util.shaped_model arguments
    (+ "seed"), written once per session under model_dir."""
    if isinstance(spec, str):
        return load_pair(spec, model_dir)
    key = ("shaped",) + tuple(sorted((k, repr(v)) for k, v in spec.items()))
    if key not in _cache:
        import hashlib
        import os
        kw = dict(spec)
        rs = np.random.RandomState(kw.pop("seed"))
        path = os.path.join(model_dir, "shaped_%s.txt" % hashlib.sha1(repr(key).encode()).hexdigest()[:16])
        em_io.em_write(shaped_model(rs, **kw), path)
        _cache[key] = (native.NativeModel.load_txt(path), O.parse_model_txt(path), path)
    return _cache[key]


# ---- terminal trajectory models of any shape (tests/terminal_shapes.py)
TERMINAL_VARS = ("distance", "bearing", "heading", "altitude", "speed")     # initial variables 2 .. 6 (variable 1 is the intent)
TERMINAL_RANGE = {"distance": (0.0, 8.0), "bearing": (0.0, 360.0), "heading": (0.0, 360.0), "altitude": (200.0, 5000.0), "speed": (75.0, 450.0)}
TERMINAL_PARENTS = {"heading": ("distance", "bearing"), "altitude": ("distance", "bearing", "heading"), "speed": ("distance", "bearing", "heading")}


def terminal_model(seed, bins=(7, 36, 36, 7, 5), grids=None, n_intent=3, parents=None, table="sparse", zero_frac=0.02, reverse=False,
                   unordered_parents=False, grid_seed=None, alt_drift=0):
    """A terminal trajectory model (initial variables intent, distance, bearing, heading, altitude, speed; dynamic heading, altitude,
    speed) in the em_read dict layout, of any shape.
    bins: bins of distance, bearing, heading, altitude, speed.
    grids: per variable name "shipped" (synthetic's guess of the trained grids; needs the shipped bin count), "uniform", "nonuniform"
    (random bin widths, up to 49 : 1, cut points rounded to 3 decimals) or an explicit boundary list; every grid spans
    TERMINAL_RANGE so that one geometry sample serves every shape; the random ones draw from grid_seed (default: seed), which the ten
    models of a directory share.  Default: "shipped" where the bin count allows it, else "uniform".
    parents: per dynamic variable the OTHER parents of its (t+1) node, as names out of "intent" and TERMINAL_VARS (default
    TERMINAL_PARENTS, the graph of the reference's doc/model_terminal_traj_fwd.png).  The variable's own current value is always added.
    THE OWN VALUE MUST BE THE LAST PARENT: setTransitionPriors.m:20-27 puts the stay prior of bin kk on columns n (kk - 1) + 1 .. n kk, which
    are "own value = kk" only when the own value is the slowest-varying parent, i.e. the parent with the highest variable index (asub2ind.m
    walks the parents in index order).  A parent above it (speed for altitude(t+1), say) moves the prior onto other bins: an all-zero
    column may then allow only an invalid bin, and the reference's re-draw loop (createEncounter.m:192) never ends.  So a parent may only
    be a variable with a lower index than the node's own; unordered_parents=True lifts the check (the test of this very rule).
    table: "sparse" = a stay mass plus the two neighbours plus a rare far jump (at most 4 distinct thresholds per column: what the compact
    c8 form decides alone); "dense" = every bin nonzero around a stay mass of 70 - 85 % (r - 1 distinct thresholds per column).
    alt_drift: -1 / +1 adds mass to the next lower / higher altitude bin (sparse tables; synthetic.terminal_trajectory_model's rule: a
    landing descends, a take-off climbs, so that the vertical-intent filters of CorTerminalModel.track accept some tracks).
    zero_frac: share of all-zero columns (unobserved parent configurations; the stay prior alone decides them).
    Every table and grid draws from a stream of its own (seed, part, variable): two calls that differ in one argument differ only in
    what that argument reaches."""
    from em_model_manned_bayes_amd import synthetic
    bins = dict(zip(TERMINAL_VARS, (int(b) for b in bins)))
    grids = dict(grids or {})
    parents = {**TERMINAL_PARENTS, **(parents or {})}
    names = ("intent",) + TERMINAL_VARS

    def stream(part, v):
        return np.random.RandomState([int(seed) & 0x7FFFFFFF, part, v])

    bnd = {}
    for v, name in enumerate(TERMINAL_VARS):
        lo, hi = TERMINAL_RANGE[name]
        g = grids.get(name, "shipped" if len(synthetic._BND[name]) == bins[name] + 1 else "uniform")
        if isinstance(g, str) and g == "shipped":
            b = synthetic._BND[name]
        elif isinstance(g, str) and g == "uniform":
            b = np.linspace(lo, hi, bins[name] + 1)
        elif isinstance(g, str) and g == "nonuniform":
            w = np.random.RandomState([int(seed if grid_seed is None else grid_seed) & 0x7FFFFFFF, 1, v]).uniform(0.25, 1.75, bins[name]) ** 2          # bin widths up to 49 : 1
            cut = np.round(lo + np.cumsum(w)[:-1] * ((hi - lo) / w.sum()), 3)
            b = np.concatenate([[lo], cut, [hi]])
        else:
            b = np.asarray(g, dtype=np.float64)
        assert len(b) == bins[name] + 1 and np.all(np.diff(b) > 0) and (b[0], b[-1]) == (lo, hi), (name, b)
        bnd[name] = np.asarray(b, dtype=np.float64)

    r_i = np.array([n_intent] + [bins[n] for n in TERMINAL_VARS], dtype=np.int32)
    dyn = ("heading", "altitude", "speed")
    r_t = np.concatenate([r_i, [bins[n] for n in dyn]]).astype(np.int32)
    G_t = np.zeros((9, 9), dtype=bool)
    for k, name in enumerate(dyn):
        own = names.index(name)
        for p in parents[name]:
            assert unordered_parents or names.index(p) < own, "%s(t+1): parent %s comes after the node's own variable (see the docstring)" % (name, p)
            G_t[names.index(p), 6 + k] = True
        G_t[own, 6 + k] = True

    def table_of(k, name):
        s, r_own = stream(2, k), bins[name]
        own = names.index(name)
        par = np.flatnonzero(G_t[:, 6 + k])
        q = int(np.prod(r_t[par]))
        stride = int(np.prod(r_t[par[par < own]]))            # asub2ind: parents with a lower index vary faster
        cur = (np.arange(q) // stride) % r_own
        cols = np.arange(q)
        wrap = name == "heading"
        if table == "sparse":
            N = np.zeros((r_own, q))
            N[cur, cols] = s.randint(60, 400, q)
            for d in (-1, 1):
                nb = np.mod(cur + d, r_own) if wrap else np.clip(cur + d, 0, r_own - 1)
                N[nb, cols] += s.randint(0, 30, q) * (s.rand(q) < 0.7)
            if alt_drift and name == "altitude":
                N[np.clip(cur + alt_drift, 0, r_own - 1), cols] += s.randint(40, 160, q)
            N[s.randint(0, r_own, q), cols] += s.randint(0, 6, q) * (s.rand(q) < 0.15)
        else:
            assert table == "dense", table
            N = s.randint(1, 40, (r_own, q)).astype(np.float64)
            N[cur, cols] += np.round(N.sum(axis=0) * s.uniform(2.5, 6.0, q))
        N[:, s.rand(q) < zero_frac] = 0
        return N

    tag = "(t-1)" if reverse else "(t+1)"
    labels_i = ['"%s"' % n for n in names]
    labels_t = ['"intent"', '"distance"', '"bearing"'] + ['"%s(t)"' % n for n in dyn] + ['"%s%s"' % (n, tag) for n in dyn]
    return {"n_initial": 6, "n_transition": 9, "labels_initial": labels_i, "labels_transition": labels_t,
            "G_initial": np.zeros((6, 6), dtype=bool), "G_transition": G_t, "r_initial": r_i, "r_transition": r_t,
            "N_initial": [np.ones((int(r), 1)) for r in r_i], "N_transition": [np.zeros((0, 0))] * 6 + [table_of(k, n) for k, n in enumerate(dyn)],
            "boundaries": [np.zeros(0)] + [bnd[n] for n in TERMINAL_VARS], "resample_rates": np.zeros(6)}


def terminal_uses_intent(spec):
    return any("intent" in p for p in (spec.get("parents") or {}).values())


def write_terminal_shape_directory(out_dir, seed=0x5EED0011, src="terminalradar", edit=None, vertical_intent=False, **spec):
    """A correlated_terminal/<src> directory for one shape: the shipped geometry model plus ten terminal_model files under
    synthetic.TERMINAL_FILE_STEMS, all of one shape and one set of boundaries (the library propagates all ten from one plan and refuses
    anything else), model k drawn from seed + k.  The ownship models have 2 intents and the intruder models 3 -- unless the intent is a
    parent of a (t+1) node: its bin count is then part of the table layout, and all ten get 3 (an ownship never has intent 3).
    vertical_intent: landing models drift down and take-off models up in forward time (alt_drift; the other way in the reverse models).
    edit(k, model): a last change to model k before it is written (the refusal and re-draw-cap variants).  Returns the directory."""
    import os
    from em_model_manned_bayes_amd import synthetic
    os.makedirs(out_dir, exist_ok=True)
    name = {"terminalradar": "terminal_v3_radar_encounter_model", "opensky": "terminal_v3_opensky_encounter_model"}[src]
    em_io.materialize_model(name, out_dir)
    for k, stem in enumerate(synthetic.TERMINAL_FILE_STEMS):
        n_intent = 3 if terminal_uses_intent(spec) or not stem.startswith("ownship") else 2
        rev = stem.endswith("reverse")
        drift = (-1 if "landing" in stem else (1 if "takeoff" in stem else 0)) * (-1 if rev else 1) if vertical_intent else 0
        m = terminal_model(seed + k, n_intent=n_intent, reverse=rev, grid_seed=seed, alt_drift=drift, **spec)
        if edit is not None:
            m = edit(k, m) or m
        em_io.em_write(m, os.path.join(out_dir, name.replace("encounter_model", "") + stem + ".txt"))
    return out_dir


# dynamic-limit rows (minVel maxVel maxTurnRate maxAltitude maxVertRate for aircraft 1 and 2) of the shape tests: the GENERIC type twice, and
# a pair whose speed and altitude limits lie INSIDE bins of every grid of terminal_shapes.py (never on a boundary: a speed clamped onto a cut
# point would be binned by the last bit of norm(v)), so that altitude and speed events are drawn again (createEncounter.m:218-238)
TERMINAL_LIMITS = {"generic": np.array([[50, 506, 12, 5000, 100], [50, 506, 12, 5000, 100]], dtype=np.float64),
                   "inside": np.array([[111.37, 388.21, 7, 3217.9, 41.7], [68.53, 186.31, 3, 1203.4, 8.3]], dtype=np.float64)}


# The hand-made half is propagated with other turn-rate limits than the sampled half.  An aircraft that starts ON an axis, heading along it,
# and turns at a rate LIMIT takes the directions axis + k * rate: when its target changes sides it comes back through the axis direction,
# its lateral steps cancel (sin(a + r) = -sin(a - r)) and it is back on the axis to within rounding noise (1e-17 NM, either sign) -- the
# bearing bin of such a position (0 or 360 degrees on the +x axis) is as ill-conditioned as on a diagonal.  With maxTurnRate = 0 the aircraft
# never turns: it stays exactly on its cut direction for its whole life, or leaves it for good along the heading a speed event gives it
# (createEncounter.m:246).  (An unlimited rate is no way out: a turn is rounded to 0.01 degrees, createEncounter.m:241, so from an axis-aligned
# heading it lands on 360.00 exactly now and then, where the reference's heading is 0 or 360 by the sign of a 1e-14 velocity component.)
TERMINAL_HAND_TURN = {"generic": 0.0, "inside": 0.0}


def terminal_hand_limits(name):
    dl = TERMINAL_LIMITS[name].copy()
    dl[:, 2] = TERMINAL_HAND_TURN[name]
    return dl


def terminal_model_of(own_intent, int_intent):
    """createEncounter.m:13-38: the models of the four tracks of an encounter, as positions in synthetic.TERMINAL_FILE_STEMS."""
    return [2 * (own_intent - 1), 2 * (own_intent - 1) + 1, 4 + 2 * (int_intent - 1), 4 + 2 * (int_intent - 1) + 1]


def terminal_hand_geo(n):
    """n hand-made geometry rows (x0 y0 z0 v0 heading0 intent for aircraft 1 and 2) + model_of: aircraft ON the four axes (x = 0 or y = 0)
    heading 0, 90, 180 or 270 along their axis, towards the runway and away from it, 0.26 to 6.5 NM out -- positions that stay on a cut
    direction of every bearing grid with a cut point at a multiple of 90, which sampled geometry never produces.  At 0.26 NM the intent
    and ownship end conditions (createEncounter.m:296-329) trigger within seconds.  No diagonals: cosd(45) v and sind(45) v are not the
    same double, the track leaves the diagonal by one ulp, and which side of the cut it is on is ill-conditioned by construction."""
    states = []
    for d in (0.26, 1.0, 2.5, 4.0, 6.5):
        for ax, (ux, uy) in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))):
            away = 90.0 * ax                                   # the heading that points from the runway along this axis
            for hdg in (away, (away + 180.0) % 360.0):
                states.append((d * ux + 0.0, d * uy + 0.0, hdg))
    # altitudes and speeds OFF every cut point of every grid of terminal_shapes.py (uniform grids put cut points on round numbers such as
    # 200 ft/s and 2600 ft): the reference bins norm(v) of the rotated velocity, which leaves a speed that sits on a cut point by an ulp
    alts, speeds = (251.3, 903.7, 1811.9, 2597.3, 3389.1, 4793.3), (81.3, 139.7, 203.9, 291.1, 357.7, 441.3)
    geo, mo = np.zeros((n, 12)), np.zeros((n, 4), dtype=np.int32)
    for e in range(n):
        own, intr = states[e % len(states)], states[(7 * e + 3 + e // len(states)) % len(states)]
        oi, ii = 1 + e % 2, 1 + (e // 2) % 3
        geo[e, :6] = [own[0], own[1], alts[e % 6], speeds[(e // 3) % 6], own[2], oi]
        geo[e, 6:] = [intr[0], intr[1], alts[(e // 5) % 6], speeds[(e + 2) % 6], intr[2], ii]
        mo[e] = terminal_model_of(oi, ii)
    return geo, mo


def terminal_sampled_geo(model_dir, n, seed, src="terminal_v3_radar_encounter_model"):
    """n geometry rows + model_of drawn from the shipped geometry model by the oracle's restatement of @CorTerminalModel/sample.m and
    createEncounter.m:13-49 (GENERIC speed limits): what CorTerminalModel.sample + _geo_rows give on the GPU."""
    import pyref
    key = ("terminal_geo", src, n, seed)
    if key not in _cache:
        pp = O.parse_model_txt(em_io.materialize_model(src, model_dir))
        labs = pp["labels_initial"]
        _, val, _ = O.geom_sample(O.OracleModel(pp), n, seed, idx_own_speed=labs.index('"own_speed"') + 1, idx_int_speed=labs.index('"int_speed"') + 1,
                                  lim1=(50, 506), lim2=(50, 506))
        names = [x.replace('"', "") for x in labs]
        rows = [pyref.create_encounter_inputs(dict(zip(names, v.astype(np.float32).astype(np.float64)))) for v in val]
        _cache[key] = (np.array([r[0] for r in rows], dtype=np.float64), np.array([r[1] for r in rows], dtype=np.int32))
    return _cache[key]


def terminal_test_geo(model_dir, n, seed=0x5EED0012):
    """The geometry of the shape tests: half sampled, half hand-made (in this order)."""
    a, b = terminal_sampled_geo(model_dir, n // 2, seed), terminal_hand_geo(n - n // 2)
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


def terminal_shape_models(directory, native_too=True):
    """(native models with the stay prior, oracle models with it, files) of a write_terminal_shape_directory directory, in
    synthetic.TERMINAL_FILE_STEMS order -- every intent with its own reverse model."""
    import glob
    import os
    from em_model_manned_bayes_amd import synthetic
    nms, oms, files = [], [], []
    for stem in synthetic.TERMINAL_FILE_STEMS:
        f = glob.glob(os.path.join(directory, "*_" + stem + ".txt"))[0]
        files.append(f)
        pp = O.parse_model_txt(f)
        oms.append(O.OracleModel(pp, alpha_transition=O.stay_prior_alpha(pp, 1.0)))      # createEncounter.m:128-129
        if native_too:
            nm = native.NativeModel.load_txt(f)
            nm.set_transition_stay_prior(1.0)
            nms.append(nm)
    return nms, oms, files


def terminal_refusal_variants(spec):
    """The sets of ten trajectory models the library refuses (terminal_tables in emgpu_terminal.cpp), as (id, words of the message, edit) with
    edit an argument of write_terminal_shape_directory(**spec): each is loadable -- the refusal is the terminal entry points' own."""
    def seven_initial(k, m):
        m = dict(m)
        Gt = np.zeros((10, 10), dtype=bool)
        old = [0, 1, 2, 3, 4, 5, 7, 8, 9]
        Gt[np.ix_(old, old)] = m["G_transition"]
        lt = m["labels_transition"]
        m.update(n_initial=7, n_transition=10, labels_initial=m["labels_initial"] + ['"extra"'], labels_transition=lt[:6] + ['"extra"'] + lt[6:],
                 G_initial=np.zeros((7, 7), dtype=bool), G_transition=Gt, r_initial=np.append(m["r_initial"], 2),
                 r_transition=np.concatenate([m["r_initial"], [2], m["r_transition"][6:]]), N_initial=m["N_initial"] + [np.ones((2, 1))],
                 N_transition=[np.zeros((0, 0))] * 7 + m["N_transition"][6:], boundaries=m["boundaries"] + [np.zeros(0)], resample_rates=np.zeros(7))
        return m

    def speed_after_altitude(k, m):
        m = dict(m, G_transition=m["G_transition"].copy(), N_transition=list(m["N_transition"]))
        m["G_transition"][7, 8] = True                             # speed(t+1) <- altitude(t+1): the slowest-varying parent of all
        m["N_transition"][8] = np.tile(m["N_transition"][8], (1, int(m["r_transition"][7])))
        return m

    def initial_out_of_order(k, m):
        m = dict(m, G_initial=m["G_initial"].copy(), N_initial=list(m["N_initial"]))
        m["G_initial"][5, 1] = True                                # speed -> distance: the topological order is no longer 1 .. 6
        m["N_initial"][1] = np.ones((int(m["r_initial"][1]), int(m["r_initial"][5])))
        return m

    def distance_dynamic(k, m):
        m = dict(m, G_transition=m["G_transition"].copy(), N_transition=list(m["N_transition"]), r_transition=m["r_transition"].copy())
        lt = list(m["labels_transition"])
        lt[1], lt[3], lt[6] = '"distance(t)"', '"heading"', lt[6].replace("heading", "distance")
        rd = int(m["r_initial"][1])
        m["labels_transition"] = lt
        m["r_transition"][6] = rd
        m["G_transition"][:, 6] = False
        m["G_transition"][1, 6] = True
        m["N_transition"][6] = np.ones((rd, rd)) + 50 * np.eye(rd)
        return m

    def categorical_heading(k, m):
        b = list(m["boundaries"])
        b[3] = np.zeros(0)
        return dict(m, boundaries=b)

    def too_many_cut_points(k, m):
        b = list(m["boundaries"])
        b[2] = np.linspace(0.0, 360.0, 67)                        # 65 cut points on the bearing variable
        return dict(m, boundaries=b)

    def one_boundary_differs(k, m):
        if k == 3:
            b = list(m["boundaries"])
            b[4] = b[4].copy()
            b[4][1] += 0.5
            m = dict(m, boundaries=b)
        return m

    def one_differs_in_r(k, m):
        if k == 3:
            bins = list(spec["bins"])
            bins[3] += 1
            m = terminal_model(77, n_intent=int(m["r_initial"][0]), **dict(spec, bins=tuple(bins)))
        return m

    six_three = "6 initial and 3 independent dynamic variables"
    return [("seven_initial_variables", six_three, seven_initial), ("speed_depends_on_new_altitude", six_three, speed_after_altitude),
            ("initial_network_out_of_order", "initial network must be in index order", initial_out_of_order),
            ("distance_is_dynamic", "must be heading, altitude and speed", distance_dynamic),
            ("categorical_heading", "need boundaries", categorical_heading),
            ("65_cut_points", "more than 64 cut points", too_many_cut_points),
            ("one_boundary_differs", "differ in shape or boundaries", one_boundary_differs),
            ("one_differs_in_r", "differ in shape or boundaries", one_differs_in_r)]
