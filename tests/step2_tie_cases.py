"""Shared inputs of test_step2_ties.py / test_gpu_step2_ties.py: tie-dense models for k_dbn_step2, a numpy restatement of how the kernel
decides a draw (emgpu_kernels_step2.h: pk_fired2, plain_fired7, or_half with the zt words, exact_borrows, exact_hit) over the draws of an
oracle sample, and the count of every kind of tie in that sample (a plain module, like start_grid_cases.py).

A draw's high halfword ties with a threshold's about (thresholds) / 65 536 of the time, so the few hundred trajectories of an instances.py
row hold none.  The COUNTED run of each model is 65 536 x 64 from FIRST: its ties are counted by kind from the oracle's own trace before a
GPU run of it is trusted -- KINDS lists the kinds and their floors, NOT_APPLICABLE the kinds a model cannot have, each with the reason.

The restatement takes the column of every (trajectory, second, variable) from the oracle's trace (the initial bins, the bins of the second
before, this second's bins of the new-value parents; asub2ind strides), the column's packed and padded words from the plan compiler's debug
hooks and the draws from the slot map (oracle.philox4x32_np).  It asserts on the way that its bin equals the oracle's at every draw: the
decided ones from the high halfword alone, the tied ones from the 32-bit redo."""
import ctypes as C
import os

import numpy as np

import instances as I
import oracle as O
from em_model_manned_bayes_amd import em_io, native, _lib as L
from util import label_index, load_pair, shaped_model

N, T, FIRST = 65536, 64, 2**33 + 11
SEC_TRANS, SEC_RES, SEC_LO = 3, 4, 6        # emgpu_plan.h: TRANS, RES; the low halfwords sit 6 sections further on (TRANS_LO 9, RES_LO 10)
BIG = 3_000_000                             # a count beside which a count of 1 - 40 is a probability below 2^-16
R_LO, R_HI = 2.0 ** -16 - 2.0 ** -17, 1.0 - 2.0 ** -16 - 2.0 ** -17    # Bernoulli thresholds 0x00008000 and 0xFFFE8000: a tie is hit or no hit alike
ALL_MASKS = {3: (0x0777, 0x0310), 4: (0xFFFF, 0x7310)}                 # kCurAll3 / kNewAll3, kCurAll4 / kNewAll4: the general instances


# ---- the models -------------------------------------------------------------------------------------------------------------------
def column_kinds(m):
    """The kinds a variable of meff m carries, column by column in rotation."""
    if m == 1:
        return ["below16", "none", "ordinary"]
    return ["below16", "shared", "one", "none", "ordinary"] + (["two"] if m >= 3 else [])


def edit_table(Nt, m, rotate=0):
    """Edits the columns of one transition table (r x q counts, meff m) in rotation:
      below16   m real thresholds, the first below 2^16 (H = 0)
      shared    m real thresholds, the first two five counts apart: one high half
      one, two  one / two real thresholds: the other slots hold padding copies (0x10000 in the plain form past the variable's meff)
      none      no real threshold (the last bin always)
      ordinary  left as it is.
    The counts vary with the column, so that the tied thresholds' low halfwords do.  rotate: where the rotation starts (a table of a few
    columns of which the trajectories visit one: the kind of that column is chosen with it)."""
    r, q = Nt.shape
    assert r >= m + 1
    kinds = column_kinds(m)
    P = len(kinds)
    for j in range(q):
        kind = kinds[(j + j // P + rotate) % P]       # (a parent with P bins as the fastest one would otherwise decide the kind alone)
        if kind == "ordinary":
            continue
        b = BIG + 997 * (j % 1021)
        c = np.zeros(r + m)
        s = (j // P) % (r - m)               # the first bin with a count: the bins a trajectory visits vary too
        if kind == "below16":
            c[s] = 7 + j % 5
            c[s + 1: s + m + 1] = b + 13 * np.arange(m)
        elif kind == "shared":
            c[s], c[s + 1] = b, 5
            c[s + 2: s + m + 1] = 2 * b + 4321 + 13 * np.arange(m - 1)      # (equal counts would put the pair on either side of 2^31)
        elif kind == "one":
            c[s], c[s + 1] = b, 3 * b + 12345
        elif kind == "two":
            c[s], c[s + 1], c[s + 2] = b, b + 777, 2 * b
        else:
            c[(r - 1 - j // P) % r] = 1234
        Nt[:, j] = c[:r]


def _dyn_ivars(p):
    """0-based initial variable of every row of the temporal map, from the labels (em_read.m:158-177)."""
    return [v for v, lab in enumerate(p["labels_transition"][: int(p["n_initial"])]) if "(t)" in lab]


def _tie_parms(base, rates, model_dir, rotate=None):
    """The em_read dict of a tie model: util.shaped_model arguments, or a shipped model's own dict with its tables edited (every
    variable keeps its meff: the below16 and shared columns have exactly that many real thresholds, no column has more)."""
    if isinstance(base, dict):
        kw = dict(base)
        rs = np.random.RandomState(kw.pop("seed"))
        ni, meff = kw["ni"], kw["meff"]
        full = [0.0] * ni
        full[: len(rates)] = rates
        p = shaped_model(rs, **dict(kw, rates=full))
        for k, m in enumerate(meff):
            edit_table(p["N_transition"][ni + k], m)
        return p
    nm, _, path = load_pair(base, model_dir)
    meff = plan_meff(nm)
    p = dict(em_io.em_read(path))
    p.pop("native")
    ni = int(p["n_initial"])
    p["N_transition"] = [np.array(a, dtype=np.float64) for a in p["N_transition"]]
    tvars = sorted(meff)
    for n, tv in enumerate(tvars):
        edit_table(p["N_transition"][tv], meff[tv], rotate[n] if rotate else 0)
    rr = np.array(p["resample_rates"], dtype=np.float64)
    dyn = _dyn_ivars(p)
    for v, rate in zip(dyn, rates):
        rr[v] = rate
    p["resample_rates"] = rr
    assert len(p["N_transition"]) == int(p["n_transition"]) and all(p["N_transition"][v].size == 0 for v in range(ni))
    return p


def plan_meff(nm):
    """{0-based transition variable: d_meff} of a native model."""
    out = {}
    for k in range(nm.n_dyn):
        tvar, r, q, meff, mp = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_uint32()
        thr, cthr = np.zeros(64, dtype=np.uint32), np.zeros(7, dtype=np.uint32)
        L.check(L.lib().emgpu_debug_dynamic_column(nm._h, k, 0, C.byref(tvar), C.byref(r), C.byref(q), thr.ctypes.data, C.byref(meff),
                                                   cthr.ctypes.data, C.byref(mp)))
        out[tvar.value - 1] = meff.value
    return out


NOT_A_FAMILY = I.NOT_A_FAMILY
# name: base (instances.shaped arguments or a shipped model), the rates of the first dynamic variables (the others keep theirs), SEED of the
# counted run, per_step, and the kernel every form must report: "both" the dense trace, "list+dense", "list", and the +start twins
MODELS = {
    "g73w4": dict(base=I.shaped(721, 6, (2, 3, 3), parents=NOT_A_FAMILY), rates=[R_LO, R_HI, 0.07], seed=0x57E2,
                  kernels={"both": "k_dbn_step2<7,3,w4,reg>"}),
    "g73w8": dict(base=I.shaped(722, 6, (5, 4, 6), parents=NOT_A_FAMILY), rates=[R_LO, R_HI, 0.07], seed=0x57E2,
                  kernels={"both": "k_dbn_step2<7,3,w8,reg>"}),
    "g73mix": dict(base=I.shaped(723, 7, (2, 5, 3), parents=NOT_A_FAMILY), rates=[R_LO, R_HI, 0.07], seed=0x57E2,
                   kernels={"both": "k_dbn_step2<7,3,reg>", "start": "k_dbn_step2<7,3>+start"}),
    "g73r0": dict(base=I.shaped(724, 7, (3, 4, 2), dependent=True), rates=[R_LO, 0.0, R_HI], seed=0x57E2,
                  kernels={"both": "k_dbn_step2<7,3>"}),
    "g93w8": dict(base=I.shaped(922, 8, (6, 5, 4), dependent=True), rates=[R_LO, R_HI, 0.07], seed=0x57E2,
                  kernels={"both": "k_dbn_step2<9,3,w8,reg>"}),
    "g93mix": dict(base=I.shaped(923, 9, (2, 6, 3), dependent=True), rates=[R_LO, R_HI, 0.07], seed=0x57E8,
                   kernels={"both": "k_dbn_step2<9,3,reg>", "list+dense": "k_dbn_step2<9,3,reg>+events"}),
    "g164w4": dict(base=I.shaped(1641, 8, (2, 3, 3, 3), dependent=True), rates=[R_LO, R_HI, 0.07, 0.11], seed=0x57E2,
                   kernels={"both": "k_dbn_step2<16,4,w4,reg>"}),
    "g164w8": dict(base=I.shaped(1642, 8, (4, 5, 6, 4), dependent=True), rates=[R_LO, R_HI, 0.07, 0.11], seed=0x57E2,
                   kernels={"both": "k_dbn_step2<16,4,w8,reg>"}),
    "g164mix": dict(base=I.shaped(1643, 8, (2, 5, 3, 6), dependent=True), rates=[R_LO, R_HI, 0.07, 0.11], seed=0x57E2,
                    kernels={"both": "k_dbn_step2<16,4,reg>", "list": "k_dbn_step2<16,4,reg>+rows-by-wave+events",
                             "start": "k_dbn_step2<16,4>+start"}),
    "cor_v1": dict(base="cor_v1", rates=[R_LO, R_HI], seed=0x57E3, kernels={"both": "k_dbn_step2<16,4,w4,reg>[cor]"}),
    "cor_v2p1_like": dict(base="cor_v2p1_like", rates=[R_LO, R_HI], seed=0x57E4, kernels={"both": "k_dbn_step2<16,4,w8,reg>[cor]"}),
    "glider_v1": dict(base="glider_v1", rates=[R_LO, R_HI], seed=0x57E3,
                      kernels={"both": "k_dbn_step2<7,3,reg>[chain,w884]", "list+dense": "k_dbn_step2<7,3,reg>[chain]+events"}),
    "skydiving_v1": dict(base="skydiving_v1", rates=[R_LO, R_HI], seed=0x57EF, kernels={"both": "k_dbn_step2<7,3,reg>[2<-1,w484]"}),
    "fai5_v1": dict(base="fai5_v1", rates=[R_LO, R_HI], seed=0x57ED, kernels={"both": "k_dbn_step2<7,3,reg>[1<-0,2<-0,w848]"}),
    "uncor_1200code_v2p1": dict(base="uncor_1200code_v2p1", rates=[R_LO, R_HI], seed=0x57E2, per_step=True,
                                kernels={"both": "k_dbn_step2<7,3,reg>[per-step,w484]"}),
    # (each variable's only dynamic parent is its own bin, frozen, and four trajectories in five start in bin 5 of 9: that column is made a
    # below16, a shared, a one and a two column)
    "littoral_cor_v1": dict(base="littoral_cor_v1", rates=[R_LO, R_HI], seed=0x57F2, rotate=[1, 2, 4, 1], kernels={"both": "k_dbn_step2<16,4,w4,reg>[frozen]"}),
}
NAMES = list(MODELS)
_models, _plans, _samples = {}, {}, {}


def per_step(name):
    return bool(MODELS[name].get("per_step"))


def mode(name):
    return L.TRANSITION_PER_STEP if per_step(name) else L.TRANSITION_REFERENCE_AUTO


def tie_model(name, model_dir):
    """(native model, oracle parms dict, path) of a tie model, written once per session."""
    if name not in _models:
        path = os.path.join(str(model_dir), "step2_ties_%s.txt" % name)
        em_io.em_write(_tie_parms(MODELS[name]["base"], MODELS[name]["rates"], str(model_dir), MODELS[name].get("rotate")), path)
        _models[name] = (native.NativeModel.load_txt(path), O.parse_model_txt(path), path)
    return _models[name]


def indices_of(pp):
    labs = pp["labels_initial"]
    return dict(idx_L=label_index(labs, "L"), idx_v=label_index(labs, "v"), idx_dh=label_index(labs, "\\dot h"))


# ---- the plan of a model, from the debug hooks ------------------------------------------------------------------------------------
def s2_levels(new, nd):
    """s2_level of emgpu_kernels_step2.h for k < nd."""
    lev = []
    for k in range(nd):
        l = 0
        for q in range(k):
            if new >> (4 * k + q) & 1:
                l = max(l, lev[q] + 1)
        lev.append(l)
    return lev


def s2_pre(cur, new, nd):
    lev = s2_levels(new, 4)
    return [lev[k] == 0 and all(not (cur >> (4 * k + q) & 1) or lev[q] == 0 for q in range(4)) for k in range(nd)]


def plan_of(name, model_dir):
    """What the restatement needs of a model's plan: per dynamic variable k (plan order) its transition and initial variable (0-based),
    its row of the trace, the padded width, every column's packed words [q, 4] and padded words [q, width], its parents as (kind, index,
    stride) in asub2ind order; R per variable; the instance's masks, levels and prefetched variables."""
    if name in _plans:
        return _plans[name]
    nm, pp, _ = tie_model(name, model_dir)
    lib = L.lib()
    ni, nd = nm.n_initial, nm.n_dyn
    tm = np.asarray(pp["temporal_map"]).reshape(-1, 2) - 1
    G, r = np.asarray(pp["G_transition"]), np.asarray(pp["r_transition"])
    kernel = MODELS[name]["kernels"]["both"]
    cm, nw = C.c_uint32(), C.c_uint32()
    L.check(lib.emgpu_debug_parent_masks(nm._h, C.byref(cm), C.byref(nw)))
    frozen = "[frozen]" in kernel
    if "[" in kernel and not frozen:
        cur, new = cm.value, nw.value                     # an instance built for the model's own masks
    elif frozen:
        cur, new = cm.value, 0
    else:
        cur, new = ALL_MASKS[4 if "<16,4" in kernel else 3]
    assert nw.value & ~new == 0 and (frozen or cm.value & ~cur == 0)
    var = []
    for k in range(nd):
        tvar, rr, q, meff, mp = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_uint32()
        thr, cthr = np.zeros(64, dtype=np.uint32), np.zeros(7, dtype=np.uint32)
        L.check(lib.emgpu_debug_dynamic_column(nm._h, k, 0, C.byref(tvar), C.byref(rr), C.byref(q), thr.ctypes.data, C.byref(meff),
                                               cthr.ctypes.data, C.byref(mp)))
        tv = tvar.value - 1
        slot = int(np.flatnonzero(tm[:, 1] == tv)[0])
        width, words = C.c_int32(), np.zeros(8, dtype=np.uint32)
        PK, PAD = np.zeros((q.value, 4), dtype=np.uint32), None
        for col in range(q.value):
            L.check(lib.emgpu_debug_padded_column(nm._h, k, col, C.byref(width), words.ctypes.data))
            if PAD is None:
                PAD = np.zeros((q.value, width.value), dtype=np.uint32)
            PAD[col] = words[: width.value]
            L.check(lib.emgpu_debug_pk_column(nm._h, k, col, PK[col].ctypes.data))
        parents, stride = [], 1
        for u in np.flatnonzero(G[:, tv]):
            if u >= ni:
                parents.append(("new", int(np.flatnonzero(tm[:, 1] == u)[0]), stride))
            elif u in tm[:, 0]:
                parents.append(("cur", int(np.flatnonzero(tm[:, 0] == u)[0]), stride))
            else:
                parents.append(("static", int(u), stride))
            stride *= int(r[u])
        assert stride == q.value, (name, k, stride, q.value)
        R = int(lib.emgpu_debug_bernoulli_threshold(float(pp["resample_rates"][tm[slot, 0]])))
        var.append(dict(tvar=tv, ivar=int(tm[slot, 0]), slot=slot, width=width.value, meff=meff.value, PK=PK, PAD=PAD, parents=parents, R=R))
    lev = s2_levels(new, nd)
    slot_k = {v["slot"]: k for k, v in enumerate(var)}
    _plans[name] = dict(var=var, cur=cur, new=new, frozen=frozen, lev=lev, maxlev=max(lev), pre=s2_pre(cur, new, nd), slot_k=slot_k)
    return _plans[name]


# ---- the kernel's decision, mirrored ------------------------------------------------------------------------------------------------
def half(w, odd):
    """the halfword of a packed word a second reads: the high one on an odd second"""
    return np.where(odd, w >> 16, w & 0xFFFF)


def pk_fired2(odd, w, t01, t23, t45):
    """pk_fired2<ODD, 3>: the sum over the six T' of min(sat16(x_h - T'), 2) -- twice the thresholds that fired, odd on a tie."""
    x = half(w, odd)
    s = np.zeros_like(x)
    for t in (t01, t23, t45):
        s += np.clip(x - (t & 0xFFFF), 0, 2) + np.clip(x - (t >> 16), 0, 2)
    return s


def or_half(odd, s, w):
    """or_half with the zt words: a 1 where the half the second reads is 0 (v_pk_sub_u16 1 - x_h, clamped)."""
    return s | np.clip(1 - half(w, odd), 0, 1)


def plain_fired7(odd, w, h0, h1, h2):
    """plain_fired7: (the bin's bit offset in the map = 7 * fired, min over a_t as unsigned = 0 exactly on a tie)"""
    x = half(w, odd)
    a = [(h - x) & 0xFFFFFFFF for h in (h0, h1, h2)]
    return (a[0] >> 29) + (a[1] >> 29) + (a[2] >> 29), np.minimum(np.minimum(a[0], a[1]), a[2])


def clamp32(x):
    return np.minimum(x, 0xFFFFFFFE)


def full_draw(odd, wh, wl):
    """the 32-bit draw of a second from its word of the primary block and its word of the secondary (_LO) block"""
    return clamp32((half(wh, odd) << 16) | half(wl, odd))


def exact_borrows(x, thresholds):
    """exact_borrows: how many of the padded column's thresholds the draw is below (select_random.m:19-20)"""
    b = np.zeros_like(x)
    for t in thresholds:
        b += x < t
    return b


def exact_hit(x, R):
    return x < R


def block_words(section, a, gidx, attempt, G8, seed):
    """Words [n, G8, 4] of the blocks 0 .. G8 - 1 of (section, a): counter = (index, attempt, section << 28 | a << 20 | block)."""
    blk = np.arange(G8, dtype=np.uint64)[None, :]
    w = O.philox4x32_np((gidx & 0xFFFFFFFF)[:, None], (gidx >> 32)[:, None], attempt.astype(np.uint64)[:, None], (section << 28) | (a << 20) | blk,
                        seed & 0xFFFFFFFF, seed >> 32, O.philox_rounds())
    return np.stack(w, axis=2).astype(np.int64)


def per_second(words, T):
    """[n, T]: the word second c reads -- word (c & 7) >> 1 of block c >> 3"""
    return np.repeat(words.reshape(words.shape[0], -1), 2, axis=1)[:, :T]


# ---- the draws of a run by kind ----------------------------------------------------------------------------------------------------
KINDS = {   # kind: floor
    "packed real tie, fired": 10, "packed real tie, not fired": 10, "packed spurious tie": 10,
    "packed x_h == 0, column with H = 0": 10, "packed x_h == 0, column without": 10,
    "plain tie H > 0, fired": 10, "plain tie H > 0, not fired": 10, "plain x_h == 0 against H = 0": 10, "plain tie, column of 1 or 2 thresholds": 10,
    "packed tie, even second": 10, "packed tie, odd second": 10, "plain tie, even second": 10, "plain tie, odd second": 10,
    "tie on a new-value parent, redone bin not 1": 10, "tie on a variable of level 1 or 2": 10, "tie on a prefetch parent at j < 7": 10,
    "resample tie, hit": 10, "resample tie, no hit": 10, "tie at second 1 of block 0": 10,
    "wave-seconds with ties in two variables of one level": 3,
}
# A floor that no seed out of 32 (0x57E2 ...) met: the best count found, which that seed then has to keep
BEST_OF_32 = {"skydiving_v1": {"packed x_h == 0, column with H = 0": 9}}     # (one 8-word variable, a sixth of its columns: 63 / 6 expected)
PACKED = [k for k in KINDS if k.startswith("packed")]
PLAIN = [k for k in KINDS if k.startswith("plain")]


def not_applicable(name, model_dir):
    """{kind: reason} of the kinds a model's instance cannot have."""
    pl = plan_of(name, model_dir)
    out = {}
    if all(v["width"] == 4 for v in pl["var"]):
        out.update({k: "no 8-word variable" for k in PACKED})
    if all(v["width"] == 8 for v in pl["var"]):
        out.update({k: "no 4-word variable" for k in PLAIN})
    if pl["new"] == 0:
        out["tie on a new-value parent, redone bin not 1"] = "no new-value parent"
    if pl["maxlev"] == 0:
        out["tie on a variable of level 1 or 2"] = "one dependency level"
        out["tie on a prefetch parent at j < 7"] = "one dependency level: nothing is prefetched"
    elif not any(pl["pre"]):
        out["tie on a prefetch parent at j < 7"] = "the instance of every parent: no level-0 variable depends on level-0 current bins alone"
    lev = pl["lev"]
    th = [v["meff"] if v["width"] == 4 else 6 for v in pl["var"]]      # tie values per column: the plain form's high halves, the packed form's slots
    pairs = [(a, b) for a in range(len(lev)) for b in range(a) if lev[a] == lev[b]]
    expect = sum(th[a] * th[b] for a, b in pairs) * (64.0 / 65536) ** 2 * (N // 64) * (T - 1)     # (an upper bound)
    if not pairs:
        out["wave-seconds with ties in two variables of one level"] = "every variable on a level of its own"
    elif expect < 3:
        out["wave-seconds with ties in two variables of one level"] = "expectation below 3 (%d pairs: at most %.1f)" % (len(pairs), expect)
    return out


def draws_by_kind(nm, pp, ref, n, T, seed, first, plan, detail=False):
    """Counts of the draws of each kind in the oracle's sample `ref`, in the blocks that take the unguarded path (8 g8 + 7 < T), with
    the mirror's bin asserted equal to the oracle's at every such draw (which pins this restatement of the slot map, of the lanes'
    columns and of the rule): every draw goes through the high-halfword rule, the tied ones through the 32-bit redo as well.
    detail: also the [n, T] array "a transition or resample draw of this second ties"."""
    var = plan["var"]
    nd = len(var)
    gidx = np.uint64(first) + np.arange(n, dtype=np.uint64)
    attempt = ref["attempts"].astype(np.int64) - 1
    G8 = (T + 7) // 8
    B = ref["dense_bin"]
    init = ref["init_bin"].astype(np.int64)
    sec = np.arange(T)
    odd = (sec & 1).astype(bool)[None, :]
    live = ((sec >= 1) & (8 * (sec >> 3) + 7 < T))[None, :]      # draws of the unguarded path
    counts = {k: 0 for k in KINDS}
    any_tie = np.zeros((n, T), dtype=bool)
    level_ties = {}
    for k, v in enumerate(var):
        got = B[:, :, v["slot"]].astype(np.int64)
        assert np.array_equal(got[:, 0], init[:, v["ivar"]])
        col = np.zeros((n, T), dtype=np.int64)
        for kind, idx, stride in v["parents"]:
            if kind == "static":
                b = init[:, idx][:, None]
            elif kind == "new":
                b = B[:, :, idx]
            else:
                b = np.repeat(B[:, :1, idx], T, axis=1) if plan["frozen"] else np.concatenate([B[:, :1, idx], B[:, :-1, idx]], axis=1)
            col += stride * (b.astype(np.int64) - 1)
        wh = per_second(block_words(SEC_TRANS, v["tvar"], gidx, attempt, G8, seed), T)
        wl = per_second(block_words(SEC_TRANS + SEC_LO, v["tvar"], gidx, attempt, G8, seed), T)
        PK, PAD = v["PK"].astype(np.int64), v["PAD"].astype(np.int64)
        pk = [PK[:, w][col] for w in range(4)]                     # the lane's packed column, word by word [n, T]
        form = "plain" if v["width"] == 4 else "packed"
        if form == "plain":
            off, amin = plain_fired7(odd, wh, pk[0], pk[1], pk[2])
            tie = amin == 0
            decided = (pk[3] >> off) & 15
        else:
            sel = or_half(odd, pk_fired2(odd, wh, pk[0], pk[1], pk[2]), wh)
            tie = (sel & 1) != 0
            decided = (pk[3] >> (4 * (sel >> 1))) & 15
        ok = live & ~tie
        assert np.array_equal(decided[ok], got[ok]), ("a decided bin differs from the oracle's", k)
        tie &= live
        any_tie |= tie
        # ---- the tied draws alone from here on: the 32-bit redo, and what the draw tied with
        at = np.nonzero(tie)
        podd, pgot = np.broadcast_to(odd, tie.shape)[at], got[at]
        xh = half(wh[at], podd)
        x = full_draw(podd, wh[at], wl[at])
        pad = PAD[col[at]]                                         # [ties, width]
        if form == "plain":
            thresholds, table = [pad[:, t] for t in range(3)], pad[:, 3]
            H = [w[at] for w in pk[:3]]                           # (0x10000 past the variable's meff, 0xFFFF for "never")
            real = [(t > 0) & (t < 0xFFFFFFFF) for t in thresholds]
        else:
            thresholds, table = [pad[:, t] for t in range(6)], pad[:, 6] | (pad[:, 7] << 32)
            H = [t >> 16 for t in thresholds]
            real = [(t > 0) & (t < 0xFFFFFFFF) for t in thresholds]
        redone = (table >> (8 * exact_borrows(x, thresholds))) & 0xFF
        assert np.array_equal(redone, pgot), ("a redone bin differs from the oracle's", k)
        hit_h = [r_ & (h == xh) for h, r_ in zip(H, real)]
        tied_real = np.logical_or.reduce(hit_h)
        fired = np.logical_or.reduce([hh & (x >= t) for hh, t in zip(hit_h, thresholds)])
        unfired = np.logical_or.reduce([hh & (x < t) for hh, t in zip(hit_h, thresholds)])
        has_h0 = np.logical_or.reduce([r_ & (h == 0) for h, r_ in zip(H, real)])
        if form == "packed":
            counts["packed real tie, fired"] += int((tied_real & (xh > 0) & fired).sum())
            counts["packed real tie, not fired"] += int((tied_real & (xh > 0) & unfired).sum())
            counts["packed spurious tie"] += int((~tied_real & (xh > 0)).sum())
            counts["packed x_h == 0, column with H = 0"] += int(((xh == 0) & has_h0).sum())
            counts["packed x_h == 0, column without"] += int(((xh == 0) & ~has_h0).sum())
        else:
            counts["plain tie H > 0, fired"] += int(((xh > 0) & fired).sum())
            counts["plain tie H > 0, not fired"] += int(((xh > 0) & unfired).sum())
            counts["plain x_h == 0 against H = 0"] += int((xh == 0).sum())
            nreal = real[0].astype(np.int64) + (real[1] & (thresholds[1] != thresholds[0])) + (real[2] & (thresholds[2] != thresholds[1]))
            counts["plain tie, column of 1 or 2 thresholds"] += int(((nreal >= 1) & (nreal <= 2)).sum())
        counts[form + " tie, even second"] += int((~podd).sum())
        counts[form + " tie, odd second"] += int(podd.sum())
        if any(plan["new"] >> (4 * k2 + k) & 1 for k2 in range(nd)):
            counts["tie on a new-value parent, redone bin not 1"] += int((pgot != 1).sum())
        if plan["lev"][k] >= 1:
            counts["tie on a variable of level 1 or 2"] += len(pgot)
        if plan["maxlev"] >= 1 and any(plan["pre"][k2] and plan["cur"] >> (4 * k2 + k) & 1 for k2 in range(nd)):
            counts["tie on a prefetch parent at j < 7"] += int(((at[1] & 7) < 7).sum())
        counts["tie at second 1 of block 0"] += int((at[1] == 1).sum())
        level_ties.setdefault(plan["lev"][k], []).append(np.pad(tie, ((0, -n % 64), (0, 0))).reshape(-1, 64, T).any(axis=1))
        if v["R"]:
            rh = per_second(block_words(SEC_RES, v["ivar"], gidx, attempt, G8, seed), T)
            rtie = live & (half(rh, odd) == (v["R"] >> 16))
            at = np.nonzero(rtie)
            rl = per_second(block_words(SEC_RES + SEC_LO, v["ivar"], gidx, attempt, G8, seed), T)
            hit = exact_hit(full_draw(np.broadcast_to(odd, rtie.shape)[at], rh[at], rl[at]), v["R"])
            counts["resample tie, hit"] += int(hit.sum())
            counts["resample tie, no hit"] += int((~hit).sum())
            counts["tie at second 1 of block 0"] += int((at[1] == 1).sum())
            any_tie |= rtie
    for ties in level_ties.values():
        counts["wave-seconds with ties in two variables of one level"] += int((np.sum(ties, axis=0) >= 2).sum())
    return (counts, any_tie) if detail else counts


def counted_sample(name, model_dir):
    """(the oracle's sample of the counted run, its counts by kind, the first index of the first wave with a redo in block 0), made once
    per session.  Left unchanged by its users."""
    if name not in _samples:
        nm, pp, _ = tie_model(name, model_dir)
        seed = MODELS[name]["seed"]
        ref = O.uncor_sample(O.OracleModel(pp), N, T, seed, first_index=FIRST, want_events=False, per_step=per_step(name))
        counts, tie = draws_by_kind(nm, pp, ref, N, T, seed, FIRST, plan_of(name, model_dir), detail=True)
        waves = tie[:, 1:8].reshape(N // 64, 64, 7).any(axis=(1, 2))
        _samples[name] = (ref, counts, FIRST + 64 * int(np.flatnonzero(waves)[0]))
    return _samples[name]


def floor_of(name, kind):
    return BEST_OF_32.get(name, {}).get(kind, KINDS[kind])


def floors_missed(name, model_dir, counts):
    """The kinds of a model below their floor (not applicable ones left out)."""
    na = not_applicable(name, model_dir)
    return {k: (counts[k], floor_of(name, k)) for k in KINDS if k not in na and counts[k] < floor_of(name, k)}


def kinds_table(name, model_dir, counts):
    na = not_applicable(name, model_dir)
    return "\n".join("  %-55s %s" % (k, "n/a: " + na[k] if k in na else "%6d  (floor %d)" % (counts[k], floor_of(name, k))) for k in KINDS)
