"""The high-halfword compare of k_uncor_fast and the draws at which it hands a block to the exact pass (emgpu_kernels_fast.h,
load_cthr_pk / eight_seconds_pk): a tie with a threshold's high half, x_h == 0 on a lane whose column has a threshold below 2^16, and the
values that are no tie any more -- x_h == H + 1 of a padding copy, x_h == 0 on a lane without such a threshold.

CPU: a Python mirror of the rule over every transition column of every shipped fast-branch model and of the test models below, every
x_h in 0 .. 65535: what the rule calls decided is select_random's bin for every low halfword, and every real tie is reported.
-m gpu: small hand-made models with the columns where the rule can go wrong, bit for bit against the oracle (bins, f32 values, attempts)
through k_uncor_fast, k_uncor_fast_mixed and k_uncor_fast_idx, and one tie-dense run whose sample is counted first: every kind of
draw above occurs at least 10 times in it."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import oracle as O
from em_model_manned_bayes_amd import em_io, native, _lib as L
from util import assert_uncor_parity, shaped_model, uncor_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST_SHAPES = [(7, 2, 2, 2), (7, 2, 4, 2), (7, 2, 4, 4), (7, 4, 2, 4), (7, 4, 6, 4), (7, 4, 6, 6), (7, 6, 6, 6), (9, 6, 6, 6)]   # kFastShapes
SEED = 0x71E5
FIRST = 2**33 + 11
X = np.arange(65536, dtype=np.int64)      # every high halfword


# ---- the rule, mirrored ---------------------------------------------------------------------------------------------------------
def pk_column(cthr, meff, M):
    """load_cthr_pk: (T' of the M compare slots, the lane treats x_h == 0 as a tie) of one compacted column."""
    tq, prev, xprev, z = [], 0, None, False
    for t in range(M):
        v = 0xFFFF
        if t < meff:
            x = int(cthr[t])
            if x != 0xFFFFFFFF and not (t > 0 and x == xprev):     # a real threshold: neither "never" nor a padding copy
                h = x >> 16
                v = h - 1 if h else 0
                z = z or h == 0
                if t > 0 and v <= prev:
                    v = prev + 1
                v = min(v, 0xFFFF)
            xprev = x
        tq.append(v)
        prev = v
    return tq, z


def pk_decide(tq, z, nibble_map, meff, x=X):
    """eight_seconds_pk at the high halfwords x: (tie reported, 1-based bin where decided)."""
    s = np.zeros(len(x), dtype=np.int64)
    for T in tq:
        s += np.clip(x - T, 0, 2)
    tie = ((s & 1) != 0) | ((x == 0) if z else False)
    n = np.minimum(s >> 1, meff)
    bins = (int(nibble_map) >> (4 * n)) & 15
    return tie, bins


def true_bins(row, x=X):
    """select_random's 1-based bin, 1 + #{t : x' >= X_t} on the column's full threshold row, of the draws x_h << 16 | 0 and
    x_h << 16 | 0xFFFF (clamped like uniform32) for the high halfwords x: the bin is monotone in the draw, so where the two agree every
    low halfword gives that bin."""
    lo_draw = x << 16
    hi_draw = np.minimum(lo_draw | 0xFFFF, 0xFFFFFFFE)
    lo = np.ones(len(x), dtype=np.int64)
    hi = np.ones(len(x), dtype=np.int64)
    for xt in row:
        lo += lo_draw >= int(xt)
        hi += hi_draw >= int(xt)
    return lo, hi


def breakpoints(tq, row):
    """Every x_h at which the rule's answer or select_random's can change: both are constant between two neighbouring ones, so a
    column that is right at these is right at every x_h in 0 .. 65535 (checked against the full range on FULL_RANGE columns of every
    model and on all columns of the test models)."""
    c = {0, 1, 2, 65535}
    for T in tq:
        c.update((T, T + 1, T + 2, T + 3))
    for xt in row:
        h = int(xt) >> 16
        c.update((h - 1, h, h + 1, h + 2))
    return np.array(sorted(v for v in c if 0 <= v <= 65535), dtype=np.int64)


FULL_RANGE = 150


def columns_of(nm):
    """(k, meff, full threshold row, compacted column, nibble map) of every transition column of every dynamic variable."""
    lib = L.lib()
    for k in range(nm.n_dyn):
        tvar, r, q, meff, mp = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_uint32()
        thr, cthr = np.zeros(64, dtype=np.uint32), np.zeros(7, dtype=np.uint32)
        col, ncol = 0, 1
        while col < ncol:
            L.check(lib.emgpu_debug_dynamic_column(nm._h, k, col, C.byref(tvar), C.byref(r), C.byref(q), thr.ctypes.data, C.byref(meff),
                                                   cthr.ctypes.data, C.byref(mp)))
            assert r.value - 1 <= 15
            ncol = q.value
            yield k, meff.value, thr[: r.value - 1].copy(), cthr[: meff.value].copy(), mp.value
            col += 1


def instance_of(nm):
    meffs = [m for _, m, _, _, _ in (next(c for c in columns_of(nm) if c[0] == k) for k in range(nm.n_dyn))]
    for s in FAST_SHAPES:
        if nm.n_initial <= s[0] and all(meffs[k] <= s[1 + k] for k in range(3)):
            return s
    return None


def is_fast_branch(nm):
    if nm.n_dyn != 3:
        return False
    cm, nw = C.c_uint32(), C.c_uint32()
    L.check(L.lib().emgpu_debug_parent_masks(nm._h, C.byref(cm), C.byref(nw)))
    return nw.value == 0 and instance_of(nm) is not None


def check_rule_on(nm, seen, stats, full_range=FULL_RANGE):
    shape = instance_of(nm)
    full = 0
    for k, meff, row, cthr, nibbles in columns_of(nm):
        M = shape[1 + k]
        key = (M, meff, row.tobytes(), nibbles)
        if key in seen:
            continue
        seen.add(key)
        assert (nibbles >> (4 * len(set(int(x) for x in cthr if x != 0xFFFFFFFF)))) & 15 == (nibbles >> (4 * meff)) & 15   # nibble d holds the last bin
        tq, z = pk_column(cthr, meff, M)
        at = breakpoints(tq, row)
        for x in ((at, X) if full < full_range else (at,)):
            tie, bins = pk_decide(tq, z, nibbles, meff, x)
            lo, hi = true_bins(row, x)
            real = lo != hi
            assert not np.any(real & ~tie), ("a real tie is not reported", k, [hex(int(v)) for v in row], x[real & ~tie][:4])
            dec = ~tie
            assert np.array_equal(bins[dec], lo[dec]), ("a decided bin differs", k, [hex(int(v)) for v in row], x[dec & (bins != lo)][:4])
            if x is X:   # nothing changes anywhere but at a breakpoint
                full += 1
                for f in (tie, bins, lo, hi):
                    assert np.all(np.isin(np.flatnonzero(f[1:] != f[:-1]) + 1, at)), (k, [hex(int(v)) for v in row])
        stats["columns"] += 1
        old = set([0] + [T + 1 for T in old_tq(cthr, meff, M) if T < 0xFFFF])   # the rule before: every slot t < meff in the chain, x_h == 0 a tie on every lane
        stats["old"] += len(old)
        stats["ties"] += int(tie.sum()) if x is X else len(set(T + 1 for T in tq if T < 0xFFFF) | ({0} if z else set()))
        stats["real"] += len(set(int(v) >> 16 for v in row if int(v) & 0xFFFF and int(v) != 0xFFFFFFFF))


def old_tq(cthr, meff, M):
    tq, prev = [], 0
    for t in range(M):
        v = 0xFFFF
        if t < meff:
            h = int(cthr[t]) >> 16
            v = h - 1 if h else 0
            if t > 0 and v <= prev:
                v = prev + 1
            v = min(v, 0xFFFF)
        tq.append(v)
        prev = v
    return tq


# ---- the test models ------------------------------------------------------------------------------------------------------------
BIG = 3_000_000   # a count beside which a count of 1 - 40 is a probability below 2^-16


def _tie_model(rates):
    """A <7,2,4,2> model (util.shaped_model) whose transition tables are edited by hand, column by column in rotation:
      variable 0 (meff 2): a real threshold below 2^16 (a) | two ordinary ones | one real threshold and its padding copy (c)
      variable 1 (meff 4): two real thresholds sharing a high half (b) | two real ones + two copies, the copies' H + 1 being ... (c)
                           | ... the high half of a real threshold of the NEXT kind of column (lanes of one wave mix the kinds)
                           | a threshold below 2^16 and three ordinary ones
      variable 2 (meff 2): columns without any real threshold ("never" + copy) | ordinary."""
    p = shaped_model(np.random.RandomState(4242), 7, (2, 4, 2), rates=rates, r=[4, 6, 3, 3, 3, 2, 2])
    ni = 7
    N0, N1, N2 = (p["N_transition"][ni + k] for k in range(3))
    for j in range(N0.shape[1]):
        kind = j % 3
        if kind == 0:
            N0[:, j] = [7, BIG, 0, 2 * BIG]              # X_0 = 7 / 3 BIG * 2^32 ~ 3341 < 2^16
        elif kind == 2:
            N0[:, j] = [0, BIG, 0, 3 * BIG]              # one real threshold: the second slot is its copy
    for j in range(N1.shape[1]):
        kind = j % 4
        if kind == 0:
            N1[:, j] = [BIG, 5, 0, BIG, 0, BIG]          # X_0 and X_1 five counts apart: the same high half
        elif kind == 1:
            N1[:, j] = [0x30000, 0, 0x10000, 0, 0, 0xC0000]   # total 2^20: thresholds 0x30000000 and 0x40000000, two copies (H + 1 = 0x4001)
        elif kind == 2:
            N1[:, j] = [0x30000, 0x10010, 0x20000, 0, 0x10000, 0x8FFF0]  # total 2^20: 0x3000.., 0x4001.. (the copies' old tie value), 0x6001.., 0x7001..
        else:
            N1[:, j] = [3, BIG, BIG, BIG, 0, BIG]        # X_0 < 2^16
    for j in range(N2.shape[1]):
        if j % 2 == 0:
            N2[:, j] = [0, 0, 1234]                      # bin 3 always: no real threshold
    return p


MODELS = {
    "ties": lambda: _tie_model([0.07, 2.0 ** -16 - 2.0 ** -20, 1.0 - 2.0 ** -16 - 2.0 ** -20, 0, 0, 0, 0]),   # (d): a rate below 2^-16, one just under 1 - 2^-16
    "ties2": lambda: _tie_model([2.0 ** -18, 0.11, 0.05, 0, 0, 0, 0]),
}
_models = {}


def tie_model(name, model_dir):
    if name not in _models:
        path = os.path.join(str(model_dir), "fast_ties_%s.txt" % name)
        em_io.em_write(MODELS[name](), path)
        _models[name] = (native.NativeModel.load_txt(path), O.parse_model_txt(path), path)
    return _models[name]


def test_the_test_models_have_the_columns_they_are_made_for(model_dir):
    nm, pp, _ = tie_model("ties", model_dir)
    assert instance_of(nm) == (7, 2, 4, 2) and is_fast_branch(nm)
    kinds = {"below16": [0, 0, 0], "shared": [0, 0, 0], "copies": [0, 0, 0], "copy_h1_real": 0, "none": [0, 0, 0], "plain": [0, 0, 0]}
    real_h = set()
    cols = list(columns_of(nm))
    for k, meff, row, cthr, nib in cols:
        real = sorted(set(int(x) for x in cthr if x != 0xFFFFFFFF))
        real_h |= {x >> 16 for x in real}
    for k, meff, row, cthr, nib in cols:
        real = sorted(set(int(x) for x in cthr if x != 0xFFFFFFFF))
        hs = [x >> 16 for x in real]
        kinds["below16"][k] += bool(real) and hs[0] == 0
        kinds["shared"][k] += len(set(hs)) < len(hs)
        kinds["copies"][k] += 0 < len(real) < meff
        kinds["none"][k] += not real
        kinds["plain"][k] += len(real) == meff and len(set(hs)) == len(hs) and hs[0] > 0
        if 0 < len(real) < meff and (hs[-1] + 1) in real_h:
            kinds["copy_h1_real"] += 1
    assert kinds["below16"][0] and kinds["below16"][1] and kinds["plain"][0] and kinds["plain"][1]          # (a): beside columns without one
    assert kinds["shared"][1] and kinds["copies"][0] and kinds["copies"][1] and kinds["copy_h1_real"] and kinds["none"][2]   # (b), (c)
    R = [L.lib().emgpu_debug_bernoulli_threshold(float(x)) for x in pp["resample_rates"][:3]]
    assert 0 < R[1] < 0x10000 and 0xFFFE0000 <= R[2] < 0xFFFF0000                                            # (d)


def test_rule_decides_like_select_random_and_reports_every_tie(model_dir):
    """Every distinct transition column of the test models and of the 13 shipped fast-branch models (62 535 of them).  The test models'
    columns and the first FULL_RANGE distinct columns of every shipped model are checked at each x_h in 0 .. 65535, and there also
    that neither the rule nor select_random changes anywhere but at a breakpoint; the remaining columns at their breakpoints, which
    by that constancy is the same statement for every x_h (the full range on all of them takes two minutes)."""
    seen, stats = set(), dict(columns=0, ties=0, real=0, old=0)
    for name in MODELS:
        check_rule_on(tie_model(name, model_dir)[0], seen, stats, full_range=10**9)
    shipped = 0
    for f in sorted(glob.glob(os.path.join(ROOT, "models", "*.npz"))):
        name = os.path.basename(f)[:-4]
        if name.startswith("terminal"):
            continue
        nm = native.NativeModel.load_txt(em_io.materialize_model(name, str(model_dir)))
        if is_fast_branch(nm):
            shipped += 1
            check_rule_on(nm, seen, stats)
    assert shipped >= 13
    print("columns (distinct) %d: tie values per column %.2f (real %.2f; the rule before: %.2f)"
          % (stats["columns"], stats["ties"] / stats["columns"], stats["real"] / stats["columns"], stats["old"] / stats["columns"]))
    assert stats["ties"] <= stats["old"]


# ---- the draws of a run, restated from the slot map -------------------------------------------------------------------------------
SEC_TRANS, SEC_RES = 3, 4      # emgpu_plan.h: the sections whose words carry the primary (high) halfwords of the 8 seconds of a block


def high_halfwords(section, a, gidx, T, seed):
    """x_h of seconds 0 .. T-1 (second 0 is never used) of every trajectory: block c >> 3, word (c & 7) >> 1, its low half for an
    even second and its high half for an odd one; counter = (index, attempt 0, section << 28 | a << 20 | block)."""
    G8 = (T + 7) // 8
    blk = np.arange(G8, dtype=np.uint64)[None, :]
    w = O.philox4x32_np((gidx & 0xFFFFFFFF)[:, None], (gidx >> 32)[:, None], 0, (section << 28) | (a << 20) | blk, seed & 0xFFFFFFFF, seed >> 32,
                        O.philox_rounds())
    w = np.stack(w, axis=2).astype(np.int64)                             # (n, G8, 4)
    x = np.stack([w & 0xFFFF, w >> 16], axis=3).reshape(len(gidx), G8 * 8)
    return x[:, :T]


def draws_by_kind(nm, pp, ref, n, T, seed, first):
    """Counts of the draws of each kind in the oracle's sample `ref`, with the rule's decided bins checked against the oracle's
    trace on the way (which pins this restatement of the slot map and of the lanes' columns)."""
    ni, shape = nm.n_initial, instance_of(nm)
    gidx = first + np.arange(n, dtype=np.uint64)
    cols = {k: [] for k in range(3)}
    for k, meff, row, cthr, nib in columns_of(nm):
        cols[k].append((meff, row, cthr, nib))
    G, r = np.asarray(pp["G_transition"]), np.asarray(pp["r_transition"])
    counts = dict(transition_tie=0, resample_tie=0, zero_needed=0, zero_not_needed=0, copy_h_plus_1=0)
    for k in range(3):
        M = shape[1 + k]
        col, stride = np.zeros(n, dtype=np.int64), 1
        for u in range(ni + 3):
            if G[u, ni + k]:
                assert u < ni                                            # fast branch: parents frozen at the initial state
                col += stride * (ref["init_bin"][:, u].astype(np.int64) - 1)
                stride *= int(r[u])
        q = len(cols[k])
        TQ, Z, NIB, OLD = np.zeros((q, M), np.int64), np.zeros(q, bool), np.zeros(q, np.int64), np.full((q, M), -1, np.int64)
        for j, (meff, row, cthr, nib) in enumerate(cols[k]):
            tq, z = pk_column(cthr, meff, M)
            TQ[j], Z[j], NIB[j] = tq, z, nib
            for t, To in enumerate(old_tq(cthr, meff, M)):
                if tq[t] == 0xFFFF and To < 0xFFFF and t < meff and int(cthr[t]) != 0xFFFFFFFF:
                    OLD[j, t] = To + 1                                    # the tie value a padding copy had
        meff = cols[k][0][0]
        x = high_halfwords(SEC_TRANS, ni + k, gidx, T, seed)[:, 1:]      # (n, T - 1): seconds 1 ..
        s = np.zeros_like(x)
        for t in range(M):
            s += np.clip(x - TQ[col, t][:, None], 0, 2)
        chain = (s & 1) != 0
        zero = x == 0
        need = Z[col][:, None]
        tie = chain | (zero & need)
        bins = (NIB[col][:, None] >> (4 * np.minimum(s >> 1, meff))) & 15
        got = ref["dense_bin"][:, 1:T, k].astype(np.int64)
        assert np.array_equal(bins[~tie], got[~tie]), k
        copy = np.zeros_like(chain)
        for t in range(M):
            copy |= x == OLD[col, t][:, None]
        counts["transition_tie"] += int(chain.sum())
        counts["zero_needed"] += int((zero & need).sum())
        counts["zero_not_needed"] += int((zero & ~need).sum())
        counts["copy_h_plus_1"] += int((copy & ~tie).sum())
        R = int(L.lib().emgpu_debug_bernoulli_threshold(float(pp["resample_rates"][k])))
        if R:
            counts["resample_tie"] += int((high_halfwords(SEC_RES, k, gidx, T, seed)[:, 1:] == (R >> 16)).sum())
    return counts


DENSE_N, DENSE_T = 65536, 64
_dense = {}


def dense_sample(model_dir):
    """The tie-dense run's oracle sample and its counts, made once."""
    if not _dense:
        nm, pp, _ = tie_model("ties", model_dir)
        ref = O.uncor_sample(O.OracleModel(pp), DENSE_N, DENSE_T, SEED, first_index=FIRST, want_events=False)
        _dense["ref"] = ref
        _dense["counts"] = draws_by_kind(nm, pp, ref, DENSE_N, DENSE_T, SEED, FIRST)
    return _dense["ref"], _dense["counts"]


def test_tie_dense_sample_holds_every_kind_of_draw(model_dir):
    """A condition on the inputs of the tie-dense GPU run (SEED was picked for it on the CPU)."""
    _, counts = dense_sample(model_dir)
    print(counts)
    assert all(v >= 10 for v in counts.values()), counts


# ---- -m gpu ---------------------------------------------------------------------------------------------------------------------
def _dense_parity(got, ref, T):
    assert np.array_equal(got["init_bin"].astype(np.int32), ref["init_bin"]) and np.array_equal(got["attempts"], ref["attempts"])
    assert np.array_equal(got["init_val"], ref["init_val"].astype(np.float32))
    assert np.array_equal(got["dyn_bin"], ref["dense_bin"]), "dense bins differ"
    assert np.array_equal(got["dyn_val"], ref["dense_val"].astype(np.float32)), "dense values differ"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("n,T", [(64 * 5 + 37, 17), (64 * 9 + 37, 64)])
def test_small_shapes_match_oracle(name, n, T, gpu_ctx, model_dir):
    """A partial last wave; T = 17: the first block, one interior block and an edge block."""
    nm, pp, _ = tie_model(name, model_dir)
    ref = O.uncor_sample(O.OracleModel(pp), n, T, SEED, first_index=FIRST, want_events=False)
    got = native.sample_dbn_host(gpu_ctx, nm, n, T, SEED, first_index=FIRST, want_dense=True, want_events=False, **uncor_indices(pp))
    assert got["kernel"] == "k_uncor_fast<7,2,4,2>"
    _dense_parity(got, ref, T)


@pytest.mark.gpu
def test_index_list_matches_oracle(gpu_ctx, model_dir):
    nm, pp, _ = tie_model("ties", model_dir)
    n, T = 64 * 7 + 37, 17
    ref = O.uncor_sample(O.OracleModel(pp), n, T, SEED, first_index=FIRST, want_events=False)
    perm = np.random.RandomState(7).permutation(n)
    got = native.sample_dbn_host(gpu_ctx, nm, n, T, SEED, want_dense=True, want_events=False, indices=(FIRST + perm).astype(np.uint64), **uncor_indices(pp))
    assert got["kernel"] == "k_uncor_fast_idx<7,2,4,2>"
    _dense_parity(got, {k: ref[k][perm] for k in ("init_bin", "init_val", "attempts", "dense_bin", "dense_val")}, T)


@pytest.mark.gpu
def test_mixed_launch_matches_oracle(gpu_ctx, model_dir):
    """Both test models in one launch, blocks at odd offsets: a workgroup at a model boundary exists twice."""
    import torch
    pairs = [tie_model(m, model_dir) for m in ("ties", "ties2")]
    T = 17
    ni, nd, G4 = 7, 3, (T + 3) // 4
    blocks = [(0, FIRST + 3, 64 * 4 + 37), (1, FIRST + 296, 257), (0, FIRST + 553, 219)]
    lo, n_total = 3, 769
    ld = lo + n_total + 5
    dev = torch.device("cuda", 0)
    ib = torch.zeros((ni, ld), dtype=torch.uint8, device=dev)
    iv = torch.zeros((ni, ld), dtype=torch.float32, device=dev)
    db = torch.zeros((G4, nd, ld), dtype=torch.int32, device=dev)
    dv = torch.zeros((G4, nd, ld, 4), dtype=torch.float32, device=dev)
    at = torch.zeros((ld,), dtype=torch.int32, device=dev)
    p, _keep = native.make_params(n_total, T, SEED, first_index=FIRST + lo, **uncor_indices(pairs[0][1]))
    native.sample_dbn_blocks_device(gpu_ctx, [pr[0] for pr in pairs], p, blocks, init_bin=ib.data_ptr(), init_val=iv.data_ptr(),
                                    dyn_bin=db.data_ptr(), dyn_val=dv.data_ptr(), attempts=at.data_ptr(), ld=ld, col_offset=lo)
    gpu_ctx.sync()
    assert gpu_ctx.last_kernel() == "k_uncor_fast_mixed<7,2,4,2>"
    gb = native.unpack_dyn_bin(db.cpu().numpy().view(np.uint32), T)
    gv = native.unpack_dyn_val(dv.cpu().numpy(), T)
    for m, first, cnt in blocks:
        c = first - FIRST
        ref = O.uncor_sample(O.OracleModel(pairs[m][1]), cnt, T, SEED, first_index=first, want_events=False)
        got = dict(init_bin=ib.cpu().numpy().T[c: c + cnt], init_val=iv.cpu().numpy().T[c: c + cnt], attempts=at.cpu().numpy()[c: c + cnt],
                   dyn_bin=gb[c: c + cnt], dyn_val=gv[c: c + cnt])
        _dense_parity(got, ref, T)


@pytest.mark.gpu
def test_tie_dense_run_matches_oracle(gpu_ctx, model_dir):
    """65 536 trajectories x 64 s on the model with copies: every kind of draw (counted above) at least 10 times."""
    nm, pp, _ = tie_model("ties", model_dir)
    ref, counts = dense_sample(model_dir)
    assert all(v >= 10 for v in counts.values()), counts
    got = native.sample_dbn_host(gpu_ctx, nm, DENSE_N, DENSE_T, SEED, first_index=FIRST, want_dense=True, want_events=False, **uncor_indices(pp))
    assert got["kernel"] == "k_uncor_fast<7,2,4,2>"
    _dense_parity(got, ref, DENSE_T)
