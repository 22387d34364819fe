"""The exact recount of k_uncor_fast's tie redo (emgpu_kernels_fast.h, eight_seconds_recount_pk / pk_gt32) and the single tie word of
the high-halfword pass, mirrored in Python on the inputs the kernel keeps: the T' registers, the low halves and the 3-bit codes of the
lane's LDS row, the nibble map.  No GPU.

The mirror does the kernel's arithmetic -- saturating 16-bit differences, no carry -- on the draw AS DRAWN (not clamped); the reference
is select_random on the full thresholds with the draw clamped like uniform32.  That the two agree at the draw 0xFFFFFFFF is the proof
that, with "never" excluded, the clamp cannot change a compare.

Mutants of `recount_not_fired` that the tests themselves run and require to fail (MUTANTS): `>=` turned into `>` on the low half; a code
of 7 counted like a threshold; the shift of a shifted threshold ignored."""
import glob
import os

import numpy as np

import oracle as O
from em_model_manned_bayes_amd import em_io, native, _lib as L
from test_gpu_fast_ties import MODELS, columns_of, instance_of, is_fast_branch, pk_column, tie_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = 0xFFFFFFFF
MUTANTS = ("low_gt", "count_code7", "ignore_shift")     # recount_not_fired(mutant=...): every one must fail the tests below


# ---- load_cthr_pk: what the lane keeps ---------------------------------------------------------------------------------------------
def pk_column_full(cthr, meff, M):
    """(T', low halves, codes) of the M compare slots of one compacted column: code 7 = "never" or a padding copy, else T' + 1 - H."""
    tq, low, code, prev, xprev = [], [], [], 0, None
    for t in range(M):
        v, c, lo = 0xFFFF, 7, 0xFFFF
        if t < meff:
            x = int(cthr[t])
            if x != NEVER and not (t > 0 and x == xprev):
                h = x >> 16
                v = h - 1 if h else 0
                if t > 0 and v <= prev:
                    v = prev + 1
                v = min(v, 0xFFFF)
                c, lo = v + 1 - h, x & 0xFFFF
            xprev = x
        tq.append(v)
        low.append(lo)
        code.append(c)
        prev = v
    return tq, low, code


# ---- pk_gt32 and the recount, in the kernel's arithmetic -----------------------------------------------------------------------------
def sat(a, b):
    """v_pk_sub_u16 ... clamp, one half."""
    return np.maximum(a - b, 0)


def gt32(ah, al, xh, xl, always=0, low_gt=False):
    """pk_gt32: 1 where (A_h, A_l) > (x_h, x_l).  All operands 16-bit, as int64 arrays."""
    g, b = sat(xh, ah), sat(ah, xh)
    c = sat(al + 1, xl) if low_gt else sat(al, xl)          # (mutant: not fired at x_l == L as well)
    k = np.minimum(b | c | always, 1)
    return sat(k, g)


def recount_not_fired(TQ, LOW, CODE, xh, xl, mutant=None):
    """#{slots not fired} of eight_seconds_recount_pk.  TQ, LOW, CODE: (..., M) arrays broadcast against the draws xh, xl (...)."""
    M = TQ.shape[-1]
    nf = np.zeros(np.broadcast(TQ[..., 0], xh).shape, dtype=np.int64)
    for t in range(M):
        code = CODE[..., t]
        never = (code + 1) >> 3
        if mutant == "ignore_shift" and t > 0:
            code = np.where(never == 1, code, 0)
        hp = ((TQ[..., t] + 1 - code) & 0xFFFF) | (never * 0xFFFF)
        assert mutant or np.all((TQ[..., t] + 1 - code >= 0) & (TQ[..., t] + 1 - code <= 0xFFFF))     # stays within its halfword
        if mutant == "count_code7":
            never = never * 0
        nf += gt32(hp, LOW[..., t], xh, xl, never, low_gt=(mutant == "low_gt"))
    return nf


def recount_bins(TQ, LOW, CODE, NIB, meff, xh, xl, mutant=None):
    n = TQ.shape[-1] - recount_not_fired(TQ, LOW, CODE, xh, xl, mutant)
    return (NIB >> (4 * np.minimum(n, meff))) & 15       # (the byte table of load_cthr_pk: entry n is nibble min(n, meff))


def draws_around(H, Lo):
    """x_h in {H - 1, H, H + 1, 0, 1, 0xFFFF} x x_l in {0, L - 1, L, L + 1, 0xFFFE, 0xFFFF} for arrays H, Lo (...): (..., 36) each;
    a value outside 0 .. 0xFFFF is replaced by the threshold's own half."""
    xh = np.stack([H - 1, H, H + 1, H * 0, H * 0 + 1, H * 0 + 0xFFFF], axis=-1)
    xl = np.stack([Lo * 0, Lo - 1, Lo, Lo + 1, Lo * 0 + 0xFFFE, Lo * 0 + 0xFFFF], axis=-1)
    xh = np.where((xh < 0) | (xh > 0xFFFF), H[..., None], xh)
    xl = np.where((xl < 0) | (xl > 0xFFFF), Lo[..., None], xl)
    return np.repeat(xh, 6, axis=-1), np.tile(xl, 6)


def check_columns(cols, M, meff, mutant=None):
    """cols: [(full threshold row, compacted column, nibble map)] of one variable.  Every real threshold of every column, 36 draws each."""
    q = len(cols)
    TQ, LOW, CODE = (np.zeros((q, M), np.int64) for _ in range(3))
    NIB = np.zeros(q, np.int64)
    r1 = max(len(row) for row, _, _ in cols)
    ROW = np.full((q, r1), NEVER + 1, np.int64)            # beyond the row: above every clamped draw
    for j, (row, cthr, nib) in enumerate(cols):
        TQ[j], LOW[j], CODE[j] = pk_column_full(cthr, meff, M)
        assert TQ[j].tolist() == pk_column(cthr, meff, M)[0]
        NIB[j] = nib
        ROW[j, : len(row)] = row
        real = sorted(set(int(x) for x in cthr if int(x) != NEVER))
        assert all(x <= 0xFFFFFFFE for x in real)          # so 0xFFFFFFFF >= X <=> 0xFFFFFFFE >= X: the clamp changes no compare with a real one
        kept = [((TQ[j, t] + 1 - CODE[j, t]) << 16) | LOW[j, t] for t in range(M) if CODE[j, t] != 7]
        assert kept == real, ("the lane's words do not give the column's real thresholds back", cthr, kept)
    bad = 0
    for t in range(M):
        on = CODE[:, t] != 7
        if not on.any():
            continue
        H, Lo = TQ[on, t] + 1 - CODE[on, t], LOW[on, t]
        xh, xl = draws_around(H, Lo)                       # (columns, 36)
        got = recount_bins(TQ[on][:, None, :], LOW[on][:, None, :], CODE[on][:, None, :], NIB[on][:, None], meff, xh, xl, mutant)
        x = np.minimum((xh << 16) | xl, 0xFFFFFFFE)        # the draw clamped, select_random.m:17-20 on the full row
        want = 1 + (x[:, :, None] >= ROW[on][:, None, :]).sum(axis=2)
        bad += int((got != want).sum())
        if mutant is None:
            assert bad == 0, ("recount differs from select_random", t, np.argwhere(got != want)[:3])
    return bad


def shipped_fast_branch_models(model_dir):
    for f in sorted(glob.glob(os.path.join(ROOT, "models", "*.npz"))):
        name = os.path.basename(f)[:-4]
        if name.startswith("terminal"):
            continue
        path = em_io.materialize_model(name, str(model_dir))
        nm = native.NativeModel.load_txt(path)
        if is_fast_branch(nm):
            yield name, nm, path


_cols = {}


def all_columns(model_dir):
    """{(M, meff): [(row, cthr, nibbles)]} over the distinct transition columns of the test models and the shipped fast-branch models."""
    if not _cols:
        seen, shipped = set(), 0
        models = [tie_model(n, model_dir)[0] for n in sorted(MODELS)]
        for _, nm, _ in shipped_fast_branch_models(model_dir):
            models.append(nm)
            shipped += 1
        assert shipped >= 13
        for nm in models:
            shape = instance_of(nm)
            for k, meff, row, cthr, nib in columns_of(nm):
                key = (shape[1 + k], meff, row.tobytes(), nib)
                if key not in seen:
                    seen.add(key)
                    _cols.setdefault((shape[1 + k], meff), []).append((row, cthr, nib))
    return _cols


def test_recount_is_select_random_on_every_shipped_column(model_dir):
    cols = all_columns(model_dir)
    n = sum(len(v) for v in cols.values())
    print("distinct columns:", n)
    assert n >= 62535
    for (M, meff), c in sorted(cols.items()):
        check_columns(c, M, meff)
    # (a code of 7 counted shows on the hand-made columns only: in a shipped column nibble d + 1 of the map repeats nibble d)
    for m in ("low_gt", "ignore_shift"):
        assert sum(check_columns(c, M, meff, mutant=m) for (M, meff), c in cols.items()) > 0, "the mutant %s passes" % m


# ---- hand-made columns: every code the kernel meets ---------------------------------------------------------------------------------
HAND = [   # (compacted column, what it is there for)
    ([0x00001234, 0x50000000], "H = 0"),
    ([0x00000010, 0x00002000], "two thresholds with H = 0: code 1 and a shift of 2"),
    ([0x00000000, 0x30000000], "a threshold of 0: fired by every draw"),
    ([0x30000005, 0x3000FFF0], "two thresholds sharing a high half"),
    ([0x40000001, 0x40000002, 0x4000FFFF, 0x40010000], "three sharing a high half, the fourth pushed on by them"),
    ([0x40000001, 0x40000002, 0x40000003, 0x40000004], "four sharing a high half: shifts of 1, 2 and 3"),
    ([0x30000000, 0x40000000, 0x40000000, 0x40000000], "padding copies"),
    ([0x30008000, 0x30008000], "a copy whose T' would be a shift"),
    ([0x12345678, 0xFFFFFFFF], "never"),
    ([0xFFFFFFFF, 0xFFFFFFFF], "no real threshold"),
    ([0xFFFF0000, 0xFFFFFFFE], "0xFFFFFFFE, shifted onto T' = 0xFFFF"),
    ([0xFFFFFFFE, 0xFFFFFFFF], "0xFFFFFFFE beside never"),
    ([0x0000FFFF, 0x00010000, 0xFFFEFFFF, 0xFFFF0000], "low halves 0xFFFF and 0 on either side of a high half"),
]


def hand_columns():
    for cthr, what in HAND:
        meff = len(cthr)
        d = len(set(cthr))                                              # distinct entries: the map of a padded column repeats its last bin from nibble d on
        nib = sum((min(n, d) + 1) << (4 * n) for n in range(meff + 1))  # bin n + 1 after n of them: every count shows
        yield np.array(cthr, dtype=np.int64), meff, nib, what


def check_hand(mutant=None):
    bad, codes = 0, set()
    for cthr, meff, nib, what in hand_columns():
        for M in sorted({meff, 4} if meff <= 4 else {meff}):
            tq, low, code = (np.array(a, dtype=np.int64) for a in pk_column_full(cthr, meff, M))
            codes |= set(code.tolist())
            pts = {(0, 0), (0xFFFF, 0xFFFF), (0xFFFF, 0xFFFE)}
            for x in cthr:
                if int(x) == NEVER:
                    continue
                xh, xl = draws_around(np.array([int(x) >> 16]), np.array([int(x) & 0xFFFF]))
                pts |= set(zip(xh[0].tolist(), xl[0].tolist()))
            xh, xl = (np.array(v, dtype=np.int64) for v in zip(*sorted(pts)))
            got = recount_bins(tq[None, :], low[None, :], code[None, :], np.int64(nib), meff, xh, xl, mutant)
            x = np.minimum((xh << 16) | xl, 0xFFFFFFFE)
            n = (x[:, None] >= cthr[None, :]).sum(axis=1)               # copies fire together; a clamped draw never reaches "never"
            want = (nib >> (4 * n)) & 15
            if mutant is None:
                assert np.array_equal(got, want), (what, M, [(hex(a), hex(b)) for a, b in zip(xh[got != want], xl[got != want])][:4])
            bad += int((got != want).sum())
    return bad, codes


def test_recount_on_hand_made_columns():
    bad, codes = check_hand()
    assert bad == 0
    assert {0, 1, 2, 3, 7} <= codes, codes             # ordinary, H = 0 / a shift of 1, larger shifts, never
    for m in MUTANTS:
        assert check_hand(mutant=m)[0] > 0, "the mutant %s passes" % m


# ---- the resample compare ---------------------------------------------------------------------------------------------------------
def resample_hits(R, rh, rl, mutant=None):
    """hit8's bits in the recount: (R_h, R_l) > (r_h, r_l), from RR1 = (R >> 16) + 1 and the low half of R as the kernel has them."""
    RR1 = (R >> 16) + 1
    return gt32(np.int64(RR1 - 1), np.int64(R & 0xFFFF), rh, rl, 0, low_gt=(mutant == "low_gt"))


def test_resample_recount_is_the_32_bit_compare(model_dir):
    lib = L.lib()
    rates = set()
    for name in sorted(MODELS):
        rates |= {float(x) for x in tie_model(name, model_dir)[1]["resample_rates"][:3]}
    for _, nm, path in shipped_fast_branch_models(model_dir):
        pp = O.parse_model_txt(path)
        rates |= {float(x) for x in np.asarray(pp["resample_rates"], dtype=np.float64).ravel()}
    Rs = sorted({int(lib.emgpu_debug_bernoulli_threshold(x)) for x in rates} | {0, 1, 0x10000, 0xFFFEFFFF})
    Rs = [R for R in Rs if R < 0xFFFF0000]                  # the fast kernel's own condition (fast_uncor_eligible)
    assert len([R for R in Rs if R]) >= 3
    bad = 0                                                 # of the three mutants only the low-half one reaches this compare: no codes, no shifts
    for R in Rs:
        rh, rl = draws_around(np.array([R >> 16]), np.array([R & 0xFFFF]))
        want = ((rh << 16) | rl) < R                        # resample_events.m:24 on the draw as drawn
        assert np.array_equal(resample_hits(R, rh, rl) == 1, want), hex(R)
        assert np.all(resample_hits(R, rh, rl) <= 1)
        bad += int((resample_hits(R, rh, rl, "low_gt") != want).sum())
    assert bad > 0, "the mutant low_gt passes"


# ---- the single tie word of the high-halfword pass -----------------------------------------------------------------------------------
def pk_words(xh, rh, tq, zc, RR1):
    """eight_seconds_pk's per-lane words for eight seconds of draws: par, zt, hitA (xh, rh: (n, 8) high halfwords; tq: (n, M); zc: (n,))."""
    par = np.zeros(len(xh), np.int64)
    hitA = np.zeros(len(xh), np.int64)
    for p in range(4):
        acc = np.zeros(len(xh), np.int64)
        u = np.zeros(len(xh), np.int64)
        for half in (0, 1):
            x, r = xh[:, 2 * p + half], rh[:, 2 * p + half]
            a = sum(np.minimum(sat(x, tq[:, t]), 2) for t in range(tq.shape[1]))
            acc |= (a & 0xFFFF) << (16 * half)
            u |= np.minimum(sat(RR1, r), 2) << (16 * half)
        par |= acc
        hitA = ((hitA << 2) | u) & 0xFFFFFFFF if p else u
    mz = xh.min(axis=1, initial=0xFFFF, where=(np.arange(8) % 2 == 0)[None, :]) | (xh.min(axis=1, initial=0xFFFF, where=(np.arange(8) % 2 == 1)[None, :]) << 16)
    z2 = zc * 0x00010001
    zt = sat(z2 & 0xFFFF, mz & 0xFFFF) | (sat(z2 >> 16, mz >> 16) << 16)
    return par, zt, hitA


def test_the_single_tie_word_is_non_zero_exactly_where_the_two_bits_were():
    rs = np.random.RandomState(0x71E)
    n, M = 200000, 4
    tq = np.sort(rs.randint(0, 48, size=(n, M)), axis=1) + np.arange(M)[None, :]      # small values: ties in most rows
    tq[rs.rand(n) < 0.3, M - 1] = 0xFFFF
    zc = (rs.rand(n) < 0.5).astype(np.int64)
    xh = rs.randint(0, 56, size=(n, 8)).astype(np.int64)
    rh = rs.randint(0, 56, size=(n, 8)).astype(np.int64)
    quiet = rs.rand(n) < 0.5                                 # half the rows: draws far above every threshold, so that rows without any tie occur
    xh[quiet] += 1000
    rh[quiet] += 1000
    RR1 = rs.randint(1, 56, size=n).astype(np.int64)
    par, zt, hitA = pk_words(xh, rh, tq, zc, RR1)
    # the old two bits, from the draws themselves and not from the pass's words: bit 0 -- an odd count or a needed x_h == 0 in some
    # second; bit 1 -- R_h == r_h in some second
    s = sum(np.clip(xh - tq[:, t][:, None], 0, 2) for t in range(M))
    amb_old = ((((s & 1) != 0).any(axis=1) | ((xh == 0).any(axis=1) & (zc == 1))) * 1) | ((rh == (RR1 - 1)[:, None]).any(axis=1) * 2)
    tie_t, tie_r = (par & 0x00010001) | zt, hitA & 0x00550055                                # the pass's two words
    word = tie_t | tie_r                                                                     # what it returns now
    assert np.array_equal(word != 0, amb_old != 0)
    assert np.array_equal((tie_t != 0) * 1 | (tie_r != 0) * 2, amb_old)                      # the redo's `which`, from the same words
    seen = np.bincount(amb_old, minlength=4)
    assert np.all(seen > 100), seen                          # none, transition only, resample only, both
