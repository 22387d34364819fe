"""The ONE tie word of eight_seconds_pk in the dense forms (HISTORY.md section 31), mirrored in numpy, no GPU: the odd bits of the four
packed counts (and the x_h = 0 bit) are ORed where they are, moved once into bits 8-11 of both halves of the word that collects the
resample fields, and one mask (kTieT | kTieR) leaves the tie bits of both kinds; hit8 comes from that word by one bit select.  Checked
against the two words the pass had before (test_fast_recount.pk_words) on random lanes, and against the rule itself (an odd count, or
x_h = 0 in a lane whose column has a threshold below 2^16) around every real threshold of every shipped fast-branch column.  A mirror
that drops the odd bit of one word pair must fail both."""
import numpy as np
import pytest

from test_fast_recount import all_columns, pk_words, sat
from test_gpu_fast_ties import pk_column

K_TIE_T, K_TIE_R = 0x01000100, 0x00550055
U32 = 0xFFFFFFFF


def tie_word(xh, rh, tq, zc, RR1, drop=None):
    """eight_seconds_pk<M, ZL = true>: (the word it returns, hit8) for eight seconds of high halfwords.  xh, rh: (n, 8); tq: (n, M);
    zc, RR1: (n,) -- RR1 is R_h + 1, one half.  drop = p: the mutant that leaves the count of word pair p out of the OR."""
    n = len(xh)
    acc4, hitA = [], np.zeros(n, np.int64)
    for p in range(4):
        acc, u = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for half in (0, 1):
            x, r = xh[:, 2 * p + half], rh[:, 2 * p + half]
            a = sum(np.minimum(sat(x, tq[:, t]), 2) for t in range(tq.shape[1]))
            acc |= a << (16 * half)
            u |= np.minimum(sat(RR1, r), 2) << (16 * half)
        acc4.append(acc if p != drop else acc * 0)
        hitA = ((hitA << 2) | u) & U32 if p else u                                  # v_lshl_or_b32
    par = (acc4[0] | acc4[1] | acc4[2]) | acc4[3]                                   # v_or3_b32, v_or_b32
    even, odd = np.arange(8) % 2 == 0, np.arange(8) % 2 == 1
    mz = xh.min(axis=1, initial=0xFFFF, where=even[None, :]) | (xh.min(axis=1, initial=0xFFFF, where=odd[None, :]) << 16)
    zt = sat(zc, mz & 0xFFFF) | (sat(zc, mz >> 16) << 16)
    par = par | zt                                                                  # (the zwave branch; zt = 0 where zc = 0)
    z = ((par << 8) | hitA) & U32                                                   # v_lshl_or_b32
    hit8 = (hitA & 0xAA) | ((hitA >> 17) & ~0xAA & U32)                             # v_bitop3_b32 0xe4
    return z & (K_TIE_T | K_TIE_R), hit8


def random_lanes(M, n=200000):
    rs = np.random.RandomState(0x71E + M)
    tq = np.sort(rs.randint(0, 48, size=(n, M)), axis=1) + np.arange(M)[None, :]      # small values: ties in most rows
    tq[rs.rand(n) < 0.3, M - 1] = 0xFFFF
    zc = (rs.rand(n) < 0.5).astype(np.int64)
    xh = rs.randint(0, 56, size=(n, 8)).astype(np.int64)
    rh = rs.randint(0, 56, size=(n, 8)).astype(np.int64)
    quiet = rs.rand(n) < 0.5                                 # half the rows far above every threshold: rows without any tie occur
    xh[quiet] += 1000
    rh[quiet] += 1000
    big = rs.rand(n) < 0.1                                   # ... and some at the top of the range, where a count reaches 2 M
    xh[big] = rs.randint(0xFFF0, 0x10000, size=(int(big.sum()), 8))
    return xh, rh, tq, zc, rs.randint(1, 56, size=n).astype(np.int64)


def old_words_differ(xh, rh, tq, zc, RR1, drop=None):
    """Lanes in which the new word's two parts are not non-zero exactly where the two old words were, or hit8 differs."""
    par, zt, hitA = pk_words(xh, rh, tq, zc, RR1)
    tie_t, tie_r = (par & 0x00010001) | zt, hitA & 0x00550055
    hit8 = (hitA & 0xAA) | ((hitA >> 17) & 0x55)
    word, h8 = tie_word(xh, rh, tq, zc, RR1, drop)
    return (((word & K_TIE_T) != 0) != (tie_t != 0)) | (((word & K_TIE_R) != 0) != (tie_r != 0)) | ((word != 0) != ((tie_t | tie_r) != 0)) | (h8 != hit8)


@pytest.mark.parametrize("M", [2, 4, 7])
def test_the_word_against_the_old_two_words_on_random_lanes(M):
    lanes = random_lanes(M)
    par, zt, hitA = pk_words(*lanes)
    kinds = np.bincount((((par & 0x00010001) | zt) != 0) * 1 | ((hitA & 0x00550055) != 0) * 2, minlength=4)
    assert np.all(kinds > 100), kinds                        # none, transition only, resample only, both
    assert int((((par & 0xFFFF) >> 1) == M).sum()) > 100     # full counts (2 M in both halves of every pair) beside the tie bits
    assert not old_words_differ(*lanes).any()
    for p in range(4):
        assert old_words_differ(*lanes, drop=p).any(), "the mutant without pair %d passes" % p


def column_draws(TQ, Z, H):
    """For columns (q, M) and one real threshold's high half H (q,): the draws x_h in {H - 1, H, H + 1, 0, 1, 0xFFFF}, each in its own
    lane and in a second of its own (all eight seconds and so all four pairs and both halves occur), the other seconds at a value of the
    column's at which nothing ties.  -> xh (6 q, 8), the columns' index per lane."""
    q = len(TQ)
    cand = np.array([0xFFFF, 0x8000, 0x4000, 0x2000, 9, 7, 5, 3, 2], np.int64)
    d = np.clip(cand[None, :, None] - TQ[:, None, :], 0, 2)                          # (q, candidates, M)
    ok = (d != 1).all(axis=2)
    assert ok.any(axis=1).all(), "no quiet draw for a column"
    quiet = cand[ok.argmax(axis=1)]
    x6 = np.stack([H - 1, H, H + 1, H * 0, H * 0 + 1, H * 0 + 0xFFFF], axis=1)
    x6 = np.where((x6 < 0) | (x6 > 0xFFFF), H[:, None], x6)
    xh = np.repeat(quiet, 6)[:, None] * np.ones((1, 8), np.int64)
    col = np.repeat(np.arange(q), 6)
    sec = (np.arange(6 * q) + np.repeat(np.arange(q), 6)) % 8
    xh[np.arange(6 * q), sec] = x6.reshape(-1)
    return xh, col


def columns_differ(model_dir, drop=None):
    bad = checked = ties = 0
    for (M, meff), cols in sorted(all_columns(model_dir).items()):
        TQ, Z = np.zeros((len(cols), M), np.int64), np.zeros(len(cols), np.int64)
        real = np.zeros((len(cols), M), bool)
        Hs = np.zeros((len(cols), M), np.int64)
        for j, (row, cthr, nib) in enumerate(cols):
            tq, z = pk_column(cthr, meff, M)
            TQ[j], Z[j] = tq, int(z)
            for t in range(meff):
                x = int(cthr[t])
                real[j, t] = x != 0xFFFFFFFF and not (t > 0 and x == int(cthr[t - 1]))
                Hs[j, t] = x >> 16
        for t in range(M):
            on = real[:, t]
            if not on.any():
                continue
            xh, col = column_draws(TQ[on], Z[on], Hs[on, t])
            tq, zc = TQ[on][col], Z[on][col]
            rh = np.full_like(xh, 5000)                                              # R_h = 100: no resample tie, no hit
            word, h8 = tie_word(xh, rh, tq, zc, np.full(len(xh), 101, np.int64), drop)
            s = sum(np.clip(xh - tq[:, u][:, None], 0, 2) for u in range(M))
            want = ((s & 1) != 0).any(axis=1) | ((xh == 0).any(axis=1) & (zc == 1))  # the rule (test_gpu_fast_ties.pk_decide), any second
            bad += int((((word & K_TIE_T) != 0) != want).sum() + ((word & K_TIE_R) != 0).sum() + (h8 != 0).sum())
            checked += len(xh)
            ties += int(want.sum())
    return bad, checked, ties


def test_the_word_around_every_real_threshold_of_the_shipped_columns(model_dir):
    bad, checked, ties = columns_differ(model_dir)
    assert checked > 6 * 62535 and ties > 62535, (checked, ties)      # every column has a real threshold, and x_h = H ties with it
    assert bad == 0, bad
    for p in range(4):
        assert columns_differ(model_dir, drop=p)[0] > 0, "the mutant without pair %d passes" % p
