"""CPU: the inputs of test_gpu_step2_ties.py (step2_tie_cases.py) are what they are made to be.

The tie models carry the kinds of column they were edited for (derived from the plan compiler's debug hooks, not from the editor); every
call form lands on the kernel instance its table names; the counted oracle sample of every model holds every kind of tie at or above its
floor, or the kind is listed as not applicable with the reason (the table is printed); and the numpy mirror of the kernel's rule agrees with
select_random.m:17-20 on the thresholds the plan compiler reports for the column -- the decided bin for both extreme low halfwords, every
real tie reported, the 32-bit redo at low halfwords on and beside every threshold's -- for both halves of a packed word: at every x_h where
the rule's answer or select_random's can change, and on one rotation of the kinds per variable at every x_h in 0 .. 65535."""
import ctypes as C

import numpy as np
import pytest

import step2_tie_cases as S
from em_model_manned_bayes_amd import _lib as L
from test_dispatch import predict

X = np.arange(65536, dtype=np.int64)
FULL_RANGE = 6           # distinct columns per variable (one rotation of the kinds) checked at every x_h, not only where anything can change
MOST = 120               # distinct columns per variable checked at all (twenty rotations; a shipped model's table has thousands)


def _real(pad_row, width):
    return sorted(set(int(t) for t in pad_row[: 3 if width == 4 else 6] if 0 < t < 0xFFFFFFFF))


@pytest.mark.parametrize("name", S.NAMES)
def test_the_tie_models_have_the_columns_they_are_made_for(name, model_dir):
    pl = S.plan_of(name, model_dir)
    R = [v["R"] for v in pl["var"]]
    assert any(0 < r < 0x10000 for r in R) and any(0xFFFE0000 <= r < 0xFFFF0000 for r in R), [hex(r) for r in R]
    for k, v in enumerate(pl["var"]):
        kinds = dict(below16=0, shared=0, copies=0, none=0, ordinary=0, one=0, two=0)
        for row in v["PAD"]:
            real = _real(row, v["width"])
            hs = [x >> 16 for x in real]
            kinds["below16"] += bool(real) and hs[0] == 0
            kinds["shared"] += len(set(hs)) < len(hs)
            kinds["copies"] += 0 < len(real) < v["meff"]
            kinds["none"] += not real
            kinds["ordinary"] += bool(real) and len(set(hs)) == len(hs) and hs[0] > 0
            kinds["one"] += len(real) == 1
            kinds["two"] += len(real) == 2
            assert len(real) <= v["meff"]
        want = ["below16", "none", "ordinary"] + (["shared", "copies", "one"] if v["meff"] >= 2 else []) + (["two"] if v["meff"] >= 3 else [])
        assert all(kinds[w] > 0 for w in want), (name, k, v["meff"], kinds)
        if v["width"] == 4:      # the plain form marks the slots past the variable's meff with 0x10000
            assert np.all(v["PK"][:, v["meff"]:3] == 0x10000) and np.all(v["PK"][:, : v["meff"]] < 0x10000)


@pytest.mark.parametrize("name", S.NAMES)
def test_every_instance_name_is_predicted(name, model_dir):
    nm, _, _ = S.tie_model(name, model_dir)
    for form, want in S.MODELS[name]["kernels"].items():
        got = predict(nm, "dense" if form == "start" else form, per_step=S.per_step(name), grid=form == "start")
        assert got == want, (name, form, got)


def test_every_listed_instance_has_a_model():
    have = {k for m in S.MODELS.values() for k in m["kernels"].values()}
    want = ["<7,3,w4,reg>", "<7,3,w8,reg>", "<7,3,reg>", "<7,3>", "<9,3,w8,reg>", "<16,4,w4,reg>", "<16,4,w8,reg>", "<16,4,reg>",
            "<16,4,w4,reg>[cor]", "<16,4,w8,reg>[cor]", "<7,3,reg>[chain,w884]", "<7,3,reg>[2<-1,w484]", "<7,3,reg>[1<-0,2<-0,w848]",
            "<7,3,reg>[per-step,w484]", "<16,4,w4,reg>[frozen]", "<7,3,reg>[chain]+events", "<16,4,reg>+rows-by-wave+events", "<9,3,reg>+events",
            "<7,3>+start", "<16,4>+start"]
    assert not [w for w in want if "k_dbn_step2" + w not in have]


@pytest.mark.parametrize("name", S.NAMES)
def test_counted_samples_hold_every_kind(name, model_dir):
    """A condition on the inputs of the counted GPU run (the model's seed was picked for it on the CPU)."""
    _, counts, first = S.counted_sample(name, model_dir)
    print("\n%s, seed %#x (first wave with a redo in block 0: %d)\n%s" % (name, S.MODELS[name]["seed"], (first - S.FIRST) // 64, S.kinds_table(name, model_dir, counts)))
    assert not S.floors_missed(name, model_dir, counts)
    na = S.not_applicable(name, model_dir)
    assert all(counts[k] == 0 for k in na if "expectation" not in na[k]), "a kind listed as not applicable occurs"


def _true_bin(x, thr):
    return 1 + (S.clamp32(x)[:, None] >= thr[None, :]).sum(axis=1)


def _check_column(v, pk, pad, thr, xs, redo=True):
    """One column at the high halfwords xs, through both halves of a packed word (the other half holds something else)."""
    pk, pad = [int(w) for w in pk], [int(w) for w in pad]
    lows = {0, 0xFFFF}
    for t in thr:
        lows.update(((int(t) & 0xFFFF) + d) & 0xFFFF for d in (-1, 0, 1))
    for odd in (False, True):
        w = (xs << 16) | 0x1234 if odd else xs | (0x4321 << 16)
        if v["width"] == 4:
            off, amin = S.plain_fired7(odd, w, pk[0], pk[1], pk[2])
            tie, decided = amin == 0, (pk[3] >> off) & 15
            th, table = pad[:3], pad[3]
        else:
            sel = S.or_half(odd, S.pk_fired2(odd, w, pk[0], pk[1], pk[2]), w)
            tie, decided = (sel & 1) != 0, (pk[3] >> (4 * (sel >> 1))) & 15
            th, table = pad[:6], pad[6] | (pad[7] << 32)
        lo, hi = _true_bin(xs << 16, thr), _true_bin((xs << 16) | 0xFFFF, thr)
        assert np.all(tie[lo != hi]), "a real tie is not reported"
        assert np.array_equal(decided[~tie], lo[~tie]) and np.array_equal(decided[~tie], hi[~tie]), "a decided bin differs"
        for low in sorted(lows) if redo else ():
            wl = np.full_like(xs, (low << 16) | 0x0F0F if odd else low | (0xF0F0 << 16))
            x = S.full_draw(odd, w, wl)
            redone = (table >> (8 * S.exact_borrows(x, th))) & 0xFF
            assert np.array_equal(redone, _true_bin((xs << 16) | low, thr)), ("the 32-bit redo differs", low)


@pytest.mark.parametrize("name", S.NAMES)
def test_the_mirror_decides_like_select_random(name, model_dir):
    nm, _, _ = S.tie_model(name, model_dir)
    pl = S.plan_of(name, model_dir)
    lib = L.lib()
    for k, v in enumerate(pl["var"]):
        seen, full = set(), 0
        tvar, r, q, meff, mp = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_uint32()
        thr, cthr = np.zeros(64, dtype=np.uint32), np.zeros(7, dtype=np.uint32)
        for col in range(len(v["PK"])):
            key = v["PK"][col].tobytes() + v["PAD"][col].tobytes()
            if key in seen or len(seen) >= MOST:
                continue
            seen.add(key)
            L.check(lib.emgpu_debug_dynamic_column(nm._h, k, col, C.byref(tvar), C.byref(r), C.byref(q), thr.ctypes.data, C.byref(meff),
                                                   cthr.ctypes.data, C.byref(mp)))
            assert r.value - 1 <= 15
            row = thr[: r.value - 1].astype(np.int64)
            at = {0, 1, 2, 65535}
            for t in list(row) + [int(x) for x in v["PAD"][col][: 3 if v["width"] == 4 else 6]]:
                at.update(((int(t) >> 16) + d) for d in (-2, -1, 0, 1, 2, 3))
            if v["width"] == 8:
                for w in v["PK"][col][:3]:
                    for tq in (int(w) & 0xFFFF, int(w) >> 16):
                        at.update(tq + d for d in (-1, 0, 1, 2, 3))
            xs = np.array(sorted(x for x in at if 0 <= x <= 65535), dtype=np.int64)
            try:
                _check_column(v, v["PK"][col], v["PAD"][col], row, xs)
                if full < FULL_RANGE:
                    full += 1
                    _check_column(v, v["PK"][col], v["PAD"][col], row, X, redo=False)
            except AssertionError as e:
                raise AssertionError((name, k, col, [hex(int(t)) for t in row]) + e.args)
