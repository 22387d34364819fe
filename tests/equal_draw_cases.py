"""Shared inputs of test_equal_draws.py / test_gpu_equal_draws.py: pairs of models in which ONE draw of a run equals a threshold.

A draw is a function of (seed, trajectory index, attempt, section, variable, block) alone -- not of the model.  So a target (trajectory i0,
second c, variable) is picked in a run by searching its draws from the slot map, its 32-bit word x is computed, and the model is rewritten
around it: every column of the variable's table gets integer counts that sum to 2^32, whose cumulative sums are then exactly the column's
thresholds (s_k < 2^32 u(x) <=> x >= s_k), as many distinct ones as the variable's meff so that instance and width stay.  Model "at" has
X_t = x (the draw fires threshold t: bin t + 2), model "above" X_t = x + 1 (bin t + 1); the other thresholds stay far from x.  For a
Bernoulli draw the rate (x + 1) / 2^32 compiles to R = x + 1 (a hit), (x + 0.5) / 2^32 to R = x (no hit).  An off-by-one in a kernel's
compare moves exactly this draw; under random sampling it has probability 2^-32 per draw.

Kinds of target: "trans" a transition draw (TRANS with TRANS_LO), "res" the Bernoulli of a dynamic variable (RES with RES_LO), "res_static"
that of a static variable (event forms), "init" the root of the initial network (the INIT word)."""
import ctypes as C
import os

import numpy as np

import instances as I
import oracle as O
import step2_tie_cases as S
from em_model_manned_bayes_amd import em_io, native, _lib as L
from util import shaped_model

N, FIRST = 64 * 3 + 37, 2**33 + 11
TWO32 = 2**32


def _unguarded(T):
    return lambda c: (c >= 1) & (8 * (c >> 3) + 7 < T)


M73 = I.shaped(723, 7, (2, 5, 3), parents=I.NOT_A_FAMILY)             # <7,3,reg>: plain, packed, plain; variable 0 is a new-value parent of 2
M73EV = I.shaped(780, 7, (2, 3, 3), parents=I.NOT_A_FAMILY, rates=I.rates_on(7, 3, extra=(3, 4)))
M164 = I.shaped(1643, 8, (2, 5, 3, 6), dependent=True)
F242, F466 = I.shaped(703, 7, (2, 4, 2)), I.shaped(775, 7, (4, 6, 6), rates=I.rates_on(7, 3, extra=(3, 4)))
BN8 = I.shaped(761, 8, (2, 2, 2))
# name: model, the kernel the call must report, form (instances.py's; "bn" = emgpu_sample_bn_host), T, kind and variable of the target (k: the
# dynamic variable in plan order; v: the static variable's id), where the target may lie (second c, word x), the seeds searched.
CASES = {
    "step2 packed, even second": dict(model=M73, kernel="k_dbn_step2<7,3,reg>", form="both", T=41, kind="trans", k=1,
                                      where=lambda c, x, T: _unguarded(T)(c) & (c % 2 == 0)),
    "step2 plain level-0 parent, odd second": dict(model=M73, kernel="k_dbn_step2<7,3,reg>", form="both", T=41, kind="trans", k=0,
                                                   where=lambda c, x, T: _unguarded(T)(c) & (c % 2 == 1)),
    "step2 partial last block": dict(model=M73, kernel="k_dbn_step2<7,3,reg>", form="both", T=21, kind="trans", k=1,
                                     where=lambda c, x, T: c >= 16),
    "step2 packed, x_h == 0": dict(model=M73, kernel="k_dbn_step2<7,3,reg>", form="both", T=41, kind="trans", k=1,
                                   where=lambda c, x, T: _unguarded(T)(c) & (x >> 16 == 0) & (x > 0)),
    "step2 plain, x_h == 0": dict(model=M73, kernel="k_dbn_step2<7,3,reg>", form="both", T=41, kind="trans", k=2,
                                  where=lambda c, x, T: _unguarded(T)(c) & (x >> 16 == 0) & (x > 0)),
    "step2 Bernoulli of a dynamic variable": dict(model=M73, kernel="k_dbn_step2<7,3,reg>", form="both", T=41, kind="res", k=2,
                                                  where=lambda c, x, T: _unguarded(T)(c) & (x < 0x30000000)),
    "step2 Bernoulli tie redo (exact_hit)": dict(model=M73, kernel="k_dbn_step2<7,3,reg>", form="both", T=41, kind="res", k=1,
                                                 where=lambda c, x, T: _unguarded(T)(c) & (x < 0x30000000) & (c % 2 == 1)),
    "step2 +events, Bernoulli of a static variable": dict(model=M73EV, kernel="k_dbn_step2<7,3,w4,reg>+events", form="list+dense", T=41,
                                                          kind="res_static", v=3, where=lambda c, x, T: (c >= 1) & (x < 0x30000000)),
    "step2 draw 0xFFFFFFFE against a threshold 0xFFFFFFFE (clamp32)": dict(
        model=I.shaped(721, 6, (2, 3, 3), parents=I.NOT_A_FAMILY), kernel="k_dbn_step2<7,3,w4,reg>", form="both", T=64, kind="trans", k=0,
        seeds=[0xE0A1], first=17205936876 - 100, where=lambda c, x, T: x == 0xFFFFFFFE),       # (found by a search over 2^33 draws)
    "step2 draw 0xFFFFFFFF (clamp32)": dict(
        model=I.shaped(721, 6, (2, 3, 3), parents=I.NOT_A_FAMILY), kernel="k_dbn_step2<7,3,w4,reg>", form="both", T=64, kind="trans", k=0,
        seeds=[0xE0A1], first=17218007807 - 100, where=lambda c, x, T: x == 0xFFFFFFFF),       # (the same search)
    "fast <7,2,4,2>: recount on chip": dict(model=F242, kernel="k_uncor_fast<7,2,4,2>", form="both", T=41, kind="trans", k=1,
                                            where=lambda c, x, T: _unguarded(T)(c)),
    "fast <7,2,4,2>: Bernoulli": dict(model=F242, kernel="k_uncor_fast<7,2,4,2>", form="both", T=41, kind="res", k=0,
                                      where=lambda c, x, T: _unguarded(T)(c) & (x < 0x30000000)),
    "fast <7,4,6,6>: recount from memory": dict(model=F466, kernel="k_uncor_fast<7,4,6,6>", form="both", T=41, kind="trans", k=2,
                                                where=lambda c, x, T: _unguarded(T)(c)),
    "fast evu": dict(model=F242, kernel="k_uncor_fast_evu<7,2,4,2>", form="list", T=41, kind="trans", k=1, where=lambda c, x, T: _unguarded(T)(c)),
    "step <7,3,8,lds>": dict(model=I.STEP_MODELS["7,3"], kernel="k_dbn_step<7,3,8,lds>", form="both", T=41, kind="trans", k=1,
                             where=lambda c, x, T: c >= 1),
    "step <7,3,8,lds> Bernoulli": dict(model=I.STEP_MODELS["7,3"], kernel="k_dbn_step<7,3,8,lds>", form="both", T=41, kind="res", k=2,
                                       where=lambda c, x, T: (c >= 1) & (x < 0x30000000)),
    "generic <7,3,4>": dict(model=I.shaped(751, 6, (2, 3, 3), dependent=True, rates=I.rates_on(6, 3, first=1.0)), kernel="k_dbn_generic<7,3,4>",
                            form="both", T=41, kind="trans", k=2, where=lambda c, x, T: c >= 1),
    "generic <7,3,4> Bernoulli": dict(model=I.shaped(751, 6, (2, 3, 3), dependent=True, rates=I.rates_on(6, 3, first=1.0)), kernel="k_dbn_generic<7,3,4>",
                                      form="both", T=41, kind="res", k=1, where=lambda c, x, T: (c >= 1) & (x < 0x30000000)),
    "root through init_network": dict(model=M73, kernel="k_dbn_step2<7,3,reg>", form="both", T=9, kind="init", where=lambda c, x, T: x > 0),
    "root through init_network_karg": dict(model=M164, kernel="k_dbn_step2<16,4,reg>", form="both", T=9, kind="init", where=lambda c, x, T: x > 0),
    "root through init_network_ps": dict(model=M73, kernel="k_dbn_step2<7,3>+start", form="start", T=9, kind="init", where=lambda c, x, T: x > 0),
    "root through k_bn<8>": dict(model=BN8, kernel="k_bn<8>", form="bn", T=1, kind="init", where=lambda c, x, T: x > 0),
}
NAMES = list(CASES)
STEP_NO_LDS = ("step <7,3,8,lds>", "k_dbn_step<7,3,8>", {"EMGPU_DEBUG_STEP_NO_LDS": "1"})    # the same pair in a child process with this variable
_cache = {}


def _base(case, model_dir):
    """(parms dict, native model, oracle parms) of the case's unedited model"""
    kw = dict(case["model"])
    key = ("base", repr(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _cache:
        p = shaped_model(np.random.RandomState(kw.pop("seed")), **kw)
        path = os.path.join(str(model_dir), "equal_base_%d.txt" % len(_cache))
        em_io.em_write(p, path)
        _cache[key] = (p, native.NativeModel.load_txt(path), O.parse_model_txt(path))
    return _cache[key]


def dyn_plan(nm, pp):
    """per dynamic variable in plan order: (0-based transition variable, initial variable, row of the trace, meff)"""
    tm = np.asarray(pp["temporal_map"]).reshape(-1, 2) - 1
    out = []
    for tv, meff in S.plan_meff(nm).items():
        slot = int(np.flatnonzero(tm[:, 1] == tv)[0])
        out.append((tv, int(tm[slot, 0]), slot, meff))
    return out


def draws_of(kind, a, gidx, T, seed):
    """[n, T] the 32-bit word of every second's draw (attempt 0), unclamped; "init": one column, the INIT word of variable a"""
    att = np.zeros(len(gidx), dtype=np.int64)
    if kind == "init":
        return S.block_words(1, 0, gidx, att, (a >> 2) + 1, seed)[:, a >> 2, a & 3][:, None]
    sec = S.SEC_TRANS if kind == "trans" else S.SEC_RES
    G8 = (T + 7) // 8
    odd = (np.arange(T) & 1).astype(bool)[None, :]
    wh, wl = (S.per_second(S.block_words(s, a, gidx, att, G8, seed), T) for s in (sec, sec + S.SEC_LO))
    return (S.half(wh, odd) << 16) | S.half(wl, odd)


def thresholds_with(x, m):
    """m thresholds, ascending: the even grid (j + 1) 2^32 / (m + 1) with the value nearest to x replaced by x; -> (thresholds, t)"""
    grid = [(j + 1) * TWO32 // (m + 1) for j in range(m)]
    t = int(np.argmin([abs(g - x) for g in grid]))
    grid[t] = int(x)
    assert all(a < b for a, b in zip(grid, grid[1:])) and 0 < grid[0] and grid[-1] < TWO32 - 1
    return grid, t


def counts_of(thresholds, r):
    c = np.zeros(r)
    c[: len(thresholds) + 1] = np.diff([0] + list(thresholds) + [TWO32])
    assert c.sum() == TWO32 and np.all(c[: len(thresholds) + 1] > 0)
    return c


def build(name, model_dir):
    """The pair of a case: dict(at=(native, oracle parms), above=..., i0, c, x, seed, first, slot / var, want_at, want_above, thresholds
    or R of both, ...), made once per session."""
    if name in _cache:
        return _cache[name]
    case = CASES[name]
    p, nm, pp = _base(case, model_dir)
    T, kind = case["T"], case["kind"]
    ni = int(p["n_initial"])
    out = dict(kind=kind, T=T)
    if kind in ("trans", "res"):
        tv, iv, slot, meff = dyn_plan(nm, pp)[case["k"]]
        a = tv if kind == "trans" else iv
        out.update(slot=slot, var=iv, tvar=tv, meff=meff)
    elif kind == "res_static":
        a = case["v"]
        out.update(var=a)
    else:
        a = int(pp["order_initial"][0]) - 1
        assert not np.asarray(pp["G_initial"])[:, a].any()
        out.update(var=a)
    first = case.get("first", FIRST)
    gidx = np.uint64(first) + np.arange(N, dtype=np.uint64)
    for seed in case.get("seeds", range(0x0E00, 0x0E00 + 20000)):
        X = draws_of(kind, a, gidx, T, seed)
        ok = np.broadcast_to(case["where"](np.arange(X.shape[1])[None, :], X, T), X.shape).copy()
        ok[:64] = False                                        # i0 inside the run: not in its first wave
        if kind == "res" and ok.any():
            # a hit shows in the dense trace only where the bin stays and is not the zero bin (a transition's own draw hides it, a zero bin has
            # no value to draw); the rates move no bin, so the unedited model's run says where that is
            ref = O.uncor_sample(O.OracleModel(pp), N, T, seed, first_index=first, want_events=False)
            db, dv = ref["dense_bin"][:, :, slot], ref["dense_val"][:, :, slot]
            ok[:, 1:] &= (db[:, 1:] == db[:, :-1]) & (dv[:, 1:] != 0)
            ok &= (ref["attempts"] == 1)[:, None]
        if ok.any():
            i0, c = (int(v[0]) for v in np.nonzero(ok))
            break
    else:
        raise AssertionError("no target: " + name)
    x = int(S.clamp32(X[i0, c]))                               # what the compare sees
    out.update(i0=i0, c=c, x=x, word=int(X[i0, c]), seed=int(seed), first=int(first))
    pair = {}
    for which in ("at", "above"):
        q = dict(p)
        if kind == "trans":
            th, t = thresholds_with(x, meff)
            th[t] += which == "above"
            q["N_transition"] = list(p["N_transition"])
            Nt = np.array(p["N_transition"][tv], dtype=np.float64)
            Nt[:] = counts_of(th, Nt.shape[0])[:, None]
            q["N_transition"][tv] = Nt
            out["want_" + which], out["thr_" + which], out["t"] = t + 2 - (which == "above"), th, t
        elif kind == "init":
            r = int(p["r_initial"][a])
            th, t = thresholds_with(x, r - 1)
            th[t] += which == "above"
            q["N_initial"] = list(p["N_initial"])
            q["N_initial"][a] = counts_of(th, r)[:, None]
            out["want_" + which], out["thr_" + which], out["t"] = t + 2 - (which == "above"), th, t
        else:
            rr = np.array(p["resample_rates"], dtype=np.float64)
            rr[a] = (x + 1.0) / TWO32 if which == "at" else (x + 0.5) / TWO32      # "at": R = x + 1, the draw x is the last hit
            q["resample_rates"] = rr
            out["R_" + which] = x + 1 if which == "at" else x
        path = os.path.join(str(model_dir), "equal_%d_%s.txt" % (NAMES.index(name), which))
        em_io.em_write(q, path)
        pair[which] = (native.NativeModel.load_txt(path), O.parse_model_txt(path), q)
    out.update(pair)
    _cache[name] = out
    return out


def start_grid(b):
    """the +start case's grid: a row that presets nothing for every trajectory (the twin instance runs, the root is still drawn)"""
    return np.zeros((N, b["at"][0].n_initial), dtype=np.int32)


def oracle_run(name, which, model_dir):
    """The oracle's answer for one model of a case (made once): uncor_sample's dict, or geom_sample's (bins, values, attempts) for "bn"."""
    key = ("oracle", name, which)
    if key not in _cache:
        b, case = build(name, model_dir), CASES[name]
        om = O.OracleModel(b[which][1])
        if case["form"] == "bn":
            _cache[key] = O.geom_sample(om, N, b["seed"], first_index=b["first"])
        else:
            _cache[key] = O.uncor_sample(om, N, b["T"], b["seed"], first_index=b["first"])
    return _cache[key]
