"""The references of the hand-made terminal-filter cases (terminal_filter_cases.py): the C oracle's filters on a side's rows, what
k_terminal_filter must leave in its outputs, and each filter of track.m:79-145 on its own through pyref's functions.  It never imports the
library; every result is computed once per side and shared."""
import numpy as np

import oracle as O
import pair_cases as PC
import pyref as P
import terminal_filter_cases as K

_DL_KEYS = ("minVel_ft_s", "maxVel_ft_s", "maxTurnRate_deg_s", "maxAltitude_ft", "maxVertRate_ft_s")
_COLS = ("t_s", "x_nm", "y_nm", "z_ft", "heading_deg", "v_ft_s")
_oracle, _named = {}, {}


def as_dict(rows):
    """rows [n, 6] as the track pyref's functions take"""
    return {k: np.array(rows[:, i], dtype=float) for i, k in enumerate(_COLS)}


def dl_dicts(o):
    return [dict(zip(_DL_KEYS, o["dl"][a])) for a in range(2)]


def oracle(s):
    """(accepted, meta [4]) of a side by O.terminal_filters; a void attempt is rejected before anything is computed (meta None)"""
    if id(s) not in _oracle:
        o = s["opts"]
        if s["void"]:
            _oracle[id(s)] = (s, False, None)
        else:
            good, meta = O.terminal_filters(s["own"], s["intr"], s["intents"][0], s["intents"][1], o["dl"], o["cum"], o["pitch"], min_enc_time_s=o["min_enc"],
                                            thres_dist_ft=o["dist"], thres_alt_low_ft=o["alt_low"], thres_vertrate_ft_s=o["vrate"])
            _oracle[id(s)] = (s, good, meta)
    return _oracle[id(s)][1:]


def pyref(s):
    """(accepted, meta [4]) of a live side by P.terminal_filters"""
    o = s["opts"]
    good, meta = P.terminal_filters([as_dict(s["own"]), as_dict(s["intr"])], s["intents"][0], s["intents"][1], dl_dicts(o), o["cum"], o["pitch"],
                                    min_enc_time_s=o["min_enc"], thres_dist_ft=o["dist"], thres_alt_low_ft=o["alt_low"], thres_vertrate_ft_s=o["vrate"])
    return good, np.array(meta, dtype=np.float64)


def named_filters(s):
    """{filter: passed} for every name of K.FILTERS, each computed by pyref's own function for it and independently of the others"""
    if id(s) in _named:
        return _named[id(s)][1]
    o = s["opts"]
    traj = [as_dict(s["own"]), as_dict(s["intr"])]
    dl = dl_dicts(o)
    oi, ii = s["intents"]
    out = {"void": not s["void"]}
    hmd, vmd, tcpa, nc = P.get_generated_miss_distance(traj)
    out["cpa"] = bool(abs(tcpa) <= 10)
    out["enc_time"] = bool(nc >= o["min_enc"])
    c1, l1 = P.check_runway_proximity(traj[0], o["dist"], o["alt_low"])
    c2, l2 = P.check_runway_proximity(traj[1], o["dist"], o["alt_low"])
    out["prox_own"] = bool((c1 and l1) or not c1)
    out["prox_int"] = bool(not (c2 and l2)) if ii == 3 else bool((c2 and l2) or not c2)
    climb, descend = P.check_intent_vertical(traj, o["vrate"])
    out["vert_own"] = bool(descend[0] if oi == 1 else climb[0])
    out["vert_int"] = bool(descend[1] if ii == 1 else (climb[1] if ii == 2 else True))
    c = 90.0 if oi == 1 else 270.0
    h = traj[0]["heading_deg"]
    out["heading"] = bool(np.count_nonzero((h >= c - 30) & (h <= c + 30)) / len(h) >= .95)
    for a, who in enumerate(("own", "int")):
        out["limits_" + who] = bool(P.check_dynamic_limits(traj[a], dl[a], np.inf, o["pitch"][a]))
        out["cum_" + who] = not P.check_cum_turn(traj[a]["heading_deg"], o["cum"][a])
    assert set(out) == set(K.FILTERS)
    _named[id(s)] = (s, out)
    return out


def expected(sides, cap2, fill=PC.FILL):
    """what a launch on `sides` must leave in buffers that held the byte `fill`: accepted [n] u8, and for the accepted sides meta [n, 4],
    len [n, 2] and the first cap2 rows of each track in traj [n, 2, cap2, 6]; a rejected side's entries keep the fill"""
    n = len(sides)
    acc = np.zeros(n, dtype=np.uint8)
    meta = np.frombuffer(bytes([fill]) * (n * 32), dtype=np.float64).reshape(n, 4).copy()
    ln = np.frombuffer(bytes([fill]) * (n * 8), dtype=np.int32).reshape(n, 2).copy()
    traj = np.frombuffer(bytes([fill]) * (n * 2 * cap2 * 48), dtype=np.float64).reshape(n, 2, cap2, 6).copy()
    for e, s in enumerate(sides):
        good, m = oracle(s)
        if not good:
            continue
        acc[e], meta[e] = 1, m
        for a, rows in enumerate((s["own"], s["intr"])):
            ln[e, a] = rows.shape[0]
            k = min(rows.shape[0], cap2)
            traj[e, a, :k] = rows[:k]
    return {"accepted": acc, "meta": meta, "len": ln, "traj": traj}


def smoothed(tracks, rows, cap):
    """k_terminal_smooth's result on a block by the oracle: v_ft_s <- f32(local_smooth(v as f64, 5)), z_ft <- f32(local_smooth(z as f64, 15))
    over each live track's span, every other value as it was"""
    C = K.t0_row(cap)
    out = tracks.copy()
    for a in range(tracks.shape[0]):
        rf, rb = int(rows[2 * a]), int(rows[2 * a + 1])
        if rf < 1 or rb < 1:
            continue
        lo, n = C - (rb - 1), rf + rb - 1
        out[a, lo: lo + n, 4] = O.local_smooth(tracks[a, lo: lo + n, 4].astype(np.float64), 5).astype(np.float32)
        out[a, lo: lo + n, 2] = O.local_smooth(tracks[a, lo: lo + n, 2].astype(np.float64), 15).astype(np.float32)
    return out
