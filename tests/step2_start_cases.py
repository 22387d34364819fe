"""Shared inputs of test_gpu_step2_start_grid.py: the models k_uncor_fast does not take, six preset rows per model, the interleaved grid and the
oracle's answer for it (one oracle run per row with the model's start set, gathered at i = k mod 6; computed once per case) -- start_grid_cases'
scheme (its N, T, SEED, FIRST, COL, LD) for the +start instances of k_dbn_step2.

A row is indexed by variable id, 0 = draw.  Row 5 (R5) is every bin of trajectory R5_FROM of an unconstrained oracle run.  What the oracle gives
for these exact inputs -- R5, the rejection attempts under each row, the rows per list -- is asserted here, so that the inputs keep exercising
what they were chosen for."""
import numpy as np

import instances as I
import oracle as O
import start_grid_cases as S
from util import load_row_model

N, T, SEED, FIRST, COL, LD, R5_FROM = S.N, S.T, S.SEED, S.FIRST, S.COL, S.LD, S.R5_FROM


def _row16(**kw):
    """a cor_v1 / littoral_cor_v1 row from variable ids (1-based, as the model file numbers them)"""
    row = [0] * 16
    for k, v in kw.items():
        row[int(k[1:]) - 1] = v
    return row


# A 1, L 2, chi 3, beta 4, C_1 5, C_2 6, v_1 7, v_2 8, dv_1 9, dv_2 10, dh_1 11, dh_2 12, dpsi_1 13, dpsi_2 14, hmd 15, vmd 16; the initial
# order is 2,1,5,6,11,12,8,7,4,9,10,13,14,16,15,3: a variable's position is not its id.  R0 the root; R2 the root and its child; R3 a vmd
# stratum with its parents L, dh_1, dh_2; R4 the airspace, the layer and both categories
_ROWS16 = [_row16(v2=3), [0] * 16, _row16(v1=2, v2=2), _row16(v2=3, v11=4, v12=6, v16=2), _row16(v1=1, v2=4, v5=2, v6=1)]

CASES = {
    # name: model (a shipped model's name or instances.shaped arguments), per_step, the general instance's name, rows 0-4 (None:
    # start_grid_cases' own), R5, the trajectories of each row's run that need more than one attempt and the most attempts any needs
    "uncor_1200code_v1": dict(model="uncor_1200code_v1", inst="k_dbn_step2<7,3>",
                              rows=[[4, 2, 0, 0, 0, 0], [0] * 6, [3, 0, 0, 0, 0, 0], [2, 2, 0, 0, 0, 0], [4, 2, 1, 0, 0, 0]],
                              r5=[4, 4, 8, 4, 3, 4], second=[0, 0, 0, 0, 18, 0], most=2),
    "glider_v1": dict(model="glider_v1", inst="k_dbn_step2<7,3>",
                      rows=[[2, 0, 0, 0, 0], [0] * 5, [3, 0, 0, 0, 0], [2, 2, 0, 0, 0], [2, 1, 0, 0, 0]],
                      r5=[2, 7, 5, 3, 4], second=[1, 2, 1, 0, 157, 0], most=4),
    "cor_v1": dict(model="cor_v1", inst="k_dbn_step2<16,4>", rows=_ROWS16, r5=[4, 3, 2, 10, 2, 2, 1, 1, 3, 3, 7, 6, 5, 7, 3, 8],
                   second=[0] * 6, most=1, list_mean=(13.8, 14.75)),
    "littoral_cor_v1": dict(model="littoral_cor_v1", inst="k_dbn_step2<16,4>[frozen]", rows=_ROWS16,
                            r5=[2, 2, 2, 9, 2, 2, 1, 1, 3, 3, 6, 5, 5, 7, 3, 8], second=[0] * 6, most=1),
    # ni 2, one dynamic variable in a four-variable instance
    "weatherballoon_v1": dict(model="weatherballoon_v1", inst="k_dbn_step2<16,4>[frozen]", rows=[[2, 0], [0, 0], [5, 0], [2, 3], [6, 7]],
                              r5=[1, 4], second=[0] * 6, most=1),
    # every parent has a lower id: any prefix is closed
    "shaped9": dict(model=I.shaped(923, 9, (2, 6, 3), dependent=True), inst="k_dbn_step2<9,3>",
                    rows=[[1] + [0] * 8, [0] * 9, [2] + [0] * 8, [1, 1] + [0] * 7, [1, 1, 1] + [0] * 6],
                    r5=[3, 8, 3, 1, 2, 2, 1, 1, 3], second=[0] * 6, most=1, list_mean=(90.0, 96.0), list_max=111),
    "uncor_1200code_v2p1-perstep": dict(model="uncor_1200code_v2p1", per_step=True, inst="k_dbn_step2<7,3>", rows=None),
}
NAMES = list(CASES)

_cache = {}


def kernel_name(case, form):
    """the name a call with a grid reports: the general instance's of the model's shape, '+start' appended last"""
    return CASES[case]["inst"] + ("+rows-by-wave+events" if form == "list" else "") + "+start"


def load(case, model_dir):
    """(native model, oracle parms dict, path)"""
    return load_row_model(CASES[case]["model"], model_dir)


def per_step(case):
    return bool(CASES[case].get("per_step"))


def rows_of(case, model_dir):
    """The six rows of a case ([6, n_initial] int32)."""
    key = ("rows", case)
    if key not in _cache:
        c = CASES[case]
        if c["rows"] is None:
            _cache[key] = S.rows_of(c["model"], model_dir)      # (R5 of the fast-branch run: the initial network does not depend on the branch)
        else:
            _, pp, _ = load(case, model_dir)
            free = O.uncor_sample(O.OracleModel(pp), R5_FROM - FIRST + 1, T, SEED, first_index=FIRST, want_dense=False, want_events=False,
                                  per_step=per_step(case))
            r5 = [int(b) for b in free["init_bin"][R5_FROM - FIRST]]
            assert r5 == c["r5"], (case, r5)
            _cache[key] = np.array(c["rows"] + [r5], dtype=np.int32)
    return _cache[key]


def grid_of(case, model_dir, n=N):
    """Interleaved: trajectory i gets rows[i % 6], so every wave holds all six rows."""
    return np.ascontiguousarray(rows_of(case, model_dir)[np.arange(n) % 6])


def per_row_of(case, model_dir):
    """The oracle's uncor_sample dict of each row's own run (the model's start = the row, all N trajectories).  Left unchanged by its users."""
    key = ("per", case)
    if key not in _cache:
        c = CASES[case]
        _, pp, _ = load(case, model_dir)
        per = [O.uncor_sample(O.OracleModel(pp, start=[int(v) for v in row]), N, T, SEED, first_index=FIRST, per_step=per_step(case))
               for row in rows_of(case, model_dir)]
        if c["rows"] is None:     # start_grid_cases' own assert: second attempts under R4
            a4 = per[4]["attempts"]
            assert int((a4 > 1).sum()) == S.R4_SECOND_ATTEMPTS[c["model"]] and a4.max() < 1000, (case, int((a4 > 1).sum()))
        else:
            second = [int((p["attempts"] > 1).sum()) for p in per]
            most = max(int(p["attempts"].max()) for p in per)
            assert second == c["second"] and most == c["most"] and min(int(p["attempts"].min()) for p in per) == 1, (case, second, most)
        if "list_mean" in c:
            means = [float(np.mean([len(e) for e in p["events"]])) for p in per]
            assert all(c["list_mean"][0] <= m <= c["list_mean"][1] for m in means), (case, means)
        if "list_max" in c:
            assert max(len(e) for p in per for e in p["events"]) == c["list_max"], case
        _cache[key] = per
    return _cache[key]


def oracle_of(case, model_dir):
    """The oracle's answer for the interleaved grid: row k's run at i = k mod 6.  Left unchanged by its users."""
    key = ("oracle", case)
    if key not in _cache:
        per = per_row_of(case, model_dir)
        ref = {f: np.stack([per[i % 6][f][i] for i in range(N)]) for f in ("init_bin", "init_val", "attempts", "dense_bin", "dense_val")}
        ref["events"] = [per[i % 6]["events"][i] for i in range(N)]
        _cache[key] = ref
    return _cache[key]


# ---- UncorEncounterModel.track on uncor_1200code_v1: the four rows that can fly (the oracle rejects R4, the lowest speed bin, and R5, the
# highest, in every round), interleaved i % 4
TRACK_CASE, TRACK_ROWS = "uncor_1200code_v1", [0, 1, 2, 3]
TN, TT, TSEED, TRACK_ROUNDS = 300, 30, 5, 8
TRACK_LATER = 93        # trajectories that need more than one round (all within 6)


def track_rows(model_dir):
    return rows_of(TRACK_CASE, model_dir)[TRACK_ROWS]


def track_oracle(model_dir):
    """(attempts of the interleaved call [TN], attempts of each row's own run): the oracle accepts every trajectory within TRACK_ROUNDS rounds and
    TRACK_LATER of them need more than one."""
    key = ("track",)
    if key not in _cache:
        _, pp, _ = load(TRACK_CASE, model_dir)
        rows = track_rows(model_dir)
        per = [O.uncor_track(O.OracleModel(pp, start=[int(v) for v in row]), TN, TT, TSEED, max_track_attempts=TRACK_ROUNDS, want_tracks=False)["attempts"]
               for row in rows]
        want = np.zeros(TN, dtype=np.int32)
        for k in range(len(rows)):
            want[k::len(rows)] = per[k][k::len(rows)]
        assert want.min() >= 1 and want.max() <= TRACK_ROUNDS, (int(want.min()), int(want.max()))
        assert int((want > 1).sum()) == TRACK_LATER and TRACK_LATER >= 5, int((want > 1).sum())
        _cache[key] = (want, per)
    return _cache[key]
