"""Shared inputs of test_start_grid.py / test_gpu_start_grid.py: the models, the six preset rows per model, the interleaved grid and the
oracle's answer for it (one oracle run per row with the model's start set, gathered at i = k mod 6; computed once per model)."""
import numpy as np

import oracle as O
from util import load_pair

MODELS = ["uncor_1200code_v2p1", "uncor_1200only_fwse_v1p2", "haa_v1"]
N, T, SEED, FIRST = 700, 37, 0xA5, 300      # two full workgroups + 188 lanes (a 60-lane last wave); T neither a multiple of 4 nor of 8
COL, LD = 100, 1024                         # the device-pointer call: leading idle lanes with negative trajectory numbers
R5_FROM = 303                               # R5: every variable preset to the bins of this trajectory of an unconstrained oracle run

# R0 RUN_uncor.m:42-44 (G, A, L), R1 nothing, R2 the root alone, R3 the first two, R4 the lowest speed bin (second rejection attempts under
# presets: 28 / 14 / 2 of the 700 trajectories below, none at the cap), R5 from the oracle (no INIT draw at all)
_ROWS7 = [[1, 4, 2, 0, 0, 0, 0], [0] * 7, [3, 0, 0, 0, 0, 0, 0], [2, 2, 0, 0, 0, 0, 0], [1, 4, 2, 1, 0, 0, 0]]
# haa_v1: "L", "v", "\psi", "\psi_f", "d_f", "d_s", "\dot h", "\dot v", "\dot \psi" -- a chain like the others, so the analogous rows are
# prefixes too; its speed is the second variable
_ROWS9 = [[2, 3, 4] + [0] * 6, [0] * 9, [3] + [0] * 8, [2, 2] + [0] * 7, [2, 1] + [0] * 7]
R5_EXPECTED = {"uncor_1200code_v2p1": [1, 4, 4, 7, 3, 4, 4], "uncor_1200only_fwse_v1p2": [1, 4, 4, 6, 3, 4, 4]}
R4_SECOND_ATTEMPTS = {"uncor_1200code_v2p1": 28, "uncor_1200only_fwse_v1p2": 14, "haa_v1": 2}

_cache = {}


def rows_of(name, model_dir):
    """The six rows of a model ([6, n_initial] int32)."""
    key = ("rows", name)
    if key not in _cache:
        _, pp, _ = load_pair(name, model_dir)
        free = O.uncor_sample(O.OracleModel(pp), R5_FROM - FIRST + 1, T, SEED, first_index=FIRST, want_dense=False, want_events=False)
        r5 = [int(b) for b in free["init_bin"][R5_FROM - FIRST]]
        if name in R5_EXPECTED:
            assert r5 == R5_EXPECTED[name], (name, r5)
        base = _ROWS7 if pp["n_initial"] == 7 else _ROWS9
        _cache[key] = np.array(base + [r5], dtype=np.int32)
    return _cache[key]


def grid_of(name, model_dir, n=N):
    """Interleaved: trajectory i gets rows[i % 6], so every wave holds all six rows (a block-wise grid would hide a lane / row mix-up)."""
    return np.ascontiguousarray(rows_of(name, model_dir)[np.arange(n) % 6])


def oracle_of(name, model_dir, n=N, t=T, seed=SEED, first=FIRST):
    """The oracle's uncor_sample dict for the interleaved grid: row k's run (the model's start = row k) at i = k mod 6.  Left unchanged by
    its users."""
    key = ("oracle", name, n, t, seed, first)
    if key not in _cache:
        _, pp, _ = load_pair(name, model_dir)
        rows = rows_of(name, model_dir)
        per = [O.uncor_sample(O.OracleModel(pp, start=[int(v) for v in row]), n, t, seed, first_index=first) for row in rows]
        if (n, t, seed, first) == (N, T, SEED, FIRST):   # the attempt counter inside the RNG key is exercised under presets
            a4 = per[4]["attempts"]
            assert int((a4 > 1).sum()) == R4_SECOND_ATTEMPTS[name] and a4.max() < 1000, (name, int((a4 > 1).sum()))
        ref = {}
        for f in ("init_bin", "init_val", "attempts", "dense_bin", "dense_val"):
            ref[f] = np.stack([per[i % 6][f][i] for i in range(n)])
        ref["events"] = [per[i % 6]["events"][i] for i in range(n)]
        _cache[key] = ref
    return _cache[key]
