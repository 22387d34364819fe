"""CPU: the pairs of equal_draw_cases.py are what they are made to be.  The plan compiler turns the rewritten tables and rates into exactly the
wanted words (X_t = x in model "at", x + 1 in model "above"; R = x + 1 and R = x); the oracle's two runs are equal in every other
trajectory and, in trajectory i0, up to the target, where they differ as predicted (bin t + 2 against bin t + 1; resampled against not); and
the call lands on the kernel the case names."""
import ctypes as C

import numpy as np
import pytest

import equal_draw_cases as E
from em_model_manned_bayes_amd import _lib as L
from test_dispatch import predict


def _thresholds_of(weights):
    out = np.zeros(len(weights) - 1, dtype=np.uint32)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    L.check(L.lib().emgpu_debug_column_thresholds(w.ctypes.data, len(w), out.ctypes.data))
    return [int(v) for v in out]


@pytest.mark.parametrize("name", E.NAMES)
def test_the_plan_holds_exactly_the_wanted_words(name, model_dir):
    b = E.build(name, model_dir)
    assert b["i0"] >= 64 and (b["kind"] == "init" or 1 <= b["c"] < b["T"])
    for which in ("at", "above"):
        nm, pp, q = b[which]
        if b["kind"] in ("trans", "init"):
            th = b["thr_" + which]
            assert th[b["t"]] == b["x"] + (which == "above") and all(abs(t - b["x"]) > 2**24 for j, t in enumerate(th) if j != b["t"])
            table = q["N_transition"][b["tvar"]] if b["kind"] == "trans" else q["N_initial"][b["var"]]
            assert _thresholds_of(table[:, 0])[: len(th)] == th
        if b["kind"] == "trans":
            k = E.CASES[name]["k"]
            tvar, r, ncol, meff, mp = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_uint32()
            thr, cthr = np.zeros(64, dtype=np.uint32), np.zeros(7, dtype=np.uint32)
            for col in (0, table.shape[1] - 1):
                L.check(L.lib().emgpu_debug_dynamic_column(nm._h, k, col, C.byref(tvar), C.byref(r), C.byref(ncol), thr.ctypes.data, C.byref(meff),
                                                           cthr.ctypes.data, C.byref(mp)))
                assert tvar.value - 1 == b["tvar"] and ncol.value == table.shape[1]
                assert [int(v) for v in thr[: len(th)]] == th
                real = [t for t in th if t < 0xFFFFFFFF]                 # (2^32 - 1 is "never": no compare slot)
                assert meff.value == len(real) <= b["meff"] and [int(v) for v in cthr[: len(real)]] == real
        if b["kind"] in ("res", "res_static"):
            assert int(L.lib().emgpu_debug_bernoulli_threshold(float(pp["resample_rates"][b["var"]]))) == b["R_" + which]
            assert b["R_at"] == b["x"] + 1 and b["R_above"] == b["x"]


@pytest.mark.parametrize("name", E.NAMES)
def test_the_kernel_chosen_is_the_intended_one(name, model_dir):
    case, b = E.CASES[name], E.build(name, model_dir)
    if case["form"] == "bn":
        return                                  # (emgpu_sample_bn_host has one launcher: the GPU test asserts the name)
    for which in ("at", "above"):
        assert predict(b[which][0], "dense" if case["form"] == "start" else case["form"], grid=case["form"] == "start") == case["kernel"]


@pytest.mark.parametrize("name", E.NAMES)
def test_the_two_oracle_runs_part_at_the_target(name, model_dir):
    case, b = E.CASES[name], E.build(name, model_dir)
    at, above = E.oracle_run(name, "at", model_dir), E.oracle_run(name, "above", model_dir)
    i0, c = b["i0"], b["c"]
    others = np.arange(E.N) != i0
    if case["form"] == "bn":
        assert all(np.array_equal(x[others], y[others]) for x, y in zip(at, above))
        assert at[0][i0, b["var"]] == b["want_at"] and above[0][i0, b["var"]] == b["want_above"]
        return
    assert at["attempts"][i0] == 1 and above["attempts"][i0] == 1
    for f in ("init_bin", "init_val", "attempts", "dense_bin", "dense_val"):
        assert np.array_equal(at[f][others], above[f][others]), f
    assert all(np.array_equal(x, y) for i, (x, y) in enumerate(zip(at["events"], above["events"])) if i != i0)
    if b["kind"] == "init":
        assert at["init_bin"][i0, b["var"]] == b["want_at"] and above["init_bin"][i0, b["var"]] == b["want_above"]
        return
    assert np.array_equal(at["init_bin"][i0], above["init_bin"][i0]) and np.array_equal(at["init_val"][i0], above["init_val"][i0])
    assert np.array_equal(at["dense_bin"][i0, :c], above["dense_bin"][i0, :c]) and np.array_equal(at["dense_val"][i0, :c], above["dense_val"][i0, :c])
    if b["kind"] == "trans":
        assert at["dense_bin"][i0, c, b["slot"]] == b["want_at"] and above["dense_bin"][i0, c, b["slot"]] == b["want_above"]
        return
    # a Bernoulli: the bins stay, model "at" has one row more -- the variable resampled at second c
    assert np.array_equal(at["dense_bin"][i0], above["dense_bin"][i0])
    ea, eb = at["events"][i0], above["events"][i0]
    mine_a, mine_b = ea[:, 1] == b["var"] + 1, eb[:, 1] == b["var"] + 1
    assert len(ea) == len(eb) + 1 and mine_a.sum() == mine_b.sum() + 1, (len(ea), len(eb))
    assert np.array_equal(ea[~mine_a][:, 1:], eb[~mine_b][:, 1:])                  # the other variables' rows: variable, value, bin
    extra = [j for j in np.flatnonzero(mine_a) if np.array_equal(np.delete(ea, j, axis=0)[:, 1:], eb[:, 1:])]
    assert extra, "model 'at' has no single row more"
    if b["kind"] == "res":
        assert at["dense_val"][i0, c, b["slot"]] != above["dense_val"][i0, c, b["slot"]]
