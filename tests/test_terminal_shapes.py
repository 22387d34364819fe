"""CPU: the shape table of the terminal propagation (terminal_shapes.py) -- every row's ten files compile to the class the row claims,
the rows together cover every class the kernel's shortcuts distinguish, and the oracle finishes every row with tracks of every length.
A failure in test_gpu_terminal_shapes.py then cannot come from a misbuilt model or from tracks that all end at once."""
import numpy as np
import pytest

import oracle as O
import terminal_shapes as S
from em_model_manned_bayes_amd import native
from util import (TERMINAL_LIMITS, TERMINAL_VARS, plan_facts, terminal_hand_geo, terminal_hand_limits, terminal_model, terminal_shape_models, terminal_test_geo,
                  write_terminal_shape_directory)

DYN = ("heading", "altitude", "speed")
RANGES = {"1-4": (1, 4), "5-6": (5, 6), "7-8": (7, 8)}


@pytest.fixture(scope="module")
def shape_dirs(tmp_path_factory):
    """id -> directory of the row's ten files, written once per module."""
    made = {}

    def get(row):
        if row["id"] not in made:
            made[row["id"]] = write_terminal_shape_directory(str(tmp_path_factory.mktemp("shape_" + row["id"])), **row["spec"])
        return made[row["id"]]
    return get


def class_holds(tag, row, facts, pp):
    """Is class `tag` true of a row's model?  facts: util.plan_facts of the compiled plan; pp: the parsed file."""
    part = tag.split(":")
    r = tuple(facts["r"])                      # bins of heading, altitude, speed as the plan has them
    rm1 = [x - 1 for x in r]
    cuts = {n: np.asarray(pp["boundaries"][1 + v], dtype=np.float64)[1:-1] for v, n in enumerate(TERMINAL_VARS)}
    G = np.asarray(pp["G_transition"], dtype=bool)
    hi = [c[1] for c in facts["col_meff"]]
    if part[0] == "rm1" and len(part) == 3:
        lo_, hi_ = RANGES[part[2]]
        return lo_ <= rm1[DYN.index(part[1])] <= hi_
    if part[0] == "rm1":
        return int(part[1]) in rm1
    if tag == "long:sparse":
        return any(9 <= m <= 48 and h <= 6 for m, h in zip(rm1, hi))
    if tag == "long:dense":
        return any(9 <= m <= 48 and h > 6 for m, h in zip(rm1, hi))
    if part[0] == "cuts":
        return len(cuts[part[1]]) == int(part[2])
    if part[0] == "grid":
        b = np.asarray(pp["boundaries"][1 + TERMINAL_VARS.index(part[2])], dtype=np.float64)
        return len(b) > 2 and np.ptp(np.diff(b)) > 0.2 * np.diff(b).mean()
    if tag in ("bearing:3bins", "bearing:4bins"):
        return len(cuts["bearing"]) + 1 == int(part[1][0])
    if tag == "bearing:cut180":
        return 180.0 in cuts["bearing"]
    if tag == "bearing:cuts_low":
        return bool(np.all(cuts["bearing"] < 180.0))
    if tag == "bearing:cuts_high":
        return bool(np.all(cuts["bearing"] > 180.0))
    intent_parent = bool(G[0, 6] and G[0, 7])
    if tag == "graph:intent:36/7/5":
        return intent_parent and r == (36, 7, 5)
    if tag == "graph:intent:other":
        return intent_parent and r != (36, 7, 5)
    if tag == "graph:speed_without_bearing":
        return not G[2, 8]
    few_cuts = all(len(cuts[n]) <= 8 for n in ("distance", "altitude", "speed"))
    if tag == "edge:36/7/5":
        return r == (36, 7, 5) and few_cuts and row["kernel"] == S.SHIPPED
    if tag == "edge:36/7/6":
        return r == (36, 7, 6) and few_cuts and row["kernel"] == S.GENERIC
    if tag == "edge:distance8":
        return r == (36, 7, 5) and len(cuts["distance"]) == 8 and row["kernel"] == S.SHIPPED
    if tag == "edge:distance9":
        return r == (36, 7, 5) and len(cuts["distance"]) == 9 and row["kernel"] == S.GENERIC
    if tag == "edge:intent":
        return r == (36, 7, 5) and few_cuts and intent_parent and row["kernel"] == S.SHIPPED
    raise KeyError(tag)


@pytest.mark.parametrize("row", S.ROWS, ids=lambda r: r["id"])
def test_rows_compile_to_the_classes_they_claim(row, shape_dirs):
    """Through plan_facts (emgpu_debug_dynamic_column over every column, with the stay prior the propagation runs with): all ten files
    have the row's bins, the largest number of distinct thresholds per column is on the side of six the row says, and every class in
    `covers` holds -- for the forward ownship model and the reverse intruder model (2 and 3 intents)."""
    nms, _, files = terminal_shape_models(shape_dirs(row))
    bins = row["spec"]["bins"]
    for k in (0, 9):
        pp = O.parse_model_txt(files[k])
        f = plan_facts(nms[k])
        assert tuple(f["r"]) == tuple(bins[2:]), f
        assert [len(b) - 1 for b in pp["boundaries"][1:]] == list(bins)
        for (op, m), (_, most), name in zip(row["distinct"], f["col_meff"], DYN):
            assert (most >= m) if op == ">=" else (most <= m), (row["id"], name, f["col_meff"], row["distinct"])
        for tag in row["covers"]:
            assert class_holds(tag, row, f, pp), (row["id"], tag, f)
        hand = terminal_hand_geo(160)[0].reshape(-1, 6)           # hand-made altitudes and speeds lie off every cut point of the row
        for column, v in ((2, 4), (3, 5)):
            cuts = np.asarray(pp["boundaries"][v], dtype=np.float64)
            assert np.abs(hand[:, column][:, None] - cuts[None, :]).min() > 0.05, (row["id"], v)
    for nm in nms[1:]:                        # one shape, one set of boundaries: what the library asks of the ten
        assert [nm.n_initial, nm.n_dyn] == [6, 3]
    first = O.parse_model_txt(files[0])["boundaries"]
    for f_ in files[1:]:
        other = O.parse_model_txt(f_)["boundaries"]
        assert all(np.array_equal(a, b) for a, b in zip(first, other))


def test_the_rows_cover_every_class():
    covered = {t for r in S.ROWS for t in r["covers"]}
    missing = [t for t in S.REQUIRED if t not in covered]
    assert not missing, "classes without a row in tests/terminal_shapes.py: %s" % missing
    assert len({r["id"] for r in S.ROWS}) == len(S.ROWS)
    for r in S.ROWS:
        assert r["kernel"] in (S.SHIPPED, S.GENERIC) and r["covers"], r["id"]
        unknown = [t for t in r["covers"] if t not in S.REQUIRED]
        assert not unknown, (r["id"], unknown)
    # ... and the check itself: without the only row of a class, that class is reported
    only = [t for t in S.REQUIRED if sum(t in r["covers"] for r in S.ROWS) == 1]
    assert "rm1:49" in only and "bearing:cuts_low" in only


def test_the_edge_pairs_differ_in_one_argument():
    """Both sides of a launcher edge are one model with one bin count changed: the same graph, grids elsewhere and table kind."""
    for what, lo, hi in S.EDGES:
        a = S.by_id(lo)
        assert a["kernel"] == S.SHIPPED, what
        if hi is None:
            assert a["spec"]["parents"] is not None, what
            continue
        b = S.by_id(hi)
        assert b["kernel"] == S.GENERIC, what
        assert {k for k in a["spec"] if a["spec"][k] != b["spec"][k]} == {"bins"}, what
        assert sum(x != y for x, y in zip(a["spec"]["bins"], b["spec"]["bins"])) == 1, what
        A, B = terminal_model(5, **a["spec"]), terminal_model(5, **b["spec"])
        assert np.array_equal(A["G_transition"], B["G_transition"])
        for v in range(6):
            if A["r_initial"][v] == B["r_initial"][v]:
                assert np.array_equal(A["boundaries"][v], B["boundaries"][v]), (what, v)


def track_spread(rows, tmax_s=120):
    return int(rows.min()), int(rows.max()), float(rows.mean())


@pytest.mark.parametrize("row", S.ROWS, ids=lambda r: r["id"])
def test_the_oracle_finishes_every_row_with_tracks_of_every_length(row, shape_dirs, model_dir):
    """oracle.propagate returns 0 at max_resample = 100000 under both limit pairs (the hand-made half with its own turn limits,
    util.TERMINAL_HAND_TURN); some track ends within 3 rows, some runs the full
    tmax_s + 1, the mean lies between 40 and 110 rows -- a row cannot pass on tracks that all end at once."""
    _, oms, _ = terminal_shape_models(shape_dirs(row), native_too=False)
    geo, mo = terminal_test_geo(model_dir, 400)
    for name, dl in TERMINAL_LIMITS.items():
        _, rows_s = O.propagate(oms, mo[:200], geo[:200], 0x5EED0013, dl, tmax_s=120.0, max_resample=100000)
        _, rows_h = O.propagate(oms, mo[200:], geo[200:], 0x5EED0013, terminal_hand_limits(name), first_index=200, tmax_s=120.0, max_resample=100000)
        for half, rows in (("sampled", rows_s), ("hand-made", rows_h), ("both", np.concatenate([rows_s, rows_h]))):
            lo, hi, mean = track_spread(rows)
            print("%s / %s / %s: rows %d .. %d, mean %.1f" % (row["id"], name, half, lo, hi, mean))
            if half == "both":
                assert lo <= 3 and hi == 121 and 40 <= mean <= 110, (row["id"], name, lo, hi, mean)


def test_a_parent_above_the_own_variable_never_finishes(tmp_path, model_dir):
    """The generator's own-value-last rule: with speed as a parent of altitude(t+1) the own value is no longer the slowest-varying parent,
    setTransitionPriors.m:20-27 puts the stay prior on other bins, an all-zero column then allows only a bin above maxAltitude, and the
    re-draw loop of createEncounter.m:192 does not end: the oracle gives up at max_resample (-3).  terminal_model refuses such a graph
    unless told otherwise."""
    spec = dict(bins=(4, 5, 6, 8, 4), table="dense", zero_frac=0.1, parents={"altitude": ("distance", "heading", "speed")})
    with pytest.raises(AssertionError, match="comes after the node's own variable"):
        terminal_model(1, **spec)
    d = write_terminal_shape_directory(str(tmp_path / "bad"), unordered_parents=True, **spec)
    _, oms, _ = terminal_shape_models(d, native_too=False)
    geo, mo = terminal_test_geo(model_dir, 400)
    with pytest.raises(RuntimeError, match="rc=-3"):
        O.propagate(oms, mo, geo, 0x5EED0013, TERMINAL_LIMITS["inside"], tmax_s=120.0, max_resample=200)
    # the same shape with the rule kept finishes
    d = write_terminal_shape_directory(str(tmp_path / "good"), **dict(spec, parents={"altitude": ("distance", "heading")}))
    _, oms, _ = terminal_shape_models(d, native_too=False)
    O.propagate(oms, mo, geo, 0x5EED0013, TERMINAL_LIMITS["inside"], tmax_s=120.0, max_resample=200)


def test_the_hand_made_geometry_sits_on_the_axes(model_dir):
    geo, mo = terminal_test_geo(model_dir, 400)
    hand = geo[200:].reshape(-1, 6)
    assert np.all((hand[:, 0] == 0) | (hand[:, 1] == 0)) and np.all(np.isin(hand[:, 4], (0.0, 90.0, 180.0, 270.0)))
    d = np.hypot(hand[:, 0], hand[:, 1])
    assert d.min() == 0.26 and d.max() == 6.5
    along = np.where(hand[:, 1] == 0, np.isin(hand[:, 4], (0.0, 180.0)), np.isin(hand[:, 4], (90.0, 270.0)))
    assert along.all()
    for q in range(4):                                   # each axis, towards and away
        ux, uy = ((1, 0), (0, 1), (-1, 0), (0, -1))[q]
        on = (np.sign(hand[:, 0]) == ux) & (np.sign(hand[:, 1]) == uy)
        assert set(hand[on, 4]) == {90.0 * q, (90.0 * q + 180.0) % 360.0}
    assert mo.min() == 0 and mo.max() == 9 and native is not None
