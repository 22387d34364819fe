"""The trajectory-model shapes k_terminal_propagate is tested on (test_terminal_shapes.py without a GPU, test_gpu_terminal_shapes.py
with one): a plain data module like instances.py.

A row is {"id", "spec", "kernel", "covers", "distinct"}:
  spec      util.terminal_model arguments (bins = distance, bearing, heading, altitude, speed); ten files per row
            (util.write_terminal_shape_directory)
  kernel    the instance launch_terminal_propagate must pick: k_terminal_propagate<35,6,4> (36/7/5 bins, the guessed variable order,
            at most 8 cut points in distance, altitude and speed) or k_terminal_propagate (row lengths read from the plan)
  covers    the classes of REQUIRED the row is there for; test_terminal_shapes.py derives each from the generated files and the
            compiled plan (class_holds) -- a row cannot claim a path its models do not take
  distinct  per dynamic variable (heading, altitude, speed) a bound on the largest number of distinct real thresholds of a column, as
            (">=", m) or ("<=", m): "dense" rows must carry more than the six the compact c8 form holds, "sparse" rows at most six

What decides a path in the kernel (emgpu_kernels_term.hip):
  thresholds per row, rm1 = bins - 1     t_draw3: 1-4 one 16-byte load, 5-6 a 16- and an 8-byte load, 7-8 two 16-byte loads (all masked
                                         by q < rm1); 9-48 the compact c8 form, then -- flag byte set: more than six distinct
                                         thresholds -- the pivots and one group of six; 49 and more the binary search
  cut points of distance                 at most 8: squared compare against s_cut8sq; more: sqrt + t_discretize's guess-and-walk
  grids                                  t_discretize / t_bearing_bin guess the bin from the mean spacing and walk: exact on a uniform
                                         grid, several bins off on a non-uniform one
  bearing cut points                     t_bearing_walk stays inside the half [0, 180) / [180, 360) of the position: bear_kA (cut points
                                         below 180) and bear_kB (at or below 180) bound the walk

Out of scope: the folded-stride edge of the launcher (a folded stride of 2^24 or more declines the <35,6,4> instance, whose column
index is built from 24-bit multiply-adds).  It needs a transition table of 16 M columns -- ten files of gigabytes each.
"""
from util import TERMINAL_VARS

SHIPPED = "k_terminal_propagate<35,6,4>"
GENERIC = "k_terminal_propagate"

NONUNIFORM = {n: "nonuniform" for n in TERMINAL_VARS}
# small parent sets for the shapes with many bins: every table stays below 10^5 columns (the ten files of a row are written and parsed
# by every test session)
INTENT_PARENTS = {"heading": ("intent", "bearing"), "altitude": ("intent", "distance", "heading"), "speed": ("distance", "heading")}
FEW_PARENTS = {"heading": ("bearing",), "altitude": ("distance", "heading"), "speed": ("distance", "bearing")}
NO_BEARING_FOR_SPEED = {"heading": ("bearing",), "altitude": ("distance", "heading"), "speed": ("distance", "heading")}


def _row(id_, kernel, covers, distinct, **spec):
    spec.setdefault("bins", (7, 36, 36, 7, 5))
    spec.setdefault("grids", None)
    spec.setdefault("parents", None)
    spec.setdefault("table", "sparse")
    spec.setdefault("zero_frac", 0.02)
    return {"id": id_, "spec": spec, "kernel": kernel, "covers": tuple(covers), "distinct": tuple(distinct)}


ROWS = [
    # the guessed shape itself: the other side of every launcher edge below
    _row("shipped", SHIPPED, ["rm1:altitude:5-6", "rm1:speed:1-4", "long:sparse", "bearing:cut180"], [("<=", 6), ("<=", 6), ("<=", 4)]),
    _row("shipped_intent", SHIPPED, ["graph:intent:36/7/5", "edge:intent"], [("<=", 6), ("<=", 6), ("<=", 4)], parents=INTENT_PARENTS),
    _row("shipped_dense", SHIPPED, ["long:dense", "graph:intent:36/7/5", "grid:nonuniform:heading", "grid:nonuniform:bearing"],
         [(">=", 30), (">=", 6), (">=", 4)], parents=INTENT_PARENTS, table="dense", grids=NONUNIFORM),
    _row("speed6", GENERIC, ["edge:36/7/6", "rm1:speed:5-6"], [("<=", 6), ("<=", 6), ("<=", 5)], bins=(7, 36, 36, 7, 6),
         parents=NO_BEARING_FOR_SPEED),
    _row("shipped_few", SHIPPED, ["edge:36/7/5", "graph:speed_without_bearing"], [("<=", 6), ("<=", 6), ("<=", 4)],
         parents=NO_BEARING_FOR_SPEED),
    _row("dist8", SHIPPED, ["edge:distance8", "cuts:distance:8"], [("<=", 6), ("<=", 6), ("<=", 4)], bins=(9, 36, 36, 7, 5), parents=FEW_PARENTS),
    _row("dist9", GENERIC, ["edge:distance9", "cuts:distance:9"], [("<=", 6), ("<=", 6), ("<=", 4)], bins=(10, 36, 36, 7, 5), parents=FEW_PARENTS),
    # short rows
    _row("tiny", GENERIC, ["rm1:heading:1-4", "rm1:altitude:1-4", "rm1:speed:1-4", "bearing:3bins"], [(">=", 3), (">=", 1), (">=", 1)],
         bins=(2, 3, 4, 2, 2), table="dense"),
    _row("tiny_nonuniform", GENERIC, ["rm1:heading:1-4", "bearing:3bins", "grid:nonuniform:bearing", "graph:intent:other"],
         [(">=", 2), (">=", 2), (">=", 3)], bins=(3, 3, 3, 3, 4), table="dense", grids=NONUNIFORM, parents=INTENT_PARENTS),
    _row("mid", GENERIC, ["rm1:heading:7-8", "rm1:speed:7-8", "rm1:8", "rm1:9", "cuts:distance:8", "cuts:altitude:9", "cuts:speed:8", "long:dense",
                          "grid:nonuniform:distance", "grid:nonuniform:bearing", "grid:nonuniform:heading", "grid:nonuniform:altitude",
                          "grid:nonuniform:speed"],
         [(">=", 8), (">=", 9), (">=", 8)], bins=(9, 12, 9, 10, 9), table="dense", grids=NONUNIFORM),
    _row("mid_sparse", GENERIC, ["rm1:heading:5-6", "rm1:altitude:7-8", "cuts:altitude:8", "cuts:speed:9", "rm1:9", "bearing:4bins", "bearing:cut180",
                                 "long:sparse"],
         [("<=", 6), ("<=", 6), ("<=", 6)], bins=(4, 4, 7, 9, 10)),
    # long rows
    _row("h49", GENERIC, ["rm1:48", "long:dense", "grid:nonuniform:heading"], [(">=", 40), (">=", 6), (">=", 4)], bins=(7, 10, 49, 7, 5), table="dense",
         grids=NONUNIFORM, parents=FEW_PARENTS),
    _row("h50", GENERIC, ["rm1:49", "cuts:distance:9", "graph:intent:other", "grid:nonuniform:distance"], [(">=", 40), (">=", 9), (">=", 9)],
         bins=(10, 13, 50, 12, 11), table="dense", grids=NONUNIFORM, parents=INTENT_PARENTS),
    _row("h64", GENERIC, ["rm1:63", "grid:nonuniform:bearing"], [(">=", 50), (">=", 3), (">=", 5)], bins=(5, 64, 64, 4, 6), table="dense", grids=NONUNIFORM,
         parents=FEW_PARENTS),
    _row("h64_sparse", GENERIC, ["rm1:63"], [("<=", 6), ("<=", 6), ("<=", 6)], bins=(5, 64, 64, 4, 6), parents=FEW_PARENTS),
    # bearing grids: every cut point in one half, and a coarse grid with a cut point on 180 exactly
    _row("bearing_low", GENERIC, ["bearing:cuts_low", "rm1:heading:5-6"], [(">=", 5), (">=", 3), (">=", 2)], bins=(4, 5, 6, 4, 3), table="dense",
         grids={"bearing": [0, 30, 75, 120, 170, 360]}),
    _row("bearing_high", GENERIC, ["bearing:cuts_high", "rm1:heading:5-6"], [(">=", 5), (">=", 3), (">=", 2)], bins=(4, 5, 6, 4, 3), table="dense",
         grids={"bearing": [0, 200, 250, 300, 340, 360]}),
    _row("bearing_4", GENERIC, ["bearing:4bins", "bearing:cut180", "rm1:altitude:7-8", "rm1:8"], [(">=", 4), (">=", 8), (">=", 4)], bins=(5, 4, 5, 9, 5),
         table="dense", grids={"bearing": [0, 90, 180, 270, 360]}),
]

# launcher edges: (what, row on the <35,6,4> side, row on the run-time-shape side or None when both sides stay on <35,6,4>)
EDGES = [
    ("36/7/5 against 36/7/6 bins", "shipped_few", "speed6"),
    ("8 against 9 distance cut points on 36/7/5", "dist8", "dist9"),
    ("36/7/5 on a graph other than the guessed one (intent as a parent)", "shipped_intent", None),
]

REQUIRED = (["rm1:%s:%s" % (v, c) for v in ("heading", "altitude", "speed") for c in ("1-4", "5-6", "7-8")] +
            ["rm1:8", "rm1:9", "rm1:48", "rm1:49", "rm1:63", "long:sparse", "long:dense"] +
            ["cuts:%s:%d" % (v, c) for v in ("distance", "altitude", "speed") for c in (8, 9)] +
            ["grid:nonuniform:%s" % v for v in TERMINAL_VARS] +
            ["bearing:3bins", "bearing:4bins", "bearing:cut180", "bearing:cuts_low", "bearing:cuts_high"] +
            ["graph:intent:36/7/5", "graph:intent:other", "graph:speed_without_bearing"] +
            ["edge:36/7/5", "edge:36/7/6", "edge:distance8", "edge:distance9", "edge:intent"])


def by_id(id_):
    return next(r for r in ROWS if r["id"] == id_)
