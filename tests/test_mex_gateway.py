"""The MATLAB gateway (em_model_manned_bayes_amd/matlab/emgpu_mex.c), EXECUTED: compiled against the working mex runtime of
tests/stubs/mex_runtime.c and driven through tests/mexrt.py.  This module holds what needs no device: the model commands, the
usage / error table of every command, and the structural checks that tie gateway, header comment, usage strings and the shipped .m
call sites together.  The sampling commands are in tests/test_gpu_mex_gateway.py."""
import os
import re

import numpy as np
import pytest

import mexrt
import oracle as O
import util
from em_model_manned_bayes_amd import _lib as L
from em_model_manned_bayes_amd import em_io, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATLAB_DIR = os.path.join(ROOT, "em_model_manned_bayes_amd", "matlab")
ALL_MODELS = sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(ROOT, "models")) if f.endswith(".npz"))
ZERO_SETTINGS = [(), (np.array([1.0, 2.0, 3.0]), True), (np.array([2.0]), False)]     # (idxZeroBoundaries, isOverwriteZeroBoundaries)


@pytest.fixture(scope="module")
def gw(tmp_path_factory):
    g = mexrt.build(tmp_path_factory.mktemp("mex"))
    yield g
    g.run_at_exit()
    g.check("module teardown")


class Borrowed(native.NativeModel):
    """NativeModel's getters on a handle the gateway owns (freed through emgpu_mex('free'), not here)."""

    def __del__(self):
        pass


def borrowed(h):
    return Borrowed(mexrt.handle(h))


def model_fields(m):
    """Everything emgpu_model_get_i32 / get_f64 / get_text hand out about a model, as comparable Python values."""
    info = (m.n_initial, m.n_transition, m.n_dyn, m.is_dynvar_depend)
    ints = {f: m.get_i32(f).tolist() for f in (L.F_R_INITIAL, L.F_R_TRANSITION, L.F_ORDER_INITIAL, L.F_ORDER_TRANSITION, L.F_TEMPORAL_MAP,
                                               L.F_ZERO_BINS, L.F_START, L.F_G_INITIAL, L.F_G_TRANSITION)}
    tabs = {}
    for v in range(1, m.n_initial + 1):
        for tag, f in (("Ni", L.F_N_INITIAL), ("Ai", L.F_ALPHA_INITIAL), ("b", L.F_BOUNDARIES)):
            tabs[(tag, v)] = m.get_f64(f, v).tobytes()
    for v in range(m.n_initial + 1, m.n_transition + 1):
        for tag, f in (("Nt", L.F_N_TRANSITION), ("At", L.F_ALPHA_TRANSITION)):
            tabs[(tag, v)] = m.get_f64(f, v).tobytes()
    return info, ints, tabs, m.get_f64(L.F_RESAMPLE_RATES).tobytes(), m.get_labels(L.F_LABELS_INITIAL), m.get_labels(L.F_LABELS_TRANSITION)


def assert_same_model(a, b):
    fa, fb = model_fields(a), model_fields(b)
    for x, y, what in zip(fa, fb, ("info", "integer fields", "tables", "resample rates", "labels_initial", "labels_transition")):
        assert x == y, what
    assert util.plan_facts(a) == util.plan_facts(b)


def raises(gw, identifier, cmd, *args, **kw):
    with pytest.raises(mexrt.MexError) as ei:
        gw.call(cmd, *args, **kw)
    assert ei.value.identifier == identifier, str(ei.value)
    return ei.value


def py_zero_args(setting):
    return () if not setting else (tuple(int(x) for x in setting[0]), setting[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# em_read: values against two independent readers, MATLAB shape and class against em_read.m

# field -> (class, dims) of the struct em_read.m:70-141 returns; ni, nt, nd = n_initial, n_transition, rows of temporal_map.
# class: "double", "logical", "cell".  Written from the reference function: textscan's x{1} is a column (r_*, resample_rates, each
# boundaries{j}); strsplit gives a row cell (labels_*); bn_sort returns a row (order_*); array2cells preallocates cell(n, 1)
# (N_*, with N_transition's first n_initial cells left empty); cell(1, n_initial) for boundaries, zero_bins, cutpoints_initial;
# zeros(n_initial, 2) for bounds_initial; temporal_map one row per dynamic variable.
EM_READ_SHAPES = {
    "labels_initial": ("cell", lambda ni, nt, nd: (1, ni)), "n_initial": ("double", lambda ni, nt, nd: (1, 1)),
    "G_initial": ("logical", lambda ni, nt, nd: (ni, ni)), "order_initial": ("double", lambda ni, nt, nd: (1, ni)),
    "r_initial": ("double", lambda ni, nt, nd: (ni, 1)), "N_initial": ("cell", lambda ni, nt, nd: (ni, 1)),
    "boundaries": ("cell", lambda ni, nt, nd: (1, ni)), "resample_rates": ("double", lambda ni, nt, nd: (ni, 1)),
    "zero_bins": ("cell", lambda ni, nt, nd: (1, ni)), "bounds_initial": ("double", lambda ni, nt, nd: (ni, 2)),
    "cutpoints_initial": ("cell", lambda ni, nt, nd: (1, ni)),
}
EM_READ_SHAPES_TRANSITION = {
    "labels_transition": ("cell", lambda ni, nt, nd: (1, nt)), "n_transition": ("double", lambda ni, nt, nd: (1, 1)),
    "G_transition": ("logical", lambda ni, nt, nd: (nt, nt)), "order_transition": ("double", lambda ni, nt, nd: (1, nt)),
    "r_transition": ("double", lambda ni, nt, nd: (nt, 1)), "N_transition": ("cell", lambda ni, nt, nd: (nt, 1)),
    "temporal_map": ("double", lambda ni, nt, nd: (nd, 2)),
}
_NUMPY_CLASS = {"double": np.float64, "logical": np.bool_, "cell": object}


def check_em_read_struct(s, q, p):
    """s: the gateway's struct; q: oracle.parse_model_txt of the same file and settings; p: em_io.em_read of them."""
    ni, nt = q["n_initial"], q["n_transition"]
    nd = q["temporal_map"].shape[0]
    table = dict(EM_READ_SHAPES)
    if nt:
        table.update(EM_READ_SHAPES_TRANSITION)
    else:
        for f in EM_READ_SHAPES_TRANSITION:
            assert s[f] is None, f                      # the reference never assigns them for a model without a transition network
    assert set(s) == set(EM_READ_SHAPES) | set(EM_READ_SHAPES_TRANSITION)
    for f, (cls, dims) in table.items():
        assert isinstance(s[f], np.ndarray) and s[f].dtype == _NUMPY_CLASS[cls], (f, type(s[f]))
        assert s[f].shape == dims(ni, nt, nd), (f, s[f].shape)
    assert s["n_initial"][0, 0] == ni == p["n_initial"]
    assert s["labels_initial"][0].tolist() == q["labels_initial"] == p["labels_initial"]
    for G, o, r, N, n, first in (("G_initial", "order_initial", "r_initial", "N_initial", ni, 0),) + \
            ((("G_transition", "order_transition", "r_transition", "N_transition", nt, ni),) if nt else ()):
        assert np.array_equal(s[G], q[G]) and np.array_equal(s[G], p[G])                       # (parent, child), not its transpose
        assert np.array_equal(s[o][0], q[o]) and np.array_equal(s[o][0], p[o])
        assert np.array_equal(s[r][:, 0], q[r]) and np.array_equal(s[r][:, 0], p[r])
        for v in range(n):
            c = s[N][v, 0]
            if v < first:
                assert c is None                                                                # em_read.m:92: cells 1..n_initial stay empty
                continue
            assert c.dtype == np.float64 and c.shape == q[N][v].shape and np.array_equal(c, q[N][v]) and np.array_equal(c, p[N][v]), (N, v)
    if nt:
        assert s["n_transition"][0, 0] == nt and s["labels_transition"][0].tolist() == q["labels_transition"] == p["labels_transition"]
        assert np.array_equal(s["temporal_map"], q["temporal_map"]) and np.array_equal(s["temporal_map"], p["temporal_map"])
    assert np.array_equal(s["resample_rates"][:, 0], q["resample_rates"]) and np.array_equal(s["resample_rates"][:, 0], p["resample_rates"])
    for v in range(ni):
        b, z, c = s["boundaries"][0, v], s["zero_bins"][0, v], s["cutpoints_initial"][0, v]
        qb = q["boundaries"][v]
        assert b.dtype == np.float64 and b.shape == (len(qb), 1), (v, b.shape)                 # a column, double.empty(0, 1) when there is none
        assert np.array_equal(b[:, 0], qb) and np.array_equal(b[:, 0], p["boundaries"][v])
        qz = int(q["zero_bins"][v])
        assert z.shape == ((1, 1) if qz else (0, 0)) and (not qz or z[0, 0] == qz)
        assert (p["zero_bins"][v] or 0) == qz
        if len(qb):
            want_c, want_bounds = qb[1:-1], [qb.min(), qb.max()]
        else:
            want_c, want_bounds = np.arange(2, int(q["r_initial"][v]) + 1, dtype=np.float64), [0.0, 0.0]
        assert c.shape == (1, len(want_c)) and np.array_equal(c[0], want_c) and np.array_equal(c[0], p["cutpoints_initial"][v]), v
        assert s["bounds_initial"][v].tolist() == want_bounds == p["bounds_initial"][v].tolist()


@pytest.mark.parametrize("name", ALL_MODELS)
def test_em_read_struct_equals_both_readers_in_value_shape_and_class(gw, name, model_dir):
    path = em_io.materialize_model(name, model_dir)
    for setting in ZERO_SETTINGS:
        if name in ("balloon_v1", "weatherballoon_v1") and setting and len(setting[0]) == 3:   # two variables: index 3 does not exist
            raises(gw, "emgpu:arg", "em_read", path, *setting)
            with pytest.raises(L.EmgpuError) as ei:
                em_io.em_read(path, *py_zero_args(setting))
            assert ei.value.code == L.ERR_ARG
            continue
        s = gw.call("em_read", path, *setting)
        check_em_read_struct(s, O.parse_model_txt(path, *py_zero_args(setting)), em_io.em_read(path, *py_zero_args(setting)))


def test_em_read_of_short_boundary_lines(gw, tmp_path):
    """A boundary line with one or two numbers has no cut points: (2:end-1)' is 1 x 0, not a wrapped-around size."""
    f = tmp_path / "short_boundaries.txt"
    f.write_text("# labels_initial\n\"a\", \"b\" \n# G_initial\n0 0 \n0 0 \n# r_initial\n2 2 \n# N_initial\n1 2 3 4 \n# boundaries\n5 \n1 2 \n"
                 "# resample_rates\n0 0 \n")
    s = gw.call("em_read", str(f))
    assert [c.shape for c in s["cutpoints_initial"][0]] == [(1, 0), (1, 0)]
    assert s["bounds_initial"].tolist() == [[5.0, 5.0], [1.0, 2.0]] and [b.shape for b in s["boundaries"][0]] == [(1, 1), (2, 1)]


# ---------------------------------------------------------------------------------------------------------------------------------
# from_struct

@pytest.mark.parametrize("name", ALL_MODELS)
def test_from_struct_of_the_em_read_struct_equals_load_txt(gw, name, model_dir, tmp_path):
    path = em_io.materialize_model(name, model_dir)
    s = gw.call("em_read", path)
    h_txt, h_struct = gw.call("load_txt", path), gw.call("from_struct", s)
    a, b = borrowed(h_txt), borrowed(h_struct)
    assert_same_model(a, b)
    assert b.get_labels(L.F_LABELS_INITIAL) == O.parse_model_txt(path)["labels_initial"]     # the labels cross the struct too
    # with the labels passed across, the binary caches of the two are the same bytes
    gw.call("save_bin", h_txt, str(tmp_path / "txt.bin"), nlhs=0)
    gw.call("save_bin", h_struct, str(tmp_path / "struct.bin"), nlhs=0)
    assert (tmp_path / "txt.bin").read_bytes() == (tmp_path / "struct.bin").read_bytes()
    # G as double (what struct(EncounterModel) can hold) instead of logical
    d = dict(s)
    d["G_initial"] = s["G_initial"].astype(np.float64)
    if s["G_transition"] is not None:
        d["G_transition"] = s["G_transition"].astype(np.float64)
    h_double = gw.call("from_struct", d)
    assert_same_model(a, borrowed(h_double))
    for h in (h_txt, h_struct, h_double):
        gw.call("free", h, nlhs=0)


def test_from_struct_start_edits_and_missing_labels(gw, model_dir):
    path = em_io.materialize_model("uncor_1200code_v2p1", model_dir)
    s = gw.call("em_read", path)
    ni = int(s["n_initial"][0, 0])
    # start: [] and NaN are unset, a number is a bin (bn_sample.m:44-50)
    d = dict(s)
    d["start"] = [2.0, np.zeros((0, 0)), float("nan"), None, 3.0, np.zeros((0, 0)), None]
    h = gw.call("from_struct", d)
    assert borrowed(h).get_i32(L.F_START).tolist() == [2, 0, 0, 0, 3, 0, 0]
    gw.call("free", h, nlhs=0)
    # an edited table and an edited boundary vector reach the native model: what from_struct exists for
    d = dict(s)
    N = s["N_initial"].copy()
    N[1, 0] = s["N_initial"][1, 0].copy()
    N[1, 0][:, 2] = [7.0, 0.0, 11.0, 13.0][: N[1, 0].shape[0]]
    B = s["boundaries"].copy()
    B[0, 3] = s["boundaries"][0, 3] + 0.25
    d["N_initial"], d["boundaries"] = N, B
    h = gw.call("from_struct", d)
    m = borrowed(h)
    r = int(s["r_initial"][1, 0])
    got = m.get_f64(L.F_N_INITIAL, 2).reshape(-1, r).T
    assert np.array_equal(got, N[1, 0]) and not np.array_equal(got, s["N_initial"][1, 0])
    assert np.array_equal(m.get_f64(L.F_BOUNDARIES, 4), B[0, 3][:, 0])
    for v in range(ni):
        if v != 1:
            assert np.array_equal(m.get_f64(L.F_N_INITIAL, v + 1).reshape(-1, int(s["r_initial"][v, 0])).T, s["N_initial"][v, 0])
    gw.call("free", h, nlhs=0)
    # a struct without labels is still a model
    d = {k: v for k, v in s.items() if not k.startswith("labels_")}
    h = gw.call("from_struct", d)
    m = borrowed(h)
    assert m.n_initial == ni and np.array_equal(m.get_f64(L.F_N_INITIAL, 2).reshape(-1, r).T, s["N_initial"][1, 0])
    gw.call("free", h, nlhs=0)
    # shape checks of its own
    raises(gw, "emgpu:usage", "from_struct", 3.0)
    raises(gw, "emgpu:usage", "from_struct", {"G_initial": s["G_initial"]})
    short = dict(s)
    short["N_initial"] = s["N_initial"][:3]
    raises(gw, "emgpu:usage", "from_struct", short)                       # fewer cells than variables: refused, not read past the end
    short = dict(s)
    short["r_transition"] = s["r_transition"][:4]
    raises(gw, "emgpu:usage", "from_struct", short)
    bad = dict(s)
    bad["labels_initial"] = [1.0, 2.0]
    raises(gw, "emgpu:usage", "from_struct", bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# set_prior, set_alpha, set_start, save_bin / load_bin, free

def test_set_prior(gw, model_dir):
    path = em_io.materialize_model("uncor_1200code_v2p1", model_dir)
    h = gw.call("load_txt", path)
    m = borrowed(h)
    ref = native.NativeModel.load_txt(path)
    for prior in ("dbe", "DBE", 0.5, "dbe", 2.0):
        gw.call("set_prior", h, prior, nlhs=0)
        ref.set_prior(prior)
        for v in range(1, m.n_initial + 1):
            assert np.array_equal(m.get_f64(L.F_ALPHA_INITIAL, v), ref.get_f64(L.F_ALPHA_INITIAL, v))
        for v in range(m.n_initial + 1, m.n_transition + 1):
            assert np.array_equal(m.get_f64(L.F_ALPHA_TRANSITION, v), ref.get_f64(L.F_ALPHA_TRANSITION, v))
    assert np.all(m.get_f64(L.F_ALPHA_INITIAL, 1) == 2.0)
    gw.call("set_prior", h, "dbe", nlhs=0)
    assert np.all(m.get_f64(L.F_ALPHA_TRANSITION, 8) == 1.0 / 39200)                     # 5 x 7840 node (bn_dirichlet_prior.m:30-34)
    e = raises(gw, "prior:notdbe", "set_prior", h, "xyz")                                 # bn_dirichlet_prior.m:28
    assert "xyz" in e.message
    raises(gw, "prior:unknown", "set_prior", h, [1.0])                                    # bn_dirichlet_prior.m:37
    assert np.all(m.get_f64(L.F_ALPHA_TRANSITION, 8) == 1.0 / 39200)                     # the failed calls changed nothing
    gw.call("free", h, nlhs=0)


def test_set_alpha(gw, model_dir):
    path = em_io.materialize_model("glider_v1", model_dir)
    h = gw.call("load_txt", path)
    m = borrowed(h)
    ni, nt = m.n_initial, m.n_transition
    rs = np.random.RandomState(5)
    s = gw.call("em_read", path)

    def table(N):
        return np.asfortranarray(rs.randint(0, 9, N.shape).astype(np.float64))
    full_i = [table(s["N_initial"][v, 0]) for v in range(ni)]
    full_t = [None] * ni + [table(s["N_transition"][v, 0]) for v in range(ni, nt)]
    gw.call("set_alpha", h, full_i, full_t, nlhs=0)

    def alpha(v, transition=False):
        r = int((s["r_transition"] if transition else s["r_initial"])[v, 0])
        return m.get_f64(L.F_ALPHA_TRANSITION if transition else L.F_ALPHA_INITIAL, v + 1).reshape(-1, r).T
    for v in range(ni):
        assert np.array_equal(alpha(v), full_i[v]), v
    for v in range(ni, nt):
        assert np.array_equal(alpha(v, True), full_t[v]), v
    # cells holding [] leave their node alone; {} for the transition leaves every transition node alone (bn_sample's shadow passes it)
    part = [None, np.zeros((0, 0)), table(s["N_initial"][2, 0])] + [None] * (ni - 3)
    gw.call("set_alpha", h, part, [], nlhs=0)
    for v in range(ni):
        assert np.array_equal(alpha(v), part[2] if v == 2 else full_i[v]), v
    for v in range(ni, nt):
        assert np.array_equal(alpha(v, True), full_t[v]), v
    gw.call("set_alpha", h, [], nlhs=0)                                                  # the minimum: nothing to set
    wrong = [np.ones((1, 1))] + [None] * (ni - 1)
    with pytest.raises(mexrt.MexError):
        gw.call("set_alpha", h, wrong, [], nlhs=0)                                        # a table of the wrong size is the library's error
    assert np.array_equal(alpha(0), full_i[0])
    gw.call("free", h, nlhs=0)


def test_set_start(gw, model_dir):
    path = em_io.materialize_model("uncor_1200code_v2p1", model_dir)
    h = gw.call("load_txt", path)
    m = borrowed(h)
    gw.call("set_start", h, np.array([1.0, 4.0, 2.0, float("nan"), 0.0, float("nan"), 0.0]), nlhs=0)
    assert m.get_i32(L.F_START).tolist() == [1, 4, 2, 0, 0, 0, 0]
    gw.call("set_start", h, np.array([[0.0], [0.0], [3.0], [0.0], [0.0], [0.0], [0.0]]), nlhs=0)      # a column works like a row
    assert m.get_i32(L.F_START).tolist() == [0, 0, 3, 0, 0, 0, 0]
    raises(gw, "emgpu:usage", "set_start", h, np.array([1.0, 2.0, 3.0]))
    raises(gw, "emgpu:usage", "set_start", h, np.zeros(8))
    with pytest.raises(mexrt.MexError):
        gw.call("set_start", h, np.array([9.0, 0, 0, 0, 0, 0, 0]), nlhs=0)                # bin 9 of a 4-bin variable
    assert m.get_i32(L.F_START).tolist() == [0, 0, 3, 0, 0, 0, 0]
    gw.call("free", h, nlhs=0)


@pytest.mark.parametrize("name", ["uncor_1200code_v2p1", "terminal_v3_radar_encounter_model", "balloon_v1"])
def test_save_bin_load_bin(gw, name, model_dir, tmp_path):
    path = em_io.materialize_model(name, model_dir)
    h = gw.call("load_txt", path)
    gw.call("set_prior", h, 0.5, nlhs=0)
    start = np.zeros(borrowed(h).n_initial)
    start[0] = 1
    gw.call("set_start", h, start, nlhs=0)
    binp = str(tmp_path / "m.emgpubin")
    gw.call("save_bin", h, binp, nlhs=0)
    h2 = gw.call("load_bin", binp)
    assert h2.dtype == np.uint64 and h2.shape == (1, 1) and mexrt.handle(h2) != mexrt.handle(h)
    assert_same_model(borrowed(h), borrowed(h2))
    assert borrowed(h2).get_i32(L.F_START)[0] == 1 and np.all(borrowed(h2).get_f64(L.F_ALPHA_INITIAL, 1) == 0.5)
    data = open(binp, "rb").read()
    cut = str(tmp_path / "cut.emgpubin")
    open(cut, "wb").write(data[: len(data) // 2])
    raises(gw, "emgpu:parse", "load_bin", cut)
    raises(gw, "emgpu:io", "load_bin", str(tmp_path / "absent.emgpubin"))
    raises(gw, "emgpu:io", "save_bin", h, str(tmp_path / "no_such_dir" / "m.bin"))
    raises(gw, "emgpu:usage", "save_bin", np.zeros((0, 0), dtype=np.uint64), binp)         # an empty handle is refused, not dereferenced
    raises(gw, "emgpu:usage", "save_bin", 5.0, binp)                                       # and so is a double
    h3 = gw.call("load_bin", binp)                                                         # after the errors, the good call still works
    assert_same_model(borrowed(h), borrowed(h3))
    for x in (h, h2, h3):
        gw.call("free", x, nlhs=0)


# ---------------------------------------------------------------------------------------------------------------------------------
# usage and error table

def test_check_maps_every_library_status_to_its_identifier(gw, model_dir, tmp_path):
    good = em_io.materialize_model("glider_v1", model_dir)
    want = gw.call("em_read", good)

    def still_good():
        s = gw.call("em_read", good)
        assert np.array_equal(s["N_initial"][3, 0], want["N_initial"][3, 0]) and np.array_equal(s["G_transition"], want["G_transition"])
    raises(gw, "emgpu:io", "load_txt", "/nonexistent")
    still_good()
    raises(gw, "emgpu:io", "em_read", "/nonexistent")
    bad = tmp_path / "bad.txt"
    bad.write_text("# labels_initial\n\"a\" \n# G_initial\n0 \n# r_initial\n2 \n# N_initial\n1 2 \n# bogus\n1 \n")
    e = raises(gw, "emgpu:parse", "em_read", str(bad))
    assert "Unknown field" in e.message                                                    # em_read.m:104 keeps its text
    still_good()
    raises(gw, "emgpu:parse", "load_txt", str(bad))
    cyc = {"G_initial": np.array([[False, True], [True, False]]), "N_initial": [np.ones((2, 2)), np.ones((2, 2))]}
    e = raises(gw, "emgpu:sort", "from_struct", cyc)
    assert "sorted" in e.message                                                           # bn_sort.m:23
    still_good()
    # a model larger than the gateway's fixed tables: refused by name on both routes
    ni = 40
    big = {"n_initial": ni, "n_transition": 0, "labels_initial": ['"v%d"' % i for i in range(ni)], "labels_transition": [],
           "G_initial": np.zeros((ni, ni), np.uint8), "G_transition": np.zeros((0, 0), np.uint8), "r_initial": np.full(ni, 2),
           "r_transition": np.zeros(0, int), "N_initial": [np.ones((2, 1))] * ni, "N_transition": [], "boundaries": [np.zeros(0)] * ni,
           "resample_rates": np.zeros(ni)}
    em_io.em_write(big, str(tmp_path / "big.txt"))
    assert raises(gw, "emgpu:usage", "em_read", str(tmp_path / "big.txt")).message.startswith("model size")
    assert raises(gw, "emgpu:usage", "from_struct", {"G_initial": np.zeros((ni, ni), bool), "N_initial": [np.ones((2, 1))] * ni}).message.startswith("model size")
    still_good()
    raises(gw, "emgpu:arg", "em_read", good, np.array([99.0]), True)
    still_good()
    raises(gw, "emgpu:usage", "no_such_command")
    raises(gw, "emgpu:usage", 5.0)                                                         # the command must be a character vector
    raises(gw, "emgpu:usage", "x" * 100)
    with pytest.raises(mexrt.MexError) as ei:                                              # no argument at all
        gw.call_raw([])
    assert ei.value.identifier == "emgpu:usage"
    still_good()


def _some_args(gw, model_dir):
    """For every command, arguments that pass every check that precedes the first use of a device."""
    path = em_io.materialize_model("uncor_1200code_v2p1", model_dir)
    h = gw.call("load_txt", path)
    s = gw.call("em_read", path)
    hs = np.full((1, 10), mexrt.handle(h), dtype=np.uint64)
    full = {
        "load_txt": [path], "em_read": [path], "from_struct": [s], "set_prior": [h, 1.0], "set_alpha": [h, []], "set_start": [h, np.zeros(7)],
        "save_bin": [h, "/nonexistent_dir/x.bin"], "load_bin": ["/nonexistent"], "free": [h], "device_count": [], "use_devices": [np.array([0.0])],
        "shutdown": [], "bn_sample": [h, 4.0, 1.0, 0.0], "sample_uncor": [h, 4.0, 10.0, 1.0, 0.0, 0.0, 3.0, 4.0, 6.0],
        "geom_sample": [h, 4.0, 1.0, 0.0], "propagate_terminal": [hs, np.zeros((12, 2)), np.zeros((4, 2)), 1.0, 0.0, 120.0, np.zeros((5, 2))],
        "track_uncor": [h, 4.0, 10.0, 1.0, 0.0, 0.0, 0.0, np.array([1.0, 2, 3, 4, 5, 6, 7])],
        "track_terminal": [h, hs, 4.0, 1.0, 0.0, np.zeros((5, 2)), np.zeros(4), np.zeros(4), np.arange(1.0, 13.0)],
        "sample2track": [np.zeros(2), np.zeros(2), np.zeros((3, 5, 2)), np.zeros(3), 0.0, 1.0],
    }
    return h, full


def test_one_argument_too_few_is_a_usage_error_for_every_command(gw, model_dir):
    cmds = gateway_commands()
    h, full = _some_args(gw, model_dir)
    assert set(full) == set(cmds)
    for cmd, c in cmds.items():
        assert len(full[cmd]) + 1 == c["need"], cmd                # the table above is exactly the minimum of every command
        if c["need"] <= 1:
            continue
        e = raises(gw, "emgpu:usage", cmd, *full[cmd][:-1], nlhs=c["nout"])
        assert ("emgpu_mex('%s'" % cmd) in e.message, (cmd, e.message)   # and says how the command is called
    assert borrowed(h).n_initial == 7                               # none of them touched the model
    gw.call("free", h, nlhs=0)


def test_every_shape_check_that_precedes_the_device(gw, model_dir):
    h, full = _some_args(gw, model_dir)
    ni = 7

    def with_arg(cmd, k, value, extra=()):
        a = list(full[cmd]) + list(extra)
        a[k] = value
        return [cmd] + a
    cases = [
        with_arg("geom_sample", 0, h, extra=[np.zeros((2, ni))]),                              # bounds_sample transposed
        with_arg("geom_sample", 0, h, extra=[np.zeros((ni, 3))]),
        with_arg("geom_sample", 0, h, extra=[np.zeros((0, 0)), 4.0, 4.0, np.zeros(3), np.zeros(2)]),   # lim1 not [min max]
        with_arg("geom_sample", 0, h, extra=[np.zeros((0, 0)), 4.0, 4.0, np.zeros(2), np.zeros(2), np.zeros((ni, 4))]),   # startGrid n_initial x n
        with_arg("propagate_terminal", 1, np.zeros((2, 12))),                                  # geo n x 12
        with_arg("propagate_terminal", 2, np.zeros((4, 3))),                                   # model_of of another n
        with_arg("propagate_terminal", 6, np.zeros((5, 3))),
        with_arg("propagate_terminal", 0, np.zeros((1, 10))),                                  # handles as doubles
        with_arg("propagate_terminal", 0, np.zeros((1, 65), dtype=np.uint64)),
        with_arg("track_uncor", 7, np.arange(1.0, 7.0)),                                       # idx6
        with_arg("track_uncor", 2, 0.0),                                                       # T = 0
        with_arg("track_uncor", 2, 10.0, extra=[0.0]),                                         # stride 0
        with_arg("track_terminal", 1, np.zeros((1, 9), dtype=np.uint64)),                      # 9 handles
        with_arg("track_terminal", 5, np.zeros((5, 1))),
        with_arg("track_terminal", 6, np.zeros(3)),
        with_arg("track_terminal", 7, np.zeros(5)),
        with_arg("track_terminal", 8, np.zeros(11)),
        with_arg("track_terminal", 0, h, extra=[np.zeros((2, ni))]),
        with_arg("sample2track", 1, np.zeros(3)),                                              # speed0 of another n
        with_arg("sample2track", 2, np.zeros((3, 5, 2))[:, :, :1]),                            # updates not 3 x T x n
        with_arg("sample2track", 2, np.zeros((2, 5, 2))),
        with_arg("sample2track", 3, np.zeros(2)),                                              # ur of two
        with_arg("use_devices", 0, np.zeros((0, 0))),
        with_arg("use_devices", 0, np.zeros(17)),
        with_arg("bn_sample", 0, np.zeros((0, 0), dtype=np.uint64)),                           # an empty handle
        with_arg("sample_uncor", 0, 7.0),                                                      # a handle that is no uint64
        with_arg("free", 0, np.zeros((0, 0), dtype=np.uint64)),
        with_arg("load_txt", 0, 7.0),                                                          # a file name that is no char
        with_arg("load_txt", 0, full["load_txt"][0], extra=[np.zeros(33)]),                    # more zero-boundary indices than the table holds
    ]
    for c in cases:
        raises(gw, "emgpu:usage", *c, nlhs=3)
    assert np.array_equal(borrowed(h).get_i32(L.F_R_INITIAL), native.NativeModel.load_txt(full["load_txt"][0]).get_i32(L.F_R_INITIAL))
    gw.call("free", h, nlhs=0)


def test_free_releases_each_kind_of_handle(gw, model_dir, tmp_path):
    path = em_io.materialize_model("glider_v1", model_dir)
    h1 = gw.call("load_txt", path)
    h2 = gw.call("from_struct", gw.call("em_read", path))
    gw.call("save_bin", h1, str(tmp_path / "g.bin"), nlhs=0)
    h3 = gw.call("load_bin", str(tmp_path / "g.bin"))
    assert len({mexrt.handle(h) for h in (h1, h2, h3)}) == 3
    for h in (h1, h2, h3):
        assert h.dtype == np.uint64 and h.shape == (1, 1)
        assert gw.call("free", h, nlhs=0) is None
    # 2^53 - 1 is the largest seed / first index a double carries exactly; the gateway's header says so
    assert float(2**53 - 1) == 2**53 - 1 and float(2**53 + 1) != 2**53 + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# structure: gateway source, header comment, usage strings, shipped .m call sites, and the tests themselves

def gateway_source():
    return open(os.path.join(MATLAB_DIR, "emgpu_mex.c")).read()


def _split_signature(text, start):
    """Arguments of the call whose '(' is at text[start]: count of top-level arguments, index after the ')'.
    Knows (), [], {}, MATLAB's '...' strings and C's escaped quotes in a usage string."""
    depth, i, nargs, seen = 0, start, 0, False
    while i < len(text):
        c = text[i]
        if c == "'":
            j = text.index("'", i + 1)
            while text[j + 1: j + 2] == "'":
                j = text.index("'", j + 2)
            i, seen = j, True
        elif c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                return nargs + (1 if seen else 0), i + 1
        elif c == "," and depth == 1:
            nargs += 1
        elif not c.isspace():
            seen = True
        i += 1
    raise AssertionError("unbalanced call at %r" % text[start: start + 80])


def _outputs_before(text, pos):
    """Number of outputs of the call that starts at text[pos] ('emgpu_mex('): [a, b] = , x = , or none."""
    head = text[max(0, pos - 200): pos]
    m = re.search(r"\[([^\[\]=]*)\]\s*=\s*$", head)
    if m:
        return len([x for x in re.split(r"[,\s]+", m.group(1).strip()) if x])
    return 1 if re.search(r"[\w\)\}]\s*=\s*$", head) else 0


def signatures(text):
    """(command, number of arguments with the command, number of outputs) of every emgpu_mex('cmd', ...) in text."""
    out = []
    for m in re.finditer(r"emgpu_mex\('([a-z_0-9]+)'", text):
        nargs, _ = _split_signature(text, m.start() + len("emgpu_mex"))
        out.append((m.group(1), nargs, _outputs_before(text, m.start())))
    return out


def gateway_commands():
    """Per command of mexFunction: need = least nrhs (need()'s minimum, the command included), nargs = highest prhs[k] read + 1,
    nout = highest plhs[k] written + 1, usage = the signatures in its usage strings."""
    src = gateway_source()
    body = src[src.index("void mexFunction("):]
    heads = list(re.finditer(r'^    (?:\} else )?if \(((?:!strcmp\(cmd, "[a-z_0-9]+"\)(?: \|\| )?)+)\) \{$', body, re.M))
    assert heads
    helper = re.search(r"static void events_out\(.*?\n\}\n", src, re.S).group(0)
    out = {}
    for k, hd in enumerate(heads):
        block = body[hd.end(): heads[k + 1].start() if k + 1 < len(heads) else len(body)]
        if "events_out(" in block:
            block += helper
        need = re.search(r"need\(nrhs, (\d+),", block)
        prhs = [int(x) for x in re.findall(r"prhs\[(\d+)\]", block)]
        plhs = [int(x) for x in re.findall(r"plhs\[(\d+)\]", block)]
        usage = signatures(" ".join(re.findall(r'"((?:[^"\\]|\\.)*)"', block)))
        for cmd in re.findall(r'"([a-z_0-9]+)"', hd.group(1)):
            out[cmd] = {"need": int(need.group(1)) if need else 1, "nargs": max(prhs + [0]) + 1, "nout": max(plhs + [-1]) + 1,
                        "usage": [(n, o) for c, n, o in usage if c == cmd]}
    return out


def _matlab_code(text):
    """A .m file without its comments, continuation lines joined."""
    lines = []
    for raw in text.split("\n"):
        in_s, prev, cut = False, "", len(raw)
        for i, c in enumerate(raw):
            if c == "'":
                if in_s:
                    in_s = False
                elif not (prev.isalnum() or prev in ")]}'._"):     # after an operand ' is a transpose, elsewhere it opens a string
                    in_s = True
            elif c == "%" and not in_s:
                cut = i
                break
            if not c.isspace():
                prev = c
        lines.append(raw[:cut].rstrip())
    return re.sub(r"\.\.\.\s*\n", " ", "\n".join(lines))


def test_arity_of_gateway_header_usage_strings_and_m_call_sites_agree():
    cmds = gateway_commands()
    src = gateway_source()
    assert set(cmds) == set(re.findall(r'!strcmp\(cmd, "([a-z_0-9]+)"\)', src)) and len(cmds) == 19
    header = {}
    for cmd, nargs, nout in signatures(src[: src.index("#include")]):
        header.setdefault(cmd, []).append((nargs, nout))
    for cmd, c in cmds.items():
        assert c["need"] <= c["nargs"], cmd
        assert cmd in header, "%s is missing from the header comment's signature list" % cmd
        for what, sigs in (("header comment", header[cmd][:1]), ("usage string", c["usage"])):
            for nargs, nout in sigs:
                assert nargs == c["nargs"], "%s of %s lists %d arguments, the code reads prhs[%d]" % (what, cmd, nargs, c["nargs"] - 1)
                assert nout == c["nout"], "%s of %s lists %d outputs, the code writes plhs[%d]" % (what, cmd, nout, c["nout"] - 1)
        assert c["usage"] or c["need"] <= 1, "%s has a minimum and no usage string" % cmd
    sites = 0
    for base, _, files in os.walk(MATLAB_DIR):
        for f in files:
            if not f.endswith(".m"):
                continue
            for cmd, nargs, nout in signatures(_matlab_code(open(os.path.join(base, f)).read())):
                sites += 1
                assert cmd in cmds, (f, cmd)
                assert cmds[cmd]["need"] <= nargs <= cmds[cmd]["nargs"], "%s calls %s with %d arguments (%d..%d)" % (f, cmd, nargs, cmds[cmd]["need"], cmds[cmd]["nargs"])
                assert nout <= cmds[cmd]["nout"], "%s takes %d outputs of %s (%d)" % (f, nout, cmd, cmds[cmd]["nout"])
    assert sites >= 25          # the parser saw the call sites (28 when this was written)
    assert "exact up to 2^53 - 1" in src[: src.index("#include")]


def test_every_command_is_run_by_the_two_gateway_modules():
    """Coverage by construction, like tests/test_instances.py for kernel names: a command of the gateway that neither
    tests/test_mex_gateway.py nor tests/test_gpu_mex_gateway.py passes to call() fails here."""
    called = set()
    for f in ("test_mex_gateway.py", "test_gpu_mex_gateway.py"):
        called |= set(re.findall(r'\.call\(\s*"([a-z_0-9]+)"', open(os.path.join(ROOT, "tests", f)).read()))
    missing = set(gateway_commands()) - called
    assert not missing, "never executed: %s" % sorted(missing)
