"""CPU: the kernel-instance table (instances.py) covers every instance the launcher sources name, and every generated model has the
plan its row asks for -- so that a failure in test_gpu_instances.py cannot come from a misbuilt model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import instances as I
from em_model_manned_bayes_amd import _lib as L
from util import load_row_model, plan_facts, shaped_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "em_model_manned_bayes_amd", "csrc")
NAME_RE = re.compile(r'"(k_[a-z0-9_]*<[^"]*)"')
TAG_RE = re.compile(r'EMGPU_S2_CASE(?:_W)?\([^;]*?"(\[[^"]*\])"\)')


def source_names(csrc=CSRC):
    """(kernel name literals, EMGPU_S2_CASE / EMGPU_S2_CASE_W tags) of the launcher sources."""
    names, tags = set(), set()
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h", ".cpp", ".hpp")):
            with open(os.path.join(csrc, f)) as fh:
                text = fh.read()
            names |= set(NAME_RE.findall(text))
            tags |= set(TAG_RE.findall(text))
    return names, tags


def all_rows():
    return I.ROWS + [r for _, lo, hi, _ in I.EDGES for r in (lo, hi)]


def base_name(kernel):
    """A reported name without its event suffixes: the instance's name literal (+ the mask tag)."""
    for suffix in ("+rows-by-wave+events", "+events"):
        if kernel.endswith(suffix):
            return kernel[: -len(suffix)]
    return kernel


def uncovered(names, tags, rows):
    reached = {base_name(r["kernel"]) for r in rows}
    missing = sorted(n for n in names if n not in reached and n not in I.COVERED_ELSEWHERE and n not in I.UNREACHABLE)
    missing += sorted(t for t in tags if not any(k.endswith(t) for k in reached) and t not in I.UNREACHABLE)
    return missing


def test_every_instance_in_the_sources_has_a_row():
    names, tags = source_names()
    assert len(names) >= 75 and len(tags) >= 16, (len(names), len(tags))   # the regexes still find what they were written for
    missing = uncovered(names, tags, all_rows())
    assert not missing, "kernel instances without a row in tests/instances.py: %s" % missing
    # ... and the other way round: no row names an instance the sources no longer have
    stale = sorted({base_name(r["kernel"]) for r in all_rows()} - {n + t for n in names for t in [""] + sorted(tags)})
    assert not stale, "rows of instances the sources do not name: %s" % stale
    for name, reason in I.UNREACHABLE.items():
        assert isinstance(reason, str) and reason.strip(), name
    for name, test_id in I.COVERED_ELSEWHERE.items():
        module, test = test_id.split("::")
        path = os.path.join(ROOT, *module.split(".")) + ".py"
        with open(path) as fh:
            src = fh.read()
        assert re.search(r"^def %s\(" % re.escape(test), src, re.M), test_id
        assert name in src, (name, test_id)                           # the test asserts the name it is listed for


def test_a_new_name_literal_without_a_row_is_reported(tmp_path):
    """The completeness check itself: a fake instance in a copy of the sources is reported, an empty table reports everything."""
    import shutil
    copy = tmp_path / "csrc"
    shutil.copytree(CSRC, copy, ignore=shutil.ignore_patterns("*.o", "*.so", "*.d"))
    with open(copy / "emgpu_kernels_fast.hip", "a") as fh:
        fh.write('\nstatic const char *kStale = "k_uncor_fast<7,8,8,8>";\n')
    names, tags = source_names(str(copy))
    assert uncovered(names, tags, all_rows()) == ["k_uncor_fast<7,8,8,8>"]
    assert len(uncovered(names, tags, [])) == len(names) + len(tags) - len(I.COVERED_ELSEWHERE)


def _expected_masks(spec):
    nd = len(spec["meff"])
    if spec["parents"] is not None:
        return tuple(spec["parents"])
    cur = sum(1 << (5 * k) for k in range(nd))
    new = sum(1 << (5 * k - 1) for k in range(1, nd)) if spec["dependent"] else 0
    return cur, new


def _shaped_specs():
    seen, out = set(), []
    for r in all_rows():
        for m in [r["model"]] + list(r.get("with_", [])):
            if isinstance(m, dict) and repr(sorted(m.items())) not in seen:
                seen.add(repr(sorted(m.items())))
                out.append(m)
    return out


@pytest.mark.parametrize("spec", _shaped_specs(), ids=lambda s: "s%d_ni%d_m%s" % (s["seed"], s["ni"], "".join(map(str, s["meff"]))))
def test_shaped_models_compile_to_the_plan_they_ask_for(spec, model_dir):
    """Over EVERY transition column (emgpu_debug_dynamic_column / _padded_column): exactly meff distinct real thresholds per column,
    d_meff = meff, the padded width of that meff; the parent masks asked for; the requested bins and rates."""
    nm, pp, _ = load_row_model(spec, model_dir)
    f = plan_facts(nm)
    meff = list(spec["meff"])
    assert nm.n_initial == spec["ni"] and nm.n_dyn == len(meff)
    assert f["col_meff"] == [(m, m) for m in meff], f
    assert f["meff"] == [m if r <= 15 else 0 for m, r in zip(meff, f["r"])], f
    assert f["width"] == [(4 if m <= 3 else 8 if m <= 6 else 0) if r <= 15 else 0 for m, r in zip(meff, f["r"])], f
    assert (f["cur"], f["new"]) == _expected_masks(spec), (hex(f["cur"]), hex(f["new"]))
    if spec["r"] is not None:
        assert list(pp["r_initial"]) == list(spec["r"])
    rates = np.asarray(pp["resample_rates"], dtype=np.float64)
    if spec["rates"] is not None:
        assert np.array_equal(rates, np.asarray(spec["rates"], dtype=np.float64))
    lib = L.lib()
    for v, rate in enumerate(rates):
        R = int(lib.emgpu_debug_bernoulli_threshold(C.c_double(float(rate))))
        if rate == 1.0:
            assert R == 0xFFFFFFFF                           # only k_dbn_generic takes it
        elif rate == I.RATE_AT_EDGE:
            assert R == 0xFFFF0000                           # the first threshold the fast and step2 kernels decline
        elif rate == I.RATE_BELOW_EDGE:
            assert R == 0xFFFEFFFF                           # the last one they take (low halfword all ones)
        elif rate > 0:
            assert 0 < R < 0xFFFE0000


def _generated(spec):
    kw = dict(spec)
    return shaped_model(np.random.RandomState(kw.pop("seed")), **kw)


@pytest.mark.parametrize("edge", I.EDGES, ids=lambda e: e[0])
def test_the_edge_pairs_differ_only_where_they_say(edge):
    """The two sides of an eligibility edge are one model with one argument changed: their shaped_model arguments differ in that
    argument alone, and the generated models are equal in every table, boundary set, graph entry and rate it does not reach."""
    what, lo, hi, field = edge
    a, b = lo["model"], hi["model"]
    assert isinstance(a, dict) and isinstance(b, dict) and lo["kernel"] != hi["kernel"], what
    assert {k for k in a if a[k] != b[k]} == {field}, what
    A, B = _generated(a), _generated(b)
    ni, nd = min(a["ni"], b["ni"]), len(a["meff"])
    same = lambda x, y: np.array_equal(np.asarray(x), np.asarray(y))
    reached_init, reached_dyn = set(), set()                  # initial variables / dynamic variables whose tables the change reaches
    if field == "meff":
        reached_dyn = {k for k in range(nd) if a["meff"][k] != b["meff"][k]}
    elif field == "r":
        changed = {v for v in range(ni) if a["r"][v] != b["r"][v]}
        reached_init = changed | {v for v in range(ni) for u in changed if A["G_initial"][u, v]}
        reached_dyn = {k for k in range(nd) for u in changed if A["G_transition"][u, a["ni"] + k] or u == k}
    elif field == "rates":
        assert not same(A["resample_rates"], B["resample_rates"]), what
    if field != "rates":
        assert same(A["resample_rates"][:ni], B["resample_rates"][:ni]), what
    assert same(A["G_initial"][:ni, :ni], B["G_initial"][:ni, :ni]), what
    for v in range(ni):
        if v not in reached_init:
            assert same(A["N_initial"][v], B["N_initial"][v]), (what, v)
        if field != "r" or a["r"][v] == b["r"][v]:
            assert same(A["boundaries"][v], B["boundaries"][v]) and A["r_initial"][v] == B["r_initial"][v], (what, v)
    for k in range(nd):
        ca, cb = A["G_transition"][:, a["ni"] + k], B["G_transition"][:, b["ni"] + k]
        assert same(ca[:ni], cb[:ni]) and same(ca[a["ni"]:], cb[b["ni"]:]), (what, k)   # the same parents
        if k not in reached_dyn:
            assert same(A["N_transition"][a["ni"] + k], B["N_transition"][b["ni"] + k]), (what, k)
