"""CPU: the dispatcher without a GPU.  emgpu_debug_kernel_choice makes the choice launch_dbn makes (choose_dbn) from a model and the null /
non-null pattern of a call's pointers; the names it predicts are compared with the ones the GPU suites assert after running the call --
instances.ROWS and EDGES, the debug variables of test_gpu_parity.py, the start grids of start_grid_cases / step2_start_cases.  The expected
names come from those tables alone."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import instances as I
import start_grid_cases as S
import step2_start_cases as S2
from em_model_manned_bayes_amd import native, _lib as L
from parity_models import DEP_MODELS, FAST_MODELS
from util import load_row_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000            # a pointer that is not null: the export never follows it
N, T = 777, 61
OUTSIDE_LAUNCH_DBN = {"mixed", "bn", "bn+start"}    # emgpu_sample_dbn_blocks_device's shared launch and emgpu_sample_bn_*: other launchers


def predict(nm, form, per_step=False, grid=False, log_weight=False, indices=False, n=N, cap=128):
    """The name launch_dbn would record for a call in `form` (instances.py; "dense" = "both", the start-grid modules' word), with the
    pointers test_gpu_instances.py's _host / _device hand in for it."""
    flags, event_cap = 0, 0
    dense = form in ("both", "dense", "idx", "list+dense", "one")
    events = form in ("list", "list+dense", "plain")
    if events:
        event_cap = min((nm.n_initial + nm.n_dyn + 1) * T + 2, 4096)
    if form == "plain":
        flags, event_cap = L.FLAG_NO_RESAMPLE | L.FLAG_NO_DEDISC | L.FLAG_NO_TERMINATOR, nm.n_initial * T + 1
    p, _keep = native.make_params(n, T, 1, transition_mode=L.TRANSITION_PER_STEP if per_step else L.TRANSITION_REFERENCE_AUTO, flags=flags,
                                  event_cap=event_cap, indices=PTR if (indices or form == "idx") else None, start=PTR if grid else None)
    o = L.SampleOut()
    if form != "one":
        o.init_bin, o.init_val, o.attempts = PTR, PTR, PTR
    if dense:
        o.dyn_bin = PTR
        if form != "one":
            o.dyn_val = PTR
    if events:
        o.ev_count, o.events = PTR, PTR
    if log_weight:
        o.log_weight = PTR
    buf = C.create_string_buffer(cap)
    L.check(L.lib().emgpu_debug_kernel_choice(nm._h, C.byref(p), C.byref(o), buf, cap))
    return buf.value.decode()


def names_of(requests, model_dir):
    """predict() for a list of dict(model=, **predict's keywords)"""
    out = []
    for r in requests:
        r = dict(r)
        nm, _, _ = load_row_model(r.pop("model"), model_dir)
        out.append(predict(nm, **r))
    return out


_CHILD = r"""
import json, sys
sys.path[:0] = [%r, %r, %r]
from test_dispatch import names_of
print("names " + json.dumps(names_of(json.loads(sys.argv[1]), sys.argv[2])))
"""


def names_in_child(requests, env, model_dir):
    """The same in a child process with `env`: the library reads its debug variables once per process."""
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    r = subprocess.run([sys.executable, "-c", code, json.dumps(requests), str(model_dir)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("names ")][-1][6:])


def _row_id(r):
    m = r["model"] if isinstance(r["model"], str) else "s%d" % r["model"]["seed"]
    return "%s-%s-%s%s" % (r["kernel"], m, r["form"], "-perstep" if r.get("per_step") else "")


def _request(row):
    return dict(model=row["model"], form=row["form"], per_step=bool(row.get("per_step")))


ALL_ROWS = I.ROWS + [r for _, lo, hi, _ in I.EDGES for r in (lo, hi)]
DBN_ROWS = [r for r in ALL_ROWS if r["form"] not in OUTSIDE_LAUNCH_DBN]


def test_only_the_forms_outside_launch_dbn_are_skipped():
    assert {r["form"] for r in ALL_ROWS} - {r["form"] for r in DBN_ROWS} == OUTSIDE_LAUNCH_DBN
    assert {r["form"] for r in DBN_ROWS} == {"both", "one", "idx", "list", "list+dense", "plain"}
    assert len(DBN_ROWS) == len(ALL_ROWS) - sum(r["form"] in OUTSIDE_LAUNCH_DBN for r in ALL_ROWS) and len(DBN_ROWS) >= 120


@pytest.mark.parametrize("row", [r for r in DBN_ROWS if not r.get("env")], ids=_row_id)
def test_the_choice_is_the_rows_kernel(row, model_dir):
    assert names_of([_request(row)], model_dir) == [row["kernel"]]


ENVS = sorted({json.dumps(r["env"], sort_keys=True) for r in DBN_ROWS if r.get("env")})


@pytest.mark.parametrize("env", ENVS)
def test_the_choice_under_a_rows_debug_variable(env, model_dir):
    rows = [r for r in DBN_ROWS if r.get("env") and json.dumps(r["env"], sort_keys=True) == env]
    assert names_in_child([_request(r) for r in rows], json.loads(env), model_dir) == [r["kernel"] for r in rows]


@pytest.mark.parametrize("rows", ["lane", "wide", "long"])
def test_event_rows_variable_sends_lists_to_the_kernels_the_parity_test_names(rows, model_dir):
    """test_gpu_parity.py::test_every_fast_model_through_the_per_lane_event_kernels: its models, its prefixes, no rows by the wave"""
    models = FAST_MODELS + (DEP_MODELS[:3] + ["cor_v1", "littoral_cor_v1"] if rows == "lane" else [])
    got = names_in_child([dict(model=m, form="list") for m in models], {"EMGPU_DEBUG_EVENT_ROWS": rows}, model_dir)
    for name, kernel in zip(models, got):
        fast = name in FAST_MODELS
        want = ("k_uncor_fast_evu_long" if rows == "long" else "k_uncor_fast_evw" if rows == "wide" or name == "haa_v1" else "k_uncor_fast_ev<") if fast else "k_dbn_step2"
        assert kernel.startswith(want) and "rows-by-wave" not in kernel, (name, kernel)


def test_no_step2_variable_sends_the_dependent_branch_to_k_dbn_step(model_dir):
    """test_gpu_parity.py::test_fallback_per_step_kernel_still_matches_oracle"""
    got = names_in_child([dict(model=m, form="both") for m in ("glider_v1", "cor_v1")], {"EMGPU_DEBUG_NO_STEP2": "1"}, model_dir)
    assert len(got) == 2 and all(k.startswith("k_dbn_step<") for k in got), got


# ---- start grids
FAST_START = {("uncor_1200code_v2p1", "dense"): "k_uncor_fast_idx<7,2,4,2>+start", ("uncor_1200code_v2p1", "list"): "k_uncor_fast_evu<7,2,4,2>+start",
              ("uncor_1200only_fwse_v1p2", "dense"): "k_uncor_fast_idx<7,4,6,6>+start", ("haa_v1", "list"): "k_uncor_fast_evu_long<9,6,6,6>+start"}


def _fast_name_ok(kernel, form):   # test_gpu_start_grid.py's _name_ok
    return kernel.endswith("+start") and kernel.startswith("k_uncor_fast_idx<" if form == "dense" else "k_uncor_fast_evu")


@pytest.mark.parametrize("presets", ["grid", "log_weight", "grid+log_weight"])
@pytest.mark.parametrize("form", ["dense", "list"])
@pytest.mark.parametrize("case", S2.NAMES)
def test_start_grid_on_the_per_timestep_kernel(case, form, presets, model_dir):
    nm, _, _ = S2.load(case, model_dir)
    kw = dict(per_step=S2.per_step(case), grid="grid" in presets, log_weight="log_weight" in presets)
    assert predict(nm, form, **kw) == S2.kernel_name(case, form)
    assert predict(nm, "list+dense", **kw).startswith("k_dbn_generic<")         # the list and the dense trace together
    assert predict(nm, "idx", **kw).startswith("k_dbn_generic<")                # an index list off the fast branch


@pytest.mark.parametrize("presets", ["grid", "log_weight", "grid+log_weight"])
@pytest.mark.parametrize("form", ["dense", "list"])
@pytest.mark.parametrize("name", S.MODELS)
def test_start_grid_on_the_fast_kernels(name, form, presets, model_dir):
    nm, _, _ = load_row_model(name, model_dir)
    kw = dict(grid="grid" in presets, log_weight="log_weight" in presets)
    kernel = predict(nm, form, **kw)
    assert _fast_name_ok(kernel, form), kernel
    if (name, form) in FAST_START:
        assert kernel == FAST_START[(name, form)]
    assert predict(nm, "list+dense", **kw).startswith("k_dbn_generic<")
    idx = predict(nm, "idx", **kw)                                              # the later rounds of UncorEncounterModel.track
    assert _fast_name_ok(idx, "dense") and idx == predict(nm, "dense", **kw)
    assert not predict(nm, form).endswith("+start")                             # no presets: the instance itself


def test_arguments_are_checked(model_dir):
    nm, _, _ = load_row_model("uncor_1200code_v2p1", model_dir)
    p, _keep = native.make_params(N, T, 1)
    o = L.SampleOut()
    o.dyn_bin = o.dyn_val = PTR
    lib, buf = L.lib(), C.create_string_buffer(64)
    want = b"k_uncor_fast<7,2,4,2>"
    assert lib.emgpu_debug_kernel_choice(nm._h, C.byref(p), C.byref(o), buf, 64) == 0 and buf.value == want
    for args in ((None, C.byref(p), C.byref(o), buf, 64), (nm._h, None, C.byref(o), buf, 64), (nm._h, C.byref(p), None, buf, 64),
                 (nm._h, C.byref(p), C.byref(o), None, 64)):
        assert lib.emgpu_debug_kernel_choice(*args) == L.ERR_ARG
    for cap in (-1, 0, 1, len(want)):                                           # no room for the terminating zero
        assert lib.emgpu_debug_kernel_choice(nm._h, C.byref(p), C.byref(o), buf, cap) == L.ERR_ARG
    assert lib.emgpu_debug_kernel_choice(nm._h, C.byref(p), C.byref(o), buf, len(want) + 1) == 0 and buf.value == want
