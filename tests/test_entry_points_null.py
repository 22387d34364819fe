"""CPU: what every exported entry point that takes an emgpu_ctx * or an emgpu_model * answers to NULL handles -- a status and a message,
never a crash, and nothing here needs a device.

TABLE holds, per entry point, two expectations recorded from the library as it was BEFORE the C ABI unit was split by owner and its entry
openings became CTX_DEVICE / CTX_ENTER ("The C ABI units"); they are written out literally, so a unit that reorders its checks or
rewords a refusal fails here:
  * `null`: every pointer NULL, every integer 0, every double 0.0;
  * `no_ctx`: the context (or the context list) NULL and everything else valid -- a model from from_arrays, parameter structs from the
    native.*_params helpers (zeroed structs with n = 1 where native has no helper), small zeroed buffers behind every other pointer.  An
    entry point that takes no context has None there.
An expectation is (status, message): the return value as an integer (None for a void function, bytes for emgpu_last_kernel_name) and
emgpu_last_error() behind the call.  The message of a call that did not fail is nobody's: it is None and not compared.

The table is complete by construction: the test fails when L.SYMBOLS holds a name whose declaration in include/emgpu.h takes a context or
a model and the table does not (or the other way round).  No entry point had to be left out: none dereferences a NULL handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from em_model_manned_bayes_amd import _lib as L, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NA, CTX, MODEL = b"null argument", b"null ctx", b"null model"

# name: (null, no_ctx)
TABLE = {
    "emgpu_count_dbn_device": ((-1, NA), (-1, CTX)),
    "emgpu_count_dbn_host": ((-1, NA), (-1, CTX)),
    "emgpu_count_dbn_weighted_device": ((-1, NA), (-1, CTX)),
    "emgpu_count_dbn_weighted_host": ((-1, NA), (-1, CTX)),
    "emgpu_count_layout": ((-1, NA), None),
    "emgpu_ctx_free": ((None, None), (None, None)),
    "emgpu_ctx_set_stream": ((-1, CTX), (-1, CTX)),
    "emgpu_ctx_sync": ((-1, CTX), (-1, CTX)),
    "emgpu_ctx_trim": ((-1, CTX), (-1, CTX)),
    "emgpu_debug_dynamic_column": ((-1, NA), None),
    "emgpu_debug_format_paths": ((-1, NA), (-1, NA)),
    "emgpu_debug_kernel_choice": ((-1, NA), None),
    "emgpu_debug_padded_column": ((-1, NA), None),
    "emgpu_debug_parent_masks": ((-1, NA), None),
    "emgpu_debug_pk_column": ((-1, NA), None),
    "emgpu_debug_terminal_counters": ((-1, NA), (-1, NA)),
    "emgpu_debug_uncor_dynamics_host": ((-1, b"bad argument"), (-1, b"bad argument")),
    "emgpu_device_alloc": ((-1, NA), (-1, NA)),
    "emgpu_device_download": ((-1, CTX), (-1, CTX)),
    "emgpu_device_free": ((0, None), (-1, CTX)),
    "emgpu_device_upload": ((-1, CTX), (-1, CTX)),
    "emgpu_discretize_dbn_device": ((-1, NA), (-1, CTX)),
    "emgpu_discretize_dbn_host": ((-1, NA), (-1, CTX)),
    "emgpu_format_f0_host": ((-1, NA), (-1, NA)),
    "emgpu_format_g_host": ((-1, NA), (-1, NA)),
    "emgpu_host_alloc": ((-1, NA), (-1, NA)),
    "emgpu_host_free": ((0, None), (-1, CTX)),
    "emgpu_host_stats": ((-1, NA), (-1, NA)),
    "emgpu_last_kernel_name": ((b"", None), (b"", None)),
    "emgpu_last_launch_count": ((0, None), (0, None)),
    "emgpu_model_free": ((None, None), None),
    "emgpu_model_get_f64": ((-1, MODEL), None),
    "emgpu_model_get_i32": ((-1, MODEL), None),
    "emgpu_model_get_text": ((-1, MODEL), None),
    "emgpu_model_info": ((-1, NA), None),
    "emgpu_model_log_prob": ((-1, MODEL), None),
    "emgpu_model_save_bin": ((-1, NA), None),
    "emgpu_model_set_f64": ((-1, b"null argument or negative length"), None),
    "emgpu_model_set_prior": ((-1, MODEL), None),
    "emgpu_model_set_start": ((-1, b"start needs n_initial entries"), None),
    "emgpu_model_set_transition_stay_prior": ((-1, MODEL), None),
    "emgpu_model_set_zero_bins": ((-1, b"zero_bins needs n_initial entries"), None),
    "emgpu_model_start_log_weight": ((-1, NA), None),
    "emgpu_parse_table_host": ((-1, NA), (-1, NA)),
    "emgpu_propagate_terminal_device": ((-1, NA), (-1, NA)),
    "emgpu_propagate_terminal_host": ((-1, NA), (-1, NA)),
    "emgpu_sample2track_device": ((-1, NA), (-1, NA)),
    "emgpu_sample2track_host": ((-1, NA), (-1, NA)),
    "emgpu_sample_bn_device": ((-1, NA), (-1, NA)),
    "emgpu_sample_bn_host": ((-1, NA), (-1, NA)),
    "emgpu_sample_dbn_blocks_device": ((-1, NA), (-1, NA)),
    "emgpu_sample_dbn_device": ((-1, NA), (-1, NA)),
    "emgpu_sample_dbn_host": ((-1, NA), (-1, NA)),
    "emgpu_sample_dbn_multi_device": ((-1, NA), (-1, NA)),
    "emgpu_sample_dbn_multi_host": ((-1, NA), (-1, NA)),
    "emgpu_sample_terminal_device": ((-1, NA), (-1, NA)),
    "emgpu_sample_text_host": ((-1, NA), (-1, NA)),
    "emgpu_sample_uncor_host": ((-1, NA), (-1, NA)),
    "emgpu_score_dbn_device": ((-1, NA), (-1, CTX)),
    "emgpu_score_dbn_host": ((-1, NA), (-1, CTX)),
    "emgpu_start_grid_log_weight": ((-1, b"null argument or n < 0"), None),
    "emgpu_text_bound": ((-1, NA), None),
    "emgpu_trace_alloc": ((-1, NA), (-1, NA)),
    "emgpu_trace_free": ((0, None), (-1, CTX)),
    "emgpu_track_terminal_host": ((-1, NA), (-1, NA)),
    "emgpu_track_uncor_device": ((-1, NA), (-1, NA)),
    "emgpu_track_uncor_grid_device": ((-1, NA), (-1, NA)),
    "emgpu_track_uncor_grid_host": ((-1, NA), (-1, NA)),
    "emgpu_track_uncor_host": ((-1, NA), (-1, NA)),
    "emgpu_track_values_device": ((-1, NA), (-1, CTX)),
    "emgpu_track_values_host": ((-1, NA), (-1, CTX)),
    "emgpu_tracks_text_host": ((-1, NA), (-1, NA)),
    "emgpu_uncor_dynamic_limits": ((-1, NA), None),
}


def handle_params():
    """name -> the kinds of its parameters by position ("ctx", "ctxs", "model", "models" or None), for every function include/emgpu.h
    declares with a context or a model among them (a `**` is an output, not a handle)."""
    hdr = open(os.path.join(ROOT, "include", "emgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    out = {}
    for name, params in re.findall(r"\b(emgpu_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr):
        kinds = []
        for prm in params.split(","):
            m = re.search(r"\bemgpu_(ctx|model)\s*(\*\s*(?:const\s*)?\*?)", prm)
            stars = m.group(2).count("*") if m else 0
            kinds.append(None if not m or (stars == 2 and "const" not in m.group(2)) else m.group(1) + ("s" if stars == 2 else ""))
        if any(kinds):
            out[name] = kinds
    return out


HANDLES = handle_params()
INTS = (C.c_int32, C.c_int64, C.c_uint32, C.c_uint64)


def null_args(name):
    f = getattr(L.lib(), name)
    assert f.argtypes is not None and len(f.argtypes) == len(HANDLES[name]), name
    return [t(0) if t in INTS else 0.0 if t is C.c_double else None for t in f.argtypes]


class Valid:
    """What `no_ctx` passes for everything that is not a context: built once, kept alive for the module."""

    def __init__(self):
        # two initial variables, the second a child of the first, and one dynamic variable that follows the second
        N_i = [np.ones((2, 1)), np.ones((3, 2))]
        G_t = np.zeros((3, 3))
        G_t[0, 2] = G_t[1, 2] = 1
        self.model = native.NativeModel.from_arrays(np.array([[0, 1], [0, 0]]), [2, 3], N_i, G_t, [2, 3, 3], [np.ones((3, 6))], temporal_map=[[2, 3]],
                                                    boundaries=[[], [0.0, 1.0, 2.0, 3.0]], labels_initial=['"G"', '"v"'],
                                                    labels_transition=['"G"', '"v"', '"v(t+1)"'])
        self.models = (C.c_void_p * 10)(*[self.model._h] * 10)
        self.sample, self.keep = native.make_params(1, 1, 1)
        self.structs = {
            L.SampleParams: self.sample,
            L.UTrackParams: native.utrack_params(self.model, 1, 1, 1),
            L.TrackParams: native.track_params(1, 1, 1.0, 1.0, 1.0, 0.0, 1000.0, nd=3, slot_vertrate=0, slot_acc=1, slot_turnrate=2),
            L.ScoreParams: native.score_params(1, 1),
            L.DiscretizeParams: native.discretize_params(1, 1),
            L.TrackValuesParams: native.track_values_params(1, 3, 1.0, 1.0, 1.0),
            L.SampleOut: native._sample_out(),
        }
        for T in (L.BnParams, L.TermParams, L.TSampleParams, L.TTrackParams):   # (native builds these inside its wrappers)
            p = T()
            p.n = 1
            self.structs[T] = p
        self.buffers = []

    def args(self, name):
        f = getattr(L.lib(), name)
        out = []
        for t, kind in zip(f.argtypes, HANDLES[name]):
            if kind in ("ctx", "ctxs"):
                out.append(None)
            elif kind == "model":
                out.append(self.model._h)
            elif kind == "models":
                out.append(self.models)
            elif t in INTS:
                out.append(t(10 if name.endswith(("terminal_device", "terminal_host")) else 1))
            elif t is C.c_double:
                out.append(1.0)
            elif hasattr(t, "_type_") and t._type_ in self.structs:
                out.append(C.byref(self.structs[t._type_]))
            else:
                self.buffers.append(C.create_string_buffer(4096))
                out.append(C.cast(self.buffers[-1], C.c_void_p) if t is C.c_void_p else C.cast(self.buffers[-1], t))
        return out


def observe(name, args):
    lib = L.lib()
    lo, hi = C.c_int64(), C.c_int64()
    assert lib.emgpu_shard_range(-1, 0, 1, C.byref(lo), C.byref(hi)) == L.ERR_ARG      # a message that is none of the table's, to see who speaks
    rc = getattr(lib, name)(*args)
    msg = lib.emgpu_last_error()
    failed = isinstance(rc, int) and rc < 0
    assert failed == (msg != b"bad shard arguments"), (name, rc, msg)
    return (rc, msg if failed else None)


def test_the_table_names_every_entry_point_that_takes_a_context_or_a_model():
    assert set(HANDLES) <= set(L.SYMBOLS)                       # (test_host.py: the header declares exactly L.SYMBOLS)
    assert len(HANDLES) >= 70, len(HANDLES)                     # the regex still finds what it was written for
    for name in ("emgpu_ctx_create", "emgpu_model_load_txt", "emgpu_model_from_arrays", "emgpu_shard_range", "emgpu_trace_out"):
        assert name not in HANDLES                              # outputs and other handles are not contexts or models
    assert sorted(TABLE) == sorted(HANDLES), sorted(set(TABLE) ^ set(HANDLES))
    for name, kinds in HANDLES.items():
        has_ctx = any(k in ("ctx", "ctxs") for k in kinds)
        assert (TABLE[name][1] is not None) == has_ctx, name


@pytest.mark.parametrize("name", sorted(TABLE))
def test_null_handles_are_refused_in_the_recorded_words(name):
    assert observe(name, null_args(name)) == TABLE[name][0]


@pytest.fixture(scope="module")
def valid():
    return Valid()


@pytest.mark.parametrize("name", sorted(n for n in TABLE if TABLE[n][1] is not None))
def test_a_null_context_is_refused_when_everything_else_is_valid(name, valid):
    assert observe(name, valid.args(name)) == TABLE[name][1]


def test_the_device_math_probe_takes_no_handle_and_refuses_null_pointers_in_its_own_words():
    """emgpu_debug_device_math has neither a context nor a model among its parameters (device pointers and a stream, like the paired-tracks
    entry points), so TABLE, which is HANDLES by construction, cannot hold it; every pointer NULL and every integer 0 is function 0 on no
    input at all: refused, with a message, before any device work (tests/test_device_math.py has every other refusal)."""
    name = "emgpu_debug_device_math"
    assert name in L.SYMBOLS and name not in HANDLES and name not in TABLE
    f = getattr(L.lib(), name)
    args = [t(0) if t in INTS else None for t in f.argtypes]
    assert len(args) == 6 and observe(name, args) == (L.ERR_ARG, b"null argument: x")


def test_the_sampling_and_track_entry_points_say_null_argument():
    """The entry points that open with CTX_DEVICE refuse a null context together with their other pointers, in those words; CTX_ENTER's
    "null ctx" is for the three emgpu_ctx_* calls and the units that check their arguments first (trace, memory)."""
    for name in ("emgpu_sample_dbn_device", "emgpu_sample_dbn_blocks_device", "emgpu_sample_dbn_multi_device", "emgpu_sample_dbn_multi_host",
                 "emgpu_sample_bn_device", "emgpu_sample_bn_host", "emgpu_propagate_terminal_device", "emgpu_propagate_terminal_host",
                 "emgpu_sample_terminal_device", "emgpu_track_terminal_host", "emgpu_sample2track_device", "emgpu_sample2track_host",
                 "emgpu_track_uncor_device", "emgpu_track_uncor_host", "emgpu_track_uncor_grid_device", "emgpu_track_uncor_grid_host",
                 "emgpu_debug_terminal_counters"):
        assert TABLE[name] == ((L.ERR_ARG, NA), (L.ERR_ARG, NA)), name
    for name in ("emgpu_ctx_sync", "emgpu_ctx_trim", "emgpu_ctx_set_stream"):
        assert TABLE[name] == ((L.ERR_ARG, CTX), (L.ERR_ARG, CTX)), name
    assert TABLE["emgpu_debug_uncor_dynamics_host"][0] == (L.ERR_ARG, b"bad argument")
    assert TABLE["emgpu_last_kernel_name"][0] == (b"", None) and TABLE["emgpu_last_launch_count"][0] == (0, None)
