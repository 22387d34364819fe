"""The surface of em_model_manned_bayes_amd.native is what the single module native.py defined before it became a package: every function,
class and constant, callables with their signatures.  The table was generated once from that module (inspect.signature of every
module-level function and class defined there, None for a constant; imported modules left out) and is kept here as text."""
import ast
import importlib
import inspect
import os
import subprocess
import sys

import pytest

from em_model_manned_bayes_amd import native

SURFACE = [
    ('EVENT_DTYPE', None),
    ('_p', '(a)'),
    ('NativeModel', '(handle)'),
    ('Context', '(device=0, stream=None)'),
    ('_host_free', '(ctx, addr)'),
    ('Trace', '(ctx, model, params, want=3, candidates=0)'),
    ('_default_ctx', None),
    ('default_context', '(device=0)'),
    ('all_device_contexts', '()'),
    ('make_params', '(n, sample_time, seed, first_index=0, transition_mode=0, flags=0, max_attempts=1000, idx_L=0, idx_v=0, idx_dh=0, layers=None, event_cap=0, indices=None, start=None)'),
    ('device_count', '()'),
    ('shard_range', '(n_total, rank, world)'),
    ('_sample_out', '(init_bin=0, init_val=0, dyn_bin=0, dyn_val=0, ev_count=0, events=0, attempts=0, ld=0, col_offset=0, log_weight=0)'),
    ('sample_dbn_device', '(ctx, model, params, init_bin=0, init_val=0, dyn_bin=0, dyn_val=0, ev_count=0, events=0, attempts=0, ld=0, col_offset=0, log_weight=0)'),
    ('mixed_blocks', '(n_total, n_models, lo=0, hi=None)'),
    ('sample_dbn_blocks_device', '(ctx, models, params, blocks, **ptrs)'),
    ('sample_dbn_multi_device', '(ctxs, model, params, outs)'),
    ('sample_dbn_host', '(ctx, model, n, sample_time, seed, want_dense=True, want_events=False, event_cap=None, want_log_weight=False, pinned=True, raw=False, **kw)'),
    ('_event_cap_error', '(rc, totals, ev_count=None)'),
    ('sample_uncor_host', '(ctx, model, n, sample_time, seed, ctrl_var, event_cap=256, events_cap=None, controls_cap=None, want_samples=True, pinned=True, **kw)'),
    ('text_bound', '(model, n, sample_time)'),
    ('sample_text_host', '(ctx, model, n, sample_time, seed, id_first=1, want_arrays=True, pinned=True, initial_cap=None, transition_cap=None, buffers=None, raw=False, **kw)'),
    ('format_g', '(ctx, x, cap=None, return_paths=False)'),
    ('split_rows', '(a, ends)'),
    ('unpack_dyn_bin', '(db, T)'),
    ('unpack_dyn_val', '(dv, T)'),
    ('pack_dyn_bin', '(db)'),
    ('score_params', '(n, sample_time, transition_mode=0, ld=0, col_offset=0)'),
    ('score_dbn_device', '(ctx, model, params, init_bin, dyn_bin=0, log_lik=0, initial=0)'),
    ('_bin_arrays', '(model, init_bin, dyn_bin, T, raw, n, col_offset)'),
    ('_raise', '(rc, **carried)'),
    ('score_dbn_host', '(ctx, model, init_bin, dyn_bin, T, transition_mode=0, raw=False, n=None, col_offset=0)'),
    ('count_dbn_device', '(ctx, model, params, init_bin, dyn_bin=0, counts_initial=0, counts_transition=0)'),
    ('split_counts', '(model, raw)'),
    ('_counts_arrays', '(model, counts)'),
    ('_counts_result', '(model, ci, ct, pairs=None, **kernels)'),
    ('_device_arrays', '(ctx, **nbytes)'),
    ('count_dbn_host', '(ctx, model, init_bin, dyn_bin, T, transition_mode=0, raw=False, n=None, col_offset=0, counts=None)'),
    ('_count_host', '(ctx, model, init_bin, dyn_bin, T, weights, transition_mode, raw, n, col_offset, counts)'),
    ('sample_count_host', '(ctx, model, n, T, seed, transition_mode=0, first_index=0, counts=None)'),
    ('count_dbn_weighted_device', '(ctx, model, params, init_bin, dyn_bin, weights, counts_initial=0, counts_transition=0)'),
    ('_weights_array', '(weights, n)'),
    ('count_dbn_weighted_host', '(ctx, model, init_bin, dyn_bin, T, weights, transition_mode=0, raw=False, n=None, col_offset=0, counts=None)'),
    ('quantize_weights', '(log_w, bits=24, keep=None)'),
    ('reweight_count_host', '(ctx, proposal, target, n, T, seed, bits=24, transition_mode=0, first_index=0, counts=None)'),
    ('pack_dyn_val', '(dv)'),
    ('wrap_mask', '(wrap)'),
    ('discretize_params', '(n, sample_time, n_fine=0, value_type=0, wrap=None, ld=0, col_offset=0)'),
    ('discretize_dbn_device', '(ctx, model, params, init_val=0, dyn_val=0, init_bin=0, dyn_bin=0, repeat=0, change=0)'),
    ('_value_arrays', '(model, init_val, dyn_val, T, raw)'),
    ('_pair_vectors', '(model, counts)'),
    ('discretize_dbn_host', '(ctx, model, init_val, dyn_val, T, n_fine=0, wrap=None, raw=False, n=None, col_offset=0, counts=None)'),
    ('_discretize_count_in_block', '(ctx, model, at, n, T, n_fine, value_type, wrap, transition_mode, dense, **kernels)'),
    ('_discretize_count_bytes', '(model, n, T, dense)'),
    ('discretize_count_host', '(ctx, model, init_val, dyn_val, n_fine=0, wrap=None, transition_mode=0)'),
    ('track_values_params', '(n, points, ur_speed, ur_vertrate, ur_heading, n_initial=5, nd=3, rows=(0, 1, 2, 3, 4), slots=(0, 1, 2), value_type=0, layout=1, ld=0, col_offset=0)'),
    ('track_values_device', '(ctx, params, xyz, init_val=0, dyn_val=0)'),
    ('_track_array', '(xyz)'),
    ('_fill_static', '(iv, static, written)'),
    ('track_values_host', '(ctx, xyz, ur_speed, ur_vertrate, ur_heading, n_initial=5, nd=3, rows=(0, 1, 2, 3, 4), slots=(0, 1, 2), value_type=0, raw=False, static=None, want_init=True, want_dyn=True)'),
    ('track_rows', '(model, variables)'),
    ('track_count_host', '(ctx, model, xyz, rows, static=None, n_fine=4, wrap=None, transition_mode=0, unit_ratios=(1.6878098571011957, 0.016666666666666666, 1.0), value_type=1)'),
    ('miss_params', '(n_pairs, n_a, n_b, points, nmac_h_ft=500.0, nmac_v_ft=100.0, ld_a=0, ld_b=0)'),
    ('miss_distance_device', '(params, xyz_a, xyz_b, idx_a=0, idx_b=0, pose_b=0, weights=0, hmd=0, vmd=0, t_cpa=0, flags=0, totals=0, stream=None)'),
    ('make_pose', '(heading_deg, ox=0.0, oy=0.0, oz=0.0)'),
    ('_planar_tracks', '(xyz, layout, dev)'),
    ('_pair_columns', '(xyz_a, xyz_b, idx_a, idx_b, layout)'),
    ('_paired', '(xyz_a, xyz_b, columns, w, pose_b, layout, ctx, stream)'),
    ('_ptr', '(t)'),
    ('_miss_tensors', '(pr, d_pose, d_w, nmac_h_ft, nmac_v_ft)'),
    ('_miss_dict', '(hmd, vmd, t_cpa, flags, totals)'),
    ('_encounter_pose_tensors', '(pr, want_weights, radius_ft, half_height_ft, seed, rate_scale, first_index, max_attempts)'),
    ('_encounter_dict', "(rate, flags, w_out, flags_key='flags')"),
    ('_encounter_weights', '(weights, rate_scale, n_pairs)'),
    ('miss_distance', "(xyz_a, xyz_b, idx_a=None, idx_b=None, pose_b=None, weights=None, nmac_h_ft=500.0, nmac_v_ft=100.0, layout='rows', ctx=None, stream=None)"),
    ('encounter_params', '(n_pairs, n_a, n_b, points, radius_ft, half_height_ft, seed, first_index=0, max_attempts=16, rate_scale=1.0, ld_a=0, ld_b=0)'),
    ('encounter_pose_device', '(params, xyz_a, xyz_b, idx_a=0, idx_b=0, weights_in=0, pose=0, rate=0, flags=0, weights_out=0, stream=None)'),
    ('encounter_pose', "(xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a=None, idx_b=None, weights=None, rate_scale=None, first_index=0, max_attempts=16, layout='rows', ctx=None, stream=None)"),
    ('encounter_miss', "(xyz_a, xyz_b, radius_ft, half_height_ft, seed, idx_a=None, idx_b=None, weights=None, rate_scale=None, first_index=0, max_attempts=16, nmac_h_ft=500.0, nmac_v_ft=100.0, layout='rows', ctx=None, stream=None)"),
    ('device_upload', '(ctx, addr, src)'),
    ('device_download', '(ctx, addr, out)'),
    ('_same_shape', '(a, b)'),
    ('sample_weighted_host', '(ctx, proposal, target, n, T, seed, raw=False, want_log_weight=False, first_index=0, transition_mode=0, flags=0, max_attempts=1000, idx_L=0, idx_v=0, idx_dh=0, layers=None, indices=None, start=None)'),
    ('sample_bn_host', '(ctx, model, n, seed, first_index=0, dediscretize=False, max_attempts=100000, bounds_sample=None, idx_own_speed=0, idx_int_speed=0, lim1=(0.0, inf), lim2=(0.0, inf), start=None, want_log_weight=False)'),
    ('terminal_t0_row', '(cap)'),
    ('propagate_terminal_joined_host', '(ctx, models, geo, model_of, seed, first_index=0, tmax_s=120.0, dyn_limits=None, max_resample=100000, cap=None, local_smooth=False)'),
    ('split_joined_tracks', '(traj, rows, cap)'),
    ('propagate_terminal_host', '(ctx, models, geo, model_of, seed, first_index=0, tmax_s=120.0, dyn_limits=None, max_resample=100000, cap=None, local_smooth=False)'),
    ('utrack_params', '(model, n, sample_time, seed, first_index=0, is_quantize500=False, is_rotorcraft=False, max_track_attempts=200, max_attempts=1000, record_stride=1)'),
    ('start_grid_log_weight', '(model, grid)'),
    ('track_uncor_host', '(ctx, model, n, sample_time, seed, want_tracks=True, start=None, **kw)'),
    ('track_uncor_device', '(ctx, model, n, sample_time, seed, tracks=0, limits=0, attempts=0, start=0, **kw)'),
    ('uncor_dynamic_limits', '(model, initial, up_min, up_max, speed_min, speed_max, is_rotorcraft=False)'),
    ('TERMINAL_GEO_FIELDS', None),
    ('_fill_terminal', '(p, geom_model, n, seed, first_index, tmax_s, dyn_limits, bounds_sample, max_attempts, max_resample, local_smooth)'),
    ('terminal_sample_params', '(geom_model, n, seed, dyn_limits, first_index=0, tmax_s=120.0, cap=None, bounds_sample=None, max_attempts=100000, max_resample=100000, local_smooth=False)'),
    ('sample_terminal_device', '(ctx, geom_model, traj_models, p, geom_val, geo, model_of, traj, rows, geom_bin=0, attempts=0)'),
    ('track_terminal_host', '(ctx, geom_model, traj_models, n, seed, dyn_limits, max_cum_turn_deg, pitch_deg, first_index=0, tmax_s=120.0, min_enc_time_s=30.0, thres_dist_ft=15190.0, thres_alt_low_ft=750.0, thres_vertrate_ft_s=5.0, bounds_sample=None, max_track_attempts=500, max_attempts=100000, max_resample=100000, allow_cap=False, local_smooth=True, want_traj=True)'),
    ('track_params', '(n, T, ur_speed, ur_vertrate, ur_heading, min_speed, max_speed, nd=0, slot_vertrate=0, slot_acc=0, slot_turnrate=0)'),
    ('sample2track_host', '(ctx, alt0, speed0, updates, ur_speed, ur_vertrate, ur_heading, min_speed, max_speed)'),
    ('_buffer_address', '(data)'),
    ('_LINE', None),
    ('_parse_error', '(rc, header_lines, what)'),
    ('parse_table', '(ctx, data, ncol, return_stats=False, header_lines=0, rows_cap=None)'),
    ('format_f0', '(ctx, x, cap=None)'),
    ('csv_bound', '(n, rows)'),
    ('tracks_text_host', '(ctx, text, ncol, cols, ids, alt0, speed0, ur_speed, ur_vertrate, ur_heading, min_speed, max_speed, want_csv=True, csv=None, csv_cap=None, want_xyz=False, header_lines=1)'),
    ('sample2track_device', '(ctx, params, alt0, speed0, dyn_val, xyz=0, flags=0, speed_minmax=0)'),
]

# one way only: a module imports from the modules of the rows above its own, never from its own row or below
ORDER = [("base",), ("layout",), ("sampling", "text"), ("trace", "tracks", "pairs")]
PACKAGE_DIR = os.path.dirname(native.__file__)


@pytest.mark.parametrize("name,signature", SURFACE, ids=[n for n, _ in SURFACE])
def test_name_is_an_attribute_with_the_parents_signature(name, signature):
    assert hasattr(native, name), "native.%s is gone" % name
    obj = getattr(native, name)
    if signature is None:
        assert not inspect.isfunction(obj) and not inspect.isclass(obj)
    else:
        assert callable(obj)
        assert str(inspect.signature(obj)) == signature


def test_the_table_is_complete_enough_to_matter():
    assert len(SURFACE) == 108 and len({n for n, _ in SURFACE}) == 108


def test_init_only_re_exports():
    with open(os.path.join(PACKAGE_DIR, "__init__.py")) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        is_doc = isinstance(node, ast.Expr) and isinstance(node.value, ast.Constant) and isinstance(node.value.value, str)
        assert is_doc or isinstance(node, ast.ImportFrom), "native/__init__.py defines something: line %d" % node.lineno
    for name, obj in vars(native).items():
        if inspect.isfunction(obj) or inspect.isclass(obj):
            assert obj.__module__ != native.__name__, name


def _package_imports(module):
    """the modules of the package that `module` imports at module level"""
    with open(os.path.join(PACKAGE_DIR, module + ".py")) as f:
        tree = ast.parse(f.read())
    return {node.module for node in ast.walk(tree) if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module}


def test_every_module_is_in_the_order_and_imports_upwards_only():
    modules = sorted(f[:-3] for f in os.listdir(PACKAGE_DIR) if f.endswith(".py") and f != "__init__.py")
    assert modules == sorted(m for row in ORDER for m in row)
    for i, row in enumerate(ORDER):
        above = {m for r in ORDER[:i] for m in r}
        for module in row:
            assert _package_imports(module) <= above, module


@pytest.mark.parametrize("module", [m for row in reversed(ORDER) for m in row])
def test_module_imports_first_in_a_fresh_interpreter(module):
    """a leaf imported before anything else of the package's modules: a cycle would fail here"""
    root = os.path.dirname(os.path.dirname(PACKAGE_DIR))
    code = "import importlib, sys; sys.path.insert(0, %r); importlib.import_module(%r)" % (root, native.__name__ + "." + module)
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_em_io_takes_the_model_class_from_the_package():
    em_io = importlib.import_module("em_model_manned_bayes_amd.em_io")
    assert em_io.NativeModel is native.NativeModel
