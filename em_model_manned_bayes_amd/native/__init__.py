"""Thin object layer over the C ABI: NativeModel (emgpu_model*), Context (emgpu_ctx*) and the
sampling calls with numpy (host) or raw device pointers (torch tensors' data_ptr()).

One module per owner, imports one way: base <- layout <- sampling, text <- trace, tracks, pairs.  This file only re-exports: a caller
writes native.X, and looks X up at call time.
"""
# flake8: noqa: F401
from .. import _lib as L
from .base import (EVENT_DTYPE, Context, NativeModel, Trace, _array_factory, _default_ctx, _device_arrays, _device_call, _error,
                   _event_cap_error, _host_free, _last_message, _p, _raise, _stream_handle, _weights_array, all_device_contexts,
                   default_context, device_count, device_download, device_upload, make_params, shard_range)
from .layout import TraceLayout, pack_dyn_bin, pack_dyn_val, split_rows, unpack_dyn_bin, unpack_dyn_val
from .sampling import (TERMINAL_GEO_FIELDS, _fill_terminal, _same_shape, _sample_out, mixed_blocks, sample_bn_host,
                       sample_dbn_blocks_device, sample_dbn_device, sample_dbn_host, sample_dbn_multi_device, sample_terminal_device,
                       sample_uncor_host, start_grid_log_weight, terminal_sample_params)
from .text import _LINE, _buffer_address, _parse_error, csv_bound, format_f0, format_g, parse_table, sample_text_host, text_bound
from .trace import (_bin_arrays, _count_bytes, _count_host, _count_scope, _counts_arrays, _counts_result, _discretize_count_bytes,
                    _discretize_count_in_block, _fill_static, _pair_vectors, _sample_in_block, _track_array, _value_arrays,
                    count_dbn_device, count_dbn_host, count_dbn_weighted_device, count_dbn_weighted_host, discretize_count_host,
                    discretize_dbn_device, discretize_dbn_host, discretize_params, quantize_weights, reweight_count_host,
                    sample_count_host, sample_weighted_host, score_dbn_device, score_dbn_host, score_params, split_counts,
                    track_count_host, track_rows, track_values_device, track_values_host, track_values_params, wrap_mask)
from .tracks import (filter_terminal_device, propagate_terminal_host, propagate_terminal_joined_host, sample2track_device,
                     sample2track_host, smooth_terminal_device, split_joined_tracks, terminal_filter_params, terminal_t0_row, track_params,
                     track_terminal_host, track_uncor_device, track_uncor_host, tracks_text_host, uncor_dynamic_limits, utrack_params)
from .pairs import (_avoid_dict, _avoid_tensors, _cpa_dict, _cpa_pose_tensors, _encounter_dict, _encounter_pose_tensors, _encounter_weights,
                    _miss_dict, _miss_segments_dict, _miss_segments_tensors, _miss_tensors, _miss_then_well_clear, _pair_columns, _paired,
                    _placed_then, _planar_tracks, _ptr, _well_clear_dict, _well_clear_tensors, avoid, avoid_device, avoid_params, cpa_avoid,
                    cpa_miss, cpa_miss_segments, cpa_pose, cpa_pose_device, cpa_pose_params, cpa_well_clear, encounter_avoid,
                    encounter_miss, encounter_miss_segments, encounter_params,
                    encounter_pose, encounter_pose_device, encounter_well_clear, make_pose, miss_distance, miss_distance_device, miss_params,
                    miss_segments, miss_segments_device, well_clear, well_clear_device, well_clear_params)
