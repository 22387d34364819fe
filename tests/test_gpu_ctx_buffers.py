"""-m gpu: the three device buffers a context grows on demand (ctx_grow in emgpu_ctx.cpp) -- the layer table of a DBN call (d_layers), the
trajectory models' table pointers of a terminal call (d_thr_base) and the scratch slots of the round drivers -- each through a small, a
large and the small call again on ONE long-lived context: the buffer is allocated, grown exactly once, then reused while larger than
needed.  Every call is repeated on a fresh native.Context(0), which has nothing to reuse; the two are the same code on the same device, so
the raw arrays are compared with array_equal and no tolerance enters.

(What a failed hipMalloc inside a grow leaves behind is argued from the code in HISTORY.md, not provoked here.)"""
import numpy as np
import pytest

import terminal_shapes as S
from em_model_manned_bayes_amd import native, _lib as L
from test_gpu_track_rounds import NAME, N, T, STRIDE, SEED, UNCOR_KERNELS, uncor_host
from util import load_pair, terminal_hand_geo, terminal_hand_limits, terminal_shape_models, uncor_indices, write_terminal_shape_directory

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kept():
    """The long-lived context: this module's own, so that its buffers start empty."""
    ctx = native.Context(0)
    yield ctx
    close(ctx)


def close(ctx):
    L.lib().emgpu_ctx_free(ctx._h)
    ctx._h = None


def on_a_fresh_context(call):
    ctx = native.Context(0)
    try:
        return call(ctx)
    finally:
        close(ctx)


def assert_same(a, b, what):
    """Two results of one call, dicts or tuples of arrays, strings and numbers: equal item for item, arrays bit for bit."""
    items = sorted(a) if isinstance(a, dict) else range(len(a))
    assert len(a) == len(b), what
    for k in items:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def small_large_small(kept, small, large, what):
    """small, large, small on the kept context, each against the same call on a fresh one; returns the kept context's three results."""
    out = []
    for step, call in (("small", small), ("large", large), ("small again", small)):
        got = call(kept)
        assert_same(got, on_a_fresh_context(call), "%s, %s" % (what, step))
        out.append(got)
    assert_same(out[0], out[2], what + ", small against small again")
    return out


def test_the_layer_table_grows_once_and_is_reused(kept, model_dir):
    """d_layers: the four rows of test_start_presets_prior_layers_quantize, then the same four followed by four more (only the first r_L
    rows are read: the draws are the four-row call's), then the four again in a buffer that holds eight."""
    nm, pp, _ = load_pair("uncor_1200only_fwse_v1p2", model_dir, is_overwrite_zero_boundaries=True)
    idx = uncor_indices(pp)
    four = np.array([[50, 500], [500, 1200], [1200, 3000], [3000, 5000]], dtype=np.float64)
    eight = np.concatenate([four, [[5000, 8000], [8000, 12000], [12000, 18000], [18000, 29000]]])

    def call(layers):
        def run(ctx):
            got = native.sample_dbn_host(ctx, nm, 64, 8, 5, want_dense=True, want_events=True, pinned=False, raw=True, layers=layers, **idx)
            del got["host_stats"], got["events"]            # (timings; events_flat holds the same rows as one array)
            return got
        return run
    first, longer, _ = small_large_small(kept, call(four), call(eight), "d_layers")
    assert_same(first, longer, "d_layers, four rows against eight")
    assert first["kernel"].startswith("k_uncor_fast"), first["kernel"]
    assert (first["attempts"] >= 1).all() and first["ev_count"].sum() > 0 and np.isfinite(first["init_val"]).all()


def test_the_table_pointers_grow_once_and_are_reused(kept, tmp_path):
    """d_thr_base: a set of one trajectory model (model_of all 0), the ten of terminal_shapes' first row, the one again."""
    d = write_terminal_shape_directory(str(tmp_path / "shape"), **S.ROWS[0]["spec"])
    nms, _, _ = terminal_shape_models(d)
    geo, mo = terminal_hand_geo(8)
    dl = terminal_hand_limits("generic")

    def call(models, model_of):
        def run(ctx):
            traj, rows = native.propagate_terminal_joined_host(ctx, models, geo, model_of, 0x5EED0014, dyn_limits=dl)
            return traj, rows, ctx.last_kernel()
        return run
    one, ten, _ = small_large_small(kept, call(nms[:1], np.zeros_like(mo)), call(nms, mo), "d_thr_base")
    assert one[2] == ten[2] == S.ROWS[0]["kernel"], (one[2], ten[2])
    for traj, rows, _ in (one, ten):
        assert rows.shape == (32,) and (rows >= 1).any() and np.isfinite(traj).all() and np.abs(traj).max() > 0


def test_the_scratch_slots_grow_once_and_are_reused(kept, model_dir):
    """The round drivers' scratch: emgpu_track_uncor_host at n = 64, then the n = 257 of test_gpu_track_rounds.py, whose three rounds touch
    every slot (both halves of the index / slot ping-pong included), then n = 64 in slots that hold 257."""
    nm, _, _ = load_pair(NAME, model_dir)

    def call(n):
        def run(ctx):
            rc, _, tracks, limits, att, kernel = uncor_host(ctx, nm, n, 0, 200)   # (the message of a call that succeeded is an earlier call's)
            return rc, tracks, limits, att, kernel
        return run
    small, large, _ = small_large_small(kept, call(64), call(N), "scratch slots")
    for rc, tracks, limits, att, kernel in (small, large):
        assert rc == L.OK and kernel == UNCOR_KERNELS, (rc, kernel)
        assert not np.isnan(tracks).any() and not np.isnan(limits).any() and att.min() >= 1
    assert large[3].max() == 3 and (T, STRIDE, SEED) == (30, 10, 0xC0DE)            # three rounds ran
    assert_same(tuple(x[:64] if isinstance(x, np.ndarray) else x for x in large), small, "scratch slots, the first 64 lanes of 257")
