"""GPU: k_terminal_propagate on the trajectory-model shapes of terminal_shapes.py against the oracle -- both kernel instances, every
row-length class of t_draw3, the discretize walks on non-uniform grids, coarse and one-sided bearing grids, aircraft that stay on a
cut direction, the launcher's choice of instance from both sides, the re-draw cap and the refusals of terminal_tables.
The bar is the one of test_gpu_parity.py's terminal tests: track lengths equal, every value of every track the oracle's f64 rounded to
f32 or one f32 step (util.assert_f32_of_f64), and NO track left out."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import em_model_manned_bayes_amd as E
import oracle as O
import terminal_shapes as S
from em_model_manned_bayes_amd import _lib as L, native
from util import (TERMINAL_LIMITS, assert_f32_of_f64, assert_parting_only_on_a_threshold, terminal_hand_geo, terminal_hand_limits, terminal_refusal_variants,
                  terminal_shape_models, write_terminal_shape_directory)

pytestmark = pytest.mark.gpu

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0014


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """id -> (directory, native models, oracle models) of a row, written and loaded once per module."""
    made = {}

    def get(row_id):
        if row_id not in made:
            d = write_terminal_shape_directory(str(tmp_path_factory.mktemp("shape_" + row_id)), **S.by_id(row_id)["spec"])
            nms, oms, _ = terminal_shape_models(d)
            made[row_id] = (d, nms, oms)
        return made[row_id]
    return get


@pytest.fixture(scope="module")
def geometry(tmp_path_factory, gpu_ctx):
    """n -> (geo [n, 12], model_of [n, 4]): the first half from CorTerminalModel.sample's geometry model (drawn on the GPU, like the other
    terminal tests), the second half the hand-made rows on the axes."""
    from em_model_manned_bayes_amd import em_io
    d = str(tmp_path_factory.mktemp("geometry_only"))
    em_io.materialize_model("terminal_v3_radar_encounter_model", d)
    t = E.CorTerminalModel(srcData="terminalradar", parameters_directory=d)
    made = {}

    def get(n):
        if n not in made:
            _, samples = t.sample(n // 2, seed=SEED, ctx=gpu_ctx)
            g, mo = t._geo_rows(samples)
            mo = np.array([[2 * (int(s["own_intent"]) - 1), 2 * (int(s["own_intent"]) - 1) + 1, 4 + 2 * (int(s["int_intent"]) - 1),
                            4 + 2 * (int(s["int_intent"]) - 1) + 1] for s in samples], dtype=np.int32)     # every intent with its own reverse model
            hg, hmo = terminal_hand_geo(n - n // 2)
            made[n] = (np.concatenate([g, hg]), np.concatenate([mo, hmo]))
        return made[n]
    return get


def propagate_both(ctx, nms, oms, geo, mo, seed, limits, first_index=0, max_resample=100000):
    """The library and the oracle on a geometry(n) batch under a limit pair of util.TERMINAL_LIMITS: the sampled half under the pair, the
    hand-made half under the same pair with its own turn limits (util.TERMINAL_HAND_TURN says why) -- two calls each, every track of both
    kept.  Returns (got, rows, ref, ref_rows, kernel names)."""
    h = geo.shape[0] // 2
    out, names = [], []
    for sl, first, dl in ((slice(0, h), first_index, TERMINAL_LIMITS[limits]), (slice(h, None), first_index + h, terminal_hand_limits(limits))):
        ref, ref_rows = O.propagate(oms, mo[sl], geo[sl], seed, dl, first_index=first, tmax_s=120.0, max_resample=max_resample)
        got, rows = native.propagate_terminal_host(ctx, nms, geo[sl], mo[sl], seed, first_index=first, tmax_s=120.0, dyn_limits=dl, max_resample=max_resample)
        names.append(ctx.last_kernel())
        out.append((got, rows, ref, ref_rows))
    return tuple(np.concatenate([o[i] for o in out]) for i in range(4)) + (names,)


def assert_tracks_equal(got, rows, ref, ref_rows, what):
    """Every track, none excluded: the same length, every value within one f32 step of the oracle's."""
    assert np.array_equal(rows, ref_rows), "%s: track lengths differ at %s" % (what, np.flatnonzero(rows != ref_rows)[:10])
    worst = 0
    for q in range(rows.size):
        worst = max(worst, assert_f32_of_f64(got[q, :rows[q]], ref[q, :rows[q]], "%s track %d" % (what, q)))
    return worst


@pytest.mark.parametrize("limits", sorted(TERMINAL_LIMITS))
@pytest.mark.parametrize("row", S.ROWS, ids=lambda r: r["id"])
def test_propagation_matches_oracle_on_every_shape(row, limits, shapes, geometry, gpu_ctx):
    _, nms, oms = shapes(row["id"])
    geo, mo = geometry(320)
    got, rows, ref, ref_rows, names = propagate_both(gpu_ctx, nms, oms, geo, mo, SEED, limits)
    assert names == [row["kernel"]] * 2
    assert rows.min() >= 1 and rows.max() == 121 and rows.min() <= 3
    worst = assert_tracks_equal(got, rows, ref, ref_rows, "%s / %s" % (row["id"], limits))
    print("%s / %s: %d tracks, %d rows, worst %d f32 step(s), excluded 0" % (row["id"], limits, rows.size, int(rows.sum()), worst))


@pytest.mark.parametrize("row_id", ["shipped", "mid"])
def test_turns_above_the_small_angle_branch(row_id, shapes, geometry, gpu_ctx):
    """maxTurnRate = 400: nothing limits a turn, so the velocity is rotated by up to 360 degrees in one step -- the kernel's
    full-evaluation branch for turns above 12.5 degrees, which no aircraft type's limit reaches.  Sampled geometry only: from an
    axis-aligned heading an unlimited turn (rounded to 0.01 degrees) can land on 360.00 exactly, where the reference's heading is 0 or
    360 by the sign of a 1e-14 velocity component."""
    _, nms, oms = shapes(row_id)
    geo, mo = geometry(320)
    h = geo.shape[0] // 2
    dl = TERMINAL_LIMITS["inside"].copy()
    dl[:, 2] = 400.0
    ref, ref_rows = O.propagate(oms, mo[:h], geo[:h], SEED + 2, dl, tmax_s=120.0)
    got, rows = native.propagate_terminal_host(gpu_ctx, nms, geo[:h], mo[:h], SEED + 2, tmax_s=120.0, dyn_limits=dl)
    assert gpu_ctx.last_kernel() == S.by_id(row_id)["kernel"]
    turn = np.abs(np.diff(ref[:, :, 4], axis=1))
    assert ((turn > 12.5) & (turn < 347.5)).any()                  # such turns are there
    assert_tracks_equal(got, rows, ref, ref_rows, row_id + " / turn 400")


@pytest.mark.parametrize("edge", S.EDGES, ids=lambda e: e[1])
def test_both_sides_of_every_launcher_edge(edge, shapes, geometry, gpu_ctx):
    """launch_terminal_propagate's choice (36/7/5 bins, at most 8 cut points of distance / altitude / speed) from both sides: each side
    runs the instance it must, on another batch than the per-row test, and equals the oracle."""
    what, lo, hi = edge
    geo, mo = geometry(120)
    names = []
    for row_id in (lo, hi) if hi else (lo,):
        _, nms, oms = shapes(row_id)
        got, rows, ref, ref_rows, kn = propagate_both(gpu_ctx, nms, oms, geo, mo, SEED + 1, "inside", first_index=1000)
        assert kn[0] == kn[1]
        names.append(kn[0])
        assert_tracks_equal(got, rows, ref, ref_rows, "%s: %s" % (what, row_id))
    assert names == ([S.SHIPPED, S.GENERIC] if hi else [S.SHIPPED]), (what, names)


def test_the_run_time_shape_instance_on_the_second_graph(shapes, geometry, tmp_path):
    """k_terminal_propagate<0,0,0> on the 36/7/5 shape with the intent as a parent (a child process with EMGPU_DEBUG_TERM_GENERIC): the
    instance a trained file of the guessed shape but another graph would still NOT get -- and must equal, draw for draw."""
    d, _, _ = shapes("shipped_intent")
    geo, mo = geometry(320)
    np.savez(str(tmp_path / "geo.npz"), geo=geo, mo=mo)
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import oracle as O
from em_model_manned_bayes_amd import native
from util import TERMINAL_LIMITS, assert_f32_of_f64, terminal_hand_limits, terminal_shape_models
ctx = native.Context(0)
nms, oms, _ = terminal_shape_models(%r)
g = np.load(%r)
h = g["geo"].shape[0] // 2
for name in sorted(TERMINAL_LIMITS):
    for sl, first, dl in ((slice(0, h), 0, TERMINAL_LIMITS[name]), (slice(h, None), h, terminal_hand_limits(name))):
        ref, ref_rows = O.propagate(oms, g["mo"][sl], g["geo"][sl], 77, dl, first_index=first, tmax_s=120.0)
        got, rows = native.propagate_terminal_host(ctx, nms, g["geo"][sl], g["mo"][sl], 77, first_index=first, tmax_s=120.0, dyn_limits=dl)
        assert ctx.last_kernel() == "k_terminal_propagate", ctx.last_kernel()
        assert np.array_equal(rows, ref_rows)
        for q in range(rows.size):
            assert_f32_of_f64(got[q, :rows[q]], ref[q, :rows[q]], name + " track " + str(first * 4 + q))
print("generic ok")
''' % (ROOT_DIR, os.path.join(ROOT_DIR, "tests"), os.path.join(ROOT_DIR, "oracle"), d, str(tmp_path / "geo.npz"))
    env = dict(os.environ, EMGPU_DEBUG_TERM_GENERIC="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "generic ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("row_id", ["h64", "tiny"])
def test_exactly_the_span_of_every_track_is_written(row_id, shapes, geometry):
    """emgpu_propagate_terminal_device into a NaN-filled buffer, on a long-row and a short-row shape: after the call rows
    C - (rb - 1) .. C + (rf - 1) of every aircraft's block are written and nothing else (the masked loads past a row's end and the
    flush of the run-time-shape instance must not reach outside), and the written rows are the oracle's."""
    import torch
    _, nms, oms = shapes(row_id)
    g, mo = geometry(320)
    dev = torch.device("cuda", 0)
    ctx = native.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    reps, cap = 64, 123
    n = reps * g.shape[0]
    geo = torch.tensor(np.tile(g, (reps, 1)), device=dev)
    mof = torch.tensor(np.tile(mo, (reps, 1)).reshape(-1), dtype=torch.int32, device=dev)
    c0 = native.terminal_t0_row(cap)
    W = 2 * c0
    out = torch.full((2 * n, W, 5), float("nan"), dtype=torch.float32, device=dev)
    rows = torch.full((4 * n,), -999, dtype=torch.int32, device=dev)
    dl = TERMINAL_LIMITS["inside"]
    p = L.TermParams()
    p.seed, p.first_index, p.n, p.tmax_s, p.max_resample, p.cap = SEED, 0, n, 120.0, 100000, cap
    for i, v in enumerate(dl.reshape(-1)):
        p.dyn_limits[i] = float(v)
    handles = (C.c_void_p * 10)(*[x._h for x in nms])
    L.check(L.lib().emgpu_propagate_terminal_device(ctx._h, handles, 10, C.byref(p), C.c_void_p(geo.data_ptr()), C.c_void_p(mof.data_ptr()),
                                                    C.c_void_p(out.data_ptr()), C.c_void_p(rows.data_ptr())))
    ctx.sync()
    assert ctx.last_kernel() == S.by_id(row_id)["kernel"]
    assert int(rows.min()) >= 1 and int(rows.max()) == 121
    rf, rb = rows[0::2], rows[1::2]
    r = torch.arange(W, device=dev)[None, :]
    valid = (r >= (c0 - (rb - 1))[:, None]) & (r <= (c0 + (rf - 1))[:, None])
    for field in range(5):
        assert bool(((~torch.isnan(out[:, :, field])) == valid).all()), field
    # the sampled half of the batch's last tile against the oracle (hand-made rows under a turn-rate limit: see util.TERMINAL_HAND_TURN)
    a, b = n - g.shape[0], n - g.shape[0] // 2
    ref, ref_rows = O.propagate(oms, mof[4 * a: 4 * b].cpu().numpy(), geo[a:b].cpu().numpy(), SEED, dl, first_index=a, tmax_s=120.0, cap=cap)
    got_rows = rows[4 * a: 4 * b].cpu().numpy()
    got = native.split_joined_tracks(np.nan_to_num(out[2 * a: 2 * b].cpu().numpy()), got_rows, cap)
    assert_tracks_equal(got, got_rows, ref, ref_rows, row_id)


@pytest.fixture(scope="module")
def other_shape_dir(tmp_path_factory):
    """A directory of a shape other than the guessed one (36/7/6 bins, the run-time-shape instance) whose landing / take-off models drift in
    altitude, so that CorTerminalModel.track's filters accept a good part of the encounters."""
    return write_terminal_shape_directory(str(tmp_path_factory.mktemp("other_shape")), vertical_intent=True, **S.by_id("speed6")["spec"])


@pytest.mark.parametrize("actypes", [("GENERIC", "GENERIC"), ("RTCA228_A3", "TEST")])
def test_fused_terminal_call_matches_oracle_on_another_shape(actypes, other_shape_dir):
    """test_gpu_parity.test_fused_terminal_call_matches_oracle's body on the 36/7/6 directory: emgpu_sample_terminal_device stage by stage."""
    from test_gpu_parity import _FusedTerminal, _terminal_oracle_models
    t = E.CorTerminalModel(srcData="terminalradar", parameters_directory=other_shape_dir)
    t.acType1, t.acType2 = actypes
    n, seed, first = 2000, 0x5EED0005, 12345
    f = _FusedTerminal(t, n, propagate_kernel=S.GENERIC)
    f.run(seed, first)
    om_geom = O.OracleModel(O.parse_model_txt(t.parameters_filename))
    f.check_slice_against_oracle(_terminal_oracle_models(t), om_geom, seed, first, 0, n)
    if actypes[0] != "GENERIC":
        assert int(f.att.max()) > 1


def test_terminal_track_matches_oracle_on_another_shape(other_shape_dir, gpu_ctx):
    """test_gpu_parity.test_terminal_track_matches_oracle's rule, unchanged, on the 36/7/6 directory: every encounter accepts the same
    attempt on both sides unless the oracle's own decision margin of the parting attempt is at rounding level (2^-22)."""
    t = E.CorTerminalModel(srcData="terminalradar", parameters_directory=other_shape_dir)
    gom = O.OracleModel(O.parse_model_txt(t.parameters_filename))
    oms = []
    for m in t._traj:
        pp = O.parse_model_txt(m.parameters_filename)
        oms.append(O.OracleModel(pp, alpha_transition=O.stay_prior_alpha(pp, 1.0)))
    d = (t.dynLimits1, t.dynLimits2)
    cum, pitch = [x["maxCumTurn_deg"] for x in d], [x["pitch_deg"] for x in d]
    n, seed, cap = 600, 0xF2, 150
    ref = O.terminal_track(gom, oms, n, seed, t._dyn_rows(), cum, pitch, first_index=5, max_track_attempts=cap, local_smooth=False)
    got = native.track_terminal_host(gpu_ctx, t.native, [m.native for m in t._traj], n, seed, t._dyn_rows(), cum, pitch, first_index=5,
                                     max_track_attempts=cap, allow_cap=True, local_smooth=False)
    assert "k_terminal_filter" in got["kernel"] and "k_terminal_propagate" in got["kernel"] and "k_terminal_propagate<" not in got["kernel"]
    same = assert_parting_only_on_a_threshold(got["attempts"], ref["attempts"], ref["margins"], 2.0 ** -22, "encounter")
    assert same.sum() >= n - max(2, n // 500), "more threshold coincidences than %d encounters can explain: %d" % (n, (~same).sum())
    ok = same & (ref["attempts"] > 0)
    assert ok.sum() >= n // 5 and (ref["attempts"][ok] > 1).any()
    assert np.array_equal(got["sample"][ok], ref["sample"][ok]) and np.array_equal(got["len"][ok], ref["len"][ok])
    np.testing.assert_allclose(got["meta"][ok], ref["meta"][ok], rtol=1e-5, atol=1e-3)
    for i in np.flatnonzero(ok)[:400]:
        for a in range(2):
            k = ref["len"][i, a]
            assert_f32_of_f64(got["traj"][i, a, :k, 1:], ref["traj"][i, a, :k, 1:], "encounter %d aircraft %d" % (i, a))
            assert np.array_equal(got["traj"][i, a, :k, 0], ref["traj"][i, a, :k, 0])


CAP_SPEC = dict(bins=(4, 5, 6, 8, 4), table="dense", zero_frac=0.02)


def _only_an_invalid_altitude(k, m):
    """Altitude bin 8 (4400 ft and above) as the current value: every such column holds one huge count in bin 7, above both maxAltitude
    limits of TERMINAL_LIMITS["inside"] (bins 1-6 and 1-2 are valid, so only an aircraft that starts up there is caught) -- the stay
    prior's 1 beside it never wins a draw."""
    N = m["N_transition"][7]
    q = N.shape[1]
    own = np.arange(q) // (q // 8)                      # the own value is the slowest-varying parent
    N[:, own == 7] = 0
    N[6, own == 7] = 1.5e9
    return m


def test_the_redraw_cap_is_reported_for_the_tracks_the_oracle_gives_up_on(tmp_path, geometry, gpu_ctx):
    """max_resample = 50 on a model in which an aircraft in the top altitude bin can only draw an invalid altitude: the library reports
    EMGPU_ERR_REJECT_CAP and marks (rows < 0) tracks of exactly the encounters for which the oracle, called one encounter at a time,
    returns -3; every other encounter's tracks equal the oracle's."""
    d = write_terminal_shape_directory(str(tmp_path / "cap"), edit=_only_an_invalid_altitude, **CAP_SPEC)
    nms, oms, _ = terminal_shape_models(d)
    geo, mo = geometry(320)
    n, cap, dl = geo.shape[0], 123, terminal_hand_limits("inside")     # (one call for both halves: the turn limits of the hand-made half)
    p = L.TermParams()
    p.seed, p.first_index, p.n, p.tmax_s, p.max_resample, p.cap = SEED, 0, n, 120.0, 50, cap
    for i, v in enumerate(dl.reshape(-1)):
        p.dyn_limits[i] = float(v)
    handles = (C.c_void_p * 10)(*[x._h for x in nms])
    traj = np.zeros((2 * n, 2 * native.terminal_t0_row(cap), 5), dtype=np.float32)
    rows = np.zeros(4 * n, dtype=np.int32)
    g64, mo32 = np.ascontiguousarray(geo), np.ascontiguousarray(mo.reshape(-1).astype(np.int32))
    rc = L.lib().emgpu_propagate_terminal_host(gpu_ctx._h, handles, 10, C.byref(p), g64.ctypes.data, mo32.ctypes.data, traj.ctypes.data, rows.ctypes.data)
    assert rc == L.ERR_REJECT_CAP, rc
    got = native.split_joined_tracks(traj, rows, cap)
    gave_up = np.zeros(n, dtype=bool)
    for e in range(n):
        try:
            ref, ref_rows = O.propagate(oms, mo[e], geo[e: e + 1], SEED, dl, first_index=e, tmax_s=120.0, max_resample=50, cap=cap)
        except RuntimeError as err:
            assert "rc=-3" in str(err)
            gave_up[e] = True
            continue
        assert_tracks_equal(got[4 * e: 4 * e + 4], rows[4 * e: 4 * e + 4], ref, ref_rows, "encounter %d" % e)
    assert np.array_equal((rows.reshape(n, 4) < 0).any(axis=1), gave_up)
    assert 10 <= gave_up.sum() <= n - 10, gave_up.sum()             # both kinds are there
    # the status is cleared: the same context completes a good call
    with pytest.raises(L.EmgpuError) as ei:
        native.propagate_terminal_host(gpu_ctx, nms, geo, mo, SEED, tmax_s=120.0, dyn_limits=dl, max_resample=50)
    assert ei.value.code == L.ERR_REJECT_CAP
    got, rows, ref, ref_rows, _ = propagate_both(gpu_ctx, nms, oms, geo, mo, SEED, "generic")
    assert_tracks_equal(got, rows, ref, ref_rows, "after the cap")


REFUSAL_SPEC = S.by_id("tiny")["spec"]


@pytest.mark.parametrize("variant", terminal_refusal_variants(REFUSAL_SPEC), ids=lambda v: v[0])
def test_refused_model_sets_give_err_unsupported(variant, tmp_path, shapes, geometry, gpu_ctx):
    """Each refusal of terminal_tables (emgpu_terminal.cpp), provoked by a set of ten loadable files: EMGPU_ERR_UNSUPPORTED with its message,
    from the host-pointer entry point; afterwards the same context completes a good call that equals the oracle."""
    id_, message, edit = variant
    d = write_terminal_shape_directory(str(tmp_path / id_), edit=edit, **REFUSAL_SPEC)
    bad, _, _ = terminal_shape_models(d)
    geo, mo = geometry(120)
    with pytest.raises(L.EmgpuError) as ei:
        native.propagate_terminal_host(gpu_ctx, bad, geo, mo, SEED, tmax_s=120.0, dyn_limits=TERMINAL_LIMITS["generic"])
    assert ei.value.code == L.ERR_UNSUPPORTED and message in str(ei.value), str(ei.value)
    _, nms, oms = shapes("tiny")
    got, rows, ref, ref_rows, _ = propagate_both(gpu_ctx, nms, oms, geo, mo, SEED, "generic")
    assert_tracks_equal(got, rows, ref, ref_rows, "after " + id_)
