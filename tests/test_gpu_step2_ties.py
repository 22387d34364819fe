"""-m gpu: k_dbn_step2's tie redo (exact_borrows, exact_hit, the packed and the plain compare of either half of a word, the columns that
depend on a redone bin) on the tie-dense models of step2_tie_cases.py -- every output bit for bit against the oracle, no tolerance, and
every instance by the exact name ctx.last_kernel() reports.

What covers the redo is the COUNTED run of each model, 65 536 x 64, whose ties of every kind are counted first from the oracle's own
draws (test_step2_ties.py prints the table; the floors are asserted again here).  The small shapes -- block 0 with its second 0, an
interior block, a partial block, a partial last wave -- start at a wave of the counted sample that has a redo in block 0, asserted from
the small sample's own draws; so do the device call at a column offset into a wider trace and the event-list forms, one of them with a
cap that the longest list fills exactly.  The +start twins run an interleaved grid of six preset rows."""
import numpy as np
import pytest

import oracle as O
import step2_tie_cases as S
from em_model_manned_bayes_amd import native
from util import assert_uncor_parity

pytestmark = pytest.mark.gpu
SMALL_N = 64 * 5 + 37
SENTINEL_BIN, SENTINEL_VAL = 0x5A, -7.25


def _dense_parity(got, ref):
    assert np.array_equal(got["init_bin"].astype(np.int32), ref["init_bin"]) and np.array_equal(got["attempts"], ref["attempts"])
    assert np.array_equal(got["init_val"], ref["init_val"].astype(np.float32))
    assert np.array_equal(got["dyn_bin"], ref["dense_bin"]), "dense bins differ"
    assert np.array_equal(got["dyn_val"], ref["dense_val"].astype(np.float32)), "dense values differ"


def _small_sample(name, model_dir, n, T, want_events=False):
    """The oracle's sample of n trajectories from the first wave of the counted sample with a redo in block 0 -- which the small sample's
    own draws must show (a second's draws do not depend on T)."""
    nm, pp, _ = S.tie_model(name, model_dir)
    seed, first = S.MODELS[name]["seed"], S.counted_sample(name, model_dir)[2]
    ref = O.uncor_sample(O.OracleModel(pp), n, T, seed, first_index=first, want_events=want_events, per_step=S.per_step(name))
    _, tie = S.draws_by_kind(nm, pp, ref, n, T, seed, first, S.plan_of(name, model_dir), detail=True)
    assert tie[:64, 1:8].any(), "no redo in block 0 of the first wave"
    return nm, pp, seed, first, ref


@pytest.mark.parametrize("name", S.NAMES)
def test_counted_run_matches_oracle(name, gpu_ctx, model_dir):
    nm, pp, _ = S.tie_model(name, model_dir)
    ref, counts, _ = S.counted_sample(name, model_dir)
    assert not S.floors_missed(name, model_dir, counts), S.kinds_table(name, model_dir, counts)
    got = native.sample_dbn_host(gpu_ctx, nm, S.N, S.T, S.MODELS[name]["seed"], first_index=S.FIRST, want_dense=True, want_events=False,
                                 transition_mode=S.mode(name), **S.indices_of(pp))
    assert got["kernel"] == S.MODELS[name]["kernels"]["both"], got["kernel"]
    _dense_parity(got, ref)


@pytest.mark.parametrize("T", [17, 64])
@pytest.mark.parametrize("name", S.NAMES)
def test_small_shapes_match_oracle(name, T, gpu_ctx, model_dir):
    """T = 17: block 0, one interior block and a partial block (the rolled loop on full draws); T = 64: unguarded blocks only."""
    nm, pp, seed, first, ref = _small_sample(name, model_dir, SMALL_N, T)
    got = native.sample_dbn_host(gpu_ctx, nm, SMALL_N, T, seed, first_index=first, want_dense=True, want_events=False,
                                 transition_mode=S.mode(name), **S.indices_of(pp))
    assert got["kernel"] == S.MODELS[name]["kernels"]["both"], got["kernel"]
    _dense_parity(got, ref)


@pytest.mark.parametrize("name", S.NAMES)
def test_device_call_at_a_column_offset_matches_oracle(name, gpu_ctx, model_dir):
    """emgpu_sample_dbn_device at column 301 of a trace of 700 columns prefilled with sentinels: the call's columns equal the oracle,
    every other column keeps its sentinel."""
    import torch
    n, T, col, ld = 255, 17, 301, 700
    nm, pp, seed, first, ref = _small_sample(name, model_dir, n, T)
    ni, nd, G4 = nm.n_initial, nm.n_dyn, (T + 3) // 4
    dev = torch.device("cuda", 0)
    buf = {"init_bin": torch.full((ni, ld), SENTINEL_BIN, dtype=torch.uint8, device=dev),
           "init_val": torch.full((ni, ld), SENTINEL_VAL, dtype=torch.float32, device=dev),
           "attempts": torch.full((ld,), -7, dtype=torch.int32, device=dev),
           "dyn_bin": torch.full((G4, nd, ld), -0x5A5A5A5B, dtype=torch.int32, device=dev),
           "dyn_val": torch.full((G4, nd, ld, 4), SENTINEL_VAL, dtype=torch.float32, device=dev)}
    torch.cuda.synchronize()
    p, _keep = native.make_params(n, T, seed, first_index=first, transition_mode=S.mode(name), **S.indices_of(pp))
    native.sample_dbn_device(gpu_ctx, nm, p, ld=ld, col_offset=col, **{k: v.data_ptr() for k, v in buf.items()})
    gpu_ctx.sync()
    assert gpu_ctx.last_kernel() == S.MODELS[name]["kernels"]["both"], gpu_ctx.last_kernel()
    h = {k: v.cpu().numpy() for k, v in buf.items()}
    out = np.ones(ld, dtype=bool)
    out[col: col + n] = False
    assert np.all(h["init_bin"][:, out] == SENTINEL_BIN) and np.all(h["init_val"][:, out] == SENTINEL_VAL) and np.all(h["attempts"][out] == -7)
    assert np.all(h["dyn_bin"][:, :, out] == -0x5A5A5A5B) and np.all(h["dyn_val"][:, :, out] == SENTINEL_VAL)
    got = dict(init_bin=h["init_bin"][:, col: col + n].T, init_val=h["init_val"][:, col: col + n].T, attempts=h["attempts"][col: col + n],
               dyn_bin=native.unpack_dyn_bin(np.ascontiguousarray(h["dyn_bin"].view(np.uint32)[:, :, col: col + n]), T),
               dyn_val=native.unpack_dyn_val(np.ascontiguousarray(h["dyn_val"][:, :, col: col + n]), T))
    _dense_parity(got, ref)


EVENT_FORMS = [(name, form) for name in S.NAMES for form in S.MODELS[name]["kernels"] if form in ("list", "list+dense")]


@pytest.mark.parametrize("name,form", EVENT_FORMS)
def test_event_forms_match_oracle(name, form, gpu_ctx, model_dir):
    """The lists row for row (and the dense trace beside them where the form has one), first with the default room, then with a cap that
    the longest list of the sample fills exactly."""
    T = 64
    nm, pp, seed, first, ref = _small_sample(name, model_dir, SMALL_N, T, want_events=True)
    longest = max(len(e) for e in ref["events"])
    assert longest > 2 * T            # (the variable resampled at nearly every second)
    for cap in (None, longest):
        got = native.sample_dbn_host(gpu_ctx, nm, SMALL_N, T, seed, first_index=first, want_dense=form == "list+dense", want_events=True,
                                     event_cap=cap, transition_mode=S.mode(name), **S.indices_of(pp))
        assert got["kernel"] == S.MODELS[name]["kernels"][form], got["kernel"]
        assert np.array_equal(got["ev_count"], [len(e) for e in ref["events"]])
        assert_uncor_parity(got, ref, T)


def start_rows(pp, free):
    """Six preset rows (by variable id, 0 = draw): the root alone at two bins, nothing, the first two and the first three variables of the
    topological order, every bin of one trajectory of an unconstrained run."""
    order = [int(v) - 1 for v in pp["order_initial"]]
    ni = int(pp["n_initial"])
    rows = np.zeros((6, ni), dtype=np.int32)
    rows[0, order[0]] = 1
    rows[2, order[0]] = 2
    rows[3, order[:2]] = free["init_bin"][5, order[:2]]
    rows[4, order[:3]] = free["init_bin"][9, order[:3]]
    rows[5] = free["init_bin"][3]
    return rows


START_FORMS = [name for name in S.NAMES if "start" in S.MODELS[name]["kernels"]]


@pytest.mark.parametrize("name", START_FORMS)
def test_start_grid_matches_oracle(name, gpu_ctx, model_dir):
    """Trajectory i gets rows[i % 6] (every wave holds all six rows), the oracle's answer is row k's own run at i = k mod 6; the grid run's
    own draws must hold ties (the presets change the trajectories, so the counted sample says nothing about them)."""
    n, T = 64 * 40 + 37, 64
    nm, pp, _ = S.tie_model(name, model_dir)
    seed, first = S.MODELS[name]["seed"], S.counted_sample(name, model_dir)[2]
    free = O.uncor_sample(O.OracleModel(pp), 16, T, seed, first_index=first, want_events=False, want_dense=False)
    rows = start_rows(pp, free)
    per = [O.uncor_sample(O.OracleModel(pp, start=[int(v) for v in row]), n, T, seed, first_index=first, want_events=False) for row in rows]
    ref = {f: np.stack([per[i % 6][f][i] for i in range(n)]) for f in ("init_bin", "init_val", "attempts", "dense_bin", "dense_val")}
    counts = S.draws_by_kind(nm, pp, ref, n, T, seed, first, S.plan_of(name, model_dir))
    ties = sum(counts[k] for k in ("packed tie, even second", "packed tie, odd second", "plain tie, even second", "plain tie, odd second"))
    assert ties >= 10 and counts["resample tie, hit"] + counts["resample tie, no hit"] >= 3, counts
    grid = np.ascontiguousarray(rows[np.arange(n) % 6])
    got = native.sample_dbn_host(gpu_ctx, nm, n, T, seed, first_index=first, want_dense=True, want_events=False, start=grid, **S.indices_of(pp))
    assert got["kernel"] == S.MODELS[name]["kernels"]["start"], got["kernel"]
    _dense_parity(got, ref)
    for k in range(6):
        assert np.all(got["init_bin"][k::6][:, rows[k] > 0] == rows[k][rows[k] > 0])
