"""The dense forms of the fast kernel with ONE tie word in the high-halfword pass (HISTORY.md section 31; its numpy mirror is
tests/test_fast_tie_word.py): bit for bit with the oracle where the word decides something -- whether a block is redone, and which of the
two low-halfword blocks the redo draws -- and in the resample hits, which now leave the word by one bit select.  The models, the counted
samples and their kinds of redo are those of tests/test_gpu_fast_recount.py (made once per session and shared with it); the redos are
counted from the oracle's draws before every launch."""
import numpy as np
import pytest

import oracle as O
from em_model_manned_bayes_amd import native
from util import assert_uncor_parity, uncor_indices
from test_gpu_fast_ties import DENSE_N, DENSE_T, FIRST, SEED, tie_model
from test_gpu_fast_recount import (KERNEL, KEYS, MIXED_BLOCKS, MIXED_LO, SHAPES, _dense_parity, _mixed_launch, dense_sample,
                                   first_with_a_redo_in_block_0, mixed_sample, model_of, redo_kinds)

KINDS = ("transition_only", "resample_only", "both", "block0", "second_1")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ties", "ties222"])
@pytest.mark.parametrize("n,T", SHAPES)
def test_small_shapes_start_at_a_redo_in_block_0(name, n, T, gpu_ctx, model_dir):
    """k_uncor_fast of both on-chip shapes at (357, 17), (613, 64) and (193, 8), from the first wave of the counted sample whose block 0
    is redone: the word is split in the cold block ahead of the second-0 patch, beside an edge block and in a partial wave."""
    nm, pp, _ = model_of(name, model_dir)
    first = first_with_a_redo_in_block_0(name, model_dir)
    ref = O.uncor_sample(O.OracleModel(pp), n, T, SEED, first_index=first, want_events=False)
    kinds = redo_kinds(nm, pp, ref, n, T, SEED, first)
    assert kinds["block0"] >= 1, kinds
    got = native.sample_dbn_host(gpu_ctx, nm, n, T, SEED, first_index=first, want_dense=True, want_events=False, **uncor_indices(pp))
    assert got["kernel"] == KERNEL[name]
    _dense_parity(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ties", "ties222"])
def test_counted_run_splits_the_word_every_way(name, gpu_ctx, model_dir):
    """65 536 x 64: waves whose word holds a transition tie alone (the redo keeps the pass's hit8, taken from the word by the bit select),
    a resample tie alone (it keeps the pass's bins), both, a tie in block 0 and one in second 1 -- counted first."""
    nm, pp, _ = model_of(name, model_dir)
    ref, kinds = dense_sample(name, model_dir)
    print(name, kinds)
    assert all(kinds[k] >= 1 for k in KINDS), kinds
    got = native.sample_dbn_host(gpu_ctx, nm, DENSE_N, DENSE_T, SEED, first_index=FIRST, want_dense=True, want_events=False, **uncor_indices(pp))
    assert got["kernel"] == KERNEL[name]
    _dense_parity(got, ref)


@pytest.mark.gpu
def test_mixed_launch_whose_blocks_begin_inside_a_wave(gpu_ctx, model_dir):
    """One launch of k_uncor_fast_mixed<7,2,4,2> (asserted in _mixed_launch) over three blocks that begin inside a wave, every kind of
    redo counted with the launch's own wave alignment."""
    refs, kinds, pairs = mixed_sample(model_dir)
    assert all(kinds[k] >= 1 for k in KINDS), kinds
    for g, r in zip(_mixed_launch(gpu_ctx, pairs, MIXED_BLOCKS, MIXED_LO, DENSE_N + 219 - MIXED_LO, DENSE_T), refs):
        _dense_parity(g, r)


@pytest.mark.gpu
def test_index_list_run_is_untouched(gpu_ctx, model_dir):
    """k_uncor_fast_idx takes the one word too, and keeps the old redo (the reload from the table) behind it."""
    nm, pp, _ = tie_model("ties", model_dir)
    ref, kinds = dense_sample("ties", model_dir)
    assert kinds["transition_only"] and kinds["resample_only"]
    n = 8192
    perm = np.random.RandomState(31).permutation(DENSE_N)[:n]
    got = native.sample_dbn_host(gpu_ctx, nm, n, DENSE_T, SEED, want_dense=True, want_events=False, indices=(FIRST + perm).astype(np.uint64), **uncor_indices(pp))
    assert got["kernel"] == "k_uncor_fast_idx<7,2,4,2>"
    _dense_parity(got, {k: ref[k][perm] for k in KEYS})


@pytest.mark.gpu
def test_event_list_run_is_untouched(gpu_ctx, model_dir):
    """k_uncor_fast_ev keeps the pass's two tie words and the old redo: a sample with redos of both sorts, dense trace and list."""
    nm, pp, _ = tie_model("ties", model_dir)
    n, T = 2048, 64
    ref = O.uncor_sample(O.OracleModel(pp), n, T, SEED, mode=O.RNG_PHILOX, first_index=FIRST)
    kinds = redo_kinds(nm, pp, ref, n, T, SEED, FIRST)
    assert kinds["transition_only"] + kinds["both"] >= 1 and kinds["resample_only"] + kinds["both"] >= 1, kinds
    got = native.sample_dbn_host(gpu_ctx, nm, n, T, SEED, first_index=FIRST, want_dense=True, want_events=True, **uncor_indices(pp))
    assert got["kernel"].startswith("k_uncor_fast_ev<7,2,4,2>"), got["kernel"]
    assert_uncor_parity(got, ref, T)
