"""The paths of the trimmed cooperative dediscretize (emgpu_coop.h: CoopTrim -- one owner-row address and the scaled boundary table in
the worker pass, the request queue written without loop-carried copies, the bins published by two-word stores) on the GPU, dense outputs
bit for bit against the oracle: a partial wave, an edge block, lanes outside the run serving as workers, a wave-block with more requests
than one round of the queue holds (the multi-round path) and one with none (the early return), and every form of the fast kernel that
shares the pass or sits beside it: k_uncor_fast, _mixed, _idx (trimmed) and the event-list form (which keeps the pass as it was).
k_dbn_step2 and k_dbn_step keep the pass as it was too, so they have no case here."""
import os

import numpy as np
import pytest

import oracle as O
from em_model_manned_bayes_amd import em_io, native
from util import assert_uncor_parity, load_pair, shaped_model, uncor_indices
from test_gpu_fast_ties import FIRST, SEED, instance_of, is_fast_branch
from test_gpu_fast_recount import _dense_parity, _mixed_launch

MODEL = "uncor_1200code_v2p1"
SHAPES = [(209, 17), (64, 8), (17, 240)]   # a partial wave and an edge block; one full wave, block 0 alone; 47 idle lanes serving as workers, 30 blocks
KEYS = ("init_bin", "init_val", "attempts", "dense_bin", "dense_val")

_refs = {}


def reference(pp, n, T, first, events=False, seed=SEED):
    """The oracle's sample, made once per shape and shared."""
    key = (id(pp), n, T, first, events, seed)
    if key not in _refs:
        _refs[key] = O.uncor_sample(O.OracleModel(pp), n, T, seed, first_index=first, want_events=events)
    return _refs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("n,T", SHAPES)
def test_dense_kernel_matches_oracle(n, T, gpu_ctx, model_dir):
    nm, pp, _ = load_pair(MODEL, model_dir)
    got = native.sample_dbn_host(gpu_ctx, nm, n, T, SEED, first_index=FIRST, want_dense=True, want_events=False, **uncor_indices(pp))
    assert got["kernel"] == "k_uncor_fast<7,2,4,2>"
    _dense_parity(got, reference(pp, n, T, FIRST))


# ---- a high-rate model: more than one round of the queue in a wave-block, and a wave-block without a request -------------------------
HIGH_N, HIGH_T, HIGH_FIRST, HIGH_SEED = 129, 9, 10, 0x26C0FFEE   # two full waves and a wave of one lane; block 1 is second 8 alone
_high = {}


def high_rate_model(model_dir):
    if not _high:
        p = shaped_model(np.random.RandomState(2626), 7, (2, 4, 2), rates=[0.97, 0.5, 0.0, 0, 0, 0, 0])
        path = os.path.join(str(model_dir), "coop_paths_high_rate.txt")
        em_io.em_write(p, path)
        _high["m"] = (native.NativeModel.load_txt(path), O.parse_model_txt(path))
    return _high["m"]


def requests_per_wave_block(ref, n, T, pp):
    """Dediscretize draws due per (wave, 8-second block), from the oracle's event list: a (trajectory, variable, second) with a row whose
    bin is not the variable's zero bin (dediscretize.m:24-39; a transition row and a resample row of one second are one draw)."""
    zero = np.asarray(pp["zero_bins"])
    cnt = np.zeros(((n + 63) // 64, (T + 7) // 8), dtype=np.int64)
    for i, e in enumerate(ref["events"]):
        t = np.cumsum(e[:, 0]).astype(np.int64)
        seen = set()
        for tt, v, b in zip(t, e[:, 1].astype(np.int64), e[:, 3].astype(np.int64)):
            if v > 0 and tt < T and b != zero[v - 1] and (v, tt) not in seen:
                seen.add((v, tt))
                cnt[i // 64, tt // 8] += 1
    return cnt


def test_the_high_rate_sample_holds_both_wave_blocks(model_dir):
    """A condition on the input of the GPU run below: the instance, and the oracle's own request counts."""
    nm, pp = high_rate_model(model_dir)
    assert instance_of(nm) == (7, 2, 4, 2) and is_fast_branch(nm)
    cnt = requests_per_wave_block(reference(pp, HIGH_N, HIGH_T, HIGH_FIRST, events=True, seed=HIGH_SEED), HIGH_N, HIGH_T, pp)
    print(cnt)
    assert cnt.max() > 256 and cnt.min() == 0, cnt
    assert (cnt[:2, 0] > 512).all(), cnt      # three rounds and more in the full waves


@pytest.mark.gpu
def test_multi_round_queue_and_early_return_match_oracle(gpu_ctx, model_dir):
    nm, pp = high_rate_model(model_dir)
    ref = reference(pp, HIGH_N, HIGH_T, HIGH_FIRST, events=True, seed=HIGH_SEED)
    cnt = requests_per_wave_block(ref, HIGH_N, HIGH_T, pp)
    assert cnt.max() > 256 and cnt.min() == 0, cnt
    got = native.sample_dbn_host(gpu_ctx, nm, HIGH_N, HIGH_T, HIGH_SEED, first_index=HIGH_FIRST, want_dense=True, want_events=False, **uncor_indices(pp))
    assert got["kernel"] == "k_uncor_fast<7,2,4,2>"
    _dense_parity(got, ref)


# ---- the other forms at (209, 17) ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_launch_matches_oracle(gpu_ctx, model_dir):
    """One launch of k_uncor_fast_mixed: two blocks of the model that begin inside a wave (columns 3 .. 102 and 103 .. 211)."""
    pair = load_pair(MODEL, model_dir)
    n, T = SHAPES[0]
    blocks = [(0, FIRST + 3, 100), (0, FIRST + 103, n - 100)]
    got = _mixed_launch(gpu_ctx, [pair], blocks, 3, n, T)
    ref = reference(pair[1], n + 3, T, FIRST)
    for (_, first, cnt), g in zip(blocks, got):
        c = first - FIRST
        _dense_parity(g, {k: ref[k][c: c + cnt] for k in KEYS})


@pytest.mark.gpu
def test_index_list_launch_matches_oracle(gpu_ctx, model_dir):
    nm, pp, _ = load_pair(MODEL, model_dir)
    n, T = SHAPES[0]
    ref = reference(pp, 4 * n, T, FIRST)
    perm = np.random.RandomState(26).permutation(4 * n)[:n]
    got = native.sample_dbn_host(gpu_ctx, nm, n, T, SEED, want_dense=True, want_events=False, indices=(FIRST + perm).astype(np.uint64), **uncor_indices(pp))
    assert got["kernel"] == "k_uncor_fast_idx<7,2,4,2>"
    _dense_parity(got, {k: ref[k][perm] for k in KEYS})


@pytest.mark.gpu
def test_event_list_launch_matches_oracle(gpu_ctx, model_dir):
    nm, pp, _ = load_pair(MODEL, model_dir)
    n, T = SHAPES[0]
    ref = reference(pp, n, T, FIRST, events=True)
    got = native.sample_dbn_host(gpu_ctx, nm, n, T, SEED, first_index=FIRST, want_dense=True, want_events=True, **uncor_indices(pp))
    assert got["kernel"].startswith("k_uncor_fast_ev<7,2,4,2>"), got["kernel"]
    assert_uncor_parity(got, ref, T)
