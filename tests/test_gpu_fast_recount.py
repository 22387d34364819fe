"""The tie redo of the fast kernel on the GPU (emgpu_kernels_fast.h): the packed exact recount of the instances that hold their
columns on chip (k_uncor_fast / k_uncor_fast_mixed of <7,2,2,2> and <7,2,4,2>) and the single tie ballot of every form, on the
tie-dense models of test_gpu_fast_ties and a <7,2,2,2> model made like them -- dense outputs bit for bit against the oracle.

A tie needs one of a handful of the 65 536 high halfwords, so a small sample holds about one.  What covers the recount are the COUNTED
runs -- 65 536 x 64 through k_uncor_fast of both on-chip shapes, and one launch of k_uncor_fast_mixed over as many columns -- whose
redos of every kind are counted first, from the oracle's draws, with the launch's own wave alignment.  The small shapes (block 0 with
its second-0 patch, interior blocks, an edge block, a partial wave) start at an index picked from the counted sample so that their
first wave has a redo in block 0, which is asserted; "ties2" has no counted sample and runs them as plumbing only."""
import os

import numpy as np
import pytest

import oracle as O
from em_model_manned_bayes_amd import em_io, native, _lib as L
from util import assert_uncor_parity, shaped_model, uncor_indices
import test_gpu_fast_ties as FT
from test_gpu_fast_ties import BIG, DENSE_N, DENSE_T, FIRST, SEED, SEC_RES, SEC_TRANS, columns_of, high_halfwords, instance_of, pk_column, tie_model

SHAPES = [(64 * 5 + 37, 17), (64 * 9 + 37, 64), (64 * 3 + 1, 8)]


def _model_222():
    """<7,2,2,2>, columns edited like test_gpu_fast_ties._tie_model: a threshold below 2^16, two sharing a high half, a padding copy,
    a variable with columns that have no real threshold; one resample rate below 2^-16."""
    p = shaped_model(np.random.RandomState(2222), 7, (2, 2, 2), rates=[0.07, 2.0 ** -16 - 2.0 ** -20, 0.3, 0, 0, 0, 0], r=[4, 3, 3, 3, 3, 2, 2])
    N0, N1, N2 = (p["N_transition"][7 + k] for k in range(3))
    for j in range(N0.shape[1]):
        if j % 3 == 0:
            N0[:, j] = [7, BIG, 0, 2 * BIG]
        elif j % 3 == 2:
            N0[:, j] = [0, BIG, 0, 3 * BIG]
    for j in range(N1.shape[1]):
        if j % 3 == 0:
            N1[:, j] = [BIG, 5, BIG]
        elif j % 3 == 1:
            N1[:, j] = [3, BIG, BIG]
    for j in range(N2.shape[1]):
        if j % 2 == 0:
            N2[:, j] = [0, 0, 1234]
    return p


_own = {}   # (the shared table of models is left as it is)


def model_of(name, model_dir):
    if name != "ties222":
        return tie_model(name, model_dir)
    if name not in _own:
        path = os.path.join(str(model_dir), "fast_recount_ties222.txt")
        em_io.em_write(_model_222(), path)
        _own[name] = (native.NativeModel.load_txt(path), O.parse_model_txt(path), path)
    return _own[name]


KERNEL = {"ties": "k_uncor_fast<7,2,4,2>", "ties2": "k_uncor_fast<7,2,4,2>", "ties222": "k_uncor_fast<7,2,2,2>"}


def test_the_222_model_runs_on_the_222_instance(model_dir):
    nm, _, _ = model_of("ties222", model_dir)
    assert instance_of(nm) == (7, 2, 2, 2) and FT.is_fast_branch(nm)


# ---- the kinds of redo in a sample, from the oracle's draws -----------------------------------------------------------------------
def redo_kinds(nm, pp, ref, n, T, seed, first, lane0=0, detail=False):
    """Counts over (wave, interior block, variable) of what the redo is asked for -- transition low halfwords only, resample only, both
    -- and over the draws: a tie in second 1 of block 0, in the low and in the high half of a packed word (even / odd second).  Waves
    are 64 consecutive lanes, the first trajectory in lane lane0 of its wave (a block of a mixed launch starts where its first column
    falls in the trace); second 0 of a trajectory is no draw and is left out.  block0: (wave, variable) pairs with a redo in block 0, whose
    second-0 patch follows the recount.  detail: also the (wave, interior block) array "some variable is redone".  ref needs init_bin only."""
    ni, shape = nm.n_initial, instance_of(nm)
    gidx = first + np.arange(n, dtype=np.uint64)
    cols = {k: [] for k in range(3)}
    for k, meff, row, cthr, nib in columns_of(nm):
        cols[k].append((meff, cthr))
    G, r = np.asarray(pp["G_transition"]), np.asarray(pp["r_transition"])
    G8 = len([g for g in range((T + 7) // 8) if 8 * g + 7 < T])      # interior blocks
    out = dict(transition_only=0, resample_only=0, both=0, second_1=0, low_half=0, high_half=0, block0=0)
    nw = (lane0 + n + 63) // 64
    wb = np.zeros((nw, G8), dtype=bool)
    for k in range(3):
        M = shape[1 + k]
        col, stride = np.zeros(n, dtype=np.int64), 1
        for u in range(ni + 3):
            if G[u, ni + k]:
                col += stride * (ref["init_bin"][:, u].astype(np.int64) - 1)
                stride *= int(r[u])
        TQ, Z = np.zeros((len(cols[k]), M), np.int64), np.zeros(len(cols[k]), bool)
        for j, (meff, cthr) in enumerate(cols[k]):
            TQ[j], Z[j] = pk_column(cthr, meff, M)
        x = high_halfwords(SEC_TRANS, ni + k, gidx, T, seed)
        s = np.zeros_like(x)
        for t in range(M):
            s += np.clip(x - TQ[col, t][:, None], 0, 2)
        tie_t = ((s & 1) != 0) | ((x == 0) & Z[col][:, None])
        R = int(L.lib().emgpu_debug_bernoulli_threshold(float(pp["resample_rates"][k])))
        tie_r = (high_halfwords(SEC_RES, k, gidx, T, seed) == (R >> 16)) if R else np.zeros_like(tie_t)
        tie_t[:, 0] = False
        tie_r[:, 0] = False
        pad = (lane0, nw * 64 - n - lane0)
        tt = np.pad(tie_t[:, : 8 * G8], (pad, (0, 0))).reshape(nw, 64, G8, 8).any(axis=(1, 3))
        tr = np.pad(tie_r[:, : 8 * G8], (pad, (0, 0))).reshape(nw, 64, G8, 8).any(axis=(1, 3))
        wb |= tt | tr
        out["transition_only"] += int((tt & ~tr).sum())
        out["resample_only"] += int((~tt & tr).sum())
        out["both"] += int((tt & tr).sum())
        if G8:
            out["block0"] += int((tt | tr)[:, 0].sum())
            out["second_1"] += int(tie_t[:, 1].sum() + tie_r[:, 1].sum())
            out["low_half"] += int(tie_t[:, 2: 8 * G8: 2].sum() + tie_r[:, 2: 8 * G8: 2].sum())
            out["high_half"] += int(tie_t[:, 1: 8 * G8: 2].sum() + tie_r[:, 1: 8 * G8: 2].sum())
    return (out, wb) if detail else out


_dense = {}


def dense_sample(name, model_dir):
    """The 65 536 x 64 oracle sample of a model and its kinds of redo, made once ("ties": the sample test_gpu_fast_ties shares)."""
    if name not in _dense:
        nm, pp, _ = model_of(name, model_dir)
        ref = FT.dense_sample(model_dir)[0] if name == "ties" else O.uncor_sample(O.OracleModel(pp), DENSE_N, DENSE_T, SEED, first_index=FIRST, want_events=False)
        kinds, wb = redo_kinds(nm, pp, ref, DENSE_N, DENSE_T, SEED, FIRST, detail=True)
        _dense[name] = (ref, kinds, FIRST + 64 * int(np.flatnonzero(wb[:, 0])[0]))
    return _dense[name][:2]


def first_with_a_redo_in_block_0(name, model_dir):
    """The index of the first wave of the counted sample that has a redo in block 0 (the draws of a second do not depend on T)."""
    dense_sample(name, model_dir)
    return _dense[name][2]


@pytest.mark.parametrize("name", ["ties", "ties222"])
def test_dense_samples_hold_every_kind_of_redo(name, model_dir):
    """A condition on the inputs of the counted GPU runs below."""
    _, kinds = dense_sample(name, model_dir)
    print(name, kinds)
    assert all(v >= 1 for v in kinds.values()), kinds


# ---- -m gpu -----------------------------------------------------------------------------------------------------------------------
def _dense_parity(got, ref):
    assert np.array_equal(got["init_bin"].astype(np.int32), ref["init_bin"]) and np.array_equal(got["attempts"], ref["attempts"])
    assert np.array_equal(got["init_val"], ref["init_val"].astype(np.float32))
    assert np.array_equal(got["dyn_bin"], ref["dense_bin"]), "dense bins differ"
    assert np.array_equal(got["dyn_val"], ref["dense_val"].astype(np.float32)), "dense values differ"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ties", "ties2", "ties222"])
@pytest.mark.parametrize("n,T", SHAPES)
def test_small_shapes_match_oracle(name, n, T, gpu_ctx, model_dir):
    """T = 17: block 0 with its second-0 patch, one interior block, one edge block; T = 64: interior blocks only; T = 8: the only block is
    block 0.  A partial last wave in each.  "ties" and "ties222" start where the counted sample has a redo in block 0, so the recount runs
    ahead of the second-0 patch (asserted from the sample's own draws); "ties2" starts at FIRST and, like test_gpu_fast_ties' small
    shapes, holds next to no redo: it checks the hot pass and the edge pass around the new control flow, not the recount."""
    nm, pp, _ = model_of(name, model_dir)
    first = FIRST if name == "ties2" else first_with_a_redo_in_block_0(name, model_dir)
    ref = O.uncor_sample(O.OracleModel(pp), n, T, SEED, first_index=first, want_events=False)
    if name != "ties2":
        kinds = redo_kinds(nm, pp, ref, n, T, SEED, first)
        assert kinds["block0"] >= 1, kinds
    got = native.sample_dbn_host(gpu_ctx, nm, n, T, SEED, first_index=first, want_dense=True, want_events=False, **uncor_indices(pp))
    assert got["kernel"] == KERNEL[name]
    _dense_parity(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ties", "ties222"])
def test_counted_run_matches_oracle(name, gpu_ctx, model_dir):
    """65 536 x 64, every block interior: redos for the transition halfwords alone, the resample halfwords alone and both, ties in second 1
    of block 0 and in either half of a packed word all occur (counted from the oracle's draws)."""
    nm, pp, _ = model_of(name, model_dir)
    ref, kinds = dense_sample(name, model_dir)
    assert all(v >= 1 for v in kinds.values()), kinds
    got = native.sample_dbn_host(gpu_ctx, nm, DENSE_N, DENSE_T, SEED, first_index=FIRST, want_dense=True, want_events=False, **uncor_indices(pp))
    assert got["kernel"] == KERNEL[name]
    _dense_parity(got, ref)


def _mixed_launch(gpu_ctx, pairs, blocks, lo, n_total, T):
    """One launch of k_uncor_fast_mixed over `blocks` = (model, first index, count); -> per block the dict _dense_parity takes."""
    import torch
    ni, nd, G4 = 7, 3, (T + 3) // 4
    ld = lo + n_total + 5
    dev = torch.device("cuda", 0)
    ib = torch.zeros((ni, ld), dtype=torch.uint8, device=dev)
    iv = torch.zeros((ni, ld), dtype=torch.float32, device=dev)
    db = torch.zeros((G4, nd, ld), dtype=torch.int32, device=dev)
    dv = torch.zeros((G4, nd, ld, 4), dtype=torch.float32, device=dev)
    at = torch.zeros((ld,), dtype=torch.int32, device=dev)
    p, _keep = native.make_params(n_total, T, SEED, first_index=FIRST + lo, **uncor_indices(pairs[0][1]))
    torch.cuda.synchronize()      # the zero fills run on torch's stream, the launch on the ctx's own non-blocking one
    native.sample_dbn_blocks_device(gpu_ctx, [pr[0] for pr in pairs], p, blocks, init_bin=ib.data_ptr(), init_val=iv.data_ptr(),
                                    dyn_bin=db.data_ptr(), dyn_val=dv.data_ptr(), attempts=at.data_ptr(), ld=ld, col_offset=lo)
    gpu_ctx.sync()
    assert gpu_ctx.last_kernel() == "k_uncor_fast_mixed<7,2,4,2>"
    gb = native.unpack_dyn_bin(db.cpu().numpy().view(np.uint32), T)
    gv = native.unpack_dyn_val(dv.cpu().numpy(), T)
    ibc, ivc, atc = ib.cpu().numpy().T, iv.cpu().numpy().T, at.cpu().numpy()
    return [dict(init_bin=ibc[f - FIRST: f - FIRST + c], init_val=ivc[f - FIRST: f - FIRST + c], attempts=atc[f - FIRST: f - FIRST + c],
                 dyn_bin=gb[f - FIRST: f - FIRST + c], dyn_val=gv[f - FIRST: f - FIRST + c]) for _, f, c in blocks]


# The counted mixed launch: "ties2" over columns 3 .. 8 231, "ties" over 8 232 .. 65 535 (rows of the shared counted sample: a column of the
# trace is the index less FIRST, so its waves are that sample's waves), "ties2" again over 219 columns: block boundaries inside a wave.
MIXED_LO = 3
MIXED_BLOCKS = [(1, FIRST + 3, 8229), (0, FIRST + 8232, DENSE_N - 8232), (1, FIRST + DENSE_N, 219)]
KEYS = ("init_bin", "init_val", "attempts", "dense_bin", "dense_val")
_mixed = {}


def mixed_sample(model_dir):
    """The oracle's samples of the three blocks and the launch's redos by kind, made once."""
    if not _mixed:
        pairs = [tie_model(m, model_dir) for m in ("ties", "ties2")]
        dense = dense_sample("ties", model_dir)[0]
        refs, total = [], {}
        for m, first, cnt in MIXED_BLOCKS:
            c = first - FIRST
            ref = {k: dense[k][c: c + cnt] for k in KEYS} if m == 0 else O.uncor_sample(O.OracleModel(pairs[m][1]), cnt, DENSE_T, SEED, first_index=first, want_events=False)
            refs.append(ref)
            for k, v in redo_kinds(pairs[m][0], pairs[m][1], ref, cnt, DENSE_T, SEED, first, lane0=c % 64).items():   # waves as the launch cuts them
                total[k] = total.get(k, 0) + v
        _mixed["refs"], _mixed["kinds"], _mixed["pairs"] = refs, total, pairs
    return _mixed["refs"], _mixed["kinds"], _mixed["pairs"]


def test_the_mixed_launch_holds_every_kind_of_redo(model_dir):
    """A condition on the inputs of the counted mixed launch below."""
    _, kinds, _ = mixed_sample(model_dir)
    print(kinds)
    assert all(v >= 1 for v in kinds.values()), kinds


@pytest.mark.gpu
def test_counted_mixed_launch_matches_oracle(gpu_ctx, model_dir):
    """Both <7,2,4,2> models in ONE launch of k_uncor_fast_mixed (its own kernel: the plan read from device memory, the resample words
    through readfirstlane) at T = 64, 65 752 columns: redos of every kind, block 0 among them, counted from the oracle's draws per block
    with the launch's wave alignment -- and every dense output of every block bit-equal."""
    refs, kinds, pairs = mixed_sample(model_dir)
    assert all(v >= 1 for v in kinds.values()), kinds
    got = _mixed_launch(gpu_ctx, pairs, MIXED_BLOCKS, MIXED_LO, DENSE_N + 219 - MIXED_LO, DENSE_T)
    for g, r in zip(got, refs):
        _dense_parity(g, r)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [17, 8])
def test_small_mixed_launch_matches_oracle(T, gpu_ctx, model_dir):
    """The same launch at 769 columns, with an edge block (T = 17) and with block 0 alone (T = 8), blocks at odd offsets.  These hold no
    redo (the counted launch above is what runs the recount): they check the edge pass and the patch of second 0 in the mixed kernel."""
    pairs = [tie_model(m, model_dir) for m in ("ties", "ties2")]
    blocks = [(0, FIRST + 3, 64 * 4 + 37), (1, FIRST + 296, 257), (0, FIRST + 553, 219)]
    got = _mixed_launch(gpu_ctx, pairs, blocks, 3, 769, T)
    for (m, first, cnt), g in zip(blocks, got):
        _dense_parity(g, O.uncor_sample(O.OracleModel(pairs[m][1]), cnt, T, SEED, first_index=first, want_events=False))


@pytest.mark.gpu
def test_index_list_run_keeps_its_redo(gpu_ctx, model_dir):
    """k_uncor_fast_idx (the reload from the table) on the counted sample, permuted: the single ballot on a form that keeps the old redo."""
    nm, pp, _ = tie_model("ties", model_dir)
    ref, kinds = dense_sample("ties", model_dir)
    assert kinds["transition_only"] and kinds["resample_only"]
    n = 16384
    perm = np.random.RandomState(11).permutation(DENSE_N)[:n]
    got = native.sample_dbn_host(gpu_ctx, nm, n, DENSE_T, SEED, want_dense=True, want_events=False, indices=(FIRST + perm).astype(np.uint64), **uncor_indices(pp))
    assert got["kernel"] == "k_uncor_fast_idx<7,2,4,2>"
    _dense_parity(got, {k: ref[k][perm] for k in ("init_bin", "init_val", "attempts", "dense_bin", "dense_val")})


@pytest.mark.gpu
def test_event_list_run_keeps_its_redo(gpu_ctx, model_dir):
    """The event-list forms (k_uncor_fast_ev with the dense trace, k_uncor_fast_evu for the list alone) on a sample with ties of both sorts."""
    nm, pp, _ = tie_model("ties", model_dir)
    n, T = 4096, 64
    ref = O.uncor_sample(O.OracleModel(pp), n, T, SEED, mode=O.RNG_PHILOX, first_index=FIRST)
    kinds = redo_kinds(nm, pp, ref, n, T, SEED, FIRST)
    print(kinds)
    assert kinds["transition_only"] + kinds["both"] >= 1 and kinds["resample_only"] + kinds["both"] >= 1, kinds
    idx = uncor_indices(pp)
    got = native.sample_dbn_host(gpu_ctx, nm, n, T, SEED, first_index=FIRST, want_dense=True, want_events=True, **idx)
    assert got["kernel"].startswith("k_uncor_fast_ev<7,2,4,2>"), got["kernel"]
    assert_uncor_parity(got, ref, T)
    alone = native.sample_dbn_host(gpu_ctx, nm, n, T, SEED, first_index=FIRST, want_dense=False, want_events=True, **idx)
    assert alone["kernel"].startswith("k_uncor_fast_evu"), alone["kernel"]
    assert np.array_equal(alone["ev_count"], np.array([len(e) for e in ref["events"]]))
    for i in range(n):
        g, r = alone["events"][i], ref["events"][i]
        assert np.array_equal(g["dt"], r[:, 0]) and np.array_equal(g["var"], r[:, 1]) and np.array_equal(g["bin"], r[:, 3]), i
        assert np.array_equal(g["value"], r[:, 2].astype(np.float32)), i
