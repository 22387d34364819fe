"""-m gpu: every sampler kernel instance of tests/instances.py, reached through the entry point and output form its row names, asserted by
its exact kernel name and compared bit for bit with the CPU oracle -- at a batch that is not a multiple of the workgroup, a length that
is not a multiple of the 8-second block, a first index above 2^32, and (device entry points) a column offset into a larger trace.
The eligibility edges of the dispatcher: a model on each side, each against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import instances as I
import oracle as O
from em_model_manned_bayes_amd import native, _lib as L
from util import assert_uncor_parity, load_row_model, uncor_indices

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST = 2**35 + 7
SEED = 0x1A57A
SENTINEL_BIN, SENTINEL_VAL = 0x5A, -7.25


def _row_id(r):
    m = r["model"] if isinstance(r["model"], str) else "s%d" % r["model"]["seed"]
    return "%s-%s-%s%s" % (r["kernel"], m, r["form"], "-perstep" if r.get("per_step") else "")


def _mode(row):
    return L.TRANSITION_PER_STEP if row.get("per_step") else L.TRANSITION_REFERENCE_AUTO


def _check_events(got_events, ref_events, what):
    assert len(got_events) == len(ref_events), what
    for i, (g, r) in enumerate(zip(got_events, ref_events)):
        assert len(g) == r.shape[0], (what, i, len(g), r.shape[0])
        assert np.array_equal(g["dt"], r[:, 0]) and np.array_equal(g["var"], r[:, 1]) and np.array_equal(g["bin"], r[:, 3]), (what, i)
        assert np.array_equal(g["value"], r[:, 2].astype(np.float32)), (what, i)


def _host(ctx, row, nm, pp, n, T):
    """The host entry point in the row's form against the oracle; returns the kernel name it reported."""
    idx = uncor_indices(pp)
    om = O.OracleModel(pp)
    form, mode, per_step = row["form"], _mode(row), bool(row.get("per_step"))
    if form == "plain":
        flags = L.FLAG_NO_RESAMPLE | L.FLAG_NO_DEDISC | L.FLAG_NO_TERMINATOR
        got = native.sample_dbn_host(ctx, nm, n, T, SEED, first_index=FIRST, want_dense=False, want_events=True, flags=flags,
                                     transition_mode=mode, event_cap=nm.n_initial * T + 1, max_attempts=1)
        rb, rev = O.dbn_sample(om, n, T, SEED, first_index=FIRST, per_step=per_step)
        assert np.array_equal(got["init_bin"], rb)
        for i, (g, r) in enumerate(zip(got["events"], rev)):
            assert len(g) == r.shape[0], i
            assert np.array_equal(g["dt"], r[:, 0]) and np.array_equal(g["var"], r[:, 1]) and np.array_equal(g["bin"], r[:, 2]), i
        return got["kernel"]
    ref = O.uncor_sample(om, n, T, SEED, first_index=FIRST, per_step=per_step)
    if form == "idx":   # an index list: a permutation of the oracle's range, every row checked at its own global index
        perm = np.random.RandomState(n).permutation(n)
        got = native.sample_dbn_host(ctx, nm, n, T, SEED, want_dense=True, want_events=False, transition_mode=mode,
                                     indices=(FIRST + perm).astype(np.uint64), **idx)
        sub = {k: ref[k][perm] for k in ("init_bin", "init_val", "attempts", "dense_bin", "dense_val")}
        assert_uncor_parity(got, sub, T, check_events=False)
        return got["kernel"]
    want_dense = form in ("both", "list+dense")
    want_events = form in ("list", "list+dense")
    got = native.sample_dbn_host(ctx, nm, n, T, SEED, first_index=FIRST, want_dense=want_dense, want_events=want_events,
                                 transition_mode=mode, **idx)
    assert_uncor_parity(got, ref, T, check_events=False)
    if want_events:
        assert np.array_equal(got["ev_count"], [len(e) for e in ref["events"]])
        _check_events(got["events"], ref["events"], row["kernel"])
    return got["kernel"]


def _device(ctx, row, nm, pp, n, T, col, ld):
    """The device entry point in the row's form, written at column `col` of a trace of `ld` columns prefilled with sentinels: the
    columns of the call equal the oracle, every other column keeps its sentinel."""
    import torch
    idx = uncor_indices(pp)
    form, mode = row["form"], _mode(row)
    ni, nd, G4 = nm.n_initial, nm.n_dyn, (T + 3) // 4
    cap = min((ni + nd + 1) * T + 2, 4096)
    dev = torch.device("cuda", 0)
    dense = form in ("both", "list+dense", "one")
    events = form in ("list", "list+dense")
    buf = {}
    if form != "one":
        buf["init_bin"] = torch.full((ni, ld), SENTINEL_BIN, dtype=torch.uint8, device=dev)
        buf["init_val"] = torch.full((ni, ld), SENTINEL_VAL, dtype=torch.float32, device=dev)
        buf["attempts"] = torch.full((ld,), -7, dtype=torch.int32, device=dev)
    if dense:
        buf["dyn_bin"] = torch.full((G4, nd, ld), -0x5A5A5A5B, dtype=torch.int32, device=dev)
        if form != "one":
            buf["dyn_val"] = torch.full((G4, nd, ld, 4), SENTINEL_VAL, dtype=torch.float32, device=dev)
    if events:
        buf["ev_count"] = torch.full((ld,), -7, dtype=torch.int32, device=dev)
        buf["events"] = torch.full((ld, cap, 2), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    p, _keep = native.make_params(n, T, SEED, first_index=FIRST, transition_mode=mode, event_cap=cap if events else 0, **idx)
    native.sample_dbn_device(ctx, nm, p, ld=ld, col_offset=col, **{k: v.data_ptr() for k, v in buf.items()})
    ctx.sync()
    kernel = ctx.last_kernel()
    h = {k: v.cpu().numpy() for k, v in buf.items()}
    ref = O.uncor_sample(O.OracleModel(pp), n, T, SEED, first_index=FIRST, per_step=bool(row.get("per_step")))
    out = np.ones(ld, dtype=bool)
    out[col: col + n] = False
    got = {}
    if "init_bin" in h:
        got["init_bin"], got["init_val"], got["attempts"] = h["init_bin"][:, col: col + n].T, h["init_val"][:, col: col + n].T, h["attempts"][col: col + n]
        assert np.all(h["init_bin"][:, out] == SENTINEL_BIN) and np.all(h["init_val"][:, out] == SENTINEL_VAL) and np.all(h["attempts"][out] == -7)
    if "dyn_bin" in h:
        db = h["dyn_bin"].view(np.uint32)
        assert np.all(h["dyn_bin"][:, :, out] == -0x5A5A5A5B)
        got_bin = native.unpack_dyn_bin(np.ascontiguousarray(db[:, :, col: col + n]), T)
        assert np.array_equal(got_bin, ref["dense_bin"]), "dense bins differ"
        if "dyn_val" in h:
            assert np.all(h["dyn_val"][:, :, out] == SENTINEL_VAL)
            got_val = native.unpack_dyn_val(np.ascontiguousarray(h["dyn_val"][:, :, col: col + n]), T)
            assert np.array_equal(got_val, ref["dense_val"].astype(np.float32)), "dense values differ"
    if got:
        assert np.array_equal(got["init_bin"].astype(np.int32), ref["init_bin"]) and np.array_equal(got["attempts"], ref["attempts"])
        assert np.array_equal(got["init_val"], ref["init_val"].astype(np.float32))
    if events:
        cnt = h["ev_count"]
        assert np.all(cnt[out] == -7)
        assert np.array_equal(cnt[col: col + n], [len(e) for e in ref["events"]])
        evh = h["events"].reshape(ld, cap * 2).view(native.EVENT_DTYPE)
        _check_events([evh[col + i, : cnt[col + i]] for i in range(n)], ref["events"], row["kernel"])
        assert np.all(h["events"][out] == -7)
    return kernel


def _mixed(ctx, row, model_dir, T):
    """emgpu_sample_dbn_blocks_device: blocks of the row's models at odd offsets of one trace (one launch: the models share the
    instance), each block's columns against the oracle at its own global indices, the columns no block covers untouched."""
    import torch
    pairs = [load_row_model(m, model_dir) for m in [row["model"]] + list(row["with_"])]
    ni, nd, G4 = pairs[0][0].n_initial, pairs[0][0].n_dyn, (T + 3) // 4
    blocks = [(0, FIRST + 3, 301), (1, FIRST + 304, 257), (0, FIRST + 561, 219), (1, FIRST + 780, 77)]   # (model, first index, n)
    lo, n_total = 3, 857                                                 # the trace covers global indices FIRST + [0, 860); col = index - FIRST
    dev = torch.device("cuda", 0)
    ld = lo + n_total + 5
    ib = torch.full((ni, ld), SENTINEL_BIN, dtype=torch.uint8, device=dev)
    iv = torch.full((ni, ld), SENTINEL_VAL, dtype=torch.float32, device=dev)
    db = torch.full((G4, nd, ld), -0x5A5A5A5B, dtype=torch.int32, device=dev)
    dv = torch.full((G4, nd, ld, 4), SENTINEL_VAL, dtype=torch.float32, device=dev)
    at = torch.full((ld,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    p, _keep = native.make_params(n_total, T, SEED, first_index=FIRST + lo, **uncor_indices(pairs[0][1]))
    native.sample_dbn_blocks_device(ctx, [pr[0] for pr in pairs], p, blocks, init_bin=ib.data_ptr(), init_val=iv.data_ptr(),
                                    dyn_bin=db.data_ptr(), dyn_val=dv.data_ptr(), attempts=at.data_ptr(), ld=ld, col_offset=lo)
    ctx.sync()
    kernel = ctx.last_kernel()
    gb = native.unpack_dyn_bin(db.cpu().numpy().view(np.uint32), T)
    gv = native.unpack_dyn_val(dv.cpu().numpy(), T)
    gib, giv, gat = ib.cpu().numpy().T, iv.cpu().numpy().T, at.cpu().numpy()
    covered = np.zeros(ld, dtype=bool)
    for m, first, cnt in blocks:
        c = first - FIRST
        covered[c: c + cnt] = True
        ref = O.uncor_sample(O.OracleModel(pairs[m][1]), cnt, T, SEED, first_index=first, want_events=False)
        assert np.array_equal(gb[c: c + cnt], ref["dense_bin"]), (m, first)
        assert np.array_equal(gv[c: c + cnt], ref["dense_val"].astype(np.float32)), (m, first)
        assert np.array_equal(gib[c: c + cnt], ref["init_bin"]) and np.array_equal(giv[c: c + cnt], ref["init_val"].astype(np.float32)), (m, first)
        assert np.array_equal(gat[c: c + cnt], ref["attempts"]), (m, first)
    assert np.all(gib[~covered] == SENTINEL_BIN) and np.all(giv[~covered] == SENTINEL_VAL) and np.all(gat[~covered] == -7)
    assert np.all(gb[~covered] == 0xA5) and np.all(gv[~covered] == SENTINEL_VAL)
    return kernel


def _bn(ctx, row, nm, pp, n):
    """bn_sample.m with dediscretized values: bins, values and attempts against the oracle's geometry draw.  "bn+start": a start grid
    whose rows preset variable 1 (a root of the initial network) to bin 1 or 2 or leave it unset, each row against the oracle run
    with that preset as the model's own start."""
    preset = np.arange(n) % 3                         # 0 = unset, else the preset bin
    start = None
    if row["form"] == "bn+start":
        start = np.zeros((n, nm.n_initial), dtype=np.int32)
        start[:, 0] = preset
    ob, ov, oa = native.sample_bn_host(ctx, nm, n, SEED, first_index=FIRST, dediscretize=True, start=start)
    kernel = ctx.last_kernel()
    for b in ((0, 1, 2) if start is not None else (0,)):
        rows = preset == b if start is not None else np.ones(n, dtype=bool)
        rb, rv, ra = O.geom_sample(O.OracleModel(pp, start=[b] + [0] * (nm.n_initial - 1)), n, SEED, first_index=FIRST)
        assert np.array_equal(ob[rows], rb[rows]), b
        assert np.array_equal(ov[rows], rv[rows].astype(np.float32)), b
        assert np.array_equal(oa[rows], ra[rows]), b
        if b:
            assert np.all(ob[rows, 0] == b)
    return kernel


def run_row(ctx, row, model_dir):
    """Every run of one row; returns the kernel names the runs reported."""
    nm, pp, _ = load_row_model(row["model"], model_dir)
    form = row["form"]
    if form == "mixed":
        return [_mixed(ctx, row, model_dir, 61)]
    if form.startswith("bn"):
        return [_bn(ctx, row, nm, pp, 777), _bn(ctx, row, nm, pp, 255)]
    kernels = []
    if form != "one":
        kernels += [_host(ctx, row, nm, pp, 777, 61), _host(ctx, row, nm, pp, 257, 9)]
    if form not in ("idx", "plain"):
        kernels += [_device(ctx, row, nm, pp, 255, 61, 301, 700), _device(ctx, row, nm, pp, 1, 7, 513, 520)]
    return kernels


_CHILD = r"""
import json, sys
sys.path[:0] = [%r, %r, %r]
from em_model_manned_bayes_amd import native
from test_gpu_instances import run_row
rows = json.loads(sys.argv[1])
ctx = native.Context(0)
for row in rows:
    ks = run_row(ctx, row, sys.argv[2])
    assert all(k == row["kernel"] for k in ks), (row["kernel"], ks)
    print("row ok", row["kernel"])
"""


def _run_in_child(rows, env, model_dir):
    """Rows whose instance a debug variable selects (read once per process): one child process per variable setting."""
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    r = subprocess.run([sys.executable, "-c", code, json.dumps(rows), str(model_dir)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.count("row ok") == len(rows), r.stdout[-2000:] + r.stderr[-4000:]


IN_PROCESS = [r for r in I.ROWS if not r.get("env")]
ENVS = sorted({json.dumps(r["env"], sort_keys=True) for r in I.ROWS if r.get("env")})


@pytest.mark.parametrize("row", IN_PROCESS, ids=_row_id)
def test_instance_matches_oracle(row, gpu_ctx, model_dir):
    kernels = run_row(gpu_ctx, row, model_dir)
    assert kernels and all(k == row["kernel"] for k in kernels), (row["kernel"], kernels)


@pytest.mark.parametrize("env", ENVS)
def test_instances_selected_by_a_debug_variable_match_oracle(env, model_dir):
    rows = [r for r in I.ROWS if r.get("env") and json.dumps(r["env"], sort_keys=True) == env]
    _run_in_child(rows, json.loads(env), model_dir)


@pytest.mark.parametrize("edge", I.EDGES, ids=lambda e: e[0])
def test_both_sides_of_an_eligibility_edge(edge, gpu_ctx, model_dir):
    """The dispatcher changes family at the edge: each side lands where the table says and matches the oracle."""
    _, lo, hi, _ = edge
    for row in (lo, hi):
        kernels = run_row(gpu_ctx, row, model_dir)
        assert all(k == row["kernel"] for k in kernels), (row["kernel"], kernels)
