"""-m gpu: a draw that EQUALS a threshold, in every kernel that compares one (equal_draw_cases.py): `xp >= t[k]` in draw_bin, `x < t` in
exact_borrows and the rolled loops, `< R` in exact_hit and the Bernoulli compares, the fast kernel's 32-bit recount.  Both models of a pair
-- X_t = x and X_t = x + 1, or R = x + 1 and R = x -- against the oracle bit for bit, n = 64 * 3 + 37 with the target inside the run; the
two oracle runs differ at the target (test_equal_draws.py), so a compare that is off by one fails one of the two."""
import os
import subprocess
import sys

import numpy as np
import pytest

import equal_draw_cases as E
import oracle as O
from em_model_manned_bayes_amd import native
from util import assert_uncor_parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(ctx, name, which, model_dir):
    """One model of a pair through the case's entry point against the oracle; returns the kernel name the call reported."""
    case, b = E.CASES[name], E.build(name, model_dir)
    nm, pp, _ = b[which]
    ref = E.oracle_run(name, which, model_dir)
    form = case["form"]
    if form == "bn":
        ob, ov, oa = native.sample_bn_host(ctx, nm, E.N, b["seed"], first_index=b["first"], dediscretize=True)
        kernel = ctx.last_kernel()
        assert np.array_equal(ob, ref[0]) and np.array_equal(ov, ref[1].astype(np.float32)) and np.array_equal(oa, ref[2])
        return kernel
    kw = dict(start=E.start_grid(b)) if form == "start" else {}
    got = native.sample_dbn_host(ctx, nm, E.N, b["T"], b["seed"], first_index=b["first"], want_dense=form != "list",
                                 want_events=form in ("list", "list+dense"), **kw)
    assert_uncor_parity(got, ref, b["T"])
    if "ev_count" in got:
        assert np.array_equal(got["ev_count"], [len(e) for e in ref["events"]])
    return got["kernel"]


@pytest.mark.parametrize("which", ["at", "above"])
@pytest.mark.parametrize("name", E.NAMES)
def test_both_models_of_a_pair_match_oracle(name, which, gpu_ctx, model_dir):
    assert run_case(gpu_ctx, name, which, model_dir) == E.CASES[name]["kernel"]


@pytest.mark.parametrize("order", [("at", "above"), ("above", "at")])
def test_mixed_launch_matches_oracle(order, gpu_ctx, model_dir):
    """k_uncor_fast_mixed: the pair of the <7,2,4,2> case in one launch, the target's block from the first model of `order`, a second block
    from the other one."""
    import torch
    name = "fast <7,2,4,2>: recount on chip"
    b = E.build(name, model_dir)
    T, first, seed = b["T"], b["first"], b["seed"]
    pairs = [b[w] for w in order]
    blocks = [(0, first, E.N), (1, first + E.N, 100)]
    ni, nd, G4, ld = 7, 3, (T + 3) // 4, E.N + 100 + 5
    dev = torch.device("cuda", 0)
    ib = torch.zeros((ni, ld), dtype=torch.uint8, device=dev)
    iv = torch.zeros((ni, ld), dtype=torch.float32, device=dev)
    db = torch.zeros((G4, nd, ld), dtype=torch.int32, device=dev)
    dv = torch.zeros((G4, nd, ld, 4), dtype=torch.float32, device=dev)
    at = torch.zeros((ld,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    p, _keep = native.make_params(E.N + 100, T, seed, first_index=first)
    native.sample_dbn_blocks_device(gpu_ctx, [pr[0] for pr in pairs], p, blocks, init_bin=ib.data_ptr(), init_val=iv.data_ptr(),
                                    dyn_bin=db.data_ptr(), dyn_val=dv.data_ptr(), attempts=at.data_ptr(), ld=ld, col_offset=0)
    gpu_ctx.sync()
    assert gpu_ctx.last_kernel() == "k_uncor_fast_mixed<7,2,4,2>"
    gb = native.unpack_dyn_bin(db.cpu().numpy().view(np.uint32), T)
    gv = native.unpack_dyn_val(dv.cpu().numpy(), T)
    for (m, f, cnt), w in zip(blocks, order):
        c = f - first
        ref = E.oracle_run(name, w, model_dir) if m == 0 else O.uncor_sample(O.OracleModel(pairs[m][1]), cnt, T, seed, first_index=f, want_events=False)
        assert np.array_equal(gb[c: c + cnt], ref["dense_bin"]) and np.array_equal(gv[c: c + cnt], ref["dense_val"].astype(np.float32)), w
        assert np.array_equal(ib.cpu().numpy().T[c: c + cnt], ref["init_bin"]) and np.array_equal(at.cpu().numpy()[c: c + cnt], ref["attempts"]), w


_CHILD = r"""
import sys
sys.path[:0] = [%r, %r, %r]
from em_model_manned_bayes_amd import native
from test_gpu_equal_draws import run_case
ctx = native.Context(0)
for which in ("at", "above"):
    k = run_case(ctx, sys.argv[1], which, sys.argv[3])
    assert k == sys.argv[2], k
    print("pair ok", which, k)
"""


def test_the_step_kernel_without_lds_in_a_child_process(model_dir):
    """k_dbn_step<7,3,8>: EMGPU_DEBUG_STEP_NO_LDS is read once per process, so the pair runs in a fresh child (as test_gpu_instances.py runs
    its env rows)."""
    name, kernel, env = E.STEP_NO_LDS
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    own = os.path.join(str(model_dir), "equal_no_lds")      # (the child writes its pair's files itself)
    os.makedirs(own, exist_ok=True)
    r = subprocess.run([sys.executable, "-c", code, name, kernel, own], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("pair ok") == 2, r.stdout[-2000:] + r.stderr[-4000:]
