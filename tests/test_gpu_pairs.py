"""-m gpu: the three Python functions on paired tracks -- native.miss_distance, encounter_pose, encounter_miss -- read their arguments
alike.  test_gpu_miss.py and test_gpu_encounter.py test the kernels, and each tests a part of the argument forms; here every form of the
tracks (numpy rows, numpy planar, a torch CPU tensor, a torch device tensor) meets every form of the stream (none, the HIP default stream,
a Context that was given a stream, a Context on a stream of its own), on the two pairings the layer is used with.  65 pairs: a wave and one
pair.  The comparison is pair_cases.same: bit for bit against the numpy restatements."""
import numpy as np
import pytest

import encounter_ref
import miss_ref
import pair_cases as PC
from em_model_manned_bayes_amd import native

pytestmark = pytest.mark.gpu

N, P = 65, 3
RADIUS, HALF_HEIGHT, SCALE, SEED = 6000.0, 800.0, 1.0e9, 11
MISS = {"hmd_ft": "hmd", "vmd_ft": "vmd", "t_cpa": "t_cpa", "flags": "flags", "totals": "totals"}
ENC = ("pose", "rate", "flags", "weights")


def test_the_three_functions_read_their_arguments_alike(gpu_ctx):
    import torch
    side = torch.cuda.Stream()
    given = native.Context(0, stream=side.cuda_stream)
    assert gpu_ctx.stream is None and given.stream == side.cuda_stream
    streams = ({}, {"stream": 0}, {"ctx": given}, {"ctx": gpu_ctx})
    forms = (("rows", lambda r: r), ("planar", lambda r: PC.planar(r)), ("rows", lambda r: torch.from_numpy(r.copy())),
             ("planar", lambda r: torch.from_numpy(PC.planar(r)).cuda()))
    rows_b = PC.tracks(N, P, 2)
    w = np.random.RandomState(3).randint(0, 2**16, N)
    pose = native.make_pose(*(np.random.RandomState(4).uniform(-lim, lim, N) for lim in (180.0, 2000.0, 2000.0, 300.0)))
    perm = np.random.RandomState(5).permutation(N).astype(np.int64)
    # one ownship against 65 intruders; 65 against 65 through a permutation
    for rows_a, idx in ((PC.tracks(1, P, 1), {}), (PC.tracks(N, P, 1), {"idx_b": perm})):
        a, b, n_a = PC.planar(rows_a), PC.planar(rows_b), rows_a.shape[0]
        want_miss = miss_ref.miss(a, b, n_a, N, N, pose_b=pose, weights=w, **idx)
        want_enc = encounter_ref.encounter(a, b, n_a, N, N, RADIUS, HALF_HEIGHT, SEED, weights_in=w, rate_scale=SCALE, **idx)
        want_both = miss_ref.miss(a, b, n_a, N, N, pose_b=want_enc["pose"], weights=want_enc["weights"], **idx)
        assert want_miss["totals"][0] == N and (want_enc["rate"] > 0.0).all()
        for layout, form in forms:
            xa, xb = form(rows_a), form(rows_b)
            for kw in streams:
                kw = dict(kw, layout=layout, **idx)
                res = native.miss_distance(xa, xb, pose_b=pose, weights=w, **kw)
                PC.same({MISS[k]: v for k, v in res.items() if k in MISS}, want_miss, MISS.values())
                assert np.array_equal(res["nmac"], (want_miss["flags"] & 1) != 0)
                enc = native.encounter_pose(xa, xb, RADIUS, HALF_HEIGHT, SEED, weights=w, rate_scale=SCALE, **kw)
                PC.same(enc, want_enc, ENC)
                # encounter_miss is encounter_pose, then miss_distance with its pose and its weights
                step = native.miss_distance(xa, xb, pose_b=enc["pose"], weights=enc["weights"], **kw)
                both = native.encounter_miss(xa, xb, RADIUS, HALF_HEIGHT, SEED, weights=w, rate_scale=SCALE, **kw)
                PC.same(both, step, MISS)
                assert np.array_equal(both["nmac"], step["nmac"])
                PC.same({"pose": enc["pose"], "rate": both["rate"], "flags": both["encounter_flags"], "weights": both["weights"]}, enc, ENC[1:])
                PC.same({MISS[k]: both[k] for k in MISS}, want_both, MISS.values())
