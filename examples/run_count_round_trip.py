#!/usr/bin/env python3
"""examples/run_count_round_trip.py -- sample -> count -> normalise gives back the model: draw 1 M trajectories of 60 s under
uncor_1200code_v2p1 on the GPU, count the trace where it lies (native.sample_count_host: only the tables come back), build a model from the
counts (NativeModel.from_arrays) and print the largest absolute difference between its log P tables and the source model's, over the cells
whose column was visited at least 1000 times.

    python examples/run_count_round_trip.py [n] [sample_time]
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from em_model_manned_bayes_amd import _lib as L  # noqa: E402
from em_model_manned_bayes_amd import em_io, native  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
T = int(sys.argv[2]) if len(sys.argv) > 2 else 60
parms = em_io.em_read(em_io.materialize_model("uncor_1200code_v2p1", tempfile.mkdtemp()))
src = parms["native"]
ctx = native.Context(0)

got = native.sample_count_host(ctx, src, n, T, seed=1)
print("sampled by %s, counted by %s: %d initial and %d transition observations" %
      (got["kernel"], got["count_kernel"], int(got["raw"][0].sum()), int(got["raw"][1].sum())))

fit = native.NativeModel.from_arrays(
    parms["G_initial"], parms["r_initial"], got["N_initial"], parms["G_transition"], src.get_i32(L.F_R_TRANSITION), got["N_transition"],
    temporal_map=parms["temporal_map"], boundaries=parms["boundaries"], resample_rates=parms["resample_rates"])

for network, counts in ((0, got["N_initial"]), (1, got["N_transition"])):
    worst, cells = 0.0, 0
    for v, N in enumerate(counts):
        if not N.size:
            continue
        a, b = fit.log_prob(network, v + 1), src.log_prob(network, v + 1)
        seen = np.broadcast_to(N.sum(axis=0) >= 1000, N.shape) & np.isfinite(a) & np.isfinite(b)
        if seen.any():
            worst, cells = max(worst, float(np.abs(a[seen] - b[seen]).max())), cells + int(seen.sum())
    print("%s network: largest |log P(fit) - log P(source)| = %.4f over %d cells in columns visited >= 1000 times" %
          ("initial" if network == 0 else "transition", worst, cells))
