#!/usr/bin/env python3
"""examples/run_values_round_trip.py -- values -> bins -> counts -> model, with the resample rates: draw 200 000 trajectories of 60 s under
uncor_1200code_v2p1 on the GPU, hand their VALUES to EncounterModel.count_values (discretized and counted on the device: only the tables and
the repeat / change vectors come back), set the result as the model's parameters and compare the resample rates it derives,
all_change ./ (all_repeat + all_change) (EncounterModel.m:243), with the source model's: a resampled value is uniform in its bin, so the
estimate of a dynamic variable is rate * (1 - 1 / n_fine).

    python examples/run_values_round_trip.py [n] [sample_time] [n_fine]
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from em_model_manned_bayes_amd import em_io, native  # noqa: E402
from em_model_manned_bayes_amd import encounter_model as E  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
T = int(sys.argv[2]) if len(sys.argv) > 2 else 60
n_fine = int(sys.argv[3]) if len(sys.argv) > 3 else 4
path = em_io.materialize_model("uncor_1200code_v2p1", tempfile.mkdtemp())
m = E.EncounterModel(path, idxZeroBoundaries=(1, 2, 3))
source_rates = np.asarray(m.resample_rates, dtype=np.float64).reshape(-1).copy()
ctx = native.Context(0)

s = native.sample_dbn_host(ctx, m.native, n, T, seed=1)
N_initial, N_transition, all_repeat, all_change = m.count_values(s["init_val"], s["dyn_val"], n_fine=n_fine, ctx=ctx)
print("%d initial and %d transition observations, %d pairs" %
      (sum(int(N.sum()) for N in N_initial), sum(int(N.sum()) for N in N_transition), int(all_repeat.sum() + all_change.sum())))
with np.errstate(invalid="ignore"):          # a static variable has no pairs: 0 / 0, as in the reference
    m.setParameters(N_initial, N_transition, all_repeat, all_change)
for v, (lab, got) in enumerate(zip(m.labels_initial, np.asarray(m.resample_rates).reshape(-1))):
    if all_repeat[v, 0] + all_change[v, 0] > 0:
        print("%-12s rate from the values / (1 - 1/%d) = %.5f, source model %.5f" % (lab, n_fine, got / (1 - 1 / n_fine), source_rates[v]))
