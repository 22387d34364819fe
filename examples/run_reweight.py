#!/usr/bin/env python3
"""examples/run_reweight.py -- importance sampling back into a model: draw trajectories under a PROPOSAL (uncor_1200code_v2p1 with the
airspace class G made uniform: N_initial{G} flattened to ones), weight every trajectory by P(trajectory | shipped model) / P(trajectory |
proposal) and count the trace with those weights where it lies (native.reweight_count_host: the trace never leaves the device, only two
log-likelihoods per trajectory come down and one uint32 weight per trajectory goes up).  The weighted tables, handed to setParameters, make
the reweighted trace the model; it is written with em_write, and the estimated P(G) is printed beside the shipped model's.

    python examples/run_reweight.py [n] [sample_time] [out.txt]
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from em_model_manned_bayes_amd import _lib as L  # noqa: E402
from em_model_manned_bayes_amd import em_io, native  # noqa: E402
from em_model_manned_bayes_amd import encounter_model as E  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
T = int(sys.argv[2]) if len(sys.argv) > 2 else 60
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(tempfile.mkdtemp(), "uncor_reweighted.txt")
path = em_io.materialize_model("uncor_1200code_v2p1", tempfile.mkdtemp())
target = native.NativeModel.load_txt(path)
proposal = native.NativeModel.load_txt(path)
G = 0                                                         # variable 1 of the model: the airspace class, a root with 4 bins
proposal.set_f64(L.F_N_INITIAL, G + 1, np.ones(4))
ctx = native.Context(0)

got = native.reweight_count_host(ctx, proposal, target, n, T, seed=1)
print("sampled by %s, scored by %s, counted by %s" % (got["kernel"], got["score_kernel"], got["count_kernel"]))
w = got["weights"]
print("weights: %d distinct values, largest : smallest = %.1f : 1, log_scale %.4f, ess %.0f = %.3f n" %
      (len(np.unique(w)), float(w.max()) / max(float(w[w > 0].min()), 1.0), got["log_scale"], got["ess"], got["ess"] / n))

m = E.EncounterModel(path, idxZeroBoundaries=(1, 2, 3))
m.setParameters(got["N_initial"], got["N_transition"], None, None)    # (None, None: the resample rates stay the shipped model's)
em_io.em_write(m.struct(), out)
print("wrote", out)

est = got["N_initial"][G][:, 0] / got["N_initial"][G].sum()
true = np.exp(target.log_prob(0, G + 1)).reshape(-1)
for c in range(4):
    print("P(G = %d): estimated %.5f, shipped model %.5f, proposal 0.25" % (c + 1, est[c], true[c]))
