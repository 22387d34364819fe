#!/usr/bin/env python3
"""examples/run_tracks_round_trip.py -- tracks -> values -> bins -> counts -> model -> file: draw trajectories under uncor_1200code_v2p1 on the
GPU, turn them into 1 Hz TRACKS with sample2track, and re-estimate the model from the tracks it accepts: UncorEncounterModel.count_tracks
derives the values of a trace from the positions (k_track_values), discretizes and counts them on the device (only the tables and the
repeat / change vectors come back), setParameters makes them the model, em_write writes it and em_read reads it back.  The resample rates
the new model derives, all_change ./ (all_repeat + all_change) (EncounterModel.m:243), are printed beside the source model's: a resampled
value is uniform in its bin, so the estimate of a dynamic variable is rate * (1 - 1 / n_fine).

    python examples/run_tracks_round_trip.py [n] [sample_time] [n_fine]
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from em_model_manned_bayes_amd import em_io, native  # noqa: E402
from em_model_manned_bayes_amd import encounter_model as E  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
T = int(sys.argv[2]) if len(sys.argv) > 2 else 61
n_fine = int(sys.argv[3]) if len(sys.argv) > 3 else 4
tmp = tempfile.mkdtemp()
path = em_io.materialize_model("uncor_1200code_v2p1", tmp)
m = E.UncorEncounterModel(parameters_filename=path)
source_rates = np.asarray(m.resample_rates, dtype=np.float64).reshape(-1).copy()
ctx = native.Context(0)

idxL, idxV, idxDV, idxDH, idxDPsi = m._track_variables()
slots = [int(np.nonzero(m.temporal_map[:, 0] == v)[0][0]) for v in (idxDH, idxDV, idxDPsi)]
s = native.sample_dbn_host(ctx, m.native, n, T, seed=1)
iv, dv = s["init_val"].astype(np.float64), s["dyn_val"].astype(np.float64)
b_v = np.asarray(m.boundaries[idxV - 1], dtype=np.float64).reshape(-1)
ur = ((1852.0 / 0.3048) / 3600.0, 1.0 / 60.0, 1.0)                      # sample2track.m:113-123
xyz, flags, _ = native.sample2track_host(ctx, iv[:, idxL - 1], iv[:, idxV - 1], dv[:, :, slots], *ur, float(b_v[0]), float(b_v[-1]))
keep = flags == 0
print("%d of %d tracks accepted (%.2f %%), %d points each" % (keep.sum(), n, 100.0 * keep.mean(), xyz.shape[1]))

# a track carries neither the airspace class G nor the altitude layer's companion A: they come with the tracks
static = {v + 1: iv[keep, v] for v in range(m.n_initial) if v + 1 not in (idxL, idxV, idxDV, idxDH, idxDPsi)}
N_initial, N_transition, all_repeat, all_change = m.count_tracks(xyz[keep], static, n_fine=n_fine, ctx=ctx)
print("%d initial and %d transition observations, %d pairs" %
      (sum(int(N.sum()) for N in N_initial), sum(int(N.sum()) for N in N_transition), int(all_repeat.sum() + all_change.sum())))
with np.errstate(invalid="ignore"):          # a static variable has no pairs: 0 / 0, as in the reference
    m.setParameters(N_initial, N_transition, all_repeat, all_change)
m.resample_rates = np.nan_to_num(np.asarray(m.resample_rates, dtype=np.float64))   # the file holds numbers: a static variable's 0 / 0 is written 0
out = os.path.join(tmp, "from_tracks.txt")
em_io.em_write(m.struct(), out)
back = em_io.em_read(out)
rates = np.asarray(back["resample_rates"], dtype=np.float64).reshape(-1)
for v, lab in enumerate(m.labels_initial):
    if all_repeat[v, 0] + all_change[v, 0] > 0:
        print("%-12s rate from the tracks / (1 - 1/%d) = %.5f, source model %.5f" % (lab, n_fine, rates[v] / (1 - 1 / n_fine), source_rates[v]))
print("written and read back: %s" % out)
