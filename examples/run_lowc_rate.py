#!/usr/bin/env python3
"""examples/run_lowc_rate.py -- P(LoWC | encounter) and P(NMAC | LoWC) of uncorrelated intruders against one straight and level ownship:
loss of DAA well clear (modified tau 35 s, DMOD and predicted horizontal miss 4000 ft, 450 ft vertically) beside the NMAC, both evaluated
on the device.  The chain of run_encounter_rate.py with one more link: intruders drawn under a proposal with their log-weights against the
shipped model, dead-reckoned into 1 Hz tracks (emgpu_sample2track_device), placed on an encounter cylinder around the ownship
(emgpu_encounter_pose_device), paired (emgpu_miss_distance_device) and asked for the loss of well clear (emgpu_well_clear_device, which
reads the miss kernel's flags on the device): native.encounter_well_clear runs the last three on one stream.

    python examples/run_lowc_rate.py [n] [sample_time] [radius_nm] [half_height_ft]

What a user has to learn from it: the well-clear volume is LARGE.  At 35 s and the closure of two fast aircraft it reaches tens of
thousands of feet, so an encounter cylinder of a mile or two places many intruders INSIDE it, "lost" at second 0 with no history before.
The flag WC_AT_START names those pairs, wc_totals[2] and [7] count them, and a study has to leave them out or use a cylinder whose
radius covers dmod + tau * (the largest closure).  The example prints the share for its own cylinder and for such a one.
"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from em_model_manned_bayes_amd import _lib as L  # noqa: E402
from em_model_manned_bayes_amd import em_io, native  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
T = int(sys.argv[2]) if len(sys.argv) > 2 else 60
NM = 6076.1154855643
radius_ft = (float(sys.argv[3]) if len(sys.argv) > 3 else 2.0) * NM
half_height_ft = float(sys.argv[4]) if len(sys.argv) > 4 else 1000.0
TAU_S, DMOD_FT, HMD_FT, H_FT = 35.0, 4000.0, 4000.0, 450.0
path = em_io.materialize_model("uncor_1200code_v2p1", tempfile.mkdtemp())
parms = em_io.em_read(path)
target = parms["native"]
proposal = native.NativeModel.load_txt(path)
proposal.set_f64(L.F_N_INITIAL, 1, np.ones(4))                 # variable 1: the airspace class G, a root with 4 bins
labs = parms["labels_initial"]
ids = [labs.index('"%s"' % s) for s in ("L", "v", "\\dot h", "\\dot v", "\\dot \\psi")]
tm = [int(r[0]) - 1 for r in np.asarray(parms["temporal_map"]).reshape(-1, 2)]
slots = [tm.index(v) for v in ids[2:]]
bv = np.asarray(parms["boundaries"][ids[1]], dtype=np.float64)
ur = ((1852.0 / 0.3048) / 3600.0, 1.0 / 60.0, 1.0)             # sample2track.m:113-123

dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)
ctx = native.Context(0, stream=stream.cuda_stream)             # the sampler, the placement and the pairing share torch's stream

# 1. intruders: sampled under the proposal, weighted against the shipped model, dead-reckoned on the device
s = native.sample_weighted_host(ctx, proposal, target, n, T, seed=1, raw=True)
w, log_scale = native.quantize_weights(s["log_weight_model"], bits=16)    # 16 bits: the rate takes the headroom up to 2^32 - 1
d_iv, d_dv = torch.from_numpy(s["init_val"]).to(dev), torch.from_numpy(s["dyn_val"]).to(dev)
xyz = torch.empty((T + 1, 3, n), dtype=torch.float64, device=dev)
bad = torch.empty(n, dtype=torch.uint8, device=dev)
tp = native.track_params(n, T, *ur, float(bv[0]), float(bv[-1]), nd=target.n_dyn, slot_vertrate=slots[0], slot_acc=slots[1], slot_turnrate=slots[2])
native.sample2track_device(ctx, tp, d_iv[ids[0]].data_ptr(), d_iv[ids[1]].data_ptr(), d_dv.data_ptr(), xyz.data_ptr(), bad.data_ptr())
print("sampled by %s; %d intruders x %d s" % (s["kernel"], n, T))

# 2. one straight and level ownship: 120 kt east at 3000 ft, from the origin
own_speed = 120.0 * ur[0]
own = torch.zeros((T + 1, 3, 1), dtype=torch.float64, device=dev)
own[:, 0, 0] = torch.arange(T + 1, dtype=torch.float64, device=dev) * own_speed
own[:, 2, 0] = 3000.0

# 3. the largest closure in the set: the fastest intruder second plus the ownship, whatever the headings turn out to be
step = xyz[1:, :2, :] - xyz[:-1, :2, :]
closure = float(torch.sqrt((step * step).sum(dim=1)).max()) + own_speed
wide_radius_ft = DMOD_FT + TAU_S * closure


def run(radius, seed):
    """placement on the cylinder of `radius`, NMAC and loss of well clear of the n pairs on one stream; the rate folded into the weights"""
    rate_scale = (4.0 * radius * half_height_ft) * (float(bv[-1]) * ur[0] + own_speed)
    return native.encounter_well_clear(own, xyz, radius, half_height_ft, seed, weights=w, rate_scale=rate_scale, tau_s=TAU_S, dmod_ft=DMOD_FT,
                                       hmd_ft=HMD_FT, h_ft=H_FT, layout="planar", ctx=ctx)


res = run(radius_ft, 2)
t, m = res["wc_totals"].astype(np.float64), res["totals"].astype(np.float64)
print("cylinder of %.0f ft radius and +-%.0f ft: pairs evaluated %d, lost well clear %d (inside DMOD %d, by tau %d), at second 0 %d, NMAC %d"
      % (radius_ft, half_height_ft, t[0], t[1], int(((res["wc_flags"] & L.WC_INSIDE_DMOD) != 0).sum()),
         int(((res["wc_flags"] & L.WC_BY_TAU) != 0).sum()), t[2], m[2]))
print("P(LoWC | encounter) reweighted to the shipped model and by rate: %.6f with every pair, %.6f without the pairs lost at second 0"
      % (t[6] / t[5], (t[6] - t[7]) / max(t[5] - t[7], 1.0)))
print("P(NMAC | LoWC): %.6f (NMAC at any second; P(NMAC | encounter) %.6f)" % (t[9] / max(t[6], 1.0), m[7] / m[5]))
print("share of the pairs lost at second 0 (WC_AT_START): %.4f weighted, %.4f of the pairs" % (t[7] / t[5], t[2] / t[0]))
later = res["t_first"][res["t_first"] > 0]
print("first second of the loss where it comes later: median %s, pairs %d" % (np.median(later) if later.size else "-", later.size))
big = run(wide_radius_ft, 3)["wc_totals"].astype(np.float64)
print("cylinder of %.0f ft radius = dmod + %.0f s x %.1f ft/s (the largest closure in the set): share lost at second 0 %.4f weighted, "
      "%.4f of the pairs; P(LoWC | encounter) %.6f" % (wide_radius_ft, TAU_S, closure, big[7] / big[5], big[2] / big[0], big[6] / big[5]))
