#!/usr/bin/env python3
"""examples/run_encounter_rate.py -- P(NMAC | encounter) and the encounter rate of uncorrelated intruders against one straight and level
ownship, with the intruders placed on an encounter cylinder on the device.  The chain of run_nmac_rate.py with the host pose replaced:
intruders are drawn under a PROPOSAL (uncor_1200code_v2p1 with the airspace class G made uniform) together with their log-weights against
the shipped model (native.sample_weighted_host), dead-reckoned into 1 Hz tracks on the device (emgpu_sample2track_device), given a random
heading and an entry point on the cylinder around the ownship, where they fly into it (emgpu_encounter_pose_device, which also folds the
swept volume per second into the integer weights), and paired with the ownship (emgpu_miss_distance_device).  Nothing of a pair visits
the host: only the eight totals and the mean rate come back.

    python examples/run_encounter_rate.py [n] [sample_time] [density_per_nm3] [radius_nm] [half_height_ft] [--between]

With weights w * rate / rate_scale, totals[6] / totals[5] is P(NMAC | encounter) under the shipped model; airspace density times the mean
rate is the number of encounters per second of flight.  --between: the same pairs once more with the tracks read as piecewise linear
between their seconds (emgpu_miss_segments_device), which finds the NMACs that fall between two samples; both estimates are printed.
"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from em_model_manned_bayes_amd import _lib as L  # noqa: E402
from em_model_manned_bayes_amd import em_io, native  # noqa: E402

between = "--between" in sys.argv[1:]
sys.argv = [a for a in sys.argv if a != "--between"]
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
T = int(sys.argv[2]) if len(sys.argv) > 2 else 60
density_nm3 = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0e-3      # aircraft per cubic nautical mile
NM = 6076.1154855643
radius_ft = (float(sys.argv[4]) if len(sys.argv) > 4 else 1.0) * NM
half_height_ft = float(sys.argv[5]) if len(sys.argv) > 5 else 500.0
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

# 3. the placement: heading, entry point and rate per pair, the rate folded into the weights.  rate_scale is the side's swept volume at a
#    bound on the relative speed (the fastest intruder bin plus the ownship): a weight grows by at most a small factor
rate_scale = (4.0 * radius_ft * half_height_ft) * (float(bv[-1]) * ur[0] + own_speed)
d_w = torch.from_numpy(w.view(np.int32)).to(dev)
pose = torch.empty((5, n), dtype=torch.float64, device=dev)
rate = torch.empty(n, dtype=torch.float64, device=dev)
eflags = torch.empty(n, dtype=torch.uint8, device=dev)
w_rate = torch.empty(n, dtype=torch.int32, device=dev)
ep = native.encounter_params(n, 1, n, T + 1, radius_ft, half_height_ft, seed=2, rate_scale=rate_scale)
native.encounter_pose_device(ep, own.data_ptr(), xyz.data_ptr(), weights_in=d_w.data_ptr(), pose=pose.data_ptr(), rate=rate.data_ptr(),
                             flags=eflags.data_ptr(), weights_out=w_rate.data_ptr(), stream=ctx.stream)

# 4. the pairing: totals[0:5] count pairs, totals[5:8] sum w * rate / rate_scale
totals = torch.zeros(8, dtype=torch.int64, device=dev)
native.miss_distance_device(native.miss_params(n, 1, n, T + 1), own.data_ptr(), xyz.data_ptr(), pose_b=pose.data_ptr(), weights=w_rate.data_ptr(),
                            totals=totals.data_ptr(), stream=ctx.stream)
if between:
    totals_seg = torch.zeros(10, dtype=torch.int64, device=dev)
    native.miss_segments_device(native.miss_params(n, 1, n, T + 1), own.data_ptr(), xyz.data_ptr(), pose_b=pose.data_ptr(),
                                weights=w_rate.data_ptr(), totals=totals_seg.data_ptr(), stream=ctx.stream)
saturated = ((eflags & L.ENC_SATURATED) != 0).sum()
no_entry = ((eflags & L.ENC_NO_ENTRY) != 0).sum()
mean_rate = rate.mean()
mean_rate_model = (rate * d_w.to(torch.float64)).sum() / d_w.to(torch.float64).sum()      # (the example's weights are below 2^31)
ctx.sync()
t = totals.cpu().numpy().view(np.uint64)

# 5. the figures
print("pairs evaluated %d, NMAC at CPA %d, NMAC at any second %d, no CPA %d; no entry %d, saturated weights %d"
      % (t[0], t[1], t[2], t[3], int(no_entry), int(saturated)))
print("NMAC share of the placed pairs, unweighted (proposal, every pair counting 1): %.6f" % (float(t[2]) / float(t[0])))
print("P(NMAC | encounter) reweighted to the shipped model and by rate: %.6f at the CPA, %.6f at any second (sum of weights %d, log_scale %.4f)"
      % (float(t[6]) / float(t[5]), float(t[7]) / float(t[5]), t[5], log_scale))
ft3_per_nm3 = NM ** 3
for name, r in (("proposal", float(mean_rate)), ("shipped model", float(mean_rate_model))):
    print("mean rate under the %s: %.4e ft^3/s = %.6f nm^3/s; at %.3g aircraft per nm^3: %.4e encounters per second, %.4f per flight hour"
          % (name, r, r / ft3_per_nm3, density_nm3, density_nm3 * r / ft3_per_nm3, 3600.0 * density_nm3 * r / ft3_per_nm3))
if between:
    g = totals_seg.cpu().numpy().view(np.uint64)
    print("between the seconds: NMAC at CPA %d, NMAC at any time %d, of which no whole second shows %d (%.2f %%)"
          % (g[1], g[2], g[8], 100.0 * float(g[8]) / max(float(g[2]), 1.0)))
    print("P(NMAC | encounter) at any time: %.6f with the segments, %.6f at whole seconds only (ratio %.4f); at the CPA: %.6f and %.6f"
          % (float(g[7]) / float(g[5]), float(t[7]) / float(t[5]), float(g[7]) / max(float(t[7]), 1.0), float(g[6]) / float(g[5]),
             float(t[6]) / float(t[5])))
