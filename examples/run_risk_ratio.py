#!/usr/bin/env python3
"""examples/run_risk_ratio.py -- the risk ratio of a vertical avoidance manoeuvre against uncorrelated intruders: P(NMAC with the
manoeuvre) / P(NMAC without), for one straight and level ownship, with everything between the sampler and the totals on the device.  The
chain of run_cpa_rate.py with one more link: intruders drawn under a proposal with their log-weights against the shipped model,
dead-reckoned into 1 Hz tracks (emgpu_sample2track_device), placed by a drawn closest approach (emgpu_cpa_pose_device), and then flown
against an ownship that answers its first alert with a climb or a descent (emgpu_avoid_device): native.cpa_avoid runs the last two on one
stream, the pose and the rate-folded weights never leaving the device.

    python examples/run_risk_ratio.py [n] [sample_time] [hmd_max_ft] [vmd_max_ft]

For each delay between the alert and the manoeuvre the script prints the weighted unmitigated and mitigated NMAC rates per encounter,
sum(w rate NMAC) / sum(w rate), and their quotient, the risk ratio, with the share of the pairs that were alerted and the number of
induced NMACs (an NMAC with the manoeuvre only).  The unmitigated rate does not depend on the delay.  The alert volume, the response
(1500 ft/min after the delay at about 0.25 g) and the sweep are an ILLUSTRATION of the machinery, not the alerting thresholds of any
standard, and the intruder never reacts; the ratio says how much a late manoeuvre costs, not how well a fielded system works.
"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from em_model_manned_bayes_amd import _lib as L  # noqa: E402
from em_model_manned_bayes_amd import em_io, native  # noqa: E402

arg = lambda k, default, kind=float: kind(sys.argv[k]) if len(sys.argv) > k else default          # noqa: E731
n, T = arg(1, 200_000, int), arg(2, 120, int)
hmd_max_ft, vmd_max_ft = arg(3, 1000.0), arg(4, 200.0)
t_lo, t_hi = T // 4, (3 * T) // 4                               # the pass is drawn from the middle half of the track
DELAYS = (0, 2, 5, 10, 15, 20, 30)
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
ctx = native.Context(0, stream=stream.cuda_stream)             # the sampler, the placement and the manoeuvre share torch's stream

# 1. intruders: sampled under the proposal, weighted against the shipped model, dead-reckoned on the device
s = native.sample_weighted_host(ctx, proposal, target, n, T, seed=1, raw=True)
w, log_scale = native.quantize_weights(s["log_weight_model"], bits=16)
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

# 3. the placement and the manoeuvre, once per delay: the same seed, so the same passes; the flux through the miss plane at the largest
#    relative speed is the rate that keeps a weight as it is
rate_scale = (4.0 * hmd_max_ft * vmd_max_ft) * (float(bv[-1]) * ur[0] + own_speed)
print("miss plane +-%.0f ft x +-%.0f ft at a second drawn from %d .. %d; log_scale %.4f" % (hmd_max_ft, vmd_max_ft, t_lo, t_hi, log_scale))
print("delay_s  alerted  P(NMAC) unmitigated  P(NMAC) mitigated  risk ratio  induced")
for delay in DELAYS:
    r = native.cpa_avoid(own, xyz, hmd_max_ft, vmd_max_ft, 2, t_lo, t_hi, weights=w, rate_scale=rate_scale, delay_s=delay, layout="planar", ctx=ctx)
    t = r["totals"].astype(np.float64)
    print("%7d  %6.1f%%  %19.5f  %17.5f  %10.4f  %7d" % (delay, 100.0 * t[8] / max(t[7], 1.0), t[9] / max(t[7], 1.0), t[10] / max(t[7], 1.0),
                                                       r["risk_ratio"], int(r["totals"][4])))
