#!/usr/bin/env python3
"""examples/run_cpa_rate.py -- the NMAC rate of uncorrelated intruders against one straight and level ownship, estimated twice from the
same intruders: once with the intruders placed on an encounter cylinder (emgpu_encounter_pose_device, as run_encounter_rate.py does) and
once with the intruders placed by their closest approach (emgpu_cpa_pose_device): a drawn second at which the two pass, a lateral miss
within +-Hm and a vertical offset within +-Vm there.  Both placements hand a pose and a rate to the segment miss distance
(emgpu_miss_segments_device); the intruders, their log-weights and the ownship are run_encounter_rate.py's.

    python examples/run_cpa_rate.py [n] [sample_time] [density_per_nm3] [radius_nm] [half_height_ft] [hmd_max_ft] [vmd_max_ft]

For each placement the script prints E_w[rate * NMAC] = sum(w rate NMAC) / sum(w) in cubic feet per second with its standard error (w the
importance weight against the shipped model, NMAC at any time of the piecewise-linear tracks), and airspace density times that figure:
the NMACs per flight hour.  The two estimate the same quantity ONLY when the tracks are long enough to cross the cylinder (an intruder
that enters a 1 nm cylinder at 100 ft/s relative speed has not reached the ownship after 60 s, and its NMAC is never seen), and when
Hm >= 500 ft and Vm >= 100 ft, so that the miss plane covers every NMAC; tracks that turn after the drawn second can also pass closer at
another time than the placement intended, which the miss distance then finds.  The script asserts nothing about the two numbers; what
the CPA placement buys is the standard error per pair: every pair it places passes close by.
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
n, T, density_nm3 = arg(1, 1_000_000, int), arg(2, 60, int), arg(3, 1.0e-3)      # density: aircraft per cubic nautical mile
NM = 6076.1154855643
radius_ft, half_height_ft = arg(4, 1.0) * NM, arg(5, 500.0)
hmd_max_ft, vmd_max_ft = arg(6, 1000.0), arg(7, 200.0)
t_lo, t_hi = T // 4, (3 * T) // 4                               # the pass is drawn from the middle half of the track
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
ctx = native.Context(0, stream=stream.cuda_stream)             # the sampler, the placements and the pairing share torch's stream

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

# 3. both placements, then the segment miss distance with the pose of each; the importance weights stay apart from the rate here, so that
#    the per-pair products are at hand for the standard error
d_w = torch.from_numpy(w.view(np.int32)).to(dev).to(torch.float64)
pose, rate = torch.empty((5, n), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
pflags, mflags = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
mp = native.miss_params(n, 1, n, T + 1)


def estimate(name, lost):
    """E_w[rate * NMAC] and its standard error (the ratio estimator's: the residuals x - est * w), from rate, mflags and d_w on the device"""
    totals = torch.zeros(10, dtype=torch.int64, device=dev)
    native.miss_segments_device(mp, own.data_ptr(), xyz.data_ptr(), pose_b=pose.data_ptr(), flags=mflags.data_ptr(), totals=totals.data_ptr(),
                                stream=ctx.stream)
    nmac = ((mflags & L.MISS_NMAC_ANY) != 0).to(torch.float64)
    x = d_w * rate * nmac
    est = x.sum() / d_w.sum()
    se = torch.sqrt(((x - est * d_w) ** 2).sum()) / d_w.sum()
    ctx.sync()
    t = totals.cpu().numpy().view(np.uint64)
    est, se = float(est), float(se)
    per_hour = 3600.0 * density_nm3 / NM ** 3
    print("%-8s pairs %d, NMAC at any time %d (%.2f %%), not placed %d; E_w[rate * NMAC] = %.4e +- %.2e ft^3/s (%.2f %%); "
          "at %.3g aircraft per nm^3: %.4e +- %.1e NMACs per flight hour"
          % (name, t[0], t[2], 100.0 * float(t[2]) / max(float(t[0]), 1.0), int(lost), est, se, 100.0 * se / max(est, 1e-300), density_nm3,
             per_hour * est, per_hour * se))
    return est, se


native.encounter_pose_device(native.encounter_params(n, 1, n, T + 1, radius_ft, half_height_ft, seed=2), own.data_ptr(), xyz.data_ptr(),
                             pose=pose.data_ptr(), rate=rate.data_ptr(), flags=pflags.data_ptr(), stream=ctx.stream)
cyl = estimate("cylinder", ((pflags & L.ENC_NO_ENTRY) != 0).sum())
native.cpa_pose_device(native.cpa_pose_params(n, 1, n, T + 1, hmd_max_ft, vmd_max_ft, seed=2, t_lo=t_lo, t_hi=t_hi), own.data_ptr(), xyz.data_ptr(),
                       pose=pose.data_ptr(), rate=rate.data_ptr(), flags=pflags.data_ptr(), stream=ctx.stream)
cpa = estimate("cpa", ((pflags & L.CPA_NO_PASS) != 0).sum())
print("cylinder %.0f ft x +-%.0f ft; miss plane +-%.0f ft x +-%.0f ft at a second drawn from %d .. %d; log_scale %.4f"
      % (radius_ft, half_height_ft, hmd_max_ft, vmd_max_ft, t_lo, t_hi, log_scale))
print("standard error per pair, cpa / cylinder: %.3f; difference of the two estimates in combined standard errors: %.2f (they agree only under the "
      "conditions in this file's header)" % (cpa[1] / max(cyl[1], 1e-300), abs(cpa[0] - cyl[0]) / max(float(np.hypot(cpa[1], cyl[1])), 1e-300)))
