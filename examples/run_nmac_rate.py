#!/usr/bin/env python3
"""examples/run_nmac_rate.py -- the NMAC rate of uncorrelated intruders against one straight and level ownship, and the same rate under
importance weights.  Intruders are drawn under a PROPOSAL (uncor_1200code_v2p1 with the airspace class G made uniform) together with their
log-weights against the shipped model (native.sample_weighted_host), dead-reckoned into 1 Hz tracks on the device
(emgpu_sample2track_device), turned and placed around the ownship by a random pose per pair from a seeded host generator, and paired with
the ownship on the device (emgpu_miss_distance_device: one ownship column against every intruder).  Only the eight totals come back:
totals[1] / totals[0] is the NMAC rate under the proposal, totals[6] / totals[5] the rate reweighted to the shipped model.

    python examples/run_nmac_rate.py [n] [sample_time]
"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from em_model_manned_bayes_amd import _lib as L  # noqa: E402
from em_model_manned_bayes_amd import em_io, native  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
T = int(sys.argv[2]) if len(sys.argv) > 2 else 60
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
ctx = native.Context(0, stream=stream.cuda_stream)             # the sampler and the pairing share torch's stream: ordered without a sync

# 1. intruders: sampled under the proposal, weighted against the shipped model, dead-reckoned on the device
s = native.sample_weighted_host(ctx, proposal, target, n, T, seed=1, raw=True)
w, log_scale = native.quantize_weights(s["log_weight_model"])
d_iv, d_dv = torch.from_numpy(s["init_val"]).to(dev), torch.from_numpy(s["dyn_val"]).to(dev)
xyz = torch.empty((T + 1, 3, n), dtype=torch.float64, device=dev)
bad = torch.empty(n, dtype=torch.uint8, device=dev)
tp = native.track_params(n, T, *ur, float(bv[0]), float(bv[-1]), nd=target.n_dyn, slot_vertrate=slots[0], slot_acc=slots[1], slot_turnrate=slots[2])
native.sample2track_device(ctx, tp, d_iv[ids[0]].data_ptr(), d_iv[ids[1]].data_ptr(), d_dv.data_ptr(), xyz.data_ptr(), bad.data_ptr())
print("sampled by %s; %d intruders x %d s" % (s["kernel"], n, T))

# 2. one straight and level ownship: 120 kt east at 3000 ft, from the origin
own = torch.zeros((T + 1, 3, 1), dtype=torch.float64, device=dev)
own[:, 0, 0] = torch.arange(T + 1, dtype=torch.float64, device=dev) * (120.0 * ur[0])
own[:, 2, 0] = 3000.0

# 3. a pose per pair: the intruder turned to a random heading, placed within 3 nm and 1000 ft of the ownship's start
rs = np.random.RandomState(2)
alt0 = s["init_val"][ids[0]].astype(np.float64)
pose = native.make_pose(rs.uniform(-180.0, 180.0, n), rs.uniform(-3.0, 3.0, n) * 6076.1154855643, rs.uniform(-3.0, 3.0, n) * 6076.1154855643,
                        3000.0 - alt0 + rs.uniform(-1000.0, 1000.0, n))
d_pose = torch.from_numpy(pose).to(dev)
d_w = torch.from_numpy(w.view(np.int32)).to(dev)
totals = torch.zeros(8, dtype=torch.int64, device=dev)
flags = torch.empty(n, dtype=torch.uint8, device=dev)
native.miss_distance_device(native.miss_params(n, 1, n, T + 1), own.data_ptr(), xyz.data_ptr(), pose_b=d_pose.data_ptr(), weights=d_w.data_ptr(),
                            flags=flags.data_ptr(), totals=totals.data_ptr(), stream=ctx.stream)
ctx.sync()
t = totals.cpu().numpy().view(np.uint64)

# 4. / 5. the rates
print("pairs evaluated %d, NMAC at CPA %d, NMAC at any second %d, no CPA %d" % (t[0], t[1], t[2], t[3]))
print("NMAC rate under the proposal: %.6f" % (float(t[1]) / float(t[0])))
print("NMAC rate reweighted to the shipped model: %.6f (sum of weights %d, log_scale %.4f)" % (float(t[6]) / float(t[5]), t[5], log_scale))
