"""tools/avoid_time.py [--n N] [--points P] [--warmup W] [--launches K] -- k_avoid[pose] on device-resident tracks, on one GPU:
tools/well_clear_time.py's protocol, 4 M pairs x 241 points by default (two PLANAR sets of 24 P n bytes each, seeded straight tracks made
by torch), a random pose per pair, every output, the Python binding's default thresholds and response.  Three pairings are timed between
two events on torch's current stream:
  identity    pair i = column i of both sets: a streaming read of both arrays;
  ownship     n_a = 1: one ownship track against every column of set B, which is read once;
  permuted    a random permutation as idx_b: every load of set B is alone in its 64-byte sector.
In the same process and on the same buffers: k_miss_distance[pose] and k_well_clear[pose] (with the alert thresholds) each alone, the two
back to back in one timed window -- the two-pass alternative that reads the bytes twice and still has no mitigated NMAC -- and
k_miss_segments[pose], on the same three pairings; and torch.sum over the two arrays (and over set B alone, for `ownship`), which reads
the same bytes.  Each figure is the median of the launches behind the warm-up, with the smallest and the largest; the JSON line holds
every launch.  The numbers are a record (HISTORY.md section 41), not a gate."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path.insert(0, HERE)
    from em_model_manned_bayes_amd import native
    from _device_timing import PairBench, med, pair_args
    pb = PairBench(pair_args(), native)
    ms = pb.ms
    ap = native.avoid_params(1, 1, 1, 1)          # the defaults, for the alert thresholds of the well-clear launch
    pb.wc_thresholds = (ap.alert_tau_s, ap.alert_dmod_ft, ap.alert_hmd_ft, ap.alert_h_ft)

    def two_passes(xa, n_a, idx_b=0):
        pb.miss(xa, n_a, idx_b)
        pb.well_clear(xa, n_a, idx_b)

    def avoid(xa, n_a, idx_b=0):
        pb.launch("avoid_device", native.avoid_params(pb.n, n_a, pb.n, pb.P), xa, idx_b, True,
                   (pb.buf("hmd"), pb.buf("vmd"), pb.buf("vmd_mit"), pb.buf("t_cpa", torch.int32), pb.buf("t_alert", torch.int32),
                    pb.buf("flags", torch.uint8)), 12)

    kernels = (("avoid", avoid, 12), ("miss", pb.miss, 8), ("well_clear", pb.well_clear, 10), ("two_passes", two_passes, 10),
               ("segments", pb.segments, 10))
    for pairing, call in pb.pairings:
        for kernel, k, width in kernels:
            pb.run(kernel + "_" + pairing, lambda: call(k), width)
    pb.run_sums()
    out = pb.report(no_rate=("two_passes_",))
    for pairing, _ in pb.pairings:          # the expectation of HISTORY.md section 41, as figures: no assertion
        av = med(ms["avoid_" + pairing])
        out["avoid_%s_over_two_passes" % pairing] = round(av / med(ms["two_passes_" + pairing]), 3)
        out["avoid_%s_over_segments" % pairing] = round(av / med(ms["segments_" + pairing]), 3)
        out["avoid_%s_over_well_clear" % pairing] = round(av / med(ms["well_clear_" + pairing]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
