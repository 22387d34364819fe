"""tools/well_clear_time.py [--n N] [--points P] [--warmup W] [--launches K] -- k_well_clear[pose] on device-resident tracks, on one GPU:
tools/miss_time.py's protocol, 4 M pairs x 241 points by default (two PLANAR sets of 24 P n bytes each, seeded straight tracks made by
torch), a random pose per pair, every output, a miss kernel's flags as miss_flags.  Three pairings are timed between two events on torch's
current stream:
  identity    pair i = column i of both sets: a streaming read of both arrays;
  ownship     n_a = 1: one ownship track against every column of set B, which is read once;
  permuted    a random permutation as idx_b: every load of set B is alone in its 64-byte sector.
In the same process and on the same buffers: k_miss_distance[pose] and k_miss_segments[pose] on the same three pairings, and torch.sum over
the two arrays (and over set B alone, for `ownship`), which reads the same bytes.  Each figure is the median of the launches behind the
warm-up, with the smallest and the largest; the JSON line holds every launch.  The numbers are a record (HISTORY.md section 38), not a gate."""
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path.insert(0, HERE)
    from em_model_manned_bayes_amd import native
    from _device_timing import PairBench, med, pair_args
    pb = PairBench(pair_args(), native)
    ms = pb.ms
    for pairing, call in pb.pairings:          # the miss kernel first: its flags of this pairing are the well-clear launch's miss_flags
        for kernel, k, width in (("miss", pb.miss, 8), ("well_clear", pb.well_clear, 10), ("segments", pb.segments, 10)):
            pb.run(kernel + "_" + pairing, lambda: call(k), width)
    pb.run_sums()
    out = pb.report()
    for pairing, _ in pb.pairings:          # the expectation of HISTORY.md section 38, as figures: no assertion
        seg = ms["segments_" + pairing]
        out["well_clear_%s_minus_segments_ms" % pairing] = round(med(ms["well_clear_" + pairing]) - med(seg), 4)
        out["segments_%s_spread_ms" % pairing] = round(max(seg) - min(seg), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
