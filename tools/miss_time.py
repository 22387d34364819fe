"""tools/miss_time.py [--n N] [--points P] [--warmup W] [--launches K] [--segments] -- k_miss_distance on device-resident tracks, on one GPU: 4 M pairs x
241 points by default (two PLANAR sets of 24 P n bytes each, seeded straight tracks made by torch).  Three pairings are timed between
two events on torch's current stream, every launch with a random pose per pair and all five outputs:
  identity    pair i = column i of both sets: a streaming read of both arrays;
  ownship     n_a = 1: one ownship track against every column of set B, which is read once;
  permuted    a random permutation as idx_b: every load of set B is alone in its 64-byte sector.
In the same process and on the same buffers, torch.sum over the two arrays (and over set B alone, for `ownship`) reads the same bytes.
Each figure is the median of the launches behind the warm-up; the JSON line holds every launch.  identity_nopose_ms is the identity pairing
without a pose.  --segments: k_miss_segments[pose] on the same three pairings, in the same process and on the same buffers (t_cpa_s and ten
totals of its own), as segments_*_ms beside the others.  The numbers are a record (HISTORY.md sections 30 and 36), not a gate."""
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path.insert(0, HERE)
    from em_model_manned_bayes_amd import native
    from _device_timing import PairBench, med, pair_args
    args = pair_args("--segments")
    pb = PairBench(args, native)
    for pairing, call in pb.pairings:
        pb.run(pairing, lambda: call(pb.miss), 8)
    pb.run("identity_nopose", lambda: pb.miss(pb.a, pb.n, with_pose=False), 8)
    if args.segments:
        for pairing, call in pb.pairings:
            pb.run("segments_" + pairing, lambda: call(pb.segments), 10)
    pb.run_sums()
    ms = pb.ms
    out, both, one = pb.head()
    ratio = lambda k, base: round(med(ms[k]) / med(ms[base]), 3)          # noqa: E731
    out.update({"identity_ms": ms["identity"], "ownship_ms": ms["ownship"], "permuted_ms": ms["permuted"], "identity_nopose_ms": ms["identity_nopose"],
                "sum_both_ms": ms["sum_both"], "sum_b_ms": ms["sum_b"], "median_ms": {k: round(med(v), 4) for k, v in ms.items()},
                "identity_GBps": round(both / med(ms["identity"]) / 1e6, 1), "ownship_GBps": round(one / med(ms["ownship"]) / 1e6, 1),
                "permuted_GBps": round(both / med(ms["permuted"]) / 1e6, 1), "sum_both_GBps": round(both / med(ms["sum_both"]) / 1e6, 1),
                "ratio_identity_to_sum": ratio("identity", "sum_both"), "ratio_ownship_to_sum_b": ratio("ownship", "sum_b"),
                "ratio_permuted_to_sum": ratio("permuted", "sum_both"), "ratio_identity_nopose_to_sum": ratio("identity_nopose", "sum_both"),
                "totals": pb.tot})
    if args.segments:
        out.update({name + "_ms": ms[name] for name in ms if name.startswith("segments_")})
        out.update({"ratio_segments_identity_to_sum": ratio("segments_identity", "sum_both"),
                    "ratio_segments_ownship_to_sum_b": ratio("segments_ownship", "sum_b"),
                    "ratio_segments_permuted_to_sum": ratio("segments_permuted", "sum_both"),
                    "ratio_segments_identity_to_identity": ratio("segments_identity", "identity")})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
