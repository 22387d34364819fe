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
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--points", type=int, default=241)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--segments", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from em_model_manned_bayes_amd import _lib as L
    from em_model_manned_bayes_amd import native
    from _device_timing import straight_tracks, timed as timed_on
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    timed = lambda fn: timed_on(stream, fn, args.warmup, args.launches)          # noqa: E731
    n, P = args.n, args.points
    gen = torch.Generator(device=dev)
    gen.manual_seed(30)

    a, b = straight_tracks(n, P, dev, gen), straight_tracks(n, P, dev, gen)
    own = a[:, :, :1].contiguous()
    rs = np.random.RandomState(30)
    pose = torch.from_numpy(native.make_pose(rs.uniform(-180.0, 180.0, n), rs.uniform(-3000.0, 3000.0, n), rs.uniform(-3000.0, 3000.0, n),
                                             rs.uniform(-300.0, 300.0, n))).to(dev)
    perm = torch.randperm(n, device=dev, generator=gen)
    hmd, vmd = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    t_cpa, flags = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    totals = torch.zeros(8, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def launch(xa, n_a, idx_b=0, with_pose=True):
        totals.zero_()
        native.miss_distance_device(native.miss_params(n, n_a, n, P), xa.data_ptr(), b.data_ptr(), 0, idx_b, pose.data_ptr() if with_pose else 0, 0,
                                    hmd.data_ptr(), vmd.data_ptr(), t_cpa.data_ptr(), flags.data_ptr(), totals.data_ptr(), stream=stream.cuda_stream)

    ms, tot = {}, {}
    for name, fn in (("identity", lambda: launch(a, n)), ("ownship", lambda: launch(own, 1)), ("permuted", lambda: launch(a, n, perm.data_ptr())),
                     ("identity_nopose", lambda: launch(a, n, with_pose=False))):
        ms[name] = timed(fn)
        tot[name] = [int(x) for x in totals.cpu().numpy().view(np.uint64)]
    if args.segments:
        t_cpa_s, totals10 = torch.empty(n, dtype=torch.float64, device=dev), torch.zeros(10, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def launch_segments(xa, n_a, idx_b=0):
            totals10.zero_()
            native.miss_segments_device(native.miss_params(n, n_a, n, P), xa.data_ptr(), b.data_ptr(), 0, idx_b, pose.data_ptr(), 0, hmd.data_ptr(),
                                        vmd.data_ptr(), t_cpa_s.data_ptr(), flags.data_ptr(), totals10.data_ptr(), stream=stream.cuda_stream)

        for name, fn in (("segments_identity", lambda: launch_segments(a, n)), ("segments_ownship", lambda: launch_segments(own, 1)),
                         ("segments_permuted", lambda: launch_segments(a, n, perm.data_ptr()))):
            ms[name] = timed(fn)
            tot[name] = [int(x) for x in totals10.cpu().numpy().view(np.uint64)]
    sum_ab = timed(lambda: (torch.sum(a), torch.sum(b)))
    sum_b = timed(lambda: torch.sum(b))
    med = statistics.median
    both, one = 2 * 24 * P * n, 24 * P * n + 24 * P
    out = {"lib": L.lib().emgpu_version().decode(), "device": torch.cuda.get_device_name(0), "n_pairs": n, "points": P,
           "bytes_read_identity": both, "bytes_read_ownship": one,
           "identity_ms": ms["identity"], "ownship_ms": ms["ownship"], "permuted_ms": ms["permuted"], "identity_nopose_ms": ms["identity_nopose"],
           "sum_both_ms": sum_ab, "sum_b_ms": sum_b,
           "median_ms": {k: round(med(v), 4) for k, v in list(ms.items()) + [("sum_both", sum_ab), ("sum_b", sum_b)]},
           "identity_GBps": round(both / med(ms["identity"]) / 1e6, 1), "ownship_GBps": round(one / med(ms["ownship"]) / 1e6, 1),
           "permuted_GBps": round(both / med(ms["permuted"]) / 1e6, 1), "sum_both_GBps": round(both / med(sum_ab) / 1e6, 1),
           "ratio_identity_to_sum": round(med(ms["identity"]) / med(sum_ab), 3), "ratio_ownship_to_sum_b": round(med(ms["ownship"]) / med(sum_b), 3),
           "ratio_permuted_to_sum": round(med(ms["permuted"]) / med(sum_ab), 3),
           "ratio_identity_nopose_to_sum": round(med(ms["identity_nopose"]) / med(sum_ab), 3), "totals": tot}
    if args.segments:
        out.update({name + "_ms": ms[name] for name in ms if name.startswith("segments_")})
        out.update({"ratio_segments_identity_to_sum": round(med(ms["segments_identity"]) / med(sum_ab), 3),
                    "ratio_segments_ownship_to_sum_b": round(med(ms["segments_ownship"]) / med(sum_b), 3),
                    "ratio_segments_permuted_to_sum": round(med(ms["segments_permuted"]) / med(sum_ab), 3),
                    "ratio_segments_identity_to_identity": round(med(ms["segments_identity"]) / med(ms["identity"]), 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
