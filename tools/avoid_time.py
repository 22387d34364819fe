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
    f64 = lambda: torch.empty(n, dtype=torch.float64, device=dev)          # noqa: E731
    i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)          # noqa: E731
    u8 = lambda: torch.empty(n, dtype=torch.uint8, device=dev)          # noqa: E731
    hmd, vmd, vmd_mit, t_cpa_s, tau_min, t_cpa, t_alert, n_lost, miss_flags, flags = f64(), f64(), f64(), f64(), f64(), i32(), i32(), i32(), u8(), u8()
    totals8, totals10, totals12 = (torch.zeros(k, dtype=torch.int64, device=dev) for k in (8, 10, 12))
    torch.cuda.synchronize()
    ap_ = native.avoid_params(1, 1, 1, 1)          # the defaults, for the alert thresholds of the well-clear launch
    mp = lambda n_a: native.miss_params(n, n_a, n, P)          # noqa: E731
    wp = lambda n_a: native.well_clear_params(n, n_a, n, P, ap_.alert_tau_s, ap_.alert_dmod_ft, ap_.alert_hmd_ft, ap_.alert_h_ft)          # noqa: E731
    vp = lambda n_a: native.avoid_params(n, n_a, n, P)          # noqa: E731

    def miss(xa, n_a, idx_b=0):
        totals8.zero_()
        native.miss_distance_device(mp(n_a), xa.data_ptr(), b.data_ptr(), 0, idx_b, pose.data_ptr(), 0, hmd.data_ptr(), vmd.data_ptr(),
                                    t_cpa.data_ptr(), miss_flags.data_ptr(), totals8.data_ptr(), stream=stream.cuda_stream)

    def segments(xa, n_a, idx_b=0):
        totals10.zero_()
        native.miss_segments_device(mp(n_a), xa.data_ptr(), b.data_ptr(), 0, idx_b, pose.data_ptr(), 0, hmd.data_ptr(), vmd.data_ptr(),
                                    t_cpa_s.data_ptr(), flags.data_ptr(), totals10.data_ptr(), stream=stream.cuda_stream)

    def well_clear(xa, n_a, idx_b=0):
        totals10.zero_()
        native.well_clear_device(wp(n_a), xa.data_ptr(), b.data_ptr(), 0, idx_b, pose.data_ptr(), 0, miss_flags.data_ptr(), t_alert.data_ptr(),
                                 n_lost.data_ptr(), tau_min.data_ptr(), flags.data_ptr(), totals10.data_ptr(), stream=stream.cuda_stream)

    def two_passes(xa, n_a, idx_b=0):
        miss(xa, n_a, idx_b)
        well_clear(xa, n_a, idx_b)

    def avoid(xa, n_a, idx_b=0):
        totals12.zero_()
        native.avoid_device(vp(n_a), xa.data_ptr(), b.data_ptr(), 0, idx_b, pose.data_ptr(), 0, hmd.data_ptr(), vmd.data_ptr(), vmd_mit.data_ptr(),
                            t_cpa.data_ptr(), t_alert.data_ptr(), flags.data_ptr(), totals12.data_ptr(), stream=stream.cuda_stream)

    ms, tot = {}, {}
    pairings = (("identity", lambda k: k(a, n)), ("ownship", lambda k: k(own, 1)), ("permuted", lambda k: k(a, n, perm.data_ptr())))
    kernels = (("avoid", avoid, totals12), ("miss", miss, totals8), ("well_clear", well_clear, totals10), ("two_passes", two_passes, totals10),
               ("segments", segments, totals10))
    for pairing, call in pairings:
        for kernel, k, totals in kernels:
            ms[kernel + "_" + pairing] = timed(lambda: call(k))
            tot[kernel + "_" + pairing] = [int(x) for x in totals.cpu().numpy().view(np.uint64)]
    ms["sum_both"] = timed(lambda: (torch.sum(a), torch.sum(b)))
    ms["sum_b"] = timed(lambda: torch.sum(b))
    med = statistics.median
    both, one = 2 * 24 * P * n, 24 * P * n + 24 * P
    read = {"identity": both, "ownship": one, "permuted": both}
    base = {"identity": "sum_both", "ownship": "sum_b", "permuted": "sum_both"}
    once = [k for k in ms if not k.startswith("sum_") and not k.startswith("two_passes_")]
    out = {"lib": L.lib().emgpu_version().decode(), "device": torch.cuda.get_device_name(0), "n_pairs": n, "points": P,
           "bytes_read_identity": both, "bytes_read_ownship": one, "ms": ms,
           "median_min_max_ms": {k: [round(med(v), 4), min(v), max(v)] for k, v in ms.items()},
           "GBps": {k: round(read[k.rsplit("_", 1)[1]] / med(ms[k]) / 1e6, 1) for k in once},
           "ratio_to_sum": {k: round(med(v) / med(ms[base[k.rsplit("_", 1)[1]]]), 3) for k, v in ms.items() if not k.startswith("sum_")},
           "sum_both_GBps": round(both / med(ms["sum_both"]) / 1e6, 1), "totals": tot}
    for pairing, _ in pairings:          # the expectation of HISTORY.md section 41, as figures: no assertion
        av = med(ms["avoid_" + pairing])
        out["avoid_%s_over_two_passes" % pairing] = round(av / med(ms["two_passes_" + pairing]), 3)
        out["avoid_%s_over_segments" % pairing] = round(av / med(ms["segments_" + pairing]), 3)
        out["avoid_%s_over_well_clear" % pairing] = round(av / med(ms["well_clear_" + pairing]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
