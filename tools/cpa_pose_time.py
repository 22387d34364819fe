"""tools/cpa_pose_time.py [--n N] [--points P] [--warmup W] [--launches K] -- k_cpa_pose on device-resident tracks, on one GPU: 4 M pairs x
241 points by default (two PLANAR sets, seeded straight tracks made by torch).  Three launches are timed between two events on torch's
current stream, each with all five outputs and weights_in:
  fixed       t_lo = t_hi = 0, pair i = column i of both sets: ten coalesced 8-byte loads per pair (k_encounter_pose's rows);
  ownship     the same second, n_a = 1: one ownship track against every column of set B;
  drawn       t_lo = 100, t_hi = 125: the lanes of a wave read 26 different rows, most loads alone in their 64-byte sector.
In the same process and on the same buffers, k_encounter_pose is timed with identity pairing, with one ownship and with a random
permutation as idx_b (tools/encounter_time.py's three), and so is that tool's torch elementwise pass: torch.add of two float64 tensors into
a third, sized to read 100 bytes per pair.  Each figure is the median of the launches behind the warm-up; the JSON line holds every launch.
The numbers are a record (HISTORY.md section 37), not a gate."""
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
    import torch
    from em_model_manned_bayes_amd import _lib as L
    from em_model_manned_bayes_amd import native
    from _device_timing import straight_tracks, timed as timed_on
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    timed = lambda fn: timed_on(stream, fn, args.warmup, args.launches)          # noqa: E731
    n, P = args.n, args.points
    t_lo, t_hi = min(100, P - 2), min(125, P - 2)
    gen = torch.Generator(device=dev)
    gen.manual_seed(37)

    a, b = straight_tracks(n, P, dev, gen), straight_tracks(n, P, dev, gen)
    own = a[:, :, :1].contiguous()
    perm = torch.randperm(n, device=dev, generator=gen)
    w_in = torch.randint(0, 2**16, (n,), dtype=torch.int32, device=dev, generator=gen)
    pose, rate = torch.empty((5, n), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    t_cpa = torch.empty(n, dtype=torch.int32, device=dev)
    flags, w_out = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    hm, vm = 3000.0, 500.0
    radius, half = 3.0 * 6076.1154855643, 1000.0
    torch.cuda.synchronize()

    def cpa(xa, n_a, lo, hi):
        native.cpa_pose_device(native.cpa_pose_params(n, n_a, n, P, hm, vm, 37, lo, hi, rate_scale=4.0 * hm * vm * 800.0), xa.data_ptr(), b.data_ptr(),
                               0, 0, w_in.data_ptr(), pose.data_ptr(), rate.data_ptr(), t_cpa.data_ptr(), flags.data_ptr(), w_out.data_ptr(),
                               stream=stream.cuda_stream)

    def cylinder(xa, n_a, idx_b=0):
        native.encounter_pose_device(native.encounter_params(n, n_a, n, P, radius, half, 33, rate_scale=4.0 * radius * half * 800.0), xa.data_ptr(),
                                     b.data_ptr(), 0, idx_b, w_in.data_ptr(), pose.data_ptr(), rate.data_ptr(), flags.data_ptr(), w_out.data_ptr(),
                                     stream=stream.cuda_stream)

    ms, counts = {}, {}
    for name, fn in (("fixed", lambda: cpa(a, n, 0, 0)), ("ownship", lambda: cpa(own, 1, 0, 0)), ("drawn", lambda: cpa(a, n, t_lo, t_hi))):
        ms[name] = timed(fn)
        fl = flags.cpu().numpy()
        counts[name] = {"fallback": int(((fl & L.CPA_FALLBACK) != 0).sum()), "no_pass": int(((fl & L.CPA_NO_PASS) != 0).sum()),
                        "saturated": int(((fl & L.CPA_SATURATED) != 0).sum()), "mean_rate": float(rate.mean().item()),
                        "t_cpa_min_max": [int(t_cpa.min().item()), int(t_cpa.max().item())]}
    for name, fn in (("encounter_identity", lambda: cylinder(a, n)), ("encounter_ownship", lambda: cylinder(own, 1)),
                     ("encounter_permuted", lambda: cylinder(a, n, perm.data_ptr()))):
        ms[name] = timed(fn)
    # the elementwise pass of tools/encounter_time.py: z = x + y reads 16 bytes and writes 8 per element, 100 n / 16 elements
    k_in = 100 * n // 16
    x, y = torch.rand(k_in, dtype=torch.float64, device=dev, generator=gen), torch.rand(k_in, dtype=torch.float64, device=dev, generator=gen)
    z = torch.empty(k_in, dtype=torch.float64, device=dev)
    ms["torch_add"] = timed(lambda: torch.add(x, y, out=z))
    med = {k: statistics.median(v) for k, v in ms.items()}
    read_b, written_b = (10 * 8 + 4) * n, (40 + 8 + 4 + 1 + 4) * n
    out = {"lib": L.lib().emgpu_version().decode(), "device": torch.cuda.get_device_name(0), "n_pairs": n, "points": P, "drawn_seconds": [t_lo, t_hi],
           "bytes_read_fixed": read_b, "bytes_written": written_b, "torch_add_bytes": 24 * k_in, "ms": ms,
           "median_ms": {k: round(v, 4) for k, v in med.items()}, "min_max_ms": {k: [min(v), max(v)] for k, v in ms.items()},
           "fixed_GBps": round((read_b + written_b) / med["fixed"] / 1e6, 1), "torch_add_GBps": round(24 * k_in / med["torch_add"] / 1e6, 1),
           "ratio_fixed_to_encounter_identity": round(med["fixed"] / med["encounter_identity"], 3),
           "ratio_ownship_to_encounter_ownship": round(med["ownship"] / med["encounter_ownship"], 3),
           "ratio_drawn_to_encounter_permuted": round(med["drawn"] / med["encounter_permuted"], 3),
           "ratio_to_torch": {k: round(med[k] / med["torch_add"], 3) for k in ("fixed", "ownship", "drawn", "encounter_identity", "encounter_permuted")},
           "counts": counts}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
