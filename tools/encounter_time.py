"""tools/encounter_time.py [--n N] [--points P] [--warmup W] [--launches K] -- k_encounter_pose on device-resident tracks, on one GPU: 4 M
pairs x 241 points by default (two PLANAR sets, seeded straight tracks made by torch; the kernel reads points 0 and 1 alone).  Three
pairings are timed between two events on torch's current stream, every launch with all four outputs and weights_in:
  identity    pair i = column i of both sets: twelve coalesced 8-byte loads per pair;
  ownship     n_a = 1: one ownship track against every column of set B;
  permuted    a random permutation as idx_b: every load of set B is alone in its 64-byte sector.
In the same process, a torch elementwise pass is timed the same way: torch.add of two float64 tensors into a third, sized to read the
100 bytes per pair the identity launch reads (twelve doubles and a weight); it writes 50 bytes per pair where the kernel writes 53.
Each figure is the median of the launches behind the warm-up; the JSON line holds every launch.  The numbers are a record (HISTORY.md section 33), not a gate."""
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
    gen = torch.Generator(device=dev)
    gen.manual_seed(33)

    a, b = straight_tracks(n, P, dev, gen), straight_tracks(n, P, dev, gen)
    own = a[:, :, :1].contiguous()
    perm = torch.randperm(n, device=dev, generator=gen)
    w_in = torch.randint(0, 2**16, (n,), dtype=torch.int32, device=dev, generator=gen)
    pose, rate = torch.empty((5, n), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    flags, w_out = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    radius, half = 3.0 * 6076.1154855643, 1000.0
    scale = 4.0 * radius * half * 800.0
    torch.cuda.synchronize()

    def launch(xa, n_a, idx_b=0):
        native.encounter_pose_device(native.encounter_params(n, n_a, n, P, radius, half, 33, rate_scale=scale), xa.data_ptr(), b.data_ptr(), 0, idx_b,
                                     w_in.data_ptr(), pose.data_ptr(), rate.data_ptr(), flags.data_ptr(), w_out.data_ptr(), stream=stream.cuda_stream)

    ms, counts = {}, {}
    for name, fn in (("identity", lambda: launch(a, n)), ("ownship", lambda: launch(own, 1)), ("permuted", lambda: launch(a, n, perm.data_ptr()))):
        ms[name] = timed(fn)
        fl = flags.cpu().numpy()
        counts[name] = {"end": int(((fl & L.ENC_END) != 0).sum()), "fallback": int(((fl & L.ENC_FALLBACK) != 0).sum()),
                        "no_entry": int(((fl & L.ENC_NO_ENTRY) != 0).sum()), "saturated": int(((fl & L.ENC_SATURATED) != 0).sum()),
                        "mean_rate": float(rate.mean().item())}
    # the elementwise pass: z = x + y reads 16 bytes and writes 8 per element, so 100 n / 16 elements read what the kernel reads
    read_b, written_b = 100 * n, 53 * n
    k_in = read_b // 16
    x, y = torch.rand(k_in, dtype=torch.float64, device=dev, generator=gen), torch.rand(k_in, dtype=torch.float64, device=dev, generator=gen)
    z = torch.empty(k_in, dtype=torch.float64, device=dev)
    torch_ms = timed(lambda: torch.add(x, y, out=z))
    med = statistics.median
    out = {"lib": L.lib().emgpu_version().decode(), "device": torch.cuda.get_device_name(0), "n_pairs": n, "points": P,
           "bytes_read_identity": read_b, "bytes_written": written_b, "torch_add_bytes": 24 * k_in, "torch_add_elements": k_in,
           "bytes_written_by_torch_add": 8 * k_in,
           "identity_ms": ms["identity"], "ownship_ms": ms["ownship"], "permuted_ms": ms["permuted"], "torch_add_ms": torch_ms,
           "median_ms": {k: round(med(v), 4) for k, v in list(ms.items()) + [("torch_add", torch_ms)]},
           "min_max_ms": {k: [min(v), max(v)] for k, v in list(ms.items()) + [("torch_add", torch_ms)]},
           "identity_GBps": round((read_b + written_b) / med(ms["identity"]) / 1e6, 1), "torch_add_GBps": round(24 * k_in / med(torch_ms) / 1e6, 1),
           "ratio_identity_to_torch": round(med(ms["identity"]) / med(torch_ms), 3), "ratio_ownship_to_torch": round(med(ms["ownship"]) / med(torch_ms), 3),
           "ratio_permuted_to_torch": round(med(ms["permuted"]) / med(torch_ms), 3), "counts": counts}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
