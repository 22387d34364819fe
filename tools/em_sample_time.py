#!/usr/bin/env python3
"""tools/em_sample_time.py -- em_sample with the host writer and with the device writer, timed on one box.

  python tools/em_sample_time.py --model uncor_1200code_v2p1 -n 25000 -T 160 [--dir /dev/shm] [--no-host] [--no-arrays] [--repeat 3]

One JSON line per run: wall seconds of em_sample, and for the device writer the phases of its library calls (emgpu_host_stats summed over
the calls: kernel_ms = sampler + formatter launches, d2h_ms, scatter_ms), the time spent in file writes, rows/s and GB/s of text; beside them
what emgpu_sample_dbn_host alone takes for the same n and T (the floor: the dense trace sampled and copied, nothing formatted).  The first
device run of a process pays for the context's buffers; the line to quote is the best of --repeat."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from em_model_manned_bayes_amd import em_io, legacy, native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="uncor_1200code_v2p1")
    ap.add_argument("-n", type=int, default=25000)
    ap.add_argument("-T", type=int, default=160)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the files go (default: /dev/shm)")
    ap.add_argument("--no-host", action="store_true", help="skip the host writer (large runs)")
    ap.add_argument("--no-arrays", action="store_true", help="device writer with return_arrays=False")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    ctx = native.Context(0)
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        path = em_io.materialize_model(a.model, d)
        fi, ft = os.path.join(d, "initial.txt"), os.path.join(d, "transition.txt")
        common = dict(model=a.model, n=a.n, T=a.T, dir=d)
        nm = native.NativeModel.load_txt(path)
        best = None
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            res = native.sample_dbn_host(ctx, nm, a.n, a.T, 42, want_dense=True, max_attempts=1, raw=True)
            s = time.perf_counter() - t0
            if best is None or s < best[0]:
                best = (s, res["host_stats"])
            del res
        print(json.dumps(dict(common, what="sample_dbn_host alone (raw arrays)", seconds=round(best[0], 4), kernel_ms=round(best[1]["kernel_ms"], 3),
                              d2h_ms=round(best[1]["d2h_ms"], 3))), flush=True)
        if not a.no_host:
            t0 = time.perf_counter()
            legacy.em_sample(path, fi, ft, num_initial_samples=a.n, num_transition_samples=a.T, ctx=ctx)
            s = time.perf_counter() - t0
            rows = a.n * a.T
            print(json.dumps(dict(common, what="em_sample text=host", seconds=round(s, 3), rows_per_s=round(rows / s), file_bytes=os.path.getsize(fi) + os.path.getsize(ft))),
                  flush=True)
        for r in range(a.repeat):
            t0 = time.perf_counter()
            legacy.em_sample(path, fi, ft, num_initial_samples=a.n, num_transition_samples=a.T, ctx=ctx, text="device", return_arrays=not a.no_arrays)
            s = time.perf_counter() - t0
            st = dict(legacy.last_text_stats)
            rows = a.n * a.T
            print(json.dumps(dict(common, what="em_sample text=device" + (" return_arrays=False" if a.no_arrays else ""), run=r, seconds=round(s, 4),
                                  rows_per_s=round(rows / s), text_GB_per_s=round(st["bytes"] / s / 1e9, 3), calls=st["calls"], batch=st["batch"],
                                  library_ms=round(st["library_ms"], 2), kernel_ms=round(st["kernel_ms"], 3), d2h_ms=round(st["d2h_ms"], 3),
                                  scatter_ms=round(st["scatter_ms"], 3), write_ms=round(st["write_ms"], 2), text_bytes=st["bytes"])), flush=True)


if __name__ == "__main__":
    main()
