#!/usr/bin/env python3
"""tools/sample2track_time.py -- sample2track with the host reader and with the device reader on the same two files, timed on one box.

  python tools/sample2track_time.py --model uncor_1200code_v2p1 -n 25000 -T 160 [--max-tracks 25000] [--dir /dev/shm] [--no-host]
                                    [--no-files] [--repeat 3]

The files are written once by em_sample(text="device").  One JSON line per run: wall seconds of sample2track and transition rows/s; for the
device reader also legacy.last_track_stats: reading the files, the library call and its phases (upload, the parse / track / CSV kernel groups
by HIP events, download, host work), writing one file per track, the bytes, hard tokens and host-formatted tracks -- and `bound_by`, the
largest of them.  With both readers the two output trees are compared byte for byte ("identical").  --no-host skips the host reader (large
runs), --no-files runs with write_files=False (a million files want a file system with the inodes for them).  The first device run of a
process pays for the context's buffers; the line to quote is the best of --repeat."""
import argparse
import filecmp
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from em_model_manned_bayes_amd import em_io, legacy, native  # noqa: E402


def same_trees(a, b):
    files = lambda r: sorted(os.path.relpath(os.path.join(d, f), r) for d, _, fs in os.walk(r) for f in fs)
    fa, fb = files(a), files(b)
    return fa == fb and all(filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False) for f in fa), len(fa)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="uncor_1200code_v2p1")
    ap.add_argument("-n", type=int, default=25000)
    ap.add_argument("-T", type=int, default=160)
    ap.add_argument("--max-tracks", type=int, default=25000)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the files go (default: /dev/shm)")
    ap.add_argument("--no-host", action="store_true", help="skip the host reader (large runs)")
    ap.add_argument("--no-files", action="store_true", help="write_files=False")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    ctx = native.Context(0)
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        path = em_io.materialize_model(a.model, d)
        fi, ft = os.path.join(d, "initial.txt"), os.path.join(d, "transition.txt")
        t0 = time.perf_counter()
        legacy.em_sample(path, fi, ft, num_initial_samples=a.n, num_transition_samples=a.T, ctx=ctx, text="device", return_arrays=False)
        common = dict(model=a.model, n=a.n, T=a.T, max_tracks=a.max_tracks, write_files=not a.no_files, dir=d)
        print(json.dumps(dict(common, what="em_sample text=device", seconds=round(time.perf_counter() - t0, 3),
                              file_bytes=os.path.getsize(fi) + os.path.getsize(ft))), flush=True)
        rows = a.n * a.T
        kw = dict(num_max_tracks=a.max_tracks, write_files=not a.no_files, verbose=False, ctx=ctx)
        out_h, out_d = os.path.join(d, "tracks_host"), os.path.join(d, "tracks_device")
        if not a.no_host:
            t0 = time.perf_counter()
            good_h, _ = legacy.sample2track(path, fi, ft, out_dir_parent=out_h, **kw)
            s = time.perf_counter() - t0
            print(json.dumps(dict(common, what="sample2track text=host", seconds=round(s, 3), rows_per_s=round(rows / s), accepted=int(good_h.sum()))), flush=True)
        for r in range(a.repeat):
            shutil.rmtree(out_d, ignore_errors=True)
            t0 = time.perf_counter()
            good_d, _ = legacy.sample2track(path, fi, ft, out_dir_parent=out_d, text="device", **kw)
            s = time.perf_counter() - t0
            st = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in legacy.last_track_stats.items()}
            phases = {k: st[k] for k in ("read_ms", "h2d_ms", "parse_ms", "track_ms", "csv_ms", "d2h_ms", "host_ms", "write_ms")}
            line = dict(common, what="sample2track text=device", run=r, seconds=round(s, 4), rows_per_s=round(rows / s), bound_by=max(phases, key=phases.get), **st)
            if not a.no_host and not a.no_files:
                line["identical"], line["files"] = same_trees(out_h, out_d)
                line["identical"] = bool(line["identical"] and (good_h == good_d).all())
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
