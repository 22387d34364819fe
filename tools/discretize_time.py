"""tools/discretize_time.py [--n N] [--T T] [--n-fine F] [--warmup W] [--launches K] [--model NAME] -- k_discretize_dbn on a device-resident
trace of values, on one GPU: 10 M trajectories x 240 s of uncor_1200code_v2p1 by default (16 B read and 4 B written per four seconds,
variable and trajectory: 36 GB).  The trace is sampled once (emgpu_sample_dbn_device; the values are kept), then three things are timed
between two events on the ctx stream, in the same process and on the same buffers: the discretize launch (f32, n_fine fine bins), a plain read
of dyn_val (torch.sum) and an elementwise pass that reads dyn_val and writes a buffer of dyn_bin's size (torch.sum over the last axis into an
f32 array [G4, n_d, n]).  The bins of the last launch are compared with the sampler's own.
Prints one JSON line.  The numbers are a record (HISTORY.md section 22), not a gate."""
import argparse
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--T", type=int, default=240)
    ap.add_argument("--n-fine", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--model", default="uncor_1200code_v2p1")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from _device_timing import timed as timed_on
    import torch
    from em_model_manned_bayes_amd import _lib as L
    from em_model_manned_bayes_amd import em_io, native
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = native.Context(0, stream=stream.cuda_stream)
    n, T, G4 = args.n, args.T, (args.T + 3) // 4
    nm = native.NativeModel.load_txt(em_io.materialize_model(args.model, tempfile.mkdtemp()))
    ni, nd = nm.n_initial, nm.n_dyn

    timed = lambda fn: timed_on(stream, fn, args.warmup, args.launches, ctx.sync)          # noqa: E731

    ib = torch.empty((ni, n), dtype=torch.uint8, device=dev)
    db = torch.empty((G4, nd, n), dtype=torch.int32, device=dev)
    iv = torch.empty((ni, n), dtype=torch.float32, device=dev)
    dv = torch.empty((G4, nd, n, 4), dtype=torch.float32, device=dev)
    p, _keep = native.make_params(n, T, 7)
    native.sample_dbn_device(ctx, nm, p, init_bin=ib.data_ptr(), init_val=iv.data_ptr(), dyn_bin=db.data_ptr(), dyn_val=dv.data_ptr())
    ctx.sync()
    ib2, db2 = torch.empty_like(ib), torch.empty_like(db)
    rc = torch.zeros(2 * ni, dtype=torch.int64, device=dev)
    tmp = torch.empty((G4, nd, n), dtype=torch.float32, device=dev)
    dp = native.discretize_params(n, T, args.n_fine, L.VALUE_F32)
    disc_ms = timed(lambda: native.discretize_dbn_device(ctx, nm, dp, iv.data_ptr(), dv.data_ptr(), ib2.data_ptr(), db2.data_ptr(),
                                                         rc.data_ptr() if args.n_fine else 0, rc.data_ptr() + 8 * ni if args.n_fine else 0))
    kernel = ctx.last_kernel()
    read_ms = timed(lambda: torch.sum(dv))
    pass_ms = timed(lambda: torch.sum(dv, dim=3, out=tmp))
    launches = args.warmup + args.launches
    cells = ib.numel() + T * nd * n
    # cells that differ from the sampler's bins: only values whose f32 rounding reached the upper boundary of their bin (padding bytes are 0 in both)
    off = int((ib2 != ib).sum().item()) + int(((db2 ^ db).view(torch.uint8) != 0).sum().item())
    mean = lambda v: sum(v) / len(v)   # noqa: E731
    spread = lambda v: max(v) - min(v)   # noqa: E731
    nbytes = 4 * iv.numel() + ib.numel() + 4 * dv.numel() + 4 * db.numel()
    out = {"lib": L.lib().emgpu_version().decode(), "device": torch.cuda.get_device_name(0), "model": args.model, "n": n, "T": T,
           "n_fine": args.n_fine, "kernel": kernel, "bytes_moved": nbytes, "discretize_ms": disc_ms, "read_ms": read_ms, "read_write_ms": pass_ms,
           "discretize_GBps": round(nbytes / mean(disc_ms) / 1e6, 1),
           "ratio_discretize_to_read": round(mean(disc_ms) / mean(read_ms), 3),
           "ratio_discretize_to_read_write": round(mean(disc_ms) / mean(pass_ms), 3),
           "read_write_spread_ms": round(spread(pass_ms), 4),
           "cells_off_the_sampled_bins": off, "cells": cells,
           "repeat_per_launch": [int(x) // launches for x in rc[:ni].tolist()], "change_per_launch": [int(x) // launches for x in rc[ni:].tolist()]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
