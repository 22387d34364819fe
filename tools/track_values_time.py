"""tools/track_values_time.py [--n N] [--T T] [--warmup W] [--launches K] [--model NAME] -- k_track_values on device-resident tracks, on one
GPU: 4 M tracks x 240 s of uncor_1200code_v2p1 by default.  The trace is sampled once (emgpu_sample_dbn_device), k_sample2track<dense> turns
it into tracks xyz [T+1][3][n], and then four things are timed between two events on the ctx stream, in the same process and on the same
buffers: k_sample2track<dense> (12 B read and 24 B written per track and second), k_track_values[PLANAR,f32] on its output (24 B read and
12 B written: the same 36 B the other way), k_track_values[ROWS,f32] on a transposed copy [n][T+1][3], and a torch copy that moves the same
number of bytes (half of them read, half written).  The two layouts' values are compared bit for bit.
Prints one JSON line.  The numbers are a record (HISTORY.md section 23), not a gate."""
import argparse
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--T", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--model", default="uncor_1200code_v2p1")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from _device_timing import timed as timed_on
    import numpy as np
    import torch
    from em_model_manned_bayes_amd import _lib as L
    from em_model_manned_bayes_amd import em_io, native
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = native.Context(0, stream=stream.cuda_stream)
    n, T, G4 = args.n, args.T, (args.T + 3) // 4
    path = em_io.materialize_model(args.model, tempfile.mkdtemp())
    parms = em_io.em_read(path)
    nm = parms["native"]
    ni, nd = nm.n_initial, nm.n_dyn
    labs = parms["labels_initial"]
    ids = [labs.index('"%s"' % s) for s in ("L", "v", "\\dot h", "\\dot v", "\\dot \\psi")]
    tm = [int(r[0]) - 1 for r in np.asarray(parms["temporal_map"]).reshape(-1, 2)]
    slots = [tm.index(v) for v in ids[2:]]
    ur = ((1852.0 / 0.3048) / 3600.0, 1.0 / 60.0, 1.0)
    bv = np.asarray(parms["boundaries"][ids[1]], dtype=np.float64)

    timed = lambda fn: timed_on(stream, fn, args.warmup, args.launches, ctx.sync)          # noqa: E731

    iv = torch.empty((ni, n), dtype=torch.float32, device=dev)
    dv = torch.empty((G4, nd, n, 4), dtype=torch.float32, device=dev)
    p, _keep = native.make_params(n, T, 7)
    native.sample_dbn_device(ctx, nm, p, init_val=iv.data_ptr(), dyn_val=dv.data_ptr())
    ctx.sync()
    xyz = torch.empty((T + 1, 3, n), dtype=torch.float64, device=dev)
    fl = torch.empty(n, dtype=torch.uint8, device=dev)
    tp = native.track_params(n, T, *ur, float(bv[0]), float(bv[-1]), nd=nd, slot_vertrate=slots[0], slot_acc=slots[1], slot_turnrate=slots[2])
    fwd_ms = timed(lambda: native.sample2track_device(ctx, tp, iv[ids[0]].data_ptr(), iv[ids[1]].data_ptr(), dv.data_ptr(), xyz.data_ptr(),
                                                      fl.data_ptr()))
    fwd_kernel = ctx.last_kernel()
    iv2, dv2 = torch.empty_like(iv), torch.zeros_like(dv)     # T - 1 seconds of values: the same 60 groups for T = 240
    kernels, ms, outs = {}, {}, {}
    for name, layout in (("planar", L.TRACKS_PLANAR), ("rows", L.TRACKS_ROWS)):
        src = xyz if layout == L.TRACKS_PLANAR else xyz.permute(2, 0, 1).contiguous()
        torch.cuda.synchronize()
        vp = native.track_values_params(n, T + 1, *ur, n_initial=ni, nd=nd, rows=ids, slots=slots, value_type=L.VALUE_F32, layout=layout)
        ms[name] = timed(lambda: native.track_values_device(ctx, vp, src.data_ptr(), iv2.data_ptr(), dv2.data_ptr()))
        kernels[name] = ctx.last_kernel()
        outs[name] = (iv2[ids].clone(), dv2.clone())
        if layout == L.TRACKS_ROWS:
            half = (24 * (T + 1) + 12 * T) * n // 2 // 8
            a, b = src.view(-1)[:half], xyz.view(-1)[:half]
            copy_ms = timed(lambda: b.copy_(a))
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs["planar"], outs["rows"]))
    mean = lambda v: sum(v) / len(v)   # noqa: E731
    nbytes = (24 * (T + 1) + 12 * T) * n
    out = {"lib": L.lib().emgpu_version().decode(), "device": torch.cuda.get_device_name(0), "model": args.model, "n": n, "T": T,
           "bytes_moved": nbytes, "forward_kernel": fwd_kernel, "forward_ms": fwd_ms, "planar_kernel": kernels["planar"],
           "planar_ms": ms["planar"], "rows_kernel": kernels["rows"], "rows_ms": ms["rows"], "copy_ms": copy_ms,
           "forward_GBps": round(nbytes / mean(fwd_ms) / 1e6, 1), "planar_GBps": round(nbytes / mean(ms["planar"]) / 1e6, 1),
           "rows_GBps": round(nbytes / mean(ms["rows"]) / 1e6, 1), "copy_GBps": round(nbytes / mean(copy_ms) / 1e6, 1),
           "ratio_planar_to_forward": round(mean(ms["planar"]) / mean(fwd_ms), 3), "ratio_rows_to_forward": round(mean(ms["rows"]) / mean(fwd_ms), 3),
           "ratio_planar_to_copy": round(mean(ms["planar"]) / mean(copy_ms), 3), "ratio_rows_to_copy": round(mean(ms["rows"]) / mean(copy_ms), 3),
           "planar_equals_rows": bool(same), "accepted": round(float((fl == 0).float().mean().item()), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
