"""tools/score_time.py [--n N] [--T T] [--warmup W] [--launches K] -- k_score_dbn on a device-resident trace, on one GPU: 10 M trajectories x
240 s, three cases: uncor_1200code_v2p1 under REFERENCE_AUTO (the frozen form), the same trace under PER_STEP, and glider_v1 (dependent
branch: per step).  Each case samples its trace once (emgpu_sample_dbn_device; the bins are kept), then times the score launch between two events on
the ctx stream, beside a plain read of the same init_bin + dyn_bin bytes in the same process: torch.sum over the two buffers.  Prints one JSON
line: per case the kernel, the bytes read, the milliseconds of every launch, GB/s, and the ratio of the mean score time to the mean read time.
The ratio is a record (HISTORY.md section 20), not a gate."""
import argparse
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("uncor_1200code_v2p1", "AUTO"), ("uncor_1200code_v2p1", "PER_STEP"), ("glider_v1", "AUTO")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--T", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from _device_timing import timed as timed_on
    import torch
    from em_model_manned_bayes_amd import em_io, native, _lib as L
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = native.Context(0, stream=stream.cuda_stream)
    n, T, G4 = args.n, args.T, (args.T + 3) // 4
    out = {"lib": L.lib().emgpu_version().decode(), "device": torch.cuda.get_device_name(0), "n": n, "T": T, "cases": {}}

    timed = lambda fn: timed_on(stream, fn, args.warmup, args.launches, ctx.sync)          # noqa: E731

    trace = {}
    for name, mode in CASES:
        nm = native.NativeModel.load_txt(em_io.materialize_model(name, tempfile.mkdtemp()))
        tmode = L.TRANSITION_PER_STEP if mode == "PER_STEP" else L.TRANSITION_REFERENCE_AUTO
        if name not in trace:
            trace.clear()
            torch.cuda.empty_cache()
            ib = torch.empty((nm.n_initial, n), dtype=torch.uint8, device=dev)
            db = torch.empty((G4, nm.n_dyn, n), dtype=torch.int32, device=dev)
            iv = torch.empty((nm.n_initial, n), dtype=torch.float32, device=dev)
            dv = torch.empty((G4, nm.n_dyn, n, 4), dtype=torch.float32, device=dev)   # the sampler's usual dense call; only the bins are kept
            p, _keep = native.make_params(n, T, 7)
            native.sample_dbn_device(ctx, nm, p, init_bin=ib.data_ptr(), init_val=iv.data_ptr(), dyn_bin=db.data_ptr(), dyn_val=dv.data_ptr())
            ctx.sync()
            del iv, dv
            torch.cuda.empty_cache()
            trace[name] = (ib, db)
        ib, db = trace[name]
        ll = torch.empty(n, dtype=torch.float64, device=dev)
        sp = native.score_params(n, T, tmode)
        score_ms = timed(lambda: native.score_dbn_device(ctx, nm, sp, ib.data_ptr(), db.data_ptr(), ll.data_ptr()))
        kernel = ctx.last_kernel()
        read_ms = timed(lambda: (torch.sum(ib), torch.sum(db)))
        nbytes = ib.numel() + 4 * db.numel()
        mean = lambda v: sum(v) / len(v)   # noqa: E731
        out["cases"]["%s %s" % (name, mode)] = {
            "kernel": kernel, "bytes_read": nbytes, "score_ms": score_ms, "read_ms": read_ms,
            "score_GBps": round(nbytes / mean(score_ms) / 1e6, 1), "read_GBps": round(nbytes / mean(read_ms) / 1e6, 1),
            "ratio_score_to_read": round(mean(score_ms) / mean(read_ms), 3),
            "finite": int(torch.isfinite(ll).sum().item())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
