"""tools/count_time.py [--n N] [--T T] [--warmup W] [--launches K] [--naive | --naive-lib PATH] -- k_count_dbn on a device-resident trace,
on one GPU: 10 M trajectories x 240 s, three cases: uncor_1200code_v2p1 under REFERENCE_AUTO (the frozen form), the same trace under PER_STEP, and glider_v1
(dependent branch: per step).  Each case samples its trace once (emgpu_sample_dbn_device; the bins are kept), then times, between two events
on the ctx stream and in the same process: the count launch, k_score_dbn on the same trace (it reads the same bytes and does the same index
arithmetic: the floor for a kernel that only reads) and a plain read of the same bytes (torch.sum over the two buffers).  The counts of the
last launch are checked for their total (every observation once per launch).
--naive: also build the kernel with -DEMGPU_COUNT_NAIVE (one global add per observation: no run lengths, no LDS partials) into a library of
its own in a temporary directory (--naive-lib PATH: take one that build_naive(DIR) made earlier, where the tree's object files are), run
the same cases with it in a child process, and report the ratio: what the two mechanisms buy.
Prints one JSON line.  The numbers are a record (HISTORY.md section 21), not a gate."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("uncor_1200code_v2p1", "AUTO"), ("uncor_1200code_v2p1", "PER_STEP"), ("glider_v1", "AUTO")]


def build_naive(out_dir):
    """libemgpu.so with the naive count kernel, linked from the tree's objects and one recompiled unit; returns its path"""
    csrc = os.path.join(HERE, "em_model_manned_bayes_amd", "csrc")
    obj = os.path.join(out_dir, "emgpu_kernels_count_naive.o")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DEMGPU_COUNT_NAIVE", "--offload-arch=gfx950", "-c",
                           os.path.join(csrc, "emgpu_kernels_count.hip"), "-o", obj])
    objs = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".o") and f != "emgpu_kernels_count.o")
    if not objs:
        raise SystemExit("--naive links the objects of a built tree: run make -C em_model_manned_bayes_amd/csrc first")
    lib = os.path.join(out_dir, "libemgpu_naive.so")
    subprocess.check_call([hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", lib] + objs + [obj])
    return lib


def measure(args):
    sys.path.insert(0, HERE)
    from em_model_manned_bayes_amd import _lib as L
    if args.lib:
        L.LIB_PATH = args.lib
    import torch
    from em_model_manned_bayes_amd import em_io, native
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = native.Context(0, stream=stream.cuda_stream)
    n, T, G4 = args.n, args.T, (args.T + 3) // 4
    out = {"lib": L.lib().emgpu_version().decode(), "device": torch.cuda.get_device_name(0), "n": n, "T": T, "cases": {}}

    def timed(fn):
        ms = []
        for _ in range(args.warmup + args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            ctx.sync()
            ms.append(round(e0.elapsed_time(e1), 4))
        return ms[args.warmup:]

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
        ci = torch.zeros(int(nm.count_layout(0)[-1]), dtype=torch.int64, device=dev)
        ct = torch.zeros(int(nm.count_layout(1)[-1]), dtype=torch.int64, device=dev)
        ll = torch.empty(n, dtype=torch.float64, device=dev)
        sp = native.score_params(n, T, tmode)
        count_ms = timed(lambda: native.count_dbn_device(ctx, nm, sp, ib.data_ptr(), db.data_ptr(), ci.data_ptr(), ct.data_ptr()))
        kernel = ctx.last_kernel()
        launches = args.warmup + args.launches
        complete = int(ci.sum().item()) == launches * n * nm.n_initial and int(ct.sum().item()) == launches * n * (T - 1) * nm.n_dyn
        score_ms = timed(lambda: native.score_dbn_device(ctx, nm, sp, ib.data_ptr(), db.data_ptr(), ll.data_ptr()))
        read_ms = timed(lambda: (torch.sum(ib), torch.sum(db)))
        nbytes = ib.numel() + 4 * db.numel()
        mean = lambda v: sum(v) / len(v)   # noqa: E731
        out["cases"]["%s %s" % (name, mode)] = {
            "kernel": kernel, "bytes_read": nbytes, "count_ms": count_ms, "score_ms": score_ms, "read_ms": read_ms,
            "count_GBps": round(nbytes / mean(count_ms) / 1e6, 1), "ratio_count_to_score": round(mean(count_ms) / mean(score_ms), 3),
            "ratio_count_to_read": round(mean(count_ms) / mean(read_ms), 3), "every_observation_counted": bool(complete),
            "largest_cell": int(max(ci.max().item(), ct.max().item())) // launches}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--T", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--naive", action="store_true")
    ap.add_argument("--naive-lib", default=None, help="a library build_naive() made earlier (a box without the tree's object files)")
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)   # the child of --naive: measure with this library
    args = ap.parse_args()
    out = measure(args)
    if args.naive or args.naive_lib:
        with tempfile.TemporaryDirectory() as d:
            lib = args.naive_lib or build_naive(d)
            # a fresh process: this one has the tree's library loaded (the naive launches take about a second each: one timed launch)
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--T", str(args.T), "--warmup", "1",
                                    "--launches", "1", "--lib", lib], stdout=subprocess.PIPE, check=True, timeout=900)
        naive = json.loads(child.stdout.decode().strip().splitlines()[-1])
        mean = lambda v: sum(v) / len(v)   # noqa: E731
        for case, r in out["cases"].items():
            r["naive_count_ms"] = naive["cases"][case]["count_ms"]
            r["naive_every_observation_counted"] = naive["cases"][case]["every_observation_counted"]
            r["ratio_naive_to_count"] = round(mean(r["naive_count_ms"]) / mean(r["count_ms"]), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
