"""tools/wcount_time.py [--n N] [--T T] [--warmup W] [--launches K] [--lds CELLS | --lds-lib PATH] [--probe-values] -- the weighted k_count_dbn on a
device-resident trace, on one GPU: 10 M trajectories x 240 s, three cases: uncor_1200code_v2p1 under REFERENCE_AUTO (the frozen form), the
same trace under PER_STEP, and glider_v1 (dependent branch: per step; its tables live in the LDS partials).  Each case samples its trace once
(emgpu_sample_dbn_device; the bins are kept), then times, between two events on the ctx stream and in the same process: the weighted count
with all weights 1 and with random 24-bit weights, and as yardsticks the unchanged k_count_dbn and k_score_dbn on the same trace.  The
counts of the last launch are checked for their total (every observation once per launch, times its weight).
--lds CELLS: also build the weighted kernel with -DEMGPU_WCOUNT_LDS_CELLS=CELLS (the other size of its u64 partials: 8192 cells are 64 KB and
two waves per SIMD, 4096 are 32 KB and five) into a library of its own in a temporary directory (--lds-lib PATH: take one that
build_lds(DIR, CELLS) made earlier, where the tree's object files are), run the same cases with it in a child process, and report the ratio.
--probe-values: also time all weights 2^24 - 1, and all weights 1 a second time behind them (does a difference follow the values or the
order of the runs?).
Prints one JSON line.  The numbers are a record (HISTORY.md section 25), not a gate."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("uncor_1200code_v2p1", "AUTO"), ("uncor_1200code_v2p1", "PER_STEP"), ("glider_v1", "AUTO")]
UNITS = ("emgpu_kernels_wcount.hip", "emgpu_count.cpp")      # the kernel and the host code that assigns its partials


def build_lds(out_dir, cells):
    """libemgpu.so with EMGPU_WCOUNT_LDS_CELLS = cells, linked from the tree's objects and the two recompiled units; returns its path"""
    csrc = os.path.join(HERE, "em_model_manned_bayes_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    mine = []
    for unit in UNITS:
        obj = os.path.join(out_dir, os.path.splitext(unit)[0] + "_lds.o")
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DEMGPU_WCOUNT_LDS_CELLS=%d" % cells,
                               "--offload-arch=gfx950", "-c", os.path.join(csrc, unit), "-o", obj])
        mine.append(obj)
    skip = {os.path.splitext(u)[0] + ".o" for u in UNITS}
    objs = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".o") and f not in skip)
    if not objs:
        raise SystemExit("--lds links the objects of a built tree: run make -C em_model_manned_bayes_amd/csrc first")
    lib = os.path.join(out_dir, "libemgpu_wcount_lds%d.so" % cells)
    subprocess.check_call([hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", lib] + objs + mine)
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
    launches = args.warmup + args.launches

    def timed(fn):
        ms = []
        for _ in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            ctx.sync()
            ms.append(round(e0.elapsed_time(e1), 4))
        return ms[args.warmup:]

    gen = torch.Generator(device=dev)
    gen.manual_seed(25)
    weights = {"ones": torch.ones(n, dtype=torch.int32, device=dev),
               "random24": torch.randint(0, 2 ** 24, (n,), dtype=torch.int32, device=dev, generator=gen)}
    if args.probe_values:   # does the time follow the values or the order of the runs?  one large constant, and the ones a second time
        weights["const24"] = torch.full((n,), 2 ** 24 - 1, dtype=torch.int32, device=dev)
        weights["ones_again"] = weights["ones"]
    w_sum = {k: int(v.sum(dtype=torch.int64).item()) for k, v in weights.items()}
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
        sizes = [int(nm.count_layout(k)[-1]) for k in (0, 1)]
        ll = torch.empty(n, dtype=torch.float64, device=dev)
        sp = native.score_params(n, T, tmode)
        mean = lambda v: sum(v) / len(v)   # noqa: E731
        r = {"bytes_read": ib.numel() + 4 * db.numel()}
        for kind, w in weights.items():
            ci, ct = (torch.zeros(s, dtype=torch.int64, device=dev) for s in sizes)
            r["weighted_%s_ms" % kind] = timed(lambda: native.count_dbn_weighted_device(ctx, nm, sp, ib.data_ptr(), db.data_ptr(), w.data_ptr(),
                                                                                         ci.data_ptr(), ct.data_ptr()))
            r["kernel"] = ctx.last_kernel()
            r["weighted_%s_complete" % kind] = bool(int(ci.sum().item()) == launches * w_sum[kind] * nm.n_initial
                                                    and int(ct.sum().item()) == launches * w_sum[kind] * (T - 1) * nm.n_dyn)
        ci, ct = (torch.zeros(s, dtype=torch.int64, device=dev) for s in sizes)
        r["count_ms"] = timed(lambda: native.count_dbn_device(ctx, nm, sp, ib.data_ptr(), db.data_ptr(), ci.data_ptr(), ct.data_ptr()))
        r["count_kernel"] = ctx.last_kernel()
        r["score_ms"] = timed(lambda: native.score_dbn_device(ctx, nm, sp, ib.data_ptr(), db.data_ptr(), ll.data_ptr()))
        for kind in weights:
            r["ratio_weighted_%s_to_count" % kind] = round(mean(r["weighted_%s_ms" % kind]) / mean(r["count_ms"]), 3)
        r["ratio_count_to_score"] = round(mean(r["count_ms"]) / mean(r["score_ms"]), 3)
        out["cases"]["%s %s" % (name, mode)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--T", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--lds", type=int, default=0, help="also time a build with this many u64 LDS partial cells")
    ap.add_argument("--lds-lib", default=None, help="a library build_lds() made earlier (a box without the tree's object files)")
    ap.add_argument("--probe-values", action="store_true", help="also time all weights 2^24 - 1, and all weights 1 a second time")
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)   # the child of --lds: measure with this library
    args = ap.parse_args()
    out = measure(args)
    if args.lds or args.lds_lib:
        with tempfile.TemporaryDirectory() as d:
            lib = args.lds_lib or build_lds(d, args.lds)
            # a fresh process: this one has the tree's library loaded
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--T", str(args.T), "--warmup", str(args.warmup),
                                    "--launches", str(args.launches), "--lib", lib], stdout=subprocess.PIPE, check=True, timeout=900)
        other = json.loads(child.stdout.decode().strip().splitlines()[-1])
        mean = lambda v: sum(v) / len(v)   # noqa: E731
        for case, r in out["cases"].items():
            for kind in ("ones", "random24"):
                key = "weighted_%s_ms" % kind
                r["other_lds_" + key] = other["cases"][case][key]
                r["other_lds_weighted_%s_complete" % kind] = other["cases"][case]["weighted_%s_complete" % kind]
                r["ratio_other_lds_to_this_%s" % kind] = round(mean(other["cases"][case][key]) / mean(r[key]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
