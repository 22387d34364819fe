"""tools/count_time.py [--n N] [--T T] [--warmup W] [--launches K] [--naive | --naive-lib PATH] [--weighted [--probe-values] [--lds CELLS |
--lds-lib PATH]] -- k_count_dbn on a device-resident trace, on one GPU: 10 M trajectories x 240 s, three cases: uncor_1200code_v2p1 under
REFERENCE_AUTO (the frozen form), the same trace under PER_STEP, and glider_v1 (dependent branch: per step; its tables live in the LDS
partials).  Each case samples its trace once (emgpu_sample_dbn_device; the bins are kept), then times, between two events on the ctx stream
and in the same process: the count launch, k_score_dbn on the same trace (it reads the same bytes and does the same index arithmetic: the
floor for a kernel that only reads) and a plain read of the same bytes (torch.sum over the two buffers).  The counts of the last launch are
checked for their total (every observation once per launch).
--weighted: time the weighted instances first, with all weights 1 and with random 24-bit weights (their totals checked too: every
observation once per launch, times its weight), and report their ratios to the unweighted count.  --probe-values: also all weights
2^24 - 1, and all weights 1 a second time behind them (does a difference follow the values or the order of the runs?).
--naive: also build the kernel with -DEMGPU_COUNT_NAIVE (one global add per observation: no run lengths, no LDS partials) into a library of
its own in a temporary directory, run the unweighted cases with it in a child process, and report the ratio: what the two mechanisms buy.
--lds CELLS (with --weighted): the same with -DEMGPU_WCOUNT_LDS_CELLS=CELLS (the other size of the u64 partials: 8192 cells are 64 KB and
two waves per SIMD, 4096 are 32 KB and five) and the weighted cases.  --naive-lib / --lds-lib PATH: take a library that build_variant made
earlier, where the tree's object files are.
Prints one JSON line, with the keys of every earlier record ("kernel" is the unweighted instance, "weighted_kernel" the weighted one).  The
numbers are a record (HISTORY.md sections 21 and 25), not a gate."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("uncor_1200code_v2p1", "AUTO"), ("uncor_1200code_v2p1", "PER_STEP"), ("glider_v1", "AUTO")]
NAIVE = (["-DEMGPU_COUNT_NAIVE"], ["emgpu_kernels_count.hip"])
LDS = (["-DEMGPU_WCOUNT_LDS_CELLS=%d"], ["emgpu_kernels_count.hip", "emgpu_count.cpp"])   # the kernel and the host code that assigns its partials


def build_variant(out_dir, defines, units):
    """libemgpu.so with `units` recompiled under `defines`, linked with the tree's other objects; returns its path"""
    csrc = os.path.join(HERE, "em_model_manned_bayes_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    mine = []
    for unit in units:
        mine.append(os.path.join(out_dir, os.path.splitext(unit)[0] + "_variant.o"))
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"] + defines +
                              ["--offload-arch=gfx950", "-c", os.path.join(csrc, unit), "-o", mine[-1]])
    skip = {os.path.splitext(u)[0] + ".o" for u in units}
    objs = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".o") and f not in skip)
    if not objs:
        raise SystemExit("a variant links the objects of a built tree: run make -C em_model_manned_bayes_amd/csrc first")
    lib = os.path.join(out_dir, "libemgpu_variant.so")
    subprocess.check_call([hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", lib] + objs + mine)
    return lib


def measure(args):
    sys.path.insert(0, HERE)
    from _device_timing import timed as timed_on
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
    mean = lambda v: sum(v) / len(v)   # noqa: E731

    timed = lambda fn: timed_on(stream, fn, args.warmup, args.launches, ctx.sync)          # noqa: E731

    weights = {}
    if args.weighted:
        gen = torch.Generator(device=dev)
        gen.manual_seed(25)
        weights = {"ones": torch.ones(n, dtype=torch.int32, device=dev),
                   "random24": torch.randint(0, 2 ** 24, (n,), dtype=torch.int32, device=dev, generator=gen)}
        if args.probe_values:
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
        r = {"bytes_read": ib.numel() + 4 * db.numel()}

        def complete(ci, ct, per_launch):   # every observation once per launch, `per_launch` = the trajectories' weights summed
            return bool(int(ci.sum().item()) == launches * per_launch * nm.n_initial
                        and int(ct.sum().item()) == launches * per_launch * (T - 1) * nm.n_dyn)

        for kind, w in weights.items():
            ci, ct = (torch.zeros(s, dtype=torch.int64, device=dev) for s in sizes)
            r["weighted_%s_ms" % kind] = timed(lambda: native.count_dbn_weighted_device(ctx, nm, sp, ib.data_ptr(), db.data_ptr(), w.data_ptr(),
                                                                                         ci.data_ptr(), ct.data_ptr()))
            r["weighted_kernel"] = ctx.last_kernel()
            r["weighted_%s_complete" % kind] = complete(ci, ct, w_sum[kind])
        ci, ct = (torch.zeros(s, dtype=torch.int64, device=dev) for s in sizes)
        r["count_ms"] = timed(lambda: native.count_dbn_device(ctx, nm, sp, ib.data_ptr(), db.data_ptr(), ci.data_ptr(), ct.data_ptr()))
        r["kernel"] = r["count_kernel"] = ctx.last_kernel()
        r["every_observation_counted"] = complete(ci, ct, n)
        r["largest_cell"] = int(max(ci.max().item(), ct.max().item())) // launches
        r["score_ms"] = timed(lambda: native.score_dbn_device(ctx, nm, sp, ib.data_ptr(), db.data_ptr(), ll.data_ptr()))
        r["read_ms"] = timed(lambda: (torch.sum(ib), torch.sum(db)))
        r["count_GBps"] = round(r["bytes_read"] / mean(r["count_ms"]) / 1e6, 1)
        r["ratio_count_to_score"] = round(mean(r["count_ms"]) / mean(r["score_ms"]), 3)
        r["ratio_count_to_read"] = round(mean(r["count_ms"]) / mean(r["read_ms"]), 3)
        for kind in weights:
            r["ratio_weighted_%s_to_count" % kind] = round(mean(r["weighted_%s_ms" % kind]) / mean(r["count_ms"]), 3)
        out["cases"]["%s %s" % (name, mode)] = r
    return out


def measure_variant(args, lib, variant, flags):
    """the cases of a child process that measures with `lib` (built here from `variant` when None): this one has the tree's library loaded"""
    with tempfile.TemporaryDirectory() as d:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--T", str(args.T), "--lib",
                                lib or build_variant(d, *variant)] + flags, stdout=subprocess.PIPE, check=True, timeout=900)
    return json.loads(child.stdout.decode().strip().splitlines()[-1])["cases"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--T", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--weighted", action="store_true", help="also time the weighted instances: all weights 1, random 24-bit weights")
    ap.add_argument("--probe-values", action="store_true", help="--weighted: also all weights 2^24 - 1, and all weights 1 a second time")
    ap.add_argument("--naive", action="store_true")
    ap.add_argument("--naive-lib", default=None, help="a library build_variant(DIR, *NAIVE) made earlier (a box without the tree's object files)")
    ap.add_argument("--lds", type=int, default=0, help="--weighted: also time a build with this many u64 LDS partial cells")
    ap.add_argument("--lds-lib", default=None, help="a library build_variant(DIR, *LDS) made earlier (a box without the tree's object files)")
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)   # the child of a variant: measure with this library
    args = ap.parse_args()
    if (args.probe_values or args.lds or args.lds_lib) and not args.weighted:
        ap.error("--probe-values and --lds time the weighted instances: add --weighted")
    out = measure(args)
    mean = lambda v: sum(v) / len(v)   # noqa: E731
    if args.naive or args.naive_lib:   # the naive launches take about a second each: one timed launch
        naive = measure_variant(args, args.naive_lib, NAIVE, ["--warmup", "1", "--launches", "1"])
        for case, r in out["cases"].items():
            r["naive_count_ms"] = naive[case]["count_ms"]
            r["naive_every_observation_counted"] = naive[case]["every_observation_counted"]
            r["ratio_naive_to_count"] = round(mean(r["naive_count_ms"]) / mean(r["count_ms"]), 2)
    if args.lds or args.lds_lib:
        other = measure_variant(args, args.lds_lib, ([LDS[0][0] % args.lds], LDS[1]),
                                ["--warmup", str(args.warmup), "--launches", str(args.launches), "--weighted"])
        for case, r in out["cases"].items():
            for kind in ("ones", "random24"):
                key = "weighted_%s_ms" % kind
                r["other_lds_" + key] = other[case][key]
                r["other_lds_weighted_%s_complete" % kind] = other[case]["weighted_%s_complete" % kind]
                r["ratio_other_lds_to_this_%s" % kind] = round(mean(other[case][key]) / mean(r[key]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
