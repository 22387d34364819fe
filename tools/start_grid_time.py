"""tools/start_grid_time.py [--parent DIR] [--models A,B,..] [--n N] [--T T] -- a start grid in one launch, device-resident outputs, on one GPU:
1 M trajectories x 240 s of uncor_1200code_v2p1 and uncor_1200only_fwse_v1p2 under a 16-row G x A grid (row i % 16 for trajectory i), the dense
outputs alone and the event list alone, 3 warm-up + 10 timed launches each, beside the same two calls without a grid (the ceiling:
k_uncor_fast_idx / k_uncor_fast_evu).

--models: the models to time instead (comma-separated).  The two variables the 16-row grid spans come from GRID_VARS (bins 1-4 of each; any other
model: its variables 1 and 2, which must then be a closed set).  For the models k_uncor_fast does not take -- cor_v1, uncor_1200code_v1, glider_v1 -- the grid
calls run on the +start instances of k_dbn_step2 and the call without a grid on the model's family instance ([cor], [chain,w884], ...).

--parent DIR: a checkout of another commit with its library built (tools/ab_checkout.sh <commit> parent -> tools/ab/parent) is timed first, in a
process of its own with its own Python package, on the same GPU in the same run: before the +start instances its calls ran on k_dbn_generic, the
baseline.  The run fails unless every timed launch of this tree's grid calls is faster than the parent's fastest launch of the same call.

A launch is timed between two events on the ctx stream: a grid call includes the upload of its 96-byte preset block."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ["uncor_1200code_v2p1", "uncor_1200only_fwse_v1p2"]
# the two variables of the 4 x 4 grid, by label (bins 1-4 of each; a preset variable's parents must be preset: both pairs are closed)
GRID_VARS = {"uncor_1200code_v2p1": ("G", "A"), "uncor_1200only_fwse_v1p2": ("G", "A"), "cor_v1": ("A", "L"), "uncor_1200code_v1": ("A", "L"),
             "glider_v1": ("L", "v")}


def child(pkg_root, n, T, warmup, launches, models):
    sys.path.insert(0, pkg_root)
    import numpy as np
    import torch
    from em_model_manned_bayes_amd import em_io, native, _lib as L
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = native.Context(0, stream=stream.cuda_stream)
    out = {"lib": L.lib().emgpu_version().decode(), "device": torch.cuda.get_device_name(0), "n": n, "T": T, "calls": {}}
    rows = np.array([[g, a] for g in (1, 2, 3, 4) for a in (1, 2, 3, 4)], dtype=np.int32)
    for name in models:
        nm = native.NativeModel.load_txt(em_io.materialize_model(name, tempfile.mkdtemp()))
        labs = nm.get_labels(L.F_LABELS_INITIAL)
        idx = {k: (labs.index('"%s"' % v) + 1 if '"%s"' % v in labs else 0) for k, v in (("idx_L", "L"), ("idx_v", "v"), ("idx_dh", "\\dot h"))}
        ni, nd, G4, cap = nm.n_initial, nm.n_dyn, (T + 3) // 4, 512
        grid = np.zeros((n, ni), dtype=np.int32)
        grid[:, [labs.index('"%s"' % v) for v in GRID_VARS[name]] if name in GRID_VARS else [0, 1]] = rows[np.arange(n) % 16]
        d_grid = torch.from_numpy(grid).to(dev)
        ib = torch.empty((ni, n), dtype=torch.uint8, device=dev)
        iv = torch.empty((ni, n), dtype=torch.float32, device=dev)
        for form in ("dense", "list"):
            if form == "dense":
                bufs = [torch.empty((G4, nd, n), dtype=torch.int32, device=dev), torch.empty((G4, nd, n, 4), dtype=torch.float32, device=dev)]
                ptrs = dict(dyn_bin=bufs[0].data_ptr(), dyn_val=bufs[1].data_ptr())
            else:
                bufs = [torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, cap, 2), dtype=torch.float32, device=dev)]
                ptrs = dict(ev_count=bufs[0].data_ptr(), events=bufs[1].data_ptr())
            for what, start in (("grid", d_grid.data_ptr()), ("unpreset", None)):
                p, _keep = native.make_params(n, T, 5, event_cap=cap if form == "list" else 0, start=start, **idx)
                ms = []
                for k in range(warmup + launches):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    native.sample_dbn_device(ctx, nm, p, init_bin=ib.data_ptr(), init_val=iv.data_ptr(), **ptrs)
                    e1.record(stream)
                    ctx.sync()
                    ms.append(round(e0.elapsed_time(e1), 4))
                out["calls"]["%s %s %s" % (name, form, what)] = {"kernel": ctx.last_kernel(), "ms": ms[warmup:], "warmup_ms": ms[:warmup]}
            del bufs
            ctx.trim()
            torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))


def run_child(pkg_root, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", pkg_root, "--n", str(args.n), "--T", str(args.T), "--warmup", str(args.warmup),
           "--launches", str(args.launches), "--models", args.models]
    txt = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--T", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--models", default=",".join(MODELS))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.n, args.T, args.warmup, args.launches, args.models.split(","))
    base = run_child(os.path.abspath(args.parent), args) if args.parent else None
    tree = run_child(HERE, args)
    print(json.dumps({"parent": base, "tree": tree}))
    mean = lambda v: sum(v) / len(v)
    ok = True
    for key, c in tree["calls"].items():
        if not key.endswith(" grid"):
            continue
        ceiling = tree["calls"][key[:-5] + " unpreset"]
        line = "%-44s %-34s %s ms  mean %.3f  x%.3f of %s (%.3f ms)" % (key, c["kernel"], c["ms"], mean(c["ms"]), mean(c["ms"]) / mean(ceiling["ms"]),
                                                                        ceiling["kernel"], mean(ceiling["ms"]))
        if base:
            b = base["calls"][key]
            faster = max(c["ms"]) < min(b["ms"])
            ok = ok and faster
            line += "  | parent %s %s ms  mean %.3f: %.2f x faster%s" % (b["kernel"], b["ms"], mean(b["ms"]), mean(b["ms"]) / mean(c["ms"]),
                                                                       "" if faster else "  NOT faster in every launch")
        print(line)
    if not ok:
        sys.exit("a timed launch of a grid call was not faster than the parent's fastest launch of the same call")


if __name__ == "__main__":
    main()
