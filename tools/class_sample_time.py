"""UncorEncounterModel.sample(100 000, 240) on uncor_1200code_v2p1 with its phases (last_sample_timing).
--lazy: the lazy call as well (samples and controls built on the device), then the cost of touching every item of its sequences, and the
library call alone into pinned and into pageable arrays.  Run under `python -m cProfile -s tottime` for the split of the eager call."""
import argparse
import sys
import tempfile
import time

sys.path.insert(0, ".")
import em_model_manned_bayes_amd as E
from em_model_manned_bayes_amd import em_io, native

ap = argparse.ArgumentParser()
ap.add_argument("--lazy", action="store_true")
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--T", type=int, default=240)
a = ap.parse_args()
mdl = E.UncorEncounterModel(em_io.materialize_model("uncor_1200code_v2p1", tempfile.mkdtemp()))
mdl.sample(2048, a.T, seed=1)
modes = (False, True) if a.lazy else (False,)
if a.lazy:
    mdl.sample(2048, a.T, seed=1, lazy=True)
fmt = lambda d: {k: round(v, 3) if isinstance(v, float) else v for k, v in d.items()}
for lazy in modes:
    for rep in range(2):
        t0 = time.perf_counter(); out = mdl.sample(a.n, a.T, seed=2, lazy=lazy); dt = time.perf_counter() - t0
        print("lazy" if lazy else "eager", a.n, "%.3f s" % dt, fmt(mdl.last_sample_timing), flush=True)
        if lazy and rep == 1:
            t0 = time.perf_counter()
            k = sum(1 for _ in out[1]) + sum(1 for _ in out[2]) + sum(1 for _ in out[3])
            print("lazy: touching all %d items of the three sequences: %.3f s" % (k, time.perf_counter() - t0), flush=True)
        del out
if a.lazy:
    labs = mdl.labels_initial
    var = lambda s: labs.index('"%s"' % s) + 1
    ctrl = (var("\\dot h"), var("\\dot \\psi"), var("\\dot v"))
    for pinned in (True, False):
        for rep in range(2):
            t0 = time.perf_counter()
            r = native.sample_uncor_host(native.default_context(), mdl.native, a.n, a.T, 2, ctrl, pinned=pinned,
                                         idx_L=var("L"), idx_v=var("v"), idx_dh=var("\\dot h"))
            dt = time.perf_counter() - t0
            print("sample_uncor_host pinned=%s %.3f s" % (pinned, dt), fmt(r["host_stats"]), flush=True)
            del r
