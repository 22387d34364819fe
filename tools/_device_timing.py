"""What the *_time.py tools share: a launch timed between two events on a stream, seeded straight tracks made on the device, and for the
tools on paired tracks (miss_time.py, well_clear_time.py, avoid_time.py) the three pairings, their buffers, the launches of the kernels
more than one of them times, the torch.sum baselines and the report."""
import argparse
import statistics

import torch

med = statistics.median


def timed(stream, fn, warmup, launches, sync=torch.cuda.synchronize):
    """The milliseconds of each of `launches` calls of fn() behind `warmup` more, each between two events on `stream` (a torch stream) and
    waited for with sync() -- a Context's sync where fn launches through one, so that its status word is looked at"""
    ms = []
    for _ in range(warmup + launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        sync()
        ms.append(round(e0.elapsed_time(e1), 4))
    return ms[warmup:]


def straight_tracks(n, P, dev, gen):
    """n straight tracks of P points as a PLANAR float64 tensor [P, 3, n] on dev: starts within 3000 ft of the origin, up to 200 ft/s
    horizontally and 20 ft/s vertically, drawn from the device generator gen"""
    xyz = torch.empty((P, 3, n), dtype=torch.float64, device=dev)
    start = (torch.rand((3, n), dtype=torch.float64, device=dev, generator=gen) - 0.5) * 6000.0
    vel = (torch.rand((3, n), dtype=torch.float64, device=dev, generator=gen) - 0.5) * 400.0
    vel[2] *= 0.1
    for p in range(P):
        xyz[p] = start + vel * float(p)
    return xyz


def pair_args(*flags):
    """The command line of a tool on paired tracks: --n, --points, --warmup, --launches and the tool's own boolean `flags`"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--points", type=int, default=241)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=7)
    for flag in flags:
        ap.add_argument(flag, action="store_true")
    return ap.parse_args()


class PairBench:
    """The protocol of the tools on paired tracks (HISTORY.md section 30), on GPU 0 and torch's current stream: two PLANAR sets of n
    seeded straight tracks of P points, a random pose per pair, and three pairings, each a function that calls a launch k(xa, n_a, idx_b=0):
      identity    pair i = column i of both sets;
      ownship     n_a = 1: the first track of set A against every column of set B;
      permuted    a random permutation as idx_b.
    Output buffers come by name from buf() and totals(), so that every launch of a tool writes the same ones; miss(), segments() and
    well_clear() are launches for the pairings; run() times a tool's kernel list and report() is the JSON record."""

    def __init__(self, args, native):
        import numpy as np
        self.native, self.np, self.n, self.P = native, np, args.n, args.points
        n, P = self.n, self.P
        self.dev = dev = torch.device("cuda", 0)
        self.stream = torch.cuda.current_stream(dev)
        self.timed = lambda fn: timed(self.stream, fn, args.warmup, args.launches)
        gen = torch.Generator(device=dev)
        gen.manual_seed(30)
        self.a, self.b = a, b = straight_tracks(n, P, dev, gen), straight_tracks(n, P, dev, gen)
        self.own = own = a[:, :, :1].contiguous()
        rs = np.random.RandomState(30)
        self.pose = torch.from_numpy(native.make_pose(rs.uniform(-180.0, 180.0, n), rs.uniform(-3000.0, 3000.0, n),
                                                      rs.uniform(-3000.0, 3000.0, n), rs.uniform(-300.0, 300.0, n))).to(dev)
        self.perm = perm = torch.randperm(n, device=dev, generator=gen)
        self.pairings = (("identity", lambda k: k(a, n)), ("ownship", lambda k: k(own, 1)), ("permuted", lambda k: k(a, n, perm.data_ptr())))
        self.wc_thresholds = ()          # well_clear()'s thresholds behind `points`: none are well_clear_params' defaults
        self._buf, self.ms, self.tot = {}, {}, {}
        torch.cuda.synchronize()

    def buf(self, name, dtype=torch.float64):
        """the address of the output buffer `name`, [n] of dtype, made at its first use"""
        if name not in self._buf:
            self._buf[name] = torch.empty(self.n, dtype=dtype, device=self.dev)
        return self._buf[name].data_ptr()

    def totals(self, k):
        """the int64 [k] tensor the launches with k totals add to"""
        if k not in self._buf:
            self._buf[k] = torch.zeros(k, dtype=torch.int64, device=self.dev)
        return self._buf[k]

    def launch(self, entry, params, xa, idx_b, with_pose, outputs, k):
        self.totals(k).zero_()
        getattr(self.native, entry)(params, xa.data_ptr(), self.b.data_ptr(), 0, idx_b, self.pose.data_ptr() if with_pose else 0, 0, *outputs,
                                    self.totals(k).data_ptr(), stream=self.stream.cuda_stream)

    def miss(self, xa, n_a, idx_b=0, with_pose=True):
        """k_miss_distance; its flags are well_clear()'s miss_flags"""
        self.launch("miss_distance_device", self.native.miss_params(self.n, n_a, self.n, self.P), xa, idx_b, with_pose,
                     (self.buf("hmd"), self.buf("vmd"), self.buf("t_cpa", torch.int32), self.buf("miss_flags", torch.uint8)), 8)

    def segments(self, xa, n_a, idx_b=0):
        """k_miss_segments[pose]"""
        self.launch("miss_segments_device", self.native.miss_params(self.n, n_a, self.n, self.P), xa, idx_b, True,
                     (self.buf("hmd"), self.buf("vmd"), self.buf("t_cpa_s"), self.buf("flags", torch.uint8)), 10)

    def well_clear(self, xa, n_a, idx_b=0):
        """k_well_clear[pose] with wc_thresholds, behind a miss() of the same pairing"""
        self.launch("well_clear_device", self.native.well_clear_params(self.n, n_a, self.n, self.P, *self.wc_thresholds), xa, idx_b, True,
                     (self.buf("miss_flags", torch.uint8), self.buf("t_first", torch.int32), self.buf("n_lost", torch.int32), self.buf("tau_min"),
                      self.buf("flags", torch.uint8)), 10)

    def run(self, name, fn, k):
        """times fn as ms[name] and keeps the k totals of its last launch as tot[name]"""
        self.ms[name] = self.timed(fn)
        self.tot[name] = [int(x) for x in self.totals(k).cpu().numpy().view(self.np.uint64)]

    def run_sums(self):
        """torch.sum over the bytes the pairings read: both sets, and set B alone for `ownship`"""
        self.ms["sum_both"] = self.timed(lambda: (torch.sum(self.a), torch.sum(self.b)))
        self.ms["sum_b"] = self.timed(lambda: torch.sum(self.b))

    def head(self):
        """the record's opening keys, and the bytes an identity or permuted launch reads and an ownship launch reads"""
        from em_model_manned_bayes_amd import _lib as L
        both, one = 2 * 24 * self.P * self.n, 24 * self.P * self.n + 24 * self.P
        return {"lib": L.lib().emgpu_version().decode(), "device": torch.cuda.get_device_name(0), "n_pairs": self.n, "points": self.P,
                "bytes_read_identity": both, "bytes_read_ownship": one}, both, one

    def report(self, no_rate=()):
        """the record of a tool whose ms keys are <kernel>_<pairing>: every launch, median / smallest / largest, GB/s (not for the kernels
        of no_rate, which read the bytes more than once) and the ratio to the torch.sum of the same bytes"""
        out, both, one = self.head()
        ms = self.ms
        read = {"identity": both, "ownship": one, "permuted": both}
        base = {"identity": "sum_both", "ownship": "sum_b", "permuted": "sum_both"}
        kernels = [k for k in ms if not k.startswith("sum_")]
        out.update({"ms": ms, "median_min_max_ms": {k: [round(med(v), 4), min(v), max(v)] for k, v in ms.items()},
                    "GBps": {k: round(read[k.rsplit("_", 1)[1]] / med(ms[k]) / 1e6, 1) for k in kernels if not k.startswith(tuple(no_rate))},
                    "ratio_to_sum": {k: round(med(ms[k]) / med(ms[base[k.rsplit("_", 1)[1]]]), 3) for k in kernels},
                    "sum_both_GBps": round(both / med(ms["sum_both"]) / 1e6, 1), "totals": self.tot})
        return out
