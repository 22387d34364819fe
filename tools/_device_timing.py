"""What the *_time.py tools share: a launch timed between two events on a stream, and seeded straight tracks made on the device."""
import torch


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
