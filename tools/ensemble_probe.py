#!/usr/bin/env python3
"""What the ensemble calls cost (sfl_distance, sfl_batch_distance, sfl_batch_envelope): the numbers of profiles/ensemble.txt.

  contexts   per size, warmed, in one process, the calls alternating, each between two device events on the context's stream
             (sfl_timer_start / sfl_timer_stop): the three distance passes alone and together, and beside them the passes
             of sfl_flow_stats over the same fields, which read half the bytes (one operand instead of two).  The events of
             the synchronous calls enclose their record's memset and its copy as well as the kernels.  Median, minimum and
             maximum over --reps; bytes/s from the compulsory bytes; share of the 8 TB/s peak.
  batches    B members (61 x 81 x 1024; 128 x 128 x 256 large), the same calls plus sfl_batch_envelope followed by
             sfl_batch_synchronize, against sfl_batch_flow_stats' dye pass (the envelope's bytes, half a distance pass's),
             host clock around synchronous calls (a batch has no timer; the figure includes the launch and the wait, a few
             microseconds the kernels' own time does not have), and the route the calls replace: sfl_batch_download of the
             fields and numpy on them.

usage: python3 tools/ensemble_probe.py [--size N ...] [--reps R] [--skip-numpy]"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfl = importlib.import_module("esp32-fluid-simulation_amd")

PEAK = 8.0e12   # bytes/s, HBM3E of an MI355X
FV, FC, FP = sfl.capi.FIELD_VELOCITY, sfl.capi.FIELD_COLOR, sfl.capi.FIELD_PRESSURE


def line(name, us, nbytes):
    med = statistics.median(us)
    text = f"  {name:<34} median {med:9.1f} us   min {min(us):9.1f}   max {max(us):9.1f}"
    if nbytes:
        rate = nbytes / (med * 1e-6)
        text += f"   {nbytes / 1e6:8.1f} MB: {rate / 1e12:5.2f} TB/s = {100 * rate / PEAK:4.1f} % of peak"
    return text


def rounds(calls, time_one, a):
    for _ in range(a.warmup):
        for c, _ in calls.values():
            time_one(c)
    us = {n: [] for n in calls}
    for _ in range(a.reps):          # alternating: every round runs each call once
        for n, (c, _) in calls.items():
            us[n].append(time_one(c))
    for n, (_, nbytes) in calls.items():
        print(line(n, us[n], nbytes))
    sys.stdout.flush()
    return {n: statistics.median(u) for n, u in us.items()}


def contexts(a):
    for size in a.size:
        rng = np.random.default_rng(size)
        cells = size * size
        with sfl.Solver(size, size) as s, sfl.Solver(size, size) as t:
            for x in (s, t):
                x.upload(FV, rng.standard_normal((size, size, 2), dtype=np.float32))
                x.upload(FC, rng.integers(0, 2 ** 32, (size, size, 3), dtype=np.uint32))
                x.upload(FP, rng.standard_normal((size, size), dtype=np.float32))

            def event_us(call):
                s.timer_start()
                call()
                return s.timer_stop() * 1e3

            calls = {"distance velocity": (lambda: s.distance(t, dye=False, pressure=False), 16 * cells),
                     "flow_stats velocity": (lambda: s.flow_stats(1.0, dye=False), 8 * cells),
                     "distance dye": (lambda: s.distance(t, velocity=False, pressure=False), 24 * cells),
                     "flow_stats dye": (lambda: s.flow_stats(1.0, velocity=False), 12 * cells),
                     "distance pressure": (lambda: s.distance(t, velocity=False, dye=False), 8 * cells),
                     "distance all three": (lambda: s.distance(t), 40 * cells)}
            print(f"contexts {size} x {size}, {a.reps} rounds, device events:")
            rounds(calls, event_us, a)


def numpy_route(b, ref_member):
    """What the calls replace: every field of every member over PCIe, then numpy."""
    t0 = time.perf_counter()
    v, c, p = b.download(FV), b.download(FC), b.download(FP)
    t1 = time.perf_counter()
    dv = np.abs(v - v[ref_member]).reshape(len(v), -1, 2).max(axis=1)
    dp = np.abs(p - p[ref_member]).reshape(len(p), -1).max(axis=1)
    dc = np.abs(c.astype(np.int64) - c[ref_member].astype(np.int64)).reshape(len(c), -1, 3)
    figures = (dv, dp, dc.max(axis=1), dc.sum(axis=1), (c != c[ref_member]).any(axis=-1).reshape(len(c), -1).sum(axis=1))
    t2 = time.perf_counter()
    lo, hi = c.min(axis=0), c.max(axis=0)
    mean = c.astype(np.uint64).sum(axis=0) // np.uint64(len(c))
    t3 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, (t3 - t2) * 1e6, figures, (mean, lo, hi)


def batch(a, dim_x, dim_y, members, large):
    cells = dim_x * dim_y * members
    with sfl.BatchSolver(dim_x, dim_y, members, large=large) as b:
        b.setup_sketch_fields()
        b.queue_forces(list(range(members)), [(20, 40)] * members, [(-12.0, 30.0)] * members)
        b.step_n_each(2, 0.05, 1.0, [5 + m % 40 for m in range(members)], 1.9)
        b.synchronize()

        def host_us(call):
            t = time.perf_counter()
            call()
            b.synchronize()
            return (time.perf_counter() - t) * 1e6

        calls = {"distance velocity (ref member 0)": (lambda: b.distance(ref_member=0, dye=False, pressure=False), 8 * cells),
                 "flow_stats velocity": (lambda: b.flow_stats(1.0, dye=False), 8 * cells),
                 "distance dye (ref member 0)": (lambda: b.distance(ref_member=0, velocity=False, pressure=False), 12 * cells),
                 "distance dye (pairwise)": (lambda: b.distance(velocity=False, pressure=False), 24 * cells),
                 "flow_stats dye": (lambda: b.flow_stats(1.0, velocity=False), 12 * cells),
                 "envelope + synchronize": (lambda: b.envelope(), 12 * cells),
                 "distance pressure (ref member 0)": (lambda: b.distance(ref_member=0, velocity=False, dye=False), 4 * cells),
                 "distance all three (ref member 0)": (lambda: b.distance(ref_member=0), 20 * cells),
                 "synchronize alone": (lambda: None, 0)}
        print(f"batch of {members} x ({dim_x} x {dim_y}){' large' if large else ''}, {a.reps} rounds, host clock around synchronous calls")
        print("  (a fixed reference member is read from the caches after its first use: its bytes are not counted)")
        rounds(calls, host_us, a)
        if not a.skip_numpy:
            rows = [numpy_route(b, 0)[:3] for _ in range(3)]
            for k, name in enumerate(("download of v, dye, p", "numpy: the distance figures", "numpy: min, max, mean of the dye")):
                print(line(name, [r[k] for r in rows], 0))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs="+", default=[8192, 2048])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-numpy", action="store_true")
    a = ap.parse_args()
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    contexts(a)
    batch(a, 61, 81, 1024, False)
    batch(a, 128, 128, 256, True)
