#!/usr/bin/env python3
"""What the flow statistics cost (sfl_flow_stats, sfl_batch_flow_stats): the numbers of profiles/flow_stats.txt.

  contexts   per size, warmed, in one process, the calls alternating, each between two device events on the context's stream
             (sfl_timer_start / sfl_timer_stop): the velocity pass, the dye pass, both, and beside them sfl_calculate_divergence
             (the same 8 B per cell read, 4 more written: the yardstick of the velocity pass) and sfl_residual.  The events of
             the synchronous calls enclose their record's memset and its 40-byte copy as well as the kernels.  Median, minimum
             and maximum over --reps; bytes/s from the compulsory bytes (8 and 12 B per cell); share of the 8 TB/s peak.
  batch      B members of 61 x 81: flow_stats of all members against one sfl_batch_step_n step, host clock around
             synchronous calls.

usage: python3 tools/flow_stats_probe.py [--size N ...] [--reps R] [--batch B]"""
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


def event_us(s, call):
    s.timer_start()
    call()
    return s.timer_stop() * 1e3


def line(name, us, bytes_per_cell, cells):
    med = statistics.median(us)
    text = f"  {name:<26} median {med:8.1f} us   min {min(us):8.1f}   max {max(us):8.1f}"
    if bytes_per_cell:
        rate = bytes_per_cell * cells / (med * 1e-6)
        text += f"   {bytes_per_cell:2d} B/cell: {rate / 1e12:5.2f} TB/s = {100 * rate / PEAK:4.1f} % of peak"
    return text


def contexts(a):
    for size in a.size:
        rng = np.random.default_rng(size)
        with sfl.Solver(size, size) as s:
            s.upload(sfl.capi.FIELD_VELOCITY, rng.standard_normal((size, size, 2), dtype=np.float32))
            s.upload(sfl.capi.FIELD_COLOR, rng.integers(0, 2 ** 32, (size, size, 3), dtype=np.uint32))
            s.upload(sfl.capi.FIELD_PRESSURE, rng.standard_normal((size, size), dtype=np.float32))
            calls = {"flow_stats velocity": (lambda: s.flow_stats(1.0, dye=False), 8),
                     "calculate_divergence": (lambda: s.calculate_divergence(1.0), 8),
                     "flow_stats dye": (lambda: s.flow_stats(1.0, velocity=False), 12),
                     "residual": (lambda: s.residual(1.0), 8),
                     "flow_stats both": (lambda: s.flow_stats(1.0), 20)}
            for _ in range(a.warmup):
                for c, _ in calls.values():
                    event_us(s, c)
            us = {n: [] for n in calls}
            for _ in range(a.reps):          # alternating: every round runs each call once
                for n, (c, _) in calls.items():
                    us[n].append(event_us(s, c))
            print(f"{size} x {size}, {a.reps} rounds, device events:")
            for n, (_, b) in calls.items():
                print(line(n, us[n], b, size * size))
            ratio = statistics.median(us["flow_stats velocity"]) / statistics.median(us["calculate_divergence"])
            print(f"  velocity pass / calculate_divergence = {ratio:.2f}")
            sys.stdout.flush()


def batch(a):
    dim_x, dim_y, members = 61, 81, a.batch
    with sfl.BatchSolver(dim_x, dim_y, members) as b:
        b.setup_sketch_fields()
        b.queue_forces(list(range(members)), [(20, 40)] * members, [(-12.0, 30.0)] * members)
        b.step_n(2, 0.05, 1.0, 20, 1.9)
        b.synchronize()

        def host_us(call):
            t = time.perf_counter()
            call()
            b.synchronize()
            return (time.perf_counter() - t) * 1e6

        calls = {"flow_stats velocity": lambda: b.flow_stats(1.0, dye=False), "flow_stats dye": lambda: b.flow_stats(1.0, velocity=False),
                 "flow_stats both": lambda: b.flow_stats(1.0), "step_n(1), 20 iterations": lambda: b.step_n(1, 0.05, 1.0, 20, 1.9)}
        for _ in range(a.warmup):
            for c in calls.values():
                host_us(c)
        us = {n: [] for n in calls}
        for _ in range(a.reps):
            for n, c in calls.items():
                us[n].append(host_us(c))
        print(f"batch of {members} x ({dim_x} x {dim_y}), {a.reps} rounds, host clock around synchronous calls:")
        for n in calls:
            print(line(n, us[n], 0, 0))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs="+", default=[8192, 2048])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    a = ap.parse_args()
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    contexts(a)
    batch(a)
