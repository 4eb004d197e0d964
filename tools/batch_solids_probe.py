#!/usr/bin/env python3
"""What solid cells cost a batch: the numbers of profiles/batch_solids.txt.

In one process, warmed, the four configurations of the same step_n(n) alternating, host clock around the call and the
synchronise that ends it -- 61 x 81 x 1024 members at 20 iterations:

  (a) no solids          the kernel of batch_grid.hip, which a batch without solids launches as ever: the baseline
  (b) an empty mask set  the kernel of batch_solids.hip with no solid cell: the same arithmetic, one byte per cell more
  (c) one shared disc    radius 8 in the middle of every member, one mask for all of them (L2-resident)
  (d) per-member 30 %    a seeded mask of each member's own, 30 % solid

The run-to-run spread of (a) is what the probe itself sees: (max - min) and the median absolute deviation over --reps.
(b) is expected inside it; a gap of more than three spreads is a finding.  Then, alone between synchronises, flow_stats
of the velocity on the plain batch (the streaming pass of flow_stats.hip) and on the batch with the disc (the pass of
batch_solids.hip), the copy of the records included.

usage: python3 tools/batch_solids_probe.py [--reps R] [--steps N] [--out profiles/batch_solids_timings.txt]"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfl = importlib.import_module("esp32-fluid-simulation_amd")

OUT = []
DIM_X, DIM_Y, MEMBERS, ITERS = 61, 81, 1024, 20


def say(text=""):
    print(text)
    sys.stdout.flush()
    OUT.append(text)


def timed(call, sync):
    sync()
    t = time.perf_counter()
    call()
    sync()
    return (time.perf_counter() - t) * 1e6


def masks():
    j, i = np.mgrid[0:DIM_Y, 0:DIM_X]
    disc = (i - DIM_X // 2) ** 2 + (j - DIM_Y // 2) ** 2 <= 64
    each = np.random.default_rng(3).random((MEMBERS, DIM_Y, DIM_X)) < 0.3
    return {"(a) no solids": None, "(b) empty mask set": np.zeros((DIM_Y, DIM_X), bool), "(c) one shared disc, r = 8": disc,
            "(d) per-member 30 % masks": each}


def main(a):
    n = a.steps
    batches = {}
    for name, mask in masks().items():
        b = sfl.BatchSolver(DIM_X, DIM_Y, MEMBERS)
        b.setup_sketch_fields()
        if mask is not None:
            b.set_solids(mask)
        b.queue_forces(list(range(MEMBERS)), [(10, 40)] * MEMBERS, [(-12.0, 30.0)] * MEMBERS)
        b.step_n(2, 0.05, 1.0, ITERS, 1.9)
        batches[name] = b
    say(f"batch of {MEMBERS} x ({DIM_X} x {DIM_Y}), step_n({n}) of {ITERS} iterations, {a.warmup} warm-up and {a.reps} timed rounds, the four "
        f"configurations alternating, host clock around call + synchronize:")
    us = {name: [] for name in batches}
    for r in range(a.warmup + a.reps):
        for name, b in batches.items():
            t = timed(lambda: b.step_n(n, 0.05, 1.0, ITERS, 1.9), b.synchronize)
            if r >= a.warmup:
                us[name].append(t)
    med = {name: statistics.median(u) for name, u in us.items()}
    base = med["(a) no solids"]
    for name, u in us.items():
        mad = statistics.median(abs(x - med[name]) for x in u)
        say(f"  {name:<28} median {med[name] / n:8.2f} us per step   min {min(u) / n:8.2f}   max {max(u) / n:8.2f}   MAD {mad / n:6.2f}   "
            f"{MEMBERS * n / med[name]:7.3f} M member-steps/s   vs (a) {100 * (med[name] - base) / base:+6.2f} %")
    ua = us["(a) no solids"]
    spread = (max(ua) - min(ua)) / n
    say(f"  run-to-run spread of (a): max - min = {spread:.2f} us per step; (b) - (a) = {(med['(b) empty mask set'] - base) / n:+.2f} us per step "
        f"= {(med['(b) empty mask set'] - base) / n / spread if spread else float('nan'):+.2f} spreads")
    say()
    say(f"flow_stats(velocity) of all {MEMBERS} members, call + copy of the records, {a.reps} rounds alternating:")
    plain, disc = batches["(a) no solids"], batches["(c) one shared disc, r = 8"]
    fs = {"plain (flow_stats.hip)": [], "with solids (batch_solids.hip)": []}
    for r in range(a.warmup + a.reps):
        for name, b in (("plain (flow_stats.hip)", plain), ("with solids (batch_solids.hip)", disc)):
            t = timed(lambda: b.flow_stats(1.0, dye=False), b.synchronize)
            if r >= a.warmup:
                fs[name].append(t)
    for name, u in fs.items():
        say(f"  {name:<32} median {statistics.median(u):8.1f} us   min {min(u):8.1f}   max {max(u):8.1f}")
    for b in batches.values():
        b.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    say("# tools/batch_solids_probe.py " + " ".join(sys.argv[1:]))
    say(f"# device: {sfl.device_info(0)[0]}")
    main(a)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")
