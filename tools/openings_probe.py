#!/usr/bin/env python3
"""What openings cost a batch, and that they cost nothing where none is set: the numbers of profiles/openings.txt.

Two modes, host clock around the call and the synchronise that ends it, warmed:

  --mode plain     nothing set: step_n(n) of a batch of 61 x 81 x 1024 members at 20 iterations, and step_n(4) of a 2048 x
                   2048 context at 40 iterations.  Uses no call that an older library lacks, so the same script runs against
                   the parent commit's library (python tools/with_lib.py <parent's libsfl_hip.so> tools/openings_probe.py
                   --mode plain); run the two alternately in one job and compare this library's median with the parent's
                   median and its run-to-run spread (max - min and MAD over --reps).
  --mode openings  in one process, alternating: (a) nothing set -- the kernel of batch_grid.hip; (b) an empty mask set -- the
                   kernel of batch_solids.hip, the baseline of the comparison; (c) a west-in / east-out map set and no mask --
                   the kernel of batch_openings.hip; (d) the map and a shared disc.  Then flow_stats of the velocity with
                   the empty mask and with the map.  Then the same four configurations of a 2048 x 2048 context at 40 iterations.

usage: python3 tools/openings_probe.py --mode plain|openings [--reps R] [--steps N] [--out FILE]"""
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
CTX, CTX_ITERS, CTX_STEPS = 2048, 40, 4


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


def report(name, u, n, base=None):
    med = statistics.median(u)
    mad = statistics.median(abs(x - med) for x in u)
    versus = "" if base is None else f"   vs (b) {100 * (med - base) / base:+6.2f} %"
    say(f"  {name:<34} median {med / n:9.2f} us per step   min {min(u) / n:9.2f}   max {max(u) / n:9.2f}   MAD {mad / n:6.2f}{versus}")
    return med


def plain(a):
    b = sfl.BatchSolver(DIM_X, DIM_Y, MEMBERS)
    b.setup_sketch_fields()
    b.queue_forces(list(range(MEMBERS)), [(10, 40)] * MEMBERS, [(-12.0, 30.0)] * MEMBERS)
    c = sfl.Solver(CTX, CTX)
    c.setup_sketch_fields()
    b.step_n(2, 0.05, 1.0, ITERS, 1.9)
    c.step_n(1, 0.05, 1.0, CTX_ITERS, 1.9)
    us = {"batch": [], "context": []}
    for r in range(a.warmup + a.reps):
        tb = timed(lambda: b.step_n(a.steps, 0.05, 1.0, ITERS, 1.9), b.synchronize)
        tc = timed(lambda: c.step_n(CTX_STEPS, 0.05, 1.0, CTX_ITERS, 1.9), c.synchronize)
        if r >= a.warmup:
            us["batch"].append(tb)
            us["context"].append(tc)
    say(f"nothing set, {a.warmup} warm-up and {a.reps} timed rounds, batch and context alternating:")
    report(f"batch {MEMBERS} x ({DIM_X} x {DIM_Y}), {ITERS} it", us["batch"], a.steps)
    report(f"context {CTX} x {CTX}, {CTX_ITERS} it", us["context"], CTX_STEPS)
    b.close()
    c.close()


def openings(a):
    n = a.steps
    j, i = np.mgrid[0:DIM_Y, 0:DIM_X]
    disc = (i - DIM_X // 4) ** 2 + (j - DIM_Y // 2) ** 2 <= 64
    tunnel = np.zeros((DIM_Y, DIM_X), np.uint8)
    tunnel[1:-1, 0], tunnel[1:-1, -1] = sfl.OPEN_INFLOW, sfl.OPEN_OUTFLOW
    kinds = {"(a) nothing set": (None, None), "(b) empty mask set": (np.zeros((DIM_Y, DIM_X), bool), None),
             "(c) west-in / east-out map": (None, tunnel), "(d) the map and a shared disc": (disc, tunnel)}
    batches = {}
    for name, (mask, open_map) in kinds.items():
        b = sfl.BatchSolver(DIM_X, DIM_Y, MEMBERS)
        b.setup_sketch_fields()
        if mask is not None:
            b.set_solids(mask)
        if open_map is not None:
            b.set_openings(open_map, (3.5, 0.0))
        b.queue_forces(list(range(MEMBERS)), [(10, 40)] * MEMBERS, [(-12.0, 30.0)] * MEMBERS)
        b.step_n(2, 0.05, 1.0, ITERS, 1.9)
        batches[name] = b
    say(f"batch of {MEMBERS} x ({DIM_X} x {DIM_Y}), step_n({n}) of {ITERS} iterations, {a.warmup} warm-up and {a.reps} timed rounds, the four "
        f"configurations alternating:")
    us = {name: [] for name in batches}
    for r in range(a.warmup + a.reps):
        for name, b in batches.items():
            t = timed(lambda: b.step_n(n, 0.05, 1.0, ITERS, 1.9), b.synchronize)
            if r >= a.warmup:
                us[name].append(t)
    base = statistics.median(us["(b) empty mask set"])
    med = {name: report(name, u, n, base) for name, u in us.items()}
    ub = us["(b) empty mask set"]
    spread = (max(ub) - min(ub)) / n
    say(f"  run-to-run spread of (b): max - min = {spread:.2f} us per step; (c) - (b) = {(med['(c) west-in / east-out map'] - base) / n:+.2f} us per step "
        f"= {(med['(c) west-in / east-out map'] - base) / n / spread if spread else float('nan'):+.2f} spreads")
    say()
    say(f"flow_stats(velocity) of all {MEMBERS} members, call + copy of the records, {a.reps} rounds alternating:")
    fs = {"empty mask (batch_solids.hip)": [], "the map (batch_openings.hip)": []}
    pair = (("empty mask (batch_solids.hip)", batches["(b) empty mask set"]), ("the map (batch_openings.hip)", batches["(c) west-in / east-out map"]))
    for r in range(a.warmup + a.reps):
        for name, b in pair:
            t = timed(lambda: b.flow_stats(1.0, dye=False), b.synchronize)
            if r >= a.warmup:
                fs[name].append(t)
    for name, u in fs.items():
        say(f"  {name:<32} median {statistics.median(u):8.1f} us   min {min(u):8.1f}   max {max(u):8.1f}")
    for b in batches.values():
        b.close()
    say()
    # the same comparison on a context: the unfused sequence of the masked step with an empty mask, and with the map
    jj, ii = np.mgrid[0:CTX, 0:CTX]
    big_disc = (ii - CTX // 4) ** 2 + (jj - CTX // 2) ** 2 <= (CTX // 8) ** 2
    big_tunnel = np.zeros((CTX, CTX), np.uint8)
    big_tunnel[1:-1, 0], big_tunnel[1:-1, -1] = sfl.OPEN_INFLOW, sfl.OPEN_OUTFLOW
    ckinds = {"(a) nothing set": (None, None), "(b) empty mask set": (np.zeros((CTX, CTX), bool), None),
              "(c) west-in / east-out map": (None, big_tunnel), "(d) the map and a disc": (big_disc, big_tunnel)}
    contexts = {}
    for name, (mask, open_map) in ckinds.items():
        c = sfl.Solver(CTX, CTX)
        c.setup_sketch_fields()
        if mask is not None:
            c.set_solids(mask)
        if open_map is not None:
            c.set_openings(open_map, (3.5, 0.0))
        c.step_n(1, 0.05, 1.0, CTX_ITERS, 1.9)
        contexts[name] = c
    say(f"context {CTX} x {CTX}, step_n({CTX_STEPS}) of {CTX_ITERS} iterations, {a.warmup} warm-up and {a.reps} timed rounds, the four configurations "
        f"alternating:")
    us = {name: [] for name in contexts}
    for r in range(a.warmup + a.reps):
        for name, c in contexts.items():
            t = timed(lambda: c.step_n(CTX_STEPS, 0.05, 1.0, CTX_ITERS, 1.9), c.synchronize)
            if r >= a.warmup:
                us[name].append(t)
    base = statistics.median(us["(b) empty mask set"])
    med = {name: report(name, u, CTX_STEPS, base) for name, u in us.items()}
    ub = us["(b) empty mask set"]
    spread = (max(ub) - min(ub)) / CTX_STEPS
    say(f"  run-to-run spread of (b): max - min = {spread:.2f} us per step; (c) - (b) = {(med['(c) west-in / east-out map'] - base) / CTX_STEPS:+.2f} us per step "
        f"= {(med['(c) west-in / east-out map'] - base) / CTX_STEPS / spread if spread else float('nan'):+.2f} spreads")
    for c in contexts.values():
        c.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["plain", "openings"], required=True)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--label", default="", help="a word for the header line: which library this run loads")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    say("# tools/openings_probe.py " + " ".join(sys.argv[1:]))
    say(f"# device: {sfl.device_info(0)[0]}; library: {a.label or 'this tree'}")
    (plain if a.mode == "plain" else openings)(a)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(OUT) + "\n")
