#!/usr/bin/env python3
"""What an inflow profile and the flux record cost, and that they cost nothing where neither is used: the numbers of
profiles/inflow.txt.

Two modes, host clock around the call and the synchronise that ends it, warmed:

  --mode plain    nothing set: step_n(n) of a batch of 61 x 81 x 1024 members at 20 iterations, and step_n(4) of a 2048 x 2048
                  context at 40 iterations.  Uses no call that an older library lacks: with --lib <the parent commit's
                  libsfl_hip.so> the same script measures the parent (the calls that library does not export are taken out of
                  the binding's table for this process).  Run the two alternately in one job and compare this library's median
                  with the parent's median and its run-to-run spread (max - min and MAD over --reps).
  --mode inflow   in one process, alternating: (a) a west-in / east-out map with the uniform inflow -- batch_open_step_kernel;
                  (b) the same with a parabolic profile over the full height of the west column --
                  batch_open_profile_step_kernel.  Then the same pair on a 2048 x 2048 context.  Then openings_flux beside
                  flow_stats(velocity) on the same batch and the same context, call + copy of the records.

usage: python3 tools/inflow_probe.py --mode plain|inflow [--lib PATH] [--reps R] [--steps N] [--out FILE]"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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


def report(name, u, n, base=None, unit="us per step"):
    med = statistics.median(u)
    mad = statistics.median(abs(x - med) for x in u)
    versus = "" if base is None else f"   vs (a) {100 * (med - base) / base:+6.2f} %"
    say(f"  {name:<40} median {med / n:9.2f} {unit}   min {min(u) / n:9.2f}   max {max(u) / n:9.2f}   MAD {mad / n:6.2f}{versus}")
    return med


def plain(sfl, a):
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


def parabola(dim_y, peak):
    cells = [(0, j) for j in range(1, dim_y - 1)]
    s = (np.arange(1, dim_y - 1) - 0.5) / (dim_y - 2)
    vel = np.stack([peak * 4 * s * (1 - s), np.zeros_like(s)], axis=1).astype(np.float32)
    return cells, vel


def tunnel(dim_x, dim_y, sfl):
    m = np.zeros((dim_y, dim_x), np.uint8)
    m[1:-1, 0], m[1:-1, -1] = sfl.OPEN_INFLOW, sfl.OPEN_OUTFLOW
    return m


def pair(a, things, n, call, title):
    say(title)
    us = {name: [] for name in things}
    for r in range(a.warmup + a.reps):
        for name, x in things.items():
            t = timed(lambda: call(x), x.synchronize)
            if r >= a.warmup:
                us[name].append(t)
    names = list(things)
    base = statistics.median(us[names[0]])
    med = {name: report(name, u, n, None if name == names[0] else base) for name, u in us.items()}
    ua = us[names[0]]
    spread = (max(ua) - min(ua)) / n
    say(f"  run-to-run spread of (a): max - min = {spread:.2f} us per step; (b) - (a) = {(med[names[1]] - base) / n:+.2f} us per step")


def inflow(sfl, a):
    batches = {}
    for name, profiled in (("(a) the map, uniform inflow", False), ("(b) the map, a full-height profile", True)):
        b = sfl.BatchSolver(DIM_X, DIM_Y, MEMBERS)
        b.setup_sketch_fields()
        b.set_openings(tunnel(DIM_X, DIM_Y, sfl), (3.5, 0.0))
        if profiled:
            b.set_inflow_profile(*parabola(DIM_Y, 5.25))
        b.queue_forces(list(range(MEMBERS)), [(10, 40)] * MEMBERS, [(-12.0, 30.0)] * MEMBERS)
        b.step_n(2, 0.05, 1.0, ITERS, 1.9)
        batches[name] = b
    pair(a, batches, a.steps, lambda b: b.step_n(a.steps, 0.05, 1.0, ITERS, 1.9),
         f"batch of {MEMBERS} x ({DIM_X} x {DIM_Y}), step_n({a.steps}) of {ITERS} iterations, {a.warmup} warm-up and {a.reps} timed rounds, alternating:")
    say()
    b = batches["(b) the map, a full-height profile"]
    say(f"the diagnostics of all {MEMBERS} members, call + copy of the records, {a.reps} rounds alternating:")
    us = {"flow_stats(velocity)": [], "openings_flux": []}
    for r in range(a.warmup + a.reps):
        for name, call in (("flow_stats(velocity)", lambda: b.flow_stats(1.0, dye=False)), ("openings_flux", b.openings_flux)):
            t = timed(call, b.synchronize)
            if r >= a.warmup:
                us[name].append(t)
    for name, u in us.items():
        report(name, u, 1, unit="us per call")
    for x in batches.values():
        x.close()
    say()
    contexts = {}
    for name, profiled in (("(a) the map, uniform inflow", False), ("(b) the map, a full-height profile", True)):
        c = sfl.Solver(CTX, CTX)
        c.setup_sketch_fields()
        c.set_openings(tunnel(CTX, CTX, sfl), (3.5, 0.0))
        if profiled:
            c.set_inflow_profile(*parabola(CTX, 5.25))
        c.step_n(1, 0.05, 1.0, CTX_ITERS, 1.9)
        contexts[name] = c
    pair(a, contexts, CTX_STEPS, lambda c: c.step_n(CTX_STEPS, 0.05, 1.0, CTX_ITERS, 1.9),
         f"context {CTX} x {CTX}, step_n({CTX_STEPS}) of {CTX_ITERS} iterations, {a.warmup} warm-up and {a.reps} timed rounds, alternating:")
    say()
    c = contexts["(b) the map, a full-height profile"]
    say(f"the diagnostics of the context, call + copy of the record, {a.reps} rounds alternating:")
    us = {"flow_stats(velocity)": [], "openings_flux": []}
    for r in range(a.warmup + a.reps):
        for name, call in (("flow_stats(velocity)", lambda: c.flow_stats(1.0, dye=False)), ("openings_flux", c.openings_flux)):
            t = timed(call, c.synchronize)
            if r >= a.warmup:
                us[name].append(t)
    for name, u in us.items():
        report(name, u, 1, unit="us per call")
    for x in contexts.values():
        x.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["plain", "inflow"], required=True)
    ap.add_argument("--lib", default=None, help="another build of the library, e.g. the parent commit's")
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if a.lib:   # before anything loads the product library
        capi = importlib.import_module("esp32-fluid-simulation_amd._capi")
        capi.LIB_PATH = os.path.abspath(a.lib)
        older = ctypes.CDLL(capi.LIB_PATH)
        for name in [n for n in capi.SIGNATURES if not hasattr(older, n)]:
            del capi.SIGNATURES[name]
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    say("# tools/inflow_probe.py " + " ".join(sys.argv[1:]))
    say(f"# device: {sfl.device_info(0)[0]}; library: {a.lib or 'this tree'}")
    (plain if a.mode == "plain" else inflow)(sfl, a)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(OUT) + "\n")
