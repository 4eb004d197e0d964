#!/usr/bin/env python3
"""What a wall table costs a step, and that it costs nothing where none is set: the numbers of profiles/walls.txt.

Two modes, host clock around the call and the synchronise that ends it, warmed:

  --mode plain   a disc set and NO table: step_n(n) of a batch of 61 x 81 x 1024 members at 20 iterations, and step_n(4) of a
                 2048 x 2048 context with a disc of radius 256 at 40 iterations, each without viscosity and with four sweeps.
                 Uses no call that an older library lacks, so the same script runs against the parent commit's library (python
                 tools/with_lib.py <parent's libsfl_hip.so> tools/walls_probe.py --mode plain); run the two alternately in one
                 job and compare this library's median with the parent's median and its spread between processes.
  --mode walls   in one process, alternating: the same four configurations (a) without a table, (b) with a table of +0.0f on the
                 disc's cells -- the walls' kernels on the bits of (a): what the kernels and the launches themselves add -- and (c)
                 with one that spins the disc (rigid_wall_velocity, omega = 0.05); (c) - (a) is what a table adds per step.

usage: python3 tools/walls_probe.py --mode plain|walls [--reps R] [--steps N] [--out FILE]"""
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
CTX, CTX_ITERS, CTX_STEPS, CTX_RADIUS = 2048, 40, 4, 256
NU, SWEEPS = 0.05, 4


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
    versus = "" if base is None else f"   table - none {(med - base) / n:+8.2f} us per step ({100 * (med - base) / base:+6.2f} %)"
    say(f"  {name:<44} median {med / n:9.2f} us per step   min {min(u) / n:9.2f}   max {max(u) / n:9.2f}   MAD {mad / n:6.2f}{versus}")
    return med


def discs():
    j, i = np.mgrid[0:DIM_Y, 0:DIM_X]
    small = (i - DIM_X // 4) ** 2 + (j - DIM_Y // 2) ** 2 <= 64
    jj, ii = np.mgrid[0:CTX, 0:CTX]
    big = (ii - CTX // 4) ** 2 + (jj - CTX // 2) ** 2 <= CTX_RADIUS ** 2
    return small, (DIM_X // 4, DIM_Y // 2), big, (CTX // 4, CTX // 2)


def make(viscous, table):
    """(batch, context) with the discs set, with or without four sweeps; table: False, "zero" (+0.0f on the disc) or "spin"."""
    small, small_at, big, big_at = discs()
    b = sfl.BatchSolver(DIM_X, DIM_Y, MEMBERS)
    b.setup_sketch_fields()
    b.set_solids(small)
    c = sfl.Solver(CTX, CTX)
    c.setup_sketch_fields()
    c.set_solids(big)
    if viscous:
        b.set_viscosity(NU, SWEEPS)
        c.set_viscosity(NU, SWEEPS)
    if table:
        spin = 0.05 if table == "spin" else 0.0
        b.set_wall_velocity(*sfl.rigid_wall_velocity(small.astype(np.uint8), 1, omega=spin, pivot2=(2 * small_at[0], 2 * small_at[1])))
        c.set_wall_velocity(*sfl.rigid_wall_velocity(big.astype(np.uint8), 1, omega=spin, pivot2=(2 * big_at[0], 2 * big_at[1])))
    b.queue_forces(list(range(MEMBERS)), [(40, 40)] * MEMBERS, [(-12.0, 30.0)] * MEMBERS)
    b.step_n(2, 0.05, 1.0, ITERS, 1.9)
    c.step_n(1, 0.05, 1.0, CTX_ITERS, 1.9)
    return b, c


def run(a, table_kinds):
    sets = {(viscous, table): make(viscous, table) for viscous in (False, True) for table in table_kinds}
    us = {key: ([], []) for key in sets}
    for r in range(a.warmup + a.reps):
        for key, (b, c) in sets.items():
            tb = timed(lambda: b.step_n(a.steps, 0.05, 1.0, ITERS, 1.9), b.synchronize)
            tc = timed(lambda: c.step_n(CTX_STEPS, 0.05, 1.0, CTX_ITERS, 1.9), c.synchronize)
            if r >= a.warmup:
                us[key][0].append(tb)
                us[key][1].append(tc)
    say(f"{a.warmup} warm-up and {a.reps} timed rounds, every configuration alternating; batch {MEMBERS} x ({DIM_X} x {DIM_Y}) with a disc of radius 8, "
        f"{ITERS} it, step_n({a.steps}); context {CTX} x {CTX} with a disc of radius {CTX_RADIUS}, {CTX_ITERS} it, step_n({CTX_STEPS}):")
    for which, n, what in ((0, a.steps, "batch"), (1, CTX_STEPS, "context")):
        for viscous in (False, True):
            base = None
            for table in table_kinds:
                name = f"{what}, {'four sweeps' if viscous else 'no viscosity'}, {dict(zero='a table of zeros', spin='a spinning table').get(table, 'no table')}"
                med = report(name, us[(viscous, table)][which], n, base)
                base = med if base is None else base
    for b, c in sets.values():
        b.close()
        c.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["plain", "walls"], required=True)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--label", default="", help="a word for the header line: which library this run loads")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    say("# tools/walls_probe.py " + " ".join(sys.argv[1:]))
    say(f"# device: {sfl.device_info(0)[0]}; library: {a.label or 'this tree'}")
    run(a, (False,) if a.mode == "plain" else (False, "zero", "spin"))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(OUT) + "\n")
