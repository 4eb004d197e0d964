#!/usr/bin/env python3
"""What solid cells cost a whole-domain context: the timings of profiles/context_solids.txt.

In one process, warmed, three contexts of the same shape with the same fields, their calls alternating, host clock around
the call and the synchronise that ends it -- at 2048 x 2048 with 40 iterations and at 8192 x 8192 with 80:

  (a) no mask            the kernels a context without solids launches as ever (sor_fused.hip, the fused step kernels, the
                         step seams): the kernels of the parent commit, the yardstick
  (b) an empty mask set  the kernels of context_solids.hip with no solid cell: the same bits as (a), another route
  (c) a disc             radius dim / 8 in the middle of the grid

for poisson_solve alone and for step_n(n).  The run-to-run spread of (a) is what the probe itself sees: max - min and the
median absolute deviation over --reps.  After the timings the three contexts' fields are compared: (b) must hold (a)'s bits.
No ratio is expected in advance; the register-blocked plain solve is expected to stay the faster one.

usage: python3 tools/context_solids_probe.py [--reps R] [--steps N] [--sizes 2048:40,8192:80] [--out profiles/context_solids_timings.txt]"""
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
DT, DX, OMEGA = 0.05, 1.0, 1.9


def say(text=""):
    print(text)
    sys.stdout.flush()
    OUT.append(text)


def timed(call, sync):
    sync()
    t = time.perf_counter()
    call()
    sync()
    return (time.perf_counter() - t) * 1e3


def report(title, ms, unit, per):
    say(title)
    med = {name: statistics.median(u) for name, u in ms.items()}
    base = med["(a) no mask"]
    for name, u in ms.items():
        mad = statistics.median(abs(x - med[name]) for x in u)
        say(f"  {name:<22} median {med[name] / per:9.3f} ms per {unit}   min {min(u) / per:9.3f}   max {max(u) / per:9.3f}   MAD {mad / per:7.3f}   "
            f"vs (a) {med[name] / base:6.2f} x")
    ua = ms["(a) no mask"]
    say(f"  run-to-run spread of (a): max - min = {(max(ua) - min(ua)) / per:.3f} ms per {unit}")


def one_size(dim, iters, a):
    cap = sfl.capi
    j, i = np.ogrid[0:dim, 0:dim]
    disc = (i - dim // 2) ** 2 + (j - dim // 2) ** 2 <= (dim // 8) ** 2
    masks = {"(a) no mask": None, "(b) empty mask set": np.zeros((dim, dim), bool), f"(c) disc, r = {dim // 8}": disc}
    ctxs = {}
    for name, mask in masks.items():
        s = sfl.Solver(dim, dim)
        s.setup_sketch_fields()
        if mask is not None:
            s.set_solids(mask)
        s.queue_forces([(dim // 4, dim // 2)], [(-12.0, 30.0)])
        s.step_n(2, DT, DX, iters, OMEGA)
        ctxs[name] = s
    say(f"{dim} x {dim}, {iters} iterations, {a.warmup} warm-up and {a.reps} timed rounds, the three contexts alternating, host clock around "
        f"call + synchronize; solve launches: " + ", ".join(f"{n.split()[0]} {s.last_solve_info()['launches']}" for n, s in ctxs.items()))
    solve = {name: [] for name in ctxs}
    for r in range(a.warmup + a.reps):
        for name, s in ctxs.items():
            t = timed(lambda: s.poisson_solve(DX, iters, OMEGA), s.synchronize)
            if r >= a.warmup:
                solve[name].append(t)
    report(f"poisson_solve({iters}):", solve, "solve", 1)
    steps = {name: [] for name in ctxs}
    for r in range(a.warmup + a.reps):
        for name, s in ctxs.items():
            t = timed(lambda: s.step_n(a.steps, DT, DX, iters, OMEGA), s.synchronize)
            if r >= a.warmup:
                steps[name].append(t)
    report(f"step_n({a.steps}):", steps, "step", a.steps)
    names = list(ctxs)
    same = all(np.array_equal(ctxs[names[0]].download(f).view(np.uint32), ctxs[names[1]].download(f).view(np.uint32))
               for f in (cap.FIELD_VELOCITY, cap.FIELD_PRESSURE, cap.FIELD_COLOR))
    say(f"  after all of it (a) and (b) hold the same bits in velocity, pressure and dye: {same}")
    say()
    for s in ctxs.values():
        s.close()
    return same


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--sizes", default="2048:40,8192:80", help="dim:iters, comma-separated")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    say("# tools/context_solids_probe.py " + " ".join(sys.argv[1:]))
    say(f"# device: {sfl.device_info(0)[0]}")
    ok = True
    for size in a.sizes.split(","):
        dim, iters = (int(x) for x in size.split(":"))
        ok = one_size(dim, iters, a) and ok
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")
    sys.exit(0 if ok else 1)
