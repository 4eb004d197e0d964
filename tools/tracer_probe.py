#!/usr/bin/env python3
"""What following tracers cost a step call: the numbers of profiles/tracers.txt.

In one process, warmed, the three variants of the same step_n(n) alternating, host clock around the call and the
synchronise that ends it:

  no set          what the call launched before there were tracers (a context: with its fused step boundaries; a batch:
                  one launch per step) -- the comparison
  following set   one advance launch behind every step (a context: no fused step boundaries, so the difference holds the
                  lost seam as well as the advance)
  ... and a trail the same with a slot written after every 4th advance; the trail is restarted (no allocation: it does
                  not grow) before every timed call

  batch           61 x 81 x 1024 members, K = 256 tracers each, step_n_each of 20 iterations
  context         2048 x 2048, 10^6 tracers

Also timed alone between device synchronises: one manual advance and one sample of the velocity.  Median, minimum and
maximum over --reps.  The figures per step are the call's over n.  Bytes of an advance: 16 per tracer for its position
(read and written) plus four texels of 8; what reaches memory of the texels depends on the caches.

usage: python3 tools/tracer_probe.py [--reps R] [--steps N] [--out profiles/tracers.txt]"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfl = importlib.import_module("esp32-fluid-simulation_amd")

FV = sfl.capi.FIELD_VELOCITY
OUT = []


def say(text=""):
    print(text)
    sys.stdout.flush()
    OUT.append(text)


def line(name, us, per=1):
    med = statistics.median(us)
    return f"  {name:<40} median {med:10.1f} us   min {min(us):10.1f}   max {max(us):10.1f}   per step {med / per:9.1f} us"


def timed(call, sync):
    sync()
    t = time.perf_counter()
    call()
    sync()
    return (time.perf_counter() - t) * 1e6


def rounds(variants, a, per):
    """variants: name -> (prepare, call); prepare runs untimed in front of every call."""
    us = {n: [] for n in variants}
    for r in range(a.warmup + a.reps):
        for n, (prepare, call, sync) in variants.items():   # alternating: every round runs each variant once
            prepare()
            t = timed(call, sync)
            if r >= a.warmup:
                us[n].append(t)
    for n in variants:
        say(line(n, us[n], per))
    return {n: statistics.median(u) for n, u in us.items()}


def report(med, n):
    base = med["step_n, no set"]
    for name in ("step_n, following set", "step_n, following set and a trail"):
        say(f"  {name} - no set: {(med[name] - base) / n:+8.1f} us per step ({100 * (med[name] - base) / base:+.1f} %)")


def starts(rng, lead, count, dim_x, dim_y):
    xy = np.empty(lead + (count, 2), np.float32)
    xy[..., 0] = rng.uniform(-1.0, dim_x, lead + (count,))
    xy[..., 1] = rng.uniform(-1.0, dim_y, lead + (count,))
    return xy


def batch(a):
    dim_x, dim_y, members, k, n = 61, 81, 1024, 256, a.steps
    rng = np.random.default_rng(1)
    xy = starts(rng, (members,), k, dim_x, dim_y)
    iters = [20] * members
    with sfl.BatchSolver(dim_x, dim_y, members) as plain, sfl.BatchSolver(dim_x, dim_y, members) as follow, \
            sfl.BatchSolver(dim_x, dim_y, members) as trail:
        for b in (plain, follow, trail):
            b.setup_sketch_fields()
            b.queue_forces(list(range(members)), [(20, 40)] * members, [(-12.0, 30.0)] * members)
            b.step_n_each(2, 0.05, 1.0, iters, 1.9)
        follow.set_tracers(xy, follow=True)
        trail.set_tracers(xy, follow=True)
        trail.trail_start(4, n // 4 + 1)
        step = lambda b: (lambda: b.step_n_each(n, 0.05, 1.0, iters, 1.9))
        variants = {"step_n, no set": (lambda: None, step(plain), plain.synchronize),
                    "step_n, following set": (lambda: None, step(follow), follow.synchronize),
                    "step_n, following set and a trail": (lambda: trail.trail_start(4, n // 4 + 1), step(trail), trail.synchronize),
                    "one advance": (lambda: None, lambda: follow.advance_tracers(0.05), follow.synchronize),
                    "one sample of the velocity": (lambda: None, lambda: follow.sample_tracers(FV, True), follow.synchronize),
                    "synchronize alone": (lambda: None, lambda: None, plain.synchronize)}
        say(f"batch of {members} x ({dim_x} x {dim_y}), K = {k} tracers per member ({members * k} in all), step_n_each({n}) of 20 iterations, "
            f"{a.reps} rounds, host clock around call + synchronize:")
        report(rounds(variants, a, n), n)
        say(f"  (an advance moves {members * k * 16 / 1e6:.1f} MB of positions and gathers {members * k * 32 / 1e6:.1f} MB of texels from "
            f"{members * dim_x * dim_y * 8 / 1e6:.1f} MB of velocity)")


def context(a):
    size, count, n = 2048, 1000000, a.steps
    rng = np.random.default_rng(2)
    xy = starts(rng, (), count, size, size)
    v = (rng.standard_normal((size, size, 2), dtype=np.float32) * 5).astype(np.float32)
    with sfl.Solver(size, size) as plain, sfl.Solver(size, size) as follow, sfl.Solver(size, size) as trail:
        for s in (plain, follow, trail):
            s.upload(FV, v)
            s.step_n(2, 0.02, 1.0, 20, 1.9)
        follow.set_tracers(xy, follow=True)
        trail.set_tracers(xy, follow=True)
        trail.trail_start(4, n // 4 + 1)
        step = lambda s: (lambda: s.step_n(n, 0.02, 1.0, 20, 1.9))
        variants = {"step_n, no set": (lambda: None, step(plain), plain.synchronize),
                    "step_n, following set": (lambda: None, step(follow), follow.synchronize),
                    "step_n, following set and a trail": (lambda: trail.trail_start(4, n // 4 + 1), step(trail), trail.synchronize),
                    "one advance": (lambda: None, lambda: follow.advance_tracers(0.02), follow.synchronize),
                    "one sample of the velocity": (lambda: None, lambda: follow.sample_tracers(FV, True), follow.synchronize),
                    "synchronize alone": (lambda: None, lambda: None, plain.synchronize)}
        say(f"context {size} x {size}, {count} tracers, step_n({n}) of 20 iterations, {a.reps} rounds, host clock around call + synchronize:")
        report(rounds(variants, a, n), n)
        say(f"  (an advance moves {count * 16 / 1e6:.1f} MB of positions and gathers {count * 32 / 1e6:.1f} MB of texels from "
            f"{size * size * 8 / 1e6:.1f} MB of velocity; the sample includes its copy of {count * 8 / 1e6:.1f} MB to the host)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    say("# tools/tracer_probe.py " + " ".join(sys.argv[1:]))
    say(f"# device: {sfl.device_info(0)[0]}")
    batch(a)
    say()
    context(a)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")
