#!/usr/bin/env python3
"""What loads cost: the numbers of profiles/loads.txt.

Two workloads, each in one process, warmed, its configurations alternating, host clock around the call and the synchronise
that ends it:

  batch    61 x 81 x 1024 members at 20 iterations, one shared disc of radius 8 in every member
  context  2048 x 2048 at 40 iterations, a disc of radius 256

and for each

  (a) step, no recorder       step_n(n) as it ran before there were loads: the new code in this path is one null-pointer test
  (b) step, a sample a step   the same call with the loads recorder on, every = 1
  (c) loads() alone           the sampler n times through the synchronous call, its copy and wait included; on the stream it
                              costs (b) - (a)
  (d) step; loads             the loop of synchronous calls the recorder replaces, n times

With --parent PATH (the library of the parent commit, built from a scratch worktree) (a) is also run on that library, the two
alternating in the same rounds through the same raw ctypes calls, on --objects batches (contexts) of each made in turn: where
an object's fields lie moves a step by more than the rounds of one object differ.  The agreement is judged inside the spread
the probe itself reports for (a) on this library: max - min over the rounds and the objects.  Then (b) is run on both
libraries too (samples_against_parent): what a sample costs on this one against what it costs on the parent's.  The synchronous
configurations (c) and (d) are measured on this library alone.

usage: python3 tools/loads_probe.py [--parent libsfl_parent.so] [--objects K] [--reps R] [--steps N] [--out profiles/loads.txt]"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfl = importlib.import_module("esp32-fluid-simulation_amd")
capi = sfl.capi

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
    return (time.perf_counter() - t) * 1e6


def disc(dim_x, dim_y, r):
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    return ((i - dim_x // 2) ** 2 + (j - dim_y // 2) ** 2 <= r * r).astype(np.uint8)


class Raw:
    """The few calls of the C ABI the comparison with the parent's library needs, on either library, through the same code."""

    def __init__(self, path, batch, dim_x, dim_y, members, mask, velocity=None, pivot=None):
        self.lib = C.CDLL(path)
        for name, (res, args) in capi.SIGNATURES.items():
            if hasattr(self.lib, name):
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = res, args
        self.batch, self.members, self.h = batch, members, C.c_void_p()
        ptr = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        if batch:
            self.ok(self.lib.sfl_batch_create(C.byref(self.h), 0, dim_x, dim_y, members))
            self.ok(self.lib.sfl_batch_setup_sketch_fields(self.h))
        else:
            self.ok(self.lib.sfl_create(C.byref(self.h), 0, dim_x, dim_y))
            self.ok(self.lib.sfl_setup_sketch_fields(self.h))
        if velocity is not None:   # (x, y) in every cell instead of the sketch's fluid at rest
            v = np.empty((members if batch else 1, dim_y, dim_x, 2), np.float32)
            v[...] = velocity
            head = (self.h, capi.FIELD_VELOCITY) + ((0, members) if batch else ())
            self.ok((self.lib.sfl_batch_upload if batch else self.lib.sfl_upload)(*head, v.ctypes.data, v.nbytes))
        self.ok(self.lib.sfl_batch_set_solids(self.h, ptr, 0) if batch else self.lib.sfl_set_solids(self.h, ptr))
        if pivot is not None:   # of the one body, in cells
            p2 = (C.c_int32 * 2)(2 * pivot[0], 2 * pivot[1])
            self.ok(self.lib.sfl_batch_set_body_pivots(self.h, p2, 0, 1) if batch else self.lib.sfl_set_body_pivots(self.h, p2, 1))

    def ok(self, rc):
        if rc != capi.OK:
            raise SystemExit(f"{self.lib._name}: {self.lib.sfl_last_error().decode()}")

    def step_n(self, n, iters):
        self.ok((self.lib.sfl_batch_step_n if self.batch else self.lib.sfl_step_n)(self.h, n, DT, DX, iters, OMEGA))

    def synchronize(self):
        self.ok((self.lib.sfl_batch_synchronize if self.batch else self.lib.sfl_synchronize)(self.h))

    def start(self, kind, capacity):
        """The recorder of `kind` ("loads", "friction", "torque"), every = 1, all members."""
        if self.batch:
            self.ok(getattr(self.lib, f"sfl_batch_{kind}_start")(self.h, 1, 0, self.members, capacity))
        else:
            self.ok(getattr(self.lib, f"sfl_{kind}_start")(self.h, 1, capacity))

    def stop(self, kind):
        self.ok(getattr(self.lib, f"sfl_batch_{kind}_stop" if self.batch else f"sfl_{kind}_stop")(self.h))

    def close(self):
        (self.lib.sfl_batch_destroy if self.batch else self.lib.sfl_destroy)(self.h)


def samples_against_parent(a, say, batch, dim_x, dim_y, members, iters, mask, configs, **fields):
    """With --parent: what a sample costs on this library and on the parent's (also for friction_probe.py and torque_probe.py).
    configs: {label: the recorders that are on}.  --objects batches (contexts) of each library, made in turn, all in the same
    rounds, either end first in turn, as (a) runs.  In a round EVERY object runs step_n(n) without a recorder and then once per
    configuration, the recorders started in front of the timed call and stopped behind it: the cost of a sample is (the
    configuration's step) - (the step without a recorder) of the SAME object in the same round -- where an object's fields lie
    moves its step by more than a sample's cost differs between the libraries, and an object of its own per configuration
    measures that.  The condition: this library's median cost is no more than the parent's median plus the parent's own
    max - min over its rounds and objects."""
    n = a.steps
    libs = {"this": capi.LIB_PATH, "parent": os.path.abspath(a.parent)}
    raws = [(name, Raw(path, batch, dim_x, dim_y, members, mask, **fields)) for _ in range(a.objects) for name, path in libs.items()]
    for _, r in raws:
        r.step_n(2, iters)
    step = {(name, label): [] for name in libs for label in configs}
    cost = {(name, label): [] for name in libs for label in configs}
    for rnd in range(a.warmup + a.reps):
        for name, r in (raws if rnd % 2 == 0 else raws[::-1]):
            t0 = timed(lambda: r.step_n(n, iters), r.synchronize)
            for label, kinds in configs.items():
                for kind in kinds:
                    r.start(kind, n)
                t = timed(lambda: r.step_n(n, iters), r.synchronize)
                for kind in kinds:
                    r.stop(kind)
                if rnd >= a.warmup:
                    step[(name, label)].append(t / n)
                    cost[(name, label)].append((t - t0) / n)
    say(f"  with recorders, {a.objects} objects of this library and of the parent's in the same rounds, us per step:")
    for label in configs:
        med = {name: statistics.median(cost[(name, label)]) for name in libs}
        for name in libs:
            c = cost[(name, label)]
            say(f"    {label:<30} {name:<7} step median {statistics.median(step[(name, label)]):9.2f}   a sample, step - (no recorder): "
                f"median {med[name]:+7.2f}   min {min(c):+7.2f}   max {max(c):+7.2f}")
        spread = max(cost[("parent", label)]) - min(cost[("parent", label)])
        verdict = "no more than" if med["this"] <= med["parent"] + spread else "MORE THAN"
        say(f"    {label:<30} this - parent = {med['this'] - med['parent']:+.2f}: {verdict} the parent's median plus its max - min of {spread:.2f}")
    for _, r in raws:
        r.close()


def report(us, n, base):
    med = {name: statistics.median(u) for name, u in us.items()}
    for name, u in us.items():
        mad = statistics.median(abs(x - med[name]) for x in u)
        say(f"  {name:<30} median {med[name] / n:9.2f} us per step   min {min(u) / n:9.2f}   max {max(u) / n:9.2f}   MAD {mad / n:7.2f}   "
            f"vs {base} {100 * (med[name] - med[base]) / med[base]:+6.2f} %")
    return med


def workload(a, batch, dim_x, dim_y, members, iters, radius):
    n = a.steps
    mask = disc(dim_x, dim_y, radius)
    what = f"batch of {members} x ({dim_x} x {dim_y})" if batch else f"context of {dim_x} x {dim_y}"
    say(f"{what}, a disc of radius {radius}, step_n({n}) of {iters} iterations, {a.warmup} warm-up and {a.reps} timed rounds, the configurations "
        f"alternating, host clock around call + synchronize:")
    # ---- the parent's library against this one, no recorder: --objects batches (contexts) of each, made in turn.  One object
    # is not enough: where its fields lie decides a few per cent of a step (two objects of ONE library differ by more than
    # the rounds of one object do), so the spread that judges the gap is the one over the objects as well
    libs = {"this": capi.LIB_PATH}
    if a.parent:
        libs["parent"] = os.path.abspath(a.parent)
    raws = [(name, k, Raw(path, batch, dim_x, dim_y, members, mask)) for k in range(a.objects) for name, path in libs.items()]
    for _, _, r in raws:
        r.step_n(2, iters)
    us = {(name, k): [] for name, k, _ in raws}
    for rnd in range(a.warmup + a.reps):
        for name, k, r in (raws if rnd % 2 == 0 else raws[::-1]):   # (either end first in turn)
            t = timed(lambda: r.step_n(n, iters), r.synchronize)
            if rnd >= a.warmup:
                us[(name, k)].append(t / n)
    per_lib = {}
    for name in libs:
        meds = [statistics.median(us[(name, k)]) for k in range(a.objects)]
        every = [t for k in range(a.objects) for t in us[(name, k)]]
        per_lib[name] = (statistics.median(every), min(every), max(every), meds)
        say(f"  (a) {name:<7} no recorder, {a.objects} objects: median {per_lib[name][0]:9.2f} us per step   min {min(every):9.2f}   max {max(every):9.2f}   "
            f"medians of the objects {', '.join(f'{m:.2f}' for m in meds)}")
    med, lo, hi, meds = per_lib["this"]
    within = max(max(us[("this", k)]) - min(us[("this", k)]) for k in range(a.objects))
    say(f"  spread of (a) this: over the rounds of one object at most {within:.2f} us per step, over the objects' medians {max(meds) - min(meds):.2f}, "
        f"over everything max - min = {hi - lo:.2f}")
    if a.parent:
        gap = med - per_lib["parent"][0]
        say(f"  this - parent = {gap:+.2f} us per step ({100 * gap / per_lib['parent'][0]:+.2f} %) = {gap / (hi - lo) if hi > lo else float('nan'):+.2f} of that max - min")
    else:
        say("  the parent's library: not measured (no --parent)")
    for _, _, r in raws:
        r.close()
    if a.parent:
        samples_against_parent(a, say, batch, dim_x, dim_y, members, iters, mask, {"(b) step, a sample a step": ("loads",)})
    # ---- the recorder, the sampler alone, the synchronous loop
    def make():
        s = sfl.BatchSolver(dim_x, dim_y, members) if batch else sfl.Solver(dim_x, dim_y)
        s.setup_sketch_fields()
        s.set_solids(mask)
        s.step_n(2, DT, DX, iters, OMEGA)
        return s

    plain, rec, loop = make(), make(), make()
    # (c): a sample with no step in front of it cannot be had from the recorder, so (c) times loads() itself, its copy and
    # synchronize included; what a sample costs on the stream is (b) - (a)
    def recorded():
        rec.loads_start(1, n)
        rec.step_n(n, DT, DX, iters, OMEGA)

    def looped():
        for _ in range(n):
            loop.step_n(1, DT, DX, iters, OMEGA)
            loop.loads()

    def sampled():
        for _ in range(n):
            plain.loads()

    runs = {"(a) step, no recorder": (lambda: plain.step_n(n, DT, DX, iters, OMEGA), plain.synchronize),
            "(b) step, a sample a step": (recorded, rec.synchronize),
            "(c) loads() alone, synchronous": (sampled, plain.synchronize),
            "(d) the loop step; loads()": (looped, loop.synchronize)}
    us = {name: [] for name in runs}
    for k in range(a.warmup + a.reps):
        for name, (call, sync) in runs.items():
            t = timed(call, sync)
            if k >= a.warmup:
                us[name].append(t)
    med = report(us, n, "(a) step, no recorder")
    say(f"  a sample behind every step costs (b) - (a) = {(med['(b) step, a sample a step'] - med['(a) step, no recorder']) / n:+.2f} us per step; "
        f"the loop it replaces (d) - (a) = {(med['(d) the loop step; loads()'] - med['(a) step, no recorder']) / n:+.2f} us per step")
    recs = rec.loads_history()
    say(f"  (the last sample: faces {recs[-1, 0, 0]['faces'].tolist()}, fx, fy = {rec.loads_history_xy()[-1, 0, 0].tolist()})")
    for s in (plain, rec, loop):
        s.close()
    say()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libsfl_hip.so of the parent commit: (a) is run on it too")
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--objects", type=int, default=4, help="batches (contexts) per library in the comparison with the parent")
    ap.add_argument("--only", choices=["batch", "context"], default=None)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    say("# tools/loads_probe.py " + " ".join(sys.argv[1:]))
    say(f"# device: {sfl.device_info(0)[0]}")
    if a.only != "context":
        workload(a, True, 61, 81, 1024, 20, 8)
    if a.only != "batch":
        workload(a, False, 2048, 2048, 1, 40, 256)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")
